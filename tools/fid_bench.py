#!/usr/bin/env python
"""Inception V3 (the FID feature net, omnitokenizer_amd/inception.py on csrc/inception.hip): the whole get_activations path
from uint8 256 x 256 images (the tokenizer's resolution) through the 299 x 299 resize to 2048-d features, ms per call,
TFLOP/s and the fraction of the fp32-MFMA rate measured in the same process (tools/mfma_peak.py's probe, as in
tools/fvd_bench.py), a per-layer breakdown, and the same network through torch fp32 F.conv2d / F.max_pool2d / F.avg_pool2d
on the same GPU and the same folded weights (BN folded into the conv, which only makes the torch path cheaper than the
reference's conv + BN).

    python tools/fid_bench.py [--batches 50 64] [--size 256] [--iters 5] [--json out.json]

FLOPs are counted from the shapes: 2 * Ho * Wo * Cout * Cin * kh * kw per conv (Conv2d_1a with its 3 real channels).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from omnitokenizer_amd import fid, inception, synth  # noqa: E402
from tools.fvd_bench import mfma_peak_tflops, timed  # noqa: E402


def layer_flops(R=299):
    """[(layer, flops per image)] of the NET steps at an R x R network input; every conv of a module reads an extent equal
    to the module's input extent (only the stride-2 convs of B and D shrink it, as their outputs)"""
    out, h, w = [], R, R
    for blk, name, kind, convs in inception.NET:
        f = 0.0
        for cname, cin, cout, k, s, p in convs:
            f += 2.0 * inception.out_size(h, k[0], s[0], p[0]) * inception.out_size(w, k[1], s[1], p[1]) * cout * cin * \
                k[0] * k[1]
        out.append((name, f))
        if kind == "conv":
            _, _, _, k, s, p = convs[0]
            h, w = inception.out_size(h, k[0], s[0], p[0]), inception.out_size(w, k[1], s[1], p[1])
        elif kind in ("pool", "B", "D"):
            h, w = inception.out_size(h, 3, 2, 0), inception.out_size(w, 3, 2, 0)
    return out


class TorchInception:
    """the network in torch fp32, NCHW, on the folded weights, with the FID patches' pools"""

    def __init__(self, model: inception.InceptionV3, device):
        sd = model._sd
        self.w = {p: tuple(t.float().to(device) for t in inception.fold_bn(sd, p))
                  for p, _ in inception._convs_with_keys(True, 3)}
        self.names = {}
        index = {0: 0, 1: 0, 2: 0, 3: 0}
        for blk, name, kind, convs in inception.NET:
            self.names[name] = f"blocks.{blk}.{index[blk]}"
            index[blk] += 1

    def conv(self, x, key, cv):
        w, b = self.w[key]
        return F.relu(F.conv2d(x, w, b, stride=cv[4], padding=cv[5]))

    def step(self, x, item):
        blk, name, kind, convs = item
        base = self.names[name]
        if kind == "conv":
            return self.conv(x, base, convs[0])
        if kind == "pool":
            return F.max_pool2d(x, 3, 2)
        c = {cv[0]: cv for cv in convs}
        run = lambda t, n: self.conv(t, f"{base}.{n}", c[n])  # noqa: E731
        if kind == "A":
            return torch.cat([run(x, "branch1x1"), run(run(x, "branch5x5_1"), "branch5x5_2"),
                              run(run(run(x, "branch3x3dbl_1"), "branch3x3dbl_2"), "branch3x3dbl_3"),
                              run(F.avg_pool2d(x, 3, 1, 1, count_include_pad=False), "branch_pool")], 1)
        if kind == "B":
            return torch.cat([run(x, "branch3x3"), run(run(run(x, "branch3x3dbl_1"), "branch3x3dbl_2"), "branch3x3dbl_3"),
                              F.max_pool2d(x, 3, 2)], 1)
        if kind == "C":
            a = run(run(run(x, "branch7x7_1"), "branch7x7_2"), "branch7x7_3")
            d = x
            for n in ("branch7x7dbl_1", "branch7x7dbl_2", "branch7x7dbl_3", "branch7x7dbl_4", "branch7x7dbl_5"):
                d = run(d, n)
            return torch.cat([run(x, "branch1x1"), a, d,
                              run(F.avg_pool2d(x, 3, 1, 1, count_include_pad=False), "branch_pool")], 1)
        if kind == "D":
            return torch.cat([run(run(x, "branch3x3_1"), "branch3x3_2"),
                              run(run(run(run(x, "branch7x7x3_1"), "branch7x7x3_2"), "branch7x7x3_3"), "branch7x7x3_4"),
                              F.max_pool2d(x, 3, 2)], 1)
        t = run(x, "branch3x3_1")
        d = run(run(x, "branch3x3dbl_1"), "branch3x3dbl_2")
        pool = F.avg_pool2d(x, 3, 1, 1, count_include_pad=False) if kind == "E1" else F.max_pool2d(x, 3, 1, 1)
        return torch.cat([run(x, "branch1x1"), run(t, "branch3x3_2a"), run(t, "branch3x3_2b"), run(d, "branch3x3dbl_3a"),
                          run(d, "branch3x3dbl_3b"), run(pool, "branch_pool")], 1)

    def features(self, u8):
        """uint8 [N, H, W, 3] on the GPU -> [N, 2048]: ToTensor, the resize, 2 x - 1, the network, the average pool"""
        x = u8.permute(0, 3, 1, 2).float().div(255)
        x = 2 * F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False) - 1
        for item in inception.NET:
            x = self.step(x, item)
        return x.mean(dim=(2, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[50, 64])
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "fid_bench needs the GPU"
    torch.backends.cudnn.benchmark = False
    peak = mfma_peak_tflops()
    print(f"measured fp32-MFMA rate: {peak:.1f} TF/s")
    model = inception.InceptionV3([3])
    model.load_state_dict(synth.synth_fid_inception_state_dict(0))
    model = model.cuda().eval()
    ref = TorchInception(model, "cuda")
    flops = layer_flops()
    total = sum(f for _, f in flops)
    results = []
    for B in a.batches:
        u8 = torch.from_numpy(synth.synth_fid_images(B, a.size, a.size, seed=B)).cuda()
        with torch.no_grad():
            ours_fn = lambda: fid.get_activations(u8, model, batch_size=B, device="cuda")  # noqa: E731
            ms = timed(ours_fn, a.iters)
            ms_t = timed(lambda: ref.features(u8).cpu(), a.iters)
            got = torch.from_numpy(ours_fn())
            want = ref.features(u8).double().cpu()
            diff = (got - want).abs().max().item()
            # the bar of tests/test_gpu_fid.py's feature tests, against the torch fp32 run (both sides round: twice it)
            bar = 2 * (50 ** 0.5) * (4032 ** 0.5) * 2 ** -24 * 4 * want.abs().max().item()
            x = inception.preprocess_images(u8)
            pk = model._weights(x.device)
            rows, rows_t, h, ht = [], [], x, x[..., :3].permute(0, 3, 1, 2).contiguous()
            for item in inception.NET:
                blk, name, kind, convs = item
                if kind == "conv":
                    _, _, _, k, s, p = convs[0]
                    fn = lambda h=h, name=name, k=k, s=s, p=p: inception.conv2d(h, *pk[name], k, s, p)  # noqa: E731
                elif kind == "pool":
                    fn = lambda h=h: inception.maxpool2d(h, 3, 2, 0)  # noqa: E731
                else:
                    fn = lambda h=h, item=item: model._module(h, item[1], item[2], item[3], pk)  # noqa: E731
                fn_t = lambda ht=ht, item=item: ref.step(ht, item)  # noqa: E731
                rows.append((name, timed(fn, a.iters)))
                rows_t.append((name, timed(fn_t, a.iters)))
                h, ht = fn(), fn_t()
            net_ms = timed(lambda: model.forward_channels_last(x), a.iters)
        tf, tf_t, tf_net = B * total / ms / 1e9, B * total / ms_t / 1e9, B * total / net_ms / 1e9
        r = {"B": B, "size": a.size, "gflop_per_image": total / 1e9, "ms": ms, "tflops": tf, "frac_of_mfma_rate": tf / peak,
             "network_ms": net_ms, "network_frac_of_mfma_rate": tf_net / peak, "torch_ms": ms_t, "torch_tflops": tf_t,
             "speedup_vs_torch": ms_t / ms, "max_feature_diff_vs_torch": diff, "bar": bar, "within_bar": diff <= bar,
             "layers": []}
        print(f"\nB {B:3d} from {a.size}x{a.size} uint8: {ms:8.2f} ms  {tf:6.1f} TF/s  {tf / peak:.2f} of the measured rate "
              f"(network alone {net_ms:.2f} ms, {tf_net / peak:.2f}) | torch fp32 {ms_t:8.2f} ms  {tf_t:6.1f} TF/s | "
              f"{ms_t / ms:.2f}x | max |feature diff| {diff:.2e} (bar {bar:.2e}: {'ok' if diff <= bar else 'EXCEEDED'})")
        print(f"  per layer:  {'layer':16s} {'ms':>8s} {'TF/s':>7s} {'frac':>5s} {'torch ms':>9s}")
        for (name, f), (_, lms), (_, tms) in zip(flops, rows, rows_t):
            ltf = B * f / lms / 1e9 if f else 0.0
            r["layers"].append({"layer": name, "ms": lms, "tflops": ltf, "torch_ms": tms})
            print(f"              {name:16s} {lms:8.3f} {ltf:7.1f} {ltf / peak:5.2f} {tms:9.3f}")
        results.append(r)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"mfma_peak_tflops": peak, "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
