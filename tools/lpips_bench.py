#!/usr/bin/env python
"""LPIPS (the tokenizer's VGG16 perceptual model, omnitokenizer_amd/lpips.py on csrc/lpips.hip and the conv / pool of
csrc/inception.hip): lpips_frames on uint8 256 x 256 frame pairs (17 pairs = one C3 clip, and 64), ms per call, TFLOP/s and
the fraction of the fp32-MFMA rate measured in the same process (tools/fvd_bench.py's probe), a per-layer breakdown with the
head's fraction of HBM bandwidth (against a device copy measured in the same process, and the 8 TB/s peak), and the same
network through torch fp32 F.conv2d / F.max_pool2d and a torch head on the same GPU and weights.

    python tools/lpips_bench.py [--pairs 17 64] [--size 256] [--iters 5] [--json out.json]

FLOPs are counted from the shapes: 2 * h * w * Cout * Cin * 9 per conv (the first with its 3 real channels), two images per
pair; the heads and pools are not counted.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from omnitokenizer_amd import inception, lpips, synth  # noqa: E402
from tools.fvd_bench import mfma_peak_tflops, timed  # noqa: E402

HBM_PEAK_TBS = 8.0


def conv_flops(H, W):
    """[(name, flops per image)] of the 13 convs at an H x W input"""
    out, h, w, cur = [], H, W, 1
    for s, i, cin, cout in lpips.CONVS:
        if s != cur:
            h, w, cur = h // 2, w // 2, s
        out.append((f"conv{i}", 2.0 * h * w * cout * cin * 9))
    return out


class TorchLPIPS:
    """the network in torch fp32, NCHW: ScalingLayer, the VGG slices, normalize_tensor, the lin layers, spatial means"""

    def __init__(self, sd, device):
        self.sd = {k: v.to(device) for k, v in sd.items()}

    def __call__(self, a, b):
        sd = self.sd
        x = torch.cat([a, b])
        x = (x - sd["scaling_layer.shift"]) / sd["scaling_layer.scale"]
        n, val, cur = a.shape[0], 0, 1
        for s, i, _, _ in lpips.CONVS:
            if s != cur:
                val = val + self.head(x, n, cur - 1)
                x = F.max_pool2d(x, 2, 2)
                cur = s
            x = F.relu(F.conv2d(x, sd[f"net.slice{s}.{i}.weight"], sd[f"net.slice{s}.{i}.bias"], padding=1))
        return val + self.head(x, n, cur - 1)

    def head(self, x, n, k):
        f = x / (torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True)) + 1e-10)
        return F.conv2d((f[:n] - f[n:]) ** 2, self.sd[f"lin{k}.model.1.weight"]).mean([2, 3], keepdim=True)


def copy_tbs():
    """device-to-device copy rate of a 1 GiB fp32 tensor, TB/s (read + write bytes)"""
    x = torch.empty(1 << 28, device="cuda")
    y = torch.empty_like(x)
    ms = timed(lambda: y.copy_(x), 10)
    return 2 * x.numel() * 4 / ms / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="+", default=[17, 64])
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "lpips_bench needs the GPU"
    torch.backends.cudnn.benchmark = False
    peak = mfma_peak_tflops()
    bw = copy_tbs()
    print(f"measured fp32-MFMA rate: {peak:.1f} TF/s; device copy {bw:.2f} TB/s (peak {HBM_PEAK_TBS} TB/s)")
    sd = synth.synth_lpips_state_dict(0)
    model = lpips.load_lpips("cuda", sd)
    ref = TorchLPIPS(sd, "cuda")
    S = a.size
    flops = conv_flops(S, S)
    total = sum(f for _, f in flops)
    results = []
    for P in a.pairs:
        ua = torch.from_numpy(synth.synth_fvd_clips(1, P, S, S, seed=P)).cuda()                  # [1, P, S, S, 3]
        ub = torch.from_numpy(synth.synth_fvd_clips(1, P, S, S, seed=P, noise=0.03, noise_seed=P + 1)).cuda()
        with torch.no_grad():
            ours = lambda: lpips.lpips_frames(ua, ub, model, layout="bthwc", shift=-0.5)  # noqa: E731
            ms = timed(ours, a.iters)
            fa = ((ua[0].cpu().float() / 255).cuda() - 0.5).permute(0, 3, 1, 2).contiguous()   # ToTensor's division
            fb = ((ub[0].cpu().float() / 255).cuda() - 0.5).permute(0, 3, 1, 2).contiguous()
            ms_t = timed(lambda: ref(fa, fb), a.iters)
            got = ours().view(-1).double().cpu()
            want = ref(fa, fb).view(-1).double().cpu()
            rel = ((got - want).abs() / want.abs()).max().item()
            # per layer, on the first chunk (at most 32 pairs: 64 images)
            n = min(P, model.max_pairs)
            pk = model.packed("cuda")
            x = torch.empty((2 * n, S, S, 4), device="cuda")
            for half, v in enumerate((ua, ub)):
                torch.ops.omnitok.lpips_preprocess(v.permute(0, 1, 4, 2, 3), -0.5, False, False, pk["shift"], pk["scale"],
                                                   0, x[half * n:(half + 1) * n])
            res = torch.zeros((n, 5), device="cuda", dtype=torch.float64)
            rows, h, cur = [], x, 1
            fl = dict(flops)
            for s, i, _, _ in lpips.CONVS:
                if s != cur:
                    hh, lw = h, pk["lins"][cur - 1]
                    t = timed(lambda hh=hh, lw=lw, k=cur - 1: lpips.layer_head(hh, lw, k, res), a.iters)
                    rows.append((f"head{cur - 1}", t, 0.0, hh.numel() * 4))
                    t = timed(lambda hh=hh: inception.maxpool2d(hh, 2, 2, 0), a.iters)
                    rows.append((f"pool{i - 1}", t, 0.0, hh.numel() * 4 * 5 / 4))
                    h, cur = inception.maxpool2d(h, 2, 2, 0), s
                w_, b_ = pk["convs"][[c[1] for c in lpips.CONVS].index(i)][1:]
                t = timed(lambda hh=h, w_=w_, b_=b_: inception.conv2d(hh, w_, b_, (3, 3), (1, 1), (1, 1), True), a.iters)
                rows.append((f"conv{i}", t, 2 * n * fl[f"conv{i}"], 0))
                h = inception.conv2d(h, w_, b_, (3, 3), (1, 1), (1, 1), True)
            t = timed(lambda hh=h: lpips.layer_head(hh, pk["lins"][4], 4, res), a.iters)
            rows.append(("head4", t, 0.0, h.numel() * 4))
            del x, h
        tf, tf_t = 2 * P * total / ms / 1e9, 2 * P * total / ms_t / 1e9
        r = {"pairs": P, "size": S, "gflop_per_pair": 2 * total / 1e9, "ms": ms, "tflops": tf, "frac_of_mfma_rate": tf / peak,
             "torch_ms": ms_t, "torch_tflops": tf_t, "speedup_vs_torch": ms_t / ms, "faster_than_torch": ms < ms_t,
             "max_rel_diff_vs_torch": rel, "layers_chunk_pairs": n, "layers": []}
        print(f"\n{P:3d} pairs at {S}x{S} uint8: {ms:8.2f} ms  {tf:6.1f} TF/s  {tf / peak:.2f} of the measured rate | "
              f"torch fp32 {ms_t:8.2f} ms  {tf_t:6.1f} TF/s | {ms_t / ms:.2f}x ({'faster' if ms < ms_t else 'SLOWER'}) | "
              f"max rel diff vs torch {rel:.2e}")
        print(f"  per layer ({n} pairs, {2 * n} images):  {'layer':8s} {'ms':>8s} {'TF/s':>7s} {'frac':>5s} {'TB/s':>6s} "
              f"{'of copy':>7s} {'of peak':>7s}")
        for name, lms, lf, by in rows:
            ltf = lf / lms / 1e9 if lf else 0.0
            tbs = by / lms / 1e9 if by else 0.0
            r["layers"].append({"layer": name, "ms": lms, "tflops": ltf, "tbs": tbs})
            print(f"              {name:8s} {lms:8.3f} {ltf:7.1f} {ltf / peak:5.2f} {tbs:6.2f} {tbs / bw:7.2f} "
                  f"{tbs / HBM_PEAK_TBS:7.2f}")
        conv_ms = sum(x[1] for x in rows if x[0].startswith("conv"))
        head_ms = sum(x[1] for x in rows if x[0].startswith("head"))
        print(f"  convs {conv_ms:.2f} ms, heads {head_ms:.2f} ms, pools {sum(x[1] for x in rows if x[0].startswith('pool')):.2f}"
              f" ms of the chunk")
        results.append(r)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"mfma_peak_tflops": peak, "copy_tbs": bw, "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
