#!/usr/bin/env python
"""I3D forward (the FVD feature net, omnitokenizer_amd/i3d.py on csrc/i3d.hip) at 224 x 224: ms per call, TFLOP/s and the
fraction of the fp32-MFMA rate measured in the same process (tools/mfma_peak.py's probe, randn operands, 2 waves / SIMD), a
per-layer breakdown, and the same network through torch fp32 F.conv3d / F.max_pool3d / F.avg_pool3d on the same GPU (what
the reference's vqgan_eval.py runs today; restated here with the same folded weights, BN folded into the conv as the
port does -- a fold the reference does not do, which only makes the torch path cheaper).

    python tools/fvd_bench.py [--batches 16 32] [--frames 17 16] [--iters 5] [--json out.json]

FLOPs are counted from the shapes: 2 * M * N * K per conv (K without the channel padding of Conv3d_1a: 3 * 343).
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from omnitokenizer_amd import _lib, i3d, synth  # noqa: E402


def mfma_peak_tflops() -> float:
    lib = _lib.load()
    x = torch.randn(4096, device="cuda")
    blocks, lds, iters = 512, 60 * 1024, 4000
    out = torch.empty(blocks * 256, device="cuda")
    clk = torch.zeros(2, dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def run():
        lib.omnitok_debug_mfma_peak(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(out.data_ptr()), blocks, iters, lds,
                                    ctypes.c_void_p(clk.data_ptr()), s)
    for _ in range(2):
        run()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(5):
        run()
    b.record()
    torch.cuda.synchronize()
    return blocks * 4 * iters * 32 * 4096.0 / (a.elapsed_time(b) / 5) / 1e9


def layer_flops(T, R):
    """[(endpoint, flops per clip)] from the shapes"""
    out, ext = [], (T, R, R)
    for p in i3d.PLAN:
        if p[0] == "unit":
            o = tuple(i3d.same_pad(e, k, s)[1] for e, k, s in zip(ext, p[4], p[5]))
            out.append((p[1], 2.0 * o[0] * o[1] * o[2] * p[3] * p[2] * p[4][0] * p[4][1] * p[4][2]))
            ext = o
        elif p[0] == "pool":
            ext = tuple(i3d.same_pad(e, k, s)[1] for e, k, s in zip(ext, p[2], p[3]))
            out.append((p[1], 0.0))
        else:
            n = ext[0] * ext[1] * ext[2]
            out.append((p[1], 2.0 * n * sum(ci * co * k ** 3 for _, ci, co, k in i3d.mixed_units(p[1]))))
    out.append(("Logits", 2.0 * (ext[0] - 1) * (ext[1] - 6) * (ext[2] - 6) * 1024 * 400))
    return out


class TorchI3D:
    """the network in torch fp32, NCDHW, with the reference's F.pad "same" padding, on the folded weights"""

    def __init__(self, sd, device):
        self.w = {}
        for name, *_ in i3d.units():
            w, b = i3d.fold_bn(sd, name)
            self.w[name] = (w.float().to(device), b.float().to(device))
        self.lw = (sd["logits.conv3d.weight"].to(device), sd["logits.conv3d.bias"].to(device))

    @staticmethod
    def _pad(x, k, s):
        pads = []
        for e, kk, ss in zip(reversed(x.shape[2:]), reversed(k), reversed(s)):
            pad = max(kk - (e % ss or ss), 0)
            pads += [pad // 2, pad - pad // 2]
        return F.pad(x, pads)

    def unit(self, x, name, k, s):
        w, b = self.w[name]
        return F.relu(F.conv3d(self._pad(x, k, s), w, b, stride=s))

    def pool(self, x, k, s):
        return F.max_pool3d(self._pad(x, k, s), k, s)

    def step(self, x, p):
        if p[0] == "unit":
            return self.unit(x, p[1], p[4], p[5])
        if p[0] == "pool":
            return self.pool(x, p[2], p[3])
        n = p[1]
        return torch.cat([self.unit(x, n + ".b0", (1, 1, 1), (1, 1, 1)),
                          self.unit(self.unit(x, n + ".b1a", (1, 1, 1), (1, 1, 1)), n + ".b1b", (3, 3, 3), (1, 1, 1)),
                          self.unit(self.unit(x, n + ".b2a", (1, 1, 1), (1, 1, 1)), n + ".b2b", (3, 3, 3), (1, 1, 1)),
                          self.unit(self.pool(x, (3, 3, 3), (1, 1, 1)), n + ".b3b", (1, 1, 1), (1, 1, 1))], dim=1)

    def head(self, x):
        return F.conv3d(F.avg_pool3d(x, (2, 7, 7), stride=1), *self.lw).squeeze(3).squeeze(3).mean(dim=2)

    def __call__(self, x):
        for p in i3d.PLAN:
            x = self.step(x, p)
        return self.head(x)


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def per_layer(run_step, x0, iters):
    """[(endpoint, ms)] timing each step on its own input (events around `iters` repeats)"""
    rows, x = [], x0
    for p in i3d.PLAN + [("head", "Logits")]:
        y = run_step(x, p)
        ms = timed(lambda: run_step(x, p), iters)
        rows.append((p[1], ms))
        x = y
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--frames", type=int, nargs="+", default=[17, 16])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "fvd_bench needs the GPU"
    torch.backends.cudnn.benchmark = False
    peak = mfma_peak_tflops()
    print(f"measured fp32-MFMA rate: {peak:.1f} TF/s")
    sd = synth.synth_i3d_state_dict(0)
    model = i3d.InceptionI3d(400)
    model.load_state_dict(sd)
    ref = TorchI3D(sd, "cuda")
    results = []
    for T in a.frames:
        flops = layer_flops(T, 224)
        total = sum(f for _, f in flops)
        for B in a.batches:
            MAXC = min(B, i3d.MAX_CHUNK)
            x = (torch.rand((B, T, 224, 224, 4), device="cuda") * 2 - 1)
            x[..., 3] = 0
            xt = x[..., :3].permute(0, 4, 1, 2, 3).contiguous()
            with torch.no_grad():
                ms = timed(lambda: model.forward_channels_last(x), a.iters)
                ms_t = timed(lambda: ref(xt), a.iters)
                diff = (model.forward_channels_last(x) - ref(xt)).abs().max().item()
                pk = model._weights(x.device)

                def ours_step(h, p):
                    if p[0] == "head":
                        return i3d.i3d_head(h, *pk["logits"])
                    if p[0] == "unit":
                        return i3d.conv3d_same(h, *pk[p[1]], p[4], p[5])
                    if p[0] == "pool":
                        return i3d.maxpool3d_same(h, p[2], p[3])
                    return model._mixed(h, p[1], pk)
                rows = per_layer(ours_step, x[:MAXC].contiguous(), a.iters)
                rows_t = per_layer(lambda h, p: ref.head(h) if p[0] == "head" else ref.step(h, p), xt[:MAXC], a.iters)
            tf, tf_t = B * total / ms / 1e9, B * total / ms_t / 1e9
            r = {"B": B, "T": T, "gflop_per_clip": total / 1e9, "ms": ms, "tflops": tf, "frac_of_mfma_rate": tf / peak,
                 "torch_ms": ms_t, "torch_tflops": tf_t, "speedup_vs_torch": ms_t / ms, "max_logit_diff_vs_torch": diff,
                 "layers": []}
            print(f"\nB {B:3d} T {T}: {ms:8.2f} ms  {tf:6.1f} TF/s  {tf / peak:.2f} of the measured rate | torch fp32 "
                  f"{ms_t:8.2f} ms  {tf_t:6.1f} TF/s | {ms_t / ms:.2f}x | max |logit diff| {diff:.2e}")
            print(f"  per layer at B = {MAXC} (one chunk):  {'endpoint':18s} {'ms':>8s} {'TF/s':>7s} {'frac':>5s} "
                  f"{'torch ms':>9s}")
            for (name, f), (_, lms), (_, tms) in zip(flops, rows, rows_t):
                ltf = MAXC * f / lms / 1e9 if f else 0.0
                r["layers"].append({"endpoint": name, "ms": lms, "tflops": ltf, "torch_ms": tms})
                print(f"  {'':34s} {name:18s} {lms:8.3f} {ltf:7.1f} {ltf / peak:5.2f} {tms:9.3f}")
            results.append(r)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"mfma_peak_tflops": peak, "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
