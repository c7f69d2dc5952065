#!/usr/bin/env python
"""Validation losses (omnitokenizer_amd/losses.py on csrc/losses.hip) at the C3 shapes, B clips of 17 x 256 x 256:

  fused    omnitok::recon_losses on x, x_recon: ms per call and GB/s of its one read of both operands, against the 8 TB/s
           peak and against a device copy measured in the same process; per flags word (l1 / mse + laplace / all three)
  eager    the same expressions composed in torch on the same GPU (F.l1_loss, F.mse_loss and the reference's
           logits_laplace) -- the baseline: there was no such path before.  mse + laplace is timed twice: "in place", as the
           reference runs it (x += 0.5, x_recon += 0.5 on the arguments; timed on scratch tensors, which drift by 0.5 per
           call -- elementwise kernels take the same time whatever the values), and "clones", what a caller pays who
           keeps x as forward(x) here does.  Both ratios are reported; the in-place one is the harder for the fused pass.
  forward  whole OmniTokenizer_VQGAN.forward(x) (perceptual_weight 0: LPIPS has its own bench, tools/lpips_bench.py)
           against encode + decode of the same batch

    python tools/validation_bench.py [--batch 32] [--frames 17] [--size 256] [--iters 10] [--repeats 3] [--json out.json]

Each figure is the median of --repeats timings of --iters back-to-back calls (events around the loop, one warm-up call).
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from omnitokenizer_amd import OmniTokenizer_VQGAN, losses, make_args, synth  # noqa: E402
from omnitokenizer_amd.config import OmniTokConfig  # noqa: E402
from tools.fvd_bench import timed  # noqa: E402
from tools.lpips_bench import copy_tbs  # noqa: E402

HBM_PEAK_TBS = 8.0


def median_ms(fn, iters, repeats):
    return statistics.median(timed(fn, iters) for _ in range(repeats))


def eager_l1(x, r):
    return F.l1_loss(r, x)


def eager_mse_laplace(x, r, clone):
    """omnitokenizer.py:391-394 with logits_laplace's arithmetic; the reference mutates x and x_recon, a caller who keeps
    them pays the two clones"""
    mse = F.mse_loss(r, x)
    if clone:
        x, r = x.clone(), r.clone()
    x += 0.5
    r += 0.5
    xl = (1 - 2 * 0.1) * x + 0.1
    rl = (1 - 2 * 0.1) * r + 0.1
    return mse, F.l1_loss(xl, rl)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=17)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "validation_bench needs the GPU"
    B, T, R = a.batch, a.frames, a.size
    out = dict(batch=B, frames=T, size=R, iters=a.iters, repeats=a.repeats, device=torch.cuda.get_device_name(0))
    out["copy_tbs"] = copy_tbs()
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.rand((B, 3, T, R, R), device="cuda", generator=g) - 0.5
    r = (x + 0.05 * torch.randn(x.shape, device="cuda", generator=g)).clamp_(-0.6, 0.6)
    gbytes = 2 * x.numel() * 4 / 1e9
    out["operand_gbytes"] = gbytes
    rows = []
    for name, flags in (("l1", losses.FLAG_L1), ("mse+laplace", losses.FLAG_MSE | losses.FLAG_LAPLACE),
                        ("all", losses.FLAG_ALL)):
        ms = median_ms(lambda: losses.recon_sums(x, r, flags), a.iters, a.repeats)
        rows.append(dict(path="fused", what=name, ms=ms, gbs=gbytes / ms * 1e3, of_peak=gbytes / ms / HBM_PEAK_TBS,
                         of_copy=gbytes / ms / out["copy_tbs"]))
    rows.append(dict(path="eager", what="l1", ms=median_ms(lambda: eager_l1(x, r), a.iters, a.repeats)))
    rows.append(dict(path="eager", what="mse+laplace", how="clones",
                     ms=median_ms(lambda: eager_mse_laplace(x, r, True), a.iters, a.repeats)))
    xs, rs = x.clone(), r.clone()   # scratch: the in-place shifts accumulate here, not in x and r
    rows.append(dict(path="eager", what="mse+laplace", how="in place",
                     ms=median_ms(lambda: eager_mse_laplace(xs, rs, False), a.iters, a.repeats)))
    del xs, rs
    out["recon"] = rows
    fused = {w["what"]: w["ms"] for w in rows if w["path"] == "fused"}
    out["speedup"] = {" ".join(filter(None, (w["what"], w.get("how")))): w["ms"] / fused[w["what"]]
                      for w in rows if w["path"] == "eager"}
    # agreement of the two paths on this input (the eager means are fp32 sums)
    s, tot = losses.recon_sums(x, r)
    n = x.numel()
    out["l1_fused_vs_eager"] = [float(tot[0] / n), float(eager_l1(x, r))]
    del s

    args = make_args(2, resolution=R, perceptual_weight=0.0)
    cfg = OmniTokConfig.from_args(args)
    m = OmniTokenizer_VQGAN(args)
    m.load_state_dict(synth.synth_state_dict(cfg, seed=0), strict=True)
    m = m.cuda().eval()
    xv = synth.synth_video(B, T, R, seed=1234).cuda()

    def enc_dec():
        return m.decode(m.encode(xv, False), False)

    it = max(2, a.iters // 3)
    out["encode_decode_ms"] = median_ms(enc_dec, it, a.repeats)
    out["forward_ms"] = median_ms(lambda: m(xv), it, a.repeats)
    out["forward_over_encode_decode"] = out["forward_ms"] / out["encode_decode_ms"]

    print(f"{out['device']}: B {B} x 3 x {T} x {R} x {R}, operands {gbytes:.3f} GB, device copy {out['copy_tbs']:.2f} TB/s")
    for w in rows:
        extra = (f"  {w['gbs']:8.0f} GB/s  {100 * w['of_peak']:5.1f}% of {HBM_PEAK_TBS:.0f} TB/s  "
                 f"{100 * w['of_copy']:5.1f}% of the copy rate") if w["path"] == "fused" else ""
        print(f"  {w['path']:5s} {w['what']:12s} {w.get('how', ''):9s} {w['ms']:8.3f} ms{extra}")
    for k, v in out["speedup"].items():
        print(f"  fused over eager, {k}: {v:.2f}x")
    print(f"  forward(x) {out['forward_ms']:.2f} ms, encode + decode {out['encode_decode_ms']:.2f} ms, ratio "
          f"{out['forward_over_encode_decode']:.3f}")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
