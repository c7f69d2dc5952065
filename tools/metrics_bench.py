#!/usr/bin/env python
"""Reconstruction metrics at C3 scale (csrc/metrics.hip): the time of psnr_ssim on a [32, 3, 17, 256, 256] fp32 pair and the
roofs it sits under, next to the reference's CPU functions.  Writes one JSON object per line.

    python tools/metrics_bench.py [--iters 20]     # on the MI355X: fp64_peak, psnr_ssim, psnr_only
    python tools/metrics_bench.py --cpu-ref        # where the reference sources are (they are not on the GPU machine):
                                                   # calculate_psnr / calculate_ssim of the reference with the cv2 stand-in
                                                   # of tests/golden/make_golden_metrics.py, on --cpu-threads processes

  fp64_peak   omnitok_debug_fp64_peak: 8 independent v_fma_f64 chains per lane, 2048 blocks of 256 threads; 2 FLOP per FMA
  psnr_ssim   "bcthw" fp32 pair (the tokenizer's layout, read in place), both metrics; CUDA events around --iters calls
              (workspace and output allocation included: PyTorch's caching allocator)
  psnr_only   the same with OMNITOK_METRICS_PSNR alone (the path calculate_psnr takes)

FLOPs counted for SSIM (the kernel's own instruction mix, per valid output pixel of a channel plane): 5 maps x 11 taps
vertical + 5 x 11 horizontal FMAs (220 FLOP), the 3 products a^2, b^2, ab per input row in the vertical window of 14
rows per 4 outputs (10.5 MUL), the map (9 ops + 1 division): 240 FLOP.  Bytes: each input element once (2 x 4 B per
pixel); the strips' 10-row halos and the tiles' 10-column halos re-read 31 % + 4 % more, from L2 / MALL mostly.
HBM share against 6.29 TB/s, the measured float4-copy rate of the chip (MI355X_MICROARCH.md), and 8 TB/s (spec).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12
FP64_SPEC = 78.6e12
B, C, F, H, W = 32, 3, 17, 256, 256


def _time(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def fp64_peak():
    import ctypes
    from omnitokenizer_amd import _lib
    lib = _lib.load()
    seeds = torch.rand(66, dtype=torch.float64, device="cuda")
    seeds[64], seeds[65] = 0.999999, 1e-7
    blocks, iters = 2048, 512
    out = torch.empty(blocks * 256, dtype=torch.float64, device="cuda")

    def run():
        _lib.check(lib.omnitok_debug_fp64_peak(ctypes.c_void_p(seeds.data_ptr()), ctypes.c_void_p(out.data_ptr()), blocks,
                                               iters, torch.cuda.current_stream().cuda_stream), "fp64_peak")
    ms = _time(run, 10)
    flop = 2.0 * blocks * 256 * iters * 128
    assert torch.isfinite(out).all()
    return flop / (ms * 1e-3)


def gpu(iters):
    from omnitokenizer_amd import metrics as mt
    peak = fp64_peak()
    print(json.dumps(dict(name="fp64_peak", tflops=round(peak / 1e12, 2), spec_tflops=FP64_SPEC / 1e12,
                          of_spec=round(peak / FP64_SPEC, 3))), flush=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    a = torch.rand(B, C, F, H, W, device="cuda", generator=g)
    b = (a + 0.08 * torch.randn(a.shape, device="cuda", generator=g)).clamp_(0, 1)
    va, vb = mt._operands(a, b, "bcthw")
    planes = B * F * C
    valid = planes * (H - 10) * (W - 10)
    flop = valid * 240.0
    nbytes = 2 * 4.0 * a.numel()
    for name, flags in (("psnr_ssim", mt.FLAG_PSNR | mt.FLAG_SSIM), ("psnr_only", mt.FLAG_PSNR)):
        ms = _time(lambda: mt._scores(va, vb, flags), iters)
        d = dict(name=name, shape=[B, C, F, H, W], layout="bcthw", ms=round(ms, 4), iters=iters,
                 hbm_tbs=round(nbytes / (ms * 1e-3) / 1e12, 2), of_hbm_measured=round(nbytes / (ms * 1e-3) / HBM_MEASURED, 3),
                 of_hbm_spec=round(nbytes / (ms * 1e-3) / HBM_SPEC, 3))
        if flags & mt.FLAG_SSIM:
            d.update(fp64_tflops=round(flop / (ms * 1e-3) / 1e12, 2), of_fp64_measured=round(flop / (ms * 1e-3) / peak, 3),
                     of_fp64_spec=round(flop / (ms * 1e-3) / FP64_SPEC, 3), fp64_floor_ms=round(flop / peak * 1e3, 4),
                     hbm_floor_ms=round(nbytes / HBM_MEASURED * 1e3, 4))
        print(json.dumps(d), flush=True)


def _cpu_chunk(args):
    lo, hi, seed = args
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_metrics as mg
    cp, cs = mg.load_reference_metrics()
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(B, F, C, H, W, generator=g)[lo:hi]
    b = (a + 0.08 * torch.randn(a.shape, generator=torch.Generator().manual_seed(seed + 1))).clamp_(0, 1)
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        t0 = time.perf_counter()
        cp.calculate_psnr(a, b)
        t1 = time.perf_counter()
        cs.calculate_ssim(a, b)
        t2 = time.perf_counter()
    return t1 - t0, t2 - t1


def cpu_ref(threads, clips):
    """the reference's calculate_psnr + calculate_ssim over `clips` clips of the C3 batch, split over `threads` processes
    (each process one share of the clips: the functions are serial per frame).  Reported: the CPU seconds per clip, and
    the wall time of the 32-clip batch on `threads` threads at perfect scaling (CPU seconds * 32 / clips / threads)"""
    import multiprocessing as mp
    os.environ.setdefault("OMP_NUM_THREADS", "1")
    per = max(1, clips // threads)
    chunks = [(lo, min(clips, lo + per), 0) for lo in range(0, clips, per)]
    t0 = time.perf_counter()
    with mp.get_context("spawn").Pool(min(threads, len(chunks))) as pool:
        res = pool.map(_cpu_chunk, chunks)
    wall = time.perf_counter() - t0
    psnr_s, ssim_s = sum(r[0] for r in res), sum(r[1] for r in res)
    print(json.dumps(dict(name="cpu_reference", clips_measured=clips, processes=min(threads, len(chunks)),
                          cpu_seconds_psnr=round(psnr_s, 2), cpu_seconds_ssim=round(ssim_s, 2),
                          cpu_s_per_clip=round((psnr_s + ssim_s) / clips, 3), wall_s_measured=round(wall, 2),
                          est_wall_s_32_clips=round((psnr_s + ssim_s) * B / clips / threads, 2), threads=threads,
                          host_cpus=os.cpu_count())), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--cpu-ref", action="store_true")
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--cpu-clips", type=int, default=32)
    a = ap.parse_args()
    if a.cpu_ref:
        cpu_ref(a.cpu_threads, a.cpu_clips)
        return
    if not torch.cuda.is_available():
        raise SystemExit("metrics_bench needs the MI355X (no CPU fallback); --cpu-ref times the reference on the CPU")
    gpu(a.iters)


if __name__ == "__main__":
    main()
