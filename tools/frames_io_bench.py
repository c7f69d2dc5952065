#!/usr/bin/env python
"""Frames in, frames out at C3 scale (csrc/frames.hip): kernel times and the share of HBM peak they reach, next to the
host-side costs they replace.  Needs the MI355X (no CPU fallback); writes one JSON object per line.

    python tools/frames_io_bench.py [--iters 50] [--cpu-threads 16]

  ingest_bilinear   32 clips of 17x360x640 uint8 -> [32, 3, 17, 256, 256] fp32 (the reference's preprocess)
  ingest_none       32 clips of 17x256x256 uint8 -> the same pixels (crop + VideoNorm: pre-pass + conversion)
  egress            [32, 3, 17, 256, 256] fp32 (a C3 decode) -> uint8 [32, 17, 256, 256, 3]
  cpu_preprocess    the reference's preprocess arithmetic (data.py:305-350, restated in torch ops) on the CPU for the
                    bilinear batch, at --cpu-threads threads
  copies            pinned host <-> device copies of the uint8 frames vs the fp32 pixels of one C3 batch

Bytes per kernel are what the algorithm must move (every source byte read once, every output byte written once);
the share is those bytes over kernel time over the 8 TB/s HBM peak (MI355X_MICROARCH.md).  Kernel time: CUDA events
around --iters back-to-back launches after a warm-up.
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

PEAK_HBM = 8.0e12


def _time(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters * 1e3  # us


def _line(name, us, nbytes, **extra):
    d = dict(name=name, us=round(us, 1), bytes=nbytes, tb_s=round(nbytes / us / 1e6, 3),
             hbm_peak_fraction=round(nbytes / us / 1e6 / (PEAK_HBM / 1e12), 3), **extra)
    print(json.dumps(d), flush=True)
    return d


def cpu_preprocess(video, resolution):
    """data.py:305-350 for in_channels 3 (sequence_length None, every frame), restated in the same torch ops"""
    video = video.permute(0, 3, 1, 2).contiguous().float() / 255.
    t, c, h, w = video.shape
    scale = resolution / min(h, w)
    target = (resolution, math.ceil(w * scale)) if h < w else (math.ceil(h * scale), resolution)
    video = F.interpolate(video, size=target, mode="bilinear", align_corners=False)
    t, c, h, w = video.shape
    ws, hs = (w - resolution) // 2, (h - resolution) // 2
    video = video[:, :, hs:hs + resolution, ws:ws + resolution].permute(1, 0, 2, 3).contiguous()
    video -= 0.5
    return video


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--cpu-reps", type=int, default=2)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "frames_io_bench needs the MI355X"
    from omnitokenizer_amd import frames as fr
    B, T, R = 32, 17, 256
    g = torch.Generator(device="cuda").manual_seed(0)
    out = {}

    big = torch.randint(0, 256, (B, T, 360, 640, 3), dtype=torch.uint8, device="cuda", generator=g)
    pix_bytes = B * 3 * T * R * R * 4
    x = fr.frames_to_pixels(big, resize="bilinear", resolution=R)
    out["ingest_bilinear"] = _line("ingest_bilinear", _time(lambda: fr.frames_to_pixels(big, resize="bilinear", resolution=R),
                                                            a.iters), big.numel() + pix_bytes, shape=list(x.shape))
    small = torch.randint(0, 256, (B, T, R, R, 3), dtype=torch.uint8, device="cuda", generator=g)
    out["ingest_none"] = _line("ingest_none", _time(lambda: fr.frames_to_pixels(small), a.iters), small.numel() + pix_bytes,
                               note="VideoNorm pre-pass included (it stops reading once a byte > 1 is seen)")
    out["ingest_none_totensor"] = _line("ingest_none_totensor", _time(lambda: fr.frames_to_pixels(small, norm="totensor"),
                                                                      a.iters), small.numel() + pix_bytes)
    rec = torch.rand(B, 3, T, R, R, device="cuda", generator=g) - 0.5
    out["egress_thwc"] = _line("egress_thwc", _time(lambda: fr.pixels_to_frames(rec), a.iters), pix_bytes + small.numel())
    out["egress_cthw"] = _line("egress_cthw", _time(lambda: fr.pixels_to_frames(rec, "cthw"), a.iters),
                               pix_bytes + small.numel())

    # the reference-style CPU pipeline for the bilinear batch
    torch.set_num_threads(a.cpu_threads)
    host = big.cpu()
    cpu_preprocess(host[0], R)
    best = float("inf")
    for _ in range(a.cpu_reps):
        t0 = time.perf_counter()
        for i in range(B):
            cpu_preprocess(host[i], R)
        best = min(best, time.perf_counter() - t0)
    d = dict(name="cpu_preprocess", threads=a.cpu_threads, batch_ms=round(best * 1e3, 1),
             ms_per_clip=round(best * 1e3 / B, 2), vs_gpu_ingest=round(best * 1e6 / out["ingest_bilinear"]["us"], 1))
    print(json.dumps(d), flush=True)

    # pinned copies: uint8 frames vs fp32 pixels of one C3 batch
    for name, dev in (("u8_frames", small), ("f32_pixels", rec)):
        h = torch.empty(dev.shape, dtype=dev.dtype, pin_memory=True)
        h2d = _time(lambda: dev.copy_(h, non_blocking=True), 10)
        d2h = _time(lambda: h.copy_(dev, non_blocking=True), 10)
        nb = dev.numel() * dev.element_size()
        print(json.dumps(dict(name="copy_" + name, bytes=nb, h2d_ms=round(h2d / 1e3, 2), d2h_ms=round(d2h / 1e3, 2),
                              h2d_gb_s=round(nb / h2d / 1e3, 1), d2h_gb_s=round(nb / d2h / 1e3, 1))), flush=True)


if __name__ == "__main__":
    main()
