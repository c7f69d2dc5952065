#!/usr/bin/env python
"""The Pillow-exact resize (omnitokenizer_amd.frames.resize_frames on csrc/resize_pil.hip) at the image models' workload:
64 images of 500 x 375 (w x h) -> 256 x 256 bicubic, out="pixels" (ImageDataset's transform, what encode() reads), ms per
batch on the GPU, the bytes per second that is, and -- where Pillow is installed -- Pillow's time for the same 64 images
(Image.resize + the ToTensor / Normalize arithmetic in numpy) in 1 process and spread over 16 (every process builds its
images first; only the transform is timed).

    python tools/resize_bench.py [--batch 64] [--height 375] [--width 500] [--size 256] [--seconds 1.0] [--json out.json]

GPU times are device events around back-to-back calls after a warm-up, over a window of --seconds:
  call   frames.resize_frames(...) as a user calls it: descriptors built in Python, workspace and output from PyTorch's
         allocator, three launches per 32 images
  graph  the same call captured once in a torch.cuda.graph and replayed: the device's share alone
Bytes: `compulsory` = the uint8 sources read once + the fp32 output written once; `moved` adds the uint8 intermediate
(written by the horizontal pass, read by the vertical one) and the coefficient tables.  The rates are end-to-end rates of
back-to-back calls on the same buffers: the working set (under 130 MB at the default workload) fits the 256 MB Infinity
Cache and stays warm in it, and the time is that of the whole call or replay, launch gaps included, not a kernel's.  They
are set against the 8 TB/s HBM peak only for scale: they are not the share of HBM bandwidth a kernel reaches.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HBM_PEAK = 8.0e12


_IMAGES = []   # a Pillow worker's images, built once by _pillow_init


def _pillow_init(seed, count, h, w):
    from PIL import Image
    rng = np.random.default_rng(seed)
    _IMAGES[:] = [Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for _ in range(count)]


def _pillow_some(args):
    """Pillow's transform of the first `count` prepared images -> seconds; only the transform is inside the clock"""
    count, size = args
    from PIL import Image
    t0 = time.perf_counter()
    for im in _IMAGES[:count]:
        u = np.asarray(im.resize((size, size), Image.BICUBIC))
        (u.astype(np.float32) / np.float32(255) - np.float32(0.5)).transpose(2, 0, 1).copy()
    return time.perf_counter() - t0


def pillow_times(batch, h, w, size, procs=16):
    """(ms for the batch in this process; spread over `procs` processes: ms of the slowest worker's transform loop and ms
    of wall time around the pool.map that hands the shares out and collects them; Pillow's version).  Every process builds
    its images before any clock starts."""
    import multiprocessing as mp

    import PIL
    _pillow_init(0, batch, h, w)
    one = min(_pillow_some((batch, size)) for _ in range(3)) * 1e3
    del _IMAGES[:]
    per = [batch // procs + (i < batch % procs) for i in range(procs)]
    jobs = [(n, size) for n in per if n]
    with mp.get_context("spawn").Pool(len(jobs), _pillow_init, (1, max(per), h, w)) as pool:   # the workers never touch the GPU
        pool.map(_pillow_some, jobs, 1)                      # start-up, imports, the images
        slowest = wall = float("inf")
        for _ in range(5):
            t0 = time.perf_counter()
            inner = pool.map(_pillow_some, jobs, 1)
            wall = min(wall, time.perf_counter() - t0)
            slowest = min(slowest, max(inner))
    return one, slowest * 1e3, wall * 1e3, PIL.__version__


def timed_window(fn, seconds):
    """ms per call: events around enough back-to-back calls to fill `seconds`"""
    import torch
    from tools.fvd_bench import timed
    ms = timed(fn, 5)
    iters = max(10, int(seconds * 1e3 / max(ms, 1e-3)))
    torch.cuda.synchronize()
    return timed(fn, iters), iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--height", type=int, default=375)
    ap.add_argument("--width", type=int, default=500)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    B, H, W, R = a.batch, a.height, a.width, a.size
    r = {"batch": B, "source_hw": [H, W], "size": R, "interpolation": "bicubic", "out": "pixels"}

    try:   # before the GPU is opened: the worker processes are plain CPU processes
        one, many, wall, ver = pillow_times(B, H, W, R)
        r.update(pillow_version=ver, pillow_ms_1_process=one, pillow_ms_16_processes=many, pillow_ms_16_processes_wall=wall)
        print(f"Pillow {ver}: {one:.2f} ms for {B} images in 1 process; spread over 16 processes {many:.2f} ms (the slowest "
              f"worker's transform loop), {wall:.2f} ms of wall time around pool.map (dispatch and collection included)")
    except ImportError:
        r.update(pillow_version=None)
        print("Pillow is not installed here: GPU figures only")

    import torch
    from omnitokenizer_amd import frames
    from tests import pil_resize_oracle as oracle
    assert torch.cuda.is_available(), "resize_bench needs the GPU"
    rng = np.random.default_rng(0)
    host = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(B)]
    imgs = [torch.from_numpy(x).cuda() for x in host]
    fn = lambda: frames.resize_frames(imgs, (R, R), True, out="pixels")  # noqa: E731
    got = fn()
    want = torch.from_numpy(oracle.resize(host[B - 1], (R, R), "bicubic")).permute(2, 0, 1).float().div(255).sub(0.5)
    exact = bool(torch.equal(got[B - 1].cpu(), want))
    print(f"last image equals the numpy restatement of Pillow bit for bit: {exact}")
    ksw, ksh = oracle.coeffs(W, R, 0)[0], oracle.coeffs(H, R, 0)[0]
    compulsory = B * (H * W * 3 + 3 * R * R * 4)
    moved = compulsory + B * (2 * H * R * 3 + 2 * 4 * R * (ksw + ksh + 4))
    ms, iters = timed_window(fn, a.seconds)
    r.update(exact=exact, call_ms=ms, call_iters=iters, compulsory_bytes=compulsory, moved_bytes=moved,
             call_compulsory_tbps=compulsory / ms / 1e9, call_rate_over_hbm_peak=compulsory / ms / 1e-3 / HBM_PEAK)
    print(f"call:  {ms:.4f} ms per batch of {B} ({ms / B * 1e3:.2f} us per image, {iters} calls), "
          f"{compulsory / ms / 1e9:.3f} TB/s compulsory = {compulsory / ms / 1e-3 / HBM_PEAK:.3f} against the 8 TB/s peak")
    try:
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            fn()
        torch.cuda.current_stream().wait_stream(s)
        with torch.cuda.graph(g):
            y = fn()
        g.replay()
        torch.cuda.synchronize()
        same = bool(torch.equal(y, got))
        gms, giters = timed_window(g.replay, a.seconds)
        r.update(graph_ms=gms, graph_iters=giters, graph_equal=same, graph_compulsory_tbps=compulsory / gms / 1e9,
                 graph_moved_tbps=moved / gms / 1e9, graph_rate_over_hbm_peak=compulsory / gms / 1e-3 / HBM_PEAK,
                 graph_moved_rate_over_hbm_peak=moved / gms / 1e-3 / HBM_PEAK)
        print(f"graph: {gms:.4f} ms per batch ({gms / B * 1e3:.2f} us per image, {giters} replays, equal to the call: {same}), "
              f"{compulsory / gms / 1e9:.3f} TB/s compulsory = {compulsory / gms / 1e-3 / HBM_PEAK:.3f} against peak; "
              f"{moved / gms / 1e9:.3f} TB/s moved = {moved / gms / 1e-3 / HBM_PEAK:.3f} against peak")
    except Exception as e:  # noqa: BLE001
        r.update(graph_ms=None, graph_error=repr(e))
        print(f"graph: not measured ({e!r})")
    if r.get("pillow_version"):
        best = r.get("graph_ms") or ms
        print(f"Pillow / GPU call: {r['pillow_ms_1_process'] / ms:.0f}x (1 process), {r['pillow_ms_16_processes'] / ms:.0f}x "
              f"(16 processes); against the device's share alone {r['pillow_ms_1_process'] / best:.0f}x / "
              f"{r['pillow_ms_16_processes'] / best:.0f}x")
    print(f"bytes per batch: {compulsory / 1e6:.1f} MB compulsory, {moved / 1e6:.1f} MB moved (a cache-warm working set: the "
          f"rates above are end-to-end, with the 8 TB/s HBM peak only as a scale)")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
