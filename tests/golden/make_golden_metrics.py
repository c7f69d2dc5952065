"""Generates tests/golden/metrics_*.npz: the reference's OWN PSNR and SSIM (evaluation/common_metrics_on_video_quality,
calculate_psnr.py and calculate_ssim.py) on seeded video pairs, for omnitokenizer_amd.metrics (csrc/metrics.hip).  Runs the
UNMODIFIED reference files, located through oracle/ref_harness.py (read-only) and loaded by file path, not through the
package __init__ (which imports the LPIPS and FVD code), in the build container only:

    python tests/golden/make_golden_metrics.py

cv2 is not installed there.  calculate_ssim.py uses two of its functions; a stand-in module in sys.modules provides exactly
those, in fp64:
  getGaussianKernel(ksize, sigma)  cv2's formula: t_i = exp((-0.5 / sigma^2) x x), x = i - (ksize - 1) / 2, times 1 / sum t
  filter2D(img, -1, k)             the correlation of img with k over the valid region, padded back to img's size with zeros
                                   (calculate_ssim.py crops [5:-5, 5:-5], which discards exactly the pad)
Everything else -- the channel loop, the constants, the crop, the float32 PSNR, the means and the aggregation -- is the
reference's own code.

Each fixture stores the inputs, as uint8 frames `u8a` / `u8b` [B,T,H,W,3] (the videos are u8 / 255 in fp32, permuted to the
reference's [B,T,C,H,W]) or, for the case "float", the fp32 tokenizer-convention pair `xa` / `xb` [B,3,T,H,W] whose videos are
xa + 0.5 and clamp(xb + 0.5, 0, 1) (vqgan_eval.py:141-148); the per-frame results `psnr` / `ssim` [B,T] of the reference's
img_psnr / calculate_ssim_function; and the dicts of calculate_psnr / calculate_ssim as `psnr_value`, `psnr_std`,
`ssim_value`, `ssim_std` [T].
"""
import importlib.util
import math
import os
import sys
import types
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
warnings.filterwarnings("ignore")

from oracle import ref_harness as rh  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def _gaussian_kernel(ksize, sigma):
    scale2x = -0.5 / (sigma * sigma)
    t = [math.exp(scale2x * (i - (ksize - 1) * 0.5) * (i - (ksize - 1) * 0.5)) for i in range(ksize)]
    s = 0.0
    for v in t:
        s += v
    s = 1.0 / s
    return np.array([v * s for v in t], dtype=np.float64).reshape(ksize, 1)


def _filter2d(img, ddepth, kernel):
    assert ddepth == -1 and img.dtype == np.float64 and img.ndim == 2
    kh, kw = kernel.shape
    H, W = img.shape
    out = np.zeros_like(img)
    vh, vw = H - kh + 1, W - kw + 1
    if vh > 0 and vw > 0:
        acc = np.zeros((vh, vw), dtype=np.float64)
        for i in range(kh):
            for j in range(kw):
                acc += kernel[i, j] * img[i:i + vh, j:j + vw]
        out[kh // 2:kh // 2 + vh, kw // 2:kw // 2 + vw] = acc
    return out


def install_cv2_standin():
    sys.modules["cv2"] = types.SimpleNamespace(getGaussianKernel=_gaussian_kernel, filter2D=_filter2d)


def load_reference_metrics():
    """(calculate_psnr module, calculate_ssim module) of the unmodified reference, loaded by file path."""
    if not rh.reference_available():
        raise RuntimeError(f"reference not found under {rh.REFERENCE_ROOT}")
    install_cv2_standin()
    d = os.path.join(rh.REFERENCE_ROOT, "evaluation", "common_metrics_on_video_quality")
    mods = []
    for name in ("calculate_psnr", "calculate_ssim"):
        spec = importlib.util.spec_from_file_location(f"_ref_{name}", os.path.join(d, name + ".py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        mods.append(m)
    return tuple(mods)


def _u8(rng, shape, lo=0, hi=256):
    return rng.integers(lo, hi, size=shape, dtype=np.uint8)


def _cases():
    """name -> dict(u8a, u8b) or dict(xa, xb)"""
    out = {}
    rng = np.random.default_rng(500)
    a = _u8(rng, (2, 5, 64, 96, 3))
    noise = rng.integers(-24, 25, size=a.shape)
    out["metrics_video"] = dict(u8a=a, u8b=np.clip(a.astype(np.int64) + noise, 0, 255).astype(np.uint8))
    a = _u8(rng, (2, 3, 37, 53, 3))
    out["metrics_odd"] = dict(u8a=a, u8b=np.clip(a.astype(np.int64) + rng.integers(-40, 41, size=a.shape), 0, 255)
                              .astype(np.uint8))
    a = _u8(rng, (2, 2, 11, 11, 3))
    out["metrics_11x11"] = dict(u8a=a, u8b=_u8(rng, a.shape))
    a = _u8(rng, (2, 2, 10, 12, 3))
    out["metrics_10x12"] = dict(u8a=a, u8b=_u8(rng, a.shape))
    a = _u8(rng, (3, 1, 48, 64, 3))
    out["metrics_image"] = dict(u8a=a, u8b=np.clip(a.astype(np.int64) + rng.integers(-8, 9, size=a.shape), 0, 255)
                                .astype(np.uint8))
    a = _u8(rng, (2, 3, 32, 40, 3))
    out["metrics_identical"] = dict(u8a=a, u8b=a.copy())
    a = _u8(rng, (2, 3, 32, 40, 3), 0, 200)
    out["metrics_offset"] = dict(u8a=a, u8b=a + np.uint8(17))
    out["metrics_noise"] = dict(u8a=_u8(rng, (2, 3, 32, 40, 3)), u8b=_u8(rng, (2, 3, 32, 40, 3)))
    g = torch.Generator().manual_seed(501)
    xa = (torch.rand(2, 3, 3, 24, 40, generator=g) - 0.5).numpy()
    xb = (torch.from_numpy(xa) + 0.35 * torch.randn(2, 3, 3, 24, 40, generator=g)).numpy()
    out["metrics_float"] = dict(xa=xa.astype(np.float32), xb=xb.astype(np.float32))
    return out


def videos_of(case):
    """the reference's [B,T,C,H,W] fp32 videos in [0, 1] of a fixture's inputs"""
    if "u8a" in case:
        return [torch.from_numpy(np.ascontiguousarray(case[k])).permute(0, 1, 4, 2, 3).float() / 255 for k in ("u8a", "u8b")]
    xa, xb = torch.from_numpy(case["xa"]), torch.from_numpy(case["xb"])
    real = xa + 0.5
    fake = torch.clamp(xb + 0.5, 0, 1)
    return [v.permute(0, 2, 1, 3, 4).contiguous() for v in (real, fake)]


def main():
    cp, cs = load_reference_metrics()
    total = 0
    for name, case in _cases().items():
        v1, v2 = videos_of(case)
        B, T = v1.shape[:2]
        psnr = np.array([[cp.img_psnr(v1[b, t].numpy(), v2[b, t].numpy()) for t in range(T)] for b in range(B)],
                        dtype=np.float64)
        ssim = np.array([[cs.calculate_ssim_function(v1[b, t].numpy(), v2[b, t].numpy()) for t in range(T)]
                         for b in range(B)], dtype=np.float64)
        rp, rs = cp.calculate_psnr(v1, v2), cs.calculate_ssim(v1, v2)
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **case, psnr=psnr, ssim=ssim,
                            psnr_value=np.array([rp["value"][t] for t in range(T)], dtype=np.float64),
                            psnr_std=np.array([rp["value_std"][t] for t in range(T)], dtype=np.float64),
                            ssim_value=np.array([rs["value"][t] for t in range(T)], dtype=np.float64),
                            ssim_std=np.array([rs["value_std"][t] for t in range(T)], dtype=np.float64))
        size = os.path.getsize(path)
        total += size
        print(f"{name}: videos {tuple(v1.shape)}, psnr {np.nanmin(psnr):.3f}..{np.nanmax(psnr):.3f}, "
              f"ssim {np.nanmin(ssim) if not np.isnan(ssim).all() else float('nan'):.4f}.., {size / 1e3:.0f} kB")
    print(f"total {total / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
