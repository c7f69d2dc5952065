"""Reconstruction metrics on the device: PSNR and SSIM of every (clip, frame), with the arithmetic of the reference's
evaluation/common_metrics_on_video_quality (INTEGRATION.md "reconstruction metrics"):

  psnr_ssim(a, b, layout)           (psnr [B,F], ssim [B,F]) fp64 on the device; operands are read in place through their
                                    strides: "btchw" (the reference's layout), "bcthw" (the tokenizer's pixels), "bthwc"
                                    (the uint8 frames of encode_frames / decode_frames), 4-D images as one frame
  calculate_psnr / calculate_ssim   drop-ins for calculate_psnr.py / calculate_ssim.py: the same result dicts, per-timestamp
                                    mean and population std over the batch (in torch fp64)
  OmniTokenizer_VQGAN.reconstruction_metrics   vqgan_eval.py's real = x + 0.5, fake = clamp(x_recon + 0.5, 0, 1), fused into
                                    the operand reads

fp32 operands are values in [0, 1]; uint8 operands are u / 255.  PSNR: 100 if mse < 1e-10, else 20 log10(1 / sqrt(mse)), the
mse of the whole 3 x H x W frame (img_psnr).  SSIM: the 11 x 11 Gaussian window (sigma 1.5) over the valid region, C1 = 0.01^2,
C2 = 0.03^2, the mean of the three channels (calculate_ssim_function); NaN when H < 11 or W < 11.  Runs in csrc/metrics.hip
(include/omnitok.h omnitok_frame_metrics), registered as the operator omnitok::frame_metrics with a shape function.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Tuple

import torch

from . import _lib
from ._lib import OmnitokMetricsOperand, check

LAYOUTS = ("btchw", "bcthw", "bthwc")
FLAG_PSNR, FLAG_SSIM = 1, 2                           # OMNITOK_METRICS_PSNR / _SSIM
_DTYPES = {torch.float32: 0, torch.uint8: 1}          # OMNITOK_METRICS_F32 / _U8
_PERM = {"btchw": (0, 1, 2, 3, 4), "bcthw": (0, 2, 1, 3, 4), "bthwc": (0, 1, 4, 2, 3)}   # layout -> (b, t, c, h, w)
_FRAME_AXIS = {"btchw": 1, "bcthw": 2, "bthwc": 1}    # where a 4-D image gets its frame axis of size 1


def _as_btchw(x, layout: str, name: str) -> torch.Tensor:
    """x in `layout` -> a [B,F,3,H,W] view of it (no copy)"""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name} must be a tensor, got {type(x).__name__}")
    if x.dtype not in _DTYPES:
        raise TypeError(f"{name}: dtype {x.dtype}, expected torch.float32 (values in [0, 1]) or torch.uint8")
    if x.dim() == 4:
        x = x.unsqueeze(_FRAME_AXIS[layout])
    elif x.dim() != 5:
        raise ValueError(f"{name} must be a 5-D video or a 4-D image in layout {layout!r}, got shape {tuple(x.shape)}")
    v = x.permute(_PERM[layout])
    if v.shape[2] != 3:
        raise ValueError(f"{name}: {v.shape[2]} channels in layout {layout!r}, expected 3 (shape {tuple(x.shape)})")
    return v


def _operands(a, b, layout: str) -> Tuple[torch.Tensor, torch.Tensor]:
    if layout not in LAYOUTS:
        raise ValueError(f"layout must be one of {list(LAYOUTS)}, got {layout!r}")
    va, vb = _as_btchw(a, layout, "a"), _as_btchw(b, layout, "b")
    if va.shape != vb.shape:
        raise ValueError(f"a and b differ in shape: {tuple(a.shape)} vs {tuple(b.shape)}")
    for name, v in (("a", va), ("b", vb)):
        if v.device.type != "cuda":
            raise RuntimeError(f"{name} is on {v.device}: the metrics run on the GPU (there is no CPU path)")
    if va.device != vb.device:
        raise RuntimeError(f"a on {va.device}, b on {vb.device}: both must be on one GPU")
    return va, vb


def _scores(va, vb, flags: int, shift_a: float = 0.0, clamp_a: bool = False, shift_b: float = 0.0,
            clamp_b: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    with torch.cuda.device(va.device):
        return torch.ops.omnitok.frame_metrics(va, vb, float(shift_a), bool(clamp_a), float(shift_b), bool(clamp_b), flags)


def psnr_ssim(a: torch.Tensor, b: torch.Tensor, layout: str = "btchw") -> Tuple[torch.Tensor, torch.Tensor]:
    """(psnr, ssim), each [B, F] float64 on the device, of two videos of equal shape on one GPU.

    layout: "btchw" [B,F,3,H,W] (the reference's), "bcthw" [B,3,F,H,W] (encode's input, decode's output), "bthwc"
        [B,F,H,W,3]; a 4-D tensor is an image ([B,3,H,W] / [B,H,W,3]) and gives F = 1.
    dtype: float32 (values in [0, 1]) or uint8 (u / 255); a and b may differ.  Any strides: a view is copied only if its
        stride along w is not 1 or 3."""
    va, vb = _operands(a, b, layout)
    return _scores(va, vb, FLAG_PSNR | FLAG_SSIM)


def reconstruction_psnr_ssim(x: torch.Tensor, x_recon: torch.Tensor, is_image: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """psnr_ssim of vqgan_eval.py's pair (lines 141-148): real = x + 0.5, fake = torch.clamp(x_recon + 0.5, 0, 1), both
    computed in fp32 inside the kernel's reads.  x, x_recon: fp32 [B,3,F,H,W] ([B,3,H,W] with is_image) in the model's
    [-0.5, 0.5] convention."""
    want = 4 if is_image else 5
    for name, t in (("x", x), ("x_recon", x_recon)):
        if isinstance(t, torch.Tensor) and t.dim() != want:
            raise ValueError(f"{name} must be [B,3,{'' if is_image else 'F,'}H,W] (is_image={is_image}), got shape "
                             f"{tuple(t.shape)}")
        if isinstance(t, torch.Tensor) and t.dtype != torch.float32:
            raise TypeError(f"{name}: dtype {t.dtype}, expected torch.float32")
    va, vb = _operands(x, x_recon, "bcthw")
    return _scores(va, vb, FLAG_PSNR | FLAG_SSIM, 0.5, False, 0.5, True)


def _reference_dict(videos1, videos2, flag: int) -> Dict:
    if not isinstance(videos1, torch.Tensor) or not isinstance(videos2, torch.Tensor):
        raise TypeError("videos1 and videos2 must be tensors")
    if videos1.shape != videos2.shape:
        raise ValueError(f"videos1 and videos2 differ in shape: {tuple(videos1.shape)} vs {tuple(videos2.shape)}")
    for name, v in (("videos1", videos1), ("videos2", videos2)):
        if v.dtype != torch.float32:
            raise TypeError(f"{name}: dtype {v.dtype}, expected torch.float32 values in [0, 1]")
        if v.dim() != 5 or v.shape[0] == 0:
            raise ValueError(f"{name} must be [batch, time, 3, h, w] with batch >= 1, got shape {tuple(v.shape)}")
    va, vb = _operands(videos1, videos2, "btchw")
    psnr, ssim = _scores(va, vb, flag)
    v = psnr if flag == FLAG_PSNR else ssim
    mean, std = v.mean(0).tolist(), v.std(0, correction=0).tolist()
    return {"value": dict(enumerate(mean)), "value_std": dict(enumerate(std)), "video_setting": videos1.shape[1:],
            "video_setting_name": "time, channel, heigth, width"}


def calculate_psnr(videos1: torch.Tensor, videos2: torch.Tensor) -> Dict:
    """The reference's calculate_psnr (calculate_psnr.py) on the device: videos [batch, time, 3, h, w] fp32 in [0, 1] on one
    GPU -> {"value": {t: mean over the batch}, "value_std": {t: population std}, "video_setting": (time, channel, h, w),
    "video_setting_name": ...}, the reference's keys and strings."""
    return _reference_dict(videos1, videos2, FLAG_PSNR)


def calculate_ssim(videos1: torch.Tensor, videos2: torch.Tensor) -> Dict:
    """The reference's calculate_ssim (calculate_ssim.py) on the device; arguments and result as calculate_psnr."""
    return _reference_dict(videos1, videos2, FLAG_SSIM)


def _operand_desc(v: torch.Tensor, shift: float, clamp: bool) -> OmnitokMetricsOperand:
    d = OmnitokMetricsOperand()
    d.data = v.data_ptr()
    for k in range(5):   # a dimension of size 1 is never stepped along: its stride is whatever the view says
        d.stride[k] = v.stride(k) if v.shape[k] > 1 else (1 if k == 4 else 0)
    d.dtype = _DTYPES[v.dtype]
    d.clamp = int(clamp)
    d.shift = shift
    return d


def _frame_metrics_native(a, b, shift_a, clamp_a, shift_b, clamp_b, flags):
    B, F, C, H, W = a.shape
    views = []
    for v in (a, b):
        if v.shape[4] > 1 and v.stride(4) not in (1, 3) or min(v.stride()) < 0:
            v = v.contiguous()
        views.append(v)
    a, b = views
    lib = _lib.load()
    dev = a.device
    nan = float("nan")
    psnr = torch.empty((B, F), device=dev, dtype=torch.float64) if flags & FLAG_PSNR else torch.full((B, F), nan, device=dev,
                                                                                                       dtype=torch.float64)
    ssim = torch.empty((B, F), device=dev, dtype=torch.float64) if flags & FLAG_SSIM else torch.full((B, F), nan, device=dev,
                                                                                                       dtype=torch.float64)
    if B == 0:
        return psnr, ssim
    need = lib.omnitok_frame_metrics_workspace(B, F, H, W)
    if need < 0:
        raise ValueError(f"frame_metrics: bad shape {tuple(a.shape)}")
    work = torch.empty(max(need, 1), device=dev, dtype=torch.uint8)
    da, db = _operand_desc(a, shift_a, clamp_a), _operand_desc(b, shift_b, clamp_b)
    check(lib.omnitok_frame_metrics(ctypes.byref(da), ctypes.byref(db), B, F, H, W, flags,
                                    ctypes.c_void_p(psnr.data_ptr()) if flags & FLAG_PSNR else None,
                                    ctypes.c_void_p(ssim.data_ptr()) if flags & FLAG_SSIM else None,
                                    ctypes.c_void_p(work.data_ptr()), need, torch.cuda.current_stream().cuda_stream),
          "frame_metrics")
    return psnr, ssim


def _register_ops():
    from torch.library import custom_op

    @custom_op("omnitok::frame_metrics", mutates_args=(), device_types="cuda")
    def _fm(a: torch.Tensor, b: torch.Tensor, shift_a: float, clamp_a: bool, shift_b: float, clamp_b: bool,
            flags: int) -> Tuple[torch.Tensor, torch.Tensor]:
        if a.dim() != 5 or a.shape != b.shape or a.shape[2] != 3:
            raise ValueError(f"frame_metrics: a {tuple(a.shape)} and b {tuple(b.shape)} must be equal [B,F,3,H,W]")
        return _frame_metrics_native(a, b, shift_a, clamp_a, shift_b, clamp_b, flags)

    @_fm.register_fake
    def _(a, b, shift_a, clamp_a, shift_b, clamp_b, flags):
        B, F = a.shape[0], a.shape[1]
        return a.new_empty((B, F), dtype=torch.float64), a.new_empty((B, F), dtype=torch.float64)


_register_ops()
