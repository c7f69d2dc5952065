"""Frames in, frames out: uint8 video frames <-> the fp32 pixels encode() reads and decode() writes.

The arithmetic is the reference's loaders and eval scripts (INTEGRATION.md "frames in, frames out"):

  frames_to_pixels(resize="none")      crop, u / 255, - 0.5: ToTensor + Normalize(0.5, 1.0), and with norm="videonorm" the
                                       reference's VideoNorm (video_utils.py:33-58: a clip with no byte > 1 is not divided)
  frames_to_pixels(resize="bilinear")  preprocess (data.py:305-350): u / 255, bilinear resize of the short side to
                                       `resolution` (align_corners=False), center crop, - 0.5
  pixels_to_frames                     (clamp(x + 0.5, 0, 1) * 255).byte() (vqgan_eval.py:141-148, utils.py:225-229)

Both run in csrc/frames.hip (include/omnitok.h omnitok_frames_to_pixels / omnitok_pixels_to_frames) and are registered as
the operators omnitok::frames_to_pixels / omnitok::pixels_to_frames with shape functions for torch.compile / export.
"""
from __future__ import annotations

import ctypes
import math
from typing import List, Optional, Sequence, Tuple, Union

import torch

from . import _lib
from ._lib import OmnitokFramesDesc, check

RESIZE_MODES = {"none": 0, "bilinear": 1}   # OMNITOK_FRAMES_NONE / _BILINEAR
LAYOUTS = {"thwc": 0, "cthw": 1}            # OMNITOK_LAYOUT_THWC / _CTHW
FLAG_VIDEONORM = 1                          # OMNITOK_FRAMES_VIDEONORM
_GEOM = 6                                   # per clip: frame_start, frame_step, crop_top, crop_left, resize_h, resize_w


def preprocess_size(h: int, w: int, resolution: int) -> Tuple[int, int]:
    """The resized (h, w) of the reference's preprocess (data.py:320-326): short side `resolution`, the long side
    math.ceil(long * (resolution / short)) in double precision."""
    scale = resolution / min(h, w)
    if h < w:
        return resolution, math.ceil(w * scale)
    return math.ceil(h * scale), resolution


def _clip_list(frames, is_image: bool) -> List[torch.Tensor]:
    """[F, H, W, 3] uint8 CUDA views, one per clip, channels interleaved with a 3-byte pixel stride."""
    if isinstance(frames, torch.Tensor):
        want = 4 if is_image else 5
        if frames.dim() != want:
            raise ValueError(f"frames must be [B,{'' if is_image else 'F,'}H,W,3] uint8 (is_image={is_image}), got shape "
                             f"{tuple(frames.shape)}")
        clips = list(frames.unbind(0))
    elif isinstance(frames, (list, tuple)):
        clips = list(frames)
    else:
        raise TypeError(f"frames must be a uint8 CUDA tensor or a list of them, got {type(frames).__name__}")
    out = []
    for i, c in enumerate(clips):
        if not isinstance(c, torch.Tensor):
            raise TypeError(f"clip {i}: not a tensor")
        if c.dtype != torch.uint8:
            raise TypeError(f"clip {i}: dtype {c.dtype}, expected torch.uint8")
        if c.dim() != (3 if is_image else 4) or c.shape[-1] != 3 or c.numel() == 0:
            raise ValueError(f"clip {i}: shape {tuple(c.shape)}, expected [{'' if is_image else 'F,'}H,W,3]")
        if c.device.type != "cuda":
            raise RuntimeError(f"clip {i} is on {c.device}: frames must be on the GPU (there is no CPU path)")
        if is_image:
            c = c.unsqueeze(0)
        if c.stride(-1) != 1 or c.stride(-2) != 3 or min(c.stride()) < 0:
            c = c.contiguous()
        out.append(c)
    if not out:
        raise ValueError("no clips")
    if len({c.device for c in out}) != 1:
        raise RuntimeError("all clips must be on one GPU")
    return out


def frames_to_pixels(frames: Union[torch.Tensor, Sequence[torch.Tensor]], is_image: bool = False, *, resize: str = "none",
                     norm: Optional[str] = None, resolution: Union[None, int, Tuple[int, int]] = None,
                     crop: Optional[Sequence[Tuple[int, int]]] = None, frame_start: int = 0,
                     sequence_length: Optional[int] = None, sample_every_n_frames: int = 1) -> torch.Tensor:
    """uint8 frames on the GPU -> fp32 pixels in [-0.5, 0.5]: [B,3,F_out,R,R] (videos) or [B,3,R,R] (is_image).

    frames: [B,F,H,W,3] (is_image: [B,H,W,3]) or a list of per-clip [F,H,W,3] ([H,W,3]) tensors of different native sizes.
    resize: "none" (crop only) or "bilinear" (the reference's preprocess; `resolution` is then required).
    norm: "videonorm" (the default of resize="none": VideoNorm, a clip with no cropped byte > 1 is not divided by 255) or
        "totensor" (always u / 255); resize="bilinear" always divides.
    resolution: side of the square output (resize="none": an int or (R_h, R_w), None = the whole frame).
    crop: None (center) or one (top, left) per clip, in the source (resize="none") or the resized frame ("bilinear").
    frame_start / sequence_length / sample_every_n_frames: source frames frame_start + k * n for k * n < sequence_length
        (default: to the last frame), preprocess's temporal crop and frame skip."""
    if resize not in RESIZE_MODES:
        raise ValueError(f"resize must be one of {sorted(RESIZE_MODES)}, got {resize!r}")
    if norm not in (None, "videonorm", "totensor"):
        raise ValueError(f"norm must be 'videonorm' or 'totensor', got {norm!r}")
    if resize == "bilinear" and norm == "videonorm":
        raise ValueError("norm='videonorm' applies to resize='none' (preprocess always divides by 255)")
    clips = _clip_list(frames, is_image)
    B = len(clips)
    if sample_every_n_frames < 1 or frame_start < 0:
        raise ValueError("sample_every_n_frames must be >= 1 and frame_start >= 0")
    # temporal crop and frame skip (data.py:312-318), per clip; the batch needs one output length
    f_outs = set()
    for c in clips:
        seq = c.shape[0] - frame_start if sequence_length is None else sequence_length
        if seq < 1 or frame_start + seq > c.shape[0]:
            raise ValueError(f"frames [{frame_start}, {frame_start + seq}) outside a clip of {c.shape[0]} frames")
        f_outs.add(len(range(0, seq, sample_every_n_frames)))
    if len(f_outs) != 1:
        raise ValueError(f"clips give different output lengths {sorted(f_outs)}: pass sequence_length")
    F_out = f_outs.pop()
    geom = []
    if resize == "bilinear":
        if resolution is None or not isinstance(resolution, int):
            raise ValueError("resize='bilinear' needs an int resolution (the output is resolution x resolution)")
        R_h = R_w = resolution
        for c in clips:
            rh, rw = preprocess_size(c.shape[1], c.shape[2], resolution)
            geom.append([frame_start, sample_every_n_frames, (rh - resolution) // 2, (rw - resolution) // 2, rh, rw])
    else:
        if resolution is None:
            sizes = {(c.shape[1], c.shape[2]) for c in clips}
            if len(sizes) != 1:
                raise ValueError(f"clips of different sizes {sorted(sizes)}: pass resolution (the crop size)")
            R_h, R_w = sizes.pop()
        else:
            R_h, R_w = (resolution, resolution) if isinstance(resolution, int) else tuple(resolution)
        for c in clips:
            geom.append([frame_start, sample_every_n_frames, (c.shape[1] - R_h) // 2, (c.shape[2] - R_w) // 2, 0, 0])
    if crop is not None:
        if len(crop) != B:
            raise ValueError(f"crop: {len(crop)} offsets for {B} clips")
        for g, (top, left) in zip(geom, crop):
            g[2], g[3] = int(top), int(left)
    flags = FLAG_VIDEONORM if (resize == "none" and norm in (None, "videonorm")) else 0
    with torch.cuda.device(clips[0].device):
        x = torch.ops.omnitok.frames_to_pixels(clips, [v for g in geom for v in g], F_out, R_h, R_w, RESIZE_MODES[resize],
                                               flags)
    return x[:, :, 0] if is_image else x


def pixels_to_frames(pixels: torch.Tensor, layout: str = "thwc") -> torch.Tensor:
    """fp32 pixels on the GPU -> uint8, (clamp(x + 0.5, 0, 1) * 255) truncated, non-finite values -> 0.
    [B,3,F,H,W] -> [B,F,H,W,3] ("thwc") or [B,3,F,H,W] ("cthw"); images [B,3,H,W] -> [B,H,W,3] or [B,3,H,W]."""
    if layout not in LAYOUTS:
        raise ValueError(f"layout must be one of {sorted(LAYOUTS)}, got {layout!r}")
    if not isinstance(pixels, torch.Tensor):
        raise TypeError("pixels must be a tensor")
    if pixels.dtype != torch.float32:
        raise TypeError(f"pixels: dtype {pixels.dtype}, expected torch.float32")
    if pixels.dim() not in (4, 5) or pixels.shape[1] != 3:
        raise ValueError(f"pixels must be [B,3,H,W] or [B,3,F,H,W], got shape {tuple(pixels.shape)}")
    if pixels.device.type != "cuda":
        raise RuntimeError(f"pixels are on {pixels.device}: they must be on the GPU (there is no CPU path)")
    image = pixels.dim() == 4
    x5 = pixels[:, :, None] if image else pixels
    with torch.cuda.device(pixels.device):
        out = torch.ops.omnitok.pixels_to_frames(x5, LAYOUTS[layout])
    if image:
        out = out[:, 0] if layout == "thwc" else out[:, :, 0]
    return out


def _frames_to_pixels_native(clips, geom, F_out, R_h, R_w, mode, flags):
    B = len(clips)
    descs = (OmnitokFramesDesc * B)()
    for i, c in enumerate(clips):
        d = descs[i]
        d.frames = c.data_ptr()
        d.frame_stride, d.row_stride = c.stride(0), c.stride(1)
        d.F, d.H, d.W = c.shape[0], c.shape[1], c.shape[2]
        (d.frame_start, d.frame_step, d.crop_top, d.crop_left, d.resize_h, d.resize_w) = geom[_GEOM * i:_GEOM * (i + 1)]
    out = torch.empty(B, 3, F_out, R_h, R_w, device=clips[0].device, dtype=torch.float32)
    work = torch.empty(B, device=clips[0].device, dtype=torch.int32) if flags & FLAG_VIDEONORM else None
    check(_lib.load().omnitok_frames_to_pixels(descs, B, F_out, R_h, R_w, mode, flags,
                                               None if work is None else ctypes.c_void_p(work.data_ptr()),
                                               ctypes.c_void_p(out.data_ptr()), torch.cuda.current_stream().cuda_stream),
          "frames_to_pixels")
    return out


def _register_ops():
    from torch.library import custom_op

    @custom_op("omnitok::frames_to_pixels", mutates_args=(), device_types="cuda")
    def _f2p(clips: List[torch.Tensor], geom: List[int], F_out: int, R_h: int, R_w: int, mode: int,
             flags: int) -> torch.Tensor:
        if len(geom) != _GEOM * len(clips):
            raise ValueError(f"geom: {len(geom)} values for {len(clips)} clips")
        return _frames_to_pixels_native(clips, geom, F_out, R_h, R_w, mode, flags)

    @_f2p.register_fake
    def _(clips, geom, F_out, R_h, R_w, mode, flags):
        return clips[0].new_empty((len(clips), 3, F_out, R_h, R_w), dtype=torch.float32)

    @custom_op("omnitok::pixels_to_frames", mutates_args=(), device_types="cuda")
    def _p2f(pixels: torch.Tensor, layout: int) -> torch.Tensor:
        x = pixels.contiguous()
        B, C, F, H, W = x.shape
        out = torch.empty((B, F, H, W, C) if layout == 0 else (B, C, F, H, W), device=x.device, dtype=torch.uint8)
        check(_lib.load().omnitok_pixels_to_frames(ctypes.c_void_p(x.data_ptr()), B, C, F, H, W, layout,
                                                   ctypes.c_void_p(out.data_ptr()), torch.cuda.current_stream().cuda_stream),
              "pixels_to_frames")
        return out

    @_p2f.register_fake
    def _(pixels, layout):
        B, C, F, H, W = pixels.shape
        return pixels.new_empty((B, F, H, W, C) if layout == 0 else (B, C, F, H, W), dtype=torch.uint8)


_register_ops()
