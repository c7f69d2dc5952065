"""Frames in, frames out: uint8 video frames <-> the fp32 pixels encode() reads and decode() writes.

The arithmetic is the reference's loaders and eval scripts (INTEGRATION.md "frames in, frames out"):

  frames_to_pixels(resize="none")      crop, u / 255, - 0.5: ToTensor + Normalize(0.5, 1.0), and with norm="videonorm" the
                                       reference's VideoNorm (video_utils.py:33-58: a clip with no byte > 1 is not divided)
  frames_to_pixels(resize="bilinear")  preprocess (data.py:305-350): u / 255, bilinear resize of the short side to
                                       `resolution` (align_corners=False), center crop, - 0.5
  pixels_to_frames                     (clamp(x + 0.5, 0, 1) * 255).byte() (vqgan_eval.py:141-148, utils.py:225-229)

  resize_frames / images_to_pixels     Pillow's Image.resize (bicubic, bilinear, box), byte for byte: torchvision's Resize
                                       on a PIL image, ImageDataset's transform (data.py:83-99)
  center_crop_arr                      the DiT / Latte loaders' preprocessing (Diffusion/DiT/train.py:92-110)

The first three run in csrc/frames.hip (include/omnitok.h omnitok_frames_to_pixels / omnitok_pixels_to_frames), the Pillow
resize in csrc/resize_pil.hip (omnitok_frames_resize_pil); they are registered as the operators omnitok::frames_to_pixels /
omnitok::pixels_to_frames / omnitok::frames_resize_pil with shape functions for torch.compile / export.
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
INTERPOLATIONS = {"bicubic": 0, "bilinear": 1, "box": 2}   # OMNITOK_RESIZE_BICUBIC / _BILINEAR / _BOX
RESIZE_OUT = {"pixels": 0, "uint8": 1}      # OMNITOK_RESIZE_OUT_PIXELS / _U8


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


def _output_length(clips, frame_start: int, sequence_length: Optional[int], sample_every_n_frames: int) -> int:
    """temporal crop and frame skip (data.py:312-318), per clip; the batch needs one output length"""
    if sample_every_n_frames < 1 or frame_start < 0:
        raise ValueError("sample_every_n_frames must be >= 1 and frame_start >= 0")
    f_outs = set()
    for c in clips:
        seq = c.shape[0] - frame_start if sequence_length is None else sequence_length
        if seq < 1 or frame_start + seq > c.shape[0]:
            raise ValueError(f"frames [{frame_start}, {frame_start + seq}) outside a clip of {c.shape[0]} frames")
        f_outs.add(len(range(0, seq, sample_every_n_frames)))
    if len(f_outs) != 1:
        raise ValueError(f"clips give different output lengths {sorted(f_outs)}: pass sequence_length")
    return f_outs.pop()


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
    F_out = _output_length(clips, frame_start, sequence_length, sample_every_n_frames)
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


def _pair(v, what: str) -> Tuple[int, int]:
    if isinstance(v, int) and not isinstance(v, bool):
        return v, v
    if isinstance(v, (tuple, list)) and len(v) == 2 and all(isinstance(x, int) and not isinstance(x, bool) for x in v):
        return int(v[0]), int(v[1])
    raise ValueError(f"{what} must be an int or (h, w), got {v!r}")


def resize_frames(frames: Union[torch.Tensor, Sequence[torch.Tensor]], size, is_image: bool = False, *,
                  interpolation: str = "bicubic", crop: Optional[Sequence[Tuple[int, int]]] = None, crop_size=None,
                  frame_start: int = 0, sequence_length: Optional[int] = None, sample_every_n_frames: int = 1,
                  out: str = "uint8") -> torch.Tensor:
    """Pillow's Image.resize((w, h), filter) of every frame, on the GPU and byte for byte (antialiased two-pass resampler,
    8-bit RGB; what torchvision's Resize((h, w)) does to a PIL image).  Lanczos is not covered.

    frames: as for frames_to_pixels: [B,F,H,W,3] (is_image: [B,H,W,3]) uint8, or a list of clips / images of different
        native sizes.
    size: (h, w), the size Pillow is asked for (an int s means (s, s)); or one (h, w) per clip.
    interpolation: "bicubic", "bilinear" or "box".
    crop, crop_size: one (top, left) per clip and the window's size (an int or (h, w)): the window of the RESIZED frame that
        is returned (RandomCrop / a center crop after the resize).  Without them the whole resized frame is returned, and
        all clips must then be resized to one size.
    frame_start / sequence_length / sample_every_n_frames: as for frames_to_pixels.
    out: "uint8" -> [B,(F,)h,w,3] uint8, Pillow's bytes; "pixels" -> [B,3,(F,)h,w] fp32 = u / 255 - 0.5, bit-identical to
        ToTensor + Normalize(0.5, 1.0) of them (what encode() reads)."""
    if interpolation not in INTERPOLATIONS:
        raise ValueError(f"interpolation must be one of {sorted(INTERPOLATIONS)}, got {interpolation!r} (Pillow's other "
                         "filters, Lanczos among them, are not covered)")
    if out not in RESIZE_OUT:
        raise ValueError(f"out must be one of {sorted(RESIZE_OUT)}, got {out!r}")
    clips = _clip_list(frames, is_image)
    B = len(clips)
    F_out = _output_length(clips, frame_start, sequence_length, sample_every_n_frames)
    if isinstance(size, (list, tuple)) and len(size) > 0 and isinstance(size[0], (list, tuple)):
        if len(size) != B:
            raise ValueError(f"size: {len(size)} sizes for {B} clips")
        sizes = [_pair(s, "size") for s in size]
    else:
        sizes = [_pair(size, "size")] * B
    if any(h < 1 or w < 1 for h, w in sizes):
        raise ValueError(f"size must be at least 1 x 1, got {sorted(set(sizes))}")
    if (crop is None) != (crop_size is None):
        raise ValueError("crop (one (top, left) per clip) and crop_size go together")
    if crop is None:
        if len(set(sizes)) != 1:
            raise ValueError(f"clips resized to different sizes {sorted(set(sizes))}: pass crop and crop_size")
        R_h, R_w = sizes[0]
        crop = [(0, 0)] * B
    else:
        R_h, R_w = _pair(crop_size, "crop_size")
        if len(crop) != B:
            raise ValueError(f"crop: {len(crop)} offsets for {B} clips")
    geom = []
    for i, ((h, w), (top, left)) in enumerate(zip(sizes, crop)):
        top, left = int(top), int(left)
        if R_h < 1 or R_w < 1 or top < 0 or left < 0 or top + R_h > h or left + R_w > w:
            raise ValueError(f"clip {i}: crop window {R_h}x{R_w} at ({top}, {left}) outside the {h}x{w} resized frame")
        geom += [frame_start, sample_every_n_frames, top, left, h, w]
    with torch.cuda.device(clips[0].device):
        y = torch.ops.omnitok.frames_resize_pil(clips, geom, F_out, R_h, R_w, INTERPOLATIONS[interpolation], RESIZE_OUT[out])
    if is_image:
        return y[:, 0] if out == "uint8" else y[:, :, 0]
    return y


def images_to_pixels(images: Union[torch.Tensor, Sequence[torch.Tensor]], resolution: int, *, interpolation: str = "bicubic",
                     resize_to: Optional[int] = None, crop: Optional[Sequence[Tuple[int, int]]] = None) -> torch.Tensor:
    """The reference's ImageDataset transform (data.py:83-99) on uint8 images on the GPU ([B,H,W,3] or a list of [H,W,3] of
    different sizes) -> fp32 [B,3,R,R] in [-0.5, 0.5], bit-identical to Resize + ToTensor + Normalize(0.5, 1.0) on PIL images.
      evaluation:          Resize((R, R), bicubic)
      train `resizecrop`:  resize_to=int(R * 1.5), crop = the (top, left) offsets RandomCrop(R) drew, one per image."""
    if not isinstance(resolution, int) or resolution < 1:
        raise ValueError(f"resolution must be a positive int, got {resolution!r}")
    if resize_to is None:
        if crop is not None:
            raise ValueError("crop applies to the resizecrop transform: pass resize_to")
        return resize_frames(images, (resolution, resolution), True, interpolation=interpolation, out="pixels")
    if crop is None:
        raise ValueError("resize_to needs crop: the (top, left) offsets of RandomCrop, one per image")
    return resize_frames(images, (resize_to, resize_to), True, interpolation=interpolation, crop=crop, crop_size=resolution,
                         out="pixels")


def center_crop_arr(images: Union[torch.Tensor, Sequence[torch.Tensor]], image_size: int) -> torch.Tensor:
    """The DiT / Latte loaders' center_crop_arr (Diffusion/DiT/train.py:92-110, Latte/datasets/video_transforms.py:16-34) on
    uint8 images on the GPU ([B,H,W,3] or a list of [H,W,3]) -> uint8 [B,S,S,3], Pillow's bytes: while the short side is at
    least 2 * S a BOX resize to (w // 2, h // 2), then a BICUBIC resize to round(side * S / short side) (Python's round, on
    the sizes after the halvings), then the center crop at ((h - S) // 2, (w - S) // 2)."""
    if not isinstance(image_size, int) or image_size < 1:
        raise ValueError(f"image_size must be a positive int, got {image_size!r}")
    imgs = [c[0] for c in _clip_list(images, True)]
    sizes, crops = [], []
    for i, img in enumerate(imgs):
        while min(img.shape[0], img.shape[1]) >= 2 * image_size:
            img = resize_frames([img], (img.shape[0] // 2, img.shape[1] // 2), True, interpolation="box")[0]
        imgs[i] = img
        scale = image_size / min(img.shape[0], img.shape[1])
        h, w = round(img.shape[0] * scale), round(img.shape[1] * scale)
        sizes.append((h, w))
        crops.append(((h - image_size) // 2, (w - image_size) // 2))
    return resize_frames(imgs, sizes, True, interpolation="bicubic", crop=crops, crop_size=image_size)


def _descs(clips, geom):
    descs = (OmnitokFramesDesc * len(clips))()
    for i, c in enumerate(clips):
        d = descs[i]
        d.frames = c.data_ptr()
        d.frame_stride, d.row_stride = c.stride(0), c.stride(1)
        d.F, d.H, d.W = c.shape[0], c.shape[1], c.shape[2]
        (d.frame_start, d.frame_step, d.crop_top, d.crop_left, d.resize_h, d.resize_w) = geom[_GEOM * i:_GEOM * (i + 1)]
    return descs


def _frames_resize_pil_native(clips, geom, F_out, R_h, R_w, filt, out_kind):
    B = len(clips)
    descs = _descs(clips, geom)
    lib = _lib.load()
    need = check(lib.omnitok_frames_resize_pil_workspace(descs, B, F_out, filt), "frames_resize_pil_workspace")
    dev = clips[0].device
    work = torch.empty(max(need, 16), device=dev, dtype=torch.uint8)
    out = torch.empty((B, 3, F_out, R_h, R_w), device=dev, dtype=torch.float32) if out_kind == 0 else \
        torch.empty((B, F_out, R_h, R_w, 3), device=dev, dtype=torch.uint8)
    check(lib.omnitok_frames_resize_pil(descs, B, F_out, R_h, R_w, filt, out_kind, ctypes.c_void_p(work.data_ptr()),
                                        work.numel(), ctypes.c_void_p(out.data_ptr()),
                                        torch.cuda.current_stream().cuda_stream), "frames_resize_pil")
    return out


def _frames_to_pixels_native(clips, geom, F_out, R_h, R_w, mode, flags):
    B = len(clips)
    descs = _descs(clips, geom)
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

    @custom_op("omnitok::frames_resize_pil", mutates_args=(), device_types="cuda")
    def _frp(clips: List[torch.Tensor], geom: List[int], F_out: int, R_h: int, R_w: int, filt: int,
             out_kind: int) -> torch.Tensor:
        if len(geom) != _GEOM * len(clips):
            raise ValueError(f"geom: {len(geom)} values for {len(clips)} clips")
        return _frames_resize_pil_native(clips, geom, F_out, R_h, R_w, filt, out_kind)

    @_frp.register_fake
    def _(clips, geom, F_out, R_h, R_w, filt, out_kind):
        if out_kind == 0:
            return clips[0].new_empty((len(clips), 3, F_out, R_h, R_w), dtype=torch.float32)
        return clips[0].new_empty((len(clips), F_out, R_h, R_w, 3), dtype=torch.uint8)

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
