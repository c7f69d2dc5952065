"""What the convolutional metric networks share (i3d.py for FVD, inception.py for FID, lpips.py for LPIPS; none of them
imports another): the operators over csrc/convnet_common.h's implicit-GEMM convolution and the pools beside it, and the
scaffold that turns a reference state_dict into packed device weights.

  operators   conv3d_same, maxpool3d_same (csrc/i3d.hip: TF "same" padding, zeros) on channels-last [B, T, H, W, C];
              conv2d, maxpool2d (-inf padding), avgpool2d, spatial_mean (csrc/inception.hip: explicit padding, floor sizing)
              on channels-last [N, H, W, C]; each a torch custom op `omnitok::<name>`.  A conv reads a channel slice of its
              input and writes channel slices of one or two outputs, so a network's concats cost nothing.
  weights     fold_bn (BatchNorm into its conv, in fp64), pack_conv_weight (the layout both convs read),
              check_state_dict (the strict key and shape check) and PackedWeights, the torch.nn.Module base that holds the
              state_dict on the host and packs it once per device.
A new network supplies its layer plan, its state_spec, `_held` (check and rename the keys) and `_pack`.
"""
from __future__ import annotations

import ctypes
from collections import OrderedDict
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import OmnitokConv2d, OmnitokConv3d, check, ptr, stream


def same_pad(s: int, k: int, stride: int) -> Tuple[int, int]:
    """(front pad, output extent) of Unit3D.compute_pad / MaxPool3dSamePadding.compute_pad (include/omnitok.h)"""
    pad = max(k - (s % stride or stride), 0)
    return pad // 2, (s + pad - k) // stride + 1


def out_size(s: int, k: int, stride: int, pad: int) -> int:
    """floor((s + 2 pad - k) / stride) + 1, 0 where the window does not fit (omnitok_conv2d_out)"""
    span = s + 2 * pad - k
    return span // stride + 1 if span >= 0 else 0


def _grid3d(shape, kernel, stride):
    return (shape[0],) + tuple(same_pad(e, k, s)[1] for e, k, s in zip(shape[1:4], kernel, stride))


def _grid2d(shape, kernel, stride, padding):
    return (shape[0],) + tuple(out_size(e, k, s, p) for e, k, s, p in zip(shape[1:3], kernel, stride, padding))


# ---- the operators ------------------------------------------------------------------------------------------------------

_LAYOUT = {5: "[B, T, H, W, C]", 4: "[N, H, W, C]"}


def _conv_desc(what, desc, ndim, grid, geometry, x, x_off, cin, w, bias, relu, y, y_off, y2, y2_off, split):
    """Checks the tensors of a conv op on channels-last tensors of `ndim` axes (grid(x.shape, *geometry) is the output grid)
    and returns a `desc` with the fields that omnitok_conv3d and omnitok_conv2d_desc share filled in"""
    for name, t in (("x", x), ("w", w), ("bias", bias), ("y", y), ("y2", y2)):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise ValueError(f"{what}: {name} must be a contiguous float32 tensor")
    if x.dim() != ndim or y.dim() != ndim or (y2 is not None and y2.dim() != ndim):
        raise ValueError(f"{what}: x, y and y2 are channels-last {_LAYOUT[ndim]}")
    want = grid(x.shape, *geometry)
    for name, t in (("y", y), ("y2", y2)):
        if t is not None and tuple(t.shape[:-1]) != want:
            raise ValueError(f"{what}: {name} is {tuple(t.shape)}, the output grid is {want}")
    d = desc()
    d.x, d.x_cs, d.x_off, d.Cin = x.data_ptr(), x.shape[-1], x_off, cin
    d.w, d.bias, d.Cout = w.data_ptr(), bias.data_ptr(), w.shape[0]
    d.relu = int(relu)
    d.y, d.y_cs, d.y_off = y.data_ptr(), y.shape[-1], y_off
    if y2 is not None:
        d.y2, d.y2_cs, d.y2_off = y2.data_ptr(), y2.shape[-1], y2_off
    d.split = split
    return d


def _conv_front(op, grid, geometry, x, w_packed, bias, relu, cin, x_off, out, out_off, out2, out2_off, split):
    """the defaults of conv3d_same and conv2d: every channel from x_off, no split, a new `out` of the output grid"""
    cin = x.shape[-1] - x_off if cin is None else cin
    split = w_packed.shape[0] if split is None else split
    if out is None:
        out = torch.empty(grid(x.shape, *geometry) + (split,), device=x.device, dtype=torch.float32)
    op(x, x_off, cin, w_packed, bias, *geometry, relu, out, out_off, out2, out2_off, split)
    return out


def _register_ops():
    from torch.library import custom_op

    @custom_op("omnitok::conv3d_same", mutates_args=("y", "y2"), device_types="cuda")
    def _conv3d(x: torch.Tensor, x_off: int, cin: int, w: torch.Tensor, bias: torch.Tensor, kernel: List[int],
                stride: List[int], relu: bool, y: torch.Tensor, y_off: int, y2: Optional[torch.Tensor], y2_off: int,
                split: int) -> None:
        d = _conv_desc("conv3d_same", OmnitokConv3d, 5, _grid3d, (kernel, stride), x, x_off, cin, w, bias,
                       relu, y, y_off, y2, y2_off, split)
        d.B, d.T, d.H, d.W = x.shape[:4]
        d.kt, d.kh, d.kw = kernel
        d.st, d.sh, d.sw = stride
        check(_lib.load().omnitok_conv3d_same(ctypes.byref(d), stream()), "conv3d_same")

    @_conv3d.register_fake
    def _(x, x_off, cin, w, bias, kernel, stride, relu, y, y_off, y2, y2_off, split):
        return None

    @custom_op("omnitok::maxpool3d_same", mutates_args=(), device_types="cuda")
    def _maxpool3d(x: torch.Tensor, kernel: List[int], stride: List[int]) -> torch.Tensor:
        if x.dtype != torch.float32 or x.dim() != 5:
            raise ValueError(f"maxpool3d_same: x must be float32 [B, T, H, W, C], got {x.dtype} {tuple(x.shape)}")
        x = x.contiguous()
        B, T, H, W, C = x.shape
        y = torch.empty(_grid3d(x.shape, kernel, stride) + (C,), device=x.device, dtype=torch.float32)
        check(_lib.load().omnitok_maxpool3d_same(ptr(x), B, T, H, W, C, *kernel, *stride, ptr(y), stream()),
              "maxpool3d_same")
        return y

    @_maxpool3d.register_fake
    def _(x, kernel, stride):
        return x.new_empty(_grid3d(x.shape, kernel, stride) + (x.shape[4],))

    @custom_op("omnitok::conv2d", mutates_args=("y", "y2"), device_types="cuda")
    def _conv2d(x: torch.Tensor, x_off: int, cin: int, w: torch.Tensor, bias: torch.Tensor, kernel: List[int],
                stride: List[int], padding: List[int], relu: bool, y: torch.Tensor, y_off: int, y2: Optional[torch.Tensor],
                y2_off: int, split: int) -> None:
        d = _conv_desc("conv2d", OmnitokConv2d, 4, _grid2d, (kernel, stride, padding), x, x_off, cin, w, bias,
                       relu, y, y_off, y2, y2_off, split)
        d.N, d.H, d.W = x.shape[:3]
        d.kh, d.kw = kernel
        d.sh, d.sw = stride
        d.ph, d.pw = padding
        check(_lib.load().omnitok_conv2d(ctypes.byref(d), stream()), "conv2d")

    @_conv2d.register_fake
    def _(x, x_off, cin, w, bias, kernel, stride, padding, relu, y, y_off, y2, y2_off, split):
        return None

    def _pool2d(what, x, k, s, p, y, y_off):
        if x.dtype != torch.float32 or x.dim() != 4 or not x.is_contiguous():
            raise ValueError(f"{what}: x must be a contiguous float32 [N, H, W, C], got {x.dtype} {tuple(x.shape)}")
        want = _grid2d(x.shape, (k, k), (s, s), (p, p))
        if y.dtype != torch.float32 or not y.is_contiguous() or tuple(y.shape[:3]) != want:
            raise ValueError(f"{what}: y is {tuple(y.shape)}, the output grid is {want}")
        N, H, W, C = x.shape
        check(getattr(_lib.load(), "omnitok_" + what)(ptr(x), N, H, W, C, k, s, p, ptr(y), y.shape[3], y_off, stream()),
              what)

    @custom_op("omnitok::maxpool2d", mutates_args=("y",), device_types="cuda")
    def _maxpool2d(x: torch.Tensor, k: int, s: int, p: int, y: torch.Tensor, y_off: int) -> None:
        _pool2d("maxpool2d", x, k, s, p, y, y_off)

    @_maxpool2d.register_fake
    def _(x, k, s, p, y, y_off):
        return None

    @custom_op("omnitok::avgpool2d", mutates_args=("y",), device_types="cuda")
    def _avgpool2d(x: torch.Tensor, k: int, s: int, p: int, y: torch.Tensor, y_off: int) -> None:
        _pool2d("avgpool2d", x, k, s, p, y, y_off)

    @_avgpool2d.register_fake
    def _(x, k, s, p, y, y_off):
        return None

    @custom_op("omnitok::spatial_mean", mutates_args=(), device_types="cuda")
    def _mean(x: torch.Tensor) -> torch.Tensor:
        if x.dtype != torch.float32 or x.dim() != 4:
            raise ValueError(f"spatial_mean: x must be float32 [N, H, W, C], got {x.dtype} {tuple(x.shape)}")
        x = x.contiguous()
        N, H, W, C = x.shape
        y = torch.empty((N, C), device=x.device, dtype=torch.float32)
        check(_lib.load().omnitok_spatial_mean(ptr(x), N, H, W, C, ptr(y), stream()), "spatial_mean")
        return y

    @_mean.register_fake
    def _(x):
        return x.new_empty((x.shape[0], x.shape[3]))


_register_ops()


def conv3d_same(x: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor, kernel: Sequence[int],
                stride: Sequence[int] = (1, 1, 1), relu: bool = True, *, cin: Optional[int] = None, x_off: int = 0,
                out: Optional[torch.Tensor] = None, out_off: int = 0, out2: Optional[torch.Tensor] = None,
                out2_off: int = 0, split: Optional[int] = None) -> torch.Tensor:
    """One Unit3D on channels-last x (channels [x_off, x_off + cin)); writes channels [out_off, out_off + split) of `out`
    (a new [B, To, Ho, Wo, Cout] tensor if None) and the columns past `split` to `out2` at out2_off.  Returns `out`."""
    return _conv_front(torch.ops.omnitok.conv3d_same, _grid3d, (list(kernel), list(stride)), x, w_packed, bias, relu, cin,
                       x_off, out, out_off, out2, out2_off, split)


def conv2d(x: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor, kernel: Sequence[int],
           stride: Sequence[int] = (1, 1), padding: Sequence[int] = (0, 0), relu: bool = True, *, cin: Optional[int] = None,
           x_off: int = 0, out: Optional[torch.Tensor] = None, out_off: int = 0, out2: Optional[torch.Tensor] = None,
           out2_off: int = 0, split: Optional[int] = None) -> torch.Tensor:
    """One BasicConv2d on channels-last x (channels [x_off, x_off + cin)); writes channels [out_off, out_off + split) of
    `out` (a new [N, Ho, Wo, Cout] tensor if None) and the columns past `split` to `out2` at out2_off.  Returns `out`."""
    return _conv_front(torch.ops.omnitok.conv2d, _grid2d, (list(kernel), list(stride), list(padding)), x, w_packed, bias,
                       relu, cin, x_off, out, out_off, out2, out2_off, split)


def maxpool3d_same(x: torch.Tensor, kernel: Sequence[int], stride: Sequence[int]) -> torch.Tensor:
    return torch.ops.omnitok.maxpool3d_same(x, list(kernel), list(stride))


def _pool2d_front(op, x, k, s, p, out, out_off):
    if out is None:
        out = torch.empty(_grid2d(x.shape, (k, k), (s, s), (p, p)) + (x.shape[3],), device=x.device, dtype=torch.float32)
    op(x, k, s, p, out, out_off)
    return out


def maxpool2d(x: torch.Tensor, k: int, s: int, p: int = 0, *, out: Optional[torch.Tensor] = None,
              out_off: int = 0) -> torch.Tensor:
    """max_pool2d(x, k, s, p) (-inf padding, floor sizing) on channels-last x, into channels [out_off, out_off + C) of out"""
    return _pool2d_front(torch.ops.omnitok.maxpool2d, x, k, s, p, out, out_off)


def avgpool2d(x: torch.Tensor, k: int, s: int, p: int = 0, *, out: Optional[torch.Tensor] = None,
              out_off: int = 0) -> torch.Tensor:
    """avg_pool2d(x, k, s, p, count_include_pad=False) on channels-last x"""
    return _pool2d_front(torch.ops.omnitok.avgpool2d, x, k, s, p, out, out_off)


def spatial_mean(x: torch.Tensor) -> torch.Tensor:
    """adaptive_avg_pool2d(x, 1) of channels-last [N, h, w, C] -> [N, C]"""
    return torch.ops.omnitok.spatial_mean(x)


# ---- weights ------------------------------------------------------------------------------------------------------------

def pack_conv_weight(w: torch.Tensor) -> torch.Tensor:
    """[Cout, Cin, kt, kh, kw] -> the packed [Cout, ldw] fp32 of omnitok_conv3d_same and (kt = 1) omnitok_conv2d:
    k = tap * Cin4 + ci, Cin4 = Cin rounded up to 4 (zero weights), zeros from K to ldw (a multiple of 32)"""
    cout, cin, kt, kh, kw = w.shape
    cin4 = (cin + 3) // 4 * 4
    ldw = int(_lib.load().omnitok_conv3d_packed_ldw(cin4, kt, kh, kw))
    if ldw < 0:
        raise ValueError(f"pack_conv_weight: unsupported shape {tuple(w.shape)}")
    p = torch.zeros((cout, kt, kh, kw, cin4), dtype=w.dtype)
    p[..., :cin] = w.detach().cpu().permute(0, 2, 3, 4, 1)
    out = torch.zeros((cout, ldw), dtype=torch.float32)
    out[:, :kt * kh * kw * cin4] = p.reshape(cout, -1).float()
    return out


def fold_bn(sd, prefix: str, conv: str, eps: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(weight, bias) of the bias-free conv `prefix`.`conv` with the BatchNorm `prefix`.bn folded in, in fp64"""
    w = sd[f"{prefix}.{conv}.weight"].double()
    g, b = sd[f"{prefix}.bn.weight"].double(), sd[f"{prefix}.bn.bias"].double()
    m, v = sd[f"{prefix}.bn.running_mean"].double(), sd[f"{prefix}.bn.running_var"].double()
    scale = g / torch.sqrt(v + eps)
    return w * scale.view(-1, *[1] * (w.dim() - 1)), b - m * scale


def check_state_dict(sd, spec, what: str, ignore: Sequence[str] = (), optional: Sequence[str] = ()):
    """RuntimeError unless sd holds exactly the keys of spec (key -> shape) with those shapes.  Keys that start with one of
    `ignore` may be there besides; the keys in `optional` may be absent, but all of them or none."""
    missing = [k for k in spec if k not in sd and k not in optional]
    if any(k in sd for k in optional):
        missing += [k for k in optional if k not in sd]
    unexpected = [k for k in sd if k not in spec and not k.startswith(tuple(ignore))]
    if missing or unexpected:
        raise RuntimeError(f"Error(s) in loading state_dict for {what}: missing keys {missing[:8]}"
                           f"{' ...' if len(missing) > 8 else ''}, unexpected keys {unexpected[:8]}"
                           f"{' ...' if len(unexpected) > 8 else ''}")
    for k, shape in spec.items():
        if k in sd and tuple(sd[k].shape) != tuple(shape):
            raise RuntimeError(f"Error(s) in loading state_dict for {what}: size mismatch for {k}: copying a param with "
                               f"shape {tuple(sd[k].shape)}, the model has {tuple(shape)}")


class PackedWeights(torch.nn.Module):
    """A network whose weights live outside torch's parameters: the state_dict as loaded, on the host (`_sd`), and what the
    kernels read, packed once per device (`_packed`).  Loading is strict (every parameter feeds the output).  A network
    defines _held(state_dict) -> the checked state_dict under its own keys, on the host, and _pack(sd, device)."""

    NOT_LOADED = "load_state_dict first"

    def __init__(self):
        super().__init__()
        self._sd: Optional["OrderedDict[str, torch.Tensor]"] = None
        self._packed: Dict[torch.device, dict] = {}

    def state_dict(self, *args, **kwargs):
        if self._sd is None:
            raise RuntimeError(f"{type(self).__name__}: no weights loaded")
        return OrderedDict((k, v.clone()) for k, v in self._sd.items())

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        self._sd = self._held(state_dict)
        self._packed = {}
        return torch.nn.modules.module._IncompatibleKeys([], [])

    def _weights(self, device: torch.device) -> dict:
        if self._sd is None:
            raise RuntimeError(f"{type(self).__name__}: {self.NOT_LOADED}")
        if device not in self._packed:
            self._packed[device] = self._pack(self._sd, device)
        return self._packed[device]
