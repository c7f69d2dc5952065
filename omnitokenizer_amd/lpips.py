"""LPIPS on the device: the reference's OmniTokenizer/modules/lpips.py (taming's VGG16 LPIPS, the tokenizer's own
perceptual model: `perceptual_model` of omnitokenizer.py, the `val/perceptual_loss` of validation_step), with its input
path and heads in csrc/lpips.hip and its VGG16 trunk on convnet.py's conv2d / maxpool2d (include/omnitok.h "LPIPS").

    model = load_lpips("cuda", "omnitokenizer.ckpt")           # a checkpoint's perceptual_model.* (no download)
    d = model(input, target)                                   # [N, 3, H, W] fp32 -> [N, 1, 1, 1], as the reference
    d = lpips_frames(x, x_recon, model, layout="bcthw")        # [B, F] of every frame pair, read in place

A pass runs 2N images (input rows [0, N), target rows [N, 2N)) of at most max_pairs pairs:
  preprocess   omnitok::lpips_preprocess of each operand: (+ shift, clamp), 2 v - 1 if normalize, ScalingLayer
  slice 1..5   omnitok::conv2d (3 x 3, pad 1, bias, ReLU) x 2, 2, 3, 3, 3, a 2 x 2 omnitok::maxpool2d before slices 2..5
  head         omnitok::lpips_layer on each slice output as soon as it exists (normalize_tensor, squared difference,
               NetLinLayer, spatial mean in fp64), so only two activation buffers are alive at a time
  finalize     omnitok::lpips_finalize: val = res[0] + ... + res[4]
Every value is a fixed-order sum, so a pair gets the same bits alone, in any batch and under any max_pairs.
"""
from __future__ import annotations

import ctypes
import os
from collections import OrderedDict
from typing import List, Optional, Tuple

import torch

from . import _lib
from ._lib import check, ptr, stream
from .convnet import PackedWeights, check_state_dict, conv2d, maxpool2d, pack_conv_weight

MIN_SIZE = 16                     # OMNITOK_LPIPS_MIN_SIZE
FLAG_NORMALIZE = 1                # OMNITOK_LPIPS_NORMALIZE
CHNS = (64, 128, 256, 512, 512)   # LPIPS.chns
# ScalingLayer's buffers (lpips.py), used when the weights come from torchvision's vgg16 and taming's vgg.pth
SCALING_SHIFT = (-.030, -.088, -.188)
SCALING_SCALE = (.458, .448, .450)
# VGG16 (torchvision cfg "D") features: (slice, features index, Cin, Cout) of every conv; a 2 x 2 max pool opens slices 2..5
CONVS = [(1, 0, 3, 64), (1, 2, 64, 64),
         (2, 5, 64, 128), (2, 7, 128, 128),
         (3, 10, 128, 256), (3, 12, 256, 256), (3, 14, 256, 256),
         (4, 17, 256, 512), (4, 19, 512, 512), (4, 21, 512, 512),
         (5, 24, 512, 512), (5, 26, 512, 512), (5, 28, 512, 512)]
LAYOUTS = ("bcthw", "btchw", "bthwc", "nchw")


def state_spec() -> "OrderedDict[str, Tuple[int, ...]]":
    """key -> shape of the reference's LPIPS().state_dict(), in its order"""
    spec = OrderedDict()
    spec["scaling_layer.shift"] = (1, 3, 1, 1)
    spec["scaling_layer.scale"] = (1, 3, 1, 1)
    for s, i, cin, cout in CONVS:
        spec[f"net.slice{s}.{i}.weight"] = (cout, cin, 3, 3)
        spec[f"net.slice{s}.{i}.bias"] = (cout,)
    for k, c in enumerate(CHNS):
        spec[f"lin{k}.model.1.weight"] = (1, c, 1, 1)
    return spec


def to_torchvision(sd) -> Tuple["OrderedDict[str, torch.Tensor]", "OrderedDict[str, torch.Tensor]"]:
    """an LPIPS state_dict -> (torchvision vgg16 `features.{i}.*` weights, taming vgg.pth's `lin{k}.model.1.weight`)"""
    vgg = OrderedDict()
    for s, i, _, _ in CONVS:
        vgg[f"features.{i}.weight"] = sd[f"net.slice{s}.{i}.weight"]
        vgg[f"features.{i}.bias"] = sd[f"net.slice{s}.{i}.bias"]
    lin = OrderedDict((f"lin{k}.model.1.weight", sd[f"lin{k}.model.1.weight"]) for k in range(len(CHNS)))
    return vgg, lin


# ---- the operators ------------------------------------------------------------------------------------------------------

def _register_ops():
    from torch.library import custom_op
    from .metrics import _operand_desc

    @custom_op("omnitok::lpips_preprocess", mutates_args=("out",), device_types="cuda")
    def _pre(src: torch.Tensor, shift: float, clamp: bool, normalize: bool, scaling_shift: List[float],
             scaling_scale: List[float], i0: int, out: torch.Tensor) -> None:
        if src.dim() != 5 or src.shape[2] != 3 or src.dtype not in (torch.float32, torch.uint8):
            raise ValueError(f"lpips_preprocess: src must be a [B, F, 3, H, W] view of float32 or uint8, got {src.dtype} "
                             f"{tuple(src.shape)}")
        B, F_, _, H, W = src.shape
        if out.dtype != torch.float32 or not out.is_contiguous() or out.dim() != 4 or tuple(out.shape[1:]) != (H, W, 4):
            raise ValueError(f"lpips_preprocess: out must be a contiguous float32 [n, {H}, {W}, 4], got {tuple(out.shape)}")
        if min(src.stride()) < 0:
            src = src.contiguous()
        sh = (ctypes.c_float * 3)(*scaling_shift)
        sc = (ctypes.c_float * 3)(*scaling_scale)
        d = _operand_desc(src, shift, clamp)
        check(_lib.load().omnitok_lpips_preprocess(ctypes.byref(d), B, F_, H, W, i0, out.shape[0],
                                                   FLAG_NORMALIZE if normalize else 0, sh, sc, ptr(out), stream()),
              "lpips_preprocess")

    @_pre.register_fake
    def _(src, shift, clamp, normalize, scaling_shift, scaling_scale, i0, out):
        return None

    @custom_op("omnitok::lpips_layer", mutates_args=("res",), device_types="cuda")
    def _layer(feats: torch.Tensor, lin_w: torch.Tensor, layer: int, res: torch.Tensor) -> None:
        if feats.dtype != torch.float32 or feats.dim() != 4 or not feats.is_contiguous() or feats.shape[0] % 2:
            raise ValueError(f"lpips_layer: feats must be a contiguous float32 [2N, h, w, C], got {feats.dtype} "
                             f"{tuple(feats.shape)}")
        N2, h, w, C = feats.shape
        if lin_w.dtype != torch.float32 or not lin_w.is_contiguous() or lin_w.numel() != C:
            raise ValueError(f"lpips_layer: lin_w must be a contiguous float32 [{C}], got {tuple(lin_w.shape)}")
        if res.dtype != torch.float64 or not res.is_contiguous() or tuple(res.shape) != (N2 // 2, 5):
            raise ValueError(f"lpips_layer: res must be a contiguous float64 [{N2 // 2}, 5], got {tuple(res.shape)}")
        lib = _lib.load()
        need = lib.omnitok_lpips_workspace(N2 // 2, h, w)
        if need < 0:
            raise ValueError(f"lpips_layer: bad shape {tuple(feats.shape)}")
        work = torch.empty(max(need, 8), device=feats.device, dtype=torch.uint8)
        check(lib.omnitok_lpips_layer(ptr(feats), N2 // 2, h, w, C, ptr(lin_w), layer, ptr(work), need, ptr(res),
                                      stream()), "lpips_layer")

    @_layer.register_fake
    def _(feats, lin_w, layer, res):
        return None

    @custom_op("omnitok::lpips_finalize", mutates_args=(), device_types="cuda")
    def _fin(res: torch.Tensor) -> torch.Tensor:
        if res.dtype != torch.float64 or res.dim() != 2 or res.shape[1] != 5:
            raise ValueError(f"lpips_finalize: res must be float64 [N, 5], got {res.dtype} {tuple(res.shape)}")
        res = res.contiguous()
        val = torch.empty(res.shape[0], device=res.device, dtype=torch.float32)
        check(_lib.load().omnitok_lpips_finalize(ptr(res), res.shape[0], ptr(val), stream()), "lpips_finalize")
        return val

    @_fin.register_fake
    def _(res):
        return res.new_empty((res.shape[0],), dtype=torch.float32)


_register_ops()


def layer_head(feats: torch.Tensor, lin_w: torch.Tensor, layer: int = 0, res: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One slice's head on channels-last feats [2N, h, w, C] (image n paired with N + n): writes and returns res [N, 5]
    float64, column `layer` = the spatial mean of sum_c w_c (a_c / (|a| + 1e-10) - b_c / (|b| + 1e-10))^2"""
    if res is None:
        res = torch.zeros((feats.shape[0] // 2, 5), device=feats.device, dtype=torch.float64)
    torch.ops.omnitok.lpips_layer(feats, lin_w.reshape(-1).contiguous(), int(layer), res)
    return res


# ---- the model ----------------------------------------------------------------------------------------------------------

class LPIPS(PackedWeights):
    """The reference's LPIPS (lpips.py, use_dropout=True) for inference: state_dict keys and forward contract as there
    ([N, 3, H, W] fp32 pairs -> [N, 1, 1, 1] fp32), on the GPU.  Weights are given by load_state_dict (strict) or
    load_lpips; they are packed once per device.  There is no CPU path and no training (Dropout is the identity)."""

    NOT_LOADED = "load_state_dict first (or load_lpips)"

    def __init__(self, max_pairs: int = 32):
        super().__init__()
        self.max_pairs = int(max_pairs)

    def _held(self, state_dict):
        """Strict: exactly the reference's LPIPS().state_dict() keys and shapes"""
        check_state_dict(state_dict, state_spec(), "LPIPS")
        return OrderedDict((k, state_dict[k].detach().cpu().float().clone()) for k in state_spec())

    def _pack(self, sd, device: torch.device) -> dict:
        convs = []
        for s, i, _, _ in CONVS:
            w = sd[f"net.slice{s}.{i}.weight"]
            convs.append((s, pack_conv_weight(w.unsqueeze(2)).to(device),
                          sd[f"net.slice{s}.{i}.bias"].contiguous().to(device)))
        lins = [sd[f"lin{k}.model.1.weight"].reshape(-1).contiguous().to(device) for k in range(len(CHNS))]
        return dict(convs=convs, lins=lins, shift=[float(v) for v in sd["scaling_layer.shift"].reshape(-1)],
                    scale=[float(v) for v in sd["scaling_layer.scale"].reshape(-1)])

    def packed(self, device) -> dict:
        """the packed weights on `device`: convs [(slice, packed weight, bias)], lins [C], shift, scale"""
        return self._weights(torch.device(device))

    def trunk(self, x: torch.Tensor, res: torch.Tensor, endpoints: Optional[list] = None) -> torch.Tensor:
        """the VGG16 slices on the preprocessed channels-last x [2N, H, W, 4], each slice's head into res [N, 5]"""
        pk = self._weights(x.device)
        cur = 1
        for s, w, b in pk["convs"]:
            if s != cur:
                layer_head(x, pk["lins"][cur - 1], cur - 1, res)
                if endpoints is not None:
                    endpoints.append(x)
                x = maxpool2d(x, 2, 2, 0)
                cur = s
            x = conv2d(x, w, b, (3, 3), (1, 1), (1, 1), True)
        layer_head(x, pk["lins"][cur - 1], cur - 1, res)
        if endpoints is not None:
            endpoints.append(x)
        return res

    def _pairs(self, va: torch.Tensor, vb: torch.Tensor, shift: float, clamp: bool, normalize: bool,
               max_pairs: int) -> torch.Tensor:
        """va, vb: [B, F, 3, H, W] views -> [B * F] fp32 (pair b * F + t)"""
        B, F_, _, H, W = va.shape
        if H < MIN_SIZE or W < MIN_SIZE:
            raise ValueError(f"LPIPS: {H} x {W} frames are too small: the reference's VGG16 slices need at least "
                             f"{MIN_SIZE} x {MIN_SIZE} (four 2 x 2 max pools)")
        if max_pairs < 1:
            raise ValueError(f"LPIPS: max_pairs {max_pairs}, expected >= 1")
        total = B * F_
        out = torch.empty(total, device=va.device, dtype=torch.float32)
        with torch.cuda.device(va.device):
            pk = self._weights(va.device)
            for i0 in range(0, total, max_pairs):
                n = min(max_pairs, total - i0)
                x = torch.empty((2 * n, H, W, 4), device=va.device, dtype=torch.float32)
                for half, v in enumerate((va, vb)):
                    torch.ops.omnitok.lpips_preprocess(v, float(shift), bool(clamp), bool(normalize), pk["shift"],
                                                       pk["scale"], i0, x[half * n:(half + 1) * n])
                res = torch.empty((n, 5), device=va.device, dtype=torch.float64)
                self.trunk(x, res)
                del x
                out[i0:i0 + n] = torch.ops.omnitok.lpips_finalize(res)
        return out

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        """input, target [N, 3, H, W] fp32 on one GPU (the reference's range, e.g. the tokenizer's [-0.5, 0.5]) ->
        [N, 1, 1, 1] fp32"""
        for name, t in (("input", input), ("target", target)):
            if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.shape[1] != 3:
                raise ValueError(f"LPIPS: {name} must be [N, 3, H, W], got {getattr(t, 'shape', type(t))}")
            if t.dtype != torch.float32:
                raise TypeError(f"LPIPS: {name}: dtype {t.dtype}, expected torch.float32")
            if t.device.type != "cuda":
                raise RuntimeError(f"LPIPS: {name} on {t.device}: the network runs on the GPU (there is no CPU path)")
        if input.shape != target.shape:
            raise ValueError(f"LPIPS: input {tuple(input.shape)} and target {tuple(target.shape)} differ in shape")
        if input.device != target.device:
            raise RuntimeError(f"LPIPS: input on {input.device}, target on {target.device}")
        va, vb = input.unsqueeze(1), target.unsqueeze(1)
        return self._pairs(va, vb, 0.0, False, False, self.max_pairs).view(-1, 1, 1, 1)


def _load_file(path):
    sd = torch.load(path, map_location="cpu", weights_only=False)
    if isinstance(sd, dict) and "state_dict" in sd and isinstance(sd["state_dict"], dict):
        sd = sd["state_dict"]
    return sd


def load_lpips(device="cuda", source=None, max_pairs: int = 32) -> LPIPS:
    """An LPIPS with its weights from `source`, packed on `device`:
      (a) a VQGAN checkpoint path or state_dict holding perceptual_model.* (the other keys are ignored);
      (b) an LPIPS state_dict (or its path): the reference's LPIPS().state_dict() keys;
      (c) a pair (torchvision vgg16 weights, taming's vgg.pth), each a state_dict or a path: features.{0, 2, ..., 28}.*
          (classifier.* ignored) and lin{0..4}.model.1.weight, with the reference's ScalingLayer constants.
    Keys and shapes are checked strictly."""
    if source is None:
        raise ValueError("load_lpips: a source is required (a checkpoint, an LPIPS state_dict, or (vgg16, vgg.pth))")
    spec = state_spec()
    if isinstance(source, (tuple, list)):
        if len(source) != 2:
            raise ValueError("load_lpips: a pair (torchvision vgg16 state_dict, taming vgg.pth) is expected")
        vgg, lin = (_load_file(s) if isinstance(s, (str, os.PathLike)) else s for s in source)
        vspec = OrderedDict()
        for _, i, cin, cout in CONVS:
            vspec[f"features.{i}.weight"] = (cout, cin, 3, 3)
            vspec[f"features.{i}.bias"] = (cout,)
        check_state_dict(vgg, vspec, "torchvision vgg16", ignore=("classifier.",))
        lspec = OrderedDict((k, v) for k, v in spec.items() if k.startswith("lin"))
        check_state_dict(lin, lspec, "vgg.pth")
        sd = OrderedDict()
        sd["scaling_layer.shift"] = torch.tensor(SCALING_SHIFT, dtype=torch.float32).view(1, 3, 1, 1)
        sd["scaling_layer.scale"] = torch.tensor(SCALING_SCALE, dtype=torch.float32).view(1, 3, 1, 1)
        for s, i, _, _ in CONVS:
            sd[f"net.slice{s}.{i}.weight"] = vgg[f"features.{i}.weight"]
            sd[f"net.slice{s}.{i}.bias"] = vgg[f"features.{i}.bias"]
        sd.update(lin)
    else:
        sd = _load_file(source) if isinstance(source, (str, os.PathLike)) else source
        if not isinstance(sd, dict):
            raise TypeError(f"load_lpips: source must be a path, a state_dict or a pair, got {type(source).__name__}")
        pre = "perceptual_model."
        if any(k.startswith(pre) for k in sd):
            sd = OrderedDict((k[len(pre):], v) for k, v in sd.items() if k.startswith(pre))
    m = LPIPS(max_pairs)
    m.load_state_dict(sd)
    m._weights(torch.device(device))
    return m


def _as_btchw(x, layout: str, name: str) -> torch.Tensor:
    from .metrics import _as_btchw as as_btchw
    if layout == "nchw":
        if not isinstance(x, torch.Tensor) or x.dim() != 4:
            raise ValueError(f"{name} must be [N, 3, H, W] in layout 'nchw', got {getattr(x, 'shape', type(x))}")
        return as_btchw(x.unsqueeze(1), "btchw", name)
    return as_btchw(x, layout, name)


def lpips_frames(a: torch.Tensor, b: torch.Tensor, model: LPIPS, layout: str = "bcthw", shift: float = 0.0,
                 normalize: bool = False, max_pairs: int = 32) -> torch.Tensor:
    """The reference LPIPS of every frame pair of two videos (or image batches) on one GPU -> [B, F] fp32.

    layout: "bcthw" [B, 3, F, H, W] (the tokenizer's pixels), "btchw" [B, F, 3, H, W], "bthwc" [B, F, H, W, 3] (uint8 frames),
        "nchw" [N, 3, H, W] (F = 1); read in place through their strides.
    dtype: float32 or uint8 (u / 255); `shift` is added first (-0.5 maps uint8 frames to the tokenizer's [-0.5, 0.5]), then
        2 v - 1 if normalize (lpips' normalize=True, for [0, 1] values), then the model's ScalingLayer.
    Runs max_pairs pairs per pass; the result has the same bits for any max_pairs."""
    if not isinstance(model, LPIPS):
        raise TypeError(f"lpips_frames: model must be an omnitokenizer_amd LPIPS, got {type(model).__name__}")
    if layout not in LAYOUTS:
        raise ValueError(f"layout must be one of {list(LAYOUTS)}, got {layout!r}")
    va, vb = _as_btchw(a, layout, "a"), _as_btchw(b, layout, "b")
    if va.shape != vb.shape:
        raise ValueError(f"a and b differ in shape: {tuple(a.shape)} vs {tuple(b.shape)}")
    for name, v in (("a", va), ("b", vb)):
        if v.device.type != "cuda":
            raise RuntimeError(f"{name} is on {v.device}: LPIPS runs on the GPU (there is no CPU path)")
    if va.device != vb.device:
        raise RuntimeError(f"a on {va.device}, b on {vb.device}: both must be on one GPU")
    B, F_ = va.shape[:2]
    return model._pairs(va, vb, float(shift), False, bool(normalize), int(max_pairs)).view(B, F_)
