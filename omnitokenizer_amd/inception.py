"""Inception V3 on the device: the reference's evaluation/pytorch-fid InceptionV3 (torchvision's Inception3 with the FID
patches, the feature net of FID), its state_dicts and its feature blocks, with every layer in csrc/inception.hip
(include/omnitok.h "Inception V3").  The conv and pool operators and the weight scaffold are convnet.py's, shared with
i3d.py and lpips.py.

    net = InceptionV3([3])                                                  # output_blocks as in the reference
    net.load_state_dict(torch.load("pt_inception-2015-12-05-6726825d.pth"))  # strict: the .pth keys or the wrapper's
    feats = net(x.cuda())[0]                                                # x [N, 3, H, W] fp32 in [0, 1] -> [N, 2048, 1, 1]

At load time every BatchNorm (eps 1e-3) is folded into its bias-free conv in fp64 (w * g / sqrt(v + eps),
b - m * g / sqrt(v + eps)), rounded to fp32 and packed in the layout omnitok_conv2d reads.  A forward runs on channels-last
activations [N, H, W, C], at most MAX_CHUNK images per pass:
  preprocess        omnitok::fid_preprocess (u8 / 255, the 299 x 299 bilinear resize, 2 x - 1)
  stem              omnitok::conv2d x 5, omnitok::maxpool2d x 2
  Mixed_5b .. 7c    the sibling 1x1 convs of one input as ONE GEMM whose column split routes the first branch straight into
                    the module output and the others into a scratch tensor; every later conv reads a channel slice of it and
                    writes its own channel slice of the module output, so the concat costs nothing; the pool branch is
                    omnitok::avgpool2d (A, C, E_1) or omnitok::maxpool2d (E_2) then a 1x1 conv, or (B, D) a max pool straight
                    into the output
  block 3's pool    omnitok::spatial_mean
Each output element is a fixed-order fp32 sum, so an image gets the same features alone and in any batch.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import List, Optional, Tuple

import torch

from . import _lib, convnet
from ._lib import check, ptr, stream
from .convnet import avgpool2d, conv2d, maxpool2d, out_size, pack_conv_weight, spatial_mean

MAX_CHUNK = 64   # images per pass through the network: bounds the activations to ~0.6 GB at 299 x 299
BN_EPS = 1e-3
RESIZE = 299
FID_U8, FID_F32 = 0, 1            # OMNITOK_FID_U8_NHWC, OMNITOK_FID_F32_NCHW
FLAG_RESIZE, FLAG_NORMALIZE = 1, 2
BLOCK_INDEX_BY_DIM = {64: 0, 192: 1, 768: 2, 2048: 3}
DIMS = {0: 64, 1: 192, 2: 768, 3: 2048}


def _conv(name, cin, cout, k, s=1, p=0):
    """(name, cin, cout, (kh, kw), (sh, sw), (ph, pw)) of one BasicConv2d"""
    k = (k, k) if isinstance(k, int) else tuple(k)
    p = (p, p) if isinstance(p, int) else tuple(p)
    return (name, cin, cout, k, (s, s), p)


def _module_a(cin, pool):
    return [_conv("branch1x1", cin, 64, 1), _conv("branch5x5_1", cin, 48, 1), _conv("branch5x5_2", 48, 64, 5, p=2),
            _conv("branch3x3dbl_1", cin, 64, 1), _conv("branch3x3dbl_2", 64, 96, 3, p=1),
            _conv("branch3x3dbl_3", 96, 96, 3, p=1), _conv("branch_pool", cin, pool, 1)]


def _module_b(cin):
    return [_conv("branch3x3", cin, 384, 3, s=2), _conv("branch3x3dbl_1", cin, 64, 1),
            _conv("branch3x3dbl_2", 64, 96, 3, p=1), _conv("branch3x3dbl_3", 96, 96, 3, s=2)]


def _module_c(cin, c7):
    return [_conv("branch1x1", cin, 192, 1), _conv("branch7x7_1", cin, c7, 1), _conv("branch7x7_2", c7, c7, (1, 7), p=(0, 3)),
            _conv("branch7x7_3", c7, 192, (7, 1), p=(3, 0)), _conv("branch7x7dbl_1", cin, c7, 1),
            _conv("branch7x7dbl_2", c7, c7, (7, 1), p=(3, 0)), _conv("branch7x7dbl_3", c7, c7, (1, 7), p=(0, 3)),
            _conv("branch7x7dbl_4", c7, c7, (7, 1), p=(3, 0)), _conv("branch7x7dbl_5", c7, 192, (1, 7), p=(0, 3)),
            _conv("branch_pool", cin, 192, 1)]


def _module_d(cin):
    return [_conv("branch3x3_1", cin, 192, 1), _conv("branch3x3_2", 192, 320, 3, s=2), _conv("branch7x7x3_1", cin, 192, 1),
            _conv("branch7x7x3_2", 192, 192, (1, 7), p=(0, 3)), _conv("branch7x7x3_3", 192, 192, (7, 1), p=(3, 0)),
            _conv("branch7x7x3_4", 192, 192, 3, s=2)]


def _module_e(cin):
    return [_conv("branch1x1", cin, 320, 1), _conv("branch3x3_1", cin, 384, 1),
            _conv("branch3x3_2a", 384, 384, (1, 3), p=(0, 1)), _conv("branch3x3_2b", 384, 384, (3, 1), p=(1, 0)),
            _conv("branch3x3dbl_1", cin, 448, 1), _conv("branch3x3dbl_2", 448, 384, 3, p=1),
            _conv("branch3x3dbl_3a", 384, 384, (1, 3), p=(0, 1)), _conv("branch3x3dbl_3b", 384, 384, (3, 1), p=(1, 0)),
            _conv("branch_pool", cin, 192, 1)]


# the network in order: (block, torchvision name, kind, its convs); kind "conv" is a lone BasicConv2d, "pool" max_pool2d(3, 2)
NET = [
    (0, "Conv2d_1a_3x3", "conv", [_conv("", 3, 32, 3, s=2)]),
    (0, "Conv2d_2a_3x3", "conv", [_conv("", 32, 32, 3)]),
    (0, "Conv2d_2b_3x3", "conv", [_conv("", 32, 64, 3, p=1)]),
    (0, "maxpool1", "pool", []),
    (1, "Conv2d_3b_1x1", "conv", [_conv("", 64, 80, 1)]),
    (1, "Conv2d_4a_3x3", "conv", [_conv("", 80, 192, 3)]),
    (1, "maxpool2", "pool", []),
    (2, "Mixed_5b", "A", _module_a(192, 32)),
    (2, "Mixed_5c", "A", _module_a(256, 64)),
    (2, "Mixed_5d", "A", _module_a(288, 64)),
    (2, "Mixed_6a", "B", _module_b(288)),
    (2, "Mixed_6b", "C", _module_c(768, 128)),
    (2, "Mixed_6c", "C", _module_c(768, 160)),
    (2, "Mixed_6d", "C", _module_c(768, 160)),
    (2, "Mixed_6e", "C", _module_c(768, 192)),
    (3, "Mixed_7a", "D", _module_d(768)),
    (3, "Mixed_7b", "E1", _module_e(1280)),
    (3, "Mixed_7c", "E2", _module_e(2048)),
]
BN_KEYS = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")


def _convs_with_keys(wrapper: bool, last_block: int = 3):
    """(state_dict prefix, (name, cin, cout, k, s, p)) of every BasicConv2d up to last_block, in state_dict order"""
    out, index = [], {0: 0, 1: 0, 2: 0, 3: 0}
    for blk, name, kind, convs in NET:
        if blk > last_block:
            break
        if kind == "pool":
            index[blk] += 1
            continue
        base = f"blocks.{blk}.{index[blk]}" if wrapper else name
        index[blk] += 1
        for c in convs:
            out.append((f"{base}.{c[0]}" if c[0] else base, c))
    return out


def state_spec(wrapper: bool = False, last_block: int = 3) -> "OrderedDict[str, Tuple[Tuple[int, ...], torch.dtype]]":
    """key -> (shape, dtype) of a state_dict in its order: the .pth file's (torchvision Inception3(num_classes=1008,
    aux_logits=False), fc included) if not wrapper, else InceptionV3's own (blocks.{i}.{j}.*, up to last_block, no fc)"""
    spec = OrderedDict()
    for prefix, (_, cin, cout, k, _, _) in _convs_with_keys(wrapper, last_block):
        spec[f"{prefix}.conv.weight"] = ((cout, cin) + k, torch.float32)
        for s in BN_KEYS:
            spec[f"{prefix}.bn.{s}"] = (((), torch.int64) if s == "num_batches_tracked" else ((cout,), torch.float32))
    if not wrapper:
        spec["fc.weight"] = ((1008, 2048), torch.float32)
        spec["fc.bias"] = ((1008,), torch.float32)
    return spec


def block_extents(H: int, W: int, last_block: int = 3) -> List[Tuple[str, int, int]]:
    """(layer, h, w) of every layer output of the reference's forward on an H x W network input, up to last_block; an
    extent of 0 is where the reference's forward fails"""
    out, h, w = [], H, W
    for blk, name, kind, convs in NET:
        if blk > last_block:
            break
        if kind == "conv":
            _, _, _, k, s, p = convs[0]
            h, w = out_size(h, k[0], s[0], p[0]), out_size(w, k[1], s[1], p[1])
        elif kind == "pool" or kind in ("B", "D"):   # max_pool2d(3, 2) and the 3x3 / stride-2 convs beside it
            h, w = out_size(h, 3, 2, 0), out_size(w, 3, 2, 0)
        out.append((name, h, w))
        if min(h, w) < 1:
            break
    return out


def min_input_size(last_block: int = 3) -> int:
    """the least H (= W) at which every layer up to last_block has an output: 11, 27, 43, 75 for blocks 0..3 (from the
    table of NET: the valid 3x3 convs take 2 off, and Conv2d_1a, the two stem pools, Mixed_6a and Mixed_7a each map s to
    floor((s - 3) / 2) + 1, which needs s >= 3)"""
    s = 1
    while min(min(h, w) for _, h, w in block_extents(s, s, last_block)) < 1:
        s += 1
    return s


def check_input_size(H: int, W: int, last_block: int):
    """ValueError where the reference's own forward would fail on an H x W network input"""
    for name, h, w in block_extents(H, W, last_block):
        if h < 1 or w < 1:
            need = min_input_size(last_block)
            raise ValueError(f"InceptionV3: a {H} x {W} input is too small for block {last_block} ({name} has no output; "
                             f"at least {need} x {need} is needed, or resize_input=True)")


# ---- the operator of Inception alone (the conv and the pools are convnet.py's) ------------------------------------------

def _preprocess_native(src: torch.Tensor, resize: bool, normalize: bool, R_h: int, R_w: int) -> torch.Tensor:
    if src.dtype == torch.uint8:
        N, H, W, _ = src.shape
        dtype, ld = FID_U8, src.stride(1)
    else:
        N, _, H, W = src.shape
        dtype, ld = FID_F32, 0
    out = torch.empty((N, R_h, R_w, 4), device=src.device, dtype=torch.float32)
    flags = (FLAG_RESIZE if resize else 0) | (FLAG_NORMALIZE if normalize else 0)
    check(_lib.load().omnitok_fid_preprocess(ptr(src), dtype, ld, N, H, W, R_h, R_w, flags, ptr(out), stream()),
          "fid_preprocess")
    return out


def _register_ops():
    from torch.library import custom_op

    @custom_op("omnitok::fid_preprocess", mutates_args=(), device_types="cuda")
    def _pre(src: torch.Tensor, resize: bool, normalize: bool, R_h: int, R_w: int) -> torch.Tensor:
        if src.dtype == torch.uint8:
            if src.dim() != 4 or src.shape[3] != 3 or src.stride(3) != 1 or src.stride(2) != 3 or \
                    src.stride(0) != src.shape[1] * src.stride(1):
                raise ValueError(f"fid_preprocess: uint8 images must be [N, H, W, 3] with dense pixels and rows, got "
                                 f"{tuple(src.shape)} strides {src.stride()}")
        elif src.dtype == torch.float32:
            if src.dim() != 4 or src.shape[1] != 3:
                raise ValueError(f"fid_preprocess: float32 images must be [N, 3, H, W], got {tuple(src.shape)}")
            src = src.contiguous()
        else:
            raise ValueError(f"fid_preprocess: images must be uint8 [N, H, W, 3] or float32 [N, 3, H, W], got {src.dtype}")
        return _preprocess_native(src, resize, normalize, R_h, R_w)

    @_pre.register_fake
    def _(src, resize, normalize, R_h, R_w):
        return src.new_empty((src.shape[0], R_h, R_w, 4), dtype=torch.float32)


_register_ops()


def preprocess_images(images: torch.Tensor, resize: bool = True, normalize: bool = True,
                      size: Tuple[int, int] = (RESIZE, RESIZE)) -> torch.Tensor:
    """uint8 [N, H, W, 3] or fp32 [N, 3, H, W] in [0, 1] on the GPU -> the fp32 network input [N, R_h, R_w, 4]
    channels-last (channel 3 zero): InceptionV3.forward's resize and normalisation after ToTensor"""
    H, W = (images.shape[1], images.shape[2]) if images.dtype == torch.uint8 else (images.shape[2], images.shape[3])
    R_h, R_w = (int(size[0]), int(size[1])) if resize else (int(H), int(W))
    return torch.ops.omnitok.fid_preprocess(images, bool(resize), bool(normalize), R_h, R_w)


def fold_bn(sd, prefix: str) -> Tuple[torch.Tensor, torch.Tensor]:
    """(weight, bias) of BasicConv2d `prefix` with its BatchNorm (eps 1e-3) folded in, in fp64"""
    return convnet.fold_bn(sd, prefix, "conv", BN_EPS)


# the sibling 1x1 convs of one input that a module runs as one GEMM (the first goes straight to the module output)
FUSED_1X1 = {"A": ("branch1x1", "branch5x5_1", "branch3x3dbl_1"), "B": ("branch3x3dbl_1",),
             "C": ("branch1x1", "branch7x7_1", "branch7x7dbl_1"), "D": ("branch3x3_1", "branch7x7x3_1"),
             "E1": ("branch1x1", "branch3x3_1", "branch3x3dbl_1"), "E2": ("branch1x1", "branch3x3_1", "branch3x3dbl_1")}


class InceptionV3(convnet.PackedWeights):
    """The reference's pytorch-fid InceptionV3 for its FID use: constructor arguments, BLOCK_INDEX_BY_DIM and the forward
    contract (fp32 [N, 3, H, W] in [0, 1] -> one [N, C, h, w] per requested block, sorted by index) as there, on the GPU.
    The outputs are channels-last views.  use_fid_inception=False (torchvision's ImageNet weights) is not provided."""

    DEFAULT_BLOCK_INDEX = 3
    BLOCK_INDEX_BY_DIM = dict(BLOCK_INDEX_BY_DIM)

    def __init__(self, output_blocks=(DEFAULT_BLOCK_INDEX,), resize_input=True, normalize_input=True,
                 requires_grad=False, use_fid_inception=True):
        if not use_fid_inception:
            raise NotImplementedError("InceptionV3: use_fid_inception=False (torchvision's ImageNet Inception) is not "
                                      "provided; FID uses the FID Inception weights")
        if requires_grad:
            raise NotImplementedError("InceptionV3: requires_grad=True: the network is inference-only")
        blocks = sorted(int(b) for b in output_blocks)
        if not blocks or blocks[0] < 0 or blocks[-1] > 3:
            raise ValueError(f"InceptionV3: output_blocks {tuple(output_blocks)}: indices 0..3")
        super().__init__()
        self.resize_input = bool(resize_input)
        self.normalize_input = bool(normalize_input)
        self.output_blocks = blocks
        self.last_needed_block = blocks[-1]

    # -- weights ------------------------------------------------------------------------------------------------------
    def _held(self, state_dict):
        """Strict: either the .pth key set (torchvision Inception3 names, fc read and ignored) or the wrapper's own
        (blocks.*; what state_dict() returns, up to the last needed block).  num_batches_tracked may be absent throughout
        (torch's BatchNorm accepts checkpoints without it)."""
        wrapper = any(k.startswith("blocks.") for k in state_dict)
        spec = state_spec(wrapper, self.last_needed_block if wrapper else 3)
        convnet.check_state_dict(state_dict, {k: shape for k, (shape, _) in spec.items()}, "InceptionV3",
                                 optional=[k for k in spec if k.endswith("num_batches_tracked")])
        # held under the wrapper's names, as the reference's InceptionV3 holds them
        L = self.last_needed_block
        own = [p for p, _ in _convs_with_keys(True, L)]
        src = own if wrapper else [p for p, _ in _convs_with_keys(False, L)]
        sd = OrderedDict()
        for o, i in zip(own, src):
            for s in ("conv.weight",) + tuple(f"bn.{b}" for b in BN_KEYS):
                if f"{i}.{s}" in state_dict:
                    sd[f"{o}.{s}"] = state_dict[f"{i}.{s}"].detach().cpu().clone()
        return sd

    def _pack(self, sd, device: torch.device) -> dict:
        packed = {}

        def put(key, w64, b64):
            packed[key] = (pack_conv_weight(w64.unsqueeze(2)).to(device), b64.float().to(device))

        index = {0: 0, 1: 0, 2: 0, 3: 0}
        for blk, mname, kind, convs in NET:
            if blk > self.last_needed_block:
                break
            base = f"blocks.{blk}.{index[blk]}"
            index[blk] += 1
            if kind == "pool":
                continue
            if kind == "conv":
                put(mname, *fold_bn(sd, base))
                continue
            fused = FUSED_1X1[kind]
            f = [fold_bn(sd, f"{base}.{n}") for n in fused]
            put(f"{mname}.1x1", torch.cat([a for a, _ in f]), torch.cat([b for _, b in f]))
            for c in convs:
                if c[0] not in fused:
                    put(f"{mname}.{c[0]}", *fold_bn(sd, f"{base}.{c[0]}"))
        return packed

    # -- forward ------------------------------------------------------------------------------------------------------
    def _module(self, x: torch.Tensor, name: str, kind: str, convs, pk: dict) -> torch.Tensor:
        N, H, W, cin = x.shape
        c = {cv[0]: cv for cv in convs}
        new = lambda h, w, ch: torch.empty((N, h, w, ch), device=x.device, dtype=torch.float32)  # noqa: E731

        def run(src, cname, out, out_off, x_off=0, cin_=None):
            cv = c[cname]
            return conv2d(src, *pk[f"{name}.{cname}"], cv[3], cv[4], cv[5], cin=cin_, x_off=x_off, out=out,
                          out_off=out_off)

        if kind == "A":
            pf = c["branch_pool"][2]
            y, mid = new(H, W, 224 + pf), new(H, W, 48 + 64)
            conv2d(x, *pk[f"{name}.1x1"], (1, 1), out=y, out_off=0, out2=mid, out2_off=0, split=64)
            run(mid, "branch5x5_2", y, 64, 0, 48)
            t = run(mid, "branch3x3dbl_2", None, 0, 48, 64)
            run(t, "branch3x3dbl_3", y, 128)
            run(avgpool2d(x, 3, 1, 1), "branch_pool", y, 224)
            return y
        if kind == "B":
            Ho, Wo = out_size(H, 3, 2, 0), out_size(W, 3, 2, 0)
            y = new(Ho, Wo, 384 + 96 + cin)
            run(x, "branch3x3", y, 0)
            t = conv2d(x, *pk[f"{name}.1x1"], (1, 1))
            t = run(t, "branch3x3dbl_2", None, 0)
            run(t, "branch3x3dbl_3", y, 384)
            maxpool2d(x, 3, 2, 0, out=y, out_off=480)
            return y
        if kind == "C":
            c7 = c["branch7x7_1"][2]
            y, mid = new(H, W, 768), new(H, W, 2 * c7)
            conv2d(x, *pk[f"{name}.1x1"], (1, 1), out=y, out_off=0, out2=mid, out2_off=0, split=192)
            t = run(mid, "branch7x7_2", None, 0, 0, c7)
            run(t, "branch7x7_3", y, 192)
            t = run(mid, "branch7x7dbl_2", None, 0, c7, c7)
            t = run(t, "branch7x7dbl_3", None, 0)
            t = run(t, "branch7x7dbl_4", None, 0)
            run(t, "branch7x7dbl_5", y, 384)
            run(avgpool2d(x, 3, 1, 1), "branch_pool", y, 576)
            return y
        if kind == "D":
            Ho, Wo = out_size(H, 3, 2, 0), out_size(W, 3, 2, 0)
            y = new(Ho, Wo, 320 + 192 + cin)
            mid = conv2d(x, *pk[f"{name}.1x1"], (1, 1))
            run(mid, "branch3x3_2", y, 0, 0, 192)
            t = run(mid, "branch7x7x3_2", None, 0, 192, 192)
            t = run(t, "branch7x7x3_3", None, 0)
            run(t, "branch7x7x3_4", y, 320)
            maxpool2d(x, 3, 2, 0, out=y, out_off=512)
            return y
        # E_1 / E_2
        y, mid = new(H, W, 2048), new(H, W, 384 + 448)
        conv2d(x, *pk[f"{name}.1x1"], (1, 1), out=y, out_off=0, out2=mid, out2_off=0, split=320)
        run(mid, "branch3x3_2a", y, 320, 0, 384)
        run(mid, "branch3x3_2b", y, 704, 0, 384)
        t = run(mid, "branch3x3dbl_2", None, 0, 384, 448)
        run(t, "branch3x3dbl_3a", y, 1088)
        run(t, "branch3x3dbl_3b", y, 1472)
        pooled = avgpool2d(x, 3, 1, 1) if kind == "E1" else maxpool2d(x, 3, 1, 1)
        run(pooled, "branch_pool", y, 1856)
        return y

    def features(self, x: torch.Tensor, endpoints: Optional[dict] = None) -> List[torch.Tensor]:
        """channels-last network input [N, H, W, 4] (channel 3 zero; what preprocess_images writes) -> the requested
        blocks' outputs, channels-last [N, h, w, C] (block 3: [N, 1, 1, 2048]).  `endpoints`, if a dict, receives every
        layer's output."""
        pk = self._weights(x.device)
        outs = []
        for blk, name, kind, convs in NET:
            if blk > self.last_needed_block:
                break
            if kind == "conv":
                _, _, _, k, s, p = convs[0]
                x = conv2d(x, *pk[name], k, s, p)
            elif kind == "pool":
                x = maxpool2d(x, 3, 2, 0)
            else:
                x = self._module(x, name, kind, convs, pk)
            if endpoints is not None:
                endpoints[name] = x
            last_of_block = name in ("maxpool1", "maxpool2", "Mixed_6e", "Mixed_7c")
            if last_of_block and blk in self.output_blocks:
                outs.append(spatial_mean(x).view(x.shape[0], 1, 1, -1) if blk == 3 else x)
        return outs

    def forward_channels_last(self, x: torch.Tensor) -> List[torch.Tensor]:
        if x.device.type != "cuda":
            raise RuntimeError(f"InceptionV3: input on {x.device}: the network runs on the GPU (there is no CPU path)")
        if x.dtype != torch.float32 or x.dim() != 4 or x.shape[3] != 4:
            raise ValueError(f"InceptionV3: expected float32 [N, H, W, 4], got {x.dtype} {tuple(x.shape)}")
        check_input_size(x.shape[1], x.shape[2], self.last_needed_block)
        with torch.cuda.device(x.device):
            chunks = [self.features(x[i:i + MAX_CHUNK].contiguous()) for i in range(0, x.shape[0], MAX_CHUNK)]
        if len(chunks) == 1:
            return chunks[0]
        return [torch.cat([c[j] for c in chunks]) for j in range(len(self.output_blocks))]

    def forward(self, inp: torch.Tensor) -> List[torch.Tensor]:
        """inp [N, 3, H, W] fp32 on the GPU, values in [0, 1] -> [N, C, h, w] per block in output_blocks (channels-last
        views; block 3 is [N, 2048, 1, 1])"""
        if not isinstance(inp, torch.Tensor) or inp.dim() != 4 or inp.shape[1] != 3:
            raise ValueError(f"InceptionV3: expected [N, 3, H, W], got {getattr(inp, 'shape', type(inp))}")
        if inp.dtype != torch.float32:
            raise TypeError(f"InceptionV3: dtype {inp.dtype}, expected torch.float32")
        if not self.resize_input:
            check_input_size(inp.shape[2], inp.shape[3], self.last_needed_block)
        if inp.device.type != "cuda":
            raise RuntimeError(f"InceptionV3: input on {inp.device}: the network runs on the GPU (there is no CPU path)")
        x = preprocess_images(inp, self.resize_input, self.normalize_input)
        return [o.permute(0, 3, 1, 2) for o in self.forward_channels_last(x)]
