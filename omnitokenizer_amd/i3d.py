"""InceptionI3d on the device: the reference's fvd/pytorch_i3d.py network (the feature net of FVD), its state_dict and its
logits, with every layer in csrc/i3d.hip (include/omnitok.h "I3D").  The conv and pool operators and the weight scaffold are
convnet.py's, shared with inception.py and lpips.py.

    i3d = InceptionI3d(400, in_channels=3)
    i3d.load_state_dict(torch.load("i3d_pretrained_400.pt"))      # strict: the reference's keys and shapes
    logits = i3d(x.cuda())                                          # x [B, 3, T, H, W] fp32 in [-1, 1] -> [B, 400]

At load time every BatchNorm (eps 1e-5) is folded into its conv in fp64 (w * g / sqrt(v + eps), b - m * g / sqrt(v + eps)),
rounded to fp32 and packed in the layout omnitok_conv3d_same reads.  A forward is ~55 launches per chunk of at most
MAX_CHUNK clips, on channels-last activations [B, T, H, W, C]:
  Conv3d_1a .. Conv3d_2c   omnitok::conv3d_same, omnitok::maxpool3d_same
  Mixed_*                  b0 | b1a | b2a as ONE 1x1x1 GEMM (b0 straight into the concat, b1a | b2a into a scratch tensor),
                           b1b and b2b from channel slices of that scratch, b3a pool then b3b; every branch writes its own
                           channel slice of the module output, so the concat costs nothing
  Logits                   omnitok::i3d_head (AvgPool3d [2, 7, 7], the logits conv with bias, the mean over time)
Each output element is a fixed-order fp32 sum, so a clip gets the same logits alone and in any batch.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import List, Optional, Tuple

import torch

from . import _lib, convnet
from ._lib import check, ptr, stream
from .convnet import conv3d_same, maxpool3d_same, pack_conv_weight, same_pad

MAX_CHUNK = 16   # clips per pass through the network (fvd.py MAX_BATCH): bounds the activations to ~0.9 GB at T = 17
BN_EPS = 1e-5

# (name, in_channels, [b0, b1a, b1b, b2a, b2b, b3b] output channels), pytorch_i3d.py:226-270
MIXED = {
    "Mixed_3b": (192, [64, 96, 128, 16, 32, 32]),
    "Mixed_3c": (256, [128, 128, 192, 32, 96, 64]),
    "Mixed_4b": (480, [192, 96, 208, 16, 48, 64]),
    "Mixed_4c": (512, [160, 112, 224, 24, 64, 64]),
    "Mixed_4d": (512, [128, 128, 256, 24, 64, 64]),
    "Mixed_4e": (512, [112, 144, 288, 32, 64, 64]),
    "Mixed_4f": (528, [256, 160, 320, 32, 128, 128]),
    "Mixed_5b": (832, [256, 160, 320, 32, 128, 128]),
    "Mixed_5c": (832, [384, 192, 384, 48, 128, 128]),
}
# the network in order: ("unit", name, cin, cout, kernel, stride) | ("pool", name, kernel, stride) | ("mixed", name)
PLAN = [
    ("unit", "Conv3d_1a_7x7", 3, 64, (7, 7, 7), (2, 2, 2)),
    ("pool", "MaxPool3d_2a_3x3", (1, 3, 3), (1, 2, 2)),
    ("unit", "Conv3d_2b_1x1", 64, 64, (1, 1, 1), (1, 1, 1)),
    ("unit", "Conv3d_2c_3x3", 64, 192, (3, 3, 3), (1, 1, 1)),
    ("pool", "MaxPool3d_3a_3x3", (1, 3, 3), (1, 2, 2)),
    ("mixed", "Mixed_3b"), ("mixed", "Mixed_3c"),
    ("pool", "MaxPool3d_4a_3x3", (3, 3, 3), (2, 2, 2)),
    ("mixed", "Mixed_4b"), ("mixed", "Mixed_4c"), ("mixed", "Mixed_4d"), ("mixed", "Mixed_4e"), ("mixed", "Mixed_4f"),
    ("pool", "MaxPool3d_5a_2x2", (2, 2, 2), (2, 2, 2)),
    ("mixed", "Mixed_5b"), ("mixed", "Mixed_5c"),
]
ENDPOINTS = [p[1] for p in PLAN] + ["Logits"]
LOGITS_IN = 384 + 384 + 128 + 128


def mixed_units(name: str) -> List[Tuple[str, int, int, int]]:
    """(unit name, cin, cout, kernel size) of the six convs of an Inception module, in the reference's module order"""
    cin, c = MIXED[name]
    return [(f"{name}.b0", cin, c[0], 1), (f"{name}.b1a", cin, c[1], 1), (f"{name}.b1b", c[1], c[2], 3),
            (f"{name}.b2a", cin, c[3], 1), (f"{name}.b2b", c[3], c[4], 3), (f"{name}.b3b", cin, c[5], 1)]


def units() -> List[Tuple[str, int, int, Tuple[int, int, int], Tuple[int, int, int]]]:
    """every Unit3D with BatchNorm and ReLU: (name, cin, cout, kernel, stride), in state_dict order"""
    out = []
    for p in PLAN:
        if p[0] == "unit":
            out.append(p[1:])
        elif p[0] == "mixed":
            out += [(n, ci, co, (k, k, k), (1, 1, 1)) for n, ci, co, k in mixed_units(p[1])]
    return out


def state_spec(num_classes: int = 400) -> "OrderedDict[str, Tuple[Tuple[int, ...], torch.dtype]]":
    """key -> (shape, dtype) of the reference's state_dict, in its order (the logits Unit3D is registered first)"""
    spec = OrderedDict()
    spec["logits.conv3d.weight"] = ((num_classes, LOGITS_IN, 1, 1, 1), torch.float32)
    spec["logits.conv3d.bias"] = ((num_classes,), torch.float32)
    for name, cin, cout, k, _ in units():
        spec[f"{name}.conv3d.weight"] = ((cout, cin) + tuple(k), torch.float32)
        for s in ("weight", "bias", "running_mean", "running_var"):
            spec[f"{name}.bn.{s}"] = ((cout,), torch.float32)
        spec[f"{name}.bn.num_batches_tracked"] = ((), torch.int64)
    return spec


def final_grid(T: int, H: int, W: int) -> Tuple[int, int, int]:
    """the extent of Mixed_5c's output (what the [2, 7, 7] average pool sees) for a [T, H, W] input"""
    ext = [T, H, W]
    for p in PLAN:
        if p[0] == "mixed":
            continue
        k, s = (p[4], p[5]) if p[0] == "unit" else (p[2], p[3])
        ext = [same_pad(e, kk, ss)[1] for e, kk, ss in zip(ext, k, s)]
    return tuple(ext)


def check_input_size(T: int, H: int, W: int):
    """ValueError where the reference's AvgPool3d([2, 7, 7]) would fail, with the least size that works"""
    t, h, w = final_grid(T, H, W)
    if t < 2:
        raise ValueError(f"I3D needs at least 9 frames (the final grid has {t} time steps for T = {T}; the [2, 7, 7] "
                         "average pool needs 2)")
    if h < 7 or w < 7:
        raise ValueError(f"I3D needs frames of at least 193 x 193 (the final grid is {h} x {w} for {H} x {W}; the "
                         "[2, 7, 7] average pool needs 7 x 7)")


# ---- the two operators of I3D alone (the conv and the pool are convnet.py's) --------------------------------------------

def _preprocess_native(frames: torch.Tensor, R_h: int, R_w: int) -> torch.Tensor:
    B, T, H, W, _ = frames.shape
    out = torch.empty((B, T, R_h, R_w, 4), device=frames.device, dtype=torch.float32)
    check(_lib.load().omnitok_i3d_preprocess(ptr(frames), B, T, H, W, R_h, R_w, ptr(out), stream()), "i3d_preprocess")
    return out


def _head_native(x: torch.Tensor, w_t: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    B, T, H, W, C = x.shape
    ncls = w_t.shape[1]
    out = torch.empty((B, ncls, H - 6, W - 6), device=x.device, dtype=torch.float32)
    check(_lib.load().omnitok_i3d_head(ptr(x), B, T, H, W, C, ptr(w_t), ptr(bias), ncls, ptr(out), stream()), "i3d_head")
    return out


def _register_ops():
    from torch.library import custom_op

    @custom_op("omnitok::i3d_preprocess", mutates_args=(), device_types="cuda")
    def _pre(frames: torch.Tensor, R_h: int, R_w: int) -> torch.Tensor:
        if frames.dtype != torch.uint8 or frames.dim() != 5 or frames.shape[4] != 3:
            raise ValueError(f"i3d_preprocess: frames must be uint8 [B, T, H, W, 3], got {frames.dtype} "
                             f"{tuple(frames.shape)}")
        return _preprocess_native(frames.contiguous(), R_h, R_w)

    @_pre.register_fake
    def _(frames, R_h, R_w):
        return frames.new_empty((frames.shape[0], frames.shape[1], R_h, R_w, 4), dtype=torch.float32)

    @custom_op("omnitok::i3d_head", mutates_args=(), device_types="cuda")
    def _head(x: torch.Tensor, w_t: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
        if x.dtype != torch.float32 or x.dim() != 5 or w_t.dim() != 2 or w_t.shape[0] != x.shape[4]:
            raise ValueError(f"i3d_head: x [B, T, H, W, C] float32 and w_t [C, classes], got {tuple(x.shape)} and "
                             f"{tuple(w_t.shape)}")
        return _head_native(x.contiguous(), w_t.contiguous(), bias.contiguous())

    @_head.register_fake
    def _(x, w_t, bias):
        return x.new_empty((x.shape[0], w_t.shape[1], x.shape[2] - 6, x.shape[3] - 6))


_register_ops()


def preprocess_frames(frames: torch.Tensor, size: Tuple[int, int] = (224, 224)) -> torch.Tensor:
    """uint8 [B, T, H, W, 3] on the GPU -> fp32 [B, T, size, 4] channels-last (channel 3 zero): fvd.py preprocess"""
    return torch.ops.omnitok.i3d_preprocess(frames, int(size[0]), int(size[1]))


def i3d_head(x: torch.Tensor, w_t: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    return torch.ops.omnitok.i3d_head(x, w_t, bias)


def fold_bn(sd, name: str) -> Tuple[torch.Tensor, torch.Tensor]:
    """(weight, bias) of Unit3D `name` with its BatchNorm folded in, in fp64"""
    return convnet.fold_bn(sd, name, "conv3d", BN_EPS)


class InceptionI3d(convnet.PackedWeights):
    """The reference's InceptionI3d (fvd/pytorch_i3d.py) for its FVD use: constructor arguments, state_dict keys and
    forward logits as there, on the GPU.  is_coinrun, other final endpoints, spatial_squeeze=False (the reference's forward
    fails on it) and in_channels != 3 are not provided."""

    VALID_ENDPOINTS = tuple(ENDPOINTS) + ("Predictions",)

    def __init__(self, num_classes=400, spatial_squeeze=True, final_endpoint="Logits", name="inception_i3d",
                 in_channels=3, dropout_keep_prob=0.5, is_coinrun=False):
        if final_endpoint not in self.VALID_ENDPOINTS:
            raise ValueError("Unknown final endpoint %s" % final_endpoint)
        if is_coinrun:
            raise NotImplementedError("InceptionI3d: is_coinrun=True (the coinrun strides) is not provided")
        if final_endpoint != "Logits":
            raise NotImplementedError(f"InceptionI3d: final_endpoint {final_endpoint!r}: only 'Logits' is provided")
        if in_channels != 3:
            raise NotImplementedError(f"InceptionI3d: in_channels {in_channels}: only 3 is provided")
        if not spatial_squeeze:
            raise NotImplementedError("InceptionI3d: spatial_squeeze=False (the reference's forward fails on it)")
        super().__init__()
        self._num_classes = int(num_classes)

    # -- weights ------------------------------------------------------------------------------------------------------
    def _held(self, state_dict):
        spec = state_spec(self._num_classes)
        convnet.check_state_dict(state_dict, {k: shape for k, (shape, _) in spec.items()}, "InceptionI3d")
        return OrderedDict((k, state_dict[k].detach().cpu().clone()) for k in spec)

    def _pack(self, sd, device: torch.device) -> dict:
        packed = {}

        def put(name, w64, b64):
            packed[name] = (pack_conv_weight(w64).to(device), b64.float().to(device))

        for p in PLAN:
            if p[0] == "unit":
                put(p[1], *fold_bn(sd, p[1]))
            elif p[0] == "mixed":
                u = {n.split(".")[1]: fold_bn(sd, n) for n, *_ in mixed_units(p[1])}
                put(p[1] + ".1x1", torch.cat([u["b0"][0], u["b1a"][0], u["b2a"][0]]),
                    torch.cat([u["b0"][1], u["b1a"][1], u["b2a"][1]]))
                for b in ("b1b", "b2b", "b3b"):
                    put(f"{p[1]}.{b}", *u[b])
        w = sd["logits.conv3d.weight"].reshape(self._num_classes, LOGITS_IN)
        packed["logits"] = (w.t().contiguous().float().to(device), sd["logits.conv3d.bias"].float().to(device))
        return packed

    # -- forward ------------------------------------------------------------------------------------------------------
    def _mixed(self, x: torch.Tensor, name: str, pk: dict) -> torch.Tensor:
        cin, c = MIXED[name]
        B, T, H, W, _ = x.shape
        y = torch.empty((B, T, H, W, c[0] + c[2] + c[4] + c[5]), device=x.device, dtype=torch.float32)
        mid = torch.empty((B, T, H, W, c[1] + c[3]), device=x.device, dtype=torch.float32)
        conv3d_same(x, *pk[name + ".1x1"], (1, 1, 1), out=y, out_off=0, out2=mid, out2_off=0, split=c[0])
        conv3d_same(mid, *pk[name + ".b1b"], (3, 3, 3), cin=c[1], x_off=0, out=y, out_off=c[0])
        conv3d_same(mid, *pk[name + ".b2b"], (3, 3, 3), cin=c[3], x_off=c[1], out=y, out_off=c[0] + c[2])
        pooled = maxpool3d_same(x, (3, 3, 3), (1, 1, 1))
        conv3d_same(pooled, *pk[name + ".b3b"], (1, 1, 1), out=y, out_off=c[0] + c[2] + c[4])
        return y

    def features(self, x: torch.Tensor, endpoints: Optional[dict] = None) -> torch.Tensor:
        """channels-last [B, T, H, W, 4] (channel 3 zero) -> Mixed_5c's output [B, T', H', W', 1024]; `endpoints`, if a
        dict, receives every endpoint's output"""
        pk = self._weights(x.device)
        for p in PLAN:
            if p[0] == "unit":
                x = conv3d_same(x, *pk[p[1]], p[4], p[5])
            elif p[0] == "pool":
                x = maxpool3d_same(x, p[2], p[3])
            else:
                x = self._mixed(x, p[1], pk)
            if endpoints is not None:
                endpoints[p[1]] = x
        return x

    def forward_channels_last(self, x: torch.Tensor) -> torch.Tensor:
        """[B, T, H, W, 4] fp32 (channel 3 zero; what preprocess_frames writes) -> the reference's logits"""
        if x.device.type != "cuda":
            raise RuntimeError(f"InceptionI3d: input on {x.device}: the network runs on the GPU (there is no CPU path)")
        if x.dtype != torch.float32 or x.dim() != 5 or x.shape[4] != 4:
            raise ValueError(f"InceptionI3d: expected float32 [B, T, H, W, 4], got {x.dtype} {tuple(x.shape)}")
        B, T, H, W, _ = x.shape
        check_input_size(T, H, W)
        with torch.cuda.device(x.device):
            outs = []
            for i in range(0, B, MAX_CHUNK):
                f = self.features(x[i:i + MAX_CHUNK].contiguous())
                outs.append(i3d_head(f, *self._weights(x.device)["logits"]))
            out = torch.cat(outs) if outs else torch.empty((0, self._num_classes, 1, 1), device=x.device)
        # the reference: logits [B, C, T'', h, w] -> squeeze(3).squeeze(3) -> mean over T'' (done in the head)
        if out.shape[2] == 1:
            out = out.squeeze(2)
            if out.shape[2] == 1:
                out = out.squeeze(2)
        return out

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x [B, 3, T, H, W] fp32 on the GPU (the reference's input, [-1, 1]) -> logits [B, num_classes] ([B, num_classes,
        h', w'] when the final grid is larger than 7 x 7, as in the reference)"""
        if not isinstance(x, torch.Tensor) or x.dim() != 5 or x.shape[1] != 3:
            raise ValueError(f"InceptionI3d: expected [B, 3, T, H, W], got {getattr(x, 'shape', type(x))}")
        if x.dtype != torch.float32:
            raise TypeError(f"InceptionI3d: dtype {x.dtype}, expected torch.float32")
        if x.device.type != "cuda":
            raise RuntimeError(f"InceptionI3d: input on {x.device}: the network runs on the GPU (there is no CPU path)")
        check_input_size(*x.shape[2:])
        xl = torch.nn.functional.pad(x.permute(0, 2, 3, 4, 1), (0, 1))   # channels-last, channel 3 = 0
        return self.forward_channels_last(xl.contiguous())
