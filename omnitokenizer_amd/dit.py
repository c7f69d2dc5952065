"""DiT denoiser on the MI355X: the inference-only counterpart of the reference's Diffusion/DiT/models.py `DiT`
(include/omnitok_dit.h, csrc/dit_*.hip).

    from omnitokenizer_amd.dit import DiT_models, load_dit
    model = DiT_models["DiT-XL/2"](input_size=32, in_channels=8, num_classes=1000).cuda()
    model.load_state_dict(load_dit("DiT-XL-2.pt"))          # download.find_model's checkpoint["ema"] rule
    eps_sigma = model.forward_with_cfg(x, t, y, cfg_scale=4.0)

The module holds the reference's parameter names, so its checkpoints load unchanged; the forward pass runs on the library's
engine (fp32 throughout by default; there is no PyTorch fallback).  Training, label dropout and fractional timesteps are not built.

    model.set_linear_format("bf16")     # opt-in: the four linears of every block on the 16-bit MFMA ("fp32" | "bf16" | "fp16")
    model.set_attention_format("bf16")  # opt-in: Q . K^T and P . V of every block's attention on the 16-bit MFMA (the same three)
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._lib import OmnitokDitConfig, check

LINEAR_FORMATS = {"fp32": 0, "bf16": 1, "fp16": 2}  # OMNITOK_DIT_LIN_* (include/omnitok_dit.h)
ATTENTION_FORMATS = LINEAR_FORMATS  # OMNITOK_DIT_ATTN_*: the same codes under a second name
FREQUENCY_EMBEDDING_SIZE = 256  # TimestepEmbedder's default (models.py:31), the only one the reference uses


class _Holder(nn.Module):
    """Parameter container that reproduces the reference's module nesting (names only)."""

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("parameter container, not callable")


class _Lin(_Holder):
    def __init__(self, out_f, in_f):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(out_f, in_f), requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(out_f), requires_grad=False)


def _seq(*mods):
    """nn.Sequential-style numbering (keys `0`, `1`, ...) over holders; None leaves the index empty (an activation)."""
    h = _Holder()
    for i, m in enumerate(mods):
        if m is not None:
            h.add_module(str(i), m)
    return h


def get_2d_sincos_pos_embed(embed_dim: int, grid_size: int) -> np.ndarray:
    """The fixed sin-cos position table of models.py:274-321 (MAE's): [grid_size^2, embed_dim] in fp64.  The w coordinate goes
    first; each coordinate's half is sin | cos over 1 / 10000^(2i / (embed_dim / 2))."""
    if embed_dim % 4:
        raise ValueError("embed_dim must be a multiple of 4")
    gh = np.arange(grid_size, dtype=np.float32)
    grid = np.stack(np.meshgrid(gh, gh), axis=0).reshape(2, -1)

    def one(pos):
        omega = 1.0 / 10000 ** (np.arange(embed_dim // 4, dtype=np.float64) / (embed_dim / 4.0))
        out = np.einsum("m,d->md", pos, omega)
        return np.concatenate([np.sin(out), np.cos(out)], axis=1)

    return np.concatenate([one(grid[0]), one(grid[1])], axis=1)


def timestep_frequencies() -> torch.Tensor:
    """freqs of TimestepEmbedder.timestep_embedding (models.py:51-54), evaluated by this torch on the CPU exactly as written
    there: the engine multiplies these by t in fp32 and takes cos / sin in fp64 (omnitok_dit_set_frequencies)."""
    half = FREQUENCY_EMBEDDING_SIZE // 2
    return torch.exp(-math.log(10000) * torch.arange(start=0, end=half, dtype=torch.float32) / half)


class DiT(nn.Module):
    """models.py:145-266, inference only.  Same constructor, same state_dict keys, same forward / forward_with_cfg."""

    _API = "dit"  # the engine's C prefix: omnitok_dit_create, ... (the Latte subclass of omnitokenizer_amd.latte runs omnitok_latte_*)
    _TOKEN_DROP_REF = "models.py:78-94"

    def __init__(self, input_size=32, patch_size=2, in_channels=4, hidden_size=1152, depth=28, num_heads=16, mlp_ratio=4.0,
                 class_dropout_prob=0.1, num_classes=1000, learn_sigma=True):
        super().__init__()
        mlp_hidden = int(hidden_size * mlp_ratio)
        cfg = OmnitokDitConfig(input_size, patch_size, in_channels, hidden_size, depth, num_heads, mlp_hidden, num_classes,
                               float(class_dropout_prob), int(bool(learn_sigma)))
        self._build(cfg, label_rows=num_classes + (1 if class_dropout_prob > 0 else 0))

    def _fn(self, name):
        return getattr(_lib.load(), f"omnitok_{self._API}_{name}")

    def _build(self, cfg, label_rows):
        """The attributes and parameter holders of the reference's module from the engine's config struct; label_rows None: a
        model without y_embedder."""
        self._cfg = cfg
        input_size, patch_size, in_channels, D, depth = cfg.input_size, cfg.patch_size, cfg.in_channels, cfg.hidden, cfg.depth
        self.learn_sigma = bool(cfg.learn_sigma)
        self.in_channels = in_channels
        self.out_channels = in_channels * 2 if self.learn_sigma else in_channels
        self.patch_size = patch_size
        self.num_heads = cfg.heads
        self.input_size = input_size
        self.hidden_size = D
        self.depth = depth
        self.mlp_hidden = cfg.mlp_hidden
        self.num_classes = cfg.num_classes
        self.class_dropout_prob = float(cfg.class_dropout)
        # the configuration is checked where the engine checks it (no GPU needed): an unsupported model fails here
        probe = ctypes.c_void_p()
        check(self._fn("create")(ctypes.byref(self._cfg), ctypes.byref(probe)), f"{self._API}_create")
        self._fn("destroy")(probe)
        n_tok = (input_size // patch_size) ** 2

        self.x_embedder = _Holder()
        self.x_embedder.proj = _Holder()
        self.x_embedder.proj.weight = nn.Parameter(torch.zeros(D, in_channels, patch_size, patch_size), requires_grad=False)
        self.x_embedder.proj.bias = nn.Parameter(torch.zeros(D), requires_grad=False)
        self.t_embedder = _Holder()
        self.t_embedder.mlp = _seq(_Lin(D, FREQUENCY_EMBEDDING_SIZE), None, _Lin(D, D))
        if label_rows is not None:
            self.y_embedder = _Holder()
            self.y_embedder.embedding_table = _Holder()
            self.y_embedder.embedding_table.weight = nn.Parameter(torch.zeros(label_rows, D), requires_grad=False)
        self.pos_embed = nn.Parameter(torch.from_numpy(get_2d_sincos_pos_embed(D, input_size // patch_size)).float().unsqueeze(0),
                                      requires_grad=False)
        assert self.pos_embed.shape == (1, n_tok, D)
        blocks = []
        for _ in range(depth):
            b = _Holder()
            b.attn = _Holder()
            b.attn.qkv, b.attn.proj = _Lin(3 * D, D), _Lin(D, D)
            b.mlp = _Holder()
            b.mlp.fc1, b.mlp.fc2 = _Lin(self.mlp_hidden, D), _Lin(D, self.mlp_hidden)
            b.adaLN_modulation = _seq(None, _Lin(6 * D, D))
            blocks.append(b)
        self.blocks = nn.ModuleList(blocks)
        self.final_layer = _Holder()
        self.final_layer.linear = _Lin(patch_size * patch_size * self.out_channels, D)
        self.final_layer.adaLN_modulation = _seq(None, _Lin(2 * D, D))
        self._engine = None
        self._engine_sig = None
        self._linear_format = "fp32"
        self._attention_format = "fp32"
        nn.Module.train(self, False)

    # ---- plumbing ---------------------------------------------------------------------------------
    @property
    def device(self):
        return self.pos_embed.device

    @property
    def linear_format(self) -> str:
        """The format of the block linears: "fp32" (the default), "bf16" or "fp16" (set_linear_format)."""
        return self._linear_format

    def set_linear_format(self, fmt: str):
        """Runs attn.qkv, attn.proj, mlp.fc1 and mlp.fc2 of every block on the 16-bit MFMA: weights and the linears' inputs rounded
        once to `fmt`, exact products, fp32 accumulators; everything else stays fp32 (omnitok_dit_set_linear_format).  This is not
        the reference's use_fp16, which casts the whole module.  Takes effect at the next forward; "fp32" restores the default
        bit for bit.  Under "fp16" a weight outside the fp16 range fails the next forward and an activation outside it fails
        check_range()."""
        if fmt not in LINEAR_FORMATS:
            raise ValueError(f"linear format {fmt!r}: one of {', '.join(LINEAR_FORMATS)}")
        if fmt != self._linear_format:
            self._linear_format = fmt
            self._engine_sig = None  # the next forward re-finalizes
        return self

    @property
    def attention_format(self) -> str:
        """The format of the attention's operands: "fp32" (the default), "bf16" or "fp16" (set_attention_format)."""
        return self._attention_format

    def set_attention_format(self, fmt: str):
        """Runs Q . K^T and P . V of every block's attention (Latte: of the spatial blocks; the temporal attention stays fp32) on the
        16-bit MFMA: q, k, v and the softmax weights rounded once to `fmt`, exact products, fp32 accumulators, softmax statistics in
        fp32 (omnitok_dit_set_attention_format).  Independent of the linear format; with both 16-bit the attention writes attn.proj's
        packed operand itself.  These are the operands of one kernel, not the reference's use_fp16.  No weight depends on it: an
        existing engine takes it at once, without a re-upload; "fp32" restores the default bit for bit.  Under "fp16" a q, k or v
        outside the fp16 range fails check_range()."""
        if fmt not in ATTENTION_FORMATS:
            raise ValueError(f"attention format {fmt!r}: one of {', '.join(ATTENTION_FORMATS)}")
        self._attention_format = fmt
        if self._engine is not None:
            check(self._fn("set_attention_format")(self._engine, ATTENTION_FORMATS[fmt]), f"{self._API}_set_attention_format")
        return self

    def train(self, mode: bool = True):
        if mode:
            raise NotImplementedError(f"omnitokenizer_amd {type(self).__name__} is inference-only: training and the label dropout "
                                      f"of LabelEmbedder.token_drop ({self._TOKEN_DROP_REF}) are not built")
        return super().train(False)

    def __del__(self):
        try:
            if self._engine is not None:
                self._fn("destroy")(self._engine)
        except Exception:
            pass

    def engine_missing(self):
        """The state_dict keys the engine of this configuration still waits for (all of them before the first forward)."""
        h = self._engine
        own = h is None
        if own:
            h = ctypes.c_void_p()
            check(self._fn("create")(ctypes.byref(self._cfg), ctypes.byref(h)), f"{self._API}_create")
        try:
            buf = ctypes.create_string_buffer(1 << 20)
            n = check(self._fn("missing")(h, buf, len(buf)), f"{self._API}_missing")
            names = buf.value.decode().split("\n") if n else []
        finally:
            if own:
                self._fn("destroy")(h)
        return names

    def _signature(self):
        return tuple((t.data_ptr(), t._version) for t in self.state_dict(keep_vars=True).values())

    def _sync_engine(self):
        dev = self.device
        if dev.type != "cuda":
            raise RuntimeError(f"{type(self).__name__} is on {dev}: move it to the GPU (.to('cuda')). The MI355X HIP path is the only "
                               "implementation; there is no CPU fallback.")
        sig = self._signature()
        if self._engine is not None and sig == self._engine_sig:
            return
        api = self._API
        stream = torch.cuda.current_stream().cuda_stream
        if self._engine is None:
            h = ctypes.c_void_p()
            check(self._fn("create")(ctypes.byref(self._cfg), ctypes.byref(h)), f"{api}_create")
            self._engine = h
            fr = timestep_frequencies().contiguous()
            check(self._fn("set_frequencies")(self._engine, ctypes.c_void_p(fr.data_ptr()), fr.numel()), f"{api}_set_frequencies")
        for name, t in self.state_dict(keep_vars=True).items():
            t = t.detach()
            if t.dtype != torch.float32:
                raise TypeError(f"{name}: parameters must be float32 (the path computes in fp32)")
            t = t.contiguous()
            shape = (ctypes.c_int64 * max(t.dim(), 1))(*t.shape)
            check(self._fn("set_weight")(self._engine, name.encode(), ctypes.c_void_p(t.data_ptr()), shape, t.dim(), stream),
                  f"{api}_set_weight({name})")
        check(self._fn("set_linear_format")(self._engine, LINEAR_FORMATS[self._linear_format]), f"{api}_set_linear_format")
        check(self._fn("set_attention_format")(self._engine, ATTENTION_FORMATS[self._attention_format]), f"{api}_set_attention_format")
        check(self._fn("finalize")(self._engine, stream), f"{api}_finalize")
        torch.cuda.current_stream().synchronize()
        self._engine_sig = sig

    def _inputs(self, x, t, y):
        if x.dim() != 4 or tuple(x.shape[1:]) != (self.in_channels, self.input_size, self.input_size):
            raise ValueError(f"x must be [B,{self.in_channels},{self.input_size},{self.input_size}], got {tuple(x.shape)}")
        B = x.shape[0]
        if t.is_floating_point():
            raise NotImplementedError("fractional timesteps (models.py:44-45) are not supported: pass integer timesteps")
        if tuple(t.shape) != (B,) or tuple(y.shape) != (B,):
            raise ValueError(f"t and y must be [{B}]")
        for v in (x, t, y):
            if v.device != self.device:
                raise RuntimeError(f"input on {v.device}, model on {self.device}")
        return x.float().contiguous(), t.long().contiguous(), y.long().contiguous()

    def _run(self, x, t, y, cfg_scale, check_range):
        x, t, y = self._inputs(x, t, y)
        self._sync_engine()
        B = x.shape[0]
        out = torch.empty(*x.shape[:-3], self.out_channels, self.input_size, self.input_size, device=x.device, dtype=torch.float32)
        stream = torch.cuda.current_stream().cuda_stream
        P = ctypes.c_void_p
        yp = P(y.data_ptr()) if y is not None else None
        if cfg_scale is None:
            check(self._fn("forward")(self._engine, P(x.data_ptr()), P(t.data_ptr()), yp, B, P(out.data_ptr()), stream),
                  f"{self._API}_forward")
        else:
            check(self._fn("forward_cfg")(self._engine, P(x.data_ptr()), P(t.data_ptr()), yp, B, float(cfg_scale), P(out.data_ptr()),
                                          stream), f"{self._API}_forward_cfg")
        if check_range:
            self.check_range()
        return out

    def check_range(self):
        """Raises ValueError if a forward since the last check saw a timestep outside [0, 1000), a label outside the embedding
        table or, under the "fp16" linear / attention format, an activation / a q, k or v outside the fp16 range (one int read-back:
        a host synchronisation)."""
        check(self._fn("check")(self._engine, torch.cuda.current_stream().cuda_stream), f"{self._API}_check")

    # ---- the reference's two entry points ------------------------------------------------------------
    @torch.no_grad()
    def forward(self, x, t, y, *, check_range: bool = True):
        """models.py:233-248: x [N,C,H,W], t [N] integer timesteps, y [N] labels -> [N,out_channels,H,W]."""
        return self._run(x, t, y, None, check_range)

    @torch.no_grad()
    def forward_with_cfg(self, x, t, y, cfg_scale, *, check_range: bool = True):
        """models.py:250-266, its three-channel guidance included."""
        return self._run(x, t, y, cfg_scale, check_range)


def _variant(depth, hidden_size, patch_size, num_heads):
    def make(**kwargs):
        return DiT(depth=depth, hidden_size=hidden_size, patch_size=patch_size, num_heads=num_heads, **kwargs)
    return make


DiT_models = {f"DiT-{n}/{p}": _variant(d, h, p, nh)
              for n, (d, h, nh) in {"XL": (28, 1152, 16), "L": (24, 1024, 16), "B": (12, 768, 12), "S": (12, 384, 6)}.items()
              for p in (2, 4, 8)}


def load_dit(path, map_location="cpu"):
    """download.find_model's rule for a checkpoint file (download.py:18-30): the `ema` weights of a train.py checkpoint when
    present, else the file's own state_dict.  Like the reference it unpickles the whole file (a train.py checkpoint carries its
    argparse Namespace): load only checkpoints you trust."""
    checkpoint = torch.load(path, map_location=map_location, weights_only=False)
    if isinstance(checkpoint, dict) and "ema" in checkpoint:
        checkpoint = checkpoint["ema"]
    return checkpoint
