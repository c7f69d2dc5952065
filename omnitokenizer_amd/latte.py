"""Latte video denoiser on the MI355X: the inference-only counterpart of the reference's Diffusion/Latte/models/latte.py `Latte`
(include/omnitok_latte.h, csrc/latte_*.hip).

    from omnitokenizer_amd.latte import Latte_models, load_latte
    model = Latte_models["Latte-XL/2-omnitokenizer"](input_size=32, num_frames=5, num_classes=101, extras=2).cuda()
    model.load_state_dict(load_latte("latte.pt"))            # find_model's rule: checkpoint["ema"], else ["model"], else ["state_dict"]
    eps_sigma = model.forward_with_cfg(x, t, y, cfg_scale=7.0)   # x [B,F,C,H,W] -> [B,F,2C,H,W]

The module holds the reference's parameter names, so its checkpoints load unchanged; the forward pass runs on the library's engine
(fp32 throughout by default, DiT.set_linear_format for 16-bit block linears and DiT.set_attention_format for 16-bit operands of
the spatial attention; there is no PyTorch fallback).  Built: extras 1 (unconditional) and 2 (class labels).  Not built: extras 78 (text
embeddings), use_fp16, training, fractional timesteps.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from ._lib import OmnitokLatteConfig
from .dit import DiT

_REF = "Diffusion/Latte/models/latte.py"


def get_1d_sincos_pos_embed_from_grid(embed_dim: int, pos) -> np.ndarray:
    """latte.py:444-462: sin | cos of pos / 10000^(2i / embed_dim), [len(pos), embed_dim] in fp64."""
    if embed_dim % 2:
        raise ValueError("embed_dim must be even")
    omega = np.arange(embed_dim // 2, dtype=np.float64)
    omega /= embed_dim / 2.
    omega = 1. / 10000 ** omega
    out = np.einsum("m,d->md", np.asarray(pos).reshape(-1), omega)
    return np.concatenate([np.sin(out), np.cos(out)], axis=1)


def get_1d_sincos_temp_embed(embed_dim: int, length: int) -> np.ndarray:
    """latte.py:411-413: the fixed temporal embedding of frames 0 .. length - 1, [length, embed_dim] in fp64."""
    return get_1d_sincos_pos_embed_from_grid(embed_dim, np.arange(0, length))


class Latte(DiT):
    """latte.py:209-403, inference only.  Same constructor, same state_dict keys, same forward / forward_with_cfg."""

    _API = "latte"
    _TOKEN_DROP_REF = "latte.py:142-151"

    def __init__(self, input_size=32, patch_size=2, in_channels=4, hidden_size=1152, depth=28, num_heads=16, mlp_ratio=4.0,
                 num_frames=16, class_dropout_prob=0.1, num_classes=1000, learn_sigma=True, extras=1, attention_mode="math"):
        nn.Module.__init__(self)
        if attention_mode not in ("math", "flash", "xformers"):
            raise NotImplementedError(f"attention_mode {attention_mode!r} ({_REF}:58-78)")
        self.attention_mode = attention_mode  # accepted: there is one attention, the library's
        self.extras = extras
        self.num_frames = num_frames
        cfg = OmnitokLatteConfig(input_size, patch_size, in_channels, hidden_size, depth, num_heads, int(hidden_size * mlp_ratio),
                                 num_classes, float(class_dropout_prob), int(bool(learn_sigma)), num_frames, extras)
        self._build(cfg, label_rows=num_classes + (1 if class_dropout_prob > 0 else 0) if extras == 2 else None)
        self.temp_embed = nn.Parameter(torch.from_numpy(get_1d_sincos_temp_embed(hidden_size, num_frames)).float().unsqueeze(0),
                                       requires_grad=False)

    def _inputs(self, x, t, y):
        want = (self.num_frames, self.in_channels, self.input_size, self.input_size)
        if x.dim() != 5 or tuple(x.shape[1:]) != want:
            raise ValueError(f"x must be [B,{','.join(map(str, want))}], got {tuple(x.shape)}")
        B = x.shape[0]
        if t.is_floating_point():
            raise NotImplementedError(f"fractional timesteps ({_REF}:103-121) are not supported: pass integer timesteps")
        if tuple(t.shape) != (B,):
            raise ValueError(f"t must be [{B}]")
        if self.extras == 2:
            if y is None or tuple(y.shape) != (B,):
                raise ValueError(f"y must be [{B}] (the model has extras == 2)")
            y = y.long().contiguous()
        else:
            y = None  # the reference ignores y without a y_embedder (latte.py:341-357)
        for v in (x, t, y):
            if v is not None and v.device != self.device:
                raise RuntimeError(f"input on {v.device}, model on {self.device}")
        return x.float().contiguous(), t.long().contiguous(), y

    @staticmethod
    def _refuse(use_fp16, text_embedding):
        if use_fp16:
            raise NotImplementedError(f"use_fp16 ({_REF}:331-332, 391-392) is not built: the path computes in fp32")
        if text_embedding is not None:
            raise NotImplementedError(f"text_embedding (extras == 78, {_REF}:243-247, 345-348) is not built")

    @torch.no_grad()
    def forward(self, x, t, y=None, text_embedding=None, use_fp16=False, *, check_range: bool = True):
        """latte.py:319-382: x [N,F,C,H,W], t [N] integer timesteps, y [N] labels (extras == 2) -> [N,F,out_channels,H,W]."""
        self._refuse(use_fp16, text_embedding)
        return self._run(x, t, y, None, check_range)

    @torch.no_grad()
    def forward_with_cfg(self, x, t, y=None, cfg_scale=7.0, use_fp16=False, text_embedding=None, *, check_range: bool = True):
        """latte.py:384-403, its guidance on channels [0, 4) of every frame included."""
        self._refuse(use_fp16, text_embedding)
        return self._run(x, t, y, cfg_scale, check_range)


def _variant(depth, hidden_size, patch_size, num_heads, **fixed):
    def make(**kwargs):
        return Latte(depth=depth, hidden_size=hidden_size, patch_size=patch_size, num_heads=num_heads, **fixed, **kwargs)
    return make


Latte_models = {f"Latte-{n}/{p}": _variant(d, h, p, nh)
                for n, (d, h, nh) in {"XL": (28, 1152, 16), "L": (24, 1024, 16), "B": (12, 768, 12), "S": (12, 384, 6)}.items()
                for p in (2, 4, 8)}
Latte_models["Latte-XL/2-omnitokenizer"] = _variant(28, 1152, 2, 16, in_channels=8)  # latte.py:520-521


def load_latte(path, map_location="cpu"):
    """find_model's rule for a checkpoint file (Diffusion/Latte/download.py:4-21): the `ema` weights of a train.py checkpoint when
    present, else its `model`, else its `state_dict`; a file that is a plain state_dict (where the reference raises) is returned as
    it is.  Like the reference it unpickles the whole file: load only checkpoints you trust."""
    checkpoint = torch.load(path, map_location=map_location, weights_only=False)
    if isinstance(checkpoint, dict):
        for key in ("ema", "model", "state_dict"):
            if key in checkpoint:
                return checkpoint[key]
    return checkpoint
