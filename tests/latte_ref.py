"""A from-scratch torch restatement of the Latte forward and its classifier-free-guidance wrapper, written against the reference's
lines (Diffusion/Latte/models/latte.py) -- helper of test_latte_cpu.py / test_gpu_latte.py, not collected.  Where the arithmetic is
the DiT's it is tests/dit_ref.py's.  It runs in whatever dtype the weights have: fp64 is the yardstick (tests/golden/latte_*.npz
holds the reference's own fp64 outputs, which test_latte_cpu.py compares this file against), fp32 on the CPU is what sets the
GPU's error bar.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from tests import dit_ref

# the two tiny models of the fixtures: (a) class-conditional, head_dim 64, 16 tokens, 5 frames, TWO block pairs (temp_embed is added
# in the first only); (b) unconditional, head_dim 72, 9 tokens (odd), 16 frames
MODELS = {
    "a": dict(input_size=8, patch_size=2, in_channels=8, hidden_size=128, depth=4, num_heads=2, mlp_ratio=4.0, num_frames=5,
              class_dropout_prob=0.1, num_classes=10, learn_sigma=True, extras=2),
    "b": dict(input_size=6, patch_size=2, in_channels=4, hidden_size=288, depth=2, num_heads=4, mlp_ratio=4.0, num_frames=16,
              class_dropout_prob=0.1, num_classes=10, learn_sigma=True, extras=1),
}
SEEDS = {"a": 303, "b": 404}
LOOP_SHAPE = (2, 3, 4, 5, 5)  # the sampling-loop fixture: [N, F, C, H, W]


def weight_shapes(cfg) -> "OrderedDict[str, tuple]":
    """latte.py's state_dict: the DiT's keys, temp_embed after pos_embed, y_embedder only with extras == 2."""
    s = OrderedDict()
    for name, shape in dit_ref.weight_shapes(cfg).items():
        if name == "y_embedder.embedding_table.weight" and cfg["extras"] != 2:
            continue
        s[name] = shape
        if name == "pos_embed":
            s["temp_embed"] = (1, cfg["num_frames"], cfg["hidden_size"])
    return s


def make_weights(cfg, seed) -> "OrderedDict[str, torch.Tensor]":
    """dit_ref.make_weights' rule over Latte's key list (temp_embed like pos_embed: N(0, 0.02)); nothing is zero-initialised, so
    every block contributes."""
    rng = np.random.default_rng(seed)
    out = OrderedDict()
    for name, shape in weight_shapes(cfg).items():
        if name.endswith(".bias") or "adaLN_modulation" in name or name in ("pos_embed", "temp_embed",
                                                                            "y_embedder.embedding_table.weight"):
            v = rng.normal(0.0, 0.02, size=shape)
        else:
            fan_out, fan_in = shape[0], int(np.prod(shape[1:]))
            a = np.sqrt(6.0 / (fan_in + fan_out))
            v = rng.uniform(-a, a, size=shape)
        out[name] = torch.from_numpy(v.astype(np.float32))
    return out


def make_inputs(name):
    """x [4, F, C, H, W], t covering {0, 1, 500, 999}, y with the null row (num_classes); an even batch for the CFG wrapper."""
    cfg = MODELS[name]
    rng = np.random.default_rng(SEEDS[name] + 1)
    x = rng.normal(size=(4, cfg["num_frames"], cfg["in_channels"], cfg["input_size"], cfg["input_size"])).astype(np.float32)
    t = np.array([0, 1, 500, 999], dtype=np.int64)
    y = np.array([3, 0, cfg["num_classes"], cfg["num_classes"]], dtype=np.int64)
    return x, t, y


def block(w, b, h, c, heads):
    """TransformerBlock.forward (latte.py:182-186) on h [S, L, D] with c [S, D]."""
    sm, cm, gm, sl, cl, gl = F.linear(c, w[b + "adaLN_modulation.1.weight"], w[b + "adaLN_modulation.1.bias"]).chunk(6, dim=1)
    a = dit_ref.attention(F.linear(dit_ref.modulate(dit_ref.layer_norm(h), sm, cm), w[b + "attn.qkv.weight"], w[b + "attn.qkv.bias"]),
                          heads)
    h = h + gm.unsqueeze(1) * F.linear(a, w[b + "attn.proj.weight"], w[b + "attn.proj.bias"])
    m = F.gelu(F.linear(dit_ref.modulate(dit_ref.layer_norm(h), sl, cl), w[b + "mlp.fc1.weight"], w[b + "mlp.fc1.bias"]),
               approximate="tanh")
    return h + gl.unsqueeze(1) * F.linear(m, w[b + "mlp.fc2.weight"], w[b + "mlp.fc2.bias"])


def forward(w, cfg, x, t, y=None):
    """latte.py:319-382 with weights `w` (a dict in the compute dtype): x [B, F, C, H, W] -> [B, F, Cout, H, W]."""
    dtype = w["pos_embed"].dtype
    p, heads = cfg["patch_size"], cfg["num_heads"]
    B, Fr = x.shape[:2]
    x = x.to(dtype).flatten(0, 1)                                                     # b f c h w -> (b f) c h w
    h = F.conv2d(x, w["x_embedder.proj.weight"], w["x_embedder.proj.bias"], stride=p).flatten(2).transpose(1, 2) + w["pos_embed"]
    N, D = h.shape[1:]
    te = dit_ref.timestep_embedding(t, dtype)
    te = F.linear(F.silu(F.linear(te, w["t_embedder.mlp.0.weight"], w["t_embedder.mlp.0.bias"])), w["t_embedder.mlp.2.weight"],
                  w["t_embedder.mlp.2.bias"])
    c = te + w["y_embedder.embedding_table.weight"][y] if cfg["extras"] == 2 else te
    c = F.silu(c)                                                                     # every adaLN_modulation starts with this SiLU
    c_spatial, c_temp = c.repeat_interleave(Fr, 0), c.repeat_interleave(N, 0)         # 'n d -> (n c) d'
    for i in range(0, cfg["depth"], 2):
        h = block(w, f"blocks.{i}.", h, c_spatial, heads)
        h = h.reshape(B, Fr, N, D).transpose(1, 2).reshape(B * N, Fr, D)              # (b f) t d -> (b t) f d
        if i == 0:
            h = h + w["temp_embed"]
        h = block(w, f"blocks.{i + 1}.", h, c_temp, heads)
        h = h.reshape(B, N, Fr, D).transpose(1, 2).reshape(B * Fr, N, D)              # (b t) f d -> (b f) t d
    shift, scale = F.linear(c_spatial, w["final_layer.adaLN_modulation.1.weight"], w["final_layer.adaLN_modulation.1.bias"]).chunk(2, dim=1)
    h = F.linear(dit_ref.modulate(dit_ref.layer_norm(h), shift, scale), w["final_layer.linear.weight"], w["final_layer.linear.bias"])
    cout = 2 * cfg["in_channels"] if cfg["learn_sigma"] else cfg["in_channels"]
    return dit_ref.unpatchify(h, p, cout).reshape(B, Fr, cout, x.shape[-2], x.shape[-1])


def forward_with_cfg(w, cfg, x, t, y, cfg_scale):
    """latte.py:384-403, the guidance on channels [0, 4) of dim 2 only."""
    half = x[: len(x) // 2]
    out = forward(w, cfg, torch.cat([half, half], dim=0), t, y)
    eps, rest = out[:, :, :4], out[:, :, 4:]
    cond, uncond = torch.split(eps, len(eps) // 2, dim=0)
    g = uncond + cfg_scale * (cond - uncond)
    return torch.cat([torch.cat([g, g], dim=0), rest], dim=2)


def toy_model(x, t, **kwargs):
    """dit_ref.toy_model for 5-D latents [N, F, C, H, W]: the eps and the variance half are concatenated on dim 2."""
    tt = t.to(x.dtype).view(-1, 1, 1, 1, 1) / 1000
    return torch.cat([0.5 * torch.tanh(x) + 0.1 * tt, torch.sin(2 * x + tt)], dim=2)


def p_sample(coef_row, model_out, x, noise, learned_range, clip):
    """dit_ref.p_sample on 5-D latents: the reference splits on dim 2 (Latte/diffusion/gaussian_diffusion.py:291), which is
    dit_ref's dim-1 split of the frames taken as a batch."""
    s, xs = dit_ref.p_sample(coef_row, model_out.flatten(0, 1), x.flatten(0, 1), noise.flatten(0, 1), learned_range, clip)
    return s.reshape(x.shape), xs.reshape(x.shape)


to_dtype = dit_ref.to_dtype
