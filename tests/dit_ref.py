"""A from-scratch torch restatement of the DiT forward, its classifier-free-guidance wrapper and one ancestral sampling step,
written against the reference's lines (Diffusion/DiT/models.py, Diffusion/DiT/diffusion/gaussian_diffusion.py) -- helper of
test_dit_cpu.py / test_gpu_dit.py, not collected.  It runs in whatever dtype the weights have: fp64 is the yardstick
(tests/golden/dit_*.npz holds the reference's own fp64 outputs, which test_dit_cpu.py compares this file against), fp32 on the CPU
is what sets the GPU's error bar.
"""
from __future__ import annotations

import math
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

# the two tiny models of the fixtures: (a) head_dim 64, 36 tokens (a key tail inside one tile pair), (b) head_dim 72, 81 tokens,
# patch K = 16
MODELS = {
    "a": dict(input_size=12, patch_size=2, in_channels=8, hidden_size=128, depth=2, num_heads=2, mlp_ratio=4.0,
              class_dropout_prob=0.1, num_classes=10, learn_sigma=True),
    "b": dict(input_size=18, patch_size=2, in_channels=4, hidden_size=288, depth=2, num_heads=4, mlp_ratio=4.0,
              class_dropout_prob=0.1, num_classes=10, learn_sigma=True),
}
SEEDS = {"a": 101, "b": 202}


def weight_shapes(cfg) -> "OrderedDict[str, tuple]":
    D, C, p = cfg["hidden_size"], cfg["in_channels"], cfg["patch_size"]
    Fh = int(D * cfg["mlp_ratio"])
    cout = 2 * C if cfg["learn_sigma"] else C
    n = (cfg["input_size"] // p) ** 2
    s = OrderedDict()
    s["pos_embed"] = (1, n, D)
    s["x_embedder.proj.weight"] = (D, C, p, p)
    s["x_embedder.proj.bias"] = (D,)
    s["t_embedder.mlp.0.weight"] = (D, 256)
    s["t_embedder.mlp.0.bias"] = (D,)
    s["t_embedder.mlp.2.weight"] = (D, D)
    s["t_embedder.mlp.2.bias"] = (D,)
    s["y_embedder.embedding_table.weight"] = (cfg["num_classes"] + (1 if cfg["class_dropout_prob"] > 0 else 0), D)
    for i in range(cfg["depth"]):
        b = f"blocks.{i}."
        s[b + "attn.qkv.weight"] = (3 * D, D)
        s[b + "attn.qkv.bias"] = (3 * D,)
        s[b + "attn.proj.weight"] = (D, D)
        s[b + "attn.proj.bias"] = (D,)
        s[b + "mlp.fc1.weight"] = (Fh, D)
        s[b + "mlp.fc1.bias"] = (Fh,)
        s[b + "mlp.fc2.weight"] = (D, Fh)
        s[b + "mlp.fc2.bias"] = (D,)
        s[b + "adaLN_modulation.1.weight"] = (6 * D, D)
        s[b + "adaLN_modulation.1.bias"] = (6 * D,)
    s["final_layer.linear.weight"] = (p * p * cout, D)
    s["final_layer.linear.bias"] = (p * p * cout,)
    s["final_layer.adaLN_modulation.1.weight"] = (2 * D, D)
    s["final_layer.adaLN_modulation.1.bias"] = (2 * D,)
    return s


def make_weights(cfg, seed) -> "OrderedDict[str, torch.Tensor]":
    """Every parameter from numpy.random.default_rng(seed), in the order of weight_shapes, as fp32 values (stable across machines and
    torch versions).  The reference zero-initialises every adaLN_modulation and the final linear (models.py:207-216): a model with
    that init outputs zeros and no block would be tested.  So: N(0, 0.02) for the modulations, every bias, the label table and
    pos_embed; Xavier-uniform-scale values (the reference's _basic_init) for the other matrices, the patch conv as a [D, C p p] one."""
    rng = np.random.default_rng(seed)
    out = OrderedDict()
    for name, shape in weight_shapes(cfg).items():
        if name.endswith(".bias") or "adaLN_modulation" in name or name in ("pos_embed", "y_embedder.embedding_table.weight"):
            v = rng.normal(0.0, 0.02, size=shape)
        else:
            fan_out, fan_in = shape[0], int(np.prod(shape[1:]))
            a = math.sqrt(6.0 / (fan_in + fan_out))
            v = rng.uniform(-a, a, size=shape)
        out[name] = torch.from_numpy(v.astype(np.float32))
    return out


def make_inputs(name):
    """x, t, y of the fixtures: t covers {0, 1, 500, 999}, y includes the null row (num_classes); an even batch for the CFG wrapper."""
    cfg = MODELS[name]
    rng = np.random.default_rng(SEEDS[name] + 1)
    x = rng.normal(size=(4, cfg["in_channels"], cfg["input_size"], cfg["input_size"])).astype(np.float32)
    t = np.array([0, 1, 500, 999], dtype=np.int64)
    y = np.array([3, 0, cfg["num_classes"], cfg["num_classes"]], dtype=np.int64)
    return x, t, y


def timestep_embedding(t, dtype, dim=256, max_period=10000):
    """models.py:51-59.  freqs, args and their cos / sin are fp32 there whatever the model's dtype (the fixture's model.double() casts
    the finished embedding); the engine's table holds cos / sin of the same fp32 args taken in fp64 and rounded once, at most one
    fp32 ulp from these."""
    half = dim // 2
    freqs = torch.exp(-math.log(max_period) * torch.arange(start=0, end=half, dtype=torch.float32) / half)
    args = t[:, None].float() * freqs[None].to(t.device)
    return torch.cat([torch.cos(args), torch.sin(args)], dim=-1).to(dtype)


def modulate(x, shift, scale):
    return x * (1 + scale.unsqueeze(1)) + shift.unsqueeze(1)  # models.py:19-20


def layer_norm(x):
    return F.layer_norm(x, (x.shape[-1],), eps=1e-6)  # elementwise_affine=False, models.py:107


def attention(qkv, heads):
    """timm's Attention.forward on the qkv rows: reshape(B, N, 3, heads, hd), scale hd^-0.5, softmax over keys."""
    B, N, D3 = qkv.shape
    hd = D3 // 3 // heads
    q, k, v = qkv.reshape(B, N, 3, heads, hd).permute(2, 0, 3, 1, 4).unbind(0)
    a = ((q * hd ** -0.5) @ k.transpose(-2, -1)).softmax(dim=-1)
    return (a @ v).transpose(1, 2).reshape(B, N, heads * hd)


def unpatchify(x, p, c):
    h = int(round(math.sqrt(x.shape[1])))  # models.py:218-231
    x = x.reshape(x.shape[0], h, h, p, p, c)
    return torch.einsum("nhwpqc->nchpwq", x).reshape(x.shape[0], c, h * p, h * p)


def forward(w, cfg, x, t, y):
    """models.py:233-248 with weights `w` (a dict in the compute dtype)."""
    dtype = w["pos_embed"].dtype
    p, heads = cfg["patch_size"], cfg["num_heads"]
    x = x.to(dtype)
    h = F.conv2d(x, w["x_embedder.proj.weight"], w["x_embedder.proj.bias"], stride=p).flatten(2).transpose(1, 2) + w["pos_embed"]
    te = timestep_embedding(t, dtype)
    te = F.linear(F.silu(F.linear(te, w["t_embedder.mlp.0.weight"], w["t_embedder.mlp.0.bias"])), w["t_embedder.mlp.2.weight"],
                  w["t_embedder.mlp.2.bias"])
    c = F.silu(te + w["y_embedder.embedding_table.weight"][y])
    for i in range(cfg["depth"]):
        b = f"blocks.{i}."
        sm, cm, gm, sl, cl, gl = F.linear(c, w[b + "adaLN_modulation.1.weight"], w[b + "adaLN_modulation.1.bias"]).chunk(6, dim=1)
        a = attention(F.linear(modulate(layer_norm(h), sm, cm), w[b + "attn.qkv.weight"], w[b + "attn.qkv.bias"]), heads)
        h = h + gm.unsqueeze(1) * F.linear(a, w[b + "attn.proj.weight"], w[b + "attn.proj.bias"])
        m = F.gelu(F.linear(modulate(layer_norm(h), sl, cl), w[b + "mlp.fc1.weight"], w[b + "mlp.fc1.bias"]), approximate="tanh")
        h = h + gl.unsqueeze(1) * F.linear(m, w[b + "mlp.fc2.weight"], w[b + "mlp.fc2.bias"])
    shift, scale = F.linear(c, w["final_layer.adaLN_modulation.1.weight"], w["final_layer.adaLN_modulation.1.bias"]).chunk(2, dim=1)
    h = F.linear(modulate(layer_norm(h), shift, scale), w["final_layer.linear.weight"], w["final_layer.linear.bias"])
    cout = 2 * cfg["in_channels"] if cfg["learn_sigma"] else cfg["in_channels"]
    return unpatchify(h, p, cout)


def forward_with_cfg(w, cfg, x, t, y, cfg_scale):
    """models.py:250-266, the guidance on channels [0, 3) only."""
    half = x[: len(x) // 2]
    out = forward(w, cfg, torch.cat([half, half], dim=0), t, y)
    eps, rest = out[:, :3], out[:, 3:]
    cond, uncond = torch.split(eps, len(eps) // 2, dim=0)
    g = uncond + cfg_scale * (cond - uncond)
    return torch.cat([torch.cat([g, g], dim=0), rest], dim=1)


def p_sample(coef_row, model_out, x, noise, learned_range, clip):
    """gaussian_diffusion.py:254-417 for one timestep shared by the batch.  coef_row: the 8 scalars of
    omnitokenizer_amd.diffusion.SpacedDiffusion.coefficient_table (fp32 values, as _extract_into_tensor's .float() leaves them);
    the arithmetic runs in model_out's dtype.  Returns (sample, pred_xstart)."""
    dtype = model_out.dtype
    k = [torch.tensor(float(v), dtype=torch.float32).to(dtype) for v in coef_row]
    x, noise = x.to(dtype), noise.to(dtype)
    C = x.shape[1]
    if learned_range:
        eps, var = torch.split(model_out, C, dim=1)
        frac = (var + 1) / 2
        logvar = frac * k[5] + (1 - frac) * k[4]
    else:
        eps, logvar = model_out, k[6] * torch.ones_like(x)
    xs = k[0] * x - k[1] * eps
    if clip:
        xs = xs.clamp(-1, 1)
    mean = k[2] * xs + k[3] * x
    return mean + k[7] * torch.exp(0.5 * logvar) * noise, xs


def toy_model(x, t, **kwargs):
    """The closed-form 'model' of the sampling-loop fixture: an eps half that depends on x and t, a variance half in (-1, 1)."""
    tt = t.to(x.dtype).view(-1, 1, 1, 1) / 1000
    return torch.cat([0.5 * torch.tanh(x) + 0.1 * tt, torch.sin(2 * x + tt)], dim=1)


def to_dtype(w, dtype):
    return OrderedDict((k, v.to(dtype)) for k, v in w.items())
