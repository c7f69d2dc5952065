"""The DiT and Latte forwards of tests/dit_ref.py / tests/latte_ref.py restated for a 16-bit linear format
(DiT.set_linear_format) -- helper of test_dit16_cpu.py / test_gpu_dit16.py / test_gpu_latte16.py, not collected.

Two changes against those files, nothing else:
  * the four matrices of every block (attn.qkv, attn.proj, mlp.fc1, mlp.fc2) pass through .to(fmt);
  * the input of each of those four linears passes through .to(fmt) once: the modulated LayerNorm rows (twice per block), the
    attention output, the GELU output.
Everything else -- biases, the residual stream, LayerNorm, attention, the conditioning, the final layer -- runs in the working
dtype.  fmt None disables both changes: the functions are then dit_ref.forward / latte_ref.forward operation for operation.
reference() gives the fp64 run (the yardstick) and d_ref, the distance of the fp32 run on the CPU from it (the GPU's error bar).
"""
from __future__ import annotations

import functools

import torch
import torch.nn.functional as F

from tests import dit_ref, latte_ref

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}


def q(v, fmt):
    """v rounded once to fmt (to nearest even), back in its own dtype; fmt None: v."""
    return v if fmt is None else v.to(DTYPES[fmt]).to(v.dtype)


def block(w, b, h, c, heads, fmt):
    """One block on h [S, L, D] with c [S, D]: latte_ref.block with the four linears' operands through q."""
    def lin(v, name):
        return F.linear(q(v, fmt), q(w[b + name + ".weight"], fmt), w[b + name + ".bias"])

    sm, cm, gm, sl, cl, gl = F.linear(c, w[b + "adaLN_modulation.1.weight"], w[b + "adaLN_modulation.1.bias"]).chunk(6, dim=1)
    a = dit_ref.attention(lin(dit_ref.modulate(dit_ref.layer_norm(h), sm, cm), "attn.qkv"), heads)
    h = h + gm.unsqueeze(1) * lin(a, "attn.proj")
    m = F.gelu(lin(dit_ref.modulate(dit_ref.layer_norm(h), sl, cl), "mlp.fc1"), approximate="tanh")
    return h + gl.unsqueeze(1) * lin(m, "mlp.fc2")


def _conditioning(w, t, y, dtype):
    te = dit_ref.timestep_embedding(t, dtype)
    te = F.linear(F.silu(F.linear(te, w["t_embedder.mlp.0.weight"], w["t_embedder.mlp.0.bias"])), w["t_embedder.mlp.2.weight"],
                  w["t_embedder.mlp.2.bias"])
    return te if y is None else te + w["y_embedder.embedding_table.weight"][y]


def _final(w, cfg, h, c):
    shift, scale = F.linear(c, w["final_layer.adaLN_modulation.1.weight"], w["final_layer.adaLN_modulation.1.bias"]).chunk(2, dim=1)
    h = F.linear(dit_ref.modulate(dit_ref.layer_norm(h), shift, scale), w["final_layer.linear.weight"], w["final_layer.linear.bias"])
    cout = 2 * cfg["in_channels"] if cfg["learn_sigma"] else cfg["in_channels"]
    return dit_ref.unpatchify(h, cfg["patch_size"], cout), cout


def dit_forward(w, cfg, x, t, y, fmt):
    dtype = w["pos_embed"].dtype
    h = F.conv2d(x.to(dtype), w["x_embedder.proj.weight"], w["x_embedder.proj.bias"], stride=cfg["patch_size"])
    h = h.flatten(2).transpose(1, 2) + w["pos_embed"]
    c = F.silu(_conditioning(w, t, y, dtype))
    for i in range(cfg["depth"]):
        h = block(w, f"blocks.{i}.", h, c, cfg["num_heads"], fmt)
    return _final(w, cfg, h, c)[0]


def latte_forward(w, cfg, x, t, y, fmt):
    dtype = w["pos_embed"].dtype
    B, Fr = x.shape[:2]
    x = x.to(dtype).flatten(0, 1)
    h = F.conv2d(x, w["x_embedder.proj.weight"], w["x_embedder.proj.bias"], stride=cfg["patch_size"]).flatten(2).transpose(1, 2)
    h = h + w["pos_embed"]
    N, D = h.shape[1:]
    c = F.silu(_conditioning(w, t, y if cfg["extras"] == 2 else None, dtype))
    c_spatial, c_temp = c.repeat_interleave(Fr, 0), c.repeat_interleave(N, 0)
    for i in range(0, cfg["depth"], 2):
        h = block(w, f"blocks.{i}.", h, c_spatial, cfg["num_heads"], fmt)
        h = h.reshape(B, Fr, N, D).transpose(1, 2).reshape(B * N, Fr, D)
        if i == 0:
            h = h + w["temp_embed"]
        h = block(w, f"blocks.{i + 1}.", h, c_temp, cfg["num_heads"], fmt)
        h = h.reshape(B, N, Fr, D).transpose(1, 2).reshape(B * Fr, N, D)
    out, cout = _final(w, cfg, h, c_spatial)
    return out.reshape(B, Fr, cout, x.shape[-2], x.shape[-1])


KINDS = {"dit": (dit_ref, dit_forward, 1, 3), "latte": (latte_ref, latte_forward, 2, 4)}  # module, forward, channel dim, guided channels


def forward(kind, w, cfg, x, t, y, fmt, cfg_scale=None):
    """forward (cfg_scale None) or forward_with_cfg of a "dit" / "latte" model under linear format fmt."""
    _, fwd, cdim, guided = KINDS[kind]
    if cfg_scale is None:
        return fwd(w, cfg, x, t, y, fmt)
    half = x[: len(x) // 2]
    out = fwd(w, cfg, torch.cat([half, half], dim=0), t, y, fmt)
    eps, rest = out.narrow(cdim, 0, guided), out.narrow(cdim, guided, out.shape[cdim] - guided)
    cond, uncond = torch.split(eps, len(eps) // 2, dim=0)
    g = uncond + cfg_scale * (cond - uncond)
    return torch.cat([torch.cat([g, g], dim=0), rest], dim=cdim)


@functools.lru_cache(maxsize=None)
def reference(kind, name, fmt, cfg_scale=None):
    """(fp64 result, d_ref = max |fp32 run - fp64 run|) of golden model `name` on the golden inputs; computed once per case."""
    mod = KINDS[kind][0]
    cfg = mod.MODELS[name]
    w32 = mod.make_weights(cfg, mod.SEEDS[name])
    x, t, y = (torch.from_numpy(v) for v in mod.make_inputs(name))
    ref = forward(kind, mod.to_dtype(w32, torch.float64), cfg, x, t, y, fmt, cfg_scale)
    run32 = forward(kind, w32, cfg, x, t, y, fmt, cfg_scale)
    return ref, float((run32.double() - ref).abs().max())
