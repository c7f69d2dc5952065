"""TEST HELPER (not collected): the DiT's attention with bf16 / fp16 operands (omnitok_dit_attn16, include/omnitok_dit.h) restated in
fp64, a bar for |kernel result - fp64 restatement| derived from the arithmetic contract alone, a plain torch restatement of the
contract, and the DiT / Latte forwards with that attention in their spatial blocks.  It is the non-causal form of
tests/lm_prefill_attn16_ref.py, which is built on tests/lm_prefill_attn_ref.py: read their docstrings first; only the differences are
stated here.

The contract is the one of omnitok_lm_attn_prefill16 without the causal mask: every query sees the N keys of its sample.  So in the bar
  * the mask is all-true: every sum runs over the N keys;
  * tiles = ceil(N / 32) for every row, keys per row N: n_O = N + tiles + 1, n_l = 17 + 2 tiles, n_exp = tiles;
  * hd is the real 64 / 72: the zeros the kernel pads head_dim 72 with add exact products and no rounding;
  * EXP_ULPS = 1 (v_exp_f32), the log1p(u16) term for the one rounding of P, and the fp16 subnormal-weight term 2^-25 sum_j |v_jd|
    over all N keys stay as they are there.
The kernel multiplies the finished dot by fl(log2(e) / sqrt(hd)) and takes v_exp_f32 (base 2): one rounded constant and one multiply,
the two roundings E already counts beside the hd of the chain (gamma(hd + 2)); the rounding of a base-2 argument, u |s' - m'|, is a
relative weight error of ln 2 times that = u (m - s) in natural units, the term the derivation has.  Nothing in it is fitted to a kernel.
"""
import functools
import math

import torch
import torch.nn.functional as F

from tests import dit16_ref, dit_ref, latte_ref
from tests import error_bounds as eb
from tests import lm_prefill_attn16_ref as r16
from tests import lm_prefill_attn_ref as ar

FMT = r16.FMT
U16 = r16.U16
EXP_ULPS = 1     # v_exp_f32: 1 ulp (csrc/attn16_tiled.h)
KT = 32          # the key tile
FMTS = ["bf16", "fp16"]
HDS = [64, 72]
# the shapes of the fp64 comparison: N x (B, heads).  16: half a tile; 32: one whole tile; 36 / 81: the golden models' N (a tail of 4 /
# two tiles and a tail of 17); 256: DiT-XL/2's N, two query blocks of whole tiles; 257: a third query block of one row and a tail of one key
NS = [16, 32, 36, 81, 256, 257]
BH = {1: (1, 1), 6: (2, 3)}


def make_qkv(B, N, H, hd, q_scale=1.0):
    """qkv [B * N, 3C] fp32: tests/lm_prefill_attn_ref.py's recipe (standard normal q, k, v; q_scale 8: its q8 case)."""
    C = H * hd
    qkv = ar.rnd(B * N, 3 * C, seed=100 + hd + N + 7 * B).view(B, N, 3, H, hd).clone()
    qkv[:, :, 0] *= q_scale
    return qkv.view(B * N, 3 * C).contiguous()


def reference16(qkv, B, N, H, fmt):
    """(out64 [B * N, C], bar [B * N, C]); see the module docstring."""
    C = qkv.shape[1] // 3
    hd = C // H
    q, k, v = ar.split64(r16.round_qkv(qkv, fmt), B, N, H)
    scale = 1.0 / math.sqrt(hd)
    s = (q @ k.transpose(-1, -2)) * scale
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    p = e / e.sum(-1, keepdim=True)
    out = p @ v
    va = v.abs()
    pv = p @ va
    tiles = math.ceil(N / KT)
    n_o = torch.tensor(float(N + tiles + 1), dtype=torch.float64)
    n_l = torch.tensor(float(17 + 2 * tiles), dtype=torch.float64)
    n_exp = tiles
    E = eb.gamma(hd + 2) * ((q.abs() @ k.abs().transpose(-1, -2)) * scale)
    gap = m - s
    near = gap <= ar.FAR
    loge = E + eb.U * gap + EXP_ULPS * 2 * eb.U * n_exp + math.log1p(U16[fmt])
    eps = torch.expm1(torch.where(near, loge, torch.zeros_like(loge)).amax(-1, keepdim=True))
    assert float(eps.max()) < 0.5
    soft = 2 * eps / (1 - eps) * pv
    far = 2 * math.exp(-ar.FAR + 1.0) * ((~near).double() @ va)
    sums = (ar._gamma(n_o) + ar._gamma(n_l)) * pv
    bar = soft + far + sums
    if fmt == "fp16":
        bar = bar + 2.0 ** -25 * va.sum(-2, keepdim=True)
    bar = bar * (1 + 2.0 ** -10)
    flat = lambda x: x.transpose(1, 2).reshape(B * N, C)
    return flat(out), flat(bar)


def tile_attention_full(q, k, v, fmt, kt):
    """r16.tile_attention without a mask and with any number of keys (k, v [B, H, keys, hd], q [B, H, N, hd]): the loop restated for
    the mutations of the CPU test, which change the key count.  With keys == N it is tile_attention(..., mask_shift=N) operation for
    operation (tests/test_dit_attn16_cpu.py compares the two bit for bit)."""
    dt = q.dtype
    nk, hd = k.shape[-2], q.shape[-1]
    scale = torch.tensor(1.0 / math.sqrt(hd), dtype=torch.float32).to(dt)
    m = torch.full(q.shape[:-1] + (1,), float("-inf"), dtype=dt)
    l = torch.zeros_like(m)
    o = torch.zeros_like(q)
    for k0 in range(0, nk, kt):
        k1 = min(k0 + kt, nk)
        s = (q @ k[..., k0:k1, :].transpose(-1, -2)) * scale
        m_new = torch.maximum(m, s.amax(-1, keepdim=True))
        p = torch.exp(s - m_new)
        alpha = torch.exp(m - m_new)
        l = l * alpha + p.sum(-1, keepdim=True)
        o = o * alpha + p.to(FMT[fmt][1]).to(dt) @ v[..., k0:k1, :]
        m = m_new
    return o / l


def emulate(qkv, B, N, H, fmt, kt=KT, rounded=("q", "k", "v"), keys=None):
    """The contract in plain torch fp32, [B * N, C]: r16.tile_attention with a full mask (mask_shift = N: row t sees keys
    j <= min(t + N, N - 1)).  `rounded` and `keys` exist for the mutations of the CPU test: keys = N - 1 drops the last key,
    keys = N + 1 admits one key past N as a duplicate of row N - 1 (what an unmasked clamped tile row would be)."""
    C = qkv.shape[1] // 3
    x = qkv.view(B, N, 3, H, C // H).permute(2, 0, 3, 1, 4)
    q, k, v = (r16.round_qkv(x[i], fmt) if n in rounded else x[i].float() for i, n in enumerate("qkv"))
    if keys is None:
        out = r16.tile_attention(q, k, v, fmt, kt, mask_shift=N)
    else:
        idx = torch.arange(keys).clamp(max=N - 1)
        out = tile_attention_full(q, k[..., idx, :], v[..., idx, :], fmt, kt)
    return out.transpose(1, 2).reshape(B * N, C)


@functools.lru_cache(maxsize=None)
def case(N, hd, bh, fmt, q_scale=1.0):
    """inputs, fp64 result and bar of a case, computed once and shared by the CPU and the GPU test (treat as read-only)"""
    B, H = BH[bh]
    qkv = make_qkv(B, N, H, hd, q_scale)
    out64, bar = reference16(qkv, B, N, H, fmt)
    return dict(B=B, N=N, H=H, qkv=qkv, out64=out64, bar=bar)


# ---- the whole model ---------------------------------------------------------------------------------------------------------------
def attention(qkv, heads, afmt, mode):
    """dit_ref.attention on the qkv rows [S, N, 3D] with q, k, v through .to(afmt) once.  mode "exact": softmax in the working dtype;
    mode "tile": online softmax over tiles of KT keys with P rounded per tile (r16.tile_attention, full mask).  afmt None:
    dit_ref.attention itself."""
    if afmt is None:
        return dit_ref.attention(qkv, heads)
    S, N, D3 = qkv.shape
    hd = D3 // 3 // heads
    q, k, v = (dit16_ref.q(t, afmt) for t in qkv.reshape(S, N, 3, heads, hd).permute(2, 0, 3, 1, 4).unbind(0))
    if mode == "exact":
        a = ((q * hd ** -0.5) @ k.transpose(-2, -1)).softmax(dim=-1) @ v
    else:
        a = r16.tile_attention(q, k, v, afmt, KT, mask_shift=N)
    return a.transpose(1, 2).reshape(S, N, heads * hd)


def block(w, b, h, c, heads, lfmt, afmt, mode):
    """dit16_ref.block (linear format lfmt) with `attention` above in place of dit_ref.attention."""
    def lin(v, name):
        return F.linear(dit16_ref.q(v, lfmt), dit16_ref.q(w[b + name + ".weight"], lfmt), w[b + name + ".bias"])

    sm, cm, gm, sl, cl, gl = F.linear(c, w[b + "adaLN_modulation.1.weight"], w[b + "adaLN_modulation.1.bias"]).chunk(6, dim=1)
    a = attention(lin(dit_ref.modulate(dit_ref.layer_norm(h), sm, cm), "attn.qkv"), heads, afmt, mode)
    h = h + gm.unsqueeze(1) * lin(a, "attn.proj")
    m = F.gelu(lin(dit_ref.modulate(dit_ref.layer_norm(h), sl, cl), "mlp.fc1"), approximate="tanh")
    return h + gl.unsqueeze(1) * lin(m, "mlp.fc2")


def dit_forward(w, cfg, x, t, y, lfmt, afmt, mode):
    """dit16_ref.dit_forward with every block's attention in afmt"""
    dtype = w["pos_embed"].dtype
    h = F.conv2d(x.to(dtype), w["x_embedder.proj.weight"], w["x_embedder.proj.bias"], stride=cfg["patch_size"])
    h = h.flatten(2).transpose(1, 2) + w["pos_embed"]
    c = F.silu(dit16_ref._conditioning(w, t, y, dtype))
    for i in range(cfg["depth"]):
        h = block(w, f"blocks.{i}.", h, c, cfg["num_heads"], lfmt, afmt, mode)
    return dit16_ref._final(w, cfg, h, c)[0]


def latte_forward(w, cfg, x, t, y, lfmt, afmt, mode):
    """dit16_ref.latte_forward with the attention of the SPATIAL blocks (0, 2, ...) in afmt; the temporal blocks' stays as it is"""
    dtype = w["pos_embed"].dtype
    B, Fr = x.shape[:2]
    x = x.to(dtype).flatten(0, 1)
    h = F.conv2d(x, w["x_embedder.proj.weight"], w["x_embedder.proj.bias"], stride=cfg["patch_size"]).flatten(2).transpose(1, 2)
    h = h + w["pos_embed"]
    N, D = h.shape[1:]
    c = F.silu(dit16_ref._conditioning(w, t, y if cfg["extras"] == 2 else None, dtype))
    c_spatial, c_temp = c.repeat_interleave(Fr, 0), c.repeat_interleave(N, 0)
    for i in range(0, cfg["depth"], 2):
        h = block(w, f"blocks.{i}.", h, c_spatial, cfg["num_heads"], lfmt, afmt, mode)
        h = h.reshape(B, Fr, N, D).transpose(1, 2).reshape(B * N, Fr, D)
        if i == 0:
            h = h + w["temp_embed"]
        h = block(w, f"blocks.{i + 1}.", h, c_temp, cfg["num_heads"], lfmt, None, mode)
        h = h.reshape(B, N, Fr, D).transpose(1, 2).reshape(B * Fr, N, D)
    out, cout = dit16_ref._final(w, cfg, h, c_spatial)
    return out.reshape(B, Fr, cout, x.shape[-2], x.shape[-1])


KINDS = {"dit": (dit_ref, dit_forward, 1, 3), "latte": (latte_ref, latte_forward, 2, 4)}  # module, forward, channel dim, guided channels


def forward(kind, w, cfg, x, t, y, lfmt, afmt, mode, cfg_scale=None):
    """forward (cfg_scale None) or forward_with_cfg of a "dit" / "latte" model under linear format lfmt and attention format afmt
    (either may be None = fp32)."""
    _, fwd, cdim, guided = KINDS[kind]
    if cfg_scale is None:
        return fwd(w, cfg, x, t, y, lfmt, afmt, mode)
    half = x[: len(x) // 2]
    out = fwd(w, cfg, torch.cat([half, half], dim=0), t, y, lfmt, afmt, mode)
    eps, rest = out.narrow(cdim, 0, guided), out.narrow(cdim, guided, out.shape[cdim] - guided)
    cond, uncond = torch.split(eps, len(eps) // 2, dim=0)
    g = uncond + cfg_scale * (cond - uncond)
    return torch.cat([torch.cat([g, g], dim=0), rest], dim=cdim)


@functools.lru_cache(maxsize=None)
def model_reference(kind, name, afmt, lfmt=None, cfg_scale=None):
    """(fp64 "exact" run, d_ref = max |fp32 "tile" run - fp64 "exact" run|) of golden model `name` on the golden inputs: the
    construction of dit16_ref.reference and r16.engine_reference, computed on the CPU, once per case."""
    mod = KINDS[kind][0]
    cfg = mod.MODELS[name]
    w32 = mod.make_weights(cfg, mod.SEEDS[name])
    x, t, y = (torch.from_numpy(v) for v in mod.make_inputs(name))
    ref = forward(kind, mod.to_dtype(w32, torch.float64), cfg, x, t, y, lfmt, afmt, "exact", cfg_scale)
    run32 = forward(kind, w32, cfg, x, t, y, lfmt, afmt, "tile", cfg_scale)
    return ref, float((run32.double() - ref).abs().max())
