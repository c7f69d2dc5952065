"""TEST HELPER: the tiled prefill attention with bf16 / fp16 operands (omnitok_lm_attn_prefill16, include/omnitok_lm.h) restated in
fp64, a bar for |kernel result - fp64 restatement| derived from the arithmetic contract alone, a plain torch restatement of the
contract, and the engine's forward with that attention.  Built on tests/lm_prefill_attn_ref.py (CASES, make_qkv, HDS, FAR): read its
docstring first; only the differences are stated here.

The contract: Q, K and V rounded ONCE to the operand format (the bits of tensor.to(fmt)): that rounding is part of the contract, not
an error, so the fp64 restatement is attention over qkv.to(fmt).  Products of two 16-bit operands are exact in fp32; the dot is
accumulated in fp32 (hd roundings, any order), scaled after it is finished; online softmax over key tiles of kt keys; every weight is
rounded ONCE to the operand format on its way into P . V; fp32 accumulation; out = O / l.

The bar is the tiled bar of tests/lm_prefill_attn_ref.py with
  * |q|, |k|, |v| of the ROUNDED operands;
  * tiles = ceil((t + 1) / kt);
  * exp_ulps (the documented error of the kernel's exponential, a parameter) in place of EXPF_ULPS;
  * log1p(u16) added to every key's log-weight error, u16 = 2^-8 (bf16) | 2^-11 (fp16): the one rounding of P.  It sits inside the
    2 eps / (1 - eps) sum p |v| term, which moves numerator and denominator: l summed before or after that rounding are both covered;
  * fp16 only: 2^-25 sum_{j <= t} |v_jd|: a weight below fp16's normal range is off by at most half the smallest subnormal (2^-25),
    against l >= 1.
Nothing in it is fitted to a kernel.
"""
import functools
import math

import torch
import torch.nn.functional as F

from tests import error_bounds as eb
from tests import lm_prefill16_ref as pr
from tests import lm_prefill_attn_ref as ar

FMT = pr.FMT
U16 = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
EXP_ULPS = 1     # v_exp_f32: 1 ulp (the 16-bit kernel's header in csrc/lm_attn_prefill.hip)
KT = 32          # its key tile


def round_qkv(qkv, fmt):
    return qkv.to(FMT[fmt][1]).float()


def reference16(qkv, B, T, H, fmt, exp_ulps, kt):
    """(out64 [B * T, C], bar [B * T, C]); see the module docstring."""
    C = qkv.shape[1] // 3
    hd = C // H
    q, k, v = ar.split64(round_qkv(qkv, fmt), B, T, H)
    scale = 1.0 / math.sqrt(hd)
    mask = torch.tril(torch.ones(T, T, dtype=torch.bool))
    s = ((q @ k.transpose(-1, -2)) * scale).masked_fill(~mask, float("-inf"))
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    p = e / e.sum(-1, keepdim=True)
    out = p @ v
    va = v.abs()
    pv = p @ va
    t1 = torch.arange(1, T + 1, dtype=torch.float64)[:, None]
    tiles = torch.ceil(t1 / kt)
    n_o, n_l, n_exp = t1 + tiles + 1, 17 + 2 * tiles, tiles
    E = eb.gamma(hd + 2) * ((q.abs() @ k.abs().transpose(-1, -2)) * scale)
    gap = m - s
    near = mask & (gap <= ar.FAR)
    loge = E + eb.U * gap + exp_ulps * 2 * eb.U * n_exp + math.log1p(U16[fmt])
    eps = torch.expm1(torch.where(near, loge, torch.zeros_like(loge)).amax(-1, keepdim=True))
    assert float(eps.max()) < 0.5
    soft = 2 * eps / (1 - eps) * pv
    far = 2 * math.exp(-ar.FAR + 1.0) * ((mask & ~near).double() @ va)
    sums = (ar._gamma(n_o) + ar._gamma(n_l)) * pv
    bar = soft + far + sums
    if fmt == "fp16":
        bar = bar + 2.0 ** -25 * (mask.double() @ va)
    bar = bar * (1 + 2.0 ** -10)
    flat = lambda x: x.transpose(1, 2).reshape(B * T, C)
    return flat(out), flat(bar)


def tile_attention(q, k, v, fmt, kt, mask_shift=0):
    """Online softmax over key tiles of kt keys in the dtype of q / k / v [B, H, T, hd] (already rounded or not: the caller's choice),
    the weights of every tile rounded to fmt before P . V, l summed from the unrounded weights.  Row t sees keys j <= t + mask_shift
    (at least key 0)."""
    dt = q.dtype
    T, hd = q.shape[-2], q.shape[-1]
    scale = torch.tensor(1.0 / math.sqrt(hd), dtype=torch.float32).to(dt)
    lim = (torch.arange(T) + mask_shift).clamp(0, T - 1)[:, None]
    m = torch.full(q.shape[:-1] + (1,), float("-inf"), dtype=dt)
    l = torch.zeros_like(m)
    o = torch.zeros_like(q)
    for k0 in range(0, T, kt):
        k1 = min(k0 + kt, T)
        s = (q @ k[..., k0:k1, :].transpose(-1, -2)) * scale
        s = s.masked_fill(torch.arange(k0, k1)[None, :] > lim, float("-inf"))
        m_new = torch.maximum(m, s.amax(-1, keepdim=True))
        p = torch.exp(s - m_new)
        alpha = torch.exp(m - m_new)
        l = l * alpha + p.sum(-1, keepdim=True)
        o = o * alpha + p.to(FMT[fmt][1]).to(dt) @ v[..., k0:k1, :]
        m = m_new
    return o / l


def emulate(qkv, B, T, H, fmt, kt, rounded=("q", "k", "v"), mask_shift=0):
    """The contract in plain torch fp32, [B * T, C].  `rounded` and `mask_shift` exist for the mutations of the CPU test."""
    C = qkv.shape[1] // 3
    x = qkv.view(B, T, 3, H, C // H).permute(2, 0, 3, 1, 4)
    q, k, v = (round_qkv(x[i], fmt) if n in rounded else x[i].float() for i, n in enumerate("qkv"))
    return tile_attention(q, k, v, fmt, kt, mask_shift).transpose(1, 2).reshape(B * T, C)


def engine_restatement(sd, idx, n_head, afmt, dt, mode, wfmt=None):
    """The oracle's forward (oracle/gpt_oracle.py) in dt with q, k, v of every block rounded to afmt.  mode "exact": softmax over the
    rounded operands in dt; mode "tile": tile_attention (kt = KT, P rounded per tile).  wfmt: the roundings of a PF_W16 prefill on
    wfmt weights as well (tests/lm_prefill16_ref.py: rounded matrices, every nn.Linear input rounded to wfmt)."""
    a16 = FMT[afmt][1]
    sd = {k: v.to(dt) for k, v in (pr.rounded(sd, wfmt) if wfmt else sd).items()}
    rw = (lambda t: t.to(FMT[wfmt][1]).to(dt)) if wfmt else (lambda t: t)
    x = F.embedding(idx, sd["tok_emb.weight"])
    B, T, C = x.shape
    x = x + sd["pos_emb"][:, :T]
    hs = C // n_head
    n_layer = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
    mask = torch.tril(torch.ones(T, T, dtype=torch.bool))
    for i in range(n_layer):
        p = f"blocks.{i}"
        h = rw(F.layer_norm(x, (C,), sd[f"{p}.ln1.weight"], sd[f"{p}.ln1.bias"]))
        q, k, v = (F.linear(h, sd[f"{p}.attn.{n}.weight"], sd[f"{p}.attn.{n}.bias"]).view(B, T, n_head, hs).transpose(1, 2).to(a16).to(dt)
                   for n in ("query", "key", "value"))
        if mode == "exact":
            att = ((q @ k.transpose(-2, -1)) * (1.0 / math.sqrt(hs))).masked_fill(~mask, float("-inf"))
            y = F.softmax(att, dim=-1) @ v
        else:
            y = tile_attention(q, k, v, afmt, KT)
        y = y.transpose(1, 2).contiguous().view(B, T, C)
        x = x + F.linear(rw(y), sd[f"{p}.attn.proj.weight"], sd[f"{p}.attn.proj.bias"])
        h = rw(F.layer_norm(x, (C,), sd[f"{p}.ln2.weight"], sd[f"{p}.ln2.bias"]))
        h = rw(F.gelu(F.linear(h, sd[f"{p}.mlp.0.weight"], sd[f"{p}.mlp.0.bias"])))
        x = x + F.linear(h, sd[f"{p}.mlp.2.weight"], sd[f"{p}.mlp.2.bias"])
    x = rw(F.layer_norm(x, (C,), sd["ln_f.weight"], sd["ln_f.bias"]))
    return F.linear(x, sd["head.weight"])


def engine_reference(sd, idx, n_head, afmt, wfmt=None):
    """(logits64 of the "exact" restatement, Y): Y = max |"tile" restatement in fp32 - "exact" restatement in fp64| over the logits,
    the restatement's own distance -- computed on the CPU, never from the code under test."""
    l64 = engine_restatement(sd, idx, n_head, afmt, torch.float64, "exact", wfmt)
    l32 = engine_restatement(sd, idx, n_head, afmt, torch.float32, "tile", wfmt)
    return l64, float((l32.double() - l64).abs().max())


@functools.lru_cache(maxsize=None)
def case(name, hd, fmt):
    """inputs (shared with tests/lm_prefill_attn_ref.py), fp64 result and bar of a case, computed once (treat as read-only)"""
    B, T = ar.CASES[name]
    qkv = ar.case(name, hd)["qkv"]
    out64, bar = reference16(qkv, B, T, ar.HEADS, fmt, EXP_ULPS, KT)
    return dict(B=B, T=T, qkv=qkv, out64=out64, bar=bar)
