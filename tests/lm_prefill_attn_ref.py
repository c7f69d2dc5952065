"""TEST HELPER: the causal attention of a batched prefill (omnitok_lm_attn_prefill, include/omnitok_lm.h) restated in fp64, a bar for
|fp32 result - fp64 restatement| derived from the arithmetic contract alone, and the inputs the CPU and GPU tests share.

The contract: score s~ = fl((q . k) scale) with the dot one fp32 chain over head_dim products and scale = fl(1 / sqrtf(hd)); weights
from expf of fp32 differences of scores (online softmax: a weight is a product of expf values whose arguments, all <= 0, telescope to
s~_j - m~, m~ the row's largest score); O = sum_j w_j v_j and l = sum_j w_j in fp32 in some order; out = O / l.  u = 2^-24.

  1. score      |s~_j - s_j| <= E_j = gamma(hd + 2) scale sum_d |q_d| |k_jd|: hd roundings of the chain (Higham, Lemma 3.1: any order),
                one of scale itself, one of the multiplication by it.
     exponent   the n_exp expf evaluations on a weight's path each carry 1 ulp <= 2u relative (HIP math API, expf: 1 ulp) and the
                rounding of their argument, u |argument|; the arguments share a sign and telescope, so these add up to u (m - s_j).
                The error of m~ itself scales every weight of the row alike and cancels in O / l.
                => w_j = exp(s_j - m) (1 + e_j), |e_j| <= expm1(E_j + u (m - s_j) + 2u n_exp).
  2. softmax    out = sum_j w_j v_j / sum_j w_j with those e_j moves by at most 2 eps / (1 - eps) sum_j p_j |v_jd|, eps = max_j |e_j| over
                the row's keys: once through the numerator, once through the denominator (|O| <= sum p |v|).
                Keys more than FAR below the row maximum may leave expf's normal range (relative error no longer small): they are left
                out of the maximum and bounded absolutely, true and computed weight each <= exp(-FAR + 1) against l >= 1.
  3. sums       a term of O passes at most n_O roundings, a term of l at most n_l, in ANY order of summation with those path lengths
                (Higham (3.5)); the division adds one, counted in n_O: (gamma(n_O) + gamma(n_l)) sum_j p_j |v_jd|.
     Path lengths, from the two kernels' structure (not from their results):
       tiled  (csrc/lm_attn_prefill.hip)  a key costs one fmaf in its tile (a masked key adds an exact 0), a tile one rescale:
              n_O = (t + 1) + tiles + 1; l: 16 in-lane adds, the other half's, per tile one add and one rescale: n_l = 17 + 2 tiles;
              n_exp = tiles (one expf for the weight, at most one per later tile), tiles = ceil((t + 1) / 32).
       rows   (csrc/lm_attn.hip: the decode kernel, 256-key chunks, 4 or 8 waves of 8 key slots, chunk merge)  a slot takes at most 8
              keys of a chunk at two roundings each, then 3 adds and a multiply across slots, 8 adds and a multiply across waves,
              chunks adds and a multiply in the merge, the division: n_O = n_l = 32 + chunks; n_exp = 8 + 3.
The bar is the sum of 2. and 3. times (1 + 2^-10) for the second-order terms left out above.  Nothing in it is fitted to a kernel.
"""
import functools
import math

import torch

from tests import error_bounds as eb

EXPF_ULPS = 1
FAR = 80.0          # exp(-80) = 1.8e-35 is still a normal fp32 number (the smallest is 1.2e-38)
HEADS = 2
HDS = [64, 96, 128]
# name -> (B, T): the shapes of the fp64 comparison.  33: one tile and one key; 70: three streams, a ragged last tile; 300: three 128-query
# blocks; 1100: nine blocks, 35 tiles
CASES = {"rnd_1x33": (1, 33), "rnd_3x70": (3, 70), "rnd_2x300": (2, 300), "rnd_1x1100": (1, 1100), "q8_3x70": (3, 70),
         "dom_first_2x300": (2, 300), "dom_last_2x300": (2, 300)}


def rnd(*shape, seed=0, scale=1.0):
    from tests.test_gpu_lm import rnd as r
    return r(*shape, seed=seed, scale=scale)


def make_qkv(case, hd):
    """qkv [B * T, 3C] fp32 of a case.  q8: the queries x 8 (scores of standard deviation 8).  dom_first: key 0 of every stream scores
    30 above the rest for every query (the running max is set in the first tile and stays).  dom_last: the score grows by 0.25 per
    key, so every tile raises the running max and rescales what came before (by e^-8 per tile, e^-75 over the row)."""
    B, T = CASES[case]
    C = HEADS * hd
    qkv = rnd(B * T, 3 * C, seed=100 + hd + T).view(B, T, 3, HEADS, hd).clone()
    if case.startswith("q8"):
        qkv[:, :, 0] *= 8.0
    if case.startswith("dom"):
        qkv[:, :, 0, :, 0] = 4.0
        per_score = math.sqrt(hd) / 4.0          # k_0 that adds 1 to the score
        if case.startswith("dom_first"):
            qkv[:, 0, 1, :, 0] = 30.0 * per_score
        else:
            qkv[:, :, 1, :, 0] = (0.25 * per_score) * torch.arange(T, dtype=torch.float32)[None, :, None]
    return qkv.view(B * T, 3 * C).contiguous()


def split64(qkv, B, T, H):
    C = qkv.shape[1] // 3
    x = qkv.double().view(B, T, 3, H, C // H).permute(2, 0, 3, 1, 4)     # 3, B, H, T, hd
    return x[0], x[1], x[2]


def attention(qkv, B, T, H, dt=torch.float64):
    """softmax(mask(q k^T / sqrt(hd))) v in dt, [B * T, C]"""
    C = qkv.shape[1] // 3
    hd = C // H
    x = qkv.to(dt).view(B, T, 3, H, hd).permute(2, 0, 3, 1, 4)
    q, k, v = x[0], x[1], x[2]
    s = (q @ k.transpose(-1, -2)) * (1.0 / math.sqrt(hd))
    s = s.masked_fill(~torch.tril(torch.ones(T, T, dtype=torch.bool)), float("-inf"))
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B * T, C)


def _gamma(n):
    n = n.double() * eb.U
    assert float(n.max()) < 0.5
    return n / (1.0 - n)


def reference(qkv, B, T, H, path="tiled"):
    """(out64 [B * T, C], bar [B * T, C]) for the kernel named by path ("tiled" | "rows"); see the module docstring."""
    C = qkv.shape[1] // 3
    hd = C // H
    q, k, v = split64(qkv, B, T, H)
    scale = 1.0 / math.sqrt(hd)
    mask = torch.tril(torch.ones(T, T, dtype=torch.bool))
    s = ((q @ k.transpose(-1, -2)) * scale).masked_fill(~mask, float("-inf"))
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    p = e / e.sum(-1, keepdim=True)
    out = p @ v
    va = v.abs()
    pv = p @ va
    t1 = torch.arange(1, T + 1, dtype=torch.float64)[:, None]          # keys of row t: t + 1
    if path == "tiled":
        tiles = torch.ceil(t1 / 32)
        n_o, n_l, n_exp = t1 + tiles + 1, 17 + 2 * tiles, tiles
    else:
        chunks = torch.ceil(t1 / 256)
        n_o = n_l = 32 + chunks
        n_exp = torch.full_like(t1, 11.0)
    # 1. log-weight error of every key that stays in expf's normal range
    E = eb.gamma(hd + 2) * ((q.abs() @ k.abs().transpose(-1, -2)) * scale)
    gap = m - s                                                          # >= 0; +inf where masked
    near = mask & (gap <= FAR)
    loge = E + eb.U * gap + EXPF_ULPS * 2 * eb.U * n_exp
    eps = torch.expm1(torch.where(near, loge, torch.zeros_like(loge)).amax(-1, keepdim=True))
    assert float(eps.max()) < 0.5
    # 2. through the softmax, and the keys outside the normal range
    soft = 2 * eps / (1 - eps) * pv
    far = 2 * math.exp(-FAR + 1.0) * ((mask & ~near).double() @ va)
    # 3. the fp32 sums and the division
    sums = (_gamma(n_o) + _gamma(n_l)) * pv
    bar = (soft + far + sums) * (1 + 2.0 ** -10)
    flat = lambda x: x.transpose(1, 2).reshape(B * T, C)
    return flat(out), flat(bar)


@functools.lru_cache(maxsize=None)
def case(name, hd):
    """inputs, fp64 result and both bars of a case, computed once and shared (treat as read-only)"""
    B, T = CASES[name]
    qkv = make_qkv(name, hd)
    out64, bar = reference(qkv, B, T, HEADS, "tiled")
    _, bar_rows = reference(qkv, B, T, HEADS, "rows")
    return dict(B=B, T=T, qkv=qkv, out64=out64, bar=bar, bar_rows=bar_rows)
