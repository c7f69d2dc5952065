"""Derived per-element error bounds for the split-precision kernels (fp64 torch, no GPU needed).

Every bar a test asserts with this module comes from one of the functions below; each states its model and the kernel
comment whose claim it encodes.  The only numbers are the named constants of this block, each with its source.

Notation: u = 2^-24 is the fp32 unit roundoff, gamma(n) = n u / (1 - n u) the worst-case relative error of a
recursively rounded n-term chain (Higham, "Accuracy and Stability of Numerical Algorithms", 2nd ed., Lemma 3.1).
Bars are taken against the fp64 evaluation of the same fp32 operands, so they measure the kernel's own arithmetic.
"""
import math

import torch

# fp32 unit roundoff (round to nearest)
U = 2.0 ** -24
# fp16 keeps 11 significand bits: |x - fp16(x)| <= 2^-11 |x| in the normal range
U16 = 2.0 ** -11
# the fp16 hi|lo split (csrc/gemm_h2.hip "Arithmetic", csrc/attn_h2.hip, csrc/planes.h pl_store_chunk):
#   x' = x s (s an exact power of two), hi = fp16(x'), lo = fp16(x' - hi), |x' - hi - lo| <= 2^-22 |x'| in the normal range
SPLIT_REL = 2.0 ** -22
# ... and at most half the fp16 subnormal spacing 2^-24 in scaled units where hi or lo is subnormal
SPLIT_FLOOR = 2.0 ** -25
# |lo| <= 2^-11 |x'| (1 + 2^-11) + 2^-25: the bound of the dropped lo.lo' product
LO_REL = U16 * (1.0 + U16)
# the three fp16 products hi.lo' + hi.hi' + lo.hi' of x' y' leave out r y' + x' r' + r r' + lo lo'
# (x' = hi + lo + r): at most (2^-22 + 2^-22 + 2^-44 + LO_REL^2) |x' y'|
SPLIT_PRODUCT_REL = 2 * SPLIT_REL + SPLIT_REL ** 2 + LO_REL ** 2
# bf16 x 3 (csrc/gemm_x3.hip): truncation split a = a0 + a1 + a2 with |a1| < 2^-7 |a|, |a2| < 2^-15 |a| (8 significand bits
# per plane counted from each plane's own leading bit); the dropped a1 b2 + a2 b1 + a2 b2 are below
# (2^-22 + 2^-22 + 2^-30) |a b|, taken as 2^-21 + 2^-30
X3_DROP_REL = 2.0 ** -21 + 2.0 ** -30
# attention P scale before the fp16 split: 2^14 (csrc/attn_h2.hip P_SHIFT), 2^9 for the deferred-rescale variant
# ("P is scaled by 2^9 instead of 2^14"); the smaller one gives the larger absolute floor in units of max P
P_SPLIT_SHIFT = 9
# ASSUMPTION, not a sourced figure: the internal rounding of the fp16 / bf16 MFMA (v_mfma_f32_32x32x16_{f16,bf16}) is not
# documented.  Products inside one instruction are exact in fp32 (11 x 11 and 8 x 8 significand bits); the model takes at most
# this many fp32-class roundings on any product's path per instruction (one for the block sum of 16 products, one for the
# accumulate).  The GPU module's faithful ratios (tests/test_gpu_error_bounds.py) are consistent with it; a k-ordered chain
# inside the instruction would be 16.  The fp32-input MFMA is a documented k-ordered fmaf chain: one rounding per k.
MFMA_ROUNDINGS = 2
# v_exp_f32 / v_rcp_f32: 1 ulp (AMD CDNA3 ISA, "Transcendental instructions": 1 ULP accuracy); 1 ulp <= 2u relative
EXP2_ULPS = 1
RCP_ULPS = 1
# 1.0f / sqrtf(v): sqrtf within 1 ulp (HIP math library, single-precision "sqrtf" table) then a correctly rounded division
RSQRT_ULPS = 2
# erf_as (csrc/gemm_common.h): Abramowitz & Stegun 7.1.26, |erf - approximation| <= 1.5e-7 absolute (the formula's stated
# bound), plus the fp32 evaluation: rcp (1 ulp), four fmaf of |p| <= 1.1, exp2 (1 ulp) and the final fmaf, each <= 2u of
# a value <= 1.1 -> 8 ulps of 1
ERF_ABS = 1.5e-7 + 8 * 2 * U
# max over x of |d/dx (x Phi(x))| = 1.1289 at x = sqrt(2) (GELU with the exact erf)
GELU_DERIV_MAX = 1.13
# Probabilistic dot-product bar (Higham & Mary, SIAM J. Sci. Comput. 41(5), 2019, Thm 3.1): with probability at least
# 1 - 2 n exp(-lambda^2 / 2) the first-order error is <= lambda sqrt(n) u sum |a||b|.  Over the N elements one test checks
# the union bound is 2 N n exp(-lambda^2 / 2); lambda = 9 keeps it below 1e-6 for N n <= 1e11 (1e7 elements of up to 1e4
# roundings each): 2e11 exp(-40.5) = 5e-7
LAMBDA = 9.0


def gamma(n):
    """Worst-case relative error of an n-rounding fp32 chain (Higham Lemma 3.1)."""
    n = float(n)
    assert n * U < 0.5, n
    return n * U / (1.0 - n * U)


def prob_gamma(n):
    """Higham & Mary 2019 probabilistic form lambda sqrt(n) u (valid for randomised operands only: rounding errors of
    constant or structured rows correlate, so tests assert it only on random data)."""
    return LAMBDA * math.sqrt(float(n)) * U


def chain_pl(k_valid, epilogue_adds=0):
    """Roundings on a product's path in the plane GEMM (csrc/gemm_pl.h: three MFMA groups W lo.A hi | W hi.A hi | W hi.A lo
    per K step of 16, K loop stopping at ceil(k_valid / 16)) plus the epilogue adds.  The scales are exact powers of two."""
    return 3 * math.ceil(k_valid / 16) * MFMA_ROUNDINGS + epilogue_adds


def chain_h2(K, epilogue_adds=0):
    """gemm_h2.hip: three fp16 MFMA per 16-k step, as the plane GEMM."""
    return chain_pl(K, epilogue_adds)


def chain_x3(K, epilogue_adds=0):
    """gemm_x3.hip: six bf16 MFMA groups per 16-k step (a0b2 a0b1 a0b0 a1b0 a1b1 a2b0)."""
    return 6 * math.ceil(K / 16) * MFMA_ROUNDINGS + epilogue_adds


def chain_fp32(K, epilogue_adds=0):
    """gemm.hip: v_mfma_f32_32x32x2_f32, a k-ordered fmaf chain (one rounding per k)."""
    return K + epilogue_adds


def act_scale(bound):
    """h2_common.h h2_scale_of_bound, restated: s = 2^-e with bound * s in (2^14, 2^15], e clamped to [-100, 100]; 1 for a zero
    bound.  The operand scale of activation rows (per row from the row maximum, or from a static / per-clip bound)."""
    b = torch.as_tensor(bound, dtype=torch.float32)
    _, x = torch.frexp(b)
    e = (x.to(torch.float64) - 15).clamp(-100, 100)
    return torch.where(b > 0, torch.exp2(-e), torch.ones_like(e))


def weight_unscale(rowmax):
    """pl_pack_weight / h2_pack_weight, restated: a weight row is multiplied by 2^(14 - x) (rowmax = m 2^x, m in [0.5, 1)), so its
    largest element lands in [2^13, 2^14); the returned factor 2^(x - 14) undoes it (1 for a zero row)."""
    b = torch.as_tensor(rowmax, dtype=torch.float32)
    _, x = torch.frexp(b)
    return torch.where(b > 0, torch.exp2(x.to(torch.float64) - 14), torch.ones_like(b, dtype=torch.float64))


def split_repr_bound(x, scale):
    """fp16 split of x at operand scale `scale` (per row [M, 1], or a float): |x - (hi + lo) / s| <= 2^-22 |x| + 2^-25 / s
    (gemm_h2.hip: "|r| <= 2^-22 |a'|"; "elements more than 2^18 below the bound ... error <= 2^-25 of the scaled unit")."""
    return SPLIT_REL * x.abs() + SPLIT_FLOOR / scale


def fp32_repr_bound(x):
    """Plain fp32 storage of an fp64 value: u |x| (and nothing below the fp32 normal range at these magnitudes)."""
    return U * x.abs()


def l2norm_rel(d):
    """Relative error per element of fp32 l2norm(x) * scale (* 8, exact): the sum of d squares (gamma(d)), its square root and
    reciprocal (RSQRT_ULPS, halved for the square root of the sum's error), two multiplies, and the error of the fp32 rounding of
    the fp64 restatement the bar is computed from: 0.5 gamma(d) + (2 RSQRT_ULPS + 3) u."""
    return 0.5 * gamma(d) + (2 * RSQRT_ULPS + 3) * U


def split_floor(scale):
    """Absolute floor of one split operand element in unscaled units (per row tensor or float)."""
    return SPLIT_FLOOR / scale


def dot_bound(a, w, n, kind="h2", a_floor=0.0, w_floor=0.0, prob=False):
    """Per-element bound on |fl(a . w^T) - a . w^T| for fp32 operands a [M, K], w [N, K] (fp64 tensors holding fp32 values).

    kind "h2" (fp16 hi|lo planes, three products): SPLIT_PRODUCT_REL sum|a||w| + a_floor sum|w| + w_floor sum|a|, with the
    floors SPLIT_FLOOR / scale of each operand row (gemm_h2.hip "dropped lo.lo' and r terms"), plus the accumulation;
    kind "x3" (bf16 x 3): X3_DROP_REL sum|a||w| plus the accumulation; kind "fp32": the accumulation only.
    Accumulation: gamma(n) sum|a||w|, or prob_gamma(n) sum|a||w| when prob (randomised operands only)."""
    aa, ww = a.abs(), w.abs()
    s = aa @ ww.t()
    acc = (prob_gamma(n) if prob else gamma(n)) * s
    if kind == "fp32":
        return acc
    if kind == "x3":
        return acc + X3_DROP_REL * s * (1 + gamma(n))
    assert kind == "h2", kind
    af = a_floor if not torch.is_tensor(a_floor) else a_floor.reshape(-1, 1)
    wf = w_floor if not torch.is_tensor(w_floor) else w_floor.reshape(1, -1)
    rep = SPLIT_PRODUCT_REL * s + af * ww.sum(1)[None, :] * (1 + LO_REL) + wf * aa.sum(1)[:, None] * (1 + LO_REL) \
        + (af * wf) * a.shape[1]
    return acc + rep * (1 + gamma(n))


def add_bound(*terms):
    """Epilogue adds c + bias (+ residual), each rounded once: sum over the partial sums of u |partial| <= gamma(k) sum |terms|
    (k = number of adds) -- the product part is already in the chain count, this covers the bias / residual magnitudes."""
    k = len(terms) - 1
    return gamma(max(k, 1)) * sum(t.abs() for t in terms[1:]) if k > 0 else 0.0


def geglu_bound(val, gate, dval, dgate):
    """GEGLU h = gelu(gate) val (csrc/gemm_common.h gelu_erf: 0.5 x (1 + erf_as(x / sqrt 2))), given bounds dval, dgate on the
    input errors: |gelu'| <= GELU_DERIV_MAX times dgate times |val|, |gelu(gate)| dval (plus the cross term), the erf error
    ERF_ABS scaled by 0.5 |gate| |val|, and the roundings of x / sqrt 2, 1 + erf, 0.5 x, the two products: 5 u |h| + 2 u |0.5 gate val|."""
    g = 0.5 * gate * (1 + torch.erf(gate / math.sqrt(2.0)))
    h = g * val
    return (GELU_DERIV_MAX * dgate * (val.abs() + dval) + g.abs() * dval + 0.5 * gate.abs() * val.abs() * ERF_ABS
            + 6 * U * (h.abs() + gate.abs() * val.abs()))


def layernorm_bound(x, gamma_, beta=None, eps=1e-5, dx=None):
    """Two-pass LayerNorm (csrc/norm.hip row_stats + ln_apply; the PL_ROWLN epilogue of gemm_pl.h computes the same two passes
    on its fp32 row) of x [M, K] (fp64 holding fp32 values, or the fp64 truth with input error dx):
      mean: fp32 sum of K terms in any order, then / K:   |dmu| <= gamma(K) mean|x| + u |mu| (+ mean dx)
      centring d = x - mu:  |dd| <= u (|x| + |mu|) + |dmu| + dx                         (the centring term)
      q = sum d^2 (fmaf pairs), var = q / K + eps:  |dvar| <= gamma(K + 2) (var + eps) + 2 mean(|d| dd) + mean(dd^2)
      rstd = 1 / sqrtf(var):  relative error <= 0.5 |dvar| / (var + eps) (first order, doubled below) + RSQRT_ULPS 2u
      y = (d rstd) gamma (+ beta), three roundings:  |dy| <= |gamma| (dd rstd + |d| rstd e_rstd) + 3u |y| + u |beta|
    Returns (bar [M, K], mean, rstd) with mean / rstd the fp64 statistics."""
    K = x.shape[-1]
    dx = torch.zeros_like(x) if dx is None else dx
    mu = x.mean(-1, keepdim=True)
    d = x - mu
    var = (d * d).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    dmu = gamma(K) * x.abs().mean(-1, keepdim=True) + U * mu.abs() + dx.mean(-1, keepdim=True)
    dd = U * (x.abs() + mu.abs()) + dmu + dx
    dvar = gamma(K + 2) * (var + eps) + 2 * (d.abs() * dd).mean(-1, keepdim=True) + (dd * dd).mean(-1, keepdim=True)
    rel = dvar / (var + eps)
    e_rstd = torch.where(rel < 0.5, rel * (0.5 + rel), torch.full_like(rel, math.inf)) + RSQRT_ULPS * 2 * U
    y = d * rstd * gamma_
    if beta is not None:
        y = y + beta
    bar = gamma_.abs() * (dd * rstd + d.abs() * rstd * e_rstd) * (1 + 4 * U) + 3 * U * y.abs()
    if beta is not None:
        bar = bar + U * beta.abs()
    return bar, mu.squeeze(-1), rstd.squeeze(-1)


def stats_bound(x, eps=1e-5):
    """(mean, rstd) of the two-pass row statistics (norm.hip row_stats): (|dmu|, |drstd|) bounds as in layernorm_bound."""
    K = x.shape[-1]
    mu = x.mean(-1)
    d = x - mu[:, None]
    var = (d * d).mean(-1)
    rstd = 1.0 / torch.sqrt(var + eps)
    dmu = gamma(K) * x.abs().mean(-1) + U * mu.abs()
    dd = U * (x.abs() + mu.abs()[:, None]) + dmu[:, None]
    dvar = gamma(K + 2) * (var + eps) + 2 * (d.abs() * dd).mean(-1) + (dd * dd).mean(-1)
    rel = dvar / (var + eps)
    e_rstd = torch.where(rel < 0.5, rel * (0.5 + rel), torch.full_like(rel, math.inf)) + RSQRT_ULPS * 2 * U
    return dmu, rstd * e_rstd


def fold_bound(d, dd, mean, dmean, rstd, e_rstd, w, fold_cols, n, b=None, u_n=None, a_floor=0.0, w_floor=0.0):
    """LayerNorm folded into the plane GEMM (gemm_pl.h PlParams fold_*).  The operand holds the centred rows d = x - mean in fp32
    (stats_pack(center=True); |d_kernel - d| <= dd per element, see layernorm_bound's centring term), W' = W o gamma for the
    columns < fold_cols, the others the raw W:
      n <  fold_cols:  out = rstd acc + b_n;  ref = rstd (d . W'^T) + b_n
        |dout| <= rstd (1 + e_rstd) (dot bound + dd . |W'|) + rstd e_rstd |d . W'| + 2u (rstd (1 + e_rstd) |acc| + |b_n|)
      n >= fold_cols:  out = acc + mean u_n (u_n = fp32(sum_k W[n][k])); ref = x . W^T.  The error of the mean cancels exactly
        (d_kernel is x - mean_kernel), so only the centring rounding u |x - mean| . |W| enters, plus the mean add-back:
        |mean| u |u_n| (u_n rounded once), 2u (|acc| + |mean u_n|) for its product and add.
    d, mean, rstd are fp64 (exact statistics), dmean / e_rstd the kernel's mean error and rstd relative error (stats_bound);
    dd here is the centring rounding alone (u |x - mean_kernel|), the mean error is added for the folded columns."""
    dd_f = dd + dmean[:, None]
    # the operand the kernel multiplies is d + (d_kernel - d): its magnitude is at most |d| + dd_f
    dot = dot_bound(d.abs() + dd_f, w, n, "h2", a_floor=a_floor, w_floor=w_floor)
    wa = w.abs()
    acc = d @ w.t()
    out = torch.empty_like(dot)
    F_ = fold_cols
    r = rstd[:, None]
    e = e_rstd[:, None]
    bf = b[:F_].abs()[None, :] if b is not None else 0.0
    out[:, :F_] = r * (1 + e) * (dot[:, :F_] + dd_f @ wa[:F_].t()) + r * e * acc[:, :F_].abs() \
        + 2 * U * (r * (1 + e) * acc[:, :F_].abs() + bf)
    if F_ < w.shape[0]:
        mu = (mean.abs() + dmean)[:, None]
        mu_u = mu * u_n[None, F_:].abs()
        out[:, F_:] = dot[:, F_:] + dd @ wa[F_:].t() + U * mu_u + 2 * U * (acc[:, F_:].abs() + mu_u) * (1 + gamma(2))
    return out


def l2norm_bound(h, dh):
    """z = h / ||h|| per row (fp32, as pre_vq's l2norm) given |h_kernel - h| <= dh: the perturbation of the exact map,
    |dz_i| <= (|dh_i| + |z_i| ||dh||_2) / (||h|| - ||dh||_2), plus the fp32 evaluation l2norm_rel(n) |z_i| (n = row length)."""
    nh = h.norm(dim=-1, keepdim=True)
    z = h / nh
    ndh = dh.norm(dim=-1, keepdim=True)
    den = torch.where(nh > ndh, nh - ndh, torch.zeros_like(nh))
    return (dh + z.abs() * ndh) / den + l2norm_rel(h.shape[-1]) * z.abs() * (1 + U)


def softmax_attention_bound(s, v, ds, n_pv, n_l, p_split=False, v_floor=0.0, v_split=False):
    """Per-element bound on the output of softmax(s) v computed as the kernels do (attn_spatial.hip / attn_h2.hip /
    attn_temporal.hip: fp32 logits, running max, exp2, fp32 sums, one division at the end).

    s [..., Nq, Nk] fp64 logits of the kernel's fp32 operands (masked entries -inf), v [..., Nk, d], ds [..., Nq, 1] a bound on
    the logit error of each query (dot_bound of q . k plus the scale / bias roundings).
      * every probability gets a relative error e_j <= expm1(ds + ln2 (u |t| + EXP2_ULPS 2u)), t the exp2 argument
        (|t| <= 2 max|s| log2 e + P_SPLIT_SHIFT); shifting all logits by the same max cancels, so
        |dO| <= e / (1 - e) sum_j P_j |v_j - O|  (first-order |dO| <= max|ds| sum_j P_j |v_j - O|, exactly)
      * P . V: when p_split, P (scaled by 2^P_SPLIT_SHIFT) and V are fp16 hi|lo planes (SPLIT_PRODUCT_REL sum P|v|, the P floor
        2^-25 2^-P_SPLIT_SHIFT sum|v| / l with l = sum_j exp(s_j - max) >= 1, and the V floor v_floor per element); the fp32
        accumulation over n_pv roundings (keys x MFMA_ROUNDINGS / 16-key step plus the running-max rescales)
      * l = sum P: positive terms, relative gamma(n_l); then O = acc / l with RCP_ULPS 2u + u.
    """
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    p = e / l
    o = p @ v
    va = v.abs()
    spread = (p.unsqueeze(-1) * (v.unsqueeze(-3) - o.unsqueeze(-2)).abs()).sum(-2)
    sa = torch.where(torch.isfinite(s), s.abs(), torch.zeros_like(s)).amax(-1, keepdim=True)
    t = 2 * sa * (1 / math.log(2)) + P_SPLIT_SHIFT
    le = ds + math.log(2) * (U * t + EXP2_ULPS * 2 * U)
    eps = torch.expm1(le)
    bar = eps / (1 - eps) * spread
    pv = p @ va
    rep = 0.0
    if p_split:
        rep = rep + SPLIT_PRODUCT_REL * pv + SPLIT_FLOOR * 2.0 ** -P_SPLIT_SHIFT * va.sum(-2, keepdim=True) / l
    if v_split:
        rep = rep + SPLIT_PRODUCT_REL * pv * (0 if p_split else 1) + v_floor * (1 + LO_REL)
    acc = gamma(n_pv) * pv
    div = gamma(n_l) + (RCP_ULPS * 2 + 1) * U
    return (bar + rep + acc + div * (o.abs() + bar + rep + acc)) * (1 + div)


def ratio(err, bar):
    """max(err / bar) over the elements (err == 0 counts as 0 where bar == 0; a NaN error or bar counts as infinite)."""
    err = torch.where(torch.isnan(err) | torch.isnan(bar), torch.full_like(err, math.inf), err)
    bar = torch.nan_to_num(bar, nan=0.0)
    r = torch.where(bar > 0, err / bar, torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    return float(r.max())
