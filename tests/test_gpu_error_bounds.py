"""GPU (-m gpu): the split-precision GEMMs, attention and norms held element by element to the derived bars of
tests/error_bounds.py (fp64 torch reference of the same fp32 operands), on inputs where such kernels go wrong: rows spanning
2^+-20 in one call, row maxima at and one ulp below a power of two, outlier channels x 20, zero and single-nonzero rows, M / N /
K tails, heads and clips whose V magnitudes differ by 1e4, near-one-hot and uniform P, a late running max, LayerNorm rows with
|mean| / std up to 1e4 and constant rows.  No tolerance is written here: every bar comes from tests/error_bounds.py.  Each case
prints max(err / bar)."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import error_bounds as eb
from tests.test_gpu_attn_h2 import unpack_qk, unpack_v

pytestmark = pytest.mark.gpu

F64 = torch.float64


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "needs the MI355X"
    from omnitokenizer_amd import ops as _ops
    return _ops


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).cuda()


def pow2_scale(bound):
    """h2_common.h h2_scale_of_bound."""
    _, x = math.frexp(bound)
    return 2.0 ** -(x - 15)


def act_unscale(x):
    """per-row factor that undoes the activation scale, restated from each row's maximum (eb.act_scale) -- independent of the
    pack kernels, whose scales are asserted equal to it and never used to build a bar."""
    return 1.0 / eb.act_scale(x.abs().amax(1))


def w_unscale(w):
    return eb.weight_unscale(w.abs().amax(1))


def assert_scales(name, got, expected):
    assert torch.equal(got.double(), expected), f"{name}: operand scales differ from the documented mapping"


def check(name, err, bar):
    r = eb.ratio(err, bar)
    print(f"{name}: max(err/bar) {r:.3g}")
    assert r <= 1, f"{name}: {r:.3g} of the derived bar"
    return r


def adversarial_rows(M, K, seed, k_valid=None):
    """rows spanning 2^+-20, 4 outlier channels x 20, zero / single-nonzero rows, a row maximum at 2^5 and one ulp below."""
    x = rnd(M, K, seed=seed) * torch.logspace(-20 * math.log10(2), 20 * math.log10(2), M, device="cuda")[:, None]
    x[:, 1:5] *= 20.0
    x[3] = 0.0
    x[5] = 0.0
    x[5, 7] = 3.0
    x[6] = x[6] / x[6].abs().max() * 32.0
    x[7] = x[6] * (1.0 - 2.0 ** -24)
    if k_valid is not None:
        x[:, k_valid:] = 0.0
    return x.contiguous()


STRUCTURED = (3, 5, 6, 7)


def random_rows(M):
    return [i for i in range(M) if i not in STRUCTURED]


# (M, N, K, k_valid): production K, the FF-out width with its padding, M / N tails
PL_SHAPES = [(1000, 512, 512, 512), (777, 192, 512, 512), (257, 512, 1408, 1365)]


@pytest.mark.parametrize("M,N,K,k_valid", PL_SHAPES)
@pytest.mark.parametrize("cfg", [1, 0])
def test_pl_f32_bias_residual_vs_bar(ops, M, N, K, k_valid, cfg):
    x = adversarial_rows(M, K, 1, k_valid)
    w = rnd(N, K, seed=2, scale=0.05)
    w[:, k_valid:] = 0.0
    bias, res = rnd(N, seed=3), rnd(M, N, seed=4)
    ap, asc = ops.pl_pack_rows(x)
    wp = ops.pl_pack_weight(w)
    a_un, w_un = act_unscale(x), w_unscale(w)
    assert_scales("pl_pack_rows", asc, a_un)
    assert_scales("pl_pack_weight", wp[1], w_un)
    # the operand planes themselves: the representation bound at each row's documented scale
    back = ops.pl_unpack_planes(ap, M, K) * a_un[:, None]
    check(f"pl_pack_rows planes M={M} K={K}", (back - x.double()).abs(), eb.split_repr_bound(x.double(), 1.0 / a_un[:, None]))
    xd, wd = x.double(), w.double()
    a_floor, w_floor = eb.split_floor(1.0 / a_un), eb.split_floor(1.0 / w_un)
    kv = k_valid if k_valid != K else 0
    prod = xd @ wd.t()
    plain = ops.linear_pl(ap, wp, M, N, K, a_scale=asc, cfg=cfg, k_valid=kv)
    n = eb.chain_pl(k_valid)
    check(f"linear_pl F32 M={M} N={N} K={K} cfg={cfg}", (plain.double() - prod).abs(),
          eb.dot_bound(xd, wd, n, "h2", a_floor, w_floor))
    ref = prod + bias.double() + res.double()
    bar = eb.dot_bound(xd, wd, n + 2, "h2", a_floor, w_floor) + eb.add_bound(ref, bias.double(), res.double())
    out = ops.linear_pl(ap, wp, M, N, K, a_scale=asc, bias=bias, residual=res, cfg=cfg, k_valid=kv)
    check(f"linear_pl F32 +bias +residual M={M} N={N} K={K} cfg={cfg}", (out.double() - ref).abs(), bar)
    rows = random_rows(M)
    pbar = eb.dot_bound(xd[rows], wd, n + 2, "h2", a_floor[rows], w_floor, prob=True) \
        + eb.add_bound(ref[rows], bias.double(), res.double()[rows])
    check("  probabilistic bar, random rows", (out.double() - ref)[rows].abs(), pbar)


def test_pl_geglu_hidden_planes_vs_bar(ops):
    M, K, inner, pad = 1000, 512, 1365, 1408
    x = rnd(M, K, seed=11) * torch.logspace(-3, 0, M, device="cuda")[:, None]
    x[:, :4] *= 20.0
    x[9] = 0.0
    bound = float(x.abs().max()) * 1.01
    w1 = rnd(2 * inner, K, seed=12, scale=0.05)
    w1p = ops.pack_geglu_weight(w1, pad)
    wp = ops.pl_pack_weight(w1p)
    ap, _ = ops.pl_pack_rows(x, static_bound=bound)
    out_bound = 64.0
    hid = ops.linear_pl(ap, wp, M, 2 * pad, K, a_scale_const=ops.pl_unscale(bound), epilogue=1, out_bound=out_bound)
    got = ops.pl_unpack_planes(hid, M, pad) * ops.pl_unscale(out_bound)
    xd, wd = x.double(), w1.double()
    a_floor = eb.split_floor(pow2_scale(bound))
    w_floor = eb.split_floor(1.0 / w_unscale(w1))   # per weight row (pack_geglu_weight only permutes rows and pads with zeros)
    dots = eb.dot_bound(xd, wd, eb.chain_pl(K), "h2", a_floor, w_floor)
    h = xd @ wd.t()
    val, gate = h[:, :inner], h[:, inner:]
    ref = F.gelu(gate) * val
    bar = eb.geglu_bound(val, gate, dots[:, :inner], dots[:, inner:]) + eb.split_repr_bound(ref, pow2_scale(out_bound))
    check("linear_pl GEGLU hidden planes", (got[:, :inner] - ref).abs(), bar)
    assert (got[:, inner:] == 0).all()


def test_pl_rowln_fp32_and_ln_planes_vs_bar(ops):
    M, N, K = 700, 512, 512
    x = adversarial_rows(M, K, 21)
    w = rnd(N, K, seed=22, scale=0.05)
    bias = rnd(N, seed=23)
    res = rnd(M, N, seed=24) * torch.logspace(-4, 4, M, device="cuda")[:, None]
    res[40] = 3.0                                           # constant row of the sum (x row 40 is tiny)
    res[41] = 1e4 + rnd(N, seed=25)                         # |mean| / std = 1e4
    gamma, beta = 1.0 + 0.2 * rnd(N, seed=26), 0.1 * rnd(N, seed=27)
    gamma[:4] *= 20.0
    ap, asc = ops.pl_pack_rows(x)
    wp = ops.pl_pack_weight(w)
    a_un, w_un = act_unscale(x), w_unscale(w)
    assert_scales("pl_pack_rows", asc, a_un)
    assert_scales("pl_pack_weight", wp[1], w_un)
    bound = 1.01 * (math.sqrt(N) * float(gamma.abs().max()) + float(beta.abs().max()))
    c, lnp = ops.linear_pl(ap, wp, M, N, K, a_scale=asc, bias=bias, residual=res, epilogue=2, out_bound=bound,
                           ln=(gamma, beta, 1e-5), cfg=0)
    xd, wd = x.double(), w.double()
    ref = xd @ wd.t() + bias.double() + res.double()
    bar_c = eb.dot_bound(xd, wd, eb.chain_pl(K, 2), "h2", eb.split_floor(1.0 / a_un), eb.split_floor(1.0 / w_un)) \
        + eb.add_bound(ref, bias.double(), res.double())
    check("linear_pl ROWLN fp32 rows", (c.double() - ref).abs(), bar_c)
    ln_bar, mu, rstd = eb.layernorm_bound(ref, gamma.double(), beta.double(), dx=bar_c)
    ln_ref = (ref - mu[:, None]) * rstd[:, None] * gamma.double() + beta.double()
    got = ops.pl_unpack_planes(lnp, M, N) * ops.pl_unscale(bound)
    check("linear_pl ROWLN LayerNorm planes", (got - ln_ref).abs(), ln_bar + eb.split_repr_bound(ln_ref, pow2_scale(bound)))


@pytest.mark.parametrize("kind", ["fp32", "x3", "h2"])
@pytest.mark.parametrize("M,N,K", [(1000, 512, 512), (257, 768, 1408)])
def test_linear_modes_vs_bar(ops, kind, M, N, K):
    """gemm_mode 0 / 1 / 2: the fp32-MFMA GEMM, bf16 x 3 and the fp16 x 2 GEMM with ONE A bound per launch, far above most rows."""
    x = adversarial_rows(M, K, 31)
    w = rnd(N, K, seed=32, scale=0.05)
    bias, res = rnd(N, seed=33), rnd(M, N, seed=34)
    xd, wd = x.double(), w.double()
    ref = xd @ wd.t() + bias.double() + res.double()
    if kind == "fp32":
        out = ops.linear(x, w, bias=bias, residual=res)
        bar = eb.dot_bound(xd, wd, eb.chain_fp32(K, 2), "fp32")
    elif kind == "x3":
        out = ops.linear_x3(x, w, bias=bias, residual=res)
        bar = eb.dot_bound(xd, wd, eb.chain_x3(K, 2), "x3")
    else:
        a_bound = float(x.abs().max())
        packed = ops.h2_pack_weight(w)
        out = ops.linear_h2(x, packed, a_bound, bias=bias, residual=res)
        assert_scales("h2_pack_weight", packed[1], w_unscale(w))
        bar = eb.dot_bound(xd, wd, eb.chain_h2(K, 2), "h2", eb.split_floor(pow2_scale(a_bound)),
                           eb.split_floor(1.0 / w_unscale(w)))
    bar = bar + eb.add_bound(ref, bias.double(), res.double())
    check(f"linear {kind} M={M} N={N} K={K}", (out.double() - ref).abs(), bar)


def _attn_inputs(Bn, N, h, seed, vamp=None):
    d = 64
    q, k = rnd(Bn * N, h * d, seed=seed), rnd(Bn * N, h * d, seed=seed + 1)
    v = rnd(Bn * N, h * d, seed=seed + 2)
    if vamp is not None:
        v = (v.reshape(Bn * N, h, d) * vamp.reshape(1, h, 1)).reshape(Bn * N, h * d)
    qs, ks = 1.0 + 0.1 * rnd(d, seed=seed + 3), 1.0 + 0.1 * rnd(d, seed=seed + 4)
    # head 1: uniform P (q = 0); head 2: a late running maximum -- query 3 meets its own direction at key N - 7
    q4 = q.reshape(Bn, N, h, d)
    k4 = k.reshape(Bn, N, h, d)
    q4[:, :, 1] = 0.0
    k4[:, N - 7, 2] = q4[:, 3, 2]
    return q.contiguous(), k.contiguous(), v.contiguous(), qs, ks


def _attn_bar(qp, kp, v, Bn, N, h, sq, sk, v_floor, split, bias=None, prep_rel=0.0):
    """bar [Bn*N, h*64] of the attention output on the kernel's prepared fp32 q / k (qk_prep_)."""
    d = 64
    q4 = qp.double().reshape(Bn, N, h, d).permute(0, 2, 1, 3)
    k4 = kp.double().reshape(Bn, N, h, d).permute(0, 2, 1, 3)
    v4 = v.double().reshape(Bn, N, h, d).permute(0, 2, 1, 3)
    s = q4 @ k4.transpose(-1, -2)
    if bias is not None:
        s = s + bias
    aa, kk = q4.abs(), k4.abs()
    n_s = eb.chain_h2(d) if split else eb.chain_fp32(d)
    sab = aa @ kk.transpose(-1, -2)
    ds = eb.gamma(n_s + 2) * sab + eb.U * torch.where(torch.isfinite(s), s.abs(), torch.zeros_like(s))
    if bias is not None:   # the bias enters as an fp32 value (table or slope x distance, one rounding) added once
        ds = ds + 2 * eb.U * torch.where(torch.isfinite(s), bias.abs(), torch.zeros_like(s))
    if prep_rel:
        ds = ds + 2 * prep_rel * sab
    if split:
        ds = ds + eb.SPLIT_PRODUCT_REL * sab + eb.split_floor(sk) * aa.sum(-1, keepdim=True) * (1 + eb.LO_REL) \
            + eb.split_floor(sq) * kk.sum(-1)[..., None, :] * (1 + eb.LO_REL)
    ds = ds.amax(-1, keepdim=True)
    n_pv = (eb.chain_h2(N) if split else eb.chain_fp32(N)) + N // 16
    vf = v_floor if not torch.is_tensor(v_floor) else v_floor.reshape(Bn, 1, 1, 1)
    bar = eb.softmax_attention_bound(s, v4, ds, n_pv=n_pv, n_l=N + N // 16, p_split=split, v_floor=vf, v_split=split)
    o = torch.softmax(s, -1) @ v4
    return bar.permute(0, 2, 1, 3).reshape(Bn * N, h * d), o.permute(0, 2, 1, 3).reshape(Bn * N, h * d)


@pytest.mark.parametrize("Bn,N", [(2, 256), (1, 1024)])
def test_attn_spatial_h2_and_fp32_vs_bar(ops, Bn, N):
    h = 8
    vamp = torch.tensor([1, 1, 1, 1e-6, 1, 1, 1, 1], device="cuda")   # head 3: V 2^-20 below the launch's one V bound
    q, k, v, qs, ks = _attn_inputs(Bn, N, h, 41, vamp)
    kv = torch.cat([k, v], dim=1)
    packed, bounds = ops.attn_pack(q, kv[:, :512], kv[:, 512:], N, h, qs, ks)
    out = ops.attn_spatial_h2(packed, bounds, Bn, N, h)
    qp, kvp = q.clone(), kv.clone()
    ops.qk_prep_(qp, kvp[:, :512], N, h, qs, ks)
    out32 = ops.attn_spatial(qp, kvp[:, :512], kvp[:, 512:], Bn, N, h)
    sq, sk, sv = pow2_scale(bounds[0]), pow2_scale(bounds[1]), pow2_scale(bounds[2])
    # the packed operand planes read back: q / k as prepared (qk_prep_'s arithmetic, bit for bit), V as given
    pk = packed.cpu()
    for words, t, sc, name in ((pk[0], qp, sq, "Q"), (pk[1], kvp[:, :512], sk, "K")):
        got = unpack_qk(words, Bn, N, h, 1.0).double() / sc
        check(f"attn_pack {name} planes", (got - t.double().cpu()).abs(), eb.split_repr_bound(t.double().cpu(), sc))
    got = unpack_v(pk[2], Bn, N, h, 1.0).double() / sv
    check("attn_pack V planes", (got - v.double().cpu()).abs(), eb.split_repr_bound(v.double().cpu(), sv))
    bar, ref = _attn_bar(qp, kvp[:, :512], v, Bn, N, h, sq, sk, eb.split_floor(sv), True)
    check(f"attn_spatial_h2 Bn={Bn} N={N}", (out.double() - ref).abs(), bar)
    bar32, _ = _attn_bar(qp, kvp[:, :512], v, Bn, N, h, 1.0, 1.0, 0.0, False)
    check(f"attn_spatial Bn={Bn} N={N}", (out32.double() - ref).abs(), bar32)


def test_attn_spatial_h2_per_clip_v_bounds_vs_bar(ops):
    """two clips (one sequence each) whose V magnitudes differ by 1e7 (beyond the 2^18 at which one shared scale would push the
    smaller clip's lo plane into fp16 subnormals), each packed at its own V bound: V planes read back at each clip's documented
    scale, and the output bar built from those scales."""
    Bn, N, h = 2, 256, 8
    q, k, v, qs, ks = _attn_inputs(Bn, N, h, 51)
    amp = torch.tensor([1e-4, 1e3], device="cuda").repeat_interleave(N)[:, None]
    v = (v * amp).contiguous()
    slots = torch.zeros(Bn, 2, device="cuda")
    slots[:, 1] = v.reshape(Bn, -1).abs().amax(1)
    sl = slots.reshape(-1)
    kv = torch.cat([k, v], dim=1)
    packed, bounds = ops.attn_pack(q, kv[:, :512], kv[:, 512:], N, h, qs, ks, v_bound=1.01, v_bound_dev=sl[1:],
                                   v_bound_stride=2, rows_per_clip=N)
    out = ops.attn_spatial_h2(packed, bounds, Bn, N, h, v_bound_dev=sl[1:], v_bound_stride=2, seq_per_clip=1)
    qp, kvp = q.clone(), kv.clone()
    ops.qk_prep_(qp, kvp[:, :512], N, h, qs, ks)
    sv = eb.act_scale(torch.tensor(1.01, dtype=torch.float32, device="cuda") * slots[:, 1])   # fp32 product, as the kernels form it
    got = unpack_v(packed[2].cpu(), Bn, N, h, 1.0).double().reshape(Bn, N, -1) / sv.cpu().reshape(Bn, 1, 1)
    vd = v.double().cpu().reshape(Bn, N, -1)
    check("attn_pack per-clip V planes", (got - vd).abs(), eb.split_repr_bound(vd, sv.cpu().reshape(Bn, 1, 1)))
    vf = eb.split_floor(sv)
    bar, ref = _attn_bar(qp, kvp[:, :512], v, Bn, N, h, pow2_scale(bounds[0]), pow2_scale(bounds[1]), vf, True)
    check("attn_spatial_h2 per-clip V bounds", (out.double() - ref).abs(), bar)


def test_attn_spatial_legacy_bias_vs_bar(ops):
    """the legacy continuous relative-position bias (per-head table gathered in the kernel), fp16-split and fp32 kernels."""
    from oracle import omnitok_oracle as orc
    from tests.helpers import GoldenCase
    c = GoldenCase("s1_legacy_r64_img")
    p = "encoder.enc_spatial_transformer.layers.0.1.spatial_rel_pos_bias"
    gh = gw = 16
    Bn, N, h = 2, gh * gw, 8
    full = orc.continuous_position_bias(c.sd, p, gh, gw)                  # h, N, N
    tab = orc.continuous_position_bias_table(c.sd, p, gh, gw)             # h, 2gh-1, 2gw-1
    tab_dev = tab.permute(1, 2, 0).reshape(-1, h).contiguous().cuda()
    q, k, v, qs, ks = _attn_inputs(Bn, N, h, 91)
    kv = torch.cat([k, v], dim=1)
    packed, bounds = ops.attn_pack(q, kv[:, :512], kv[:, 512:], N, h, qs, ks)
    out = ops.attn_spatial_h2(packed, bounds, Bn, N, h, tab_dev, gh, gw)
    qp, kvp = q.clone(), kv.clone()
    ops.qk_prep_(qp, kvp[:, :512], N, h, qs, ks)
    out32 = ops.attn_spatial(qp, kvp[:, :512], kvp[:, 512:], Bn, N, h, tab_dev, gh, gw)
    bias = full.double().cuda()[None]
    bar, ref = _attn_bar(qp, kvp[:, :512], v, Bn, N, h, pow2_scale(bounds[0]), pow2_scale(bounds[1]),
                         eb.split_floor(pow2_scale(bounds[2])), True, bias=bias)
    check("attn_spatial_h2 legacy bias", (out.double() - ref).abs(), bar)
    bar32, _ = _attn_bar(qp, kvp[:, :512], v, Bn, N, h, 1.0, 1.0, 0.0, False, bias=bias)
    check("attn_spatial legacy bias", (out32.double() - ref).abs(), bar32)


@pytest.mark.parametrize("T", [1, 5, 9, 17])
@pytest.mark.parametrize("causal,alibi", [(True, False), (False, False), (True, True)])
def test_attn_temporal_vs_bar(ops, T, causal, alibi):
    from oracle import omnitok_oracle as orc
    cols, h, d = 70, 8, 64
    q, kv = rnd(cols * T, h * d, seed=61), rnd(cols * T, 2 * h * d, seed=62)
    kv[:, h * d + 3 * d:h * d + 4 * d] *= 1e-4                     # head 3: V 1e4 smaller
    qs, ks = 1.0 + 0.1 * rnd(d, seed=63), 1.0 + 0.1 * rnd(d, seed=64)
    slopes = torch.tensor(orc.alibi_slopes(h), dtype=torch.float32, device="cuda") if alibi else None
    out = ops.attn_temporal(q, kv[:, :h * d], kv[:, h * d:], cols, T, h, qs, ks, causal, slopes)
    # the prepared operands in fp32 (the kernel's own l2norm / scale arithmetic is that of qk_prep_)
    qq = (F.normalize(q.double().reshape(cols, T, h, d), dim=-1) * qs.double() * 8.0).float()
    kk = (F.normalize(kv[:, :h * d].double().reshape(cols, T, h, d), dim=-1) * ks.double()).float()
    bias = torch.zeros(h, T, T, dtype=F64, device="cuda")
    if alibi:
        ar = torch.arange(T, device="cuda")
        bias = -(ar[None, :] - ar[:, None]).abs().double()[None] * slopes.double().view(h, 1, 1)
    if causal:
        bias = bias + torch.triu(torch.full((T, T), -math.inf, dtype=F64, device="cuda"), 1)
    # the kernel normalises q and k itself (qk_prep_'s arithmetic): its fp32 operands differ from qq / kk by eb.l2norm_rel(d)
    bar, ref = _attn_bar(qq.reshape(cols * T, h * d), kk.reshape(cols * T, h * d), kv[:, h * d:], cols, T, h, 1.0, 1.0, 0.0,
                         False, bias=bias[None], prep_rel=eb.l2norm_rel(d))
    check(f"attn_temporal T={T} causal={causal} alibi={alibi}", (out.double() - ref).abs(), bar)


def test_layernorm_row_stats_stats_pack_vs_bar(ops):
    M, K = 600, 512
    scale = torch.logspace(-6, 6, M, device="cuda")[:, None]
    x = rnd(M, K, seed=71) * scale + scale * torch.where(torch.arange(M, device="cuda") % 3 == 0, 1e4, 0.5)[:, None]
    x[10] = 7.25            # constant rows
    x[11] = 0.0
    x[:, :4] *= 20.0
    x = x.contiguous()
    gamma, beta = 1.0 + 0.2 * rnd(K, seed=72), 0.1 * rnd(K, seed=73)
    gamma[:4] *= 20.0
    xd = x.double()
    bar, mu, rstd = eb.layernorm_bound(xd, gamma.double(), beta.double())
    ref = (xd - mu[:, None]) * rstd[:, None] * gamma.double() + beta.double()
    check("layernorm", (ops.layernorm(x, gamma, beta).double() - ref).abs(), bar)
    dmu, drstd = eb.stats_bound(xd)
    st = ops.row_stats(x).double()
    check("row_stats mean", (st[:, 0] - mu).abs(), dmu)
    check("row_stats rstd", (st[:, 1] - rstd).abs(), drstd)
    for center in (False, True):
        planes, scales, st2 = ops.stats_pack(x, center=center)
        check(f"stats_pack(center={center}) mean", (st2[:, 0].double() - mu).abs(), dmu)
        check(f"stats_pack(center={center}) rstd", (st2[:, 1].double() - rstd).abs(), drstd)
        # the operand rows: x, or x - mean rounded once to fp32 (the kernel's own mean; its error is checked above)
        rows32 = x - st2[:, :1] if center else x
        un = act_unscale(rows32)
        assert_scales(f"stats_pack(center={center})", scales, un)
        back = ops.pl_unpack_planes(planes, M, K) * un[:, None]
        target = xd - st2[:, :1].double() if center else xd
        extra = eb.fp32_repr_bound(target) if center else 0.0
        check(f"stats_pack(center={center}) planes", (back - target).abs(),
              eb.split_repr_bound(target, 1.0 / un[:, None]) * (1 + eb.U) + extra)


@pytest.mark.parametrize("with_beta", [False, True])
def test_pl_folded_layernorm_vs_bar(ops, with_beta):
    """LayerNorm folded into the plane GEMM (stats_pack(center=True) + fold=): columns < 512 give LayerNorm(x) . W^T (+ W beta),
    the others x . W^T through the mean add-back, as the merged q | k launch; rows with |mean| / std up to 1e4, a constant row."""
    M, K, N, Fc = 640, 512, 768, 512
    sc = torch.logspace(-4, 4, M, device="cuda")[:, None]
    x = rnd(M, K, seed=81) * sc + sc * torch.where(torch.arange(M, device="cuda") % 4 == 0, 1e4, 0.3)[:, None]
    x[:, :4] *= 20.0
    x[12] = 3.5
    x = x.contiguous()
    gamma, beta = 1.0 + 0.2 * rnd(K, seed=82), 0.1 * rnd(K, seed=83)
    gamma[:4] *= 20.0
    w = rnd(N, K, seed=84, scale=0.05)
    planes, scales, st = ops.stats_pack(x, center=True)
    w2, b, u = ops.fold_layernorm_weight(w, gamma, beta if with_beta else None, rows_fold=Fc)
    wp = ops.pl_pack_weight(w2)
    out = ops.linear_pl(planes, wp, M, N, K, a_scale=scales, fold=(st, b, u, Fc))
    centred = x - st[:, :1]                       # the operand rows: x - mean_kernel rounded once
    a_un, w_un = act_unscale(centred), w_unscale(w2)
    assert_scales("stats_pack(center=True)", scales, a_un)
    assert_scales("pl_pack_weight", wp[1], w_un)
    xd, w2d = x.double(), w2.double()
    mu = xd.mean(1)
    d = xd - mu[:, None]
    rstd = 1.0 / torch.sqrt((d * d).mean(1) + 1e-5)
    dmu, drstd = eb.stats_bound(xd)
    ref = torch.empty(M, N, dtype=F64, device="cuda")
    ref[:, :Fc] = rstd[:, None] * (d @ w2d[:Fc].t()) + b[:Fc].double()
    ref[:, Fc:] = xd @ w2d[Fc:].t()
    dd = eb.U * (xd - st[:, :1].double()).abs()     # the centring rounding
    bar = eb.fold_bound(d, dd, mu, dmu, rstd, drstd / rstd, w2d, Fc, eb.chain_pl(K, 2), b=b.double(), u_n=u.double(),
                        a_floor=eb.split_floor(1.0 / a_un), w_floor=eb.split_floor(1.0 / w_un))
    check(f"linear_pl folded LayerNorm beta={with_beta}", (out.double() - ref).abs(), bar)


def test_layernorm_prevq_vs_bar(ops):
    """the encoder's last LayerNorm fused with pre_vq and its l2norm: z = l2norm(LayerNorm(x) . w^T + b), 8 channels."""
    n, a, c, dim = 2, 9, 33, 512
    M = n * a * c
    sc = torch.logspace(-3, 3, M, device="cuda")[:, None]
    x = rnd(M, dim, seed=101) * sc + sc * torch.where(torch.arange(M, device="cuda") % 5 == 0, 1e4, 0.2)[:, None]
    x[:, :4] *= 20.0
    x = x.contiguous()
    gamma, beta = 1.0 + 0.2 * rnd(dim, seed=102), 0.1 * rnd(dim, seed=103)
    w, b = rnd(8, dim, seed=104, scale=0.05), rnd(8, seed=105, scale=0.1)
    z = ops.layernorm_prevq(x, gamma, beta, w, b, n, a, c, transpose=False, l2=True)
    bar_y, mu, rstd = eb.layernorm_bound(x.double(), gamma.double(), beta.double())
    y = (x.double() - mu[:, None]) * rstd[:, None] * gamma.double() + beta.double()
    hh = y @ w.double().t() + b.double()
    dh = eb.gamma(dim + 1) * ((y.abs() + bar_y) @ w.double().abs().t() + b.double().abs()) + bar_y @ w.double().abs().t()
    ref = hh / hh.norm(dim=-1, keepdim=True)
    check("layernorm_prevq", (z.double() - ref).abs(), eb.l2norm_bound(hh, dh))
