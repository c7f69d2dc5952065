"""CPU: the derived error bounds of tests/error_bounds.py against emulations of the kernels' documented arithmetic.

Faithful emulations (csrc/gemm_h2.hip / gemm_pl.h: fp16 hi|lo planes at power-of-two scales, three products per 16-k step, fp32
accumulation; csrc/attn_h2.hip: split q / k / P / V, fp32 softmax; csrc/norm.hip: two-pass statistics) must stay inside their
bars; mutants that the old scalar bars let through (one row's lo plane dropped, P without its lo plane, ...) must not."""
import math

import pytest
import torch

from tests import error_bounds as eb

F32, F64 = torch.float32, torch.float64


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F64).float().double()


def scale_of_bound(bound):
    """h2_common.h h2_scale_of_bound: s = 2^-e with bound * s in (2^14, 2^15]."""
    b = torch.as_tensor(bound, dtype=F64)
    _, x = torch.frexp(b.float())
    s = torch.ldexp(torch.ones_like(b), -(x.double() - 15)).float().double()
    return torch.where(b > 0, s, torch.ones_like(b))


def split(x, s):
    """x (fp32 values) at scale s -> (hi, lo) fp16 planes as fp64 (planes.h pl_store_chunk)."""
    xs = (x * s).float()
    hi = xs.half()
    lo = (xs - hi.float()).half()
    return hi.double(), lo.double()


def mfma_accumulate(terms, K):
    """fp32 accumulation of per-16-k block sums (each block sum of exact products rounded once, then added once).
    terms: list of (A [M, K], W [N, K]) fp64 plane pairs; order = the kernel's product order inside a K step."""
    nk = math.ceil(K / 16)
    M, N = terms[0][0].shape[0], terms[0][1].shape[0]
    acc = torch.zeros(M, N, dtype=F32)
    for j in range(nk):
        sl = slice(16 * j, min(16 * j + 16, K))
        for a, w in terms:
            acc = acc + (a[:, sl] @ w[:, sl].t()).float()
    return acc


def plane_gemm(a, w, bias=None, res=None, a_bound=None, drop_lo_row=None, drop_product=None):
    """gemm_pl.h / gemm_h2.hip arithmetic: per-row (or static-bound) A scale, weight rows scaled to [2^13, 2^14), products
    W lo.A hi | W hi.A hi | W hi.A lo, scales removed in the epilogue, then + bias, + residual."""
    sa = scale_of_bound(a.abs().amax(1, keepdim=True) if a_bound is None else torch.tensor(a_bound, dtype=F64))
    sw = scale_of_bound(w.abs().amax(1, keepdim=True)) * 0.5
    ah, al = split(a, sa)
    wh, wl = split(w, sw)
    if drop_lo_row is not None:
        al[drop_lo_row] = 0
    terms = [(ah, wl), (ah, wh), (al, wh)]
    if drop_product is not None:
        del terms[drop_product]
    c = mfma_accumulate(terms, a.shape[1]).double() / (sa * sw.reshape(1, -1))
    c = c.float()
    if bias is not None:
        c = c + bias.float()
    if res is not None:
        c = c + res.float()
    return c.double(), sa.reshape(-1) if a_bound is None else sa, sw.reshape(-1)


def adversarial_rows(M, K, seed):
    """rows spanning 2^+-20, 4 outlier channels x 20, a zero row, a single-nonzero row, a row max at a power of two and one
    ulp below it."""
    a = rnd(M, K, seed=seed) * torch.logspace(-20 * math.log10(2), 20 * math.log10(2), M, dtype=F64)[:, None]
    a[:, 1:5] *= 20
    a[3] = 0
    a[5] = 0
    a[5, 7] = 3.0
    a[6] = a[6] / a[6].abs().max() * 2.0 ** 5
    a[7] = a[6] * (1 - 2.0 ** -24)
    return a.float().double()


SCALAR_GEMM_BAR = 3e-6  # tests/test_gpu_gemm_split.py::test_split_gemm_error_class: 3e-6 max(scale, 1) sqrt(K / 512)


@pytest.mark.parametrize("K,k_valid", [(512, 512), (1408, 1365)])
def test_plane_gemm_emulation_inside_bars_and_mutants_outside(K, k_valid):
    M, N = 96, 80
    a = adversarial_rows(M, K, seed=1)
    a[:, k_valid:] = 0
    w = rnd(N, K, seed=2) * 0.05
    w[:, k_valid:] = 0
    bias, res = rnd(N, seed=3), rnd(M, N, seed=4)
    ref = a @ w.t() + bias + res
    c, sa, sw = plane_gemm(a, w, bias, res)
    n = eb.chain_pl(k_valid, 2)
    bar = eb.dot_bound(a, w, n, "h2", a_floor=eb.split_floor(sa), w_floor=eb.split_floor(sw)) + eb.add_bound(ref, bias, res)
    r = eb.ratio((c - ref).abs(), bar)
    print(f"plane GEMM K={K} k_valid={k_valid}: faithful max(err/bar) {r:.3f}")
    assert r <= 1
    # the probabilistic bar on the random rows (rows 3..7 are structured)
    rows = [i for i in range(M) if i not in (3, 5, 6, 7)]
    pbar = eb.dot_bound(a[rows], w, n, "h2", a_floor=eb.split_floor(sa[rows]), w_floor=eb.split_floor(sw), prob=True) \
        + eb.add_bound(ref[rows], bias, res[rows])
    rp = eb.ratio((c - ref)[rows].abs(), pbar)
    print(f"  probabilistic bar: {rp:.3f}")
    assert rp <= 1
    scalar = SCALAR_GEMM_BAR * max(ref.abs().max().item(), 1.0) * math.sqrt(K / 512)
    # one small row without its A lo plane: outside the bar, inside the scalar bar of the old test
    row = M // 3
    cm, _, _ = plane_gemm(a, w, bias, res, drop_lo_row=row)
    rm = eb.ratio((cm - ref).abs(), bar)
    rmp = eb.ratio((cm - ref)[rows].abs(), pbar)
    print(f"  mutant A lo dropped for row {row}: {rm:.2f} of the worst-case bar, {rmp:.2f} of the probabilistic bar; "
          f"scalar bar passes: {(cm - ref).abs().max().item() < scalar}")
    # at K = 512 both bars catch it; at K = 1408 the worst-case bar grows with the longer chain (0.67 of it) and only the
    # probabilistic bar, which the GPU module asserts on the random rows as well, catches it
    assert rmp > 1
    if K == 512:
        assert rm > 1
    assert (cm - ref).abs().max().item() < scalar
    # one of the three products dropped everywhere
    for prod in range(3):
        cp, _, _ = plane_gemm(a, w, bias, res, drop_product=prod)
        rp = eb.ratio((cp - ref).abs(), bar)
        print(f"  mutant product {prod} dropped: {rp:.1f} of the bar")
        assert rp > 1


def test_plane_gemm_static_bound_too_large_underflows():
    M, N, K = 64, 64, 512
    a = rnd(M, K, seed=5) * torch.logspace(0, -3, M, dtype=F64)[:, None]
    w = rnd(N, K, seed=6) * 0.05
    ref = a @ w.t()
    bound = float(a.abs().max()) * 1.01
    c, sa, sw = plane_gemm(a, w, a_bound=bound)
    bar = eb.dot_bound(a, w, eb.chain_pl(K), "h2", a_floor=eb.split_floor(sa), w_floor=eb.split_floor(sw))
    r = eb.ratio((c - ref).abs(), bar)
    print(f"static bound: faithful {r:.3f}")
    assert r <= 1
    cm, _, _ = plane_gemm(a, w, a_bound=bound * 2.0 ** 30)
    rm = eb.ratio((cm - ref).abs(), bar)   # the bar keeps the scale of the true bound
    print(f"  mutant bound x 2^30: {rm:.3g} of the bar")
    assert rm > 1


def test_x3_dropped_terms_model():
    """gemm_x3.hip's truncation split: the three dropped products are below X3_DROP_REL |a b| -- and can exceed 2^-24 |a b|,
    the figure the kernel header once stated."""
    def trunc_bf16(x):
        return (x.float().view(torch.int32) & ~0xFFFF).view(F32).double()
    a, b = rnd(200000, seed=7), rnd(200000, seed=8)
    a0 = trunc_bf16(a); a1 = trunc_bf16(a - a0); a2 = a - a0 - a1
    b0 = trunc_bf16(b); b1 = trunc_bf16(b - b0); b2 = b - b0 - b1
    assert torch.equal(trunc_bf16(a2), a2) and torch.equal(trunc_bf16(b2), b2)  # exact three-way split
    dropped = (a1 * b2 + a2 * b1 + a2 * b2).abs() / (a * b).abs()
    print(f"bf16x3 dropped / |ab|: max {dropped.max().item() * 2 ** 24:.2f} x 2^-24")
    assert (dropped < eb.X3_DROP_REL).all()
    assert dropped.max().item() > 2.0 ** -24


def split_attention(q, k, v, sq, sk, sv, p_hi_only=False, drop_v_lo_head=None):
    """attn_h2.hip arithmetic on [h, N, 64]: logits from split q / k (three products per 16 channels, fp32), P = 2^14 exp(s - m)
    in fp32, split (or hi only), O = sum P v from split V (three products per 16 keys), l = fp32 sum of P, O / l."""
    h, N, d = q.shape
    qh, ql = split(q, sq)
    kh, kl = split(k, sk)
    vh, vl = split(v, sv)
    if drop_v_lo_head is not None:
        vl[drop_v_lo_head] = 0
    out = torch.empty(h, N, d, dtype=F64)
    for i in range(h):
        s = mfma_accumulate([(qh[i], kl[i]), (qh[i], kh[i]), (ql[i], kh[i])], d).double() / (sq * sk)
        s = s.float()
        m = s.amax(-1, keepdim=True)
        p = torch.exp2((s - m) * 1.4426950408889634 + 14).float()
        ph, pl = split(p.double(), 1.0)
        if p_hi_only:
            pl = torch.zeros_like(pl)
        o = mfma_accumulate([(ph, vl[i].t()), (ph, vh[i].t()), (pl, vh[i].t())], N).double() / sv
        l = p.sum(-1, keepdim=True, dtype=F32)
        out[i] = (o.float() * (1.0 / l)).double()
    return out


def attention_bar(q, k, v, sq, sk, sv):
    s = q @ k.transpose(-1, -2)
    n_s = eb.chain_h2(q.shape[-1])
    ds = torch.stack([eb.dot_bound(q[i], k[i], n_s, "h2", a_floor=eb.split_floor(sq), w_floor=eb.split_floor(sk))
                      for i in range(q.shape[0])]).amax(-1, keepdim=True) + eb.U * s.abs().amax(-1, keepdim=True)
    N = q.shape[1]
    return eb.softmax_attention_bound(s, v, ds, n_pv=eb.chain_h2(N) + N // 32, n_l=N + N // 32, p_split=True,
                                      v_floor=eb.split_floor(sv), v_split=True)


@pytest.mark.parametrize("N", [256, 1024])
def test_attention_emulation_inside_bars_and_mutants_outside(N):
    h, d = 4, 64
    qs = 1 + 0.1 * rnd(d, seed=9)
    q = (torch.nn.functional.normalize(rnd(h, N, d, seed=10), dim=-1) * qs * 8).float().double()
    k = torch.nn.functional.normalize(rnd(h, N, d, seed=11), dim=-1).float().double()
    q[0] *= 0.0                                   # head 0: uniform P
    k[1, N - 7] = q[1, 3] / 8                     # head 1: a late running max for query 3 (near one-hot)
    v = rnd(h, N, d, seed=12) * torch.tensor([1.0, 1.0, 1e-4, 1.0], dtype=F64)[:, None, None]  # head 2: V 1e4 smaller
    v = v.float().double()
    sq, sk = scale_of_bound(8 * 1.01 * float(qs.abs().max())), scale_of_bound(1.01)
    sv = scale_of_bound(1.01 * float(v.abs().max()))   # one V bound for the launch: head 2 sits 1e4 below it
    ref = torch.softmax(q @ k.transpose(-1, -2), -1) @ v
    bar = attention_bar(q, k, v, sq, sk, sv)
    o = split_attention(q, k, v, sq, sk, sv)
    r = eb.ratio((o - ref).abs(), bar)
    print(f"attention N={N}: faithful {r:.3f}")
    assert r <= 1
    om = split_attention(q, k, v, sq, sk, sv, p_hi_only=True)
    rm = eb.ratio((om - ref).abs(), bar)
    print(f"  mutant P hi only: {rm:.1f} of the bar; old 1e-5 bar passes: {(om - ref).abs().max().item() < 1e-5}")
    assert rm > 1
    om = split_attention(q, k, v, sq, sk, sv, drop_v_lo_head=2)
    rm = eb.ratio((om - ref).abs(), bar)
    print(f"  mutant V lo dropped for head 2: {rm:.1f} of the bar; old 1e-5 bar passes: {(om - ref).abs().max().item() < 1e-5}")
    assert rm > 1
    assert (om - ref).abs().max().item() < 1e-5


def two_pass_ln(x, g, b, eps, one_pass=False):
    x32 = x.float()
    mean = x32.sum(-1, keepdim=True) / x.shape[-1]
    if one_pass:
        var = (x32 * x32).sum(-1, keepdim=True) / x.shape[-1] - mean * mean
    else:
        d = x32 - mean
        var = (d * d).sum(-1, keepdim=True) / x.shape[-1]
    rstd = 1.0 / torch.sqrt(var + eps)
    return (((x32 - mean) * rstd) * g.float() + b.float()).double()


def test_layernorm_emulation_inside_bar_and_one_pass_outside():
    M, K = 64, 512
    x = rnd(M, K, seed=13) * torch.logspace(-6, 6, M, dtype=F64)[:, None]
    x = x + torch.logspace(-6, 6, M, dtype=F64)[:, None] * torch.where(torch.arange(M) % 2 == 0, 1e4, 1.0)[:, None].double()
    x[10] = 7.25                                        # constant row
    x = x.float().double()
    g, b = (1 + 0.2 * rnd(K, seed=14)), 0.1 * rnd(K, seed=15)
    g[:4] *= 20
    g, b = g.float().double(), b.float().double()
    bar, mu, rstd = eb.layernorm_bound(x, g, b)
    ref = (x - mu[:, None]) * rstd[:, None] * g + b
    y = two_pass_ln(x, g, b, 1e-5)
    r = eb.ratio((y - ref).abs(), bar)
    print(f"LayerNorm two-pass: faithful {r:.3f}")
    assert r <= 1
    ym = two_pass_ln(x, g, b, 1e-5, one_pass=True)
    rm = eb.ratio((ym - ref).abs(), bar)
    print(f"  mutant one-pass variance (|mean|/std 1e4): {rm:.3g} of the bar")
    assert rm > 1


def test_geglu_bound_covers_the_erf_approximation():
    """gelu_erf's A&S 7.1.26 erf against the exact GELU over [-12, 12]: inside geglu_bound with zero input errors."""
    x = torch.linspace(-12, 12, 200001, dtype=F64).float().double()
    xs = (x.float() * 0.70710678118654752440).double()
    ax = xs.abs()
    t = 1 / (1 + 0.3275911 * ax)
    p = ((((1.061405429 * t - 1.453152027) * t + 1.421413741) * t - 0.284496736) * t + 0.254829592) * t
    erf = torch.sign(xs) * (1 - p * torch.exp(-ax * ax))
    got = 0.5 * x * (1 + erf)
    val = torch.ones_like(x)
    bar = eb.geglu_bound(val, x, torch.zeros_like(x), torch.zeros_like(x))
    ref = torch.nn.functional.gelu(x)
    r = eb.ratio((got - ref).abs(), bar)
    print(f"gelu_erf (fp64 evaluation of A&S 7.1.26): {r:.3f} of the bar")
    assert r <= 1
