"""GPU (-m gpu): the opt-in 16-bit prefill (omnitok_lm_set_prefill_format, GPT.set_prefill_format("w16")): the bf16 / fp16 MFMA GEMM
omnitok_lm_gemm16, the LayerNorm producer omnitok_lm_layernorm16 and the engine's prefill routed through them.

Kernel-level operands come from tests.test_gpu_lm.rnd rounded by torch (.to(torch.bfloat16 / float16)): they are exact in 16 bits, every
product is exact in fp32, so the bars are derived from the fp32 accumulation alone:
  GEMM       |y - y64| <= gamma(K + e) (|a| |w|^T + |bias| + |residual|), e = the epilogue's adds: the worst case of an fp32 sum of K + e
             terms in ANY order (Higham, Lemma 3.1 / (3.5)) -- it does not lean on tests/error_bounds.py's MFMA_ROUNDINGS assumption;
  GELU       eb.geglu_bound with val = 1: GELU_DERIV_MAX times the bar above, 0.5 |x| ERF_ABS for gelu_erf's erf_as, and the roundings;
  16-bit out rounding is monotone, so round16(g - B) <= y16 <= round16(g + B) with B the fp32 bar and torch's rounding of the ends.
Whole-model logits have no derived bound (the 16-bit roundings are discontinuous): their bar is 3 d_ref, d_ref = max |restatement in
fp32 - restatement in fp64| (tests/lm_prefill16_ref.py), computed on the CPU from the reference side alone.
"""
import argparse
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import gpt_oracle as go
from tests import error_bounds as eb
from tests import lm_prefill16_ref as pr
from tests.test_gpu_lm import rnd
from tests.test_oracle_gpt import GPT_CASES, load_gpt_case

pytestmark = pytest.mark.gpu
FMT = pr.FMT
FMTS = ["bf16", "fp16"]
SHAPES = [(1, 300, 256), (33, 320, 768), (130, 1000, 1536), (257, 520, 3072), (64, 1536, 6144)]
BAR_FACTOR = 3.0   # of d_ref: two fp32 summation orders of the restatement stay within 0.87 .. 1.2 of each other's d_ref


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def lib():
    from omnitokenizer_amd import _lib
    return _lib.load()


def gemm16(lib, a16, w16, fmt, bias=None, residual=None, y32=None, y16=None, act=0, flag=None):
    M, K = a16.shape
    N = w16.shape[0]
    rc = lib.omnitok_lm_gemm16(_p(a16), _p(w16), FMT[fmt][0], _p(bias), _p(residual), _p(y32), _p(y16), M, N, K, act, _p(flag),
                               torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.omnitok_last_error()


def wide(t16):
    return t16.cpu().to(torch.float64)


# ---- 1 / 2: the GEMM against fp64 ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gemm_case(fmt, M, N, K):
    """operands (16-bit, host), the fp64 results of the three forms and their bars; computed once per (format, shape)"""
    dt = FMT[fmt][1]
    a16, w16 = rnd(M, K, seed=1).to(dt), rnd(N, K, seed=2, scale=0.05).to(dt)
    bias, res = rnd(N, seed=3), rnd(M, N, seed=4)
    a, w, b, r = a16.double(), w16.double(), bias.double(), res.double()
    dot = a @ w.t()
    mag = a.abs() @ w.abs().t()
    pre = dot + b
    bar1 = eb.gamma(K + 1) * (mag + b.abs())
    bar2 = eb.gamma(K + 2) * (mag + b.abs() + r.abs())
    one, zero = torch.ones_like(pre), torch.zeros_like(pre)
    gelu = F.gelu(pre)
    bar3 = eb.geglu_bound(one, pre, zero, bar1)
    return dict(a16=a16, w16=w16, bias=bias, res=res, plain=pre, bar_plain=bar1, resid=pre + r, bar_resid=bar2, gelu=gelu, bar_gelu=bar3)


@pytest.mark.parametrize("M,N,K", SHAPES)
@pytest.mark.parametrize("fmt", FMTS)
def test_gemm16_against_fp64(lib, fmt, M, N, K):
    c = gemm_case(fmt, M, N, K)
    a, w, bias = c["a16"].cuda(), c["w16"].cuda(), c["bias"].cuda()
    y = torch.empty(M, N, device="cuda")
    gemm16(lib, a, w, fmt, bias=bias, y32=y)
    r0 = eb.ratio((y.cpu().double() - c["plain"]).abs(), c["bar_plain"])
    y = c["res"].cuda().clone()
    gemm16(lib, a, w, fmt, bias=bias, residual=y, y32=y)
    r1 = eb.ratio((y.cpu().double() - c["resid"]).abs(), c["bar_resid"])
    y = torch.empty(M, N, device="cuda")
    gemm16(lib, a, w, fmt, bias=bias, y32=y, act=1)
    r2 = eb.ratio((y.cpu().double() - c["gelu"]).abs(), c["bar_gelu"])
    print(f"gemm16 {fmt} M {M} N {N} K {K}: worst err / bar: plain {r0:.3f}, residual {r1:.3f}, gelu {r2:.3f}")
    assert r0 <= 1.0 and r1 <= 1.0 and r2 <= 1.0


def between(y16, lo64, hi64, dt):
    """round16(lo) <= y16 <= round16(hi) elementwise, the ends rounded by torch"""
    y = wide(y16)
    return bool(((y >= lo64.to(dt).double()) & (y <= hi64.to(dt).double())).all())


@pytest.mark.parametrize("M,N,K", SHAPES)
@pytest.mark.parametrize("fmt", FMTS)
def test_gemm16_16bit_output(lib, fmt, M, N, K):
    c = gemm_case(fmt, M, N, K)
    dt = FMT[fmt][1]
    a, w, bias = c["a16"].cuda(), c["w16"].cuda(), c["bias"].cuda()
    y16 = torch.empty(M, N, device="cuda", dtype=dt)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    gemm16(lib, a, w, fmt, bias=bias, y16=y16, act=1, flag=flag)
    g, B = c["gelu"], c["bar_gelu"]
    assert between(y16, g - B, g + B, dt)
    assert int(flag.item()) == 0 and torch.isfinite(y16).all()


def test_gemm16_fp16_output_overflow_is_flagged(lib):
    M, N, K = 33, 320, 768
    c = gemm_case("fp16", M, N, K)
    a, w = c["a16"].cuda(), c["w16"].cuda()
    col = 77
    bias = c["bias"].clone()
    bias[col] = 1e5
    y16 = torch.empty(M, N, device="cuda", dtype=torch.float16)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    gemm16(lib, a, w, "fp16", bias=bias.cuda(), y16=y16, act=1, flag=flag)
    assert int(flag.item()) == 4
    y = y16.cpu()
    assert torch.isposinf(y[:, col]).all()
    keep = torch.arange(N) != col
    assert torch.isfinite(y[:, keep]).all()
    g, B = c["gelu"], c["bar_gelu"]
    assert between(y16[:, keep.cuda()], (g - B)[:, keep], (g + B)[:, keep], torch.float16)
    # the same call in bf16 has fp32's range: no flag, 1e5 is finite
    cb = gemm_case("bf16", M, N, K)
    yb = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
    flag.zero_()
    gemm16(lib, cb["a16"].cuda(), cb["w16"].cuda(), "bf16", bias=bias.cuda(), y16=yb, act=1, flag=flag)
    assert int(flag.item()) == 0 and torch.isfinite(yb).all()


# ---- 3: one-hot exactness ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [256, 768])
@pytest.mark.parametrize("fmt,scale", [("bf16", 0.05), ("fp16", 0.05), ("fp16", 1e-6)])
def test_gemm16_one_hot_is_exact(lib, fmt, scale, K):
    """a16 = I_K: y32[k, n] must EQUAL the widened w16[n, k] -- every lane, half and k step of both operand maps and the C write (the
    weights are asymmetric: a transposed write cannot pass).  Scale 1e-6: fp16 subnormal inputs of the f16 MFMA."""
    N, dt = 300, FMT[fmt][1]
    w16 = rnd(N, K, seed=2, scale=scale).to(dt).cuda()
    want = w16.float().t().contiguous()
    if scale < 1e-3:
        sub = (want.abs() < 2.0 ** -14) & (want != 0)
        assert float(sub.float().mean()) > 0.9
    a16 = torch.eye(K, device="cuda").to(dt)
    y = torch.full((K, N), float("nan"), device="cuda")
    gemm16(lib, a16, w16, fmt, y32=y)
    assert float((want != 0).float().mean()) > 0.95
    assert torch.equal(y, want)


# ---- 4: row independence -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_gemm16_rows_are_independent_bitwise(lib, fmt):
    M, N, K, dt = 257, 1000, 1536, FMT[fmt][1]
    a16, w16 = rnd(M, K, seed=1).to(dt).cuda(), rnd(N, K, seed=2, scale=0.05).to(dt).cuda()
    bias = rnd(N, seed=3).cuda()
    full = torch.empty(M, N, device="cuda")
    gemm16(lib, a16, w16, fmt, bias=bias, y32=full, act=1)
    again = torch.empty(M, N, device="cuda")
    gemm16(lib, a16, w16, fmt, bias=bias, y32=again, act=1)
    assert torch.equal(full, again)
    part = torch.empty(33, N, device="cuda")
    gemm16(lib, a16[5:38], w16, fmt, bias=bias, y32=part, act=1)
    assert torch.equal(part, full[5:38])
    one = torch.empty(1, N, device="cuda")
    gemm16(lib, a16[256:257], w16, fmt, bias=bias, y32=one, act=1)
    assert torch.equal(one, full[256:257])
    bad = a16.clone()
    bad[:5] = float("nan")
    bad[38:130] = float("inf")
    bad[130:] = float("-inf")
    bad[200, ::2] = float("nan")
    out = torch.empty(M, N, device="cuda")
    gemm16(lib, bad, w16, fmt, bias=bias, y32=out, act=1)
    assert torch.equal(out[5:38], full[5:38]) and torch.isfinite(out[5:38]).all()
    assert not torch.isfinite(out[:5]).any()


# ---- 5: the LayerNorm producer -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,K", [(3, 256), (130, 1536)])
@pytest.mark.parametrize("fmt", FMTS)
def test_layernorm16(lib, fmt, rows, K):
    dt = FMT[fmt][1]
    x, g, b = rnd(rows, K, seed=1), rnd(K, seed=5, scale=0.1) + 1.0, rnd(K, seed=6, scale=0.1)
    y16 = torch.empty(rows, K, device="cuda", dtype=dt)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    xd, gd, bd = x.cuda(), g.cuda(), b.cuda()
    rc = lib.omnitok_lm_layernorm16(_p(xd), _p(gd), _p(bd), _p(y16), FMT[fmt][0], rows, K, _p(flag),
                                    torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.omnitok_last_error()
    ln64 = F.layer_norm(x.double(), (K,), g.double(), b.double())
    bar, _, _ = eb.layernorm_bound(x.double(), g.double(), b.double())
    assert between(y16, ln64 - bar, ln64 + bar, dt)
    assert int(flag.item()) == 0


# ---- 6: the engine on the golden models ----------------------------------------------------------------------------------------------
def make_gpt(sd, dims, fmt="fp32", prefill="fp32"):
    from omnitokenizer_amd.gpt import GPT
    V, BS, L, H, C = dims
    m = GPT(argparse.Namespace(), V, BS, n_layer=L, n_head=H, n_embd=C)
    res = m.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return m.cuda().eval().set_weight_format(fmt).set_prefill_format(prefill)


def dmax(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


@functools.lru_cache(maxsize=None)
def golden_case(name, fmt):
    g, sd, dims = load_gpt_case(name)
    V, BS, L, H, C = dims
    T = min(BS, 40)
    idx = torch.randint(0, V, (3, T), generator=torch.Generator().manual_seed(11))
    l64, k64, v64, d_ref = pr.reference(sd, idx, H, fmt)
    return dict(sd=sd, dims=dims, T=T, idx=idx, l64=l64, k64=k64, v64=v64, d_ref=d_ref, bar=BAR_FACTOR * d_ref)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", GPT_CASES)
def test_engine_prefill16_vs_restatement(name, fmt):
    """forward under PF_W16 (B = 3, T = min(block_size, 40)) against the fp64 restatement, bar 3 d_ref.  Two golden models have
    block_size 40 = T, so no position T exists for "the step after the prefill": that check prefills the first T - 1 tokens and steps
    token T - 1, whose logits are held against restatement column T - 1 (the column after that prefix) at the same bar, and the
    layer-0 cache rows of the prefix against the restatement's K/V.  Recorded, not asserted: the distance to the fp32 prefill of the
    same 16-bit engine (the figure in include/omnitok_lm.h)."""
    c = golden_case(name, fmt)
    T, idx, bar, H = c["T"], c["idx"].cuda(), c["bar"], c["dims"][3]
    m = make_gpt(c["sd"], c["dims"], fmt, "w16")
    logits, _ = m(idx)
    assert m.prefill_format == "w16" and logits.shape == c["l64"].shape and torch.isfinite(logits).all()
    e_fwd = dmax(logits, c["l64"])
    m.reset_streams(3, T)
    pre = m.prefill(idx[:, :T - 1].contiguous(), want_logits=True)
    assert torch.equal(pre, logits[:, :T - 1])          # a row does not depend on how many rows follow it
    after = m.step(idx[:, T - 1].contiguous())
    e_step = dmax(after, c["l64"][:, T - 1])
    e_kv = 0.0
    for b in range(3):
        k, v = m.cache_rows(0, b, 0, T - 1)
        assert torch.isfinite(k).all() and torch.isfinite(v).all()
        e_kv = max(e_kv, dmax(k, c["k64"][b, :, :T - 1]), dmax(v, c["v64"][b, :, :T - 1]))
    m.check_overflow()
    m.set_prefill_format("fp32")
    l32, _ = m(idx)
    print(f"{name} {fmt}: d_ref {c['d_ref']:.3e}; forward {e_fwd:.3e} = {e_fwd / c['d_ref']:.2f} d_ref, step after the prefill "
          f"{e_step:.3e} = {e_step / c['d_ref']:.2f} d_ref, layer-0 K/V {e_kv:.3e}; |PF_W16 - fp32 prefill| {dmax(logits, l32):.3e}, "
          f"max |logit| {float(c['l64'].abs().max()):.2f}")
    assert e_fwd <= bar
    assert e_step <= bar
    assert e_kv <= bar
    assert not torch.equal(logits, l32)                  # the switch is live


# ---- 7: engine invariants, bitwise ---------------------------------------------------------------------------------------------------
def test_engine_prefill16_invariants_bitwise():
    from omnitokenizer_amd import _lib
    c = golden_case("gpt_hd96", "bf16")
    idx = c["idx"].cuda()
    m = make_gpt(c["sd"], c["dims"], "bf16", "w16")
    batch, _ = m(idx)
    alone, _ = m(idx[1:2].contiguous())
    assert torch.equal(alone[0], batch[1])
    again, _ = m(idx)
    assert torch.equal(again, batch)
    tg = torch.randint(0, m.vocab_size, tuple(idx.shape), generator=torch.Generator().manual_seed(13))
    tg[:, :2] = -1
    tg = tg.cuda()
    want = m.token_losses(idx, tg)
    before = _lib.get_option("lm_loss_chunk_rows")
    try:
        _lib.set_option("lm_loss_chunk_rows", 7)
        got = m.token_losses(idx, tg)
    finally:
        _lib.set_option("lm_loss_chunk_rows", before)
    assert set(got) == set(want)
    for k in want:
        a, b = got[k], want[k]
        assert torch.equal(torch.as_tensor(a), torch.as_tensor(b)), k
    from omnitokenizer_amd import lm_losses as ll
    ref = ll.token_cross_entropy(batch, tg)
    for k in ("nll", "rank"):
        assert torch.equal(want[k], ref[k]), k


# ---- 8: state and routing ------------------------------------------------------------------------------------------------------------
def test_prefill16_state_and_routing():
    from omnitokenizer_amd import _lib
    lib = _lib.load()
    c = golden_case("gpt_hd64", "bf16")
    idx = c["idx"].cuda()
    m = make_gpt(c["sd"], c["dims"])                      # fp32 weights, fp32 prefill
    base, _ = m(idx)
    m.set_prefill_format("w16")
    with pytest.raises(_lib.OmnitokError, match=r"omnitok_lm_set_prefill_format.*omnitok_lm_set_weight_format"):
        m(idx)
    m.set_weight_format("bf16")
    l16, _ = m(idx)
    assert torch.isfinite(l16).all() and dmax(l16, c["l64"]) <= c["bar"]
    # the switch touches neither `finalized` nor the cache: no re-sync, the same cache, and a step continues the prefilled streams
    nxt = idx[:, 0].contiguous()
    m.reset_streams(3, c["T"] + 1)
    sig, cache = m._engine_sig, m.cache_bytes()
    assert sig is not None and cache > 0
    m.prefill(idx[:, :8].contiguous())
    s_ref = m.step(nxt, advance=False).clone()
    m.set_prefill_format("fp32")
    assert lib.omnitok_lm_prefill_format(m._engine) == 0
    m.set_prefill_format("w16")
    assert lib.omnitok_lm_prefill_format(m._engine) == 1 and m._engine_sig == sig and m.cache_bytes() == cache
    assert torch.equal(m.step(nxt, advance=False), s_ref)
    # PF_FP32 restored: the bits from before the switch was touched -- of the bf16 engine's fp32 prefill and of the fp32 engine
    w32r, _ = make_gpt(pr.rounded(c["sd"], "bf16"), c["dims"])(idx)
    back, _ = m.set_prefill_format("fp32")(idx)
    assert torch.equal(back, w32r) and not torch.equal(back, l16)
    again, _ = m.set_weight_format("fp32")(idx)
    assert torch.equal(again, base)


def test_prefill16_fp16_activation_overflow_is_flagged():
    c = golden_case("gpt_hd64", "fp16")
    idx = c["idx"].cuda()
    m = make_gpt(c["sd"], c["dims"], "fp16", "w16")
    m(idx)
    m.check_overflow()                                    # the unmodified model: nothing to report
    sd = {k: v.clone() for k, v in c["sd"].items()}
    sd["blocks.0.mlp.0.bias"][:] = 1e5
    bad = make_gpt(sd, c["dims"], "fp16", "w16")
    bad(idx)
    from omnitokenizer_amd import _lib
    assert _lib.load().omnitok_lm_overflowed(bad._engine, torch.cuda.current_stream().cuda_stream) == 4
    bad(idx)
    with pytest.raises(RuntimeError, match="w16.*fp16 range"):
        bad.check_overflow()
    bad.check_overflow()                                  # ... which cleared the flag
    ok = make_gpt(sd, c["dims"], "bf16", "w16")            # bf16 has fp32's range
    lg, _ = ok(idx)
    ok.check_overflow()
    assert torch.isfinite(lg).all()


# ---- 9: one production-width shape ---------------------------------------------------------------------------------------------------
def test_engine_prefill16_production_width():
    """2 layers at n_embd 1536 / 16 heads (the reference's width), V = 1000, B = 2, T = 300: K = 1536 and 6144 with ragged M (600 rows)
    and N (1000), across an attention chunk boundary (256 keys); bf16 against the restatement at the bar of the golden models."""
    V, BS, L, H, C, B, T = 1000, 320, 2, 16, 1536, 2, 300
    sd = go.synth_gpt_state(V, BS, L, H, C, seed=31)
    idx = torch.randint(0, V, (B, T), generator=torch.Generator().manual_seed(32))
    l64, _, _, d_ref = pr.reference(sd, idx, H, "bf16")
    m = make_gpt(sd, (V, BS, L, H, C), "bf16", "w16")
    logits, _ = m(idx.cuda())
    err = dmax(logits, l64)
    print(f"production width bf16: d_ref {d_ref:.3e}, forward {err:.3e} = {err / d_ref:.2f} d_ref, max |logit| {float(l64.abs().max()):.2f}")
    assert torch.isfinite(logits).all() and err <= BAR_FACTOR * d_ref
