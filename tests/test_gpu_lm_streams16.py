"""GPU (-m gpu): the opt-in 16-bit many-stream decode step (omnitok_lm_set_streams_format, GPT.set_streams_format("w16")): the bf16 / fp16
MFMA GEMM omnitok_lm_gemm_streams16 (csrc/lm_gemm_streams16.hip) and the engine's step routed through it.

Kernel-level operands come from tests.test_gpu_lm.rnd rounded by torch (.to(torch.bfloat16 / float16)): they are exact in 16 bits and every
product of two of them is exact in fp32, so only the accumulation rounds.  Bars, as tests/test_gpu_lm_streams.py derives them for the
fp32 kernel:
  GEMM       |y - y64| <= gamma(K + e) (|x| |w|^T + |bias| + |residual|), e = the epilogue's adds: the worst case of an fp32 sum of K + e
             terms joined in ANY order (Higham, Lemma 3.1 / (3.5)) -- the block sums inside an MFMA, the wave join and the split join are
             orders of that sum, and the bar does not lean on tests/error_bounds.py's MFMA_ROUNDINGS assumption;
  GELU       eb.geglu_bound with val = 1 on the bar above (gelu_erf's erf_as and its roundings);
  16-bit out the fp32 bar plus half an ulp of the format at the largest value the bar admits: 2^-8 (bf16: 8 significand bits) or 2^-11
             (fp16) relative, and 2^-25 absolute for an fp16 subnormal.
Whole-model logits have no derived bound (the 16-bit roundings are discontinuous): their bar is 3 d_ref, BAR_FACTOR of
tests/test_gpu_lm_prefill16.py with the reason given there, d_ref = max |restatement in fp32 - restatement in fp64|
(tests/lm_prefill16_ref.py), computed on the CPU from the reference side alone.
"""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import gpt_oracle as go
from tests import error_bounds as eb
from tests import lm_prefill16_ref as pr
from tests.test_gpu_lm import rnd
from tests.test_gpu_lm_prefill16 import BAR_FACTOR
from tests.test_gpu_lm_streams import StreamsMin, dmax
from tests.test_gpu_lm_w16 import make_gpt
from tests.test_oracle_gpt import GPT_CASES, load_gpt_case

pytestmark = pytest.mark.gpu
FMT = pr.FMT
FMTS = ["bf16", "fp16"]
U16 = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
SF16_RANGE = 16
BS_ALL = [1, 17, 32, 33, 96, 97, 128]
# (N, K): one row and one block | a row tail and fewer blocks than waves, so two waves own an empty slice | two tiles' tail, one block
# per wave | the model's shapes with ragged N: 6 blocks per wave in one launch (lm_streams16_ksplit: KS == 1 up to K = 1536), KS == 2
# and KS == 4 | three blocks per wave and 513 row tiles
# | 2, 4 and 5 blocks per wave (the kernel is instantiated per block count 1 .. 6)
SHAPES = [(1, 64), (33, 128), (100, 256), (1000, 1536), (320, 3072), (1536, 6144), (16400, 768), (70, 512), (70, 1024), (70, 1280)]
KS1, KS2 = (1000, 1536), (320, 3072)      # a shape on each side of the split rule: the GEMM kernel's epilogue | the reduce kernel's


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def lib():
    from omnitokenizer_amd import _lib
    return _lib.load()


def gemm(lib, x16, w16, fmt, bias=None, res=None, y32=None, y16=None, act=0, flag=None):
    """omnitok_lm_gemm_streams16 on device tensors; returns the output it wrote (fp32 unless y16 is given)"""
    B, K = x16.shape
    N = w16.shape[0]
    if y32 is None and y16 is None:
        y32 = torch.full((B, N), float("nan"), device="cuda")
    rc = lib.omnitok_lm_gemm_streams16(_p(x16), _p(w16), FMT[fmt][0], _p(bias), _p(res), _p(y32), _p(y16), B, N, K, act, _p(flag),
                                       torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.omnitok_last_error()
    return y32 if y16 is None else y16


# ---- 1: the kernel against fp64 on the same rounded operands -------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def gemm_case(fmt, N, K):
    """128 streams of operands (16-bit, host), the fp64 results of the forms and their bars, computed once per (format, shape); a
    call of B streams takes the first B rows (a row's result does not depend on B)"""
    dt = FMT[fmt][1]
    x16, w16 = rnd(128, K, seed=1).to(dt), rnd(N, K, seed=2, scale=0.05).to(dt)
    bias, res = rnd(N, seed=3), rnd(128, N, seed=4)
    x, w, b, r = x16.double(), w16.double(), bias.double(), res.double()
    dot, mag = x @ w.t(), x.abs() @ w.abs().t()
    pre = dot + b
    bar_dot = eb.gamma(K) * mag
    bar_pre = eb.gamma(K + 1) * (mag + b.abs())
    bar_res = eb.gamma(K + 2) * (mag + b.abs() + r.abs())
    one, zero = torch.ones_like(pre), torch.zeros_like(pre)
    gelu, bar_gelu = F.gelu(pre), eb.geglu_bound(one, pre, zero, bar_pre)

    def bar16(ref, bar):
        return bar + U16[fmt] * (ref.abs() + bar) + (2.0 ** -25 if fmt == "fp16" else 0.0)

    return dict(x16=x16, w16=w16, bias=bias, res=res, dot=dot, bar_dot=bar_dot, resid=pre + r, bar_res=bar_res, gelu=gelu, bar_gelu=bar_gelu,
                bar_dot16=bar16(dot, bar_dot), bar_gelu16=bar16(gelu, bar_gelu))


@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("fmt", FMTS)
def test_gemm_streams16_against_fp64(lib, fmt, N, K):
    """Every B on both sides of the stream-tile boundaries (NT 1 .. 4) x five epilogue forms: plain (no bias), bias + residual in
    place, bias + GELU, and the 16-bit outputs of the first and the last."""
    c = gemm_case(fmt, N, K)
    dt = FMT[fmt][1]
    w, bias = c["w16"].cuda(), c["bias"].cuda()
    worst = {}
    for B in BS_ALL:
        x = c["x16"][:B].cuda()
        got = {"plain": gemm(lib, x, w, fmt), "gelu": gemm(lib, x, w, fmt, bias=bias, act=1)}
        y = c["res"][:B].cuda().clone()
        got["resid"] = gemm(lib, x, w, fmt, bias=bias, res=y, y32=y)
        got["plain16"] = gemm(lib, x, w, fmt, y16=torch.zeros(B, N, device="cuda", dtype=dt))
        got["gelu16"] = gemm(lib, x, w, fmt, bias=bias, act=1, y16=torch.zeros(B, N, device="cuda", dtype=dt))
        for name, ref, bar in (("plain", "dot", "bar_dot"), ("resid", "resid", "bar_res"), ("gelu", "gelu", "bar_gelu"),
                               ("plain16", "dot", "bar_dot16"), ("gelu16", "gelu", "bar_gelu16")):
            r = eb.ratio((got[name].cpu().double() - c[ref][:B]).abs(), c[bar][:B])
            worst[name] = max(worst.get(name, 0.0), r)
    print(f"gemm_streams16 {fmt} N {N} K {K}, B in {BS_ALL}: worst err / bar " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst


# ---- 2: one-hot exactness --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [128, 256])
@pytest.mark.parametrize("fmt,scale", [("bf16", 0.05), ("fp16", 0.05), ("fp16", 1e-6)])
def test_gemm_streams16_one_hot_is_exact(lib, fmt, scale, K):
    """x16[k] = 2^e(k) at column k alone, K streams in calls of 128: y[k, n] must EQUAL 2^e(k) w16[n, k] bit for bit -- no summation, so
    every weight row (N = 100: a ragged fourth tile), both lane halves, every k step and wave slice is checked, and a
    transposed write cannot pass (the weights are asymmetric).  Scale 1e-6: fp16 subnormal inputs of the f16 MFMA."""
    N, dt = 100, FMT[fmt][1]
    w16 = rnd(N, K, seed=2, scale=scale).to(dt).cuda()
    val = torch.tensor([2.0 ** ((k % 5) - 2) for k in range(K)], device="cuda")
    want = (w16.float() * val[None, :]).t().contiguous()      # [K, N]: exact, a power of two times a 16-bit value
    if scale < 1e-3:
        wf = w16.float()
        assert float(((wf.abs() < 2.0 ** -14) & (wf != 0)).float().mean()) > 0.9
    x16 = torch.diag(val).to(dt)
    y = torch.full((K, N), float("nan"), device="cuda")
    for k0 in range(0, K, 128):
        gemm(lib, x16[k0:k0 + 128].contiguous(), w16, fmt, y32=y[k0:k0 + 128])
    assert float((want != 0).float().mean()) > 0.95
    assert torch.equal(y, want)


# ---- 3: stream independence, bit for bit -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(33, 128), KS1, KS2])
@pytest.mark.parametrize("fmt", FMTS)
def test_gemm_streams16_streams_are_independent_bitwise(lib, fmt, N, K):
    """A stream's row (bias, GELU on; then bias + residual) is equal alone, in any slot of a batch of 17, 40 and 128, and beside
    streams full of NaN / Inf; two calls give equal bits."""
    c = gemm_case(fmt, N, K)
    x, w, bias, res = c["x16"].cuda(), c["w16"].cuda(), c["bias"].cuda(), c["res"].cuda()

    def run(rows, xs=x):
        rows = torch.as_tensor(rows, device="cuda")
        return (gemm(lib, xs[rows].contiguous(), w, fmt, bias=bias, act=1),
                gemm(lib, xs[rows].contiguous(), w, fmt, bias=bias, res=res[rows].contiguous()))

    full = run(list(range(128)))
    again = run(list(range(128)))
    g = torch.Generator().manual_seed(7)
    for f, a in zip(full, again):
        assert torch.equal(f, a) and torch.isfinite(f).all() and float(f.abs().max()) > 0
    for n in (1, 17, 40, 128):
        rows = torch.randperm(128, generator=g)[:n].tolist()
        if n == 1:
            rows = [77]
        for f, p in zip(full, run(rows)):
            assert torch.equal(p, f[rows]), n
    bad = x.clone()
    bad[0] = float("nan")
    bad[31, ::3] = float("inf")
    bad[32] = float("-inf")
    bad[100, 5] = float("nan")
    poisoned = [0, 31, 32, 100]
    keep = [r for r in range(128) if r not in poisoned]
    for f, p in zip(full, run(list(range(128)), bad)):
        assert torch.equal(p[keep], f[keep])
        assert not torch.isfinite(p[poisoned]).all(1).any()


# ---- 4: the 16-bit output and the flag -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(100, 256), KS1, KS2])
@pytest.mark.parametrize("fmt", FMTS)
def test_gemm_streams16_y16_is_round16_of_the_fp32_result(lib, fmt, N, K):
    c = gemm_case(fmt, N, K)
    dt = FMT[fmt][1]
    x, w, bias = c["x16"][:97].cuda(), c["w16"].cuda(), c["bias"].cuda()
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    y32 = gemm(lib, x, w, fmt, bias=bias, act=1)
    y16 = gemm(lib, x, w, fmt, bias=bias, act=1, y16=torch.zeros(97, N, device="cuda", dtype=dt), flag=flag)
    assert torch.equal(y16, y32.to(dt)) and float((y16 != 0).float().mean()) > 0.95
    assert int(flag.item()) == 0


@pytest.mark.parametrize("N,K", [(100, 256), KS1, KS2])
def test_gemm_streams16_fp16_output_overflow_is_flagged(lib, N, K):
    """a GELU output beyond 65504 (bias 1e5 in one column) becomes +inf in fp16 and raises bit 16, from the GEMM kernel's epilogue
    (KS == 1) and from the reduce kernel's (KS > 1); the same call in bf16 has fp32's range"""
    col = 77
    for fmt, want in (("fp16", SF16_RANGE), ("bf16", 0)):
        c = gemm_case(fmt, N, K)
        dt = FMT[fmt][1]
        bias = c["bias"].clone()
        bias[col] = 1e5
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        y16 = gemm(lib, c["x16"][:40].cuda(), c["w16"].cuda(), fmt, bias=bias.cuda(), act=1,
                   y16=torch.zeros(40, N, device="cuda", dtype=dt), flag=flag).cpu()
        assert int(flag.item()) == want
        keep = torch.arange(N) != col
        assert torch.isfinite(y16[:, keep]).all()
        assert torch.isposinf(y16[:, col]).all() if want else torch.isfinite(y16[:, col]).all()
        y32 = gemm(lib, c["x16"][:40].cuda(), c["w16"].cuda(), fmt, bias=bias.cuda(), act=1, flag=flag)     # fp32 output: never flagged
        assert int(flag.item()) == want and torch.isfinite(y32).all()


# ---- 5: the engine on the golden models ------------------------------------------------------------------------------------------------
NS = 40


def make_streams16_gpt(sd, dims, n, fmt, streams="w16", prefill="fp32"):
    return make_gpt(sd, dims, fmt).set_max_streams(n).set_prefill_format(prefill).set_streams_format(streams)


@functools.lru_cache(maxsize=None)
def golden_case(name, fmt):
    g, sd, dims = load_gpt_case(name)
    V, BS, L, H, C = dims
    T = min(BS, 24)
    idx = torch.randint(0, V, (NS, T), generator=torch.Generator().manual_seed(81))
    l64, _, _, d_ref = pr.reference(sd, idx, H, fmt)
    return dict(sd=sd, dims=dims, T=T, idx=idx, l64=l64, d_ref=d_ref, bar=BAR_FACTOR * d_ref)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", GPT_CASES)
def test_engine_streams16_vs_restatement(name, fmt):
    """40 streams with their own tokens, teacher-forced SF_W16 steps through every position (fp32 cache), against the fp64 restatement
    of the rounding points; then the steps that follow a PF_W16 prefill of the first 12 tokens, at the same bar.  Recorded, not
    asserted: the distance to the SF_FP32 step of the same 16-bit engine."""
    c = golden_case(name, fmt)
    T, idx, bar = c["T"], c["idx"].cuda(), c["bar"]
    m = make_streams16_gpt(c["sd"], c["dims"], NS, fmt, prefill="w16")
    assert m.streams_format == "w16" and m.max_streams == NS and m.cache_format == "fp32"
    m.reset_streams(NS, T)
    stepped = torch.stack([m.step(idx[:, t].contiguous()) for t in range(T)], 1)
    assert torch.isfinite(stepped).all() and float((c["l64"][0] - c["l64"][1]).abs().max()) > 10 * bar    # the streams differ
    e_step = dmax(stepped, c["l64"])
    m.reset_streams(NS, T)
    m.prefill(idx[:, :12].contiguous())
    after = torch.stack([m.step(idx[:, t].contiguous()) for t in range(12, T)], 1)
    e_after = dmax(after, c["l64"][:, 12:])
    m.check_overflow()
    m.set_streams_format("fp32").reset_streams(NS, T)
    s32 = torch.stack([m.step(idx[:, t].contiguous()) for t in range(T)], 1)
    print(f"{name} {fmt} x {NS} streams: d_ref {c['d_ref']:.3e}; stepped {e_step:.3e} = {e_step / c['d_ref']:.2f} d_ref, steps after a "
          f"PF_W16 prefill {e_after:.3e} = {e_after / c['d_ref']:.2f} d_ref; |SF_W16 - SF_FP32| {dmax(stepped, s32):.3e}, max |logit| "
          f"{float(c['l64'].abs().max()):.2f}")
    assert e_step <= bar
    assert e_after <= bar
    assert not torch.equal(stepped, s32)                 # the switch is live


# ---- 6: one production-width shape -------------------------------------------------------------------------------------------------------
def test_engine_streams16_production_width():
    """2 layers at n_embd 1536 / 16 heads (the reference's width), V = 1000: K = 1536 and 6144, every K split of the step's shapes and a
    ragged N.  48 streams with their own tokens are prefilled (PF_W16) to 126 tokens and stepped 6 times, across the 128-key attention chunk
    boundary; the logits of six streams, at least one of each stream tile, against the restatement at the bar of the golden models."""
    V, BS, L, H, C, B, T0, NSTEP = 1000, 140, 2, 16, 1536, 48, 126, 6
    sd = go.synth_gpt_state(V, BS, L, H, C, seed=91)
    idx = torch.randint(0, V, (B, T0 + NSTEP), generator=torch.Generator().manual_seed(92))
    pick = [0, 13, 31, 32, 40, 47]
    l64, _, _, d_ref = pr.reference(sd, idx[pick], H, "bf16")
    m = make_streams16_gpt(sd, (V, BS, L, H, C), B, "bf16", prefill="w16")
    d = idx.cuda()
    m.reset_streams(B, T0 + NSTEP)
    m.prefill(d[:, :T0].contiguous())
    got = torch.stack([m.step(d[:, T0 + s].contiguous()) for s in range(NSTEP)], 1)
    m.check_overflow()
    err = dmax(got[pick], l64[:, T0:])
    print(f"production width bf16 x {B} streams: d_ref {d_ref:.3e}, steps {err:.3e} = {err / d_ref:.2f} d_ref, max |logit| "
          f"{float(l64.abs().max()):.2f}")
    assert torch.isfinite(got).all() and err <= BAR_FACTOR * d_ref


# ---- 7: routing and state --------------------------------------------------------------------------------------------------------------
def steps(m, idx, B, n=3):
    m.reset_streams(B, n + 1)
    return torch.stack([m.step(idx[:B, t].contiguous()) for t in range(n)], 1)


def test_streams16_routing_and_state():
    from omnitokenizer_amd import _lib
    lib = _lib.load()
    c = golden_case("gpt_hd64", "bf16")
    idx = c["idx"].cuda()
    never = make_streams16_gpt(c["sd"], c["dims"], NS, "bf16", streams="fp32")
    base16, base17 = steps(never, idx, 16), steps(never, idx, 17)
    m = make_streams16_gpt(c["sd"], c["dims"], NS, "bf16")
    w16_16, w16_17 = steps(m, idx, 16), steps(m, idx, 17)
    assert lib.omnitok_lm_streams_format(m._engine) == 1
    assert torch.equal(w16_16, base16)                   # below "lm_streams_min" (17): the VALU kernels, the switch has no effect
    assert not torch.equal(w16_17, base17) and torch.isfinite(w16_17).all()
    with StreamsMin(1):                                  # ... and with the threshold at 1 every B takes the 16-bit kernel
        low = steps(m, idx, 16)
    assert not torch.equal(low, base16) and torch.equal(low, w16_17[:16])       # a stream's bits do not depend on its batch
    # the switch touches neither `finalized` nor the cache, and switching back restores the bits of an engine that never switched
    sig, cache = m._engine_sig, m.cache_bytes()
    m.set_streams_format("fp32")
    assert lib.omnitok_lm_streams_format(m._engine) == 0 and m._engine_sig == sig and m.cache_bytes() == cache and sig is not None
    assert torch.equal(steps(m, idx, 17), base17)
    # fp32 weights + SF_W16: an error that names both switches, whatever B is; no fallback
    f32 = make_streams16_gpt(c["sd"], c["dims"], NS, "fp32", streams="fp32")
    ok1, ok17 = steps(f32, idx, 1), steps(f32, idx, 17)
    f32.set_streams_format("w16")
    for B in (1, 17):
        f32.reset_streams(B, 4)
        with pytest.raises(_lib.OmnitokError, match=r"omnitok_lm_set_streams_format.*omnitok_lm_set_weight_format"):
            f32.step(idx[:B, 0].contiguous())
    f32.set_streams_format("fp32")
    assert torch.equal(steps(f32, idx, 1), ok1) and torch.equal(steps(f32, idx, 17), ok17)


def test_streams16_fp16_activation_overflow_is_flagged():
    from omnitokenizer_amd import _lib
    c = golden_case("gpt_hd64", "fp16")
    idx = c["idx"].cuda()
    m = make_streams16_gpt(c["sd"], c["dims"], NS, "fp16")
    steps(m, idx, 17)
    m.check_overflow()                                    # the unmodified model: nothing to report
    sd = {k: v.clone() for k, v in c["sd"].items()}
    sd["blocks.0.mlp.0.bias"][:] = 1e5                    # FC1's GELU output leaves the fp16 range
    bad = make_streams16_gpt(sd, c["dims"], NS, "fp16")
    bad.reset_streams(17, 4)
    bad.step(idx[:17, 0].contiguous())
    assert _lib.load().omnitok_lm_overflowed(bad._engine, torch.cuda.current_stream().cuda_stream) == SF16_RANGE
    bad.step(idx[:17, 1].contiguous())
    with pytest.raises(RuntimeError, match=r"set_weight_format\('bf16'\).*set_streams_format\('fp32'\)"):
        bad.check_overflow()
    bad.check_overflow()                                  # ... which cleared the flag
    bad.reset_streams(16, 4)                              # 16 streams: the VALU kernels keep fp32 activations, nothing to flag
    bad.step(idx[:16, 0].contiguous())
    bad.check_overflow()
    ok = make_streams16_gpt(sd, c["dims"], NS, "bf16")    # bf16 has fp32's range
    lg = steps(ok, idx, 17)
    ok.check_overflow()
    assert torch.isfinite(lg).all()


# ---- 8: graph replay and sampling ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sampler():
    c = golden_case("gpt_hd64", "bf16")
    return make_streams16_gpt(c["sd"], c["dims"], 24, "bf16"), c


def test_streams16_graph_replay_equals_eager(sampler):
    m, c = sampler
    idx, T = c["idx"].cuda(), 6
    m.reset_streams(24, T + 1)
    eager = torch.stack([m.step(idx[:24, t].contiguous()) for t in range(T)], 1)
    m.reset_streams(24, T + 1)
    buf, logits, replay = m.graph_step(24)
    got = []
    for t in range(T):
        buf.copy_(idx[:24, t])
        replay()
        got.append(logits.clone())
    m.check_overflow()
    assert torch.equal(torch.stack(got, 1), eager)
    # the graph keeps the launches it was captured with: the setter drops it
    assert m._graphs and m.set_streams_format("fp32")._graphs == {}
    m.set_streams_format("w16")


def test_streams16_sample_with_past_cfg_12_samples(sampler):
    """classifier-free guidance doubles the batch: 12 samples are 24 engine rows, the many-stream path"""
    from omnitokenizer_amd import gpt as og
    m, c = sampler
    V = c["dims"][0]
    x = torch.randint(0, V - 1, (12, 1), generator=torch.Generator().manual_seed(52)).cuda()
    out = {}
    for use_graph in (True, False):
        torch.manual_seed(6)
        out[use_graph] = og.sample_with_past_cfg(x, m, 12, temperature=1.0, top_k=8, top_p=1.0, cfg_ratio=1.5, use_graph=use_graph)
        m.check_overflow()
    assert torch.equal(out[True], out[False])
    assert out[True].shape == (12, 12) and int(out[True].min()) >= 0 and int(out[True].max()) < V
