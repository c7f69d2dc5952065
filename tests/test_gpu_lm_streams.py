"""GPU (-m gpu): more than 16 streams per LM engine (omnitok_lm_set_max_streams, GPT.set_max_streams) on the many-stream MFMA GEMM
(omnitok_lm_gemm_streams, csrc/lm_gemm_mfma.hip lm_gemm_streams_kernel).

What the kernel promises (include/omnitok_lm.h): fp32 products of fp32 activations with the weight's exact fp32 value, fp32
accumulation in an order fixed by (N, K) -- so a row of the output is bit-equal whatever the batch around it holds -- and the
existing epilogue.  Bars:
  * plain + bias + residual against fp64: the forward bound of an fp32 dot product of K fused terms summed in ANY order plus the two
    epilogue adds, gamma(K + 2) (|x| |w|^T + |bias| + |residual|) elementwise (Higham, Accuracy and Stability, (3.5)); nothing measured;
  * LayerNorm + GELU against torch in fp32: test_gemv's 2e-5 sqrt(K / 1536);
  * whole-model logits against the float64 oracle: the suite's LOGIT_TOL; 16-bit engines against the oracle on rounded weights fed the
    engine's own cache, as tests/test_gpu_lm_kv16.py does;
  * K/V rows of an fp32 cache against the float64 oracle's: LOGIT_TOL as well -- they are outputs of the same LayerNorm + GEMM chain
    as the logits, of the same magnitude (|k|, |v| of order 1), after fewer layers."""
import argparse
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import gpt_oracle as go
from tests import error_bounds as eb
from tests.test_gpu_lm import LOGIT_TOL, rnd
from tests.test_gpu_lm_kv16 import engine_rows, oracle_on_cache
from tests.test_gpu_lm_w16 import make_gpt, rounded
from tests.test_oracle_gpt import GPT_CASES, load_gpt_case

pytestmark = pytest.mark.gpu
FMT = {"fp32": (0, torch.float32), "bf16": (1, torch.bfloat16), "fp16": (2, torch.float16)}


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def lib():
    from omnitokenizer_amd import _lib
    return _lib.load()


class StreamsMin:
    """sets "lm_streams_min" (the smallest batch that takes the many-stream kernel) and restores what get_option read before"""

    def __init__(self, n):
        from omnitokenizer_amd import _lib
        self.lib, self.n = _lib, n

    def __enter__(self):
        self.saved = self.lib.get_option("lm_streams_min")
        self.lib.set_option("lm_streams_min", self.n)
        return self

    def __exit__(self, *exc):
        self.lib.set_option("lm_streams_min", self.saved)


def gemm(lib, x, w, fmt, bias=None, res=None, g=None, beta=None, act=0, y=None):
    """omnitok_lm_gemm_streams on device tensors; res is added (y may be res itself)"""
    B, K = x.shape
    N = w.shape[0]
    if y is None:
        y = torch.empty(B, N, device="cuda")
    rc = lib.omnitok_lm_gemm_streams(_p(x), _p(w), FMT[fmt][0], _p(bias), _p(res), _p(g), _p(beta), _p(y), B, N, K, act,
                                     torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.omnitok_last_error()
    return y


# ---- kernel level ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=3)
def weights(N, K, fmt, scale=0.05):
    """test_gemv's weight matrix rounded by torch to fmt: (the tensor the kernel reads, on the device; its fp32 values on the host)"""
    w = rnd(N, K, seed=2, scale=scale).to(FMT[fmt][1])
    return w.cuda(), w.float()


@functools.lru_cache(maxsize=2)
def inputs(N, K):
    """128 streams of test_gemv's inputs; a call of B streams takes the first B rows (a row's result does not depend on B)"""
    x, bias, res = rnd(128, K, seed=1), rnd(N, seed=3), rnd(128, N, seed=4)
    g, beta = rnd(K, seed=5, scale=0.1) + 1.0, rnd(K, seed=6, scale=0.1)
    return x, bias, res, g, beta


@pytest.mark.parametrize("B", [5, 17, 33, 64, 128])
@pytest.mark.parametrize("N,K", [(1536, 1536), (1000, 1536), (1536, 6144), (2048, 2048), (1000, 8192), (300, 256), (8193, 768)])
@pytest.mark.parametrize("fmt", ["fp32", "bf16", "fp16"])
def test_gemm_streams(lib, fmt, N, K, B):
    """One to four stream tiles (B = 5 .. 128, ragged last tile), ragged last row tile (N = 1000, 300, 8193), 1, 3, 4, 10 and 16 K
    splits across workgroups with 2 .. 6 blocks of 32 k per wave, whole or ragged (K = 256 .. 8192).  "lm_streams_min" 1: B = 5 takes the many-stream kernel too."""
    x, bias, res, g, beta = inputs(N, K)
    x, res = x[:B].contiguous(), res[:B].contiguous()
    wd, w = weights(N, K, fmt)
    xd, bd, rd, gd, betad = (t.cuda() for t in (x, bias, res, g, beta))
    with StreamsMin(1):
        y0 = gemm(lib, xd, wd, fmt, bias=bd, res=rd).cpu()
        y1 = gemm(lib, xd, wd, fmt, bias=bd, g=gd, beta=betad, act=1).cpu()
        y2 = rd.clone()
        gemm(lib, xd, wd, fmt, res=y2, y=y2)          # residual in place, no bias
    x64, w64 = x.double(), w.double()
    dot, mag = F.linear(x64, w64), F.linear(x64.abs(), w64.abs())
    e0, bar0 = (y0.double() - (dot + bias.double() + res.double())).abs(), eb.gamma(K + 2) * (mag + bias.double().abs() + res.double().abs())
    e2, bar2 = (y2.cpu().double() - (dot + res.double())).abs(), eb.gamma(K + 2) * (mag + res.double().abs())
    tol = 2e-5 * math.sqrt(K / 1536)
    e1 = (y1 - F.gelu(F.linear(F.layer_norm(x, (K,), g, beta), w, bias))).abs().max().item()
    print(f"{fmt} B {B} N {N} K {K}: bias+residual {float((e0 / bar0).max()):.3f} of the bar, residual in place "
          f"{float((e2 / bar2).max()):.3f} of the bar, ln+gelu {e1:.2e} (tol {tol:.2e})")
    assert (e0 <= bar0).all() and (e2 <= bar2).all()
    assert e1 < tol


@pytest.mark.parametrize("fmt,N,K,scale", [("fp32", 300, 256, 0.05), ("fp32", 1536, 1536, 0.05), ("fp32", 1000, 6144, 0.05),
                                           ("bf16", 300, 256, 0.05), ("bf16", 1536, 1536, 0.05), ("bf16", 1000, 6144, 0.05),
                                           ("fp16", 300, 256, 0.05), ("fp16", 1536, 1536, 0.05), ("fp16", 1000, 6144, 0.05),
                                           ("fp16", 300, 256, 1e-6), ("fp16", 1536, 1536, 1e-6), ("fp16", 1000, 6144, 1e-6)])
def test_gemm_streams_one_hot_is_exact(lib, fmt, N, K, scale):
    """x = rows of the identity, 128 streams per call: y[k, n] must EQUAL w[n, k] -- no summation, so every lane, MFMA step, wave
    slice and K split of the kernel is checked exactly for every column, and so is the widening of 16-bit weights (scale 1e-6: fp16
    subnormals)."""
    w = rnd(N, K, seed=2, scale=scale).to(FMT[fmt][1])
    if scale < 1e-5:
        wf = w.float()
        assert float(((wf.abs() < 2.0 ** -14) & (wf != 0)).float().mean()) > 0.9
    wd, want = w.cuda(), w.cuda().float().t().contiguous()    # want[k, n] = w[n, k]
    eye = torch.eye(K, device="cuda")
    y = torch.empty(K, N, device="cuda")
    for k0 in range(0, K, 128):
        gemm(lib, eye[k0:k0 + 128], wd, fmt, y=y[k0:k0 + 128])
    assert torch.equal(y, want)
    assert float((want != 0).float().mean()) > 0.95


@pytest.mark.parametrize("fmt", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("N,K", [(1536, 1536), (1000, 6144)])
def test_stream_independence(lib, fmt, N, K):
    """Rows 3, 17 and 39 of a 40-stream call (LayerNorm, bias, GELU and residual on) are bit-equal when they are computed as a call
    of their own, in other slots of a 17-stream call, and beside a NaN and an Inf stream; two identical calls are bit-equal."""
    x, bias, res, g, beta = inputs(N, K)
    wd, _ = weights(N, K, fmt)
    xd, rd = x[:40].cuda(), res[:40].cuda()
    bd, gd, betad = bias.cuda(), g.cuda(), beta.cuda()
    rows = [3, 17, 39]

    def run(xs, rs):
        return gemm(lib, xs.contiguous(), wd, fmt, bias=bd, res=rs.contiguous(), g=gd, beta=betad, act=1)

    y40 = run(xd, rd)
    assert torch.equal(run(xd, rd), y40)
    assert torch.isfinite(y40).all() and float(y40.abs().max()) > 0
    with StreamsMin(1):
        assert torch.equal(run(xd[rows], rd[rows]), y40[rows])
    other = [20, 21, 39, 22, 23, 24, 25, 26, 3, 27, 28, 29, 30, 31, 32, 33, 17]       # 17 streams: rows 39, 3, 17 in slots 2, 8, 16
    y17 = run(xd[other], rd[other])
    assert torch.equal(y17, y40[other])
    xbad = xd.clone()
    xbad[0] = float("nan")
    xbad[1, ::7] = float("inf")
    ybad = run(xbad, rd)
    assert torch.equal(ybad[2:], y40[2:]) and not torch.isfinite(ybad[:2]).any()
    # without a LayerNorm an Inf activation meets every weight row: the whole row of y is non-finite, the other rows unchanged
    plain40 = gemm(lib, xd, wd, fmt, bias=bd)
    plainbad = gemm(lib, xbad, wd, fmt, bias=bd)
    assert torch.equal(plainbad[2:], plain40[2:]) and not torch.isfinite(plainbad[:2]).any()


# ---- engine level: the golden models ---------------------------------------------------------------------------------------------
NS = 40


def dmax(a, b):
    return float(torch.nan_to_num((a.cpu().double() - b.cpu().double()).abs(), nan=math.inf).max())


def make_streams_gpt(sd, dims, n, fmt="fp32"):
    m = make_gpt(sd, dims, fmt).set_max_streams(n)
    if fmt != "fp32":
        m.set_cache_format(fmt)
    return m


@pytest.fixture(scope="module")
def golden():
    """per (golden model, format), computed once: 40 streams with a token sequence each, stepped and prefilled (+ one step)"""
    cache = {}

    def get(name, fmt):
        if (name, fmt) not in cache:
            g, sd, dims = load_gpt_case(name)
            V, BS, L, H, C = dims
            T = min(BS - 2, 40)
            idx = torch.randint(0, V, (NS, T + 1), generator=torch.Generator().manual_seed(31))
            m = make_streams_gpt(sd, dims, NS, fmt)
            assert m.max_streams == NS and m.weight_format == fmt and m.cache_format == fmt
            d = idx.cuda()
            m.reset_streams(NS, T + 4)
            stepped = torch.stack([m.step(d[:, t].contiguous()) for t in range(T + 1)], 1).cpu()
            rows_s = engine_rows(m, NS, T + 1)
            nbytes, max_len = m.cache_bytes(), m._cache_shape[1]
            m.reset_streams(NS, T + 4)
            batched = m.prefill(d[:, :T].contiguous(), want_logits=True).cpu()
            after = m.step(d[:, T].contiguous()).cpu()
            rows_p = engine_rows(m, NS, T + 1)
            m.check_overflow()
            cache[name, fmt] = dict(sd=sd, dims=dims, T=T, idx=idx, stepped=stepped, batched=batched, after=after, rows_s=rows_s,
                                    rows_p=rows_p, bytes=nbytes, max_len=max_len)
        return cache[name, fmt]
    return get


@pytest.mark.parametrize("name", GPT_CASES)
def test_forty_streams_vs_fp64(golden, name):
    """Stepped logits of every position, the prefill's and the step after it against the float64 oracle; the K/V rows of streams 0,
    16 and 39 against the oracle's.  Every stream has its own tokens: mixed-up streams cannot pass."""
    c = golden(name, "fp32")
    V, BS, L, H, C = c["dims"]
    T, idx = c["T"], c["idx"]
    sd64 = {k: v.double() for k, v in c["sd"].items()}
    with torch.no_grad():
        ref, kv = go.forward_with_past(sd64, idx, H, None)
    assert float((ref[0] - ref[1]).abs().max()) > 100 * LOGIT_TOL      # the streams differ
    es, ep, ea = dmax(c["stepped"], ref), dmax(c["batched"], ref[:, :T]), dmax(c["after"], ref[:, T])
    ek = max(dmax(rows[i][j][b], kv[i][j][b]) for rows in (c["rows_s"], c["rows_p"]) for i in range(L) for j in (0, 1)
             for b in (0, 16, 39))
    print(f"{name} x {NS} streams: stepped {es:.2e}, prefill {ep:.2e}, step after prefill {ea:.2e}, K/V rows {ek:.2e} (tol {LOGIT_TOL:.0e})")
    assert es < LOGIT_TOL and ep < LOGIT_TOL and ea < LOGIT_TOL and ek < LOGIT_TOL
    assert c["bytes"] == L * 2 * NS * c["max_len"] * C * 4


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("name", GPT_CASES)
def test_forty_streams_16bit_weights_and_cache(golden, name, fmt):
    """16-bit weights + a 16-bit cache: logits against the oracle on rounded(sd) fed the engine's own cache (tests/test_gpu_lm_kv16.py),
    at LOGIT_TOL; the cached rows are fixed points of the rounding and take half the fp32 cache's bytes."""
    c, c32 = golden(name, fmt), golden(name, "fp32")
    V, BS, L, H, C = c["dims"]
    T, idx, dt = c["T"], c["idx"], FMT[fmt][1]
    rsd = rounded(c["sd"], fmt)
    es = dmax(c["stepped"], oracle_on_cache(rsd, idx, H, c["rows_s"]))
    ref_p = oracle_on_cache(rsd, idx, H, c["rows_p"])
    ep, ea = dmax(c["batched"], ref_p[:, :T]), dmax(c["after"], ref_p[:, T])
    print(f"{name} {fmt} x {NS} streams: stepped {es:.2e}, prefill {ep:.2e}, step after prefill {ea:.2e} (tol {LOGIT_TOL:.0e})")
    assert es < LOGIT_TOL and ep < LOGIT_TOL and ea < LOGIT_TOL
    for rows in (c["rows_s"], c["rows_p"]):
        for k, v in rows:
            assert torch.equal(k.to(dt).float(), k) and torch.equal(v.to(dt).float(), v)
            assert float((k != 0).float().mean()) > 0.95 and float((v != 0).float().mean()) > 0.95
    assert c["bytes"] * 2 == c32["bytes"] and c["bytes"] > 0
    assert dmax(c["stepped"], c32["stepped"]) > LOGIT_TOL       # the formats are live


@pytest.mark.parametrize("B", [17, 72, 128])
def test_valu_groups_serve_more_than_16_streams(B):
    """Both paths work for every B <= 128: with "lm_streams_min" above B the step of B streams runs the <= 16-stream kernels in
    groups of 8 / 4 / 2 / 1.  Stepped with advance on (the default, and what a captured graph replays) over 6 positions against the
    float64 oracle: pos and cache_len of EVERY stream move -- streams 64 .. B - 1 included --, eagerly and under graph replay, and
    the many-stream kernel on the same streams agrees within the two paths' common bar."""
    g, sd, dims = load_gpt_case("gpt_hd64")
    V, BS, L, H, C = dims
    T = 6
    m = make_gpt(sd, dims).set_max_streams(B)
    idx = torch.randint(0, V, (B, T), generator=torch.Generator().manual_seed(71))
    sd64 = {k: v.double() for k, v in sd.items()}
    with torch.no_grad():
        ref = go.forward(sd64, idx, H)
    d = idx.cuda()
    out = {}
    for name, smin, graph in (("valu", 129, False), ("valu, graph", 129, True), ("mfma", 1, False)):
        with StreamsMin(smin):
            m._graphs = {}                     # the kernels are chosen when the step is captured
            m.reset_streams(B, T + 2)
            if graph:
                buf, logits, replay = m.graph_step(B)
                got = []
                for t in range(T):
                    buf.copy_(d[:, t])
                    replay()
                    got.append(logits.clone())
            else:
                got = [m.step(d[:, t].contiguous()) for t in range(T)]
            m._graphs = {}
        m.check_overflow()
        assert torch.equal(m._len[:B].cpu(), torch.full((B,), T, dtype=torch.int32)), name
        assert torch.equal(m._pos[:B].cpu(), torch.full((B,), T, dtype=torch.int32)), name
        out[name] = torch.stack(got, 1)
        e = dmax(out[name], ref)
        print(f"{B} streams, {name}: {e:.2e} (tol {LOGIT_TOL:.0e})")
        assert e < LOGIT_TOL, name
    assert torch.equal(out["valu"], out["valu, graph"])
    k, _ = m.cache_rows(0, B - 1, 0, T)
    assert float((k != 0).float().mean()) > 0.95      # the last stream wrote T distinct rows
    assert len({tuple(r.tolist()) for r in k[0]}) == T


# ---- engine level: the reference's widths ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,H,V", [(1536, 24, 1000), (2048, 16, 8193)])
def test_reference_widths_ragged_lengths(C, H, V):
    """Two layers at n_embd 1536 / 2048: every GEMM shape of the reference's step (K = C and 4 C, several K splits, a vocabulary that
    is no multiple of the row tile), 48 streams whose caches end on both sides of the 128-key chunk boundary, 4 teacher-forced steps
    against float64.  Then streams 0 .. 15 again from the same lengths as a batch of 16 with "lm_streams_min" 1: the same bits."""
    from omnitokenizer_amd.gpt import GPT
    B, BS, L, NSTEP = 48, 140, 2, 4
    sd = go.synth_gpt_state(V, BS, L, H, C, seed=C + H)
    m = GPT(argparse.Namespace(), V, BS, n_layer=L, n_head=H, n_embd=C)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval().set_max_streams(B)
    seqs = torch.randint(0, V, (B, BS), generator=torch.Generator().manual_seed(C * 100 + H)).cuda()
    sd64 = {k: v.cuda().double() for k, v in sd.items()}
    with torch.no_grad():
        ref = go.forward(sd64, seqs[:, :136], H)       # [B, 136, V] float64: one causal forward covers every position
    del sd64
    lens = [126 + (5 * b) % 6 for b in range(B)]       # 126 .. 131, mixed over the streams and over every stream tile
    assert set(lens) == set(range(126, 132))
    Lt = torch.tensor(lens, dtype=torch.int32, device="cuda")
    m.reset_streams(B, 136)
    assert m._cache_shape == (B, 136)
    lg = m.prefill(seqs[:, :131].contiguous(), want_logits=True)
    e = dmax(lg, ref[:, :131])
    assert e < LOGIT_TOL, f"prefill: {e:.2e}"
    ar = torch.arange(B, device="cuda")

    def steps(n):
        m._len[:n] = Lt[:n]
        m._pos[:n] = Lt[:n]
        out = []
        for s in range(NSTEP):
            out.append(m.step(seqs[ar[:n], Lt[:n].long() + s].contiguous()).clone())
        m.check_overflow()
        return out

    got = steps(B)
    errs = [dmax(got[s], torch.stack([ref[b, lens[b] + s] for b in range(B)])) for s in range(NSTEP)]
    print(f"C {C} H {H} V {V} x {B} streams: per step {['%.2e' % x for x in errs]}")
    assert max(errs) < LOGIT_TOL
    with StreamsMin(1):
        again = steps(16)
    for s in range(NSTEP):
        assert torch.equal(again[s], got[s][:16]), s


# ---- beyond 4 GiB --------------------------------------------------------------------------------------------------------------------
def test_cache_slabs_beyond_4gib():
    """128 streams x 8192 positions x 1536 in fp32: one K slab is 6.4 GB (stream 86 is the first whose K rows lie wholly past 4 GiB)
    and the V slab starts at 6.4 GB.  3 steps of 128 distinct sequences: logits of streams 0, 86 and 127 and stream 127's cached
    rows against float64."""
    free, _ = torch.cuda.mem_get_info()
    if free < 20 * 2 ** 30:
        pytest.skip(f"needs 20 GB of free device memory for a 12.9 GB cache, {free / 2 ** 30:.1f} GB are free")
    from omnitokenizer_amd.gpt import GPT
    V, BS, L, H, C, B, T = 1000, 8192, 1, 16, 1536, 128, 3
    sd = go.synth_gpt_state(V, BS, L, H, C, seed=41)
    m = GPT(argparse.Namespace(), V, BS, n_layer=L, n_head=H, n_embd=C)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval().set_max_streams(B)
    idx = torch.randint(0, V, (B, T), generator=torch.Generator().manual_seed(42))
    m.reset_streams(B, 8192)
    assert m._cache_shape == (B, 8192) and m.cache_bytes() == 2 * B * 8192 * C * 4 > 12e9
    d = idx.cuda()
    got = torch.stack([m.step(d[:, t].contiguous()) for t in range(T)], 1).cpu()
    m.check_overflow()
    pick = [0, 86, 127]
    sd64 = {k: v.double() for k, v in sd.items()}
    with torch.no_grad():
        ref, kv = go.forward_with_past(sd64, idx[pick], H, None)
    e = dmax(got[pick], ref)
    k, v = m.cache_rows(0, 127, 0, T)
    ek = max(dmax(k, kv[0][0][2]), dmax(v, kv[0][1][2]))
    print(f"128 streams, 12.9 GB cache: logits of streams {pick} {e:.2e}, K/V rows of stream 127 {ek:.2e} (tol {LOGIT_TOL:.0e})")
    assert e < LOGIT_TOL and ek < LOGIT_TOL
    assert float((k != 0).float().mean()) > 0.95 and float((v != 0).float().mean()) > 0.95
    del m
    torch.cuda.empty_cache()


def test_a_cache_the_device_cannot_hold_is_an_error_not_a_half_allocated_engine(lib):
    """128 streams x 8192 positions of the reference's 24 x 1536 model are 618 GB in fp32: omnitok_lm_alloc_cache returns hipMalloc's
    error, the engine has no cache afterwards (a step asks for one), and a cache that fits can be allocated right after."""
    from omnitokenizer_amd._lib import OmnitokLmConfig
    h = ctypes.c_void_p()
    assert lib.omnitok_lm_create(ctypes.byref(OmnitokLmConfig(8192, 8192, 24, 16, 1536)), ctypes.byref(h)) == 0
    try:
        assert lib.omnitok_lm_set_max_streams(h, 128) == 0
        assert lib.omnitok_lm_alloc_cache(h, 2, 64) == 0 and lib.omnitok_lm_cache_bytes(h) == 2 * 24 * 2 * 64 * 1536 * 4
        rc = lib.omnitok_lm_alloc_cache(h, 128, 8192)
        assert rc == -2 and b"hipMalloc" in lib.omnitok_last_error(), (rc, lib.omnitok_last_error())
        assert lib.omnitok_lm_cache_bytes(h) == 0
        k = torch.empty(16, 1, 96, device="cuda")
        assert lib.omnitok_lm_cache_read(h, 0, 0, 0, 1, _p(k), _p(k), None) == -3 and b"no cache" in lib.omnitok_last_error()
        assert lib.omnitok_lm_alloc_cache(h, 128, 64) == 0 and lib.omnitok_lm_cache_bytes(h) == 128 * 24 * 2 * 64 * 1536 * 4
    finally:
        lib.omnitok_lm_destroy(h)
    torch.cuda.synchronize()


# ---- sampling ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sampler():
    g, sd, dims = load_gpt_case("gpt_hd64")
    return make_streams_gpt(sd, dims, 24), dims


def test_sample_with_past_24_streams(sampler):
    from omnitokenizer_amd import gpt as og
    m, (V, BS, L, H, C) = sampler
    x = torch.randint(0, V, (24, 3), generator=torch.Generator().manual_seed(51)).cuda()
    out = {}
    for use_graph in (True, False):
        torch.manual_seed(5)
        out[use_graph] = og.sample_with_past(x, m, 12, temperature=1.0, top_k=8, top_p=1.0, use_graph=use_graph)
        m.check_overflow()
    assert torch.equal(out[True], out[False])
    assert out[True].shape == (24, 12) and int(out[True].min()) >= 0 and int(out[True].max()) < V
    assert len({tuple(r.tolist()) for r in out[True]}) > 12       # the streams are not copies of each other
    tok, lg = og.sample_with_past(x, m, 12, sample_logits=False, return_logits=True)
    assert lg.shape == (24, 12, V) and torch.equal(tok, lg.argmax(-1))
    first = (lg == lg.max(-1, keepdim=True).values).int().argmax(-1)      # the lowest index among equal maxima
    assert torch.equal(tok, first)


def test_sample_with_past_cfg_12_samples(sampler):
    """classifier-free guidance doubles the batch: B = 12 samples are 24 engine rows"""
    from omnitokenizer_amd import gpt as og
    m, (V, BS, L, H, C) = sampler
    x = torch.randint(0, V - 1, (12, 1), generator=torch.Generator().manual_seed(52)).cuda()
    out = {}
    for use_graph in (True, False):
        torch.manual_seed(6)
        out[use_graph] = og.sample_with_past_cfg(x, m, 12, temperature=1.0, top_k=8, top_p=1.0, cfg_ratio=1.5, use_graph=use_graph)
        m.check_overflow()
    assert torch.equal(out[True], out[False])
    assert out[True].shape == (12, 12) and int(out[True].min()) >= 0 and int(out[True].max()) < V
    tok, lg = og.sample_with_past_cfg(x, m, 12, sample_logits=False, cfg_ratio=1.5, return_logits=True)
    first = (lg == lg.max(-1, keepdim=True).values).int().argmax(-1)
    assert lg.shape == (12, 12, V) and torch.equal(tok, first)
    with pytest.raises(ValueError, match="at most 24 streams"):
        og.sample_with_past_cfg(torch.zeros(13, 1, dtype=torch.long, device="cuda"), m, 4)


# ---- the switch ----------------------------------------------------------------------------------------------------------------------
def test_switch_semantics():
    g, sd, dims = load_gpt_case("gpt_hd64")
    V, BS, L, H, C = dims
    m = make_gpt(sd, dims)
    assert m.max_streams == 16
    with pytest.raises(ValueError, match="at most 16 streams"):
        m.reset_streams(17, 8)
    x = torch.randint(0, V, (24, 4), generator=torch.Generator().manual_seed(61)).cuda()
    _, _, h = m.forward_with_past(x[:16], past=None)
    m.graph_step(16)
    assert m._graphs
    ml = m._cache_shape[1]
    bytes16 = m.cache_bytes()
    assert m._cache_shape == (16, ml) and bytes16 > 0
    # on a live model: the cache, the graphs and the earlier handles go
    assert m.set_max_streams(24) is m
    assert m._graphs == {} and m._cache_shape == (0, 0) and m.cache_bytes() == 0
    from omnitokenizer_amd import _lib
    assert _lib.load().omnitok_lm_max_streams(m._engine) == 24
    with pytest.raises(RuntimeError, match="replaced"):
        m.forward_with_past(x[:16, :1], past=[h], past_length=4)
    with pytest.raises(RuntimeError, match="cache not allocated"):
        m.step(x[:16, 0].contiguous())
    with pytest.raises(ValueError, match="at most 24 streams"):
        m.reset_streams(25, 8)
    m.reset_streams(24, ml)
    assert m._cache_shape == (24, ml) and m.cache_bytes() * 16 == bytes16 * 24
    # 24 streams through the reference's interface, against the float64 oracle
    logits, _, h24 = m.forward_with_past(x, past=None)
    nxt = torch.randint(0, V, (24, 1), generator=torch.Generator().manual_seed(62)).cuda()
    l2, _, _ = m.forward_with_past(nxt, past=[h24], past_length=4)
    sd64 = {k: v.double() for k, v in sd.items()}
    with torch.no_grad():
        ref = go.forward(sd64, torch.cat([x.cpu(), nxt.cpu()], 1), H)
    e = max(dmax(logits[:, -1], ref[:, 3]), dmax(l2[:, 0], ref[:, 4]))
    assert e < LOGIT_TOL, e
    # token_losses (the prefill with the loss head) of 24 streams equals the cross-entropy of forward()'s logits
    from omnitokenizer_amd import lm_losses as ll
    tg = torch.randint(0, V, (24, 4), generator=torch.Generator().manual_seed(63)).cuda()
    full, _ = m(x)
    want, out = ll.token_cross_entropy(full, tg), m.token_losses(x, tg)
    for k in want:
        assert torch.equal(out[k], want[k]), k
    # back to the default: 17 streams are refused again
    m.set_max_streams(16)
    with pytest.raises(ValueError, match="at most 16 streams"):
        m.reset_streams(17, 8)
