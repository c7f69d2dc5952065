"""GPU (-m gpu): fp8 (e4m3fn) K/V cache with one power-of-two scale per cached row (omnitok_lm_set_cache_quant, GPT.set_cache_quant).

What an fp8 cache computes (include/omnitok_lm.h): a token's K/V rows are quantised once, where they are stored, by the rule of
omnitokenizer_amd.gpt.fp8_quantize_rows applied to one head's row; the step that produces a token uses its fp32 row; a cached
element enters as widen(q) * s in front of the unchanged fp32 chain.  So
  * the attention kernel on (bytes, scales) equals the fp32 kernel on the dequantised values s * q BIT FOR BIT, and what it appends
    are fp8_quantize_rows' bytes and scales (test_attn_decode_kv8_*);
  * the cache holds fixed points (as values) of the quantisation, and layer 0 -- whose K/V depend on tokens and positions only --
    holds the fp32 engine's rows quantised by torch (test_scatter_*, test_cache_contents_are_fixed_points);
  * logits are compared with the CPU oracle FED THE ENGINE'S OWN CACHE (tests/test_gpu_lm_kv16.py), where only the fp32 summation
    order is left, at the fp32 path's own LOGIT_TOL."""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import gpt_oracle as go
from omnitokenizer_amd.gpt import fp8_quantize_rows
from tests import lm_prefill16_ref as pr
from tests.test_gpu_lm import LOGIT_TOL, rnd
from tests.test_gpu_lm_kv16 import engine_rows, oracle_on_cache, run
from tests.test_gpu_lm_prefill16 import BAR_FACTOR
from tests.test_gpu_lm_w16 import make_gpt, rounded
from tests.test_oracle_gpt import GPT_CASES, load_gpt_case

pytestmark = pytest.mark.gpu
KV8_NONFINITE = 32      # the new bit of omnitok_lm_overflowed


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def lib():
    from omnitokenizer_amd import _lib
    return _lib.load()


def quant(x):
    """(q float8_e4m3fn [..., hd], s float32 [...]) of fp32 rows x [..., hd] on the CPU: fp8_quantize_rows per row of hd elements"""
    x = x.detach().cpu().float()
    q, s = fp8_quantize_rows(x.reshape(-1, x.shape[-1]))
    return q.view(x.shape), s.view(x.shape[:-1])


def dequant(q, s):
    return q.float() * s[..., None]         # exact in fp32 (a power of two times 4 significant bits), subnormals kept


def dq(x):
    return dequant(*quant(x))


def dmax(a, b):
    return float(torch.nan_to_num((a.cpu().double() - b.cpu().double()).abs(), nan=math.inf).max())


def u8(q):
    return q.view(torch.uint8)


# ---- kernel level ----------------------------------------------------------------------------------------------------------
B, H = 3, 4
QSCALE = 2.0 ** -18     # of q: the keys of the top octaves (|k| ~ 2^20) then score a few units, so many keys carry weight


def spread(*shape, seed):
    """N(0, 1) rows whose magnitudes are spread over +-20 octaves: ldexp by a seeded random exponent per row"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g)
    e = torch.randint(-20, 21, (*shape[:-1], 1), generator=g, dtype=torch.int32)
    return torch.ldexp(x, e)


@functools.lru_cache(maxsize=2)
def quantized_caches(max_len, hd):
    """(qk, sk, qv, sv) on the CPU: B x H x max_len spread rows, quantised by fp8_quantize_rows.  Shared: never modified."""
    qk, sk = quant(spread(B, H, max_len, hd, seed=7))
    qv, sv = quant(spread(B, H, max_len, hd, seed=8))
    assert len(torch.unique(sk)) > 30 and len(torch.unique(sv)) > 30       # (a wrong scale index cannot go unseen)
    return qk, sk, qv, sv


def make_qkv(hd, seed):
    C = H * hd
    qkv = torch.cat([rnd(B, C, seed=seed) * QSCALE, spread(B, H, hd, seed=seed + 1).reshape(B, C),
                     spread(B, H, hd, seed=seed + 2).reshape(B, C)], 1)
    return qkv.contiguous()


class Caches:
    """device caches of one (max_len, hd): bytes + scales for the kv8 entry, and what they must hold after every call"""

    def __init__(self, qk, sk, qv, sv):
        self.k8, self.v8 = u8(qk).clone().cuda(), u8(qv).clone().cuda()
        self.ks, self.vs = sk.clone().cuda(), sv.clone().cuda()
        self.ref = [u8(qk).clone(), sk.clone(), u8(qv).clone(), sv.clone()]      # CPU: expected bytes and scales

    def twin(self):
        """fp32 caches holding s * q (exact) of the expected state"""
        k8, ks, v8, vs = self.ref
        return dequant(k8.view(torch.float8_e4m3fn), ks), dequant(v8.view(torch.float8_e4m3fn), vs)

    def call(self, lib, hd, max_len, qkv, lens):
        """One call of omnitok_lm_attn_decode_kv8 in place and one of omnitok_lm_attn_decode on the fp32 twin; checks the appended
        rows and that nothing else changed.  Returns (out8, out32)."""
        s = torch.cuda.current_stream().cuda_stream
        C = H * hd
        nchunk = (max_len + 255) // 256
        kt, vt = (t.cuda() for t in self.twin())
        kw, vw = kt.cpu().clone(), vt.cpu().clone()
        d = qkv.cuda()
        cl = torch.tensor(lens, dtype=torch.int32, device="cuda")
        scratch = torch.empty(B * H * nchunk * (2 + hd), device="cuda")
        out8, out32 = torch.empty(B, C, device="cuda"), torch.empty(B, C, device="cuda")
        assert lib.omnitok_lm_attn_decode_kv8(_p(d), _p(self.k8), _p(self.v8), _p(self.ks), _p(self.vs), _p(cl), B, H, hd, max_len,
                                              _p(scratch), _p(out8), s) == 0
        assert lib.omnitok_lm_attn_decode(_p(d), _p(kt), _p(vt), _p(cl), B, H, hd, max_len, _p(scratch), _p(out32), s) == 0
        _, kn, vn = (t.reshape(B, H, hd) for t in qkv.split(C, dim=1))
        k8, ks, v8, vs = self.ref
        for b, ln in enumerate(lens):
            ln = min(ln, max_len - 1)           # (a stream past the cache is clamped to its last row)
            (qn, sn), (qm, sm) = quant(kn[b]), quant(vn[b])
            k8[b, :, ln], ks[b, :, ln], v8[b, :, ln], vs[b, :, ln] = u8(qn), sn, u8(qm), sm
            kw[b, :, ln], vw[b, :, ln] = kn[b], vn[b]
        # the appended rows hold fp8_quantize_rows' bytes and scales, no other byte or scale changed; the twin holds the unrounded row
        assert torch.equal(self.k8.cpu(), k8) and torch.equal(self.v8.cpu(), v8)
        assert torch.equal(self.ks.cpu(), ks) and torch.equal(self.vs.cpu(), vs)
        assert torch.equal(kt.cpu(), kw) and torch.equal(vt.cpu(), vw)
        return out8, out32


@pytest.mark.parametrize("hd", [64, 96, 128])
def test_attn_decode_kv8_equals_fp32_kernel_on_dequantized_cache(lib, hd):
    """Bit for bit, with "lm_attn_waves" 8 and 4, at lengths around the chunk boundaries and (head_dim 128) at the last slot of an
    8192-token cache, on caches whose row scales are spread over 40 octaves."""
    from omnitokenizer_amd import _lib
    saved = _lib.get_option("lm_attn_waves")
    shapes = [(700, ([0, 1, 5], [255, 256, 257], [511, 640, 699]))] + ([(8192, ([1, 4100, 8191],))] if hd == 128 else [])
    try:
        for waves in (8, 4):
            _lib.set_option("lm_attn_waves", waves)
            for max_len, cases in shapes:
                c = Caches(*quantized_caches(max_len, hd))
                for lens in cases:
                    qkv = make_qkv(hd, seed=9 + lens[0])
                    out8, out32 = c.call(lib, hd, max_len, qkv, lens)
                    assert torch.equal(out8, out32), (hd, waves, max_len, lens, dmax(out8, out32))
                    assert torch.isfinite(out8).all() and float(out8.abs().max()) > 0
                kt, _ = c.twin()
                assert not torch.equal(kt[0, :, cases[-1][0]], qkv[0, H * hd:2 * H * hd].view(H, hd))   # (the quantisation is live)
    finally:
        _lib.set_option("lm_attn_waves", saved)


def edge_rows(hd, k=3):
    """fp32 rows [n, hd] at the edges of the scale rule"""
    g = torch.Generator().manual_seed(5)
    small = torch.rand(hd, generator=g) * 2 - 1                       # |x| < 1
    zero = torch.zeros(hd)
    at = small.clone() * 2.0 ** k
    at[3] = -448.0 * 2.0 ** k                                          # amax exactly 448 * 2^k: m == 0.875, e = k
    above = at.clone()
    above[3] = torch.nextafter(at[3].abs(), torch.tensor(math.inf))    # ... and its fp32 successor: e = k + 1
    tiny = small.clone() * 1e-40                                       # fp32 subnormals: e clamps at -126
    tiny[0] = 1e-40
    sub = (torch.rand(hd, generator=g) * 0.9 + 0.1) * 2.0 ** -15       # after scaling by 2^8: below 2^-6, e4m3's subnormal range
    sub[::2] *= -1
    sub[7] = 1.0                                                       # ... all but this one (e = -8, code 256)
    rows = torch.stack([zero, at, above, tiny, sub])
    q, s = quant(rows)
    assert s[0] == 1 and s[1] == 2.0 ** k and s[2] == 2.0 ** (k + 1) and s[3] == 2.0 ** -126 and s[4] == 2.0 ** -8
    assert float(dequant(q, s)[3].abs().max()) < 2.0 ** -126 and float(dequant(q, s)[3].abs().max()) > 0       # fp32 subnormals
    w = q[4].float().abs()
    assert int((w >= 2.0 ** -6).sum()) == 1 and int(((w > 0) & (w < 2.0 ** -6)).sum()) > hd // 2                   # e4m3 subnormals
    return rows


def test_attn_decode_kv8_edge_rows(lib):
    """An all-zero row, amax exactly 448 * 2^k and its successor, a row of fp32 subnormals (the clamp at e = -126) and a row in
    e4m3's subnormal range -- in the cache and as appended rows: outputs bit-equal to the twin, appended bits fp8_quantize_rows'."""
    hd, max_len = 64, 700
    rows = edge_rows(hd)
    n = rows.shape[0]
    k = spread(B, H, max_len, hd, seed=17)
    v = spread(B, H, max_len, hd, seed=18)
    for b in range(B):
        for h in range(H):
            for i in range(n):
                k[b, h, 10 + i + h] = rows[i]
                v[b, h, 12 + (i + 1) % n + h] = rows[i]
                k[b, h, 250 + 3 * i + b] = rows[i]          # around the chunk boundary too
    qk, sk = quant(k)
    qv, sv = quant(v)
    c = Caches(qk, sk, qv, sv)
    for i in range(n):
        qkv = make_qkv(hd, seed=40 + i)
        kn, vn = qkv[:, H * hd:2 * H * hd].view(B, H, hd), qkv[:, 2 * H * hd:].view(B, H, hd)
        for b in range(B):
            for h in range(H):
                if (b + h) % 2 == 0:            # (the other heads keep their random rows)
                    kn[b, h], vn[b, h] = rows[i], rows[(i + 2) % n]
        lens = [20 + i, 300 + i, 690 + i]
        out8, out32 = c.call(lib, hd, max_len, qkv, lens)
        assert torch.equal(out8, out32), (i, dmax(out8, out32))
        assert torch.isfinite(out8).all() and float(out8.abs().max()) > 0


def test_attn_decode_kv8_past_the_cache_stays_inside_the_slab(lib):
    """cache_len >= max_len: the stream is clamped to its own last row -- the neighbouring heads' and streams' bytes and scales
    are what they were (Caches.call compares every byte and scale)."""
    hd, max_len = 64, 300
    c = Caches(*quant(spread(B, H, max_len, hd, seed=27)), *quant(spread(B, H, max_len, hd, seed=28)))
    out8, out32 = c.call(lib, hd, max_len, make_qkv(hd, seed=29), [max_len, 5, max_len + 7])
    assert torch.equal(out8, out32) and torch.isfinite(out8).all()


def test_attn_decode_kv8_nan_row_touches_no_other_row(lib):
    """A NaN planted in one K element of qkv: the exported entry has no flag word (the engine raises the bit:
    test_non_finite_rows_are_flagged); here every OTHER row keeps its bytes and scales, V's appended rows are what they are without
    the NaN, and every other head's and stream's output keeps its bits."""
    hd, max_len, lens = 64, 300, [7, 100, 256]

    def fresh():
        return Caches(*quant(spread(B, H, max_len, hd, seed=27)), *quant(spread(B, H, max_len, hd, seed=28)))
    qkv = make_qkv(hd, seed=33)
    ok = fresh()
    clean, _ = ok.call(lib, hd, max_len, qkv, lens)
    qkv[1, H * hd + 2 * hd + 5] = float("nan")       # stream 1, head 2, K element 5
    c = fresh()
    s = torch.cuda.current_stream().cuda_stream
    d, cl = qkv.cuda(), torch.tensor(lens, dtype=torch.int32, device="cuda")
    scratch, out = torch.empty(B * H * 2 * (2 + hd), device="cuda"), torch.empty(B, H * hd, device="cuda")
    assert lib.omnitok_lm_attn_decode_kv8(_p(d), _p(c.k8), _p(c.v8), _p(c.ks), _p(c.vs), _p(cl), B, H, hd, max_len, _p(scratch),
                                          _p(out), s) == 0
    keep = torch.ones(B, H, max_len, dtype=torch.bool)
    keep[1, 2, 100] = False                          # the one row whose contents are unspecified
    assert torch.equal(c.k8.cpu()[keep], ok.k8.cpu()[keep]) and torch.equal(c.ks.cpu()[keep], ok.ks.cpu()[keep])
    assert torch.equal(c.v8.cpu(), ok.v8.cpu()) and torch.equal(c.vs.cpu(), ok.vs.cpu())
    out, clean = out.cpu().view(B, H, hd), clean.cpu().view(B, H, hd)
    assert torch.equal(out[[0, 2]], clean[[0, 2]]) and torch.equal(out[1, [0, 1, 3]], clean[1, [0, 1, 3]])


# ---- engine level ----------------------------------------------------------------------------------------------------------
def make_gpt8(sd, dims, fmt="fp32"):
    return make_gpt(sd, dims, fmt).set_cache_quant("fp8")


@pytest.mark.parametrize("hd,n_head", [(64, 4), (96, 8), (128, 2)])
def test_scatter_quantizes_layer0_rows_by_the_rule(hd, n_head):
    """A prefill of T = 5 tokens: every layer-0 row of the fp8 cache equals dequant(fp8_quantize_rows(the fp32 engine's row)).
    head_dim 96 is the case whose heads straddle a wave under the fp32 / 16-bit scatter's mapping.  (n_embd must be a multiple of
    256 for the engine, so the head counts are the smallest that give one: 4, 8 and 2.)"""
    V, BS, L, C, T = 300, 48, 1, hd * n_head, 5
    sd = go.synth_gpt_state(V, BS, L, n_head, C, seed=61)
    idx = torch.randint(0, V, (2, T), generator=torch.Generator().manual_seed(62)).cuda()
    got = {}
    for name, m in (("fp8", make_gpt8(sd, (V, BS, L, n_head, C))), ("fp32", make_gpt(sd, (V, BS, L, n_head, C)))):
        m.reset_streams(2, T + 2)
        m.prefill(idx)
        m.check_overflow()
        got[name] = engine_rows(m, 2, T)[0]
    for kv in (0, 1):
        r8, r32 = got["fp8"][kv], got["fp32"][kv]
        assert r8.shape == (2, n_head, T, hd) and float((r8 != 0).float().mean()) > 0.9
        assert torch.equal(r8, dq(r32)), ("kv"[kv], dmax(r8, dq(r32)))
        assert not torch.equal(r8, r32)


@pytest.fixture(scope="module")
def cases():
    """per golden model, computed once: 3 x T tokens stepped and prefilled through an fp8-cache engine and an fp32-cache engine,
    their caches read back, the oracle on each fp8 cache, and the fp8 engine switched back."""
    cache = {}

    def get(name):
        if name not in cache:
            g, sd, dims = load_gpt_case(name)
            V, BS, L, H_, C = dims
            T = min(BS - 2, 40)
            idx = torch.randint(0, V, (3, T), generator=torch.Generator().manual_seed(11))
            r32 = run(make_gpt(sd, dims), idx.cuda(), T)
            m8 = make_gpt8(sd, dims)
            assert m8.cache_quant == "fp8" and m8.cache_format == "fp32" and m8.weight_format == "fp32"
            r8 = run(m8, idx.cuda(), T)
            shape = m8._cache_shape
            ref_s, ref_p = oracle_on_cache(sd, idx, H_, r8["rows_s"]), oracle_on_cache(sd, idx, H_, r8["rows_p"])
            assert m8.set_cache_quant("none") is m8
            assert m8._graphs == {} and m8._cache_shape == (0, 0) and m8.cache_bytes() == 0
            with pytest.raises(RuntimeError, match="cache not allocated"):     # ... until reset_streams allocates again
                m8.step(idx[:, 0].cuda().contiguous())
            back = run(m8, idx.cuda(), T)
            cache[name] = dict(r8=r8, r32=r32, ref_s=ref_s, ref_p=ref_p, back=back, dims=dims, shape=shape)
        return cache[name]
    return get


@pytest.mark.parametrize("name", GPT_CASES)
def test_cache_contents_are_fixed_points(cases, name):
    """After stepping (the kernel's append) and after a prefill (the scatter): every layer's rows are fixed points, as values, of
    the quantisation; layer 0's equal the fp32 engine's rows quantised by torch, bit for bit."""
    c = cases(name)
    for which in ("rows_s", "rows_p"):
        r8, r32 = c["r8"][which], c["r32"][which]
        assert len(r8) == c["dims"][2]
        for i, (k, v) in enumerate(r8):
            assert torch.equal(dq(k), k) and torch.equal(dq(v), v), (which, i)
            assert float((k != 0).float().mean()) > 0.9 and float((v != 0).float().mean()) > 0.9      # (rows were written)
            assert not torch.equal(dq(r32[i][0]), r32[i][0])       # (the fp32 engine's rows are NOT such fixed points)
        for kv in (0, 1):
            assert torch.equal(r8[0][kv], dq(r32[0][kv])), (which, "kv"[kv])


@pytest.mark.parametrize("name", GPT_CASES)
def test_logits_vs_oracle_on_the_engines_cache(cases, name):
    """Stepped logits and the teacher-forced logits of prefill(want_logits=True), each against the oracle fed that run's cache, at
    the fp32 path's LOGIT_TOL."""
    c = cases(name)
    es, ep = dmax(c["r8"]["stepped"], c["ref_s"]), dmax(c["r8"]["batched"], c["ref_p"])
    print(f"{name} fp8 cache: stepped {es:.2e}, prefill {ep:.2e} (tol {LOGIT_TOL:.0e})")
    assert es < LOGIT_TOL and ep < LOGIT_TOL


def test_long_prefix_multi_chunk():
    """A 600-token prefix (several attention chunks, the prefill's scatter) and 6 sampled tokens; the 6 stepped positions against
    the oracle on the engine's cache."""
    from omnitokenizer_amd import gpt as og
    V, BS, L, H_, C = 256, 700, 1, 4, 256
    sd = go.synth_gpt_state(V, BS, L, H_, C, seed=21)
    m = make_gpt8(sd, (V, BS, L, H_, C))
    x = torch.randint(0, V, (2, 600), generator=torch.Generator().manual_seed(22))
    new, lg = og.sample_with_past(x.cuda(), m, 6, sample_logits=False, return_logits=True)
    m.check_overflow()
    seq = torch.cat([x, new.cpu()], 1)[:, :605]          # the tokens that entered: positions 0 .. 604
    rows = engine_rows(m, 2, 605)
    err = dmax(lg, oracle_on_cache(sd, seq, H_, rows, t0=599))
    print(f"long prefix fp8 cache: {err:.2e}")
    assert err < LOGIT_TOL
    k = rows[0][0]
    assert torch.equal(dq(k), k) and float((k != 0).float().mean()) > 0.9


def step_all(m, idx, n):
    m.reset_streams(n, idx.shape[1] + 2)
    d = idx.cuda()
    out = torch.stack([m.step(d[:, t].contiguous()) for t in range(idx.shape[1])], 1).cpu()
    m.check_overflow()
    return out, engine_rows(m, n, idx.shape[1])


def test_seventeen_streams_take_the_many_stream_path():
    """17 streams with their own tokens under set_max_streams(32): the many-stream step over an fp8 cache, against the oracle on
    the engine's cache."""
    g, sd, dims = load_gpt_case(GPT_CASES[0])
    V, BS, L, H_, C = dims
    T = min(BS - 2, 12)
    idx = torch.randint(0, V, (17, T), generator=torch.Generator().manual_seed(71))
    m = make_gpt8(sd, dims).set_max_streams(32)
    assert m.cache_quant == "fp8" and m.max_streams == 32
    got, rows = step_all(m, idx, 17)
    ref = oracle_on_cache(sd, idx, H_, rows)
    assert float((ref[0] - ref[16]).abs().max()) > 100 * LOGIT_TOL      # the streams differ
    err = dmax(got, ref)
    print(f"17 streams fp8 cache: {err:.2e}")
    assert err < LOGIT_TOL
    assert all(torch.equal(dq(k), k) and torch.equal(dq(v), v) for k, v in rows)


@pytest.mark.parametrize("name", GPT_CASES)
def test_switch_is_live_and_switches_back(cases, name):
    """The quantised cache moves the stepped logits by more than the tolerance; set_cache_quant("none") gives back the default
    engine's bits; the cache takes elements x 1 + rows x 4 bytes: a quarter of the fp32 cache plus the scales."""
    c = cases(name)
    V, BS, L, H_, C = c["dims"]
    live = dmax(c["r8"]["stepped"], c["r32"]["stepped"])
    print(f"{name} fp8 cache: stepped logits move by {live:.2e}")
    assert live > LOGIT_TOL
    for k in ("stepped", "batched"):
        assert torch.equal(c["back"][k], c["r32"][k]), k
    assert c["back"]["bytes"] == c["r32"]["bytes"]
    mb, ml = c["shape"]
    elements, nrows = L * 2 * mb * ml * C, L * 2 * mb * H_ * ml
    assert c["r8"]["bytes"] == elements + 4 * nrows
    assert c["r32"]["bytes"] == 4 * elements and c["r8"]["bytes"] == c["r32"]["bytes"] // 4 + 4 * nrows


def test_bf16_weights_and_fp8_cache():
    """bf16 weights + an fp8 cache (the bf16 cache format set as well: it decides nothing while the quant is on): the oracle on
    rounded(sd) fed the engine's cache, at the bar of the 16-bit weights + cache test."""
    g, sd, dims = load_gpt_case(GPT_CASES[0])
    V, BS, L, H_, C = dims
    T = min(BS - 2, 40)
    idx = torch.randint(0, V, (3, T), generator=torch.Generator().manual_seed(11))
    m = make_gpt8(sd, dims, "bf16").set_cache_format("bf16")
    assert (m.weight_format, m.cache_format, m.cache_quant) == ("bf16", "bf16", "fp8")
    r = run(m, idx.cuda(), T)
    rsd = rounded(sd, "bf16")
    es = dmax(r["stepped"], oracle_on_cache(rsd, idx, H_, r["rows_s"]))
    ep = dmax(r["batched"], oracle_on_cache(rsd, idx, H_, r["rows_p"]))
    print(f"weights bf16 + fp8 cache: stepped {es:.2e}, prefill {ep:.2e}")
    assert es < LOGIT_TOL and ep < LOGIT_TOL
    mb, ml = m._cache_shape
    assert r["bytes"] == L * 2 * mb * ml * (C + 4 * H_)
    assert all(torch.equal(dq(k), k) for k, _ in r["rows_s"])


def test_decode_quant_and_fp8_cache():
    """set_decode_quant("fp8") + an fp8 cache: the steps read the fp8 weight image and append quantised rows; against the oracle on
    fp8_dequantized(sd) fed the engine's cache, at the fp8 weights' own bar (LOGIT_TOL)."""
    from omnitokenizer_amd import fp8_dequantized
    g, sd, dims = load_gpt_case(GPT_CASES[0])
    V, BS, L, H_, C = dims
    T = min(BS - 2, 24)
    idx = torch.randint(0, V, (3, T), generator=torch.Generator().manual_seed(11))
    m = make_gpt8(sd, dims).set_decode_quant("fp8")
    assert (m.decode_quant, m.cache_quant) == ("fp8", "fp8")
    got, rows = step_all(m, idx, 3)
    err = dmax(got, oracle_on_cache(fp8_dequantized(sd), idx, H_, rows))
    print(f"fp8 weights + fp8 cache: stepped {err:.2e}")
    assert err < LOGIT_TOL
    assert all(torch.equal(dq(k), k) and torch.equal(dq(v), v) for k, v in rows)


def w16_steps_on_cache(sd, idx, n_head, fmt, rows, dt):
    """tests/lm_prefill16_ref.py's restatement of the 16-bit rounding points, one position at a time, attending to rows[i][:, :, :t]
    -- the ENGINE'S cache -- in place of its own past (the token's own K/V stay its own).  Logits [B, T, V] in dt."""
    f16 = pr.FMT[fmt][1]
    sd = {k: v.to(dt) for k, v in pr.rounded(sd, fmt).items()}

    def r16(t):
        return t.to(f16).to(dt)

    Bn, T = idx.shape
    C = sd["tok_emb.weight"].shape[1]
    hs = C // n_head
    outs = []
    for t in range(T):
        x = F.embedding(idx[:, t], sd["tok_emb.weight"]) + sd["pos_emb"][0, t]
        for i in range(len(rows)):
            p = f"blocks.{i}"
            h = r16(F.layer_norm(x, (C,), sd[f"{p}.ln1.weight"], sd[f"{p}.ln1.bias"]))
            k, q, v = (F.linear(h, sd[f"{p}.attn.{n}.weight"], sd[f"{p}.attn.{n}.bias"]).view(Bn, n_head, 1, hs)
                       for n in ("key", "query", "value"))
            K = torch.cat([rows[i][0][:, :, :t].to(dt), k], 2)
            Vv = torch.cat([rows[i][1][:, :, :t].to(dt), v], 2)
            att = F.softmax((q @ K.transpose(-2, -1)) * (1.0 / math.sqrt(hs)), dim=-1)
            y = (att @ Vv).reshape(Bn, C)
            x = x + F.linear(r16(y), sd[f"{p}.attn.proj.weight"], sd[f"{p}.attn.proj.bias"])
            h = r16(F.layer_norm(x, (C,), sd[f"{p}.ln2.weight"], sd[f"{p}.ln2.bias"]))
            h = r16(F.gelu(F.linear(h, sd[f"{p}.mlp.0.weight"], sd[f"{p}.mlp.0.bias"])))
            x = x + F.linear(h, sd[f"{p}.mlp.2.weight"], sd[f"{p}.mlp.2.bias"])
        outs.append(F.linear(r16(F.layer_norm(x, (C,), sd["ln_f.weight"], sd["ln_f.bias"])), sd["head.weight"]))
    return torch.stack(outs, 1)


def test_streams_w16_and_fp8_cache_at_17_streams():
    """set_streams_format("w16") on bf16 weights + an fp8 cache, 17 streams: against the fp64 restatement of the SF_W16 rounding
    points fed the engine's cache, at that path's own bar -- BAR_FACTOR x d_ref, d_ref the restatement's fp32-vs-fp64 distance
    (tests/test_gpu_lm_streams16.py)."""
    g, sd, dims = load_gpt_case(GPT_CASES[0])
    V, BS, L, H_, C = dims
    T = min(BS - 2, 10)
    idx = torch.randint(0, V, (17, T), generator=torch.Generator().manual_seed(81))
    m = make_gpt8(sd, dims, "bf16").set_max_streams(32).set_streams_format("w16")
    assert (m.streams_format, m.cache_quant, m.weight_format) == ("w16", "fp8", "bf16")
    got, rows = step_all(m, idx, 17)
    l64 = w16_steps_on_cache(sd, idx, H_, "bf16", rows, torch.float64)
    d_ref = dmax(w16_steps_on_cache(sd, idx, H_, "bf16", rows, torch.float32), l64)
    err = dmax(got, l64)
    print(f"SF_W16 bf16 + fp8 cache x 17 streams: d_ref {d_ref:.3e}, stepped {err:.3e} = {err / d_ref:.2f} d_ref")
    assert torch.isfinite(got).all() and err <= BAR_FACTOR * d_ref
    assert all(torch.equal(dq(k), k) and torch.equal(dq(v), v) for k, v in rows)


def test_graph_replay_and_stale_handles():
    from omnitokenizer_amd import gpt as og
    g, sd, dims = load_gpt_case(GPT_CASES[0])
    m = make_gpt8(sd, dims)
    x = torch.from_numpy(g["idx"])[:, :4].cuda()
    tok_g, lg_g = og.sample_with_past(x, m, 10, sample_logits=False, use_graph=True, return_logits=True)
    assert m._graphs
    tok_e, lg_e = og.sample_with_past(x, m, 10, sample_logits=False, use_graph=False, return_logits=True)
    assert torch.equal(tok_g, tok_e) and torch.equal(lg_g, lg_e)
    m.check_overflow()
    # a handle from before the switch is rejected, and no graph captured on the old cache is left to replay
    _, _, h = m.forward_with_past(x, past=None)
    m.graph_step(x.shape[0])
    assert m._graphs
    assert m.set_cache_quant("none") is m
    assert m._graphs == {} and m._cache_shape == (0, 0) and m.cache_bytes() == 0
    with pytest.raises(RuntimeError, match="replaced"):
        m.forward_with_past(x[:, :1], past=[h], past_length=4)
    with pytest.raises(RuntimeError, match="cache not allocated"):
        m.step(x[:, 0].contiguous())
    tok_h = og.sample_with_past(x, m.set_cache_quant("fp8"), 10, sample_logits=False, use_graph=True)
    assert torch.equal(tok_h, tok_g) and m.cache_quant == "fp8"


def test_stepping_past_an_fp8_cache_is_flagged(lib):
    """One more step than the cache holds raises the past-cache bit (and no other) and stays inside the stream's own slabs: the
    other stream's rows -- bytes and scales, read back as s * q -- are what they were."""
    g, sd, dims = load_gpt_case("gpt_hd64")
    m = make_gpt8(sd, dims)
    m.reset_streams(2, 4)
    cap = m._cache_shape[1]
    s = torch.cuda.current_stream().cuda_stream
    tok = torch.tensor([1, 2], device="cuda")
    for _ in range(cap - 1):
        m._pos.zero_()                      # keep the position embedding in range; only the cache length grows
        m.step(tok)
    m.check_overflow()
    m._len[1] = 2                           # stream 1 stays inside; stream 0 fills its last row, then steps past it
    m._pos.zero_()
    m.step(tok)
    m.check_overflow()                      # `cap` tokens fit
    before = [[t.clone() for t in m.cache_rows(i, 1, 0, cap)] for i in range(m.n_layer)]
    own = [[t.clone() for t in m.cache_rows(i, 0, 0, cap - 1)] for i in range(m.n_layer)]
    m._len[1] = 2
    m._pos.zero_()
    m.step(tok)                             # one more does not
    assert lib.omnitok_lm_overflowed(m._engine, s) == 1
    for i in range(m.n_layer):
        for kv in (0, 1):
            now = m.cache_rows(i, 1, 0, cap)[kv]
            keep = torch.ones(cap, dtype=torch.bool)
            keep[2] = False                 # (stream 1's own append)
            # (bit patterns: rows nobody wrote yet hold whatever the allocation held, a NaN now and then)
            assert torch.equal(now[:, keep].view(torch.int32), before[i][kv][:, keep].view(torch.int32)), (i, kv)
            assert torch.equal(m.cache_rows(i, 0, 0, cap - 1)[kv], own[i][kv]), (i, kv)
    m._len.fill_(cap)
    m._pos.zero_()
    m.step(tok)
    with pytest.raises(RuntimeError, match="K/V cache"):
        m.check_overflow()
    m.check_overflow()                      # the flag was cleared


SMALL = (300, 48, 1, 4, 256)


@pytest.mark.parametrize("value", [float("nan"), float("inf")])
def test_non_finite_rows_are_flagged(lib, value):
    """One element of key.bias is NaN (or inf): that head's K row is not finite.  The fp8 cache raises bit 32 of the flag word and
    no other -- from the step's append and from the prefill's scatter; without the quant no cache ever does."""
    V, BS, L, H_, C = SMALL
    sd = go.synth_gpt_state(V, BS, L, H_, C, seed=25)
    sd["blocks.0.attn.key.bias"] = sd["blocks.0.attn.key.bias"].clone()
    sd["blocks.0.attn.key.bias"][70] = value             # head 1, element 6
    tok = torch.tensor([1, 2], device="cuda")
    idx = torch.randint(0, V, (2, 8), generator=torch.Generator().manual_seed(26)).cuda()
    s = torch.cuda.current_stream().cuda_stream
    m = make_gpt8(sd, SMALL)
    m.reset_streams(2, 16)
    m.check_overflow()
    m.step(tok)
    assert lib.omnitok_lm_overflowed(m._engine, s) == KV8_NONFINITE
    assert lib.omnitok_lm_overflowed(m._engine, s) == 0          # cleared
    m.step(tok)
    with pytest.raises(RuntimeError, match=r"fp8 cache.*NaN or an infinity"):
        m.check_overflow()
    m.check_overflow()
    m.reset_streams(2, 16)
    m.prefill(idx)
    assert lib.omnitok_lm_overflowed(m._engine, s) == KV8_NONFINITE
    m.set_cache_quant("none")
    for fmt in ("bf16", "fp32"):
        m.set_cache_format(fmt)
        m.reset_streams(2, 16)
        m.step(tok)
        m.reset_streams(2, 16)
        m.prefill(idx)
        assert lib.omnitok_lm_overflowed(m._engine, s) == 0
