"""GPU (-m gpu): bf16 / fp16 K/V cache of the LM decode (omnitok_lm_set_cache_format, GPT.set_cache_format).

What a 16-bit cache computes (include/omnitok_lm.h): a token's K/V rows are rounded once, where they are stored; the step that produces
a token uses its fp32 row; everything else is the fp32 arithmetic.  So
  * the attention kernel on a packed cache equals the fp32 kernel on the widened values BIT FOR BIT (test_attn_decode_kv16_*);
  * the cache holds fixed points of the rounding, and layer 0 -- whose K/V depend on tokens and positions only -- holds the fp32
    engine's rows rounded by torch (test_cache_contents);
  * logits are compared with the CPU oracle FED THE ENGINE'S OWN CACHE (GPT.cache_rows): an oracle that rounds its own K/V lands on
    the other side of a rounding boundary now and then (its own fp32 and fp64 runs differ by up to 8.3e-4 with bf16), while on the
    engine's cache only the fp32 summation order is left, and the bar is the fp32 path's own LOGIT_TOL."""
import argparse
import ctypes
import functools

import pytest
import torch

from oracle import gpt_oracle as go
from tests.test_gpu_lm import LOGIT_TOL, rnd
from tests.test_gpu_lm_w16 import make_gpt, rounded
from tests.test_oracle_gpt import GPT_CASES, load_gpt_case

pytestmark = pytest.mark.gpu
FMT = {"bf16": (1, torch.bfloat16), "fp16": (2, torch.float16)}


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def lib():
    from omnitokenizer_amd import _lib
    return _lib.load()


def bits(t):
    return t.view(torch.int16)


# ---- kernel level ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def packed_caches(max_len, hd, fmt, scale=1.0):
    """test_attn_decode's caches (B 3, H 4), rounded by torch, on the device"""
    dt = FMT[fmt][1]
    return (rnd(3, 4, max_len, hd, seed=7, scale=scale).to(dt).cuda(), rnd(3, 4, max_len, hd, seed=8, scale=scale).to(dt).cuda())


def attn_both(lib, fmt, hd, max_len, kc16, vc16, qkv, lens):
    """One call of omnitok_lm_attn_decode_kv16 on (kc16, vc16), in place, and one of omnitok_lm_attn_decode on their fp32 twins.
    Returns (out16, out32, twin k, twin v)."""
    B, H = 3, 4
    s = torch.cuda.current_stream().cuda_stream
    nchunk = (max_len + 255) // 256
    kt, vt = kc16.float(), vc16.float()      # the widened values: exact
    cl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    scratch = torch.empty(B * H * nchunk * (2 + hd), device="cuda")
    out16, out32 = torch.empty(B, H * hd, device="cuda"), torch.empty(B, H * hd, device="cuda")
    assert lib.omnitok_lm_attn_decode_kv16(_p(qkv), _p(kc16), _p(vc16), FMT[fmt][0], _p(cl), B, H, hd, max_len, _p(scratch), _p(out16),
                                           s) == 0
    assert lib.omnitok_lm_attn_decode(_p(qkv), _p(kt), _p(vt), _p(cl), B, H, hd, max_len, _p(scratch), _p(out32), s) == 0
    return out16, out32, kt, vt


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("hd", [64, 96, 128])
def test_attn_decode_kv16_equals_fp32_kernel_on_widened_cache(lib, hd, fmt):
    """Bit for bit, with "lm_attn_waves" 8 and 4, at test_attn_decode's lengths around the chunk boundaries and at the last slot of
    an 8192-token cache; the new token's rows are appended with torch's rounding, nothing else changes, the twin keeps fp32 rows."""
    from omnitokenizer_amd import _lib
    B, H, dt = 3, 4, FMT[fmt][1]
    C = H * hd
    saved = _lib.get_option("lm_attn_waves")
    try:
        for waves in (8, 4):
            _lib.set_option("lm_attn_waves", waves)
            for max_len, cases in ((700, ([0, 1, 5], [255, 256, 257], [511, 640, 699])), (8192, ([1, 4100, 8191],))):
                kc16, vc16 = (t.clone() for t in packed_caches(max_len, hd, fmt))
                kref, vref = kc16.clone(), vc16.clone()      # what the packed caches must hold after every call
                for lens in cases:
                    qkv = rnd(B, 3 * C, seed=9 + lens[0]).cuda()
                    out16, out32, kt, vt = attn_both(lib, fmt, hd, max_len, kc16, vc16, qkv, lens)
                    assert torch.equal(out16, out32), (hd, fmt, waves, max_len, lens, (out16 - out32).abs().max().item())
                    assert torch.isfinite(out16).all() and float(out16.abs().max()) > 0
                    _, kn, vn = (t.reshape(B, H, hd) for t in qkv.split(C, dim=1))
                    kw, vw = kref.float(), vref.float()
                    for b, ln in enumerate(lens):
                        kref[b, :, ln], vref[b, :, ln] = kn[b].to(dt), vn[b].to(dt)
                        kw[b, :, ln], vw[b, :, ln] = kn[b], vn[b]
                    # the appended rows hold torch's bits, no other element changed; the fp32 twin holds the unrounded row
                    assert torch.equal(bits(kc16), bits(kref)) and torch.equal(bits(vc16), bits(vref)), (hd, fmt, waves, max_len, lens)
                    assert torch.equal(kt, kw) and torch.equal(vt, vw)
                    assert not torch.equal(kt, kc16.float())     # (the rounding is live: the two appended rows differ)
    finally:
        _lib.set_option("lm_attn_waves", saved)


def test_attn_decode_kv16_fp16_subnormal_rows(lib):
    """K and V at scale 1e-6: more than 90 % of the cached values are fp16 subnormals (below 2^-14 = 6.1e-5).  Their widening is
    exact, so the outputs still equal the fp32 kernel's on the widened cache -- a flushed subnormal would be a zero there.  The new
    token's K/V are as small: they are appended as the subnormals torch rounds them to."""
    hd, max_len, fmt = 64, 700, "fp16"
    B, H, C = 3, 4, 4 * hd
    kc16, vc16 = (t.clone() for t in packed_caches(max_len, hd, fmt, 1e-6))
    for t in (kc16, vc16):
        w = t.float()
        assert float(((w.abs() < 2.0 ** -14) & (w != 0)).float().mean()) > 0.9
    lens = [5, 257, 699]
    qkv = rnd(B, 3 * C, seed=3)
    qkv[:, C:] *= 1e-6
    qkv = qkv.cuda()
    out16, out32, _, _ = attn_both(lib, fmt, hd, max_len, kc16, vc16, qkv, lens)
    assert torch.equal(out16, out32) and float(out16.abs().max()) > 0
    _, kn, vn = (t.reshape(B, H, hd) for t in qkv.split(C, dim=1))
    for b, ln in enumerate(lens):
        assert torch.equal(bits(kc16[b, :, ln]), bits(kn[b].to(torch.float16))) and torch.equal(bits(vc16[b, :, ln]), bits(vn[b].to(torch.float16)))
        assert float((kc16[b, :, ln].float() != 0).float().mean()) > 0.9


# ---- engine level ----------------------------------------------------------------------------------------------------------
def engine_rows(m, B, n):
    """the engine's cache, [(K, V)] per layer, each [B, n_head, n, head_dim] fp32 on the host"""
    out = []
    for i in range(m.n_layer):
        ks, vs = zip(*(m.cache_rows(i, b, 0, n) for b in range(B)))
        out.append((torch.stack(ks).cpu(), torch.stack(vs).cpu()))
    return out


def oracle_on_cache(sd, idx, H, rows, t0=0):
    """Logits [B, T - t0, V] of positions t0 .. T - 1: at step t the oracle computes the token's own K/V in fp32 and attends to
    rows[i][:, :, :t] -- the ENGINE'S cache -- in place of its own past."""
    outs = []
    with torch.no_grad():
        for t in range(t0, idx.shape[1]):
            cache = None if t == 0 else [(k[:, :, :t], v[:, :, :t]) for k, v in rows]
            lg, _ = go.forward_with_past(sd, idx[:, t:t + 1], H, cache, position=t)
            outs.append(lg[:, 0])
    return torch.stack(outs, 1)


def run(m, idx, T):
    m.reset_streams(3, T + 4)
    stepped = torch.stack([m.step(idx[:, t].contiguous()) for t in range(T)], 1)
    rows_s, nbytes = engine_rows(m, 3, T), m.cache_bytes()
    m.reset_streams(3, T + 4)
    batched = m.prefill(idx, want_logits=True)
    rows_p = engine_rows(m, 3, T)
    m.check_overflow()
    return dict(stepped=stepped.cpu(), batched=batched.cpu(), rows_s=rows_s, rows_p=rows_p, bytes=nbytes)


@pytest.fixture(scope="module")
def cases():
    """per (golden model, cache format, "lm_attn_short"), computed once: 3 x T tokens stepped and prefilled through a 16-bit-cache
    engine and an fp32-cache engine, their caches read back, the oracle on each 16-bit cache, and the 16-bit engine switched back."""
    from omnitokenizer_amd import _lib
    cache, plain = {}, {}

    def get(name, fmt, short=1):
        if (name, fmt, short) not in cache:
            saved = _lib.get_option("lm_attn_short")
            _lib.set_option("lm_attn_short", short)      # read at omnitok_lm_alloc_cache: both engines allocate below
            try:
                g, sd, dims = load_gpt_case(name)
                V, BS, L, H, C = dims
                T = min(BS - 2, 40)
                idx = torch.randint(0, V, (3, T), generator=torch.Generator().manual_seed(11))
                if (name, short) not in plain:
                    plain[name, short] = run(make_gpt(sd, dims), idx.cuda(), T)
                m16 = make_gpt(sd, dims).set_cache_format(fmt)
                assert m16.cache_format == fmt and m16.weight_format == "fp32"
                r16 = run(m16, idx.cuda(), T)
                ref_s, ref_p = oracle_on_cache(sd, idx, H, r16["rows_s"]), oracle_on_cache(sd, idx, H, r16["rows_p"])
                back = run(m16.set_cache_format("fp32"), idx.cuda(), T)
                cache[name, fmt, short] = dict(r16=r16, r32=plain[name, short], ref_s=ref_s, ref_p=ref_p, back=back, L=L)
            finally:
                _lib.set_option("lm_attn_short", saved)
        return cache[name, fmt, short]
    return get


def dmax(a, b):
    return (a.cpu() - b.cpu()).abs().max().item()


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("name", GPT_CASES)
def test_cache_contents(cases, name, fmt):
    """After stepping (the kernel's append) and after a prefill (the scatter): every layer's rows are fixed points of the rounding;
    layer 0's equal the fp32 engine's rows rounded by torch, bit for bit; the cache takes exactly half the bytes."""
    c, dt = cases(name, fmt), FMT[fmt][1]
    assert c["r16"]["bytes"] * 2 == c["r32"]["bytes"] and c["r16"]["bytes"] > 0
    for which in ("rows_s", "rows_p"):
        r16, r32 = c["r16"][which], c["r32"][which]
        assert len(r16) == c["L"]
        for i, (k, v) in enumerate(r16):
            assert torch.equal(k.to(dt).float(), k) and torch.equal(v.to(dt).float(), v), (which, i)
            assert float((k != 0).float().mean()) > 0.95 and float((v != 0).float().mean()) > 0.95     # (rows were written)
            assert not torch.equal(r32[i][0].to(dt).float(), r32[i][0])    # (the fp32 engine's rows are NOT such fixed points)
        for kv in (0, 1):
            assert torch.equal(r16[0][kv], r32[0][kv].to(dt).float()), (which, "kv"[kv])


@pytest.mark.parametrize("name,fmt,short", [(n, f, 1) for n in GPT_CASES for f in FMT] + [(GPT_CASES[0], f, 0) for f in FMT])
def test_logits_vs_oracle_on_the_engines_cache(cases, name, fmt, short):
    """Stepped logits and the teacher-forced logits of prefill(want_logits=True), each against the oracle fed that run's cache, at
    the fp32 path's LOGIT_TOL.  "lm_attn_short" 0 (256-key chunks in the step) on one model."""
    c = cases(name, fmt, short)
    es, ep = dmax(c["r16"]["stepped"], c["ref_s"]), dmax(c["r16"]["batched"], c["ref_p"])
    print(f"{name} {fmt} short {short}: stepped {es:.2e}, prefill {ep:.2e} (tol {LOGIT_TOL:.0e})")
    assert es < LOGIT_TOL and ep < LOGIT_TOL


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_long_prefix_multi_chunk(fmt):
    """test_prefill_long_prefix_multi_chunk's model: a 600-token prefix (several attention chunks, the prefill's scatter) and 6
    sampled tokens; the 6 stepped positions against the oracle on the engine's cache."""
    from omnitokenizer_amd import gpt as og
    V, BS, L, H, C = 256, 700, 1, 4, 256
    sd = go.synth_gpt_state(V, BS, L, H, C, seed=21)
    m = make_gpt(sd, (V, BS, L, H, C)).set_cache_format(fmt)
    x = torch.randint(0, V, (2, 600), generator=torch.Generator().manual_seed(22))
    new, lg = og.sample_with_past(x.cuda(), m, 6, sample_logits=False, return_logits=True)
    m.check_overflow()
    seq = torch.cat([x, new.cpu()], 1)[:, :605]          # the tokens that entered: positions 0 .. 604
    rows = engine_rows(m, 2, 605)
    ref = oracle_on_cache(sd, seq, H, rows, t0=599)
    err = dmax(lg, ref)
    print(f"long prefix {fmt}: {err:.2e}")
    assert err < LOGIT_TOL
    k = rows[0][0]
    assert torch.equal(k.to(FMT[fmt][1]).float(), k) and float((k != 0).float().mean()) > 0.95


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("name", GPT_CASES)
def test_format_is_live_and_switches_back(cases, name, fmt):
    """The rounded cache moves the stepped logits by more than the tolerance (3.3e-3 .. 1.6e-2 with bf16, 3.7e-4 .. 2.4e-3 with
    fp16 for an oracle with a rounded cache on these models); set_cache_format("fp32") gives back the fp32 engine's bits."""
    c = cases(name, fmt)
    live = dmax(c["r16"]["stepped"], c["r32"]["stepped"])
    print(f"{name} {fmt}: stepped logits move by {live:.2e}")
    assert live > LOGIT_TOL
    for k in ("stepped", "batched"):
        assert torch.equal(c["back"][k], c["r32"][k]), k
    assert c["back"]["bytes"] == c["r32"]["bytes"]


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_weight_and_cache_format_together(fmt):
    """16-bit weights + a 16-bit cache: the oracle on rounded(sd) fed the engine's cache."""
    g, sd, dims = load_gpt_case(GPT_CASES[0])
    V, BS, L, H, C = dims
    T = min(BS - 2, 40)
    idx = torch.randint(0, V, (3, T), generator=torch.Generator().manual_seed(11))
    m = make_gpt(sd, dims, fmt).set_cache_format(fmt)
    assert (m.weight_format, m.cache_format) == (fmt, fmt)
    r = run(m, idx.cuda(), T)
    rsd = rounded(sd, fmt)
    es = dmax(r["stepped"], oracle_on_cache(rsd, idx, H, r["rows_s"]))
    ep = dmax(r["batched"], oracle_on_cache(rsd, idx, H, r["rows_p"]))
    print(f"weights {fmt} + cache {fmt}: stepped {es:.2e}, prefill {ep:.2e}")
    assert es < LOGIT_TOL and ep < LOGIT_TOL


def test_graph_replay_and_stale_handles():
    from omnitokenizer_amd import gpt as og
    g, sd, dims = load_gpt_case(GPT_CASES[0])
    m = make_gpt(sd, dims).set_cache_format("bf16")
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
    assert m.set_cache_format("fp16") is m
    assert m._graphs == {} and m._cache_shape == (0, 0) and m.cache_bytes() == 0
    with pytest.raises(RuntimeError, match="replaced"):
        m.forward_with_past(x[:, :1], past=[h], past_length=4)
    # ... and the engine refuses to step without a cache instead of touching freed memory
    with pytest.raises(RuntimeError, match="cache not allocated"):
        m.step(x[:, 0].contiguous())
    tok_h = og.sample_with_past(x, m, 10, sample_logits=False, use_graph=True)
    assert tok_h.shape == tok_g.shape and m.cache_format == "fp16"


SMALL = (300, 48, 1, 4, 256)


def test_fp16_range_is_flagged(lib):
    """key.bias = 1e5: every K element is outside the fp16 range.  The fp16 cache raises bit 2 of the flag word -- from the step's
    append and from the prefill's scatter; bf16 and fp32 caches never do."""
    V, BS, L, H, C = SMALL
    sd = go.synth_gpt_state(V, BS, L, H, C, seed=25)
    sd["blocks.0.attn.key.bias"] = torch.full_like(sd["blocks.0.attn.key.bias"], 1e5)
    tok = torch.tensor([1, 2], device="cuda")
    idx = torch.randint(0, V, (2, 8), generator=torch.Generator().manual_seed(26)).cuda()
    s = torch.cuda.current_stream().cuda_stream
    m = make_gpt(sd, SMALL).set_cache_format("fp16")
    m.reset_streams(2, 16)
    m.check_overflow()
    m.step(tok)
    assert lib.omnitok_lm_overflowed(m._engine, s) == 2
    assert lib.omnitok_lm_overflowed(m._engine, s) == 0          # cleared
    k, _ = m.cache_rows(0, 0)
    assert k.shape == (H, 1, C // H) and torch.isinf(k).all()
    m.step(tok)
    with pytest.raises(RuntimeError, match=r"fp16.*bf16"):
        m.check_overflow()
    m.check_overflow()
    m.reset_streams(2, 16)
    m.prefill(idx)
    with pytest.raises(RuntimeError, match=r"fp16.*bf16"):
        m.check_overflow()
    for fmt in ("bf16", "fp32"):
        m.set_cache_format(fmt)
        m.reset_streams(2, 16)
        m.step(tok)
        m.step(tok)
        m.reset_streams(2, 16)
        m.prefill(idx)
        assert lib.omnitok_lm_overflowed(m._engine, s) == 0
        m.check_overflow()


def test_stepping_past_a_16bit_cache_is_flagged(lib):
    g, sd, dims = load_gpt_case("gpt_hd64")
    m = make_gpt(sd, dims).set_cache_format("bf16")
    m.reset_streams(1, 4)
    cap = m._cache_shape[1]
    tok = torch.tensor([1], device="cuda")
    for _ in range(cap):
        m._pos.zero_()                      # keep the position embedding in range; only the cache length grows
        m.step(tok)
    m.check_overflow()                      # `cap` tokens fit
    m._pos.zero_()
    m.step(tok)                             # one more does not
    assert lib.omnitok_lm_overflowed(m._engine, torch.cuda.current_stream().cuda_stream) == 1
    m._len.fill_(cap)
    m._pos.zero_()
    m.step(tok)
    with pytest.raises(RuntimeError, match="K/V cache"):
        m.check_overflow()
    m.check_overflow()                      # the flag was cleared


def test_cache_read_ranges_with_a_cache(lib):
    g, sd, dims = load_gpt_case("gpt_hd64")
    V, BS, L, H, C = dims
    m = make_gpt(sd, dims).set_cache_format("fp16")
    m.reset_streams(2, 8)
    mb, ml = m._cache_shape
    m.step(torch.tensor([1, 2], device="cuda"))
    k, v = m.cache_rows(L - 1, 1)
    assert k.shape == v.shape == (H, 1, C // H) and float((k != 0).float().mean()) > 0.9
    assert m.cache_rows(0, 0, 0, ml)[0].shape == (H, ml, C // H)       # the whole slab, rows beyond the length included
    assert m.cache_rows(0, 0, 1, 1)[0].shape == (H, 0, C // H)
    for args in ((L, 0, 0, 1), (0, mb, 0, 1), (0, 0, 0, ml + 1), (0, 0, ml, ml + 1), (0, 0, 2, 1)):
        with pytest.raises(ValueError, match="lm_cache_read"):
            m.cache_rows(*args)
