"""CPU: the cache-quant entry points of include/omnitok_lm.h (omnitok_lm_set_cache_quant, omnitok_lm_cache_quant,
omnitok_lm_attn_decode_kv8), GPT.set_cache_quant and Net2NetTransformer(lm_cache_quant=...) -- argument errors and bookkeeping, all
before any HIP call (host addresses are never dereferenced: the calls are refused first)."""
import argparse
import ctypes
import os
import re

import pytest

KQ_NONE, KQ_FP8 = 0, 1


@pytest.fixture(scope="module")
def lib():
    from omnitokenizer_amd import build, _lib
    build.build()
    return _lib.load()


def make_engine(lib, V, BS, L, H, C):
    from omnitokenizer_amd._lib import OmnitokLmConfig
    h = ctypes.c_void_p()
    assert lib.omnitok_lm_create(ctypes.byref(OmnitokLmConfig(V, BS, L, H, C)), ctypes.byref(h)) == 0
    return h


def test_header_constants_match_the_binding():
    from omnitokenizer_amd import gpt as og
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "omnitok_lm.h")).read()
    got = {n.lower(): int(v) for n, v in re.findall(r"#define OMNITOK_LM_KQ_(\w+) (\d+)", hdr)}
    assert got == og.CACHE_QUANTS == {"none": KQ_NONE, "fp8": KQ_FP8}
    # a switch of its own: the cache formats are still exactly three
    assert len(re.findall(r"#define OMNITOK_LM_KV_(\w+) (\d+)", hdr)) == 3 and len(og.KV_FORMATS) == 3


def test_cache_quant_argument_errors_and_round_trips(lib):
    assert lib.omnitok_lm_set_cache_quant(None, KQ_FP8) == -1 and b"null" in lib.omnitok_last_error()
    assert lib.omnitok_lm_cache_quant(None) == -1
    h = make_engine(lib, 300, 48, 1, 4, 256)
    try:
        assert lib.omnitok_lm_cache_quant(h) == KQ_NONE            # a fresh engine
        for prev in (KQ_NONE, KQ_FP8, KQ_NONE, KQ_FP8):
            assert lib.omnitok_lm_set_cache_quant(h, prev) == 0 and lib.omnitok_lm_cache_quant(h) == prev
            for bad in (2, -1, 7):
                assert lib.omnitok_lm_set_cache_quant(h, bad) == -1 and b"unknown value" in lib.omnitok_last_error()
                assert lib.omnitok_lm_cache_quant(h) == prev       # ... and a refused value changes nothing
            assert lib.omnitok_lm_cache_bytes(h) == 0              # no cache yet
    finally:
        lib.omnitok_lm_destroy(h)


def test_cache_quant_is_independent_of_the_other_switches(lib):
    h = make_engine(lib, 300, 48, 1, 4, 256)
    try:
        assert lib.omnitok_lm_set_cache_quant(h, KQ_FP8) == 0
        # the other switches keep their defaults ...
        assert lib.omnitok_lm_cache_format(h) == 0 and lib.omnitok_lm_decode_quant(h) == 0
        assert lib.omnitok_lm_weight_format(h) == 0 and lib.omnitok_lm_max_streams(h) == 16
        # ... and setting each of them leaves the quant (and the others) alone
        for fmt in (1, 2, 0, 2):
            assert lib.omnitok_lm_set_cache_format(h, fmt) == 0
            assert lib.omnitok_lm_cache_format(h) == fmt and lib.omnitok_lm_cache_quant(h) == KQ_FP8
        assert lib.omnitok_lm_set_cache_format(h, 3) == -1 and lib.omnitok_lm_cache_format(h) == 2     # format 3 is still refused
        assert lib.omnitok_lm_set_decode_quant(h, 1) == 0 and lib.omnitok_lm_cache_quant(h) == KQ_FP8
        assert lib.omnitok_lm_set_weight_format(h, 1) == 0 and lib.omnitok_lm_cache_quant(h) == KQ_FP8
        assert lib.omnitok_lm_set_max_streams(h, 32) == 0 and lib.omnitok_lm_cache_quant(h) == KQ_FP8
        assert lib.omnitok_lm_set_cache_quant(h, KQ_NONE) == 0
        assert (lib.omnitok_lm_cache_format(h), lib.omnitok_lm_decode_quant(h), lib.omnitok_lm_weight_format(h),
                lib.omnitok_lm_max_streams(h)) == (2, 1, 1, 32)
        assert lib.omnitok_lm_cache_bytes(h) == 0
    finally:
        lib.omnitok_lm_destroy(h)
    assert lib.omnitok_lm_cache_bytes(None) == 0


def test_attn_decode_kv8_argument_errors(lib):
    buf = (ctypes.c_float * 1024)()     # a host address: never dereferenced, the calls are refused first
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    f = lib.omnitok_lm_attn_decode_kv8
    tail = (p, 1, 4, 64, 128, p, p, None)    # cache_len, B, n_head, head_dim, max_len, scratch, out, stream
    for hole in range(5):               # qkv, kc8, vc8, kscale, vscale
        a = [p, p, p, p, p]
        a[hole] = None
        assert f(*a, *tail) == -1 and b"null" in lib.omnitok_last_error(), hole
    assert f(p, p, p, p, p, None, 1, 4, 64, 128, p, p, None) == -1 and b"null" in lib.omnitok_last_error()    # cache_len
    assert f(p, p, p, p, p, p, 1, 4, 64, 128, None, p, None) == -1 and b"null" in lib.omnitok_last_error()    # scratch
    assert f(p, p, p, p, p, p, 1, 4, 64, 128, p, None, None) == -1 and b"null" in lib.omnitok_last_error()    # out
    for hd in (80, 32, 0, 256):
        assert f(p, p, p, p, p, p, 1, 4, hd, 128, p, p, None) == -1 and b"head_dim" in lib.omnitok_last_error()
    for off in (1, 4, 8):
        q = ctypes.c_void_p(p.value + off)
        for hole in range(3):           # qkv, kc8, vc8
            a = [p, p, p]
            a[hole] = q
            assert f(*a, p, p, *tail) == -1 and b"unaligned" in lib.omnitok_last_error(), (off, hole)
    assert f(p, p, p, p, p, p, 1, 4, 64, 0, p, p, None) == -1 and b"sizes" in lib.omnitok_last_error()       # max_len
    assert f(p, p, p, p, p, p, 1, 0, 64, 128, p, p, None) == -1 and b"sizes" in lib.omnitok_last_error()     # n_head
    assert f(p, p, p, p, p, p, 70000, 4, 64, 128, p, p, None) == -1 and b"rows" in lib.omnitok_last_error()  # B
    assert f(None, None, None, None, None, None, 0, 4, 64, 128, None, None, None) == 0                        # B == 0: nothing to do


def test_kv16_entry_points_still_refuse_what_they_refused(lib):
    buf = (ctypes.c_float * 1024)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    tail = (p, 1, 4, 64, 128, p, p, None)
    for fmt in (0, 3, -1):
        assert lib.omnitok_lm_attn_decode_kv16(p, p, p, fmt, *tail) == -1 and b"fmt" in lib.omnitok_last_error()
    for fmt in (1, 2):
        assert lib.omnitok_lm_attn_decode_kv16(p, None, p, fmt, *tail) == -1 and b"null" in lib.omnitok_last_error()
        q = ctypes.c_void_p(p.value + 8)
        assert lib.omnitok_lm_attn_decode_kv16(p, q, p, fmt, *tail) == -1 and b"unaligned" in lib.omnitok_last_error()
        assert lib.omnitok_lm_attn_decode_kv16(p, p, p, fmt, p, 1, 4, 80, 128, p, p, None) == -1 and b"head_dim" in lib.omnitok_last_error()
    h = make_engine(lib, 300, 48, 1, 4, 256)
    try:
        for bad in (3, -1):
            assert lib.omnitok_lm_set_cache_format(h, bad) == -1 and lib.omnitok_lm_cache_format(h) == 0
    finally:
        lib.omnitok_lm_destroy(h)


def test_gpt_cache_quant_without_gpu():
    from omnitokenizer_amd.gpt import GPT, CACHE_QUANTS
    V, BS, L, H, C = 300, 48, 2, 4, 256
    m = GPT(argparse.Namespace(), V, BS, n_layer=L, n_head=H, n_embd=C)
    assert m.cache_quant == "none" and m.cache_format == "fp32" and m.cache_bytes() == 0
    keys = list(m.state_dict())
    for name in ("fp8", "none", "fp8"):
        m._graphs[1] = "stale"
        m._cache_shape = (3, 40)
        m._engine_sig = ("kept",)
        gen = m._generation
        assert m.set_cache_quant(name) is m
        assert m.cache_quant == name and name in CACHE_QUANTS
        assert m._cache_shape == (0, 0) and m._graphs == {} and m._generation == gen + 1
        assert m._engine_sig == ("kept",)        # the weights are not uploaded again
        assert (m.cache_format, m.weight_format, m.decode_quant, m.max_streams) == ("fp32", "fp32", "none", 16)
    gen = m._generation
    for bad in ("int8", "fp16", None, 1):
        with pytest.raises(ValueError, match="cache quant"):
            m.set_cache_quant(bad)
    assert m.cache_quant == "fp8" and m._generation == gen        # a refused name changes nothing
    # the other switches leave it alone, and it leaves them alone
    m.set_cache_format("bf16").set_weight_format("fp16").set_decode_quant("fp8").set_max_streams(32)
    assert m.cache_quant == "fp8"
    m.set_cache_quant("none")
    assert (m.cache_format, m.weight_format, m.decode_quant, m.max_streams) == ("bf16", "fp16", "fp8", 32)
    assert list(m.state_dict()) == keys and all(t.dtype.is_floating_point and t.element_size() == 4 for t in m.state_dict().values())
    with pytest.raises(RuntimeError, match="no streams"):
        m.cache_rows(0, 0)
    m.check_overflow()                          # no engine: nothing to report


def test_net2net_reads_lm_cache_quant():
    from omnitokenizer_amd import OmniTokenizer_VQGAN, make_args
    from omnitokenizer_amd.lm_transformer import Net2NetTransformer
    tok = OmniTokenizer_VQGAN(make_args(2, resolution=64))
    base = dict(class_cond_dim=10, unconditional=False, vtokens=False, block_size=80, n_layer=1, n_head=4, n_embd=256,
                vtokens_pos=False, n_unmasked=0, starts_with_sos=False, class_first=False)
    net = Net2NetTransformer(argparse.Namespace(**base, lm_cache_quant="fp8"), first_stage_model=tok, first_stage_key="video",
                             cond_stage_key="label")
    assert net.transformer.cache_quant == "fp8" and net.transformer.cache_format == "fp32" and net.transformer.decode_quant == "none"
    net = Net2NetTransformer(argparse.Namespace(**base), first_stage_model=tok, first_stage_key="video", cond_stage_key="label")
    assert net.transformer.cache_quant == "none"
    with pytest.raises(ValueError, match="cache quant"):
        Net2NetTransformer(argparse.Namespace(**base, lm_cache_quant="int4"), first_stage_model=tok, first_stage_key="video",
                           cond_stage_key="label")
