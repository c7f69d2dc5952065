"""CPU: the cache-format entry points of include/omnitok_lm.h (omnitok_lm_set_cache_format, omnitok_lm_cache_format,
omnitok_lm_cache_read, omnitok_lm_attn_decode_kv16) and GPT.set_cache_format -- argument errors and bookkeeping, all before any HIP
call (host addresses are never dereferenced: the calls are refused first)."""
import argparse
import ctypes
import os
import re

import pytest

KV_FP32, KV_BF16, KV_FP16 = 0, 1, 2
ERR_STATE = -3


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
    got = {n.lower(): int(v) for n, v in re.findall(r"#define OMNITOK_LM_KV_(\w+) (\d+)", hdr)}
    assert got == og.KV_FORMATS == {"fp32": KV_FP32, "bf16": KV_BF16, "fp16": KV_FP16}
    # a prefix of their own: the weight formats are still exactly three
    assert len(re.findall(r"#define OMNITOK_LM_W_(\w+) (\d+)", hdr)) == 3


def test_cache_format_argument_errors(lib):
    assert lib.omnitok_lm_set_cache_format(None, KV_BF16) == -1 and b"null" in lib.omnitok_last_error()
    assert lib.omnitok_lm_cache_format(None) == -1
    h = make_engine(lib, 300, 48, 1, 4, 256)
    try:
        assert lib.omnitok_lm_cache_format(h) == KV_FP32           # a fresh engine
        for bad in (3, -1):
            assert lib.omnitok_lm_set_cache_format(h, bad) == -1 and b"format" in lib.omnitok_last_error()
            assert lib.omnitok_lm_cache_format(h) == KV_FP32       # ... and a refused format changes nothing
        for fmt in (KV_FP16, KV_BF16, KV_FP32):
            assert lib.omnitok_lm_set_cache_format(h, fmt) == 0 and lib.omnitok_lm_cache_format(h) == fmt
            assert lib.omnitok_lm_set_cache_format(h, 7) == -1 and lib.omnitok_lm_cache_format(h) == fmt
            assert lib.omnitok_lm_weight_format(h) == 0            # independent of the weight format
            assert lib.omnitok_lm_cache_bytes(h) == 0              # no cache yet
        assert lib.omnitok_lm_set_weight_format(h, 2) == 0 and lib.omnitok_lm_cache_format(h) == KV_FP32
    finally:
        lib.omnitok_lm_destroy(h)


def test_attn_decode_kv16_argument_errors(lib):
    buf = (ctypes.c_float * 1024)()     # a host address: never dereferenced, the calls are refused first
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    tail = (p, 1, 4, 64, 128, p, p, None)    # cache_len, B, n_head, head_dim, max_len, scratch, out, stream
    assert lib.omnitok_lm_attn_decode_kv16(p, p, p, KV_FP32, *tail) == -1 and b"fmt" in lib.omnitok_last_error()
    assert lib.omnitok_lm_attn_decode_kv16(p, p, p, 3, *tail) == -1 and b"fmt" in lib.omnitok_last_error()
    for fmt in (KV_BF16, KV_FP16):
        for hole in range(3):           # qkv, kc16, vc16
            a = [p, p, p]
            a[hole] = None
            assert lib.omnitok_lm_attn_decode_kv16(*a, fmt, *tail) == -1 and b"null" in lib.omnitok_last_error()
        assert lib.omnitok_lm_attn_decode_kv16(p, p, p, fmt, None, 1, 4, 64, 128, p, p, None) == -1    # cache_len
        assert lib.omnitok_lm_attn_decode_kv16(p, p, p, fmt, p, 1, 4, 64, 128, None, p, None) == -1    # scratch
        assert lib.omnitok_lm_attn_decode_kv16(p, p, p, fmt, p, 1, 4, 64, 128, p, None, None) == -1    # out
        assert lib.omnitok_lm_attn_decode_kv16(p, p, p, fmt, p, 1, 4, 80, 128, p, p, None) == -1 and b"head_dim" in lib.omnitok_last_error()
        for off in (2, 8):
            q = ctypes.c_void_p(p.value + off)
            assert lib.omnitok_lm_attn_decode_kv16(p, q, p, fmt, *tail) == -1 and b"unaligned" in lib.omnitok_last_error()
            assert lib.omnitok_lm_attn_decode_kv16(p, p, q, fmt, *tail) == -1 and b"unaligned" in lib.omnitok_last_error()


def test_cache_read_argument_errors(lib):
    buf = (ctypes.c_float * 1024)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    assert lib.omnitok_lm_cache_read(None, 0, 0, 0, 1, p, p, None) == -1 and b"null" in lib.omnitok_last_error()
    h = make_engine(lib, 300, 48, 2, 4, 256)
    try:
        assert lib.omnitok_lm_cache_read(h, 0, 0, 0, 1, None, p, None) == -1 and b"null" in lib.omnitok_last_error()
        assert lib.omnitok_lm_cache_read(h, 0, 0, 0, 1, p, None, None) == -1
        for fmt in (KV_FP32, KV_BF16, KV_FP16):
            assert lib.omnitok_lm_set_cache_format(h, fmt) == 0
            assert lib.omnitok_lm_cache_read(h, 0, 0, 0, 1, p, p, None) == ERR_STATE and b"no cache" in lib.omnitok_last_error()
            assert lib.omnitok_lm_cache_read(h, 1, 0, 0, 0, p, p, None) == ERR_STATE
            # what no cache could satisfy is an argument error, with or without a cache
            assert lib.omnitok_lm_cache_read(h, 2, 0, 0, 1, p, p, None) == -1 and b"layer" in lib.omnitok_last_error()
            assert lib.omnitok_lm_cache_read(h, -1, 0, 0, 1, p, p, None) == -1
            assert lib.omnitok_lm_cache_read(h, 0, -1, 0, 1, p, p, None) == -1     # stream
            assert lib.omnitok_lm_cache_read(h, 0, 0, -1, 1, p, p, None) == -1     # range
            assert lib.omnitok_lm_cache_read(h, 0, 0, 0, -1, p, p, None) == -1
    finally:
        lib.omnitok_lm_destroy(h)


def test_gpt_cache_format_without_gpu():
    from omnitokenizer_amd.gpt import GPT, KV_FORMATS
    V, BS, L, H, C = 300, 48, 2, 4, 256
    m = GPT(argparse.Namespace(), V, BS, n_layer=L, n_head=H, n_embd=C)
    assert m.cache_format == "fp32" and m.weight_format == "fp32" and m.cache_bytes() == 0
    keys = list(m.state_dict())
    for fmt in ("bf16", "fp16", "fp32"):
        m._graphs[1] = "stale"
        m._cache_shape = (3, 40)
        m._engine_sig = ("kept",)
        gen = m._generation
        assert m.set_cache_format(fmt) is m
        assert m.cache_format == fmt and fmt in KV_FORMATS
        assert m._cache_shape == (0, 0) and m._graphs == {} and m._generation == gen + 1
        assert m._engine_sig == ("kept",)        # the weights are not uploaded again
        assert m.weight_format == "fp32"         # independent switches
    m.set_cache_format("bf16")
    gen = m._generation
    with pytest.raises(ValueError, match="cache format"):
        m.set_cache_format("int8")
    assert m.cache_format == "bf16" and m._generation == gen     # a refused format changes nothing
    assert m.set_weight_format("fp16").cache_format == "bf16"
    assert list(m.state_dict()) == keys and all(t.dtype.is_floating_point and t.element_size() == 4 for t in m.state_dict().values())
    with pytest.raises(RuntimeError, match="no streams"):
        m.cache_rows(0, 0)
