"""CPU: the prefill-format entry points of include/omnitok_lm.h (omnitok_lm_set_prefill_format, omnitok_lm_prefill_format) and the
argument checks of the two building blocks omnitok_lm_gemm16 / omnitok_lm_layernorm16 -- all refused before any HIP call."""
import argparse
import ctypes

import pytest

PF_FP32, PF_W16 = 0, 1
W_FP32, W_BF16, W_FP16 = 0, 1, 2


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
    import os
    import re
    from omnitokenizer_amd import gpt as og
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "omnitok_lm.h")).read()
    got = {n.lower(): int(v) for n, v in re.findall(r"#define OMNITOK_LM_PF_(\w+) (\d+)", hdr)}
    assert got == og.PREFILL_FORMATS == {"fp32": PF_FP32, "w16": PF_W16}


def test_prefill_format_argument_errors_and_round_trip(lib):
    assert lib.omnitok_lm_set_prefill_format(None, PF_W16) == -1 and b"null" in lib.omnitok_last_error()
    assert lib.omnitok_lm_prefill_format(None) == -1
    h = make_engine(lib, 300, 48, 1, 4, 256)
    try:
        assert lib.omnitok_lm_prefill_format(h) == PF_FP32        # a fresh engine
        for bad in (2, -1, 7):
            assert lib.omnitok_lm_set_prefill_format(h, bad) == -1 and b"format" in lib.omnitok_last_error()
            assert lib.omnitok_lm_prefill_format(h) == PF_FP32    # ... and a refused format changes nothing
        for fmt in (PF_W16, PF_FP32, PF_W16):
            assert lib.omnitok_lm_set_prefill_format(h, fmt) == 0 and lib.omnitok_lm_prefill_format(h) == fmt
            assert lib.omnitok_lm_set_prefill_format(h, 5) == -1 and lib.omnitok_lm_prefill_format(h) == fmt
        # independent of the other switches, in both directions
        assert lib.omnitok_lm_weight_format(h) == W_FP32 and lib.omnitok_lm_cache_format(h) == 0
        assert lib.omnitok_lm_set_weight_format(h, W_FP16) == 0 and lib.omnitok_lm_prefill_format(h) == PF_W16
    finally:
        lib.omnitok_lm_destroy(h)


def _host_ptr():
    buf = (ctypes.c_float * 1024)()     # a host address: never dereferenced, the calls are refused first
    return buf, ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)


def test_gemm16_argument_errors(lib):
    buf, p = _host_ptr()
    off = ctypes.c_void_p(p.value + 2)
    g = lib.omnitok_lm_gemm16
    for fmt in (W_BF16, W_FP16):
        assert g(None, p, fmt, None, None, p, None, 4, 8, 64, 0, None, None) == -1 and b"null" in lib.omnitok_last_error()
        assert g(p, None, fmt, None, None, p, None, 4, 8, 64, 0, None, None) == -1 and b"null" in lib.omnitok_last_error()
        assert g(off, p, fmt, None, None, p, None, 4, 8, 64, 0, None, None) == -1 and b"unaligned" in lib.omnitok_last_error()
        assert g(p, off, fmt, None, None, p, None, 4, 8, 64, 0, None, None) == -1 and b"unaligned" in lib.omnitok_last_error()
        assert g(p, p, fmt, None, None, None, None, 4, 8, 64, 0, None, None) == -1 and b"one of" in lib.omnitok_last_error()  # neither
        assert g(p, p, fmt, None, None, p, p, 4, 8, 64, 0, None, None) == -1 and b"one of" in lib.omnitok_last_error()        # both
        assert g(p, p, fmt, None, p, None, p, 4, 8, 64, 0, None, None) == -1 and b"residual" in lib.omnitok_last_error()      # + y16
        for K in (0, 16, 48, 100, -32):
            assert g(p, p, fmt, None, None, p, None, 4, 8, K, 0, None, None) == -1 and b"K" in lib.omnitok_last_error()
        for M in (0, -1, 65536):
            assert g(p, p, fmt, None, None, p, None, M, 8, 64, 0, None, None) == -1
        assert g(p, p, fmt, None, None, p, None, 4, 0, 64, 0, None, None) == -1
        assert g(p, p, fmt, None, None, p, None, 4, 8, 64, 2, None, None) == -1 and b"act" in lib.omnitok_last_error()
    for fmt in (W_FP32, 3, -1):
        assert g(p, p, fmt, None, None, p, None, 4, 8, 64, 0, None, None) == -1 and b"fmt" in lib.omnitok_last_error()
    del buf


def test_layernorm16_argument_errors(lib):
    buf, p = _host_ptr()
    off = ctypes.c_void_p(p.value + 4)
    f = lib.omnitok_lm_layernorm16
    for fmt in (W_BF16, W_FP16):
        for i in range(4):
            args = [p, p, p, p]
            args[i] = None
            assert f(*args, fmt, 3, 256, None, None) == -1 and b"null" in lib.omnitok_last_error()
            args[i] = off
            assert f(*args, fmt, 3, 256, None, None) == -1 and b"unaligned" in lib.omnitok_last_error()
        for K in (0, 16, 100, 250):
            assert f(p, p, p, p, fmt, 3, K, None, None) == -1 and b"K" in lib.omnitok_last_error()
        assert f(p, p, p, p, fmt, 0, 256, None, None) == -1
    for fmt in (W_FP32, 3):
        assert f(p, p, p, p, fmt, 3, 256, None, None) == -1 and b"fmt" in lib.omnitok_last_error()
    del buf


def test_gpt_prefill_format_without_gpu():
    from omnitokenizer_amd.gpt import GPT
    m = GPT(argparse.Namespace(), 300, 48, n_layer=2, n_head=4, n_embd=256)
    assert m.prefill_format == "fp32"
    keys = list(m.state_dict())
    m._graphs[1] = "kept"
    m._engine_sig = ("kept",)
    assert m.set_prefill_format("w16") is m and m.prefill_format == "w16"
    assert m._engine_sig == ("kept",) and m._graphs == {1: "kept"}      # neither the engine's weights nor the graphs are dropped
    assert m.set_weight_format("bf16").prefill_format == "w16"           # ... and it survives the switches that rebuild the engine
    assert list(m.state_dict()) == keys
    with pytest.raises(ValueError, match="prefill format"):
        m.set_prefill_format("nope")
    assert m.prefill_format == "w16"
    assert m.set_prefill_format("fp32").prefill_format == "fp32"
