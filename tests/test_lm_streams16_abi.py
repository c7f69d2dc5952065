"""CPU: the streams-format entry points of include/omnitok_lm.h (omnitok_lm_set_streams_format, omnitok_lm_streams_format), the
argument checks of the building block omnitok_lm_gemm_streams16 -- all refused before any HIP call -- and GPT.set_streams_format."""
import argparse
import ctypes

import pytest

SF_FP32, SF_W16 = 0, 1
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
    from omnitokenizer_amd.gpt import GPT
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "omnitok_lm.h")).read()
    got = {n.lower(): int(v) for n, v in re.findall(r"#define OMNITOK_LM_SF_(\w+) (\d+)", hdr)}
    assert got == GPT.STREAMS_FORMATS == {"fp32": SF_FP32, "w16": SF_W16}


def test_streams_format_argument_errors_and_round_trip(lib):
    assert lib.omnitok_lm_set_streams_format(None, SF_W16) == -1 and b"null" in lib.omnitok_last_error()
    assert lib.omnitok_lm_streams_format(None) == -1
    h = make_engine(lib, 300, 48, 1, 4, 256)
    try:
        assert lib.omnitok_lm_streams_format(h) == SF_FP32        # a fresh engine
        for bad in (2, -1, 7):
            assert lib.omnitok_lm_set_streams_format(h, bad) == -1 and b"format" in lib.omnitok_last_error()
            assert lib.omnitok_lm_streams_format(h) == SF_FP32    # ... and a refused format changes nothing
        for fmt in (SF_W16, SF_FP32, SF_W16):
            assert lib.omnitok_lm_set_streams_format(h, fmt) == 0 and lib.omnitok_lm_streams_format(h) == fmt
            assert lib.omnitok_lm_set_streams_format(h, 5) == -1 and lib.omnitok_lm_streams_format(h) == fmt

        def others():
            return (lib.omnitok_lm_weight_format(h), lib.omnitok_lm_cache_format(h), lib.omnitok_lm_prefill_format(h),
                    lib.omnitok_lm_prefill_attention(h), lib.omnitok_lm_prefill_attention_operands(h), lib.omnitok_lm_max_streams(h))

        # independent of the other switches, in both directions
        assert others() == (W_FP32, 0, 0, 0, 0, 16)
        assert lib.omnitok_lm_set_weight_format(h, W_FP16) == 0 and lib.omnitok_lm_set_cache_format(h, 1) == 0
        assert lib.omnitok_lm_set_prefill_format(h, 1) == 0 and lib.omnitok_lm_set_prefill_attention(h, 1) == 0
        assert lib.omnitok_lm_set_prefill_attention_operands(h, 2) == 0 and lib.omnitok_lm_set_max_streams(h, 40) == 0
        assert lib.omnitok_lm_streams_format(h) == SF_W16
        assert lib.omnitok_lm_set_streams_format(h, SF_FP32) == 0 and others() == (W_FP16, 1, 1, 1, 2, 40)
        assert lib.omnitok_lm_set_streams_format(h, SF_W16) == 0 and others() == (W_FP16, 1, 1, 1, 2, 40)
    finally:
        lib.omnitok_lm_destroy(h)


def _host_ptr():
    buf = (ctypes.c_float * 1024)()     # a host address: never dereferenced, the calls are refused first
    return buf, ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)


def test_gemm_streams16_argument_errors(lib):
    buf, p = _host_ptr()
    off = ctypes.c_void_p(p.value + 4)
    g = lib.omnitok_lm_gemm_streams16
    err = lib.omnitok_last_error
    for fmt in (W_BF16, W_FP16):
        #        a16 w16 fmt  bias  res   y32   y16   B  N  K   act flag stream
        assert g(None, p, fmt, None, None, p, None, 4, 8, 64, 0, None, None) == -1 and b"null" in err()
        assert g(p, None, fmt, None, None, p, None, 4, 8, 64, 0, None, None) == -1 and b"null" in err()
        assert g(p, p, fmt, None, None, None, None, 4, 8, 64, 0, None, None) == -1 and b"one of" in err()    # neither output
        assert g(p, p, fmt, None, None, p, p, 4, 8, 64, 0, None, None) == -1 and b"one of" in err()          # both
        assert g(p, p, fmt, None, p, None, p, 4, 8, 64, 0, None, None) == -1 and b"residual" in err()        # residual + y16
        for i in (0, 1, 3, 4, 5):                                                                            # every pointer, unaligned
            args = [p, p, fmt, None, None, p, None, 4, 8, 64, 0, None, None]
            args[i] = off
            assert g(*args) == -1 and b"unaligned" in err(), i
        assert g(p, p, fmt, None, None, None, off, 4, 8, 64, 0, None, None) == -1 and b"unaligned" in err()
        for B in (0, -1, 129, 1000):
            assert g(p, p, fmt, None, None, p, None, B, 8, 64, 0, None, None) == -1 and b"B" in err()
        for N in (0, -5):
            assert g(p, p, fmt, None, None, p, None, 4, N, 64, 0, None, None) == -1 and b"N" in err()
        for K in (0, 32, 96, 100, -64):
            assert g(p, p, fmt, None, None, p, None, 4, 8, K, 0, None, None) == -1 and b"K" in err()
        for act in (2, -1):
            assert g(p, p, fmt, None, None, p, None, 4, 8, 64, act, None, None) == -1 and b"act" in err()
    for fmt in (W_FP32, 3, -1):
        assert g(p, p, fmt, None, None, p, None, 4, 8, 64, 0, None, None) == -1 and b"fmt" in err()
    del buf


def test_gpt_streams_format_without_gpu():
    from omnitokenizer_amd.gpt import GPT
    m = GPT(argparse.Namespace(), 300, 48, n_layer=2, n_head=4, n_embd=256)
    assert m.streams_format == "fp32"
    keys = list(m.state_dict())
    m._graphs[1] = "dropped"
    m._engine_sig = ("kept",)
    assert m.set_streams_format("w16") is m and m.streams_format == "w16"
    assert m._graphs == {} and m._engine_sig == ("kept",)   # the launches change: the graphs go; the engine's weights stay
    assert m.set_weight_format("bf16").streams_format == "w16"            # ... and it survives the switches that rebuild the engine
    assert m.set_cache_format("bf16").set_max_streams(40).streams_format == "w16"
    assert list(m.state_dict()) == keys
    with pytest.raises(ValueError, match="streams format"):
        m.set_streams_format("nope")
    assert m.streams_format == "w16"
    assert m.set_streams_format("fp32").streams_format == "fp32"
