"""CPU: the attention-operand entry points of include/omnitok_lm.h (omnitok_lm_set_prefill_attention_operands,
omnitok_lm_prefill_attention_operands) and the argument checks of the building block omnitok_lm_attn_prefill16 -- all refused before
any HIP call."""
import argparse
import ctypes

import pytest

AOP_FP32, AOP_BF16, AOP_FP16 = 0, 1, 2
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


def test_symbols_exist(lib):
    for name in ("omnitok_lm_set_prefill_attention_operands", "omnitok_lm_prefill_attention_operands", "omnitok_lm_attn_prefill16"):
        assert hasattr(lib, name), name


def test_header_constants_match_the_binding():
    import os
    import re
    from omnitokenizer_amd import gpt as og
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "omnitok_lm.h")).read()
    got = {n.lower(): int(v) for n, v in re.findall(r"#define OMNITOK_LM_AOP_(\w+) (\d+)", hdr)}
    assert got == og.PREFILL_ATTENTION_OPERANDS == {"fp32": AOP_FP32, "bf16": AOP_BF16, "fp16": AOP_FP16}


def test_operands_argument_errors_and_round_trip(lib):
    assert lib.omnitok_lm_set_prefill_attention_operands(None, AOP_BF16) == -1 and b"null" in lib.omnitok_last_error()
    assert lib.omnitok_lm_prefill_attention_operands(None) == -1 and b"null" in lib.omnitok_last_error()
    h = make_engine(lib, 300, 48, 1, 4, 256)
    get = lib.omnitok_lm_prefill_attention_operands
    try:
        assert get(h) == AOP_FP32                                         # a fresh engine
        for bad in (3, -1, 7):
            assert lib.omnitok_lm_set_prefill_attention_operands(h, bad) == -1 and b"operands" in lib.omnitok_last_error()
            assert get(h) == AOP_FP32                                     # ... and a refused value changes nothing
        for fmt in (AOP_BF16, AOP_FP16, AOP_FP32, AOP_FP16):
            assert lib.omnitok_lm_set_prefill_attention_operands(h, fmt) == 0 and get(h) == fmt
            assert lib.omnitok_lm_set_prefill_attention_operands(h, 5) == -1 and get(h) == fmt
        # independent of the other four switches, in both directions
        assert (lib.omnitok_lm_weight_format(h), lib.omnitok_lm_cache_format(h), lib.omnitok_lm_prefill_format(h),
                lib.omnitok_lm_prefill_attention(h), lib.omnitok_lm_max_streams(h)) == (W_FP32, 0, 0, 0, 16)
        assert lib.omnitok_lm_set_weight_format(h, W_BF16) == 0 and lib.omnitok_lm_set_cache_format(h, 1) == 0
        assert lib.omnitok_lm_set_prefill_format(h, 1) == 0 and lib.omnitok_lm_set_max_streams(h, 64) == 0
        assert lib.omnitok_lm_set_prefill_attention(h, 1) == 0
        assert get(h) == AOP_FP16
        assert lib.omnitok_lm_set_prefill_attention_operands(h, AOP_BF16) == 0
        assert (lib.omnitok_lm_weight_format(h), lib.omnitok_lm_cache_format(h), lib.omnitok_lm_prefill_format(h),
                lib.omnitok_lm_prefill_attention(h), lib.omnitok_lm_max_streams(h)) == (W_BF16, 1, 1, 1, 64)
    finally:
        lib.omnitok_lm_destroy(h)


def _host_ptr():
    buf = (ctypes.c_float * 1024)()     # a host address: never dereferenced, the calls are refused first
    return buf, ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)


def test_attn_prefill16_argument_errors(lib):
    buf, p = _host_ptr()
    off = ctypes.c_void_p(p.value + 4)
    f = lib.omnitok_lm_attn_prefill16
    err = lib.omnitok_last_error
    # (qkv, B, T, n_head, head_dim, op_fmt, out32, out16, out_fmt, flag, stream)
    assert f(None, 1, 4, 2, 64, W_BF16, p, None, 0, None, None) == -1 and b"null" in err()
    assert f(off, 1, 4, 2, 64, W_BF16, p, None, 0, None, None) == -1 and b"unaligned" in err()
    assert f(p, 1, 4, 2, 64, W_BF16, off, None, 0, None, None) == -1 and b"unaligned" in err()
    assert f(p, 1, 4, 2, 64, W_FP16, None, off, W_BF16, None, None) == -1 and b"unaligned" in err()
    assert f(p, 1, 4, 2, 64, W_BF16, p, None, 0, ctypes.c_void_p(p.value + 2), None) == -1 and b"flag" in err()
    assert f(p, 1, 4, 2, 64, W_BF16, None, None, 0, None, None) == -1 and b"one of" in err()         # neither output
    assert f(p, 1, 4, 2, 64, W_BF16, p, p, W_BF16, None, None) == -1 and b"one of" in err()          # both
    for op in (W_FP32, 3, -1):
        assert f(p, 1, 4, 2, 64, op, p, None, 0, None, None) == -1 and b"op_fmt" in err()           # unknown operand format
        assert f(p, 1, 4, 2, 64, op, None, p, W_FP16, None, None) == -1 and b"op_fmt" in err()
    for fmt in (W_FP32, 3, -1):
        assert f(p, 1, 4, 2, 64, W_FP16, None, p, fmt, None, None) == -1 and b"out_fmt" in err()    # unknown fmt with out16
    for hd in (0, 32, 80, 100, 256, -64):
        assert f(p, 1, 4, 2, hd, W_BF16, p, None, 0, None, None) == -1 and b"head_dim" in err()
    for B, T in ((0, 4), (-1, 4), (1, 0), (1, -3), (1, 65536), (256, 256), (65535, 2), (3, 21846)):
        assert f(p, B, T, 2, 64, W_FP16, p, None, 0, None, None) == -1 and b"B * T" in err(), (B, T)
    assert f(p, 1, 4, 0, 64, W_BF16, p, None, 0, None, None) == -1
    del buf


def test_gpt_prefill_attention_operands_without_gpu():
    from omnitokenizer_amd.gpt import GPT
    m = GPT(argparse.Namespace(), 300, 48, n_layer=2, n_head=4, n_embd=256)
    assert m.prefill_attention_operands == "fp32"
    keys = list(m.state_dict())
    m._graphs[1] = "kept"
    m._engine_sig = ("kept",)
    assert m.set_prefill_attention_operands("bf16") is m and m.prefill_attention_operands == "bf16"
    assert m._engine_sig == ("kept",) and m._graphs == {1: "kept"}      # neither the engine's weights nor the graphs are dropped
    assert m.prefill_attention == "rows"                                 # the other switch is its own
    assert m.set_weight_format("fp16").prefill_attention_operands == "bf16"   # ... and it survives the switches that rebuild the engine
    assert m.set_cache_format("bf16").prefill_attention_operands == "bf16" and m.prefill_format == "fp32"
    assert list(m.state_dict()) == keys
    with pytest.raises(ValueError, match="prefill attention operands"):
        m.set_prefill_attention_operands("nope")
    assert m.prefill_attention_operands == "bf16"
    assert m.set_prefill_attention_operands("fp16").prefill_attention_operands == "fp16"
    assert m.set_prefill_attention_operands("fp32").prefill_attention_operands == "fp32"
