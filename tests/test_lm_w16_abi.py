"""CPU: the weight-format entry points of include/omnitok_lm.h (omnitok_lm_set_weight_format, omnitok_lm_weight_format,
omnitok_lm_step_weight_bytes, omnitok_lm_gemv_w16) -- argument errors and the byte count, all before any HIP call."""
import argparse
import ctypes

import pytest

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
    got = {n.lower(): int(v) for n, v in re.findall(r"#define OMNITOK_LM_W_(\w+) (\d+)", hdr)}
    assert got == og.WEIGHT_FORMATS == {"fp32": W_FP32, "bf16": W_BF16, "fp16": W_FP16}


def test_weight_format_argument_errors(lib):
    assert lib.omnitok_lm_set_weight_format(None, W_BF16) == -1 and b"null" in lib.omnitok_last_error()
    assert lib.omnitok_lm_weight_format(None) == -1
    assert lib.omnitok_lm_step_weight_bytes(None) == 0
    h = make_engine(lib, 300, 48, 1, 4, 256)
    try:
        assert lib.omnitok_lm_weight_format(h) == W_FP32          # a fresh engine
        for bad in (3, -1):
            assert lib.omnitok_lm_set_weight_format(h, bad) == -1 and b"format" in lib.omnitok_last_error()
            assert lib.omnitok_lm_weight_format(h) == W_FP32      # ... and a refused format changes nothing
        for fmt in (W_FP16, W_BF16, W_FP32):
            assert lib.omnitok_lm_set_weight_format(h, fmt) == 0 and lib.omnitok_lm_weight_format(h) == fmt
    finally:
        lib.omnitok_lm_destroy(h)


def test_gemv_w16_argument_errors(lib):
    buf = (ctypes.c_float * 1024)()     # a host address: never dereferenced, the calls are refused first
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    args = (None, None, None, None, p, 1, 4, 256, 0, None)
    assert lib.omnitok_lm_gemv_w16(p, p, W_FP32, *args) == -1 and b"fmt" in lib.omnitok_last_error()
    assert lib.omnitok_lm_gemv_w16(p, p, 3, *args) == -1
    for fmt in (W_BF16, W_FP16):
        assert lib.omnitok_lm_gemv_w16(None, p, fmt, *args) == -1 and b"null" in lib.omnitok_last_error()
        assert lib.omnitok_lm_gemv_w16(p, None, fmt, *args) == -1
        assert lib.omnitok_lm_gemv_w16(p, p, fmt, None, None, None, None, None, 1, 4, 256, 0, None) == -1
        assert lib.omnitok_lm_gemv_w16(p, p, fmt, None, None, None, None, p, 1, 4, 100, 0, None) == -1        # K % 256
        assert lib.omnitok_lm_gemv_w16(p, p, fmt, None, None, None, None, p, 17, 4, 256, 0, None) == -1       # B > 16
        assert lib.omnitok_lm_gemv_w16(p, ctypes.c_void_p(p.value + 2), fmt, *args) == -1 and b"unaligned" in lib.omnitok_last_error()


def test_step_weight_bytes(lib):
    V, C, L = 8192, 1536, 24            # the reference's LM
    want = (12 * C * C * L + V * C) * 4
    h = make_engine(lib, V, 5120, L, 16, C)
    try:
        assert lib.omnitok_lm_step_weight_bytes(h) == want
        assert lib.omnitok_lm_set_weight_format(h, W_BF16) == 0
        assert lib.omnitok_lm_step_weight_bytes(h) == want // 2
        assert lib.omnitok_lm_set_weight_format(h, W_FP16) == 0
        assert lib.omnitok_lm_step_weight_bytes(h) == want // 2
        assert lib.omnitok_lm_set_weight_format(h, W_FP32) == 0
        assert lib.omnitok_lm_step_weight_bytes(h) == want
    finally:
        lib.omnitok_lm_destroy(h)


def test_gpt_weight_format_property_without_gpu():
    from omnitokenizer_amd.gpt import GPT
    V, BS, L, H, C = 300, 48, 2, 4, 256
    m = GPT(argparse.Namespace(), V, BS, n_layer=L, n_head=H, n_embd=C)
    full = (12 * C * C * L + V * C) * 4
    assert m.weight_format == "fp32" and m.step_weight_bytes() == full
    keys = list(m.state_dict())
    m._graphs[1] = "stale"
    m._engine_sig = ("stale",)
    assert m.set_weight_format("bf16") is m
    assert m.weight_format == "bf16" and m.step_weight_bytes() == full // 2
    assert m._engine_sig is None and m._graphs == {}
    assert list(m.state_dict()) == keys and all(t.dtype.is_floating_point and t.element_size() == 4 for t in m.state_dict().values())
    with pytest.raises(ValueError, match="weight format"):
        m.set_weight_format("int8")
    assert m.set_weight_format("fp32").step_weight_bytes() == full
