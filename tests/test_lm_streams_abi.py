"""CPU: the many-stream entry points of include/omnitok_lm.h (omnitok_lm_set_max_streams, omnitok_lm_max_streams,
omnitok_lm_gemm_streams) and GPT.set_max_streams -- argument errors and bookkeeping, all before any HIP call (host addresses are
never dereferenced: the calls are refused first)."""
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


def test_max_streams_default_and_argument_errors(lib):
    assert lib.omnitok_lm_set_max_streams(None, 32) == -1 and b"null" in lib.omnitok_last_error()
    assert lib.omnitok_lm_max_streams(None) == -1
    h = make_engine(lib, 300, 48, 1, 4, 256)
    try:
        assert lib.omnitok_lm_max_streams(h) == 16                     # a fresh engine
        for bad in (0, 129, -1):
            assert lib.omnitok_lm_set_max_streams(h, bad) == -1 and b"streams" in lib.omnitok_last_error()
            assert lib.omnitok_lm_max_streams(h) == 16                 # ... and a refused n changes nothing
        # the default limit is the one the engine always had
        assert lib.omnitok_lm_alloc_cache(h, 17, 64) == -1 and b"16" in lib.omnitok_last_error()
        for n in (128, 1, 32):
            assert lib.omnitok_lm_set_max_streams(h, n) == 0 and lib.omnitok_lm_max_streams(h) == n
            assert lib.omnitok_lm_set_max_streams(h, 129) == -1 and lib.omnitok_lm_max_streams(h) == n
            assert lib.omnitok_lm_cache_bytes(h) == 0                  # no cache yet
            assert lib.omnitok_lm_weight_format(h) == 0 and lib.omnitok_lm_cache_format(h) == 0     # independent switches
        assert lib.omnitok_lm_alloc_cache(h, 33, 64) == -1 and b"32" in lib.omnitok_last_error()
        assert lib.omnitok_lm_alloc_cache(h, 0, 64) == -1
        assert lib.omnitok_lm_cache_bytes(h) == 0
    finally:
        lib.omnitok_lm_destroy(h)


def test_streams_min_option_is_readable(lib):
    from omnitokenizer_amd import _lib
    before = _lib.get_option("lm_streams_min")
    assert before == 17
    try:
        _lib.set_option("lm_streams_min", 1)
        assert _lib.get_option("lm_streams_min") == 1
        assert lib.omnitok_set_option(b"lm_streams_min", 0) == -1      # at least one stream
        assert _lib.get_option("lm_streams_min") == 1
    finally:
        _lib.set_option("lm_streams_min", before)


def test_gemm_streams_argument_errors(lib):
    buf = (ctypes.c_float * 1024)()     # a host address: never dereferenced, the calls are refused first
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)

    def call(x=p, w=p, fmt=W_FP32, bias=p, res=None, g=None, beta=None, y=p, B=17, N=300, K=256, act=0):
        return lib.omnitok_lm_gemm_streams(x, w, fmt, bias, res, g, beta, y, B, N, K, act, None)

    for fmt in (W_FP32, W_BF16, W_FP16):
        for hole in ("x", "w", "y"):
            assert call(fmt=fmt, **{hole: None}) == -1 and b"null" in lib.omnitok_last_error(), (fmt, hole)
        for B in (0, 129, -1):
            assert call(fmt=fmt, B=B) == -1 and b"bad sizes" in lib.omnitok_last_error(), B
        assert call(fmt=fmt, K=100) == -1 and b"bad sizes" in lib.omnitok_last_error()
        assert call(fmt=fmt, K=0) == -1 and call(fmt=fmt, N=0) == -1
        assert call(fmt=fmt, act=2) == -1 and b"act" in lib.omnitok_last_error()
        assert call(fmt=fmt, g=p) == -1 and b"ln_gamma" in lib.omnitok_last_error()     # gamma without beta
        for off in (4, 8):
            q = ctypes.c_void_p(p.value + off)
            for hole in ("x", "w", "y"):
                assert call(fmt=fmt, **{hole: q}) == -1 and b"unaligned" in lib.omnitok_last_error(), (fmt, hole, off)
    for fmt in (7, 3, -1):
        assert call(fmt=fmt) == -1 and b"fmt" in lib.omnitok_last_error()


def test_gpt_max_streams_without_gpu():
    from omnitokenizer_amd.gpt import GPT
    V, BS, L, H, C = 300, 48, 2, 4, 256
    m = GPT(argparse.Namespace(), V, BS, n_layer=L, n_head=H, n_embd=C)
    assert m.max_streams == 16 and m.cache_bytes() == 0
    keys = list(m.state_dict())
    for n in (128, 24, 1, 16):
        m._graphs[1] = "stale"
        m._cache_shape = (3, 40)
        m._engine_sig = ("kept",)
        gen = m._generation
        assert m.set_max_streams(n) is m
        assert m.max_streams == n
        assert m._cache_shape == (0, 0) and m._graphs == {} and m._generation == gen + 1
        assert m._engine_sig == ("kept",)        # the weights are not uploaded again
        assert m.weight_format == "fp32" and m.cache_format == "fp32"
    m.set_max_streams(24)
    gen = m._generation
    for bad in (0, 129, -3, 2.5, "32", True):
        with pytest.raises(ValueError, match="max_streams"):
            m.set_max_streams(bad)
        assert m.max_streams == 24 and m._generation == gen     # a refused n changes nothing
    assert m.set_weight_format("bf16").set_cache_format("fp16").max_streams == 24
    assert list(m.state_dict()) == keys


def test_net2net_passes_the_setting_through():
    from omnitokenizer_amd.lm_transformer import Net2NetTransformer
    base = dict(class_cond_dim=10, unconditional=False, vtokens=True, block_size=48, n_layer=1, n_head=4, n_embd=256,
                vtokens_pos=False, n_unmasked=0, starts_with_sos=False, class_first=False)
    assert Net2NetTransformer(argparse.Namespace(**base)).transformer.max_streams == 16
    assert Net2NetTransformer(argparse.Namespace(lm_max_streams=64, **base)).transformer.max_streams == 64
    with pytest.raises(ValueError, match="max_streams"):
        Net2NetTransformer(argparse.Namespace(lm_max_streams=129, **base))
