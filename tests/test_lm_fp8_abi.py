"""CPU: the decode-quant entry points of include/omnitok_lm.h (omnitok_lm_set_decode_quant, omnitok_lm_decode_quant,
omnitok_lm_quantize_fp8, omnitok_lm_gemv_fp8; omnitok_lm_step_weight_bytes under the switch) -- argument errors and the byte count,
all before any HIP call -- and the torch restatement of the quantiser, omnitokenizer_amd.fp8_dequantized, against a scalar loop."""
import argparse
import ctypes
import math

import pytest
import torch

DQ_NONE, DQ_FP8 = 0, 1
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
    got = {n.lower(): int(v) for n, v in re.findall(r"#define OMNITOK_LM_DQ_(\w+) (\d+)", hdr)}
    assert got == og.DECODE_QUANTS == {"none": DQ_NONE, "fp8": DQ_FP8}
    # not a weight format: that set is what it was
    assert og.WEIGHT_FORMATS == {"fp32": W_FP32, "bf16": W_BF16, "fp16": W_FP16}


def test_decode_quant_argument_errors(lib):
    assert lib.omnitok_lm_set_decode_quant(None, DQ_FP8) == -1 and b"null" in lib.omnitok_last_error()
    assert lib.omnitok_lm_decode_quant(None) == -1
    h = make_engine(lib, 300, 48, 1, 4, 256)
    try:
        assert lib.omnitok_lm_decode_quant(h) == DQ_NONE             # a fresh engine
        for bad in (2, -1):
            assert lib.omnitok_lm_set_decode_quant(h, bad) == -1 and b"unknown value" in lib.omnitok_last_error()
            assert lib.omnitok_lm_decode_quant(h) == DQ_NONE         # ... and a refused value changes nothing
        assert lib.omnitok_lm_set_decode_quant(h, DQ_FP8) == 0 and lib.omnitok_lm_decode_quant(h) == DQ_FP8
        assert lib.omnitok_lm_set_decode_quant(h, 7) == -1 and lib.omnitok_lm_decode_quant(h) == DQ_FP8
        # independent of the weight format, in both directions
        assert lib.omnitok_lm_weight_format(h) == W_FP32
        assert lib.omnitok_lm_set_weight_format(h, W_BF16) == 0 and lib.omnitok_lm_decode_quant(h) == DQ_FP8
        assert lib.omnitok_lm_set_decode_quant(h, DQ_NONE) == 0 and lib.omnitok_lm_weight_format(h) == W_BF16
    finally:
        lib.omnitok_lm_destroy(h)


def test_gemv_fp8_argument_errors(lib):
    buf = (ctypes.c_float * 1024)()     # a host address: never dereferenced, the calls are refused first
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    args = (None, None, None, None, p, 1, 4, 256, 0, None)
    assert lib.omnitok_lm_gemv_fp8(None, p, p, *args) == -1 and b"null" in lib.omnitok_last_error()
    assert lib.omnitok_lm_gemv_fp8(p, None, p, *args) == -1 and b"null" in lib.omnitok_last_error()
    assert lib.omnitok_lm_gemv_fp8(p, p, None, *args) == -1 and b"null" in lib.omnitok_last_error()
    assert lib.omnitok_lm_gemv_fp8(p, p, p, None, None, None, None, None, 1, 4, 256, 0, None) == -1
    assert lib.omnitok_lm_gemv_fp8(p, p, p, None, None, None, None, p, 1, 4, 100, 0, None) == -1        # K % 256
    assert lib.omnitok_lm_gemv_fp8(p, p, p, None, None, None, None, p, 17, 4, 256, 0, None) == -1       # B > 16
    assert lib.omnitok_lm_gemv_fp8(p, p, p, None, None, None, None, p, 1, 0, 256, 0, None) == -1        # N
    assert lib.omnitok_lm_gemv_fp8(p, p, p, None, None, None, None, p, 1, 4, 256, 2, None) == -1        # act
    assert lib.omnitok_lm_gemv_fp8(p, p, p, None, None, p, None, p, 1, 4, 256, 0, None) == -1           # gamma without beta
    assert lib.omnitok_lm_gemv_fp8(p, ctypes.c_void_p(p.value + 4), p, *args) == -1 and b"unaligned" in lib.omnitok_last_error()
    assert lib.omnitok_lm_gemv_fp8(ctypes.c_void_p(p.value + 4), p, p, *args) == -1 and b"unaligned" in lib.omnitok_last_error()
    # the 16-bit entry keeps refusing everything but its two formats
    assert lib.omnitok_lm_gemv_w16(p, p, 3, *args) == -1


def test_quantize_fp8_argument_errors(lib):
    buf = (ctypes.c_float * 1024)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    assert lib.omnitok_lm_quantize_fp8(None, p, p, 4, 256, None, None) == -1 and b"null" in lib.omnitok_last_error()
    assert lib.omnitok_lm_quantize_fp8(p, None, p, 4, 256, None, None) == -1
    assert lib.omnitok_lm_quantize_fp8(p, p, None, 4, 256, None, None) == -1
    assert lib.omnitok_lm_quantize_fp8(p, p, p, 0, 256, None, None) == -1 and b"sizes" in lib.omnitok_last_error()
    assert lib.omnitok_lm_quantize_fp8(p, p, p, 4, 0, None, None) == -1
    assert lib.omnitok_lm_quantize_fp8(p, p, p, 4, 254, None, None) == -1                               # K % 4
    assert lib.omnitok_lm_quantize_fp8(ctypes.c_void_p(p.value + 4), p, p, 4, 256, None, None) == -1 and b"unaligned" in lib.omnitok_last_error()
    assert lib.omnitok_lm_quantize_fp8(p, ctypes.c_void_p(p.value + 4), p, 4, 256, None, None) == -1


def test_step_weight_bytes(lib):
    V, C, L = 8192, 1536, 24            # the reference's LM
    want = (12 * C * C * L + V * C) * 4
    want8 = (12 * C * C * L + V * C) * 1 + (12 * C * L + V) * 4
    h = make_engine(lib, V, 5120, L, 16, C)
    try:
        for fmt, per in ((W_FP32, 1), (W_BF16, 2), (W_FP16, 2), (W_FP32, 1)):      # the switch off: the present values
            assert lib.omnitok_lm_set_weight_format(h, fmt) == 0
            assert lib.omnitok_lm_step_weight_bytes(h) == want // per
        assert lib.omnitok_lm_set_decode_quant(h, DQ_FP8) == 0
        for fmt in (W_FP32, W_BF16, W_FP16):                                       # ... on: whatever the weight format is
            assert lib.omnitok_lm_set_weight_format(h, fmt) == 0
            assert lib.omnitok_lm_step_weight_bytes(h) == want8
        assert lib.omnitok_lm_set_decode_quant(h, 5) == -1                         # refused: nothing changes
        assert lib.omnitok_lm_step_weight_bytes(h) == want8
        assert lib.omnitok_lm_set_decode_quant(h, DQ_NONE) == 0
        assert lib.omnitok_lm_step_weight_bytes(h) == want // 2
    finally:
        lib.omnitok_lm_destroy(h)


def test_gpt_decode_quant_property_without_gpu():
    from omnitokenizer_amd.gpt import GPT
    V, BS, L, H, C = 300, 48, 2, 4, 256
    m = GPT(argparse.Namespace(), V, BS, n_layer=L, n_head=H, n_embd=C)
    full = (12 * C * C * L + V * C) * 4
    full8 = (12 * C * C * L + V * C) + (12 * C * L + V) * 4
    assert m.decode_quant == "none" and m.step_weight_bytes() == full
    keys = list(m.state_dict())
    m._graphs[1] = "stale"
    m._engine_sig = ("stale",)
    assert m.set_decode_quant("fp8") is m
    assert m.decode_quant == "fp8" and m.step_weight_bytes() == full8
    assert m._engine_sig is None and m._graphs == {}
    assert list(m.state_dict()) == keys and all(t.dtype == torch.float32 for t in m.state_dict().values())
    with pytest.raises(ValueError, match="decode quant"):
        m.set_decode_quant("int8")
    assert m.decode_quant == "fp8"
    assert m.set_weight_format("bf16").decode_quant == "fp8" and m.step_weight_bytes() == full8
    assert m.set_decode_quant("none").step_weight_bytes() == full // 2 and m.weight_format == "bf16"


def test_net2net_reads_lm_decode_quant():
    from omnitokenizer_amd import OmniTokenizer_VQGAN, make_args
    from omnitokenizer_amd.lm_transformer import Net2NetTransformer
    tok = OmniTokenizer_VQGAN(make_args(2, resolution=64))
    base = dict(class_cond_dim=10, unconditional=False, vtokens=False, block_size=80, n_layer=1, n_head=4, n_embd=256,
                vtokens_pos=False, n_unmasked=0, starts_with_sos=False, class_first=False)
    net = Net2NetTransformer(argparse.Namespace(**base, lm_decode_quant="fp8"), first_stage_model=tok, first_stage_key="video",
                             cond_stage_key="label")
    assert net.transformer.decode_quant == "fp8" and net.transformer.weight_format == "fp32"
    net = Net2NetTransformer(argparse.Namespace(**base), first_stage_model=tok, first_stage_key="video", cond_stage_key="label")
    assert net.transformer.decode_quant == "none"


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def e4m3fn_scalar(v):
    """One Python float (exactly representable in fp32, |v| <= 448) -> its e4m3fn code: round to nearest even, subnormals kept.
    The format: 1 sign, 4 exponent bits (bias 7), 3 mantissa bits; normals 2^(E - 7) (1 + M / 8), E = 1 .. 15 (E = 15 with
    M = 7 is NaN: 448 = 2^8 x 1.75 is the largest value); subnormals M x 2^-9."""
    sign = 0x80 if math.copysign(1.0, v) < 0 else 0
    a = abs(v)
    assert a <= 448
    if a == 0:
        return sign
    x = math.frexp(a)[1] - 1                    # a = f x 2^x, f in [1, 2)
    ulp = 2.0 ** (max(x, -6) - 3)               # spacing of the format at a (the subnormals share the spacing of E = 1)
    n = a / ulp                                 # exact: a power-of-two division
    lo = math.floor(n)
    r = lo + 1 if (n - lo > 0.5 or (n - lo == 0.5 and lo % 2 == 1)) else lo     # round half to even, on the integer grid
    # r counts ulps: r < 8 is a subnormal (or zero), otherwise 8 .. 16 ulps of binade max(x, -6); 16 carries into the next binade
    if r < 8:
        return sign | r
    E = max(x, -6) + 7
    if r == 16:
        E, r = E + 1, 8
    code = (E << 3) | (r - 8)
    assert code <= 0x7E
    return sign | code


def quantize_row_scalar(row):
    amax = max(abs(v) for v in row)
    if amax == 0:
        e = 0
    else:
        m, x = math.frexp(amax)
        e = x - 9 if m <= 0.875 else x - 8
        e = min(max(e, -126), 127)
    return [e4m3fn_scalar(math.ldexp(v, -e)) for v in row], math.ldexp(1.0, e)


def boundary_rows(K=32):
    """Rows of K fp32 values at the rule's and the format's boundaries (shared with the GPU quantiser test)."""
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)  # noqa: E731
    up = lambda v: float(torch.nextafter(f32(v), f32(float("inf"))))  # noqa: E731
    fill = [0.3, -0.7, 1.1, -2.9, 5.0, -13.0, 27.0, -100.0]
    rows = {}
    rows["zero"] = [0.0] * K
    for e in (0, 5, -20):                         # amax exactly 448 2^e, and one ulp above it
        rows[f"448*2^{e}"] = [math.ldexp(448.0, e)] + [math.ldexp(v, e) for v in fill]
        rows[f"448*2^{e}+ulp"] = [up(math.ldexp(448.0, e))] + [math.ldexp(v, e) for v in fill]
    rows["m=0.875"] = [0.875, -0.875] + [v / 512 for v in fill]       # (448 = 0.875 x 2^9: the same boundary at another octave)
    rows["m=0.875+ulp"] = [-up(0.875)] + [v / 512 for v in fill]
    rows["m=0.5"] = [0.5] + [v / 1024 for v in fill]
    # e4m3 midpoints after scaling (amax 256 -> e = 0): between 16 and 18 (tie -> 16), 18 and 20 (-> 20), 1.0625 (-> 1.0),
    # 1.1875 (-> 1.25), 240 / 256 midpoint 248 (-> 256); and neighbours one fp32 ulp off the ties
    ties = [17.0, 19.0, -17.0, -19.0, 1.0625, 1.1875, 248.0, up(17.0), -up(19.0), 16.999998, 2.0 ** -6 + 2.0 ** -10]
    rows["ties"] = [256.0] + ties
    # subnormal results (amax 256 -> e = 0): the subnormals k 2^-9, their midpoints, half the smallest (tie -> 0), just above it,
    # three halves of it (tie -> 2 x 2^-9), the largest subnormal and its tie with the smallest normal
    sub = [2.0 ** -9, 2.0 ** -10, up(2.0 ** -10), 3 * 2.0 ** -10, -2.0 ** -10, -3 * 2.0 ** -10, 7 * 2.0 ** -9, 15 * 2.0 ** -10,
           5 * 2.0 ** -10, 2.0 ** -11, -2.0 ** -30, 2.0 ** -6]
    rows["subnormals"] = [256.0] + sub
    rows["negative zero"] = [-0.0, 1.0, -0.0, 0.0, -1.0]
    for e in (-60, -30, 30, 100, -120):           # scales many octaves apart
        rows[f"octave {e}"] = [math.ldexp(v, e) for v in fill] + [math.ldexp(-1.0, e - 12)]
    rows["fp32 subnormal amax"] = [2.0 ** -140, -2.0 ** -149]          # e clamps at -126
    rows["fp32 max"] = [3.4028234663852886e38, -1.0e38, 1.0]
    w = torch.zeros(len(rows), K)
    for i, r in enumerate(rows.values()):
        assert len(r) <= K
        w[i, :len(r)] = torch.tensor(r, dtype=torch.float64).to(torch.float32)
    return list(rows), w


def test_fp8_quantize_rows_against_scalar_loop():
    from omnitokenizer_amd.gpt import fp8_quantize_rows
    names, w = boundary_rows()
    g = torch.Generator().manual_seed(3)
    w = torch.cat([w, torch.randn(6, w.shape[1], generator=g) * torch.logspace(-3, 3, 6)[:, None]])
    names += [f"random {i}" for i in range(6)]
    q, s = fp8_quantize_rows(w)
    codes = q.view(torch.uint8)
    assert not ((codes & 0x7F) == 0x7F).any()                         # never the NaN code: nothing saturates, nothing is NaN
    for i, name in enumerate(names):
        want_q, want_s = quantize_row_scalar([float(v) for v in w[i]])
        assert float(s[i]) == want_s, name
        assert codes[i].tolist() == want_q, name
        amax = float(w[i].abs().max())
        if amax > 0 and math.log2(want_s) > -126:                     # the smallest power of two that fits 448
            assert amax / want_s <= 448 < 2 * amax / want_s, name
    by = dict(zip(names, range(len(names))))
    assert float(s[by["zero"]]) == 1.0 and float(s[by["448*2^0"]]) == 1.0 and float(s[by["448*2^0+ulp"]]) == 2.0
    assert float(s[by["m=0.875"]]) == 2.0 ** -9 and float(s[by["m=0.875+ulp"]]) == 2.0 ** -8
    assert float(s[by["fp32 subnormal amax"]]) == 2.0 ** -126
    assert codes[by["negative zero"]][:5].tolist() == [0x80, 0x78, 0x80, 0x00, 0xF8]   # amax 1 = 0.5 x 2^1 -> e = -8; 256 = 0x78


def test_fp8_dequantized_replaces_the_five_families_only():
    from oracle import gpt_oracle as go
    from omnitokenizer_amd import fp8_dequantized
    from omnitokenizer_amd.gpt import fp8_quantize_rows
    sd = go.synth_gpt_state(300, 48, 2, 4, 256, seed=31)
    out = fp8_dequantized(sd)
    assert list(out) == list(sd)
    mats = (".attn.key.weight", ".attn.query.weight", ".attn.value.weight", ".attn.proj.weight", ".mlp.0.weight", ".mlp.2.weight")
    n = 0
    for k, v in sd.items():
        if k == "head.weight" or k.endswith(mats):
            q, s = fp8_quantize_rows(v)
            want = q.float() * s[:, None]
            assert out[k].dtype == torch.float32 and torch.equal(out[k], want), k
            rel = ((want - v).abs() / v.abs().clamp_min(1e-30))[v.abs() > s[:, None] * 2.0 ** -6]
            assert float(rel.max()) <= 2.0 ** -4, k                   # 3 mantissa bits: half an ulp of a normal
            n += 1
        else:
            assert out[k] is v, k
    assert n == 6 * 2 + 1
