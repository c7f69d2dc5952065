"""The 16-bit linear format of the DiT / Latte engines, the checks that need no GPU: the switch's argument rules and read-back,
omnitok_dit_gemm16's refusals before any HIP call, the Python setter, and the restatement tests/dit16_ref.py against
tests/dit_ref.py / tests/latte_ref.py."""
import ctypes
import os
import re

import pytest
import torch

from tests import dit16_ref, dit_ref, latte_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p
FP32, BF16, FP16 = 0, 1, 2
EPI_BIAS, EPI_GELU16, EPI_GATE = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    from omnitokenizer_amd import build, _lib
    build.build()
    return _lib.load()


def err(lib):
    return lib.omnitok_last_error().decode()


def test_header_constants_and_latte_header(lib):
    from omnitokenizer_amd import _lib
    from omnitokenizer_amd.dit import LINEAR_FORMATS
    hdr = open(os.path.join(ROOT, "include", "omnitok_dit.h")).read()
    for name, value in (("OMNITOK_DIT_LIN_FP32", FP32), ("OMNITOK_DIT_LIN_BF16", BF16), ("OMNITOK_DIT_LIN_FP16", FP16),
                        ("OMNITOK_DIT_EPI_BIAS", EPI_BIAS), ("OMNITOK_DIT_EPI_GELU16", EPI_GELU16),
                        ("OMNITOK_DIT_EPI_GATE_RESIDUAL", EPI_GATE)):
        assert re.search(rf"#define {name} {value}\b", hdr), name
    assert LINEAR_FORMATS == {"fp32": FP32, "bf16": BF16, "fp16": FP16}
    # Latte's pair lives in omnitok_latte_linear.h, which omnitok_latte.h includes: header, table and library agree
    latte = open(os.path.join(ROOT, "include", "omnitok_latte.h")).read()
    assert '#include "omnitok_latte_linear.h"' in latte
    sub = open(os.path.join(ROOT, "include", "omnitok_latte_linear.h")).read()
    declared = set(re.findall(r"\b(omnitok_[a-z0-9_]+)\s*\(", sub))
    assert declared == set(_lib.LATTE_LINEAR_EXPORTED_SYMBOLS) == {"omnitok_latte_set_linear_format", "omnitok_latte_linear_format"}
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(raw, n) for n in declared)
    assert {"dit_gemm16.hip", "lm_gemm16.hip"} <= set(__import__("omnitokenizer_amd.build", fromlist=["x"]).SOURCES)


def _engines(lib):
    from omnitokenizer_amd._lib import OmnitokDitConfig, OmnitokLatteConfig
    base = dict(input_size=12, patch_size=2, in_channels=8, hidden=128, depth=2, heads=2, mlp_hidden=512, num_classes=10,
                class_dropout=0.1, learn_sigma=1)
    d, l = P(), P()
    assert lib.omnitok_dit_create(ctypes.byref(OmnitokDitConfig(**base)), ctypes.byref(d)) == 0, err(lib)
    assert lib.omnitok_latte_create(ctypes.byref(OmnitokLatteConfig(**base, num_frames=5, extras=2)), ctypes.byref(l)) == 0, err(lib)
    return (("dit", d), ("latte", l))


def test_set_linear_format_rules_and_read_back(lib):
    for api, h in _engines(lib):
        setf, getf = getattr(lib, f"omnitok_{api}_set_linear_format"), getattr(lib, f"omnitok_{api}_linear_format")
        ws = getattr(lib, f"omnitok_{api}_workspace_bytes")
        assert getf(h) == FP32                                    # the default
        assert setf(None, BF16) == -1 and "null" in err(lib)
        assert getf(None) == -1
        w32 = ws(h, 3)
        for bad in (-1, 3, 16):
            assert setf(h, bad) == -1 and "format" in err(lib)
            assert getf(h) == FP32 and ws(h, 3) == w32            # a refused value changes nothing
        for fmt in (BF16, FP16):
            assert setf(h, fmt) == 0 and getf(h) == fmt
            # the real workspace of the format: no fp32 fc1 output, a packed one of half the bytes (M = 3 * tokens rows, F = 512)
            rows = 3 * 36 * (5 if api == "latte" else 1)
            assert ws(h, 3) == w32 - rows * 512 * 2
            assert setf(h, 7) == -1 and getf(h) == fmt
        assert setf(h, FP32) == 0 and getf(h) == FP32 and ws(h, 3) == w32
        # setting a format clears `finalized`: a forward is refused for its state, not run
        assert getattr(lib, f"omnitok_{api}_forward")(h, P(16), P(16), P(16), 1, P(16), None) == -3 and "not finalized" in err(lib)
        getattr(lib, f"omnitok_{api}_destroy")(h)


def test_gemm16_refuses_bad_arguments_before_any_hip_call(lib):
    a, w, b, y, g = P(1 << 20), P(2 << 20), P(3 << 20), P(4 << 20), P(5 << 20)   # never dereferenced: every call is refused

    def call(a16=a, w16=w, fmt=BF16, bias=b, epi=EPI_BIAS, y32=y, y16=None, gate=None, ld=0, n_tok=0, x=None, M=8, N=96, K=64, flag=None):
        return lib.omnitok_dit_gemm16(a16, w16, fmt, bias, epi, y32, y16, gate, ld, n_tok, x, M, N, K, flag, None)

    cases = [
        (dict(a16=None), "null"), (dict(w16=None), "null"), (dict(bias=None), "null"),
        (dict(a16=P((1 << 20) + 8)), "unaligned"), (dict(w16=P((2 << 20) + 2)), "unaligned"), (dict(y32=P((4 << 20) + 4)), "unaligned"),
        (dict(K=48), "K % 32"), (dict(K=0), "K % 32"), (dict(M=0), "M 0"), (dict(M=(1 << 24) + 1), "2^24"), (dict(N=0), "N 0"),
        (dict(fmt=FP32), "fmt"), (dict(fmt=3), "fmt"), (dict(epi=3), "epilogue"), (dict(epi=-1), "epilogue"),
        (dict(y32=None), "do not match"),                                  # EPI_BIAS without its output
        (dict(y16=y), "do not match"),                                     # ... or with another one
        (dict(epi=EPI_GELU16), "do not match"),                            # fc1 writes y16, not y32
        (dict(epi=EPI_GELU16, y32=None, y16=y, fmt=FP16), "flag"),         # an fp16 output needs the range word
        (dict(epi=EPI_GATE, y32=None, x=y), "do not match"),               # gated form without a gate
        (dict(epi=EPI_GATE, y32=None, gate=g), "do not match"),            # ... without x
        (dict(epi=EPI_GATE, y32=None, gate=g, x=y, n_tok=0), "n_tokens"),
        (dict(epi=EPI_GATE, y32=None, gate=P((5 << 20) + 4), x=y, n_tok=4), "unaligned"),
    ]
    for kw, word in cases:
        assert call(**kw) == -1, kw
        assert word in err(lib), (kw, err(lib))
    # the producers refuse the same way
    assert lib.omnitok_dit_ln_modulate16(a, a, a, 0, 4, 4, 64, FP32, y, None, None) == -1 and "fmt" in err(lib)
    assert lib.omnitok_dit_ln_modulate16(a, a, a, 0, 4, 4, 64, FP16, y, None, None) == -1 and "null" in err(lib)
    assert lib.omnitok_dit_ln_modulate16(a, a, a, 0, 4, 4, 62, BF16, y, None, None) == -1
    assert lib.omnitok_dit_round16(a, BF16, y, 6, None, None) == -1 and "% 4" in err(lib)
    assert lib.omnitok_dit_round16(a, 5, y, 8, None, None) == -1 and "fmt" in err(lib)
    assert lib.omnitok_dit_round16(a, FP16, y, 8, None, None) == -1 and "null" in err(lib)


def test_python_switch_default_and_unknown_names():
    from omnitokenizer_amd.dit import DiT
    from omnitokenizer_amd.latte import Latte
    for m in (DiT(**dit_ref.MODELS["a"]), Latte(**latte_ref.MODELS["a"])):
        assert m.linear_format == "fp32"
        for bad in ("int8", "BF16", "", None, 1):
            with pytest.raises(ValueError, match="linear format"):
                m.set_linear_format(bad)
            assert m.linear_format == "fp32" and m._engine is None    # refused before any engine call
        with pytest.raises(AttributeError):
            m.linear_format = "bf16"                                  # read-only
        assert m.set_linear_format("bf16") is m and m.linear_format == "bf16"
        assert m.set_linear_format("fp16").linear_format == "fp16"
    # the reference's own switch means something else (the whole module in .half()) and stays refused
    m = Latte(**latte_ref.MODELS["a"]).set_linear_format("fp16")
    x, t = torch.zeros(1, 5, 8, 8, 8), torch.zeros(1, dtype=torch.long)
    with pytest.raises(NotImplementedError, match="use_fp16"):
        m(x, t, t, use_fp16=True)
    with pytest.raises(NotImplementedError, match="use_fp16"):
        m.forward_with_cfg(torch.cat([x, x]), torch.cat([t, t]), torch.cat([t, t]), 2.0, use_fp16=True)


@pytest.mark.parametrize("kind,name", [("dit", "a"), ("dit", "b"), ("latte", "a"), ("latte", "b")])
def test_restatement_without_rounding_is_the_fp64_reference(kind, name):
    mod = dit16_ref.KINDS[kind][0]
    cfg = mod.MODELS[name]
    w = mod.to_dtype(mod.make_weights(cfg, mod.SEEDS[name]), torch.float64)
    x, t, y = (torch.from_numpy(v) for v in mod.make_inputs(name))
    assert torch.equal(dit16_ref.forward(kind, w, cfg, x, t, y, None), mod.forward(w, cfg, x, t, y))
    assert torch.equal(dit16_ref.forward(kind, w, cfg, x, t, y, None, 3.5), mod.forward_with_cfg(w, cfg, x, t, y, 3.5))


def test_restatement_rounds_what_it_says_and_d_ref_is_small():
    """q is tensor.to(fmt) once; the 16-bit restatement differs from the full-precision one by far more than its own fp32 error."""
    v = torch.tensor([1.0 + 2.0 ** -9, 65520.0, 1e-7, -3.1415926], dtype=torch.float64)
    assert torch.equal(dit16_ref.q(v, "bf16"), v.to(torch.bfloat16).double()) and dit16_ref.q(v, None) is v
    assert torch.isinf(dit16_ref.q(v, "fp16")[1]) and float(dit16_ref.q(v, "fp16")[2]) == float(torch.tensor(1e-7).half())  # subnormal kept
    full, _ = dit16_ref.reference("dit", "a", None)
    for fmt in ("bf16", "fp16"):
        ref, d_ref = dit16_ref.reference("dit", "a", fmt)
        shift = float((ref - full).abs().max())
        print(f"dit a {fmt}: d_ref {d_ref:.2e}, distance from the full-precision result {shift:.2e}, max |out| {float(full.abs().max()):.2f}")
        assert 0 < d_ref < shift < 0.01 * float(full.abs().max())
