"""The 16-bit attention format of the DiT / Latte engines, the checks that need no GPU: the helper tests/dit_attn16_ref.py holds its
own restatement (a plain fp32 torch restatement of the contract stays inside the derived bar; restatements that break the contract --
a key dropped, a key too many, an operand left unrounded -- leave it: the bar is neither fitted to a kernel nor vacuous), the argument
rules of omnitok_dit_attn16 and of the engines' setters, and the Python switch."""
import ctypes
import os
import re

import pytest
import torch

from tests import dit16_ref, dit_attn16_ref as a16, dit_ref, latte_ref
from tests import error_bounds as eb
from tests import lm_prefill_attn16_ref as r16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p
FP32, BF16, FP16 = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    from omnitokenizer_amd import build, _lib
    build.build()
    return _lib.load()


def err(lib):
    return lib.omnitok_last_error().decode()


def ratio(c, out32):
    return eb.ratio((out32.double() - c["out64"]).abs(), c["bar"])


# ---- the helper ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", a16.FMTS)
@pytest.mark.parametrize("bh", list(a16.BH))
@pytest.mark.parametrize("hd", a16.HDS)
@pytest.mark.parametrize("N", a16.NS)
def test_fp32_restatement_is_inside_the_bar(N, hd, bh, fmt):
    c = a16.case(N, hd, bh, fmt)
    r = ratio(c, a16.emulate(c["qkv"], c["B"], N, c["H"], fmt))
    rel = float((c["bar"] / c["out64"].abs().clamp_min(1e-30)).median())
    print(f"N {N} hd {hd} bh {bh} {fmt}: fp32 torch restatement, worst err / bar {r:.3f}; median bar / |out| {rel:.2e}, "
          f"bar {float(c['bar'].min()):.2e} .. {float(c['bar'].max()):.2e}, max |out| {float(c['out64'].abs().max()):.2f}")
    assert r <= 1.0
    assert torch.isfinite(c["bar"]).all() and float(c["bar"].max()) < (0.1 if fmt == "bf16" else 0.02)   # outputs are O(1)


@pytest.mark.parametrize("fmt", a16.FMTS)
@pytest.mark.parametrize("hd", a16.HDS)
@pytest.mark.parametrize("N", a16.NS)
@pytest.mark.parametrize("keys", [-1, +1])
def test_a_key_too_few_or_too_many_leaves_the_bar(keys, N, hd, fmt):
    """The last key dropped (a tail masked one key early) / one key past N admitted as a duplicate of row N - 1 (what a clamped tile
    row is when the tail mask lets it through)."""
    c = a16.case(N, hd, 6, fmt)
    r = ratio(c, a16.emulate(c["qkv"], c["B"], N, c["H"], fmt, keys=N + keys))
    print(f"N {N} hd {hd} {fmt}: {N + keys} keys instead of {N}: worst err / bar {r:.1f}")
    assert r > 1.0


@pytest.mark.parametrize("fmt", a16.FMTS)
@pytest.mark.parametrize("hd", a16.HDS)
def test_an_unrounded_k_leaves_the_bar(hd, fmt):
    """K left in fp32 against the rounded operands of the reference; queries x 8 (the q8 case of tests/lm_prefill_attn_ref.py), so
    that a score moves by what K's rounding is worth"""
    N = 81
    c = a16.case(N, hd, 6, fmt, 8.0)
    inside = ratio(c, a16.emulate(c["qkv"], c["B"], N, c["H"], fmt))
    r = ratio(c, a16.emulate(c["qkv"], c["B"], N, c["H"], fmt, rounded=("q", "v")))
    print(f"N {N} hd {hd} {fmt} q x 8: K left unrounded: worst err / bar {r:.2f} (rounded: {inside:.3f})")
    assert inside <= 1.0 < r


def test_restated_loop_is_tile_attention_with_a_full_mask():
    for fmt in a16.FMTS:
        c = a16.case(81, 72, 6, fmt)
        B, N, H = c["B"], c["N"], c["H"]
        x = r16.round_qkv(c["qkv"], fmt).view(B, N, 3, H, 72).permute(2, 0, 3, 1, 4)
        assert torch.equal(a16.tile_attention_full(x[0], x[1], x[2], fmt, a16.KT),
                           r16.tile_attention(x[0], x[1], x[2], fmt, a16.KT, mask_shift=N))


def test_restatement_single_key_is_rounded_v():
    qkv = a16.make_qkv(2, 1, 3, 72)
    for fmt in a16.FMTS:
        v = r16.round_qkv(qkv, fmt)[:, 2 * 216:]
        out64, bar = a16.reference16(qkv, 2, 1, 3, fmt)
        assert torch.equal(out64, v.double()) and torch.equal(a16.emulate(qkv, 2, 1, 3, fmt), v)


@pytest.mark.parametrize("kind,name", [("dit", "a"), ("dit", "b"), ("latte", "a"), ("latte", "b")])
def test_model_restatement_without_attention_rounding_is_the_linear_one(kind, name):
    mod = a16.KINDS[kind][0]
    cfg = mod.MODELS[name]
    w = mod.to_dtype(mod.make_weights(cfg, mod.SEEDS[name]), torch.float64)
    x, t, y = (torch.from_numpy(v) for v in mod.make_inputs(name))
    for lfmt in (None, "bf16"):
        assert torch.equal(a16.forward(kind, w, cfg, x, t, y, lfmt, None, "exact"), dit16_ref.forward(kind, w, cfg, x, t, y, lfmt))
    assert torch.equal(a16.forward(kind, w, cfg, x, t, y, None, None, "tile", 3.5), mod.forward_with_cfg(w, cfg, x, t, y, 3.5))
    # a 16-bit attention format moves the result; d_ref (which holds the rounding of P, absent from the "exact" run) is of that size,
    # and both are small against the output
    full = mod.forward(w, cfg, x, t, y)
    ref, d_ref = a16.model_reference(kind, name, "bf16")
    shift = float((ref - full).abs().max())
    print(f"{kind} {name} attention bf16: d_ref {d_ref:.2e}, distance from the full-precision result {shift:.2e}")
    assert 0 < shift < 0.01 * float(full.abs().max()) and 0 < d_ref < 0.01 * float(full.abs().max())


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------------
def test_header_constants_and_symbols(lib):
    from omnitokenizer_amd import _lib
    from omnitokenizer_amd.dit import ATTENTION_FORMATS
    hdr = open(os.path.join(ROOT, "include", "omnitok_dit.h")).read()
    for name in ("FP32", "BF16", "FP16"):
        assert re.search(rf"#define OMNITOK_DIT_ATTN_{name} OMNITOK_DIT_LIN_{name}\b", hdr), name
    assert ATTENTION_FORMATS == {"fp32": FP32, "bf16": BF16, "fp16": FP16}
    assert {"omnitok_dit_attn16", "omnitok_dit_set_attention_format", "omnitok_dit_attention_format"} <= set(_lib.DIT_EXPORTED_SYMBOLS)
    latte = open(os.path.join(ROOT, "include", "omnitok_latte.h")).read()
    assert '#include "omnitok_latte_attention.h"' in latte
    sub = open(os.path.join(ROOT, "include", "omnitok_latte_attention.h")).read()
    declared = set(re.findall(r"\b(omnitok_[a-z0-9_]+)\s*\(", sub))
    assert declared == set(_lib.LATTE_ATTENTION_EXPORTED_SYMBOLS) == {"omnitok_latte_set_attention_format", "omnitok_latte_attention_format"}
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(raw, n) for n in declared | {"omnitok_dit_attn16"})
    src = open(os.path.join(ROOT, "omnitokenizer_amd", "csrc", "dit_common.h")).read()
    assert re.search(r"DIT_FLAG_ATTN16_RANGE = 8\b", src)


def test_attn16_refuses_bad_arguments_before_any_hip_call(lib):
    q, o, f = P(1 << 20), P(2 << 20), P(3 << 20)   # never dereferenced: every call is refused

    def call(qkv=q, B=2, N=36, heads=2, hd=72, op=BF16, out32=o, out16=None, out_fmt=0, flag=f):
        return lib.omnitok_dit_attn16(qkv, B, N, heads, hd, op, out32, out16, out_fmt, flag, None)

    cases = [
        (dict(qkv=None), "null"),
        (dict(qkv=P((1 << 20) + 8)), "unaligned"), (dict(out32=P((2 << 20) + 4)), "unaligned"),
        (dict(out32=None, out16=P((2 << 20) + 8), out_fmt=BF16), "unaligned"), (dict(flag=P((3 << 20) + 2)), "unaligned flag"),
        (dict(hd=80), "head_dim 80"), (dict(hd=96), "head_dim 96"),
        (dict(op=FP32), "op_fmt 0"), (dict(op=3), "op_fmt 3"),
        (dict(out16=o), "exactly one"), (dict(out32=None), "exactly one"),
        (dict(out32=None, out16=o, out_fmt=FP32), "out_fmt 0"), (dict(out32=None, out16=o, out_fmt=3), "out_fmt 3"),
        (dict(B=0), "B 0"), (dict(N=0), "N 0"), (dict(heads=0), "heads 0"), (dict(heads=1025), "heads 1025"),
        (dict(N=65535 * 128 + 1), "N "),
    ]
    for kw, word in cases:
        assert call(**kw) == -1, kw
        assert "dit_attn16" in err(lib) and word in err(lib), (kw, err(lib))


def _engines(lib):
    from omnitokenizer_amd._lib import OmnitokDitConfig, OmnitokLatteConfig
    base = dict(input_size=12, patch_size=2, in_channels=8, hidden=128, depth=2, heads=2, mlp_hidden=512, num_classes=10,
                class_dropout=0.1, learn_sigma=1)
    d, l = P(), P()
    assert lib.omnitok_dit_create(ctypes.byref(OmnitokDitConfig(**base)), ctypes.byref(d)) == 0, err(lib)
    assert lib.omnitok_latte_create(ctypes.byref(OmnitokLatteConfig(**base, num_frames=5, extras=2)), ctypes.byref(l)) == 0, err(lib)
    return (("dit", d), ("latte", l))


def test_set_attention_format_rules_and_read_back(lib):
    for api, h in _engines(lib):
        setf, getf = getattr(lib, f"omnitok_{api}_set_attention_format"), getattr(lib, f"omnitok_{api}_attention_format")
        lin, ws = getattr(lib, f"omnitok_{api}_linear_format"), getattr(lib, f"omnitok_{api}_workspace_bytes")
        assert setf(None, BF16) == -1 and "null" in err(lib) and f"{api}_set_attention_format" in err(lib)
        assert getf(None) == -1 and "null" in err(lib)
        assert getf(h) == FP32                                    # the default, on a created, never finalized engine
        w32 = ws(h, 3)
        for bad in (-1, 3, 16):
            assert setf(h, bad) == -1 and "format" in err(lib)
            assert getf(h) == FP32                                # a refused value changes nothing
        for fmt in (BF16, FP16, FP32, FP16):
            assert setf(h, fmt) == 0 and getf(h) == fmt
            assert setf(h, 7) == -1 and getf(h) == fmt
            assert lin(h) == FP32 and ws(h, 3) == w32             # independent of the linear format; no workspace of its own
        getattr(lib, f"omnitok_{api}_destroy")(h)


def test_python_switch_default_and_unknown_names():
    from omnitokenizer_amd.dit import DiT
    from omnitokenizer_amd.latte import Latte
    for m in (DiT(**dit_ref.MODELS["a"]), Latte(**latte_ref.MODELS["a"])):
        assert m.attention_format == "fp32"
        for bad in ("int8", "BF16", "", None, 1):
            with pytest.raises(ValueError, match="attention format"):
                m.set_attention_format(bad)
            assert m.attention_format == "fp32" and m._engine is None    # refused before any engine call
        with pytest.raises(AttributeError):
            m.attention_format = "bf16"                                  # read-only
        assert m.set_attention_format("bf16") is m and m.attention_format == "bf16"
        assert m.linear_format == "fp32"                                 # the two switches are independent
        assert m.set_linear_format("fp16").attention_format == "bf16"
        assert m.set_attention_format("fp16").attention_format == "fp16" and m.set_attention_format("fp32").attention_format == "fp32"
