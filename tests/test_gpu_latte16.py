"""The 16-bit linear format of the Latte video denoiser on the GPU (Latte.set_linear_format): both kinds of block run
omnitok_dit_gemm16, the temporal attention's output reaches attn.proj rounded once, the whole model against tests/dit16_ref.py in
fp64 (bar 3 x d_ref, as tests/test_gpu_dit16.py), the switch's state and batch invariance.  Lines starting with DIT16_PARITY carry
the measured figures (profiles/dit16_parity.json)."""
import os

import numpy as np
import pytest
import torch

from tests import dit16_ref, latte_ref
from tests import test_gpu_dit16 as t16
from tests.test_gpu_dit16 import lib  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FMTS = t16.FMTS


@pytest.mark.parametrize("hd", [64, 72])
@pytest.mark.parametrize("fmt", FMTS)
def test_packed_temporal_attention_output_is_the_output_rounded_once(lib, fmt, hd):
    B, F, N, heads = 2, 5, 9, 3
    qkv = t16.rnd(81 + hd, B * F * N, 3 * heads * hd).cuda()
    out32 = torch.empty(B * F * N, heads * hd, device="cuda")
    t16.ok(lib, lib.omnitok_latte_attn_temporal(t16.p(qkv), B, F, N, heads, hd, t16.p(out32), t16.stream()))
    out16, flag = t16.attn_rounded(lib, out32, fmt)
    assert torch.equal(out16.view(torch.int16), out32.to(t16.FMT[fmt][1]).view(torch.int16)) and flag == 0
    assert torch.isfinite(out32).all() and float(out32.abs().max()) > 0.5


_MODELS = {}


def model(name, fmt):
    if name not in _MODELS:
        from omnitokenizer_amd.latte import Latte
        m = Latte(**latte_ref.MODELS[name])
        m.load_state_dict(latte_ref.make_weights(latte_ref.MODELS[name], latte_ref.SEEDS[name]), strict=True)
        _MODELS[name] = m.cuda().eval()
    return _MODELS[name].set_linear_format(fmt)


def inputs(name):
    x, t, y = (torch.from_numpy(v).cuda() for v in latte_ref.make_inputs(name))
    return x, t, (y if latte_ref.MODELS[name]["extras"] == 2 else None)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", ["a", "b"])
def test_forward_and_cfg_against_the_restatement(lib, name, fmt):
    g = np.load(os.path.join(GOLDEN, f"latte_model_{name}.npz"))
    for k, v in zip(("x", "t", "y"), latte_ref.make_inputs(name)):
        assert np.array_equal(v, g[k]), k                                   # the goldens' inputs
    scale = float(g["cfg_scale"])
    m = model(name, fmt)
    x, t, y = inputs(name)
    for key, out, cs in (("forward", m(x, t, y), None), ("forward_with_cfg", m.forward_with_cfg(x, t, y, scale), scale)):
        ref, d_ref = dit16_ref.reference("latte", name, fmt, cs)
        err = float((out.cpu().double() - ref).abs().max())
        full = float((ref - torch.from_numpy(g[key])).abs().max())
        t16.report(model=f"latte {name}", fmt=fmt, what=key, gpu_max_abs_err=err, d_ref=d_ref, ratio=err / d_ref,
                   restatement_vs_full_precision_golden=full, max_abs_ref=float(ref.abs().max()))
        assert out.shape == ref.shape and out.dtype == torch.float32
        assert err <= 3 * d_ref, f"{name} {fmt} {key}: GPU error {err:.3e} against 3 x d_ref {d_ref:.3e}"


def test_switching_formats_and_back(lib):
    m = model("a", "fp32")
    x, t, y = inputs("a")
    before = m(x, t, y)
    assert m._fn("linear_format")(m._engine) == 0
    half = m.set_linear_format("bf16")(x, t, y)
    assert m._fn("linear_format")(m._engine) == 1 and m.linear_format == "bf16"
    assert not torch.equal(half, before) and float((half - before).abs().max()) < 0.02
    assert torch.equal(m.set_linear_format("fp32")(x, t, y), before)
    with pytest.raises(NotImplementedError, match="use_fp16"):   # the reference's switch stays refused under every format
        m.set_linear_format("fp16")(x, t, y, use_fp16=True)


def test_fp16_range_names_the_block_of_either_kind(lib):
    from omnitokenizer_amd.latte import Latte
    w = latte_ref.make_weights(latte_ref.MODELS["a"], latte_ref.SEEDS["a"])
    w["blocks.3.attn.proj.weight"][0, 0] = -7e4   # a temporal block
    m = Latte(**latte_ref.MODELS["a"])
    m.load_state_dict(w, strict=True)
    m = m.cuda().eval().set_linear_format("fp16")
    x, t, y = inputs("a")
    with pytest.raises(ValueError, match=r"latte_finalize: blocks\.3\.attn\.proj\.weight"):
        m(x, t, y)
    assert torch.isfinite(m.set_linear_format("bf16")(x, t, y)).all()


def test_batch_invariance_of_the_forward_bf16(lib):
    m = model("a", "bf16")
    cfg = latte_ref.MODELS["a"]
    x = t16.rnd(91, 5, cfg["num_frames"], cfg["in_channels"], cfg["input_size"], cfg["input_size"]).cuda()
    t = torch.tensor([0, 999, 500, 1, 250], device="cuda")
    y = torch.tensor([1, 10, 3, 10, 0], device="cuda")
    full = m(x, t, y)
    assert torch.isfinite(full).all()
    for i in range(5):
        assert torch.equal(m(x[i:i + 1], t[i:i + 1], y[i:i + 1]), full[i:i + 1]), i
