"""The 16-bit attention format of the DiT and Latte engines on the GPU (DiT.set_attention_format, omnitok_dit_set_attention_format):
the golden models against tests/dit_attn16_ref.py in fp64, the switch's state, batch invariance, the fp16 range rule, the untouched
temporal path of Latte and the sampling loop.

The whole-model bar is 3 x d_ref, d_ref = the distance of the restatement's fp32 "tile" run on the CPU from its fp64 "exact" run --
computed from the restatement, never from the GPU's output (the factor is the one tests/test_gpu_dit16.py and
tests/test_gpu_lm_prefill16.py use for the same construction).  Lines starting with DIT_ATTN16_PARITY carry the measured figures
(profiles/dit_attn16_parity.json)."""
import json

import pytest
import torch

from tests import dit_attn16_ref as a16
from tests import dit_ref, latte_ref

pytestmark = pytest.mark.gpu

FMTS = a16.FMTS
CODE = {"fp32": 0, "bf16": 1, "fp16": 2}
MODS = {"dit": dit_ref, "latte": latte_ref}


@pytest.fixture(scope="module")
def lib():
    from omnitokenizer_amd import build, _lib
    build.build()
    return _lib.load()


def rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def report(**kw):
    print("DIT_ATTN16_PARITY " + json.dumps(kw))


def fresh(kind, name, edit=None):
    from omnitokenizer_amd.dit import DiT
    from omnitokenizer_amd.latte import Latte
    mod = MODS[kind]
    w = mod.make_weights(mod.MODELS[name], mod.SEEDS[name])
    if edit:
        edit(w)
    m = (DiT if kind == "dit" else Latte)(**mod.MODELS[name])
    m.load_state_dict(w, strict=True)
    return m.cuda().eval()


_MODELS = {}


def model(kind, name, afmt, lfmt="fp32"):
    """One engine per golden model, switched to the two formats (the tests below run in any order)."""
    if (kind, name) not in _MODELS:
        _MODELS[kind, name] = fresh(kind, name)
    return _MODELS[kind, name].set_linear_format(lfmt).set_attention_format(afmt)


def inputs(kind, name):
    x, t, y = (torch.from_numpy(v).cuda() for v in MODS[kind].make_inputs(name))
    return x, t, (y if kind == "dit" or latte_ref.MODELS[name]["extras"] == 2 else None)


@pytest.mark.parametrize("lin", ["fp32", "same"])
@pytest.mark.parametrize("afmt", FMTS)
@pytest.mark.parametrize("name", ["a", "b"])
@pytest.mark.parametrize("kind", ["dit", "latte"])
def test_forward_and_cfg_against_the_restatement(lib, kind, name, afmt, lin):
    lfmt = afmt if lin == "same" else "fp32"
    m = model(kind, name, afmt, lfmt)
    x, t, y = inputs(kind, name)
    scale = 4.0
    for key, out, cs in (("forward", m(x, t, y), None), ("forward_with_cfg", m.forward_with_cfg(x, t, y, scale), scale)):
        ref, d_ref = a16.model_reference(kind, name, afmt, None if lfmt == "fp32" else lfmt, cs)
        err = float((out.cpu().double() - ref).abs().max())
        report(model=f"{kind} {name}", attention_format=afmt, linear_format=lfmt, what=key, gpu_max_abs_err=err, d_ref=d_ref,
               ratio=err / d_ref, max_abs_ref=float(ref.abs().max()))
        assert out.shape == ref.shape and out.dtype == torch.float32
        assert err <= 3 * d_ref, f"{kind} {name} attention {afmt} linear {lfmt} {key}: GPU error {err:.3e} against 3 x d_ref {d_ref:.3e}"
    assert m._fn("attention_format")(m._engine) == CODE[afmt] and m._fn("linear_format")(m._engine) == CODE[lfmt]


@pytest.mark.parametrize("lfmt", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["dit", "latte"])
def test_switching_and_back_is_the_model_that_never_switched(lib, kind, lfmt):
    x, t, y = inputs(kind, "a")
    never = fresh(kind, "a").set_linear_format(lfmt)
    want, want_cfg = never(x, t, y), never.forward_with_cfg(x, t, y, 4.0)
    m = model(kind, "a", "bf16", lfmt)
    half = m(x, t, y)
    assert not torch.equal(half, want) and float((half - want).abs().max()) < 0.02
    m.set_attention_format("fp32")
    assert torch.equal(m(x, t, y), want) and torch.equal(m.forward_with_cfg(x, t, y, 4.0), want_cfg)


@pytest.mark.parametrize("kind", ["dit", "latte"])
def test_setting_the_format_does_not_refinalize(lib, kind):
    m = model(kind, "a", "fp32", "bf16")
    x, t, y = inputs(kind, "a")
    before = m(x, t, y)
    assert m.engine_missing() == []
    calls = []
    fn = m._fn
    m._fn = lambda name: (calls.append(name), fn(name))[1]
    try:
        m.set_attention_format("fp16")
        assert m._fn("attention_format")(m._engine) == 2          # applied to the existing engine at once
        after = m(x, t, y)
        assert "set_attention_format" in calls and "forward" in calls
        assert "set_weight" not in calls and "finalize" not in calls and "create" not in calls
    finally:
        del m._fn
    assert m.engine_missing() == [] and m.attention_format == "fp16" and m.linear_format == "bf16"
    assert not torch.equal(after, before) and torch.isfinite(after).all()
    # the C setter on the finalized engine: a forward still runs (finalized was not cleared), a refused value changes nothing
    assert m._fn("set_attention_format")(m._engine, 9) == -1 and m._fn("attention_format")(m._engine) == 2
    assert m._fn("set_attention_format")(m._engine, 0) == 0
    m._attention_format = "fp32"
    assert torch.equal(m(x, t, y), before)


@pytest.mark.parametrize("kind,name", [("dit", "b"), ("latte", "a")])
def test_batch_invariance_of_the_forward_bf16_bf16(lib, kind, name):
    m = model(kind, name, "bf16", "bf16")
    cfg = MODS[kind].MODELS[name]
    frames = (cfg["num_frames"],) if kind == "latte" else ()
    x = rnd(91, 5, *frames, cfg["in_channels"], cfg["input_size"], cfg["input_size"]).cuda()
    t = torch.tensor([0, 999, 500, 1, 250], device="cuda")
    y = torch.tensor([1, 10, 3, 10, 0], device="cuda")
    full = m(x, t, y)
    assert torch.isfinite(full).all()
    for i in range(5):
        assert torch.equal(m(x[i:i + 1], t[i:i + 1], y[i:i + 1]), full[i:i + 1]), i


@pytest.mark.parametrize("kind", ["dit", "latte"])
def test_check_range_names_the_attention_format(lib, kind):
    def big_q(w):
        w["blocks.0.attn.qkv.bias"][0] = 7.0e4      # column 0 of q, head 0
    m = fresh(kind, "a", big_q).set_attention_format("fp16")
    x, t, y = inputs(kind, "a")
    m(x, t, y, check_range=False)                   # returns: nothing is read back
    with pytest.raises(ValueError, match=r"a q, k or v outside the fp16 range \(attention format fp16: use bf16 or fp32\)"):
        m.check_range()
    m.check_range()                                 # the bits were cleared
    with pytest.raises(ValueError, match=r"timestep outside \[0, 1000\) and a q, k or v outside the fp16 range"):
        m(x, torch.full_like(t, 1000), y)
    m.set_attention_format("bf16")
    assert torch.isfinite(m(x, t, y)).all()         # bf16 has fp32's range: check_range passes
    m.set_attention_format("fp32")
    assert torch.isfinite(m(x, t, y)).all()


@pytest.mark.parametrize("lfmt", ["fp32", "bf16"])
def test_latte_temporal_blocks_are_untouched(lib, lfmt):
    """Spatial blocks whose attn.proj is zero contribute nothing through their attention: with them the output under attention format
    bf16 must be the fp32-attention output bit for bit -- any difference would come from the temporal path."""
    def no_spatial_proj(w):
        for i in range(0, latte_ref.MODELS["a"]["depth"], 2):
            w[f"blocks.{i}.attn.proj.weight"].zero_()
            w[f"blocks.{i}.attn.proj.bias"].zero_()
    m = fresh("latte", "a", no_spatial_proj).set_linear_format(lfmt)
    x, t, y = inputs("latte", "a")
    want = m(x, t, y)
    got = m.set_attention_format("bf16")(x, t, y)
    assert m._fn("attention_format")(m._engine) == 1
    assert torch.equal(got, want) and torch.isfinite(want).all()
    # the same model with its projections shows the switch is live
    live = fresh("latte", "a").set_linear_format(lfmt)
    assert not torch.equal(live.set_attention_format("bf16")(x, t, y), live.set_attention_format("fp32")(x, t, y))


def test_sampling_loop_bf16_bf16_is_repeatable(lib):
    from omnitokenizer_amd.diffusion import create_diffusion
    m = model("dit", "a", "bf16", "bf16")
    d = create_diffusion("4")
    z = rnd(95, 2, 8, 12, 12).cuda()
    z = torch.cat([z, z], 0)
    y = torch.tensor([1, 7, 10, 10], device="cuda")
    kw = dict(y=y, cfg_scale=4.0)

    def loop():
        torch.manual_seed(5)
        return d.p_sample_loop(m.forward_with_cfg, z.shape, z, clip_denoised=False, model_kwargs=kw, device="cuda")

    first, second = loop(), loop()
    assert first.shape == z.shape and torch.isfinite(first).all() and torch.equal(first, second)
    m.set_attention_format("fp32")
    assert not torch.equal(loop(), first)   # the loop ran the format the model held
