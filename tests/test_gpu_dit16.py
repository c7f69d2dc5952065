"""The 16-bit linear format of the DiT on the GPU (DiT.set_linear_format, omnitok_dit_gemm16): the GEMM and its three epilogues
against fp64 with derived bars, bitwise row independence, the producers of the packed operands against torch's own rounding, the
whole model against tests/dit16_ref.py in fp64, the switch's state, the fp16 range rules, the sampling loop and batch invariance.

The whole-model bar is 3 x d_ref, d_ref = the distance of the restatement's fp32 CPU run from its fp64 run -- computed here from
the restatement, never from the GPU's output (the factor is the one tests/test_gpu_lm_prefill16.py uses for the same
construction).  Lines starting with DIT16_PARITY carry the measured figures (profiles/dit16_parity.json)."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import dit16_ref, dit_ref
from tests import error_bounds as eb

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
U = eb.U
P = ctypes.c_void_p
FMT = {"bf16": (1, torch.bfloat16), "fp16": (2, torch.float16)}
FMTS = ["bf16", "fp16"]
EPI_BIAS, EPI_GELU16, EPI_GATE = 0, 1, 2
F16_RANGE = 4  # DIT_FLAG_F16_RANGE
N_TOK = 36     # tokens per sample of the gated form: 128-row tiles span two samples' gate rows


@pytest.fixture(scope="module")
def lib():
    from omnitokenizer_amd import build, _lib
    build.build()
    return _lib.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


def ok(lib, rc):
    assert rc == 0, lib.omnitok_last_error().decode()


def p(t):
    return None if t is None else P(t.data_ptr())


def rnd(seed, *shape, scale=1.0):
    return torch.from_numpy((np.random.default_rng(seed).normal(size=shape) * scale).astype(np.float32))


def report(**kw):
    print("DIT16_PARITY " + json.dumps(kw))


def gemm16(lib, a16, w16, fmt, bias, epi, y32=None, y16=None, gate=None, ld_gate=0, n_tokens=0, x=None, flag=None):
    M, K = a16.shape
    ok(lib, lib.omnitok_dit_gemm16(p(a16), p(w16), FMT[fmt][0], p(bias), epi, p(y32), p(y16), p(gate), ld_gate, n_tokens, p(x), M,
                                   w16.shape[0], K, p(flag), stream()))


def gelu_tanh64(v):
    return 0.5 * v * (1 + torch.tanh(np.sqrt(2 / np.pi) * (v + 0.044715 * v ** 3)))


# ---- the GEMM against fp64 ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gemm_case(fmt, M, N, K):
    """Operands exactly representable in the format, the fp64 results of the three epilogues and their bars; once per case.
    acc: K exact products added in fp32 (at most K roundings on a product's path) -> gamma(K) sum |a||w|; + bias one more.
    gelu: |d gelu / dx| <= 1.13 on that error, plus the fp32 evaluation of tests/test_gpu_dit.py's GELU bar
    (0.5 |v| 12 u + 3 u |g|); the 16-bit rounding is checked by bracketing.  gate: x + g y in ONE rounding (an fma) on y's error:
    |g| bar (1 + u) + u |result|."""
    dt = FMT[fmt][1]
    a16, w16 = rnd(1, M, K).to(dt), rnd(2, N, K, scale=0.05).to(dt)
    rows = (M + N_TOK - 1) // N_TOK
    bias, x, gate = rnd(3, N, scale=0.5), rnd(4, M, N), rnd(5, rows, N + 32)
    a, w, b = a16.double(), w16.double(), bias.double()
    pre = a @ w.t() + b
    bar = eb.gamma(K + 1) * (a.abs() @ w.abs().t() + b.abs())
    gelu = gelu_tanh64(pre)
    bar_gelu = eb.GELU_DERIV_MAX * bar + 0.5 * pre.abs() * 12 * U + 3 * U * gelu.abs()
    g = gate[:, 32:].double().repeat_interleave(N_TOK, 0)[:M]
    gated = x.double() + g * pre
    bar_gated = g.abs() * bar * (1 + U) + U * gated.abs()
    return dict(a16=a16, w16=w16, bias=bias, x=x, gate=gate, pre=pre, bar=bar, gelu=gelu, bar_gelu=bar_gelu, gated=gated,
                bar_gated=bar_gated)


def between(y16, lo64, hi64, dt):
    """round16(lo) <= y16 <= round16(hi) elementwise, the ends rounded by torch"""
    y = y16.cpu().double()
    return bool(((y >= lo64.to(dt).double()) & (y <= hi64.to(dt).double())).all())


def run_case(lib, fmt, M, N, K):
    c = gemm_case(fmt, M, N, K)
    dt = FMT[fmt][1]
    a, w, bias = c["a16"].cuda(), c["w16"].cuda(), c["bias"].cuda()
    y = torch.full((M, N), float("nan"), device="cuda")
    gemm16(lib, a, w, fmt, bias, EPI_BIAS, y32=y)
    r0 = eb.ratio((y.cpu().double() - c["pre"]).abs(), c["bar"])
    y16 = torch.full((M, N), float("nan"), device="cuda", dtype=dt)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    gemm16(lib, a, w, fmt, bias, EPI_GELU16, y16=y16, flag=flag)
    in_bracket = between(y16, c["gelu"] - c["bar_gelu"], c["gelu"] + c["bar_gelu"], dt)
    x, gate = c["x"].cuda(), c["gate"].cuda()
    gemm16(lib, a, w, fmt, bias, EPI_GATE, gate=gate[:, 32:], ld_gate=gate.shape[1], n_tokens=N_TOK, x=x)
    r2 = eb.ratio((x.cpu().double() - c["gated"]).abs(), c["bar_gated"])
    print(f"dit_gemm16 {fmt} M {M} N {N} K {K}: err / bar: bias {r0:.3f}, gated {r2:.3f}; gelu16 inside its bracket: {in_bracket}")
    assert r0 <= 1.0 and r2 <= 1.0 and in_bracket
    assert int(flag.item()) == 0 and torch.isfinite(y16.float()).all()


@pytest.mark.parametrize("K", [32, 96, 288])       # the half trip alone, a full trip and a half trip, four full trips and a half
@pytest.mark.parametrize("N", [96, 128, 160])      # an N tail, one whole tile, a tile and a tail
@pytest.mark.parametrize("M", [1, 108, 130])       # one row, an M tail, a tile and a tail
@pytest.mark.parametrize("fmt", FMTS)
def test_gemm16_against_fp64(lib, fmt, M, N, K):
    run_case(lib, fmt, M, N, K)


@pytest.mark.parametrize("fmt", FMTS)
def test_gemm16_gated_tile_spans_two_samples(lib, fmt):
    """M = 180 rows of 36 tokens: the first 128-row tile holds samples 0 .. 3 (the fourth cut by the tile edge), the second the
    rest -- every row must take the gate row of ITS sample."""
    run_case(lib, fmt, 180, 160, 96)
    c = gemm_case(fmt, 180, 160, 96)
    g = c["gate"][:, 32:].double()
    assert float((g[0] - g[1]).abs().min()) > 0   # the samples' gates differ in every column: a wrong row cannot pass the bar
    wrong = c["x"].double() + g.roll(1, 0).repeat_interleave(N_TOK, 0) * c["pre"]
    assert eb.ratio((wrong - c["gated"]).abs(), c["bar_gated"]) > 1e3


# ---- bitwise rows ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_rows_do_not_depend_on_the_batch_or_on_other_rows(lib, fmt):
    """fc1 and the gated epilogue: sample i of a B = 5 call has the bits of the B = 1 call, also with NaN in every other sample's
    operand rows, residual rows and gate row."""
    B, N, K, dt = 5, 160, 96, FMT[fmt][1]
    M = B * N_TOK
    a, w, bias = rnd(11, M, K).to(dt).cuda(), rnd(12, N, K, scale=0.05).to(dt).cuda(), rnd(13, N).cuda()
    x0, gate = rnd(14, M, N).cuda(), rnd(15, B, 2 * N).cuda()
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")

    def both(a, x, gate, rows):
        h = torch.empty(rows, N, device="cuda", dtype=dt)
        gemm16(lib, a, w, fmt, bias, EPI_GELU16, y16=h, flag=flag)
        x = x.clone()
        gemm16(lib, a, w, fmt, bias, EPI_GATE, gate=gate, ld_gate=gate.shape[1], n_tokens=N_TOK, x=x)
        return h.view(torch.int16), x

    full_h, full_x = both(a, x0, gate, M)
    for i in range(B):
        r = slice(i * N_TOK, (i + 1) * N_TOK)
        h, x = both(a[r].contiguous(), x0[r].contiguous(), gate[i:i + 1].contiguous(), N_TOK)
        assert torch.equal(h, full_h[r]) and torch.equal(x, full_x[r]), i
        an, xn, gn = a.clone(), x0.clone(), gate.clone()
        keep = torch.zeros(M, dtype=torch.bool, device="cuda")
        keep[r] = True
        an[~keep], xn[~keep] = float("nan"), float("nan")
        gn[torch.arange(B, device="cuda") != i] = float("nan")
        h, x = both(an, xn, gn, M)
        assert torch.equal(h[r], full_h[r]) and torch.equal(x[r], full_x[r]), i
        assert torch.isnan(x[~keep]).all()
    assert int(flag.item()) == 0


# ---- the producers of the packed operands ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_ln_modulate16_is_ln_modulate_rounded_once(lib, fmt):
    code, dt = FMT[fmt]
    B, n_tok, D, ld = 3, 5, 160, 3 * 160 + 32
    x = (rnd(41, B * n_tok, D, scale=2.0) + 0.5).cuda()
    x[7] = 0.75  # a constant row
    mod = rnd(42, B, ld, scale=0.3).cuda()
    mod[1, 32 + D:32 + 2 * D] = -1.0  # scale -1: a row of sample 1 is its shift -- fp16 subnormals and the ends of its range
    mod[1, 32:32 + 8] = torch.tensor([1e-7, -3e-8, 6e-8, 2e-5, -6.1e-5, 0.0, 65504.0, -65519.0])
    args = (p(x), P(mod.data_ptr() + 32 * 4), P(mod.data_ptr() + (32 + D) * 4), ld, B * n_tok, n_tok, D)
    out32 = torch.empty_like(x)
    ok(lib, lib.omnitok_dit_ln_modulate(*args, p(out32), stream()))
    out16 = torch.empty(B * n_tok, D, device="cuda", dtype=dt)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    ok(lib, lib.omnitok_dit_ln_modulate16(*args, code, p(out16), p(flag), stream()))
    assert torch.equal(out16.view(torch.int16), out32.to(dt).view(torch.int16))
    assert int(flag.item()) == 0 and torch.isfinite(out16.float()).all()
    if fmt == "fp16":
        sub = (out16.float().abs() < 2.0 ** -14) & (out16.float() != 0)
        assert int(sub.sum()) >= 3  # subnormal results are kept, not flushed
    # a finite value outside the fp16 range: +-inf and the range bit under fp16, neither under bf16
    mod[2, 32 + 5] = 7e4
    ok(lib, lib.omnitok_dit_ln_modulate(*args, p(out32), stream()))
    ok(lib, lib.omnitok_dit_ln_modulate16(*args, code, p(out16), p(flag), stream()))
    assert torch.equal(out16.view(torch.int16), out32.to(dt).view(torch.int16))
    assert int(flag.item()) == (F16_RANGE if fmt == "fp16" else 0)
    assert bool(torch.isinf(out16[2 * n_tok:, 5].float()).all()) == (fmt == "fp16")


def attn_rounded(lib, out32, fmt):
    """the rounding pass the engine runs behind its attention kernels, and the range word it left"""
    code, dt = FMT[fmt]
    out16 = torch.empty(out32.shape, device="cuda", dtype=dt)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    ok(lib, lib.omnitok_dit_round16(p(out32), code, p(out16), out32.numel(), p(flag), stream()))
    return out16, int(flag.item())


@pytest.mark.parametrize("hd", [64, 72])
@pytest.mark.parametrize("fmt", FMTS)
def test_packed_attention_output_is_the_attention_output_rounded_once(lib, fmt, hd):
    B, N, heads = 3, 36, 2
    qkv = rnd(61 + hd, B * N, 3 * heads * hd).cuda()
    out32 = torch.empty(B * N, heads * hd, device="cuda")
    ok(lib, lib.omnitok_dit_attn(p(qkv), B, N, heads, hd, p(out32), stream()))
    out16, flag = attn_rounded(lib, out32, fmt)
    assert torch.equal(out16.view(torch.int16), out32.to(FMT[fmt][1]).view(torch.int16)) and flag == 0
    # NaN, +-inf and a finite value past the range: torch's bits; only the last raises the bit, and only under fp16
    out32[0, :4] = torch.tensor([float("nan"), float("inf"), -float("inf"), 1e5], device="cuda")
    out16, flag = attn_rounded(lib, out32[:1].contiguous(), fmt)
    want = out32[:1].to(FMT[fmt][1])
    assert torch.equal(torch.isnan(out16), torch.isnan(want))
    assert torch.equal(out16.view(torch.int16)[:, 1:], want.view(torch.int16)[:, 1:]) and flag == (F16_RANGE if fmt == "fp16" else 0)
    out32[0, 3] = 0.0
    assert attn_rounded(lib, out32[:1].contiguous(), fmt)[1] == 0   # an infinity that was one already is not a range error


@pytest.mark.parametrize("fmt", FMTS)
def test_fc1_epilogue_is_the_gelu_kernel_on_the_same_accumulators(lib, fmt):
    """EPI_GELU16 against omnitok_dit_gelu_tanh applied to EPI_BIAS's fp32 output (the same accumulators) and rounded by torch:
    within one 16-bit ulp, at most 1 element in 1000 off by that ulp (a last-bit difference in tanhf may flip a rounding).
    Observed on an MI355X: bf16 0 of 20800 elements differ, fp16 3 of 20800 by one ulp."""
    M, N, K, dt = 130, 160, 288, FMT[fmt][1]
    a, w, bias = rnd(71, M, K).to(dt).cuda(), rnd(72, N, K, scale=0.08).to(dt).cuda(), rnd(73, N, scale=0.5).cuda()
    pre = torch.empty(M, N, device="cuda")
    gemm16(lib, a, w, fmt, bias, EPI_BIAS, y32=pre)
    assert float(pre.abs().max()) > 2.0 and float(pre.min()) < -1.0   # both tails of the GELU
    ok(lib, lib.omnitok_dit_gelu_tanh(p(pre), pre.numel(), stream()))
    want = pre.to(dt)
    got = torch.empty(M, N, device="cuda", dtype=dt)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    gemm16(lib, a, w, fmt, bias, EPI_GELU16, y16=got, flag=flag)
    assert torch.equal(torch.signbit(got.float()) | (got == 0), torch.signbit(want.float()) | (want == 0))
    ulps = (got.view(torch.int16).int() - want.view(torch.int16).int()).abs()   # same sign: the distance in 16-bit ulps
    ulps = torch.where((got == 0) & (want == 0), torch.zeros_like(ulps), ulps)
    off = int((ulps > 0).sum())
    report(what=f"fc1 epilogue vs gelu kernel, {fmt}", elements=M * N, differ_by_one_ulp=off, max_ulps=int(ulps.max()))
    assert int(ulps.max()) <= 1 and off * 1000 <= M * N
    assert int(flag.item()) == 0


# ---- the whole model -------------------------------------------------------------------------------------------------------------------
_MODELS = {}


def model(name, fmt):
    """One DiT per golden model, switched to fmt (the tests below run in any order)."""
    if name not in _MODELS:
        from omnitokenizer_amd.dit import DiT
        m = DiT(**dit_ref.MODELS[name])
        m.load_state_dict(dit_ref.make_weights(dit_ref.MODELS[name], dit_ref.SEEDS[name]), strict=True)
        _MODELS[name] = m.cuda().eval()
    return _MODELS[name].set_linear_format(fmt)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", ["a", "b"])
def test_forward_and_cfg_against_the_restatement(lib, name, fmt):
    g = np.load(os.path.join(GOLDEN, f"dit_model_{name}.npz"))
    x, t, y = dit_ref.make_inputs(name)
    assert np.array_equal(x, g["x"]) and np.array_equal(t, g["t"]) and np.array_equal(y, g["y"])   # the goldens' inputs
    scale = float(g["cfg_scale"])
    m = model(name, fmt)
    x, t, y = (torch.from_numpy(v).cuda() for v in (x, t, y))
    for key, out, cs in (("forward", m(x, t, y), None), ("forward_with_cfg", m.forward_with_cfg(x, t, y, scale), scale)):
        ref, d_ref = dit16_ref.reference("dit", name, fmt, cs)
        err = float((out.cpu().double() - ref).abs().max())
        full = float((ref - torch.from_numpy(g[key])).abs().max())
        report(model=f"dit {name}", fmt=fmt, what=key, gpu_max_abs_err=err, d_ref=d_ref, ratio=err / d_ref,
               restatement_vs_full_precision_golden=full, max_abs_ref=float(ref.abs().max()))
        assert out.shape == ref.shape and out.dtype == torch.float32
        assert err <= 3 * d_ref, f"{name} {fmt} {key}: GPU error {err:.3e} against 3 x d_ref {d_ref:.3e}"


def test_switching_formats_and_back(lib):
    m = model("a", "fp32")
    x, t, y = (torch.from_numpy(v).cuda() for v in dit_ref.make_inputs("a"))
    before, before_cfg = m(x, t, y), m.forward_with_cfg(x, t, y, 4.0)
    assert m._fn("linear_format")(m._engine) == 0
    w32 = m._fn("workspace_bytes")(m._engine, 4)
    m.set_linear_format("bf16")
    assert m.linear_format == "bf16" and m._engine_sig is None
    half = m(x, t, y)
    assert m._fn("linear_format")(m._engine) == 1
    assert m._fn("workspace_bytes")(m._engine, 4) == w32 - 4 * 36 * 512 * 2
    assert not torch.equal(half, before) and float((half - before).abs().max()) < 0.02
    # the format it already has: nothing is uploaded again, the engine is not finalized again
    calls = []
    fn = m._fn
    m._fn = lambda name: (calls.append(name), fn(name))[1]
    try:
        m.set_linear_format("bf16")
        assert torch.equal(m(x, t, y), half)
        assert "set_weight" not in calls and "finalize" not in calls and "forward" in calls
    finally:
        del m._fn
    m.set_linear_format("fp16")
    h16 = m(x, t, y)
    assert not torch.equal(h16, half) and not torch.equal(h16, before)
    m.set_linear_format("fp32")
    assert torch.equal(m(x, t, y), before)
    assert torch.equal(m.forward_with_cfg(x, t, y, 4.0), before_cfg)


def fresh(name, edit):
    from omnitokenizer_amd.dit import DiT
    w = dit_ref.make_weights(dit_ref.MODELS[name], dit_ref.SEEDS[name])
    edit(w)
    m = DiT(**dit_ref.MODELS[name])
    m.load_state_dict(w, strict=True)
    return m.cuda().eval()


def test_fp16_range_of_weights_and_activations(lib):
    x, t, y = (torch.from_numpy(v).cuda() for v in dit_ref.make_inputs("a"))

    def big_weight(w):
        w["blocks.1.mlp.fc1.weight"][3, 5] = 1e5
    m = fresh("a", big_weight).set_linear_format("fp16")
    with pytest.raises(ValueError, match=r"blocks\.1\.mlp\.fc1\.weight"):
        m(x, t, y)
    with pytest.raises(ValueError, match=r"blocks\.1\.mlp\.fc1\.weight"):   # still refused, not half finalized
        m(x, t, y)
    assert torch.isfinite(m.set_linear_format("bf16")(x, t, y)).all()     # the engine stays usable: bf16 has fp32's range
    assert torch.isfinite(m.set_linear_format("fp32")(x, t, y)).all()

    def big_bias(w):
        w["blocks.0.mlp.fc1.bias"][7] = 7e4
    m = fresh("a", big_bias).set_linear_format("fp16")
    m(x, t, y, check_range=False)                                          # returns: nothing is read back
    m.forward_with_cfg(x, t, y, 2.0, check_range=False)
    with pytest.raises(ValueError, match="fp16"):
        m.check_range()
    m.check_range()                                                        # the bits were cleared
    with pytest.raises(ValueError, match="fp16"):
        m(x, t, y)
    with pytest.raises(ValueError, match="timestep.*fp16"):                # beside the existing bits, whose wording is unchanged
        m(x, torch.full_like(t, 1000), y)
    m.set_linear_format("bf16")
    assert torch.isfinite(m(x, t, y)).all()                                # bf16 never sets the bit


# ---- the sampling loop and batch invariance under bf16 ---------------------------------------------------------------------------------------
def test_loop_fast_and_generic_paths_agree_bf16(lib):
    from omnitokenizer_amd.diffusion import create_diffusion
    m = model("a", "bf16")
    d = create_diffusion("4")
    z = rnd(95, 2, 8, 12, 12).cuda()
    z = torch.cat([z, z], 0)
    y = torch.tensor([1, 7, 10, 10], device="cuda")
    noise = rnd(96, 4, *z.shape).cuda()
    kw = dict(y=y, cfg_scale=4.0)
    fast = d.p_sample_loop(m.forward_with_cfg, z.shape, z, clip_denoised=False, model_kwargs=kw, device="cuda", step_noise=noise)

    def generic(x, t, **k):
        return m.forward_with_cfg(x, t, **k)

    slow = d.p_sample_loop(generic, z.shape, z, clip_denoised=False, model_kwargs=kw, device="cuda", step_noise=noise)
    assert torch.equal(fast, slow) and fast.shape == z.shape and torch.isfinite(fast).all()
    m.set_linear_format("fp32")
    plain = d.p_sample_loop(m.forward_with_cfg, z.shape, z, clip_denoised=False, model_kwargs=kw, device="cuda", step_noise=noise)
    assert not torch.equal(plain, fast)   # the loop ran the format the model held


def test_generate_images_equals_its_body_bf16(lib):
    from omnitokenizer_amd import OmniTokenizer_VQGAN, make_args, synth
    from omnitokenizer_amd.config import OmniTokConfig
    from omnitokenizer_amd.dit import DiT
    from omnitokenizer_amd.diffusion import create_diffusion, generate_images
    from omnitokenizer_amd.frames import pixels_to_frames
    args = make_args(2, resolution=64, use_vae=True)
    vae = OmniTokenizer_VQGAN(args)
    vae.load_state_dict(synth.synth_state_dict(OmniTokConfig.from_args(args), seed=0), strict=True)
    vae = vae.cuda().eval()
    cfg = dict(input_size=8, patch_size=2, in_channels=8, hidden_size=128, depth=1, num_heads=2, num_classes=10)
    dit = DiT(**cfg)
    dit.load_state_dict(dit_ref.make_weights({**dit_ref.MODELS["a"], **cfg}, 5), strict=True)
    dit = dit.cuda().eval().set_linear_format("bf16")
    d = create_diffusion("2")
    labels = torch.tensor([3, 8], device="cuda")
    imgs = generate_images(dit, d, vae, labels, cfg_scale=1.5, seed=11)
    assert imgs.shape == (2, 64, 64, 3) and imgs.dtype == torch.uint8 and dit.linear_format == "bf16"
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)
    z = torch.randn(2, 8, 8, 8, device="cuda", generator=gen)
    z = torch.cat([z, z], 0)
    noise = torch.stack([torch.randn(*z.shape, device="cuda", generator=gen) for _ in range(2)])
    y = torch.cat([labels, torch.full((2,), 10, device="cuda")])
    samples = d.p_sample_loop(dit.forward_with_cfg, z.shape, z, clip_denoised=False, model_kwargs=dict(y=y, cfg_scale=1.5),
                              device="cuda", step_noise=noise)
    assert torch.isfinite(samples).all()
    pixels = vae.decode((samples.chunk(2, dim=0)[0] / 0.18215).contiguous(), is_image=True)
    assert torch.equal(imgs, pixels_to_frames(pixels))


def test_batch_invariance_of_the_forward_bf16(lib):
    m = model("b", "bf16")
    cfg = dit_ref.MODELS["b"]
    x = rnd(91, 5, cfg["in_channels"], cfg["input_size"], cfg["input_size"]).cuda()
    t = torch.tensor([0, 999, 500, 1, 250], device="cuda")
    y = torch.tensor([1, 10, 3, 10, 0], device="cuda")
    full = m(x, t, y)
    assert torch.isfinite(full).all()
    for i in range(5):
        assert torch.equal(m(x[i:i + 1], t[i:i + 1], y[i:i + 1]), full[i:i + 1]), i
