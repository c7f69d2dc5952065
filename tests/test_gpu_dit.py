"""DiT denoiser on the GPU: every new kernel alone against fp64, the whole forward and forward_with_cfg against the reference's
recorded fp64 outputs, batch invariance, the sampling loop and generate_images.

The bar of the whole-model checks is not a constant: it is 4 x the max-abs error of tests/dit_ref.py run in fp32 by torch on the
CPU against the same fp64 outputs (recorded per model in the fixture by make_golden_dit.py) -- the orders of magnitude must match,
the summation orders (an MFMA chain against blocked BLAS) do not.  The stand-alone kernels are held to the per-operation bounds
of tests/error_bounds.py where one applies, else to a bound derived in the test.  Lines starting with DIT_PARITY carry the measured
figures (profiles/dit_parity.json)."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import dit_ref
from tests import error_bounds as eb

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
U = eb.U
P = ctypes.c_void_p


@pytest.fixture(scope="module")
def lib():
    from omnitokenizer_amd import build, _lib
    build.build()
    return _lib.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


def ok(lib, rc):
    assert rc == 0, lib.omnitok_last_error().decode()


def rnd(seed, *shape, scale=1.0):
    return torch.from_numpy((np.random.default_rng(seed).normal(size=shape) * scale).astype(np.float32))


def report(**kw):
    print("DIT_PARITY " + json.dumps(kw))


# ---- attention -----------------------------------------------------------------------------------------------------------------
def run_attn(lib, qkv, B, N, heads, hd):
    q = qkv.cuda().contiguous()
    out = torch.full((B * N, heads * hd), float("nan"), device="cuda")
    ok(lib, lib.omnitok_dit_attn(P(q.data_ptr()), B, N, heads, hd, P(out.data_ptr()), stream()))
    torch.cuda.synchronize()
    return out.cpu()


def attn_ref_and_bar(qkv, B, N, heads, hd):
    """fp64 attention of the fp32 operands and softmax_attention_bound's bar: logit error = the fp32 chain of hd products and the
    scale's rounding; P.V adds the keys of whole 32-key tiles plus one rescale per tile; l the same."""
    x = qkv.double().reshape(B, N, 3, heads, hd).permute(2, 0, 3, 1, 4)
    q, k, v = x[0], x[1], x[2]
    scale = float(np.float32(1.0 / math.sqrt(hd)))
    s = (q @ k.transpose(-1, -2)) * scale
    tiles = (N + 31) // 32
    ds = (eb.gamma(hd) * (q.abs() @ k.abs().transpose(-1, -2)) * scale + 2 * U * s.abs()).amax(-1, keepdim=True)
    bar = eb.softmax_attention_bound(s, v, ds, n_pv=32 * tiles + tiles, n_l=32 * tiles + tiles)
    ref = torch.softmax(s, -1) @ v
    return ref.transpose(1, 2).reshape(B * N, heads * hd), bar.transpose(1, 2).reshape(B * N, heads * hd)


@pytest.mark.parametrize("bh", [1, 6])
@pytest.mark.parametrize("hd", [64, 72])
@pytest.mark.parametrize("N", [16, 32, 36, 81, 256])
def test_attention_against_fp64(lib, N, hd, bh):
    B, heads = (1, 1) if bh == 1 else (3, 2)
    qkv = rnd(1000 + N + hd + bh, B * N, 3 * heads * hd)
    out = run_attn(lib, qkv, B, N, heads, hd)
    ref, bar = attn_ref_and_bar(qkv, B, N, heads, hd)
    err = (out.double() - ref).abs()
    r = eb.ratio(err, bar)
    print(f"attn N {N} hd {hd} BH {bh}: max err {float(err.max()):.2e}, err / bar {r:.3f}")
    assert torch.isfinite(out).all() and r <= 1.0


@pytest.mark.parametrize("hd", [64, 72])
def test_attention_row_of_large_logits(lib, hd):
    """One query and a few keys 30 x larger: logits in the hundreds, where the softmax only survives anchored at the running max --
    and the max moves from tile to tile (the large keys sit in the second and the last tile)."""
    B, heads, N = 1, 2, 81
    qkv = rnd(7 + hd, B * N, 3 * heads * hd).reshape(N, 3, heads, hd)
    qkv[5, 0] *= 30.0
    qkv[40, 1] *= 30.0
    qkv[80, 1] *= 30.0
    qkv = qkv.reshape(N, -1)
    out = run_attn(lib, qkv, B, N, heads, hd)
    ref, bar = attn_ref_and_bar(qkv, B, N, heads, hd)
    s_max = float((qkv.double().reshape(N, 3, heads, hd)[:, 0].transpose(0, 1) @
                   qkv.double().reshape(N, 3, heads, hd)[:, 1].permute(1, 2, 0)).abs().max() / math.sqrt(hd))
    assert s_max > 100.0
    err = (out.double() - ref).abs()
    print(f"large logits hd {hd}: max |s| {s_max:.0f}, max err {float(err.max()):.2e}, err / bar {eb.ratio(err, bar):.3f}")
    assert torch.isfinite(out).all() and eb.ratio(err, bar) <= 1.0


def test_attention_hd72_padding_does_not_read_the_neighbouring_head(lib):
    """head_dim 72: the third 32-dim block of O is one quarter live.  What lies behind column 71 of head 0's V in memory is head
    1's V -- NaN here.  Head 0's output must be the value it has with a finite neighbour, bit for bit."""
    B, heads, N, hd = 2, 2, 36, 72
    qkv = rnd(31, B * N, 3 * heads * hd)
    clean = run_attn(lib, qkv, B, N, heads, hd)
    poisoned = qkv.clone().reshape(B * N, 3, heads, hd)
    poisoned[:, 2, 1] = float("nan")
    out = run_attn(lib, poisoned.reshape(B * N, -1), B, N, heads, hd)
    assert torch.isfinite(out[:, :hd]).all()
    assert torch.equal(out[:, :hd], clean[:, :hd])
    assert torch.isnan(out[:, hd:]).all()  # head 1 itself multiplies the NaNs


# ---- the element-wise kernels, B = 3 so that rows are no multiple of any tile ----------------------------------------------------
def test_ln_modulate_against_fp64(lib):
    B, n_tok, D, ld = 3, 5, 160, 3 * 160 + 32
    x = rnd(41, B * n_tok, D, scale=2.0) + 0.5
    x[7] = 0.75  # a constant row: variance 0
    mod = rnd(42, B, ld, scale=0.3)
    shift, scale = mod[:, 32:32 + D], mod[:, 32 + D:32 + 2 * D]
    xd, md = x.cuda(), mod.cuda()
    out = torch.empty_like(xd)
    ok(lib, lib.omnitok_dit_ln_modulate(P(xd.data_ptr()), P(md.data_ptr() + 32 * 4), P(md.data_ptr() + (32 + D) * 4), ld, B * n_tok,
                                        n_tok, D, P(out.data_ptr()), stream()))
    out = out.cpu()
    g = (1.0 + scale.double()).repeat_interleave(n_tok, 0)
    b = shift.double().repeat_interleave(n_tok, 0)
    xx = x.double()
    mu = xx.mean(-1, keepdim=True)
    ref = (xx - mu) / torch.sqrt(((xx - mu) ** 2).mean(-1, keepdim=True) + 1e-6) * g + b
    bar, _, _ = eb.layernorm_bound(xx, g, b, eps=1e-6)
    bar = bar + 2 * U * ref.abs() + 2 * U * (ref - b).abs()  # the rounding of 1 + scale, and the fma's
    err = (out.double() - ref).abs()
    print(f"ln_modulate: max err {float(err.max()):.2e}, err / bar {eb.ratio(err, bar):.3f}, constant row {out[7, :3].tolist()}")
    assert torch.isfinite(out).all() and eb.ratio(err, bar) <= 1.0
    assert torch.equal(out[7], shift[7 // n_tok])  # (x - mean) is exactly 0: the row is the shift


def test_gate_residual_and_gelu_against_fp64(lib):
    B, n_tok, D, ld = 3, 7, 96, 200
    x, y, gate = rnd(51, B * n_tok, D), rnd(52, B * n_tok, D), rnd(53, B, ld)
    xd, yd, gd = x.cuda(), y.cuda(), gate.cuda()
    ok(lib, lib.omnitok_dit_gate_residual(P(xd.data_ptr()), P(yd.data_ptr()), P(gd.data_ptr() + 8 * 4), ld, B * n_tok, n_tok, D, stream()))
    g = gate[:, 8:8 + D].double().repeat_interleave(n_tok, 0)
    ref = x.double() + g * y.double()
    err = (xd.cpu().double() - ref).abs()
    bar = U * ref.abs() * (1 + U)  # ONE rounding: the gate is fused into the read of y as an fma
    assert eb.ratio(err, bar) <= 1.0, float(err.max())
    # GELU, tanh form: the argument of tanh carries 4 roundings (|x tanh'(x)| <= 0.45), tanhf 4 ulp of its value, then 1 + tanh and
    # two products: 0.5 |v| (4 * 0.45 u + 8 u + 2 u) + 3 u |y|
    v = torch.cat([rnd(54, 1000, scale=3.0), torch.tensor([0.0, -0.0, 20.0, -20.0, 1e-20, -9.0])])
    vd = v.cuda()
    ok(lib, lib.omnitok_dit_gelu_tanh(P(vd.data_ptr()), v.numel(), stream()))
    vv = v.double()
    ref = 0.5 * vv * (1 + torch.tanh(math.sqrt(2 / math.pi) * (vv + 0.044715 * vv ** 3)))
    assert torch.allclose(ref.float(), torch.nn.functional.gelu(v, approximate="tanh"), atol=1e-6)
    err = (vd.cpu().double() - ref).abs()
    bar = 0.5 * vv.abs() * 12 * U + 3 * U * ref.abs()
    print(f"gelu_tanh: max err {float(err.max()):.2e}, err / bar {eb.ratio(err, bar):.3f}")
    assert eb.ratio(err, bar) <= 1.0


@pytest.mark.parametrize("C", [4, 8])  # K = p p C = 16 and 32
def test_patch_embed_and_unpatchify_against_fp64(lib, C):
    B, H, p, D = 3, 6, 2, 96
    N = (H // p) ** 2
    x, w, bias, pos = rnd(61 + C, B, C, H, H), rnd(62, D, C, p, p, scale=0.3), rnd(63, D, scale=0.1), rnd(64, N, D, scale=0.1)
    xd, wd, bd, pd = x.cuda(), w.cuda(), bias.cuda(), pos.cuda()
    out = torch.empty(B * N, D, device="cuda")
    ok(lib, lib.omnitok_dit_patch_embed(P(xd.data_ptr()), B, P(wd.data_ptr()), P(bd.data_ptr()), P(pd.data_ptr()), B, C, H, p, D,
                                        P(out.data_ptr()), stream()))
    patches = torch.nn.functional.unfold(x.double(), p, stride=p).transpose(1, 2).reshape(B * N, C * p * p)  # (c, i, j) order
    wm = w.double().reshape(D, -1)
    acc = patches @ wm.t()
    ref = acc + bias.double() + pos.double().repeat(B, 1)
    bar = eb.dot_bound(patches, wm, C * p * p, "fp32") + eb.add_bound(acc, bias.double().expand_as(acc), pos.double().repeat(B, 1)) \
        + 2 * U * ref.abs()
    err = (out.cpu().double() - ref).abs()
    print(f"patch_embed K {C * p * p}: max err {float(err.max()):.2e}, err / bar {eb.ratio(err, bar):.3f}")
    assert eb.ratio(err, bar) <= 1.0
    # x_batch < B: sample b reads x[b % x_batch] (the CFG wrapper's cat([half, half]))
    out2 = torch.empty((B + 1) * N, D, device="cuda")
    ok(lib, lib.omnitok_dit_patch_embed(P(xd.data_ptr()), 2, P(wd.data_ptr()), P(bd.data_ptr()), P(pd.data_ptr()), 4, C, H, p, D,
                                        P(out2.data_ptr()), stream()))
    assert torch.equal(out2[2 * N:], out2[:2 * N]) and torch.equal(out2[:2 * N], out[:2 * N])
    # unpatchify is a permutation: exact
    cout = 2 * C
    lin = rnd(65, B * N, p * p * cout)
    ld = lin.cuda()
    img = torch.empty(B, cout, H, H, device="cuda")
    ok(lib, lib.omnitok_dit_unpatchify(P(ld.data_ptr()), B, N, p, cout, P(img.data_ptr()), stream()))
    assert torch.equal(img.cpu(), dit_ref.unpatchify(lin.reshape(B, N, -1), p, cout))


@pytest.mark.parametrize("learned", [True, False])
@pytest.mark.parametrize("clip", [True, False])
def test_p_sample_against_fp64(lib, clip, learned):
    from omnitokenizer_amd.diffusion import create_diffusion
    d = create_diffusion("10", learn_sigma=learned)
    coef = d.coefficient_table()
    B, C, HW = 3, 4, 25
    t = torch.tensor([0, 4, 9])  # t = 0: no noise
    x, noise = rnd(71, B, C, 5, 5, scale=1.5), rnd(72, B, C, 5, 5)
    mo = rnd(73, B, 2 * C if learned else C, 5, 5)
    if learned:  # frac at both ends of [0, 1], and beyond neither
        mo[:, C:] = mo[:, C:].clamp(-1, 1)
        mo[:, C, 0, :] = -1.0
        mo[:, C, 1, :] = 1.0
    dev = [v.cuda().contiguous() for v in (mo, x, noise, torch.from_numpy(coef), t)]
    sample, xs = torch.empty(B, C, 5, 5, device="cuda"), torch.empty(B, C, 5, 5, device="cuda")
    ok(lib, lib.omnitok_dit_p_sample(P(dev[0].data_ptr()), P(dev[1].data_ptr()), P(dev[2].data_ptr()), P(dev[3].data_ptr()),
                                     d.num_timesteps, P(dev[4].data_ptr()), B, C, HW, int(learned), int(clip), P(sample.data_ptr()),
                                     P(xs.data_ptr()), stream()))
    worst = 0.0
    for b in range(B):
        k = coef[int(t[b])].astype(np.float64)
        ref, ref_xs = dit_ref.p_sample(coef[int(t[b])], mo[b:b + 1].double(), x[b:b + 1], noise[b:b + 1], learned, clip)
        eps = mo[b:b + 1, :C].double()
        frac = (mo[b:b + 1, C:].double() + 1) / 2 if learned else None
        logvar = frac * k[5] + (1 - frac) * k[4] if learned else torch.full_like(eps, k[6])
        # pred_xstart: two products and a subtraction; mean: the same on top of it (clamp is 1-Lipschitz); the noise term: frac and
        # logvar carry 5 roundings of values up to |min_log|, 0.5 logvar enters expf (2 ulp) -- relative (6 |logvar| + 6) u -- then
        # two products and the final add
        e_xs = 3 * U * (abs(k[0]) * x[b:b + 1].double().abs() + abs(k[1]) * eps.abs())
        sigma = k[7] * torch.exp(0.5 * logvar) * noise[b:b + 1].double().abs()
        bar = abs(k[2]) * e_xs + 3 * U * (abs(k[2]) * ref_xs.abs() + abs(k[3]) * x[b:b + 1].double().abs()) \
            + sigma * (6 * max(abs(k[4]), abs(k[5]), abs(k[6])) + 8) * U + 2 * U * ref.abs()
        worst = max(worst, eb.ratio((sample[b:b + 1].cpu().double() - ref).abs(), bar),
                    eb.ratio((xs[b:b + 1].cpu().double() - ref_xs).abs(), e_xs + U * ref_xs.abs()))
        if int(t[b]) == 0:  # no noise at t = 0: the sample is the posterior mean whatever the draw
            assert torch.allclose(sample[b:b + 1].cpu().double(), k[2] * ref_xs + k[3] * x[b:b + 1].double(), rtol=1e-6, atol=1e-7)
        if clip:
            assert float(xs[b].abs().max()) <= 1.0
    print(f"p_sample clip {clip} learned {learned}: err / bar {worst:.3f}")
    assert worst <= 1.0


# ---- the whole model -------------------------------------------------------------------------------------------------------------------
_MODELS = {}


def model(name):
    if name not in _MODELS:
        from omnitokenizer_amd.dit import DiT
        m = DiT(**dit_ref.MODELS[name])
        m.load_state_dict(dit_ref.make_weights(dit_ref.MODELS[name], dit_ref.SEEDS[name]), strict=True)
        _MODELS[name] = m.cuda().eval()
    return _MODELS[name]


@pytest.mark.parametrize("name", ["a", "b"])
def test_forward_and_cfg_against_the_reference(lib, name):
    g = np.load(os.path.join(GOLDEN, f"dit_model_{name}.npz"))
    m = model(name)
    x, t, y = (torch.from_numpy(g[k]).cuda() for k in ("x", "t", "y"))
    for key, out in (("forward", m(x, t, y)), ("forward_with_cfg", m.forward_with_cfg(x, t, y, float(g["cfg_scale"])))):
        ref = torch.from_numpy(g[key])
        err = float((out.cpu().double() - ref).abs().max())
        cpu = float(g[f"cpu_fp32_err_{key}"])
        report(model=name, what=key, gpu_max_abs_err=err, cpu_fp32_max_abs_err=cpu, ratio=err / cpu, max_abs_ref=float(ref.abs().max()))
        assert out.shape == ref.shape and out.dtype == torch.float32
        assert err <= 4 * cpu, f"{name} {key}: GPU error {err:.3e} against 4 x the CPU's fp32 error {cpu:.3e}"
    out = m.forward_with_cfg(x, t, y, float(g["cfg_scale"]))
    h = x.shape[0] // 2
    assert torch.equal(out[:h, :3], out[h:, :3])                    # both halves get the same guided eps ...
    plain = m(torch.cat([x[:h], x[:h]]), t, y)
    assert torch.equal(out[:, 3:], plain[:, 3:])                    # ... and every other channel passes through
    assert not torch.equal(out[:h, 3:], out[h:, 3:])


def test_forward_range_errors(lib):
    m = model("a")
    x = torch.zeros(2, 8, 12, 12, device="cuda")
    y = torch.zeros(2, dtype=torch.long, device="cuda")
    with pytest.raises(ValueError, match="timestep"):
        m(x, torch.tensor([0, 1000], device="cuda"), y)
    with pytest.raises(ValueError, match="label"):
        m(x, torch.tensor([0, 999], device="cuda"), torch.tensor([0, 11], device="cuda"))
    m(x, torch.tensor([0, 999], device="cuda"), torch.tensor([0, 10], device="cuda"))  # the null row is in range
    with pytest.raises(ValueError, match="even"):
        m.forward_with_cfg(x[:1], torch.zeros(1, dtype=torch.long, device="cuda"), y[:1], 2.0)


# ---- batch invariance: sample i of a B = 5 call equals the B = 1 call bit for bit ----------------------------------------------------------
def test_batch_invariance_of_the_new_kernels(lib):
    B, N, heads = 5, 36, 2
    for hd in (64, 72):
        qkv = rnd(81 + hd, B * N, 3 * heads * hd)
        full = run_attn(lib, qkv, B, N, heads, hd)
        for i in range(B):
            assert torch.equal(run_attn(lib, qkv[i * N:(i + 1) * N], 1, N, heads, hd), full[i * N:(i + 1) * N]), (hd, i)
    D, ld = 160, 512
    x, y, mod = rnd(82, B * N, D).cuda(), rnd(83, B * N, D).cuda(), rnd(84, B, ld).cuda()
    ln = torch.empty_like(x)
    ok(lib, lib.omnitok_dit_ln_modulate(P(x.data_ptr()), P(mod.data_ptr()), P(mod.data_ptr() + D * 4), ld, B * N, N, D, P(ln.data_ptr()),
                                        stream()))
    gr = x.clone()
    ok(lib, lib.omnitok_dit_gate_residual(P(gr.data_ptr()), P(y.data_ptr()), P(mod.data_ptr() + 2 * D * 4), ld, B * N, N, D, stream()))
    C, H, p = 4, 12, 2
    img, w, bias, pos = rnd(85, B, C, H, H).cuda(), rnd(86, D, C, p, p).cuda(), rnd(87, D).cuda(), rnd(88, N, D).cuda()
    pe = torch.empty(B * N, D, device="cuda")
    ok(lib, lib.omnitok_dit_patch_embed(P(img.data_ptr()), B, P(w.data_ptr()), P(bias.data_ptr()), P(pos.data_ptr()), B, C, H, p, D,
                                        P(pe.data_ptr()), stream()))
    for i in range(B):
        rows = slice(i * N, (i + 1) * N)
        xi, yi, mi, ii = x[rows].contiguous(), y[rows].contiguous(), mod[i:i + 1].contiguous(), img[i:i + 1].contiguous()
        o = torch.empty_like(xi)
        ok(lib, lib.omnitok_dit_ln_modulate(P(xi.data_ptr()), P(mi.data_ptr()), P(mi.data_ptr() + D * 4), ld, N, N, D, P(o.data_ptr()),
                                            stream()))
        assert torch.equal(o, ln[rows]), i
        ok(lib, lib.omnitok_dit_gate_residual(P(xi.data_ptr()), P(yi.data_ptr()), P(mi.data_ptr() + 2 * D * 4), ld, N, N, D, stream()))
        assert torch.equal(xi, gr[rows]), i
        o = torch.empty(N, D, device="cuda")
        ok(lib, lib.omnitok_dit_patch_embed(P(ii.data_ptr()), 1, P(w.data_ptr()), P(bias.data_ptr()), P(pos.data_ptr()), 1, C, H, p, D,
                                            P(o.data_ptr()), stream()))
        assert torch.equal(o, pe[rows]), i


@pytest.mark.parametrize("name", ["a", "b"])
def test_batch_invariance_of_the_forward(lib, name):
    m = model(name)
    cfg = dit_ref.MODELS[name]
    x = rnd(91, 5, cfg["in_channels"], cfg["input_size"], cfg["input_size"]).cuda()
    t = torch.tensor([0, 999, 500, 1, 250], device="cuda")
    y = torch.tensor([1, 10, 3, 10, 0], device="cuda")
    full = m(x, t, y)
    for i in range(5):
        assert torch.equal(m(x[i:i + 1], t[i:i + 1], y[i:i + 1]), full[i:i + 1]), (name, i)


# ---- the sampling loop -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,clip", [("clip", True), ("noclip", False)])
def test_p_sample_loop_against_the_golden_trajectory(lib, tag, clip):
    from omnitokenizer_amd.diffusion import create_diffusion
    g = np.load(os.path.join(GOLDEN, "dit_loop.npz"))
    d = create_diffusion(str(g["respacing"]))
    x0 = torch.from_numpy(g["x0"]).float().cuda()
    noise = torch.from_numpy(g["step_noise"]).float().cuda()
    traj = [o["sample"] for o in d.p_sample_loop_progressive(dit_ref.toy_model, tuple(x0.shape), noise=x0, clip_denoised=clip,
                                                             device="cuda", step_noise=noise)]
    assert len(traj) == d.num_timesteps == 10
    err = max(float((s.cpu().double() - torch.from_numpy(g[f"trajectory_{tag}"][k])).abs().max()) for k, s in enumerate(traj))
    cpu = float(g[f"cpu_fp32_err_{tag}"])
    report(model="toy", what=f"p_sample_loop_{tag}", gpu_max_abs_err=err, cpu_fp32_max_abs_err=cpu, ratio=err / cpu,
           max_abs_ref=float(np.abs(g[f"trajectory_{tag}"]).max()))
    assert err <= 4 * cpu
    last = d.p_sample_loop(dit_ref.toy_model, tuple(x0.shape), noise=x0, clip_denoised=clip, device="cuda",
                           step_noise=lambda k, shape, dev: noise[k])
    assert torch.equal(last, traj[-1])


def test_loop_with_the_engine_fast_and_generic_paths_agree(lib):
    from omnitokenizer_amd.diffusion import create_diffusion
    m = model("a")
    d = create_diffusion("4")
    n = 2
    z = rnd(95, n, 8, 12, 12).cuda()
    z = torch.cat([z, z], 0)
    y = torch.tensor([1, 7, 10, 10], device="cuda")
    noise = rnd(96, 4, *z.shape).cuda()
    kw = dict(y=y, cfg_scale=4.0)
    fast = d.p_sample_loop(m.forward_with_cfg, z.shape, z, clip_denoised=False, model_kwargs=kw, device="cuda", step_noise=noise)
    calls = []

    def generic(x, t, **k):  # any other callable: the same p_sample kernel on its output
        calls.append(t.clone())
        return m.forward_with_cfg(x, t, **k)

    slow = d.p_sample_loop(generic, z.shape, z, clip_denoised=False, model_kwargs=kw, device="cuda", step_noise=noise)
    assert torch.equal(fast, slow) and fast.shape == z.shape and torch.isfinite(fast).all()
    assert [int(c[0]) for c in calls] == [d.timestep_map[i] for i in (3, 2, 1, 0)] == [999, 666, 333, 0]
    # a bad label surfaces after the loop (one read-back), not silently
    with pytest.raises(ValueError, match="label"):
        d.p_sample_loop(m.forward_with_cfg, z.shape, z, model_kwargs=dict(y=y + 5, cfg_scale=4.0), device="cuda", step_noise=noise)


def test_generate_images_equals_the_three_calls(lib):
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
    dit = dit.cuda().eval()
    d = create_diffusion("2")
    labels = torch.tensor([3, 8], device="cuda")
    imgs = generate_images(dit, d, vae, labels, cfg_scale=1.5, seed=11)
    assert imgs.shape == (2, 64, 64, 3) and imgs.dtype == torch.uint8
    # by hand: the draws of the same generator, p_sample_loop, decode, pixels_to_frames
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
    assert torch.isfinite(pixels).all()
    assert torch.equal(imgs, pixels_to_frames(pixels))
    assert torch.equal(imgs, generate_images(dit, d, vae, labels, cfg_scale=1.5, seed=11))
    assert not torch.equal(imgs, generate_images(dit, d, vae, labels, cfg_scale=1.5, seed=12))
