"""The DDIM sampler on the GPU: omnitok_dit_ddim_step alone against fp64 with a derived bar, its null-noise path, the variance half
it must not read, batch invariance across its scalar and float4 forms, the loops against the reference's recorded fp64 trajectories
(tests/golden/ddim_loop.npz), the engine fast path, and generate_images / generate_videos with sample_method="ddim".

The bar of the trajectories is the one of tests/test_gpu_dit.py and tests/test_gpu_latte.py: 4 x the max-abs error of the same loop run
in fp32 by torch on the CPU (tests/ddim_ref.py), recorded beside each trajectory.  Lines starting with DDIM_PARITY carry the measured
figures."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests import ddim_ref, dit_ref, latte_ref
from tests import error_bounds as eb

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "ddim_loop.npz"))
U = eb.U
P = ctypes.c_void_p


@pytest.fixture(scope="module")
def lib():
    from omnitokenizer_amd import build, _lib
    build.build()
    return _lib.load()


def rnd(seed, *shape, scale=1.0):
    return torch.from_numpy((np.random.default_rng(seed).normal(size=shape) * scale).astype(np.float32))


def report(**kw):
    print("DDIM_PARITY " + json.dumps(kw))


def bits(v):
    return v.contiguous().view(torch.int32)


def run_step(lib, mo, x, noise, coef, t, learned, clip, reverse, n_steps=None):
    """One call of the C entry on device tensors; noise may be None (NULL).  Returns (x_out, pred_xstart)."""
    B, C = x.shape[0], x.shape[1]
    HW = x[0, 0].numel()
    sample, xs = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
    rc = lib.omnitok_dit_ddim_step(P(mo.data_ptr()), P(x.data_ptr()), P(noise.data_ptr()) if noise is not None else None,
                                   P(coef.data_ptr()), coef.shape[0] if n_steps is None else n_steps, P(t.data_ptr()), B, C, HW,
                                   int(learned), int(clip), int(reverse), P(sample.data_ptr()), P(xs.data_ptr()),
                                   torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.omnitok_last_error().decode()
    torch.cuda.synchronize()
    return sample, xs


def step_inputs(B, C, H, W, learned, seed=0):
    x, noise = rnd(171 + seed, B, C, H, W, scale=1.5), rnd(172 + seed, B, C, H, W)
    mo = rnd(173 + seed, B, 2 * C if learned else C, H, W)
    return mo, x, noise


def step_bar(k, x, eps, noise, xs_ref, e_ref, reverse):
    """Per-element bounds (xs, out) on the kernel's error against the fp64 evaluation of the same fp32 operands, u = 2^-24 per fp32
    operation, valid whether a multiply-add is fused (one rounding) or not (two):
      xs = k0 x - k1 eps, two products and a subtraction:  e_xs = 3 u (|k0 x| + |k1 eps|); the clamp is 1-Lipschitz
      d  = k0 x - xs: the product (u |k0 x|, absent when fused), the error of xs, the subtraction (u |d|)
      e  = d / k1: the error of d over |k1|, plus the division (u |e|)
      out = xs ka + kb e (+ k4 noise): the errors of xs and e through |ka| and |kb|, then a rounding per product and per addition, each
      of a partial sum no larger than the sum of the terms' magnitudes -- 3 u of it.
    Magnitudes of computed values are taken as the exact ones plus their error bound."""
    a, b = (k[0] * x).abs(), (k[1] * eps).abs()
    e_xs = 3 * U * (a + b)
    d_ref = (k[0] * x - xs_ref).abs()
    e_d = U * a + e_xs + U * (d_ref + U * a + e_xs)
    e_e = e_d / abs(k[1]) + U * (d_ref + e_d) / abs(k[1])
    ka, kb = (abs(k[5]), abs(k[6])) if reverse else (abs(k[2]), abs(k[3]))
    terms = ka * (xs_ref.abs() + e_xs) + kb * (e_ref.abs() + e_e)
    if noise is not None and not reverse:
        terms = terms + abs(k[4]) * noise.abs()
    return e_xs + U * xs_ref.abs(), ka * e_xs + kb * e_e + 3 * U * terms


MODES = [("eta0", 0.0, False), ("eta0.5", 0.5, False), ("eta1", 1.0, False), ("reverse", 0.0, True)]


@pytest.mark.parametrize("mode,eta,reverse", MODES)
@pytest.mark.parametrize("learned", [True, False])
@pytest.mark.parametrize("clip", [True, False])
def test_ddim_step_against_fp64(lib, clip, learned, mode, eta, reverse):
    from omnitokenizer_amd.diffusion import create_ddim_diffusion
    d = create_ddim_diffusion("10", learn_sigma=learned)
    coef = d.ddim_coefficient_table(eta)
    B, C = 3, 4
    t = torch.tensor([0, 4, 9])
    mo, x, noise = step_inputs(B, C, 5, 5, learned)
    if eta == 0 or reverse:
        noise = None   # what the binding passes
    dev = [v.cuda().contiguous() if v is not None else None for v in (mo, x, noise, torch.from_numpy(coef), t)]
    sample, xs = (v.cpu() for v in run_step(lib, *dev, learned, clip, reverse))
    worst, teeth_eps = 0.0, 0.0
    for b in range(B):
        tb = int(t[b])
        k = coef[tb].astype(np.float64)
        sl = slice(b, b + 1)
        nb = noise[sl].double() if noise is not None else None
        ref, ref_xs = ddim_ref.ddim_step(coef[tb], mo[sl].double(), x[sl], nb, learned, clip, reverse)
        eps = mo[sl, :C].double()
        e_ref = (k[0] * x[sl].double() - ref_xs) / k[1]
        bar_xs, bar = step_bar(k, x[sl].double(), eps, nb, ref_xs, e_ref, reverse)
        worst = max(worst, eb.ratio((sample[sl].double() - ref).abs(), bar), eb.ratio((xs[sl].double() - ref_xs).abs(), bar_xs))
        # teeth, in fp64: the model's eps in place of the re-derived one (it differs under clip only) ...
        with_eps = ref_xs * (k[5] if reverse else k[2]) + (k[6] if reverse else k[3]) * eps
        if nb is not None:
            with_eps = with_eps + k[4] * nb
        teeth_eps = max(teeth_eps, eb.ratio((with_eps - ref).abs(), bar))
        # ... and the neighbouring timestep's row
        other = coef[tb + 1 if tb == 0 else tb - 1]
        wrong, wrong_xs = ddim_ref.ddim_step(other, mo[sl].double(), x[sl], nb, learned, clip, reverse)
        assert eb.ratio((wrong - ref).abs(), bar) > 10.0, (tb, "a step with the neighbouring row passes the bar")
        if tb == 0 and not reverse:   # k2 = 1, k3 = k4 = 0
            assert torch.equal(sample[sl], xs[sl])
        if clip:
            assert float(xs[sl].abs().max()) <= 1.0
    if clip:
        assert teeth_eps > 10.0, "a step with the model's eps in place of the re-derived one passes the bar"
    else:
        assert teeth_eps <= 1.0   # without the clamp the re-derived eps is the model's, up to rounding
    print(f"ddim_step {mode} clip {clip} learned {learned}: err / bar {worst:.3f}, teeth (model's eps) {teeth_eps:.1f}")
    report(what="ddim_step", mode=mode, clip=clip, learned=learned, err_over_bar=worst)
    assert worst <= 1.0


def test_null_noise_path(lib):
    from omnitokenizer_amd.diffusion import create_ddim_diffusion
    d = create_ddim_diffusion("10")
    t = torch.tensor([0, 4, 9]).cuda()
    mo, x, noise = (v.cuda() for v in step_inputs(3, 4, 5, 5, True))
    coef0 = torch.from_numpy(d.ddim_coefficient_table(0.0)).cuda()
    for clip in (True, False):
        a = run_step(lib, mo, x, None, coef0, t, True, clip, False)
        b = run_step(lib, mo, x, noise, coef0, t, True, clip, False)      # sigma == 0: a finite draw changes nothing
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.isfinite(a[0]).all()
        nan = torch.full_like(noise, float("nan"))
        r = run_step(lib, mo, x, None, coef0, t, True, clip, True)
        rn = run_step(lib, mo, x, nan, coef0, t, True, clip, True)        # the reverse step does not read it
        assert torch.equal(bits(r[0]), bits(rn[0])) and torch.equal(bits(r[1]), bits(rn[1])) and torch.isfinite(rn[0]).all()
        assert not torch.equal(r[0], a[0])
    # with sigma > 0 the draw is read
    coef5 = torch.from_numpy(d.ddim_coefficient_table(0.5)).cuda()
    with_noise = run_step(lib, mo, x, noise, coef5, t, True, False, False)[0]
    without = run_step(lib, mo, x, None, coef5, t, True, False, False)[0]
    assert torch.equal(with_noise[0], without[0]) and not torch.equal(with_noise[1:], without[1:])   # t == 0: sigma masked


def test_variance_half_is_not_read(lib):
    from omnitokenizer_amd.diffusion import create_ddim_diffusion
    d = create_ddim_diffusion("10")
    t = torch.tensor([0, 4, 9]).cuda()
    mo, x, noise = (v.cuda() for v in step_inputs(3, 4, 5, 5, True))
    poisoned = mo.clone()
    poisoned[:, 4:] = float("nan")
    for eta, reverse in ((0.0, False), (0.5, False), (0.0, True)):
        coef = torch.from_numpy(d.ddim_coefficient_table(eta)).cuda()
        draw = noise if eta > 0 else None
        a = run_step(lib, mo, x, draw, coef, t, True, True, reverse)
        b = run_step(lib, poisoned, x, draw, coef, t, True, True, reverse)
        assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1])) and torch.isfinite(b[0]).all()


# (5, 8, 6, 6) and (5, 4, 5, 5): C HW = 288 and 100, four elements per thread; (5, 3, 5, 5): 75, one per thread, as is every call
# whose pointers are not 16-byte aligned
@pytest.mark.parametrize("shape", [(5, 8, 6, 6), (5, 4, 5, 5), (5, 3, 5, 5)])
def test_batch_invariance_and_the_two_forms(lib, shape):
    from omnitokenizer_amd.diffusion import create_ddim_diffusion
    d = create_ddim_diffusion("10")
    B, C, H, W = shape
    t = torch.tensor([0, 9, 4, 1, 7]).cuda()
    mo, x, noise = (v.cuda() for v in step_inputs(B, C, H, W, True, seed=B * C * H))
    for eta, reverse in ((0.0, False), (0.5, False), (0.0, True)):
        coef = torch.from_numpy(d.ddim_coefficient_table(eta)).cuda()
        draw = noise if eta > 0 else None
        full = run_step(lib, mo, x, draw, coef, t, True, True, reverse)
        for i in range(B):
            one = run_step(lib, mo[i:i + 1], x[i:i + 1], draw[i:i + 1] if draw is not None else None, coef, t[i:i + 1], True, True, reverse)
            assert torch.equal(bits(one[0]), bits(full[0][i:i + 1])) and torch.equal(bits(one[1]), bits(full[1][i:i + 1])), (eta, reverse, i)
        # the same data one float further into its buffers: unaligned, so the one-element form whatever C HW is
        def shifted(v):
            buf = torch.empty(v.numel() + 1, device="cuda")
            buf[1:] = v.reshape(-1)
            return buf[1:].view(v.shape)
        off = run_step(lib, shifted(mo), shifted(x), shifted(draw) if draw is not None else None, coef, t, True, True, reverse)
        assert torch.equal(bits(off[0]), bits(full[0])) and torch.equal(bits(off[1]), bits(full[1])), (eta, reverse)


# ---- the loops against the reference's trajectories ---------------------------------------------------------------------------------
TRAJECTORIES = [(f"dit_eta{e:g}_{'clip' if c else 'noclip'}", e, c) for e in (0.0, 0.5, 1.0) for c in (True, False)] \
    + [(f"latte_eta{e:g}_noclip", e, False) for e in (0.0, 0.5)]


@pytest.mark.parametrize("key,eta,clip", TRAJECTORIES)
def test_ddim_loop_against_the_golden_trajectory(lib, key, eta, clip):
    from omnitokenizer_amd.diffusion import create_ddim_diffusion
    video = key.startswith("latte")
    pre, toy = ("latte_", latte_ref.toy_model) if video else ("", dit_ref.toy_model)
    d = create_ddim_diffusion(str(G["respacing"]))
    x0 = torch.from_numpy(G[pre + "x0"]).float().cuda()
    assert x0.dim() == (5 if video else 4)
    noise = torch.from_numpy(G[pre + "step_noise"]).float().cuda()
    traj = [o["sample"] for o in d.ddim_sample_loop_progressive(toy, tuple(x0.shape), noise=x0, clip_denoised=clip, device="cuda", eta=eta,
                                                                step_noise=noise)]
    assert len(traj) == d.num_timesteps == 10
    err = max(float((s.cpu().double() - torch.from_numpy(G[key][k])).abs().max()) for k, s in enumerate(traj))
    cpu = float(G[f"cpu_fp32_err_{key}"])
    report(model="toy", what=f"ddim_sample_loop_{key}", gpu_max_abs_err=err, cpu_fp32_max_abs_err=cpu, ratio=err / cpu,
           max_abs_ref=float(np.abs(G[key]).max()))
    assert err <= 4 * cpu, f"{key}: GPU error {err:.3e} against 4 x the CPU's fp32 error {cpu:.3e}"
    calls = []

    def draw(k, shape, dev):
        calls.append(k)
        return noise[k]

    last = d.ddim_sample_loop(toy, tuple(x0.shape), noise=x0, clip_denoised=clip, device="cuda", eta=eta, step_noise=draw)
    assert torch.equal(bits(last), bits(traj[-1]))
    assert calls == (list(range(10)) if eta > 0 else [])   # step_noise is consulted only when eta > 0


def test_ddim_reverse_walk_against_the_golden_trajectory(lib):
    from omnitokenizer_amd.diffusion import create_ddim_diffusion
    d = create_ddim_diffusion(str(G["respacing"]))
    x = torch.from_numpy(G["x0"]).float().cuda()
    err = 0.0
    for i in range(d.num_timesteps):
        out = d.ddim_reverse_sample(dit_ref.toy_model, x, torch.full((x.shape[0],), i, device="cuda"), clip_denoised=False)
        x = out["sample"]
        err = max(err, float((x.cpu().double() - torch.from_numpy(G["dit_reverse"][i])).abs().max()))
    cpu = float(G["cpu_fp32_err_dit_reverse"])
    report(model="toy", what="ddim_reverse_sample_walk", gpu_max_abs_err=err, cpu_fp32_max_abs_err=cpu, ratio=err / cpu,
           max_abs_ref=float(np.abs(G["dit_reverse"]).max()))
    assert err <= 4 * cpu, f"reverse walk: GPU error {err:.3e} against 4 x the CPU's fp32 error {cpu:.3e}"


# ---- the engine ------------------------------------------------------------------------------------------------------------------------------
_MODELS = {}


def dit_model():
    if "a" not in _MODELS:
        from omnitokenizer_amd.dit import DiT
        m = DiT(**dit_ref.MODELS["a"])
        m.load_state_dict(dit_ref.make_weights(dit_ref.MODELS["a"], dit_ref.SEEDS["a"]), strict=True)
        _MODELS["a"] = m.cuda().eval()
    return _MODELS["a"]


def test_ddim_loop_with_the_engine_fast_and_generic_paths_agree(lib):
    from omnitokenizer_amd.diffusion import create_ddim_diffusion
    m = dit_model()
    d = create_ddim_diffusion("ddim4")
    assert d.timestep_map == [0, 250, 500, 750]
    z = rnd(195, 2, 8, 12, 12).cuda()
    z = torch.cat([z, z], 0)
    y = torch.tensor([1, 7, 10, 10], device="cuda")
    noise = rnd(196, 4, *z.shape).cuda()
    kw = dict(y=y, cfg_scale=4.0)
    for eta in (0.0, 0.5):
        fast = d.ddim_sample_loop(m.forward_with_cfg, z.shape, z, clip_denoised=False, model_kwargs=kw, device="cuda", eta=eta,
                                  step_noise=noise)
        calls = []

        def generic(x, t, **k):  # any other callable: the same kernel on its output
            calls.append(t.clone())
            return m.forward_with_cfg(x, t, **k)

        slow = d.ddim_sample_loop(generic, z.shape, z, clip_denoised=False, model_kwargs=kw, device="cuda", eta=eta, step_noise=noise)
        assert torch.equal(fast, slow) and fast.shape == z.shape and torch.isfinite(fast).all()
        assert [int(c[0]) for c in calls] == [750, 500, 250, 0]
    # a bad label surfaces after the loop (one read-back), not silently
    with pytest.raises(ValueError, match="label"):
        d.ddim_sample_loop(m.forward_with_cfg, z.shape, z, model_kwargs=dict(y=y + 5, cfg_scale=4.0), device="cuda")


def tiny_vae():
    from omnitokenizer_amd import OmniTokenizer_VQGAN, make_args, synth
    from omnitokenizer_amd.config import OmniTokConfig
    args = make_args(2, resolution=64, use_vae=True)
    vae = OmniTokenizer_VQGAN(args)
    vae.load_state_dict(synth.synth_state_dict(OmniTokConfig.from_args(args), seed=0), strict=True)
    return vae.cuda().eval()


def generator_after(seed, *shapes):
    """The draws of a generator seeded like generate_images' and its state after them."""
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    draws = [torch.randn(*s, device="cuda", generator=gen) for s in shapes]
    return draws, gen.get_state()


def test_generate_images_with_ddim_equals_the_three_calls(lib, monkeypatch):
    from omnitokenizer_amd import diffusion as dm
    from omnitokenizer_amd.dit import DiT
    from omnitokenizer_amd.frames import pixels_to_frames
    vae = tiny_vae()
    cfg = dict(input_size=8, patch_size=2, in_channels=8, hidden_size=128, depth=1, num_heads=2, num_classes=10)
    dit = DiT(**cfg)
    dit.load_state_dict(dit_ref.make_weights({**dit_ref.MODELS["a"], **cfg}, 5), strict=True)
    dit = dit.cuda().eval()
    d = dm.create_ddim_diffusion("ddim2")
    labels = torch.tensor([3, 8], device="cuda")
    y = torch.cat([labels, torch.full((2,), 10, device="cuda")])
    seen = []
    real = torch.randn

    def spy(*a, **k):   # the draws of generate_images' own generator, to count them and to read its state after the call
        if k.get("generator") is not None:
            seen.append(k["generator"])
        return real(*a, **k)

    monkeypatch.setattr(torch, "randn", spy)
    results = {}
    for eta in (0.0, 0.5):
        del seen[:]
        imgs = dm.generate_images(dit, d, vae, labels, cfg_scale=1.5, seed=11, sample_method="ddim", eta=eta)
        assert len(seen) == (1 if eta == 0 else 3) and all(g is seen[0] for g in seen)   # z, then one draw per step
        used = seen[0].get_state()
        assert imgs.shape == (2, 64, 64, 3) and imgs.dtype == torch.uint8
        # by hand: z from the seeded generator, then (eta > 0 only) one draw per step in step order; ddim_sample_loop; decode
        shapes = [(2, 8, 8, 8)] + ([(4, 8, 8, 8)] * 2 if eta > 0 else [])
        (z, *draws), after = generator_after(11, *shapes)
        assert torch.equal(used, after), "the generator is consumed for z only at eta 0, and for one draw per step above"
        z = torch.cat([z, z], 0)
        samples = d.ddim_sample_loop(dit.forward_with_cfg, z.shape, z, clip_denoised=False, model_kwargs=dict(y=y, cfg_scale=1.5),
                                     device="cuda", eta=eta, step_noise=torch.stack(draws) if draws else None)
        assert torch.isfinite(samples).all()
        pixels = vae.decode((samples.chunk(2, dim=0)[0] / 0.18215).contiguous(), is_image=True)
        assert torch.equal(imgs, pixels_to_frames(pixels))
        results[eta] = imgs
    assert not torch.equal(results[0.0], results[0.5])
    assert not torch.equal(results[0.0], dm.generate_images(dit, d, vae, labels, cfg_scale=1.5, seed=12, sample_method="ddim"))
    # the ancestral sampler on the same object is the default, and a plain SpacedDiffusion cannot run DDIM
    ddpm = dm.generate_images(dit, d, vae, labels, cfg_scale=1.5, seed=11)
    assert torch.equal(ddpm, dm.generate_images(dit, d, vae, labels, cfg_scale=1.5, seed=11, sample_method="ddpm", eta=0.7))
    assert not torch.equal(ddpm, results[0.0])
    with pytest.raises(TypeError, match="create_ddim_diffusion"):
        dm.generate_images(dit, dm.create_diffusion("2"), vae, labels, sample_method="ddim")


def test_generate_videos_with_ddim_equals_the_three_calls(lib):
    from omnitokenizer_amd.diffusion import create_ddim_diffusion, generate_videos
    from omnitokenizer_amd.frames import pixels_to_frames
    from omnitokenizer_amd.latte import Latte
    vae = tiny_vae()
    latte = Latte(**latte_ref.MODELS["a"])
    latte.load_state_dict(latte_ref.make_weights(latte_ref.MODELS["a"], latte_ref.SEEDS["a"]), strict=True)
    latte = latte.cuda().eval()
    d = create_ddim_diffusion("ddim2")
    labels = torch.tensor([3, 8], device="cuda")
    y = torch.cat([labels, torch.full((2,), 10, device="cuda")])
    results = {}
    for eta in (0.0, 0.5):
        vids = generate_videos(latte, d, vae, labels, cfg_scale=1.5, seed=11, sample_method="ddim", eta=eta)
        assert vids.shape == (2, 17, 64, 64, 3) and vids.dtype == torch.uint8
        shapes = [(2, 5, 8, 8, 8)] + ([(4, 5, 8, 8, 8)] * 2 if eta > 0 else [])
        (z, *draws), _ = generator_after(11, *shapes)
        z = torch.cat([z, z], 0)
        samples = d.ddim_sample_loop(latte.forward_with_cfg, z.shape, z, clip_denoised=False, model_kwargs=dict(y=y, cfg_scale=1.5),
                                     device="cuda", eta=eta, step_noise=torch.stack(draws) if draws else None)
        assert torch.isfinite(samples).all() and samples.shape == z.shape
        latents = (samples.chunk(2, dim=0)[0] / 0.18215).permute(0, 1, 3, 4, 2).contiguous()   # b f c h w -> b f h w c
        assert torch.equal(vids, pixels_to_frames(vae.decode(latents, is_image=False)))
        results[eta] = vids
    assert not torch.equal(results[0.0], results[0.5])
