"""Latte video denoiser on the GPU: the temporal-attention kernel and the two small operators alone against fp64, the whole forward
and forward_with_cfg against the reference's recorded fp64 outputs, batch and stride invariance, the 5-D sampling loop and
generate_videos.

The bar of the whole-model checks is 4 x the max-abs error of tests/latte_ref.py run in fp32 by torch on the CPU against the same
fp64 outputs (recorded per model in the fixture by make_golden_latte.py): the DiT tests' margin, taken over from them.  The
temporal attention is held to tests/error_bounds.py softmax_attention_bound with the term counts csrc/latte_attn.hip states for
its sums; the operators to bounds derived in the test.  Lines starting with LATTE_PARITY carry the measured figures."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import dit_ref, latte_ref
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
    print("LATTE_PARITY " + json.dumps(kw))


# ---- temporal attention --------------------------------------------------------------------------------------------------------
def run_tattn(lib, qkv, B, F, N, heads, hd):
    q = qkv.cuda().contiguous()
    out = torch.full((B * F * N, heads * hd), float("nan"), device="cuda")
    ok(lib, lib.omnitok_latte_attn_temporal(P(q.data_ptr()), B, F, N, heads, hd, P(out.data_ptr()), stream()))
    torch.cuda.synchronize()
    return out.cpu()


def tattn_ref_and_bar(qkv, B, F, N, heads, hd):
    """fp64 attention over the frames of every (b, n, head) of the fp32 operands, and softmax_attention_bound's bar with the counts of
    csrc/latte_attn.hip: a logit is four fmaf chains of hd / 4 links and two adds (hd / 4 + 2 roundings on a product's path), then
    the product with the once-rounded scale (2 u |s|); P.V is one chain over the F frames (n_pv = F), l the F - 1 adds of F terms."""
    x = qkv.double().reshape(B, F, N, 3, heads, hd).permute(3, 0, 2, 4, 1, 5)   # [3, B, N, heads, F, hd]
    q, k, v = x[0], x[1], x[2]
    scale = float(np.float32(1.0 / math.sqrt(hd)))
    s = (q @ k.transpose(-1, -2)) * scale
    ds = (eb.gamma(hd // 4 + 2) * (q.abs() @ k.abs().transpose(-1, -2)) * scale + 2 * U * s.abs()).amax(-1, keepdim=True)
    bar = eb.softmax_attention_bound(s, v, ds, n_pv=F, n_l=F - 1)
    ref = torch.softmax(s, -1) @ v                                              # [B, N, heads, F, hd]

    def rows(t):
        return t.permute(0, 3, 1, 2, 4).reshape(B * F * N, heads * hd)
    return rows(ref), rows(bar)


@pytest.mark.parametrize("bnh", [(1, 1, 1), (2, 9, 3)])
@pytest.mark.parametrize("hd", [64, 72])
@pytest.mark.parametrize("F", [1, 2, 5, 16, 17, 32])
def test_temporal_attention_against_fp64(lib, F, hd, bnh):
    B, N, heads = bnh
    qkv = rnd(2000 + 10 * F + hd + B, B * F * N, 3 * heads * hd)
    out = run_tattn(lib, qkv, B, F, N, heads, hd)
    ref, bar = tattn_ref_and_bar(qkv, B, F, N, heads, hd)
    err = (out.double() - ref).abs()
    r = eb.ratio(err, bar)
    print(f"temporal attn F {F} hd {hd} (B, N, heads) {bnh}: max err {float(err.max()):.2e}, err / bar {r:.3f}")
    assert torch.isfinite(out).all() and r <= 1.0
    if F == 1:  # one frame: the softmax weight is exactly 1 and the output is V
        assert torch.equal(out, qkv.reshape(B * N, 3, heads * hd)[:, 2])


@pytest.mark.parametrize("hd", [64, 72])
def test_temporal_attention_row_of_large_logits(lib, hd):
    """One query frame and two key frames 30 x larger: logits in the hundreds, where the softmax only survives anchored at the row
    maximum."""
    B, F, N, heads = 1, 17, 2, 2
    qkv = rnd(9 + hd, B * F * N, 3 * heads * hd).reshape(F, N, 3, heads, hd)
    qkv[5, 1, 0] *= 30.0
    qkv[3, 1, 1] *= 30.0
    qkv[16, 1, 1] *= 30.0
    qkv = qkv.reshape(F * N, -1)
    out = run_tattn(lib, qkv, B, F, N, heads, hd)
    ref, bar = tattn_ref_and_bar(qkv, B, F, N, heads, hd)
    x = qkv.double().reshape(F, N, 3, heads, hd)
    s_max = float(torch.einsum("fnhd,gnhd->nhfg", x[:, :, 0], x[:, :, 1]).abs().max() / math.sqrt(hd))
    assert s_max > 100.0
    err = (out.double() - ref).abs()
    print(f"large logits hd {hd}: max |s| {s_max:.0f}, max err {float(err.max()):.2e}, err / bar {eb.ratio(err, bar):.3f}")
    assert torch.isfinite(out).all() and eb.ratio(err, bar) <= 1.0


def test_temporal_attention_hd72_does_not_read_the_neighbouring_head(lib):
    """head_dim 72 is no multiple of the 64 lanes: what lies behind column 71 of head 0 in memory is head 1 -- NaN here, q, k and v.
    Head 0's output must be the value it has with a finite neighbour, bit for bit; so must the last head's, whose row ends there."""
    B, F, N, heads, hd = 2, 5, 4, 3, 72
    qkv = rnd(33, B * F * N, 3 * heads * hd)
    clean = run_tattn(lib, qkv, B, F, N, heads, hd)
    poisoned = qkv.clone().reshape(B * F * N, 3, heads, hd)
    poisoned[:, :, 1] = float("nan")
    out = run_tattn(lib, poisoned.reshape(B * F * N, -1), B, F, N, heads, hd)
    for h in (0, 2):
        cols = slice(h * hd, (h + 1) * hd)
        assert torch.isfinite(out[:, cols]).all() and torch.equal(out[:, cols], clean[:, cols]), h
    assert torch.isnan(out[:, hd:2 * hd]).all()  # head 1 itself multiplies the NaNs


@pytest.mark.parametrize("hd", [64, 72])
@pytest.mark.parametrize("F", [5, 16])
def test_temporal_attention_stride_and_batch_invariance(lib, F, hd):
    """Bit for bit: the (B, N, heads) = (2, 9, 3) result equals the kernel run with N = 1 on each position's gathered F rows (the
    layout the reference rearranges into), and sample b of a B = 3 call equals the call with that sample alone."""
    B, N, heads = 2, 9, 3
    qkv = rnd(4000 + F + hd, B * F * N, 3 * heads * hd)
    full = run_tattn(lib, qkv, B, F, N, heads, hd).reshape(B, F, N, heads * hd)
    q4 = qkv.reshape(B, F, N, -1)
    for b in range(B):
        for n in range(N):
            alone = run_tattn(lib, q4[b, :, n].contiguous(), 1, F, 1, heads, hd)
            assert torch.equal(alone, full[b, :, n]), (b, n)
    # all positions at once in the rearranged layout '(b t) f d'
    gathered = q4.transpose(1, 2).reshape(B * N * F, -1)
    assert torch.equal(run_tattn(lib, gathered, B * N, F, 1, heads, hd).reshape(B, N, F, -1).transpose(1, 2), full)
    B3 = 3
    qkv3 = rnd(4100 + F + hd, B3 * F * N, 3 * heads * hd)
    full3 = run_tattn(lib, qkv3, B3, F, N, heads, hd)
    for b in range(B3):
        rows = slice(b * F * N, (b + 1) * F * N)
        assert torch.equal(run_tattn(lib, qkv3[rows], 1, F, N, heads, hd), full3[rows]), b


def test_temporal_attention_refuses_bad_shapes_without_a_launch(lib):
    qkv = rnd(5, 33 * 2, 3 * 80).cuda()
    out = torch.full((33 * 2, 80), float("nan"), device="cuda")
    for F, hd, word in ((33, 64, "frames"), (0, 64, "frames"), (5, 80, "head_dim"), (5, 96, "head_dim")):
        assert lib.omnitok_latte_attn_temporal(P(qkv.data_ptr()), 1, F, 2, 1, hd, P(out.data_ptr()), stream()) == -1
        assert word in lib.omnitok_last_error().decode()
    torch.cuda.synchronize()
    assert torch.isnan(out).all()  # nothing ran


# ---- the operators ---------------------------------------------------------------------------------------------------------------
def test_add_temp_embed_against_fp64(lib):
    B, F, N, D = 3, 5, 7, 96
    x, temp = rnd(41, B * F * N, D, scale=2.0), rnd(42, F, D)
    xd, td = x.cuda(), temp.cuda()
    ok(lib, lib.omnitok_latte_add_temp_embed(P(xd.data_ptr()), P(td.data_ptr()), B, F, N, D, stream()))
    ref = (x.double().reshape(B, F, N, D) + temp.double()[None, :, None, :]).reshape(B * F * N, D)
    err = (xd.cpu().double() - ref).abs()
    assert eb.ratio(err, U * ref.abs()) <= 1.0, float(err.max())   # exactly one rounding
    assert torch.equal(xd.cpu(), (x.reshape(B, F, N, D) + temp[None, :, None, :]).reshape(B * F * N, D))  # i.e. the fp32 sum


@pytest.mark.parametrize("channels,cout", [(4, 8), (3, 8), (4, 2)])
def test_cfg_blend_with_a_channel_count(lib, channels, cout):
    """latte.py:399-403 on B F = 6 images: channels [0, channels) of both halves become uncond + s (cond - uncond) (three fp32
    roundings: the difference, the product, the sum), every other channel keeps its bits."""
    images, HW, s = 6, 25, 7.0
    x = rnd(51 + channels + cout, images, cout, HW)
    xd = x.cuda()
    ok(lib, lib.omnitok_latte_cfg_blend(P(xd.data_ptr()), images, cout, channels, HW, s, stream()))
    out = xd.cpu()
    nc, h = min(channels, cout), images // 2
    assert torch.equal(out[:h, :nc], out[h:, :nc])
    assert torch.equal(out[:, nc:], x[:, nc:])
    cond, uncond = x[:h, :nc].double(), x[h:, :nc].double()
    ref = uncond + s * (cond - uncond)
    bar = (2 * U * (s * (cond - uncond)).abs() + U * ref.abs()) * (1 + 4 * U)
    assert eb.ratio((out[:h, :nc].double() - ref).abs(), bar) <= 1.0
    assert torch.equal(out[:h, :nc], x[h:, :nc] + s * (x[:h, :nc] - x[h:, :nc]))  # torch's own three roundings


def test_the_dit_blend_still_guides_three_channels(lib):
    """tests/test_gpu_dit.py's assertions on forward_with_cfg, restated: the DiT's guidance did not move to four channels."""
    from omnitokenizer_amd.dit import DiT
    g = np.load(os.path.join(GOLDEN, "dit_model_a.npz"))
    m = DiT(**dit_ref.MODELS["a"])
    m.load_state_dict(dit_ref.make_weights(dit_ref.MODELS["a"], dit_ref.SEEDS["a"]), strict=True)
    m = m.cuda().eval()
    x, t, y = (torch.from_numpy(g[k]).cuda() for k in ("x", "t", "y"))
    out = m.forward_with_cfg(x, t, y, float(g["cfg_scale"]))
    err = float((out.cpu().double() - torch.from_numpy(g["forward_with_cfg"])).abs().max())
    assert err <= 4 * float(g["cpu_fp32_err_forward_with_cfg"])
    h = x.shape[0] // 2
    plain = m(torch.cat([x[:h], x[:h]]), t, y)
    assert torch.equal(out[:h, :3], out[h:, :3]) and torch.equal(out[:, 3:], plain[:, 3:])
    assert not torch.equal(out[:h, 3], out[h:, 3])   # channel 3 is not guided


# ---- the whole model -------------------------------------------------------------------------------------------------------------------
_MODELS = {}


def model(name):
    if name not in _MODELS:
        from omnitokenizer_amd.latte import Latte
        m = Latte(**latte_ref.MODELS[name])
        m.load_state_dict(latte_ref.make_weights(latte_ref.MODELS[name], latte_ref.SEEDS[name]), strict=True)
        _MODELS[name] = m.cuda().eval()
    return _MODELS[name]


@pytest.mark.parametrize("name", ["a", "b"])
def test_forward_and_cfg_against_the_reference(lib, name):
    g = np.load(os.path.join(GOLDEN, f"latte_model_{name}.npz"))
    m = model(name)
    x, t, y = (torch.from_numpy(g[k]).cuda() for k in ("x", "t", "y"))
    if latte_ref.MODELS[name]["extras"] != 2:
        y = None
    scale = float(g["cfg_scale"])
    for key, out in (("forward", m(x, t, y)), ("forward_with_cfg", m.forward_with_cfg(x, t, y, scale))):
        ref = torch.from_numpy(g[key])
        err = float((out.cpu().double() - ref).abs().max())
        cpu = float(g[f"cpu_fp32_err_{key}"])
        report(model=name, what=key, gpu_max_abs_err=err, cpu_fp32_max_abs_err=cpu, ratio=err / cpu, max_abs_ref=float(ref.abs().max()))
        assert out.shape == ref.shape and out.dtype == torch.float32
        assert err <= 4 * cpu, f"{name} {key}: GPU error {err:.3e} against 4 x the CPU's fp32 error {cpu:.3e}"
    out = m.forward_with_cfg(x, t, y, scale)
    h = x.shape[0] // 2
    assert torch.equal(out[:h, :, :4], out[h:, :, :4])               # both halves get the same guided eps, on channels [0, 4) ...
    plain = m(torch.cat([x[:h], x[:h]]), t, y)
    assert torch.equal(out[:, :, 4:], plain[:, :, 4:])               # ... and every other channel passes through
    assert not torch.equal(out[:h, :, 4:], out[h:, :, 4:])
    assert not torch.equal(out[:, :, :4], plain[:, :, :4])


def test_forward_range_errors(lib):
    m = model("a")
    x = torch.zeros(2, 5, 8, 8, 8, device="cuda")
    y = torch.zeros(2, dtype=torch.long, device="cuda")
    with pytest.raises(ValueError, match="timestep"):
        m(x, torch.tensor([0, 1000], device="cuda"), y)
    with pytest.raises(ValueError, match="label"):
        m(x, torch.tensor([0, 999], device="cuda"), torch.tensor([0, 11], device="cuda"))
    m(x, torch.tensor([0, 999], device="cuda"), torch.tensor([0, 10], device="cuda"))  # the null row is in range
    with pytest.raises(ValueError, match="even"):
        m.forward_with_cfg(x[:1], torch.zeros(1, dtype=torch.long, device="cuda"), y[:1], 2.0)
    # a model without labels ignores y, as the reference does
    b = model("b")
    xb = rnd(90, 1, 16, 4, 6, 6).cuda()
    tb = torch.tensor([7], device="cuda")
    assert torch.equal(b(xb, tb, torch.tensor([12345], device="cuda")), b(xb, tb))


@pytest.mark.parametrize("name", ["a", "b"])
def test_batch_invariance_of_the_forward(lib, name):
    m = model(name)
    cfg = latte_ref.MODELS[name]
    x = rnd(91, 3, cfg["num_frames"], cfg["in_channels"], cfg["input_size"], cfg["input_size"]).cuda()
    t = torch.tensor([0, 999, 500], device="cuda")
    y = torch.tensor([1, 10, 3], device="cuda") if cfg["extras"] == 2 else None
    full = m(x, t, y)
    assert torch.isfinite(full).all()
    for i in range(3):
        assert torch.equal(m(x[i:i + 1], t[i:i + 1], None if y is None else y[i:i + 1]), full[i:i + 1]), (name, i)


# ---- the sampling loop -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,clip", [("clip", True), ("noclip", False)])
def test_p_sample_loop_5d_against_the_golden_trajectory(lib, tag, clip):
    from omnitokenizer_amd.diffusion import create_diffusion
    g = np.load(os.path.join(GOLDEN, "latte_loop.npz"))
    d = create_diffusion(str(g["respacing"]))
    x0 = torch.from_numpy(g["x0"]).float().cuda()
    noise = torch.from_numpy(g["step_noise"]).float().cuda()
    assert x0.dim() == 5
    traj = [o["sample"] for o in d.p_sample_loop_progressive(latte_ref.toy_model, tuple(x0.shape), noise=x0, clip_denoised=clip,
                                                             device="cuda", step_noise=noise)]
    assert len(traj) == d.num_timesteps == 10 and traj[0].shape == x0.shape
    err = max(float((s.cpu().double() - torch.from_numpy(g[f"trajectory_{tag}"][k])).abs().max()) for k, s in enumerate(traj))
    cpu = float(g[f"cpu_fp32_err_{tag}"])
    report(model="toy", what=f"p_sample_loop_5d_{tag}", gpu_max_abs_err=err, cpu_fp32_max_abs_err=cpu, ratio=err / cpu,
           max_abs_ref=float(np.abs(g[f"trajectory_{tag}"]).max()))
    assert err <= 4 * cpu
    last = d.p_sample_loop(latte_ref.toy_model, tuple(x0.shape), noise=x0, clip_denoised=clip, device="cuda",
                           step_noise=lambda k, shape, dev: noise[k])
    assert torch.equal(last, traj[-1])


def test_p_sample_5d_is_the_4d_step_over_the_frames_and_4d_still_answers(lib):
    from omnitokenizer_amd.diffusion import create_diffusion
    d = create_diffusion("10")
    N, F = 3, 4
    x5, noise5 = rnd(97, N, F, 4, 5, 5).cuda(), rnd(98, N, F, 4, 5, 5).cuda()
    t = torch.tensor([0, 4, 9], device="cuda")          # per sample: every frame of a sample takes its t
    o5 = d.p_sample(latte_ref.toy_model, x5, t, clip_denoised=False, noise=noise5)
    o4 = d.p_sample(dit_ref.toy_model, x5.flatten(0, 1), t.repeat_interleave(F), clip_denoised=False, noise=noise5.flatten(0, 1))
    for k in ("sample", "pred_xstart"):
        assert o5[k].shape == x5.shape and torch.equal(o5[k].flatten(0, 1), o4[k]), k
    with pytest.raises(ValueError, match="model output"):
        d.p_sample(lambda x, t: torch.cat([x, x], dim=1), x5, t)   # doubled on dim 1: not a video model's output
    # the old path against its own golden trajectory (tests/test_gpu_dit.py's construction)
    g = np.load(os.path.join(GOLDEN, "dit_loop.npz"))
    d = create_diffusion(str(g["respacing"]))
    x0 = torch.from_numpy(g["x0"]).float().cuda()
    assert x0.dim() == 4
    last = d.p_sample_loop(dit_ref.toy_model, tuple(x0.shape), noise=x0, clip_denoised=True, device="cuda",
                           step_noise=torch.from_numpy(g["step_noise"]).float().cuda())
    err = float((last.cpu().double() - torch.from_numpy(g["trajectory_clip"][-1])).abs().max())
    assert err <= 4 * float(g["cpu_fp32_err_clip"])


def tiny_vae():
    from omnitokenizer_amd import OmniTokenizer_VQGAN, make_args, synth
    from omnitokenizer_amd.config import OmniTokConfig
    args = make_args(2, resolution=64, use_vae=True)
    vae = OmniTokenizer_VQGAN(args)
    vae.load_state_dict(synth.synth_state_dict(OmniTokConfig.from_args(args), seed=0), strict=True)
    return vae.cuda().eval()


def test_generate_videos_equals_the_three_calls(lib):
    from omnitokenizer_amd.diffusion import create_diffusion, generate_videos
    from omnitokenizer_amd.frames import pixels_to_frames
    from omnitokenizer_amd.latte import Latte
    vae = tiny_vae()
    latte = model("a")
    d = create_diffusion("2")
    labels = torch.tensor([3, 8], device="cuda")
    vids = generate_videos(latte, d, vae, labels, cfg_scale=1.5, seed=11)
    assert vids.shape == (2, 17, 64, 64, 3) and vids.dtype == torch.uint8   # 5 latent frames -> 1 + 4 * 4 pixel frames
    # by hand: the draws of the same generator, p_sample_loop, decode, pixels_to_frames
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)
    z = torch.randn(2, 5, 8, 8, 8, device="cuda", generator=gen)
    z = torch.cat([z, z], 0)
    noise = torch.stack([torch.randn(*z.shape, device="cuda", generator=gen) for _ in range(2)])
    y = torch.cat([labels, torch.full((2,), 10, device="cuda")])
    samples = d.p_sample_loop(latte.forward_with_cfg, z.shape, z, clip_denoised=False, model_kwargs=dict(y=y, cfg_scale=1.5),
                              device="cuda", step_noise=noise)
    assert torch.isfinite(samples).all() and samples.shape == z.shape
    latents = (samples.chunk(2, dim=0)[0] / 0.18215).permute(0, 1, 3, 4, 2).contiguous()   # b f c h w -> b f h w c
    pixels = vae.decode(latents, is_image=False)
    assert pixels.shape == (2, 3, 17, 64, 64) and torch.isfinite(pixels).all()
    assert torch.equal(vids, pixels_to_frames(pixels))
    assert torch.equal(vids, generate_videos(latte, d, vae, labels, cfg_scale=1.5, seed=11))
    assert not torch.equal(vids, generate_videos(latte, d, vae, labels, cfg_scale=1.5, seed=12))
    # a model without labels: labels=None, one video, no guidance
    cfg = {**latte_ref.MODELS["a"], "extras": 1, "depth": 2}
    plain = Latte(**cfg)
    plain.load_state_dict(latte_ref.make_weights(cfg, 6), strict=True)
    plain = plain.cuda().eval()
    one = generate_videos(plain, d, vae, None, cfg_scale=1.0, seed=3)
    assert one.shape == (1, 17, 64, 64, 3) and one.dtype == torch.uint8
    assert torch.equal(one, generate_videos(plain, d, vae, None, cfg_scale=1.0, seed=3))
    with pytest.raises(ValueError, match="labels are required"):
        generate_videos(latte, d, vae, None)
