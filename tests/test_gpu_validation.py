"""GPU: the validation losses (csrc/losses.hip, omnitokenizer_amd/losses.py) and OmniTokenizer_VQGAN.forward(x) /
validation_step against the reference's own forward(x) (tests/golden/val_*.npz, make_golden_validation.py).

Kernel bar.  The kernels form every summand in fp32 exactly as torch / numpy fp32 arithmetic forms it and add the summands
in fp64.  Two fp64 summations of the same n terms t_i, in any order, differ by at most 2 (n - 1) 2^-53 sum |t_i| (each is
within (n - 1) u sum |t_i| of the exact sum, u = 2^-53): KERNEL_BAR = n 2^-52 sum |t_i|.  Nothing measured enters it.

forward(x) bars.  With d_pix = max |x_recon_gpu - x_recon_ref64| (asserted <= PIX_BAR = 1e-4, the project's pixel bar) and
d = x_recon - x of the reference's fp64 run:
  | mean |d'| - mean |d| |      <= d_pix                      (reverse triangle inequality, per element)
  | mean d'^2 - mean d^2 |      <= d_pix (2 max |d| + d_pix)  ((a + e)^2 - a^2 = e (2a + e))
  | laplace' - laplace |        <= 0.8 d_pix                  (the map v -> 0.8 (v + 0.5) + 0.1 has slope 0.8)
  | commitment' - commitment |  <= 0.25 d_z (2 max |z - e| + d_z), d_z = max |z_gpu - z_ref64|, ids equal everywhere
  | kl' - kl |                  <= 0.5 kl_weight m (d_m (2 max |mu| + d_m) + d_m (exp(max lv + d_m) + 1)), m elements per
                                   item, d_m = max |moments_gpu - moments_ref64| (mean value theorem on exp(lv) - lv)
each times its weight, plus ROUND = 2^-22 of the reference value for the final roundings (the fp32 summands' own 2^-24
relative rounding, the fp32 mean and the fp32 products with the weights).
"""
import numpy as np
import pytest
import torch

from tests.validation_cases import VAL_CASES, ValCase

pytestmark = pytest.mark.gpu

PIX_BAR = 1e-4
ROUND = 2.0 ** -22
# perceptual_loss end to end against the reference's fp64 run: pixel error propagated through VGG16, no derivable bound.
# Largest |ours - ref64| over each fixture's values on its first MI355X run (profiles/r13_validation.txt); the bar is 4x the
# largest of them (box-to-box variation of the split-precision GEMMs upstream).
PERC_MEASURED = {
    "val_s2_sdpa_r64_img_l1": 1.678e-08, "val_s2_sdpa_r64_vid_l1": 5.557e-09, "val_s2_sdpa_r64_vid_mse": 2.399e-08,
    "val_s1_legacy_r64_vid": 1.324e-09, "val_vae_s2_sdpa_r64_vid": 2.269e-08, "val_genup2_r64_img": 2.383e-08,
    "val_ext_s2_sdpa_r64_img": 5.960e-08, "val_s2_sdpa_r64_vid_b2_l1": 2.277e-08,
}
# measured maximum 5.960e-08 -> bar 2.384e-07.  The values lie between 0.33 and 0.62, where one fp32 ulp is 5.96e-08: the
# maximum is exactly one ulp of the external-codebook fixture's reference (an fp32 run, it has no fp64 one), the bar four.
PERC_BAR = 4.0 * max(PERC_MEASURED.values())


# ---- the kernels against fp64 numpy on identical inputs ----------------------------------------------------------------

def np_recon_terms(x, r):
    """the three summands in numpy fp32, torch's operation order (every numpy op rounds on its own)"""
    h, e8, e1 = np.float32(0.5), np.float32(0.8), np.float32(0.1)
    d = r - x
    lap = np.abs((e8 * (x + h) + e1) - (e8 * (r + h) + e1))
    return np.abs(d), d * d, lap


def np_kl_terms(mu, logvar):
    lv = np.clip(logvar, np.float32(-30.0), np.float32(20.0))
    var = np.exp(lv.astype(np.float64)).astype(np.float32)   # the kernel's definition: fp64 exp rounded to fp32
    return ((mu * mu + var) - np.float32(1.0)) - lv


def kernel_bar(terms64):
    return terms64.size * 2.0 ** -52 * np.abs(terms64).sum()


def mixed(shape, seed):
    """mixed sign and scale: N(0, 1) times 10^U(-3, 1), some exact zeros and pixel-range values"""
    g = np.random.default_rng(seed)
    v = g.standard_normal(shape, dtype=np.float32) * (10.0 ** g.uniform(-3, 1, shape)).astype(np.float32)
    v.reshape(-1)[::7] = g.uniform(-0.5, 0.5, v.reshape(-1)[::7].shape).astype(np.float32)
    v.reshape(-1)[::11] = 0.0
    return v


@pytest.mark.parametrize("shape", [(1, 1), (3, 63), (2, 3, 5, 7, 11), (5, 1027), (4, 3, 64, 64), (2, 9000003)])
def test_recon_losses_kernel_against_fp64_numpy(shape):
    from omnitokenizer_amd import losses, reconstruction_losses
    x, r = mixed(shape, 1), mixed(shape, 2)
    B = shape[0]
    n = x[0].size
    assert shape[0] * n <= 2 ** 24 or shape == (2, 9000003)   # the last case is the one an fp32 accumulator would fail
    xt, rt = torch.from_numpy(x).cuda(), torch.from_numpy(r).cuda()
    x0, r0 = xt.clone(), rt.clone()
    sums, total = losses.recon_sums(xt, rt)
    assert torch.equal(xt, x0) and torch.equal(rt, r0)   # inputs are not modified
    sums, total = sums.cpu().numpy(), total.cpu().numpy()
    terms = [t.astype(np.float64).reshape(B, n) for t in np_recon_terms(x, r)]
    for k, t in enumerate(terms):
        for b in range(B):
            err, bar = abs(sums[b, k] - t[b].sum()), kernel_bar(t[b])
            assert err <= bar, (shape, k, b, err, bar)
        # the batch total is the index-ordered sum of the per-item sums, to the bit
        acc = 0.0
        for b in range(B):
            acc += sums[b, k]
        assert total[k] == acc
        assert abs(total[k] - t.sum()) <= kernel_bar(t)
    means = reconstruction_losses(xt, rt)
    for k, key in enumerate(("l1", "mse", "logits_laplace")):
        assert means[key].dtype == torch.float64 and tuple(means[key].shape) == (B,)
        assert np.array_equal(means[key].cpu().numpy(), sums[:, k] / n)
    # a flags word computes only what it names
    s1, _ = losses.recon_sums(xt, rt, losses.FLAG_MSE | losses.FLAG_LAPLACE)
    s1 = s1.cpu().numpy()
    assert (s1[:, 0] == 0).all() and np.array_equal(s1[:, 1:], sums[:, 1:])
    # a view whose storage offset breaks the 16-byte alignment takes the element-wise path: same summands
    if n > 4:
        xo, ro = torch.from_numpy(np.concatenate([[0.0], x.reshape(-1)]).astype(np.float32)).cuda()[1:].view(shape), \
            torch.from_numpy(np.concatenate([[0.0], r.reshape(-1)]).astype(np.float32)).cuda()[1:].view(shape)
        assert xo.data_ptr() % 16 != 0
        so, _ = losses.recon_sums(xo, ro)
        for k, t in enumerate(terms):
            for b in range(B):
                assert abs(so[b, k].item() - t[b].sum()) <= kernel_bar(t[b])


@pytest.mark.parametrize("N,c,n_codes", [(1, 8, 16), (63, 8, 8192), (1000, 6, 50), (20480, 8, 8192), (257, 4, 3)])
def test_commitment_kernel_gathers_the_code_rows(N, c, n_codes):
    from omnitokenizer_amd import losses
    g = np.random.default_rng(N)
    z, E = mixed((N, c), 3), mixed((n_codes, c), 4)
    ids = g.integers(0, n_codes, N)
    ids[0], ids[-1] = n_codes - 1, 0
    zt, Et, it = torch.from_numpy(z).cuda(), torch.from_numpy(E).cuda(), torch.from_numpy(ids).cuda()
    got = losses.commitment_sum(zt.view(1, N, c), it.view(1, N), Et)
    d = z - E[ids]                      # the explicit E[ids]
    t = (d * d).astype(np.float64)
    assert tuple(got.shape) == (1,) and got.dtype == torch.float64
    assert abs(got.item() - t.sum()) <= kernel_bar(t), (got.item(), t.sum())
    assert torch.equal(zt.cpu(), torch.from_numpy(z)) and torch.equal(Et.cpu(), torch.from_numpy(E))


@pytest.mark.parametrize("shape", [(1, 2, 1), (3, 2, 63), (2, 16, 5, 8, 8), (4, 6, 1027)])
def test_kl_kernel_against_fp64_numpy(shape):
    from omnitokenizer_amd import losses
    g = np.random.default_rng(5)
    B, c2 = shape[:2]
    half = (B, c2 // 2) + tuple(shape[2:])
    mu, lv = mixed(half, 6), mixed(half, 7)
    flat = lv.reshape(-1)   # a view: lv is contiguous
    flat[::5] = g.uniform(-60, 40, flat[::5].shape).astype(np.float32)   # log-variances outside [-30, 20] too
    if flat.size > 8:
        assert (lv < -30).any() and (lv > 20).any()
    mom = np.concatenate([mu, lv], axis=1)
    sums, total = losses.kl_sums(torch.from_numpy(mom).cuda())
    t = np_kl_terms(mu, lv).astype(np.float64).reshape(B, -1)
    for b in range(B):
        assert abs(sums[b].item() - t[b].sum()) <= kernel_bar(t[b]), (b, sums[b].item(), t[b].sum())
    acc = 0.0
    for b in range(B):
        acc += sums[b].item()
    assert total.item() == acc


def _model(c, lpips=True):
    from omnitokenizer_amd import OmniTokenizer_VQGAN
    from omnitokenizer_amd.lpips import load_lpips
    m = OmniTokenizer_VQGAN(c.args, attention_mode=c.mode)
    m.load_state_dict(c.sd, strict=True)
    m = m.cuda().eval()
    if lpips:
        m.set_perceptual_model(load_lpips("cuda", c.lpips_sd))
    return m


def test_losses_are_deterministic_also_beside_a_busy_second_stream():
    from omnitokenizer_amd import losses
    c = ValCase("val_s2_sdpa_r64_vid_l1")
    m = _model(c, lpips=False)
    x, r = torch.from_numpy(mixed((8, 3, 5, 128, 128), 7)).cuda(), torch.from_numpy(mixed((8, 3, 5, 128, 128), 8)).cuda()
    xe = c.x.cuda().repeat(8, 1, 1, 1, 1)
    m.encode(xe, False)   # workspace growth and first-call work happen here, not beside the timed pair
    torch.cuda.synchronize()
    quiet = [t.clone() for t in losses.recon_sums(x, r)]
    again = losses.recon_sums(x, r)
    assert all(torch.equal(a, b) for a, b in zip(quiet, again))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            m.encode(xe, False)
    busy = losses.recon_sums(x, r)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(quiet, busy))
    z = torch.from_numpy(mixed((4096, 8), 9)).cuda()
    ids = torch.randint(0, 8192, (4096,), device="cuda")
    E = m.codebook.embeddings.data
    assert torch.equal(losses.commitment_sum(z, ids, E), losses.commitment_sum(z, ids, E))
    mom = torch.from_numpy(mixed((2, 16, 2, 8, 8), 10)).cuda()
    assert all(torch.equal(a, b) for a, b in zip(losses.kl_sums(mom), losses.kl_sums(mom)))


# ---- forward(x) against the reference ----------------------------------------------------------------------------------

def _forward(c, m):
    x = c.x.cuda()
    x0 = x.clone()
    kw = {}
    if c.noise is not None:
        kw["noise"] = c.noise
    if c.frame_idx is not None:
        kw["frame_idx"] = c.frame_idx.cuda()
    out = m(x, **kw)
    assert torch.equal(x, x0), "forward(x) modified its input"   # the mse path in particular
    return x, out


@pytest.mark.parametrize("name", VAL_CASES)
def test_forward_against_the_reference(name):
    import torch.nn.functional as F
    c = ValCase(name)
    a = c.args
    m = _model(c)
    x, (recon_loss, x_recon, vq, perc) = _forward(c, m)
    assert recon_loss.dim() == 0 and recon_loss.dtype == torch.float32 and perc.dtype == torch.float32
    assert tuple(perc.shape) == c.g["perceptual64"].shape
    # pixels (after the +0.5 shift on the non-l1 path, as the reference returns them)
    d_pix = (x_recon.cpu().double() - c.x_recon64).abs().max().item()
    print(f"{name}: d_pix {d_pix:.3e}")
    assert d_pix <= PIX_BAR
    x_ref = c.x_seen.double()
    if a.gen_upscale is not None:   # the resize runs in torch on the device: its distance to the fp64 resize adds to d
        up = dict(scale_factor=a.gen_upscale, mode="bilinear", align_corners=True)
        x_ref = F.interpolate(c.x.double(), **up)
        d_pix += (F.interpolate(x, **up).cpu().double() - x_ref).abs().max().item()
    d = (c.x_recon64 - c.shift) - x_ref
    dmax = d.abs().max().item()
    ref = c.scalar("recon_loss64")
    if c.l1_path:
        bar = a.l1_weight * d_pix
    else:
        bar = a.l1_weight * d_pix * (2 * dmax + d_pix) + 0.8 * a.logitslaplace_weight * d_pix
    err = abs(recon_loss.item() - ref)
    print(f"{name}: recon_loss {recon_loss.item()!r} ref64 {ref!r} err {err:.3e} bar {bar + ROUND * abs(ref):.3e}")
    assert err <= bar + ROUND * abs(ref)
    if c.is_vae:
        assert set(vq) == {"commitment_loss"}
        _, mom = m.encode(x, c.is_image, noise=c.noise, return_moments=True)
        mom64 = c.wide("moments")
        d_m = (mom.cpu().double() - mom64).abs().max().item()
        mu, lv = torch.chunk(mom64, 2, dim=1)
        per_item = mu[0].numel()
        bar = 0.5 * a.kl_weight * per_item * (d_m * (2 * mu.abs().max().item() + d_m)
                                              + d_m * (np.exp(min(lv.max().item(), 20.0) + d_m) + 1.0))
        ref = c.scalar("kl64")
        err = abs(vq["commitment_loss"].item() - ref)
        print(f"{name}: kl {vq['commitment_loss'].item()!r} ref64 {ref!r} d_m {d_m:.3e} err {err:.3e} bar {bar + ROUND * abs(ref):.3e}")
        assert vq["commitment_loss"].dim() == 0 and vq["commitment_loss"].dtype == torch.float32
        assert err <= bar + ROUND * abs(ref)
    else:
        ids = vq["encodings"].cpu()
        assert torch.equal(ids, torch.from_numpy(c.g["ids"].astype(np.int64))), "ids differ from the reference's"
        ref = c.scalar("perplexity64")
        assert abs(vq["perplexity"].item() - ref) < 1e-3 * ref   # the bar of test_forward_codebook_statistics
        if c.is_ext:
            assert vq["commitment_loss"].abs().max().item() == 0.0 and c.scalar("commitment64") == 0.0
        else:
            assert m.codebook.call_cnt == 1
            _, z = m.encode(x, c.is_image, return_latents=True)
            z64 = c.wide("z")
            d_z = (z.cpu().double() - z64).abs().max().item()
            E = c.sd["codebook.embeddings"].double()
            zmax = (z64 - E[ids]).abs().max().item()
            bar = 0.25 * d_z * (2 * zmax + d_z)
            ref = c.scalar("commitment64")
            err = abs(vq["commitment_loss"].item() - ref)
            print(f"{name}: commitment {vq['commitment_loss'].item()!r} ref64 {ref!r} d_z {d_z:.3e} err {err:.3e} "
                  f"bar {bar + ROUND * abs(ref):.3e}")
            assert vq["commitment_loss"].dim() == 0 and vq["commitment_loss"].dtype == torch.float32
            assert err <= bar + ROUND * abs(ref)
    # perceptual_loss, step (b): end to end against the reference's fp64 run
    perr = np.abs(perc.cpu().numpy().astype(np.float64) - c.g["perceptual64"]).max()
    print(f"{name}: perceptual end to end max |ours - ref64| {perr:.3e}")
    assert perr <= PERC_BAR, (perr, PERC_BAR)


@pytest.mark.parametrize("name", VAL_CASES)
def test_perceptual_term_on_the_reference_own_frames(name):
    """step (a): frame selection, shift, ordering and weighting, on the fixture's own x and fp32 x_recon, held to the bar of
    tests/test_gpu_lpips.py (val_bar, built from the reference's fp64 per-slice means of the same frames)"""
    from tests.test_gpu_lpips import val_bar
    c = ValCase(name)
    m = _model(c)
    wmax = [float(c.lpips_sd[f"lin{k}.model.1.weight"].max()) for k in range(5)]
    xs = c.x_seen.cuda()
    xr = c.x_recon32.cuda()       # carries the reference's +0.5 on the non-l1 path ...
    if c.shift:
        # ... which the kernel's own `shift` reproduces: x + 0.5 formed in fp32 inside the read
        assert torch.equal(m._perceptual_loss(xs, xs * 0.5, c.is_image, c.shift, None),
                           m._perceptual_loss(xs + c.shift, xs * 0.5 + c.shift, c.is_image, 0.0, None))
        xs = xs + c.shift
    fi = None if c.frame_idx is None else c.frame_idx.cuda()
    got = m._perceptual_loss(xs, xr, c.is_image, 0.0, fi).cpu().numpy().astype(np.float64).reshape(-1)
    w = c.args.perceptual_weight
    vb = val_bar(c.g["lpips_res64"], c.g["lpips_val64"], wmax)
    err = np.abs(got / w - c.g["lpips_val64"])
    print(f"{name}: perceptual on the reference's frames: err {err.max():.3e} bar {vb.min():.3e}")
    assert got.shape == c.g["lpips_val64"].shape and (err <= vb).all(), (err, vb)


@pytest.mark.parametrize("name", VAL_CASES)
def test_validation_step_and_codebook_state(name):
    """validation_step returns and logs forward(x)'s own scalars: with the generators seeded alike before each, the two draw
    the same frame per clip (device) and the same posterior noise (host), so every value is equal to the bit"""
    c = ValCase(name)
    x = c.x.cuda()
    m = _model(c)
    torch.manual_seed(3)
    recon_loss, _, vq, perc = m(x)
    m2 = _model(c)
    logged = []
    m2.log = lambda k, v, **kw: logged.append((k, v))
    torch.manual_seed(3)
    out = m2.validation_step({"video": x}, 0)
    # the reference's names, in the order it logs them (omnitokenizer.py:611-618)
    keys = ["val/recon_loss", "val/perceptual_loss"] + (["val/kl_loss"] if c.is_vae else ["val/perplexity", "val/commitment_loss"])
    assert list(out) == keys and [k for k, _ in logged] == keys and all(v is out[k] for k, v in logged)
    # 0-dim, but for the external codebook's commitment loss, the [1] zero tensor VectorQuantize reports
    assert all((v.dim() == 0 or (c.is_ext and k == "val/commitment_loss" and tuple(v.shape) == (1,))) and torch.isfinite(v).all()
               for k, v in out.items())
    assert torch.equal(out["val/recon_loss"], recon_loss)
    assert torch.equal(out["val/perceptual_loss"], perc.mean())   # what Lightning's log records of the un-reduced tensor
    if c.is_vae:
        assert torch.equal(out["val/kl_loss"], vq["commitment_loss"])
    else:
        assert torch.equal(out["val/perplexity"], vq["perplexity"])
        assert torch.equal(out["val/commitment_loss"].reshape(-1), vq["commitment_loss"].reshape(-1))
    if c.frame_idx is not None and not c.is_vae:
        # the seeded draw is torch.randint(0, T, [B]) on the device, and it is used exactly as an explicit frame_idx is
        torch.manual_seed(3)
        drawn = torch.randint(0, c.frames, [c.batch], device="cuda")
        assert torch.equal(_model(c)(x, frame_idx=drawn)[3], perc)
    if not c.is_vae:
        # call_cnt and the usage EMA advance exactly as on the log_image path
        m3 = _model(c)
        _, _, _, _, vq3 = m3(x, log_image=True)
        assert m.codebook.call_cnt == m2.codebook.call_cnt == m3.codebook.call_cnt == 1
        assert torch.equal(m.codebook.codebook_usage.data, m3.codebook.codebook_usage.data)
        assert torch.equal(m2.codebook.codebook_usage.data, m3.codebook.codebook_usage.data)
        assert set(vq3) <= set(vq) | {"commitment_loss"} and torch.equal(vq3["encodings"], vq["encodings"])
        assert torch.equal(vq3["batch_usage"], vq["batch_usage"])
        if not c.is_ext:
            assert torch.equal(vq3["commitment_loss"], vq["commitment_loss"])   # the log_image dict carries it too


def test_forward_refuses_stream_capture():
    c = ValCase("val_s2_sdpa_r64_img_l1")
    m = _model(c)
    x = c.x.cuda()
    m(x)   # every allocation the call needs exists before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="cannot be recorded into a HIP graph"):
        with torch.cuda.graph(g):
            m(x)
    torch.cuda.synchronize()
    assert m.codebook.call_cnt == 1
