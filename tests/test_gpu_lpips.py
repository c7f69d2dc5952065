"""GPU (-m gpu): LPIPS (csrc/lpips.hip, omnitokenizer_amd/lpips.py) against torch and against the reference's own values
(tests/golden/lpips_*.npz, make_golden_lpips.py).

Bars (derived, not measured).  u = 2^-24, gamma_n = n u / (1 - n u).
  Preprocess: the same fp32 operations in the same order as the torch expression: equal bits.  The uint8 conversion is
    float(u) / 255 correctly rounded, ToTensor's (CPU) division; the references below convert on the CPU, because torch's
    CUDA division by a Python scalar multiplies by the rounded reciprocal instead.
  Head, per pixel.  Let e be a bound on the normwise relative error of each normalised feature vector a / |a| (and
  b / |b|).  Then |Delta d| <= 2 e normwise, and with non-negative lin weights w (trained LPIPS has them, and so do the
  synthetic ones; asserted below), the weighted Cauchy-Schwarz inequality gives
      |Delta sum_c w_c d_c^2| <= 2 sqrt(v) sqrt(max w) 2 e + max w (2 e)^2,   v = sum_c w_c d_c^2 <= 4 max w,
  plus the rounding of the sum and the squares, (gamma_C + 3 u) v.  Over the pixels, mean(sqrt(v)) <= sqrt(mean(v)) =
  sqrt(res) (Jensen); the fp64 mean adds nothing at this scale.  So the head's error on a slice is at most
      HEAD(res, e, C, wmax) = 4 e sqrt(wmax res) + 4 e^2 wmax + (gamma_C + 3 u) res.
  The head's own roundings (the C-term sum of squares, sqrt, + 1e-10 and the division) give e_head = gamma_C / 2 + 3 u.
  Against an fp64 torch evaluation of the same fp32 features: HEAD(res64, e_head, C, max w).
  Full forward: the features reach the head with the rounding of the fp32 trunk.  As in tests/test_gpu_fid.py, a layer of
    K-term fp32 sums gives an independent relative error ~ sqrt(K) u per layer, 4 bounding sum |w x| / |y|, added in
    quadrature over the L roundings on the path: delta_l = sqrt(L_l) sqrt(K_l) 4 u with (L, K) = (3, 576), (5, 1152),
    (8, 2304), (11, 4608), (14, 4608) for slices 1..5 (the preprocess counts as one rounding; max pools are exact).
    A normalised vector's relative error is at most twice its input's: e_l = 2 delta_l + e_head.
    RES_BAR_l = HEAD(res64_l, e_l, C_l, max w_l), VAL_BAR = sum_l RES_BAR_l + u |val64|.  val32 (the reference's own fp32
    run, a different summation order) is held to 2 VAL_BAR; tests/test_lpips_cpu.py checks that it lies inside VAL_BAR.
"""
import os

import numpy as np
import pytest
import torch

from omnitokenizer_amd import lpips, synth

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = 2.0 ** -24
CASES = ["lpips_16x16", "lpips_50x70", "lpips_64x64", "lpips_256x256", "lpips_same_32x32", "lpips_light_40x40"]
PATH = [(3, 576), (5, 1152), (8, 2304), (11, 4608), (14, 4608)]


def _gamma(n):
    return n * U / (1 - n * U)


def head_bar(res, e, C, wmax):
    res = np.maximum(np.asarray(res, dtype=np.float64), 0.0)
    return 4 * e * np.sqrt(wmax * res) + 4 * e * e * wmax + (_gamma(C) + 3 * U) * res


def res_bars(res64, wmax):
    """[n, 5] per-slice bars of the full forward against the fp64 reference"""
    out = np.zeros_like(np.asarray(res64, dtype=np.float64))
    for l, (L, K) in enumerate(PATH):
        C = lpips.CHNS[l]
        e = 2 * np.sqrt(L) * np.sqrt(K) * 4 * U + _gamma(C) / 2 + 3 * U
        out[:, l] = head_bar(res64[:, l], e, C, wmax[l])
    return out


def val_bar(res64, val64, wmax):
    return res_bars(res64, wmax).sum(1) + U * np.abs(val64)


def lin_wmax(sd):
    ws = [sd[f"lin{k}.model.1.weight"].double() for k in range(5)]
    assert all((w >= 0).all() for w in ws)   # the bar's Cauchy-Schwarz step needs non-negative weights
    return [float(w.max()) for w in ws]


def _fix(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def _pairs(f):
    from tests.golden.make_golden_lpips import case_images
    return case_images(int(f["H"]), int(f["W"]), int(f["seed"]), str(f["mode"]), int(f["seed2"]), int(f["n"]))


def _to_input(u):
    from tests.golden.make_golden_lpips import to_input
    return to_input(u)


@pytest.fixture(scope="module")
def weights():
    from tests.golden.make_golden_lpips import WEIGHT_SEED
    return synth.synth_lpips_state_dict(WEIGHT_SEED)


@pytest.fixture(scope="module")
def model(weights):
    return lpips.load_lpips("cuda", weights)


def _unit(u):
    """float(u) / 255, ToTensor's correctly rounded division (on the CPU), back on u's device"""
    return (u.cpu().to(torch.float32) / 255).to(u.device)


def _scaling(sd):
    return sd["scaling_layer.shift"].cuda(), sd["scaling_layer.scale"].cuda()


def _preprocess(model, v5, shift=0.0, clamp=False, normalize=False):
    B, F_, _, H, W = v5.shape
    pk = model.packed("cuda")
    out = torch.empty((B * F_, H, W, 4), device="cuda", dtype=torch.float32)
    torch.ops.omnitok.lpips_preprocess(v5, shift, clamp, normalize, pk["shift"], pk["scale"], 0, out)
    return out


# ---- 1. preprocess ------------------------------------------------------------------------------------------------------

def test_preprocess_bit_identical_fp32_nchw(model, weights):
    sh, sc = _scaling(weights)
    x = torch.randn((3, 3, 37, 29), generator=torch.Generator().manual_seed(1)).cuda() * 0.4
    got = _preprocess(model, x.unsqueeze(1))
    want = ((x - sh) / sc).permute(0, 2, 3, 1)
    assert torch.equal(got[..., :3], want)
    assert torch.equal(got[..., 3], torch.zeros_like(got[..., 3]))


def test_preprocess_bit_identical_bcthw_shift_clamp(model, weights):
    sh, sc = _scaling(weights)
    x = torch.randn((2, 3, 5, 20, 17), generator=torch.Generator().manual_seed(2)).cuda() * 0.7   # [B, 3, F, H, W]
    got = _preprocess(model, x.permute(0, 2, 1, 3, 4), shift=0.5, clamp=True)
    v = torch.clamp(x + 0.5, 0, 1)
    want = ((v.permute(0, 2, 1, 3, 4).reshape(-1, 3, 20, 17) - sh) / sc).permute(0, 2, 3, 1)
    assert torch.equal(got[..., :3], want)


@pytest.mark.parametrize("normalize", [False, True])
def test_preprocess_bit_identical_uint8_bthwc(model, weights, normalize):
    sh, sc = _scaling(weights)
    u = torch.from_numpy(np.random.Generator(np.random.PCG64(3)).integers(0, 256, (2, 3, 18, 21, 3), dtype=np.uint8)).cuda()
    got = _preprocess(model, u.permute(0, 1, 4, 2, 3), shift=-0.5, normalize=normalize)
    v = _unit(u) + (-0.5)
    if normalize:
        v = 2 * v - 1
    want = (v.reshape(-1, 18, 21, 3).permute(0, 3, 1, 2) - sh) / sc
    assert torch.equal(got[..., :3], want.permute(0, 2, 3, 1))


# ---- 2. the head --------------------------------------------------------------------------------------------------------

def _head64(a, b, w):
    """fp64 torch: normalize_tensor, squared difference, 1x1 conv, spatial mean; a, b [N, h, w, C] -> [N]"""
    a, b, w = a.double(), b.double(), w.double()
    na = torch.sqrt((a * a).sum(-1, keepdim=True)) + 1e-10
    nb = torch.sqrt((b * b).sum(-1, keepdim=True)) + 1e-10
    return ((a / na - b / nb) ** 2 * w).sum(-1).mean((1, 2))


@pytest.mark.parametrize("C,h,w", [(64, 256, 256), (64, 16, 16), (128, 35, 25), (256, 12, 6), (512, 8, 8), (512, 3, 4),
                                   (512, 1, 1), (512, 1, 3), (128, 33, 1)])
def test_head_matches_fp64(C, h, w):
    g = torch.Generator().manual_seed(C + h * 7 + w)
    N = 3
    feats = torch.relu(torch.randn((2 * N, h, w, C), generator=g))
    feats[N:] = torch.relu(feats[:N] + 0.3 * torch.randn((N, h, w, C), generator=g))
    lw = torch.randn(C, generator=g).abs() / C ** 0.5
    res = lpips.layer_head(feats.cuda(), lw.cuda(), 2).cpu()
    assert (res[:, [0, 1, 3, 4]] == 0).all()
    want = _head64(feats[:N], feats[N:], lw)
    bar = head_bar(want.numpy(), _gamma(C) / 2 + 3 * U, C, float(lw.max()))
    err = (res[:, 2] - want).abs().numpy()
    assert (err <= bar).all(), (err, bar)


def test_head_identical_and_zero_pixels():
    C, h, w, N = 256, 9, 11, 2
    g = torch.Generator().manual_seed(5)
    a = torch.relu(torch.randn((N, h, w, C), generator=g))
    a[:, 2:5, 3:7] = 0          # all-zero pixels, as after ReLU in deep slices
    lw = torch.rand(C, generator=g)
    res = lpips.layer_head(torch.cat([a, a]).cuda(), lw.cuda(), 0).cpu()
    assert torch.equal(res, torch.zeros_like(res))
    z = torch.zeros((2 * N, h, w, C))
    res = lpips.layer_head(z.cuda(), lw.cuda(), 4).cpu()
    assert torch.equal(res, torch.zeros_like(res))
    b = torch.relu(torch.randn((N, h, w, C), generator=g))
    b[:, 2:5, 3:7] = 0
    res = lpips.layer_head(torch.cat([a, b]).cuda(), lw.cuda(), 1).cpu()
    assert torch.isfinite(res).all() and (res[:, 1] > 0).all()


# ---- 3. the full forward against the reference --------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES)
def test_forward_matches_reference(model, weights, case):
    f = _fix(case)
    a, b = (_to_input(u) for u in _pairs(f))
    val = model(a.cuda(), b.cuda())
    assert val.shape == (int(f["n"]), 1, 1, 1) and val.dtype == torch.float32
    res = torch.empty((int(f["n"]), 5), dtype=torch.float64, device="cuda")
    x = torch.empty((2 * int(f["n"]), int(f["H"]), int(f["W"]), 4), device="cuda")
    pk = model.packed("cuda")
    for half, v in enumerate((a.cuda(), b.cuda())):
        torch.ops.omnitok.lpips_preprocess(v.unsqueeze(1), 0.0, False, False, pk["shift"], pk["scale"], 0,
                                           x[half * int(f["n"]):(half + 1) * int(f["n"])])
    model.trunk(x, res)
    res, val = res.cpu().numpy(), val.view(-1).cpu().numpy().astype(np.float64)
    wmax = lin_wmax(weights)
    rb = res_bars(f["res64"], wmax)
    assert (np.abs(res - f["res64"]) <= rb).all(), (res - f["res64"], rb)
    vb = val_bar(f["res64"], f["val64"], wmax)
    assert (np.abs(val - f["val64"]) <= vb).all(), (val - f["val64"], vb)
    assert (np.abs(val - f["val32"]) <= 2 * vb).all(), (val - f["val32"], vb)
    if str(f["mode"]) == "same":
        assert (val == 0).all()


# ---- 4. batch independence ----------------------------------------------------------------------------------------------

def test_batch_and_chunk_independence(model):
    from tests.golden.make_golden_lpips import NOISE
    a = _to_input(synth.synth_fid_images(7, 48, 40, 81)).cuda()
    b = _to_input(synth.synth_fid_images(7, 48, 40, 81, NOISE, 82)).cuda()
    full = model(a, b).view(-1)
    alone = model(a[3:4], b[3:4]).view(-1)
    assert torch.equal(full[3:4], alone)
    for mp in (1, 5, 32):
        got = lpips.lpips_frames(a, b, model, layout="nchw", max_pairs=mp).view(-1)
        assert torch.equal(got, full), mp


# ---- 5. layouts ---------------------------------------------------------------------------------------------------------

def test_layouts_agree(model):
    g = torch.Generator().manual_seed(9)
    x = (torch.rand((2, 3, 3, 24, 20), generator=g) - 0.5).cuda()          # [B, 3, F, H, W]
    y = (x + 0.05 * torch.randn(x.shape, generator=g).cuda()).clamp(-0.5, 0.5)
    got = lpips.lpips_frames(x, y, model, layout="bcthw")
    assert got.shape == (2, 3)
    af = x.permute(0, 2, 1, 3, 4).contiguous().view(-1, 3, 24, 20)
    bf = y.permute(0, 2, 1, 3, 4).contiguous().view(-1, 3, 24, 20)
    assert torch.equal(got, model(af, bf).view(2, 3))
    assert torch.equal(got, lpips.lpips_frames(x.permute(0, 2, 1, 3, 4), y.permute(0, 2, 1, 3, 4), model, layout="btchw"))
    ua = torch.from_numpy(np.random.Generator(np.random.PCG64(4)).integers(0, 256, (2, 3, 24, 20, 3), dtype=np.uint8)).cuda()
    ub = torch.from_numpy(np.random.Generator(np.random.PCG64(5)).integers(0, 256, (2, 3, 24, 20, 3), dtype=np.uint8)).cuda()
    gu = lpips.lpips_frames(ua, ub, model, layout="bthwc", shift=-0.5)
    fa = (_unit(ua) + (-0.5)).permute(0, 1, 4, 2, 3).reshape(-1, 3, 24, 20)
    fb = (_unit(ub) + (-0.5)).permute(0, 1, 4, 2, 3).reshape(-1, 3, 24, 20)
    assert torch.equal(gu, model(fa, fb).view(2, 3))
    gn = lpips.lpips_frames(ua, ub, model, layout="bthwc", normalize=True)
    na = 2 * _unit(ua) - 1
    nb = 2 * _unit(ub) - 1
    want = model(na.permute(0, 1, 4, 2, 3).reshape(-1, 3, 24, 20), nb.permute(0, 1, 4, 2, 3).reshape(-1, 3, 24, 20))
    assert torch.equal(gn, want.view(2, 3))


# ---- 6. the tokenizer's perceptual distance -----------------------------------------------------------------------------

def test_vqgan_perceptual_distance(model):
    from omnitokenizer_amd import OmniTokenizer_VQGAN, make_args
    from omnitokenizer_amd.config import OmniTokConfig
    args = make_args(2, resolution=64)
    vq = OmniTokenizer_VQGAN(args)
    vq.load_state_dict(synth.synth_state_dict(OmniTokConfig.from_args(args), seed=0), strict=True)
    vq = vq.cuda().eval()
    x = synth.synth_video(2, 5, 64, seed=1234).cuda()
    rec = vq.decode(vq.encode(x, False), False)
    usage = vq.codebook.codebook_usage.clone()
    cnt = vq.codebook.call_cnt
    d = vq.perceptual_distance(x, rec, False, model)
    B, _, F_, H, W = x.shape
    af = x.permute(0, 2, 1, 3, 4).contiguous().view(-1, 3, H, W)     # the reference's all_frames / all_frames_recon
    bf = rec.permute(0, 2, 1, 3, 4).contiguous().view(-1, 3, H, W)
    assert d.shape == (B, F_) and torch.equal(d, model(af, bf).view(B, F_))
    assert (d > 0).all()
    assert vq.codebook.call_cnt == cnt and torch.equal(vq.codebook.codebook_usage, usage)
    di = vq.perceptual_distance(x[:, :, 0], rec[:, :, 0], True, model)
    assert di.shape == (B, 1) and torch.equal(di[:, 0], d[:, 0])


# ---- 7. errors ----------------------------------------------------------------------------------------------------------

def test_errors(model):
    a = torch.zeros((2, 3, 32, 32))
    with pytest.raises(RuntimeError, match="GPU"):
        model(a, a)
    with pytest.raises(RuntimeError, match="GPU"):
        lpips.lpips_frames(a, a, model, layout="nchw")
    with pytest.raises(ValueError, match="shape"):
        model(a.cuda(), torch.zeros((2, 3, 32, 31)).cuda())
    with pytest.raises(ValueError, match="16"):
        model(torch.zeros((1, 3, 15, 64)).cuda(), torch.zeros((1, 3, 15, 64)).cuda())
    with pytest.raises(ValueError, match="16"):
        lpips.lpips_frames(torch.zeros((1, 3, 2, 64, 12)).cuda(), torch.zeros((1, 3, 2, 64, 12)).cuda(), model)
    with pytest.raises(TypeError):
        model(a.double().cuda(), a.double().cuda())
