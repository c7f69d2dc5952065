"""GPU (-m gpu): the I3D layers (csrc/i3d.hip), InceptionI3d (omnitokenizer_amd/i3d.py) and FVD (omnitokenizer_amd/fvd.py)
against torch and against the reference's own logits and Frechet distances (tests/golden/fvd_*.npz, make_golden_fvd.py).

Bars (derived, not measured):
  PRE_BAR = 1e-6.  The resize runs on 0..255 with the arithmetic of frames.hip's BILINEAR mode; torch's CPU kernels differ from
    it (and among themselves, by dispatch) in the order of the two lerps and their contraction: a few roundings of values
    <= 255, at most 4 * 2^-24 * 255 = 6e-5 before the scaling by 2 / 255, 5e-7 after it.  Where the size does not change the
    taps are (v, 1, 0), both sides compute 2 v / 255 - 1 with the same roundings: equal bits.
  conv3d_same, per output element: the kernel is one fp32 fma chain over k (and the bias add), so
    |y - y64| <= gamma_(K+1) * (sum_k |w_k x_k| + |bias|) + u |y64|, gamma_n = n u / (1 - n u), u = 2^-24, where y64 is the
    fp64 evaluation of the same fp32 weights and inputs (F.pad + F.conv3d + bias + ReLU; the ReLU does not increase it).
  maxpool3d_same: a max is exact; bit-identical to torch's F.pad + max_pool3d on the same input.
  i3d_head: the 98-term pool sum (gamma_98 of its |.| sum), the division, the C-term logits chain and the mean over T':
    |out - out64| <= (gamma_(C+100) + 2u) * (|W| . pool(|x|) + |bias|) per pooled step, which the mean does not grow.
  LOGIT_BAR(ref) = sqrt(L) * sqrt(Kmax) * 2^-24 * 4 * max|logits64|, L = 23 fp32 layers on the longest path (Conv3d_1a, 2b,
    2c, two per Mixed module, pool + logits), Kmax = 27 * 192 = 5184 (Mixed_5c.b1b): independent per-layer relative rounding
    errors of a K-term sum grow like sqrt(K) u and add in quadrature over layers; 4 bounds sum |w x| / |y| at these
    activations.  tests/test_fvd_cpu.py checks that the reference's own fp32 run is inside it.
  FVD_BAR: the Frechet distance is W^2, W the 2-Wasserstein distance of the two fitted Gaussians.  Moving every logit by at
    most d moves each Gaussian (mean m, covariance A^T A, A = centred logits / sqrt(n - 1)) by at most
    eps = d sqrt(D) sqrt(1 + 4 n / (n - 1)) in W (couple both through the same n-dim normal), D = 400.  So
    |W'^2 - W^2| <= 2 eps (2 W + 2 eps) with d = LOGIT_BAR.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from omnitokenizer_amd import fvd, i3d, synth

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = 2.0 ** -24
PRE_BAR = 1e-6
CASES = ["fvd_t17_40x52", "fvd_t16_64x64"]


def _gamma(n):
    return n * U / (1 - n * U)


def logit_bar(logits64):
    return np.sqrt(23) * np.sqrt(27 * 192) * U * 4 * float(np.abs(logits64).max())


def fvd_bar(fvd64, d, n, dim=400):
    eps = d * np.sqrt(dim) * np.sqrt(1 + 4 * n / (n - 1))
    w = np.sqrt(max(fvd64, 0.0))
    return 2 * eps * (2 * w + 2 * eps)


def _fix(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


@pytest.fixture(scope="module")
def model():
    from tests.golden.make_golden_fvd import WEIGHT_SEED
    m = i3d.InceptionI3d(400, in_channels=3)
    m.load_state_dict(synth.synth_i3d_state_dict(WEIGHT_SEED))
    return m.cuda().eval()


def _sets(f):
    from tests.golden.make_golden_fvd import case_sets
    return case_sets(int(f["T"]), int(f["H"]), int(f["W"]), int(f["seed"]), int(f["noise_seed"]), int(f["other_seed"]),
                     int(f["n"]))


# ---- preprocess ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(2, 3, 40, 52), (1, 2, 64, 64), (1, 2, 300, 257), (2, 3, 224, 224)])
def test_preprocess_matches_torch(shape):
    B, T, H, W = shape
    u = torch.from_numpy(np.random.Generator(np.random.PCG64(H * W)).integers(0, 256, (B, T, H, W, 3), dtype=np.uint8))
    frames = u.float().flatten(end_dim=1).permute(0, 3, 1, 2).contiguous()
    want = F.interpolate(frames, size=(224, 224), mode="bilinear", align_corners=False)
    want = (2. * want / 255. - 1).view(B, T, 3, 224, 224).permute(0, 1, 3, 4, 2)
    got = i3d.preprocess_frames(u.cuda()).cpu()
    assert got.shape == (B, T, 224, 224, 4)
    assert torch.equal(got[..., 3], torch.zeros_like(got[..., 3]))
    err = (got[..., :3] - want).abs().max().item()
    if (H, W) == (224, 224):
        assert torch.equal(got[..., :3], want), err
    assert err <= PRE_BAR, err


# ---- conv3d_same --------------------------------------------------------------------------------------------------------

def _conv_ref(x, w, b, k, s, relu, absolute=False):
    """fp64 F.pad + F.conv3d + bias (+ ReLU) on channels-last x [B, T, H, W, C]; w [Cout, Cin, k]"""
    xc = x.permute(0, 4, 1, 2, 3).double()
    pads = []
    for e, kk, ss in zip(reversed(xc.shape[2:]), reversed(k), reversed(s)):
        pad = max(kk - (e % ss or ss), 0)
        pads += [pad // 2, pad - pad // 2]
    xc = F.pad(xc, pads)
    w64, b64 = w.double(), b.double()
    if absolute:
        xc, w64, b64 = xc.abs(), w64.abs(), b64.abs()
    y = F.conv3d(xc, w64, b64, stride=tuple(s))
    if relu and not absolute:
        y = torch.relu(y)
    return y.permute(0, 2, 3, 4, 1)


def _check_conv(B, T, H, W, cin, cout, k, s, relu=True, x_cs=None, x_off=0, y_cs=None, y_off=0, seed=0):
    g = torch.Generator().manual_seed(seed)
    x_cs = x_cs or cin
    x = torch.randn((B, T, H, W, x_cs), generator=g).abs()   # post-ReLU-like activations
    w = torch.randn((cout, cin) + tuple(k), generator=g) * (2.0 / (cin * np.prod(k))) ** 0.5
    b = 0.1 * torch.randn(cout, generator=g)
    xs = x[..., x_off:x_off + cin]
    want = _conv_ref(xs, w, b, k, s, relu)
    absum = _conv_ref(xs, w, b, k, s, False, absolute=True)
    wp = i3d.pack_conv_weight(w).cuda()
    To, Ho, Wo = want.shape[1:4]
    y_cs = y_cs or cout
    sentinel = 12345.0
    y = torch.full((B, To, Ho, Wo, y_cs), sentinel, device="cuda")
    i3d.conv3d_same(x.cuda(), wp, b.cuda(), k, s, relu, cin=cin, x_off=x_off, out=y, out_off=y_off)
    y = y.cpu()
    got = y[..., y_off:y_off + cout].double()
    K = cin * int(np.prod(k))
    bar = _gamma(K + 1) * absum + U * want.abs()
    assert torch.isfinite(got).all()
    excess = ((got - want).abs() - bar).max().item()
    assert excess <= 0, f"conv {cin}->{cout} k{k} s{s} on {T}x{H}x{W}: error exceeds the bar by {excess:.3e}"
    rest = torch.cat([y[..., :y_off], y[..., y_off + cout:]], dim=-1)
    assert (rest == sentinel).all(), "channels outside the output slice were written"
    return got


def _network_layers(T=17, R=224):
    """(T, H, W, cin, cout, k, s) of every conv of the network at a T x R x R input"""
    layers = []
    ext = (T, R, R)
    for p in i3d.PLAN:
        if p[0] == "unit":
            cin = 4 if p[2] == 3 else p[2]
            layers.append((*ext, cin, p[3], p[4], p[5]))
            ext = tuple(i3d.same_pad(e, kk, ss)[1] for e, kk, ss in zip(ext, p[4], p[5]))
        elif p[0] == "pool":
            ext = tuple(i3d.same_pad(e, kk, ss)[1] for e, kk, ss in zip(ext, p[2], p[3]))
        else:
            cin, c = i3d.MIXED[p[1]]
            layers += [(*ext, cin, c[0] + c[1] + c[3], (1, 1, 1), (1, 1, 1)), (*ext, c[1], c[2], (3, 3, 3), (1, 1, 1)),
                       (*ext, c[3], c[4], (3, 3, 3), (1, 1, 1)), (*ext, cin, c[5], (1, 1, 1), (1, 1, 1))]
    return layers


@pytest.mark.parametrize("layer", _network_layers(), ids=lambda l: f"{l[3]}-{l[4]}_k{l[5][0]}s{l[6][0]}_{l[0]}x{l[1]}")
def test_conv_every_layer_shape(layer):
    T, H, W, cin, cout, k, s = layer
    _check_conv(1, T, H, W, cin, cout, k, s)


@pytest.mark.parametrize("ext", [(17, 224, 224), (16, 223, 222), (9, 31, 30), (8, 15, 16)])
def test_conv_stride2_asymmetric_pads(ext):
    """7^3 / stride 2 (Conv3d_1a: front 2, back 3 on 224; 3 / 3 on 17) and 3^3 / stride 2 on odd and even extents"""
    T, H, W = ext
    if H >= 200:
        assert i3d.same_pad(224, 7, 2) == (2, 112) and i3d.same_pad(17, 7, 2) == (3, 9)
        _check_conv(1, T, H, W, 4, 64, (7, 7, 7), (2, 2, 2))
    else:
        _check_conv(2, T, H, W, 8, 40, (3, 3, 3), (2, 2, 2))
        _check_conv(2, T, H, W, 4, 16, (7, 7, 7), (2, 2, 2))


@pytest.mark.parametrize("cout", [16, 24, 48, 65, 200])
def test_conv_n_tails(cout):
    _check_conv(3, 5, 12, 13, 32, cout, (3, 3, 3), (1, 1, 1))
    _check_conv(3, 5, 12, 13, 64, cout, (1, 1, 1), (1, 1, 1))


@pytest.mark.parametrize("cin,k", [(4, (3, 3, 3)), (12, (1, 1, 1)), (20, (3, 3, 3)), (36, (1, 3, 3)), (4, (1, 1, 1))])
def test_conv_k_tails(cin, k):
    """K = taps * Cin not a multiple of 32"""
    _check_conv(2, 4, 9, 11, cin, 48, k, (1, 1, 1))


def test_conv_channel_slices_and_no_relu():
    _check_conv(2, 5, 14, 14, 24, 32, (3, 3, 3), (1, 1, 1), x_cs=64, x_off=20, y_cs=100, y_off=36)
    _check_conv(2, 5, 14, 14, 16, 48, (1, 1, 1), (1, 1, 1), relu=False, x_cs=48, x_off=32, y_cs=52, y_off=3)


def test_conv_split_routes_columns():
    """one 1x1x1 GEMM whose columns [0, split) go to y and the rest to y2 (the fused b0 | b1a | b2a)"""
    g = torch.Generator().manual_seed(5)
    x = torch.randn((2, 4, 7, 7, 64), generator=g).abs()
    w = torch.randn((80, 64, 1, 1, 1), generator=g) * 0.2
    b = torch.randn(80, generator=g) * 0.1
    y = torch.full((2, 4, 7, 7, 100), 7.0, device="cuda")
    y2 = torch.full((2, 4, 7, 7, 56), 7.0, device="cuda")
    i3d.conv3d_same(x.cuda(), i3d.pack_conv_weight(w).cuda(), b.cuda(), (1, 1, 1), out=y, out_off=10, out2=y2,
                    out2_off=8, split=32)
    full = torch.empty((2, 4, 7, 7, 80), device="cuda")
    i3d.conv3d_same(x.cuda(), i3d.pack_conv_weight(w).cuda(), b.cuda(), (1, 1, 1), out=full)
    y, y2, full = y.cpu(), y2.cpu(), full.cpu()
    assert torch.equal(y[..., 10:42], full[..., :32]) and torch.equal(y2[..., 8:56], full[..., 32:])
    assert (y[..., :10] == 7).all() and (y[..., 42:] == 7).all() and (y2[..., :8] == 7).all()


# ---- maxpool, head ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,s,ext", [((1, 3, 3), (1, 2, 2), (9, 112, 112)), ((1, 3, 3), (1, 2, 2), (9, 57, 55)),
                                     ((3, 3, 3), (2, 2, 2), (9, 28, 28)), ((3, 3, 3), (2, 2, 2), (8, 27, 29)),
                                     ((2, 2, 2), (2, 2, 2), (5, 14, 14)), ((2, 2, 2), (2, 2, 2), (4, 13, 15)),
                                     ((3, 3, 3), (1, 1, 1), (5, 14, 14))])
def test_maxpool_bit_exact(k, s, ext):
    g = torch.Generator().manual_seed(sum(ext))
    x = torch.randn((2,) + ext + (24,), generator=g)   # signed: the zero padding matters
    got = i3d.maxpool3d_same(x.cuda(), k, s).cpu()
    xc = x.permute(0, 4, 1, 2, 3)
    pads = []
    for e, kk, ss in zip(reversed(ext), reversed(k), reversed(s)):
        pad = max(kk - (e % ss or ss), 0)
        pads += [pad // 2, pad - pad // 2]
    want = F.max_pool3d(F.pad(xc, pads), k, s).permute(0, 2, 3, 4, 1)
    assert got.shape == want.shape and torch.equal(got, want)


@pytest.mark.parametrize("ext", [(3, 7, 7), (2, 7, 7), (4, 9, 8)])
def test_head(ext):
    g = torch.Generator().manual_seed(1)
    C, ncls = 1024, 400
    x = torch.randn((3,) + ext + (C,), generator=g).abs()
    w = torch.randn((ncls, C), generator=g) / 32
    b = torch.randn(ncls, generator=g) * 0.1
    got = i3d.i3d_head(x.cuda(), w.t().contiguous().cuda(), b.cuda()).cpu().double()

    def ref(xx, ww, bb):
        p = F.avg_pool3d(xx.permute(0, 4, 1, 2, 3).double(), (2, 7, 7), stride=1)
        return F.conv3d(p, ww.double().view(ncls, C, 1, 1, 1), bb.double()).mean(dim=2)
    want = ref(x, w, b)
    bar = (_gamma(C + 100) + 2 * U) * ref(x.abs(), w.abs(), b.abs())
    assert got.shape == want.shape
    assert ((got - want).abs() <= bar).all(), ((got - want).abs() - bar).max().item()


# ---- the network and FVD ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES)
def test_logits_match_reference_fp64(model, case):
    f = _fix(case)
    for i, u in enumerate(_sets(f)):
        got = fvd.get_fvd_logits(u, model, "cuda").cpu().double().numpy()
        want = f["logits64"][i]
        assert got.shape == want.shape
        err, bar = np.abs(got - want).max(), logit_bar(f["logits64"])
        assert err <= bar, f"{case} set {i}: logits error {err:.3e} > bar {bar:.3e}"
        # forward() on the reference's [B, 3, T, 224, 224] input gives the same bits
        if i == 0:
            x = fvd.preprocess(u, device="cuda")
            assert np.array_equal(model(x).cpu().double().numpy(), got)


@pytest.mark.parametrize("case", CASES)
def test_fvd_matches_reference_fp64(model, case):
    f = _fix(case)
    sets = _sets(f)
    emb = [fvd.get_fvd_logits(torch.from_numpy(u).cuda(), model, "cuda") for u in sets]
    d = logit_bar(f["logits64"])
    for j, (a, b) in enumerate([(0, 1), (0, 2), (0, 0)]):
        got = fvd.frechet_distance(emb[a], emb[b]).item()
        want = float(f["fvd64"][j])
        bar = fvd_bar(want, d, int(f["n"]))
        assert abs(got - want) <= bar, f"{case} pair {j}: FVD {got} vs reference {want}, bar {bar:.3e}"
    assert fvd.compute_fvd(sets[0], sets[1], model, "cuda").item() == fvd.frechet_distance(emb[0], emb[1]).item()


def test_batch_invariance(model):
    f = _fix("fvd_t17_40x52")
    s = _sets(f)
    clips = torch.from_numpy(np.concatenate([s[0], s[2]])).cuda()   # 16 clips
    alone = fvd.get_fvd_logits(clips[3:4], model, "cuda").cpu()
    five = fvd.get_fvd_logits(clips[:5], model, "cuda").cpu()
    sixteen = fvd.get_fvd_logits(clips, model, "cuda").cpu()
    assert torch.equal(alone[0], five[3]) and torch.equal(alone[0], sixteen[3])
    assert torch.equal(five, sixteen[:5])


def test_vqgan_eval_loop_on_device(model):
    """vqgan_eval.py:141-164: encode -> decode -> uint8 frames -> I3D logits -> Frechet distance, all on the device; the
    reference's numpy uint8 path gives the same bits"""
    from omnitokenizer_amd import OmniTokenizer_VQGAN, make_args
    from omnitokenizer_amd.config import OmniTokConfig
    from omnitokenizer_amd.frames import pixels_to_frames
    args = make_args(2, resolution=64)
    tok = OmniTokenizer_VQGAN(args)
    tok.load_state_dict(synth.synth_state_dict(OmniTokConfig.from_args(args), seed=0), strict=True)
    tok = tok.cuda().eval()
    x = synth.synth_video(4, 9, 64, seed=99, kind="natural").cuda()
    with torch.no_grad():
        ids = tok.encode(x, False)
        real_u8 = pixels_to_frames(x, "thwc")
        fake_u8 = tok.decode_frames(ids, False, layout="thwc")
    assert real_u8.is_cuda and fake_u8.is_cuda and fake_u8.shape == (4, 9, 64, 64, 3)
    real = fvd.get_fvd_logits(real_u8, model, "cuda")
    fake = fvd.get_fvd_logits(fake_u8, model, "cuda")
    got = fvd.frechet_distance(real, fake)
    host = fvd.frechet_distance(fvd.get_fvd_logits(real_u8.cpu().numpy(), model, "cuda"),
                                fvd.get_fvd_logits(fake_u8.cpu().numpy(), model, "cuda"))
    assert torch.isfinite(got) and got.item() > 0
    assert got.item() == host.item()
