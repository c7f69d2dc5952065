"""GPU (-m gpu): the Inception V3 layers (csrc/inception.hip), InceptionV3 (omnitokenizer_amd/inception.py) and FID
(omnitokenizer_amd/fid.py) against torch and against the reference's own features and Frechet distances
(tests/golden/fid_*.npz, make_golden_fid.py).

Bars (derived, not measured):
  PRE_BAR = 1e-6.  v = u / 255 is ToTensor's division (equal bits); the resize then runs with the arithmetic of i3d.hip's
    (frames.hip's BILINEAR mode), which differs from torch's CPU kernels in the order of the two lerps and their contraction:
    a few roundings of values <= 1, at most 4 * 2^-24 = 2.4e-7, doubled by 2 x - 1 (plus its own rounding, 6e-8).  Where no
    resize happens, or the size does not change (taps (v, 1, 0)), both sides compute the same roundings: equal bits.
  conv2d, per output element: one fp32 fma chain over k (and the bias add), so
    |y - y64| <= gamma_(K+1) * (sum_k |w_k x_k| + |bias|) + u |y64|, gamma_n = n u / (1 - n u), u = 2^-24, y64 the fp64
    evaluation of the same fp32 weights and inputs (F.conv2d + bias + ReLU; the ReLU does not increase it).
  maxpool2d: a max is exact; bit-identical to torch's max_pool2d (-inf padding), NaN included.
  avgpool2d: a sum of c <= k^2 terms and one division: |y - y64| <= gamma_c * sum|x| / c + u |y64| (c = the in-image taps).
  spatial_mean: the same with c = h w.
  FEATURE_BAR(dims) = sqrt(L) * sqrt(Kmax) * 2^-24 * 4 * max|act64|, L the fp32 layers on the longest path to the block
    (with the preprocess) and Kmax its largest reduction: (4, 288), (6, 720), (38, 2592), (50, 4032) for dims 64, 192, 768,
    2048.  Independent per-layer relative rounding errors of a K-term sum grow like sqrt(K) u and add in quadrature over the
    layers; 4 bounds sum |w x| / |y| at these activations.  tests/test_fid_cpu.py checks that the reference's own fp32 run
    is inside it.
  FID_BAR: the Frechet distance is W^2, W the 2-Wasserstein distance of the two fitted Gaussians.  Moving every activation
    by at most d moves each Gaussian by at most eps = d sqrt(D) sqrt(1 + 4 n / (n - 1)) in W, so
    |W'^2 - W^2| <= 2 eps (2 W + 2 eps) with d = FEATURE_BAR, plus sqrtm's own 1e-9 of the traces.
"""
import hashlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from omnitokenizer_amd import fid, i3d, inception, lpips, synth

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = 2.0 ** -24
PRE_BAR = 1e-6
FEATURE_CASES = ["fid_64x80", "fid_299x299"]
PATH = {64: (4, 288), 192: (6, 720), 768: (38, 2592), 2048: (50, 4032)}


def _gamma(n):
    return n * U / (1 - n * U)


def feature_bar(act64, dims):
    L, K = PATH[dims]
    return np.sqrt(L) * np.sqrt(K) * U * 4 * float(np.abs(act64).max())


def fid_bar(fid64, d, n, dim, traces):
    eps = d * np.sqrt(dim) * np.sqrt(1 + 4 * n / (n - 1))
    w = np.sqrt(max(fid64, 0.0))
    return 2 * eps * (2 * w + 2 * eps) + 1e-9 * traces


def _fix(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def _sets(f):
    from tests.golden.make_golden_fid import case_sets
    return case_sets(int(f["H"]), int(f["W"]), int(f["seed"]), int(f["noise_seed"]), int(f["other_seed"]), int(f["n"]))


@pytest.fixture(scope="module")
def weights():
    from tests.golden.make_golden_fid import WEIGHT_SEED
    return synth.synth_fid_inception_state_dict(WEIGHT_SEED)


@pytest.fixture(scope="module")
def models(weights):
    out = {}
    for d, b in inception.BLOCK_INDEX_BY_DIM.items():
        m = inception.InceptionV3([b])
        m.load_state_dict(weights)
        out[d] = m.cuda().eval()
    return out


# ---- preprocess ---------------------------------------------------------------------------------------------------------

def _torch_pre(x01, resize, normalize):
    if resize:
        x01 = F.interpolate(x01, size=(299, 299), mode="bilinear", align_corners=False)
    if normalize:
        x01 = 2 * x01 - 1
    return x01.permute(0, 2, 3, 1)


@pytest.mark.parametrize("shape", [(2, 64, 80), (1, 299, 299), (2, 300, 257), (3, 24, 24), (1, 256, 256)])
@pytest.mark.parametrize("resize,normalize", [(True, True), (False, True), (True, False), (False, False)])
def test_preprocess_matches_torch(shape, resize, normalize):
    N, H, W = shape
    u = torch.from_numpy(np.random.Generator(np.random.PCG64(H * W)).integers(0, 256, (N, H, W, 3), dtype=np.uint8))
    x01 = u.permute(0, 3, 1, 2).contiguous().to(torch.float32).div(255)    # ToTensor
    want = _torch_pre(x01, resize, normalize)
    for src in (u.cuda(), x01.cuda()):
        got = inception.preprocess_images(src, resize, normalize).cpu()
        assert got.shape == want.shape[:3] + (4,)
        assert torch.equal(got[..., 3], torch.zeros_like(got[..., 3]))
        if not resize or (H, W) == (299, 299):
            assert torch.equal(got[..., :3], want)
        err = (got[..., :3] - want).abs().max().item()
        assert err <= PRE_BAR, err


def test_preprocess_row_stride():
    """uint8 rows further apart than 3 W bytes (a column crop of wider images) read in place"""
    g = np.random.Generator(np.random.PCG64(3))
    wide = torch.from_numpy(g.integers(0, 256, (2, 40, 57, 3), dtype=np.uint8)).cuda()
    view = wide[:, :, 5:50]
    assert view.stride(1) == 57 * 3 and not view.is_contiguous()
    got = inception.preprocess_images(view).cpu()
    want = inception.preprocess_images(view.contiguous()).cpu()
    assert torch.equal(got, want)


# ---- conv2d -------------------------------------------------------------------------------------------------------------

def _conv_ref(x, w, b, s, p, relu, absolute=False):
    """fp64 F.conv2d + bias (+ ReLU) on channels-last x [N, H, W, C]; w [Cout, Cin, kh, kw]"""
    xc, w64, b64 = x.permute(0, 3, 1, 2).double(), w.double(), b.double()
    if absolute:
        xc, w64, b64 = xc.abs(), w64.abs(), b64.abs()
    y = F.conv2d(xc, w64, b64, stride=tuple(s), padding=tuple(p))
    if relu and not absolute:
        y = torch.relu(y)
    return y.permute(0, 2, 3, 1)


def _check_conv(N, H, W, cin, cout, k, s=(1, 1), p=(0, 0), relu=True, x_cs=None, x_off=0, y_cs=None, y_off=0, seed=0):
    g = torch.Generator().manual_seed(seed)
    x_cs = x_cs or cin
    x = torch.randn((N, H, W, x_cs), generator=g).abs()   # post-ReLU-like activations
    w = torch.randn((cout, cin) + tuple(k), generator=g) * (2.0 / (cin * np.prod(k))) ** 0.5
    b = 0.1 * torch.randn(cout, generator=g)
    xs = x[..., x_off:x_off + cin]
    want = _conv_ref(xs, w, b, s, p, relu)
    absum = _conv_ref(xs, w, b, s, p, False, absolute=True)
    wp = i3d.pack_conv_weight(w.unsqueeze(2)).cuda()
    Ho, Wo = want.shape[1:3]
    y_cs = y_cs or cout
    sentinel = 12345.0
    y = torch.full((N, Ho, Wo, y_cs), sentinel, device="cuda")
    inception.conv2d(x.cuda(), wp, b.cuda(), k, s, p, relu, cin=cin, x_off=x_off, out=y, out_off=y_off)
    y = y.cpu()
    got = y[..., y_off:y_off + cout].double()
    K = cin * int(np.prod(k))
    bar = _gamma(K + 1) * absum + U * want.abs()
    assert torch.isfinite(got).all()
    excess = ((got - want).abs() - bar).max().item()
    assert excess <= 0, f"conv {cin}->{cout} k{k} s{s} p{p} on {H}x{W}: error exceeds the bar by {excess:.3e}"
    rest = torch.cat([y[..., :y_off], y[..., y_off + cout:]], dim=-1)
    assert (rest == sentinel).all(), "channels outside the output slice were written"
    return got


def _network_layers(R=299):
    """(H, W, cin, cout, k, s, p) of every distinct conv launch of the network at an R x R input (the fused 1x1s as one)"""
    layers, h, w = [], R, R
    for blk, name, kind, convs in inception.NET:
        if kind == "conv":
            _, cin, cout, k, s, p = convs[0]
            layers.append((h, w, 4 if cin == 3 else cin, cout, k, s, p))
            h, w = inception.out_size(h, k[0], s[0], p[0]), inception.out_size(w, k[1], s[1], p[1])
            continue
        if kind == "pool":
            h, w = inception.out_size(h, 3, 2, 0), inception.out_size(w, 3, 2, 0)
            continue
        fused = inception.FUSED_1X1[kind]
        c = {cv[0]: cv for cv in convs}
        cin = convs[0][1]
        layers.append((h, w, cin, sum(c[n][2] for n in fused), (1, 1), (1, 1), (0, 0)))
        for cv in convs:
            if cv[0] not in fused:
                layers.append((h, w, cv[1], cv[2], cv[3], cv[4], cv[5]))
        if kind in ("B", "D"):
            h, w = inception.out_size(h, 3, 2, 0), inception.out_size(w, 3, 2, 0)
    return sorted(set(layers), key=layers.index)


@pytest.mark.parametrize("layer", _network_layers(),
                         ids=lambda l: f"{l[2]}-{l[3]}_k{l[4][0]}x{l[4][1]}s{l[5][0]}p{l[6][0]}{l[6][1]}_{l[0]}")
def test_conv_every_layer_shape(layer):
    H, W, cin, cout, k, s, p = layer
    _check_conv(1, H, W, cin, cout, k, s, p)


@pytest.mark.parametrize("ext", [(299, 299), (64, 81), (31, 30), (17, 17), (8, 9)])
def test_conv_stride2_no_padding(ext):
    """3 x 3 / stride 2 with no padding (Conv2d_1a, Mixed_6a, Mixed_7a) on odd and even extents: floor sizing"""
    H, W = ext
    _check_conv(2, H, W, 8, 40, (3, 3), (2, 2))
    if H > 100:
        _check_conv(1, H, W, 4, 32, (3, 3), (2, 2))


@pytest.mark.parametrize("k,p", [((1, 7), (0, 3)), ((7, 1), (3, 0)), ((1, 3), (0, 1)), ((3, 1), (1, 0)), ((5, 5), (2, 2)),
                                 ((3, 3), (1, 1))])
def test_conv_asymmetric_kernels_and_padding(k, p):
    _check_conv(2, 17, 13, 32, 48, k, (1, 1), p)
    _check_conv(1, 8, 8, 64, 96, k, (1, 1), p)


@pytest.mark.parametrize("cout", [8, 20, 32, 33, 48, 65, 200])
def test_conv_n_tails(cout):
    """Cout <= 32 takes the 256 x 32 tile; 33 and up the 64- and 128-wide ones"""
    _check_conv(3, 12, 13, 32, cout, (3, 3), (1, 1), (1, 1))
    _check_conv(3, 12, 13, 64, cout, (1, 1))


@pytest.mark.parametrize("cin,k", [(4, (3, 3)), (12, (1, 1)), (20, (3, 3)), (36, (1, 3)), (4, (1, 1)), (44, (7, 1))])
def test_conv_k_tails(cin, k):
    """K = taps * Cin not a multiple of 32"""
    _check_conv(2, 9, 11, cin, 48, k, (1, 1), (k[0] // 2, k[1] // 2))


def test_conv_channel_slices_and_no_relu():
    _check_conv(2, 14, 14, 24, 32, (3, 3), (1, 1), (1, 1), x_cs=64, x_off=20, y_cs=100, y_off=36)
    _check_conv(2, 14, 14, 16, 48, (1, 7), (1, 1), (0, 3), relu=False, x_cs=48, x_off=32, y_cs=52, y_off=3)
    _check_conv(2, 14, 14, 48, 20, (1, 1), relu=False, x_cs=112, x_off=64, y_cs=40, y_off=12)


def test_conv_split_routes_columns():
    """one 1x1 GEMM whose columns [0, split) go to y and the rest to y2 (the fused sibling 1x1s of a module)"""
    g = torch.Generator().manual_seed(5)
    x = torch.randn((2, 7, 7, 64), generator=g).abs().cuda()
    w = torch.randn((176, 64, 1, 1), generator=g) * 0.2
    b = (torch.randn(176, generator=g) * 0.1).cuda()
    wp = i3d.pack_conv_weight(w.unsqueeze(2)).cuda()
    y = torch.full((2, 7, 7, 300), 7.0, device="cuda")
    y2 = torch.full((2, 7, 7, 120), 7.0, device="cuda")
    inception.conv2d(x, wp, b, (1, 1), out=y, out_off=8, out2=y2, out2_off=4, split=64)
    full = inception.conv2d(x, wp, b, (1, 1))
    y, y2, full = y.cpu(), y2.cpu(), full.cpu()
    assert torch.equal(y[..., 8:72], full[..., :64]) and torch.equal(y2[..., 4:116], full[..., 64:])
    assert (y[..., :8] == 7).all() and (y[..., 72:] == 7).all() and (y2[..., :4] == 7).all() and (y2[..., 116:] == 7).all()


# ---- pools, spatial mean ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,s,p,ext", [(3, 2, 0, (147, 147)), (3, 2, 0, (71, 71)), (3, 2, 0, (35, 34)), (3, 2, 0, (17, 18)),
                                       (3, 1, 1, (8, 8)), (3, 1, 1, (5, 7)), (2, 2, 1, (6, 7))])
def test_maxpool_bit_exact(k, s, p, ext):
    g = torch.Generator().manual_seed(sum(ext))
    x = torch.randn((2,) + ext + (24,), generator=g) - 3.0     # mostly negative: the -inf padding matters
    x[0, 0, 0, :4] = float("nan")
    x[1, ext[0] // 2, ext[1] - 1, 8:12] = float("nan")
    want = F.max_pool2d(x.permute(0, 3, 1, 2), k, s, p).permute(0, 2, 3, 1)
    got = inception.maxpool2d(x.cuda(), k, s, p).cpu()
    assert got.shape == want.shape
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.isnan(want).any()
    assert torch.equal(torch.nan_to_num(got, 1e30), torch.nan_to_num(want, 1e30))
    # into a channel slice of a wider tensor (B's and D's pool branch)
    out = torch.full(want.shape[:3] + (40,), 5.0, device="cuda")
    inception.maxpool2d(x.cuda(), k, s, p, out=out, out_off=12)
    out = out.cpu()
    assert torch.equal(torch.nan_to_num(out[..., 12:36], 1e30), torch.nan_to_num(want, 1e30))
    assert (out[..., :12] == 5).all() and (out[..., 36:] == 5).all()


@pytest.mark.parametrize("ext", [(35, 35), (17, 17), (8, 8), (5, 3), (1, 1), (2, 6)])
def test_avgpool_count_exclude_pad(ext):
    g = torch.Generator().manual_seed(ext[0] * 7 + ext[1])
    x = torch.randn((2,) + ext + (32,), generator=g)
    xc = x.permute(0, 3, 1, 2).double()
    want = F.avg_pool2d(xc, 3, 1, 1, count_include_pad=False).permute(0, 2, 3, 1)
    absavg = F.avg_pool2d(xc.abs(), 3, 1, 1, count_include_pad=False).permute(0, 2, 3, 1)
    cnt = F.avg_pool2d(torch.ones_like(xc[:, :1]), 3, 1, 1, divisor_override=1).permute(0, 2, 3, 1)
    got = inception.avgpool2d(x.cuda(), 3, 1, 1).cpu().double()
    # the corner divides by 4, the edge by 6, the inside by 9 (on a 1 x 1 map by 1)
    if min(ext) >= 3:
        assert cnt[0, 0, 0, 0] == 4 and cnt[0, 0, 1, 0] == 6 and cnt[0, 1, 1, 0] == 9
    bar = torch.tensor([_gamma(int(c)) for c in cnt.flatten()], dtype=torch.float64).view(cnt.shape) * absavg + \
        U * want.abs()
    assert ((got - want).abs() <= bar).all(), ((got - want).abs() - bar).max().item()


@pytest.mark.parametrize("shape", [(3, 8, 8, 2048), (2, 17, 17, 768), (2, 35, 35, 192), (2, 73, 73, 64), (1, 1, 1, 64)])
def test_spatial_mean(shape):
    g = torch.Generator().manual_seed(shape[1])
    x = torch.randn(shape, generator=g).abs()
    got = inception.spatial_mean(x.cuda()).cpu().double()
    want = x.double().mean(dim=(1, 2))
    n = shape[1] * shape[2]
    bar = _gamma(n) * x.double().abs().mean(dim=(1, 2)) + U * want.abs()
    assert got.shape == want.shape and ((got - want).abs() <= bar).all()


# ---- the network and FID ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", FEATURE_CASES)
@pytest.mark.parametrize("dims", [64, 192, 768, 2048])
def test_features_match_reference_fp64(models, case, dims):
    f = _fix(case)
    want_all = f[f"act64_{dims}"]
    for i, u in enumerate(_sets(f)):
        got = fid.get_activations(u, models[dims], dims=dims, device="cuda")
        want = want_all[i]
        assert got.dtype == np.float64 and got.shape == want.shape
        err, bar = np.abs(got - want).max(), feature_bar(want_all, dims)
        assert err <= bar, f"{case} dims {dims} set {i}: error {err:.3e} > bar {bar:.3e}"
        if i == 0:
            # the reference's forward on ToTensor's fp32 [N, 3, H, W] gives the same bits, as does a CUDA uint8 input
            x01 = torch.from_numpy(u).permute(0, 3, 1, 2).contiguous().float().div(255).cuda()
            out = models[dims](x01)[0]
            assert out.shape[:2] == (u.shape[0], dims)
            pooled = out.mean(dim=(2, 3)) if dims != 2048 else out[:, :, 0, 0]
            assert np.array_equal(fid.get_activations(x01, models[dims], dims=dims, device="cuda"), got)
            assert np.array_equal(fid.get_activations(torch.from_numpy(u).cuda(), models[dims], dims=dims), got)
            assert np.abs(pooled.cpu().double().numpy() - got).max() <= bar


def test_fid_matches_reference(models):
    f = _fix("fid_dist_d64")
    sets = _sets(f)
    act = [fid.get_activations(torch.from_numpy(u).cuda(), models[64], dims=64, device="cuda") for u in sets]
    d = feature_bar(f["act64"], 64)
    assert max(np.abs(a - w).max() for a, w in zip(act, f["act64"])) <= d
    st = [(np.mean(a, axis=0), np.cov(a, rowvar=False)) for a in act]
    for j, (a, b) in enumerate([(0, 1), (0, 2), (0, 0)]):
        got = fid.calculate_frechet_distance(*st[a], *st[b])
        want = float(f["fid64"][j])
        bar = fid_bar(want, d, int(f["n"]), 64, np.trace(st[a][1]) + np.trace(st[b][1]))
        assert abs(got - want) <= bar, f"pair {j}: FID {got} vs reference {want}, bar {bar:.3e}"
    assert fid.compute_fid(sets[0], sets[1], models[64], dims=64) == \
        fid.calculate_frechet_distance(*st[0], *st[1])


def test_fid_given_paths_and_saved_stats(models, tmp_path):
    """the folder path (PNG files read with PIL, in subfolders or not) and .npz statistics give the same numbers as the
    arrays"""
    from PIL import Image
    f = _fix("fid_dist_d64")
    sets = _sets(f)[:2]
    dirs = []
    for i, u in enumerate(sets):
        d = tmp_path / f"set{i}" / ("sub" if i else "")
        d.mkdir(parents=True, exist_ok=True)
        for j, img in enumerate(u):
            Image.fromarray(img).save(d / f"{j:04d}.png")
        dirs.append(str(tmp_path / f"set{i}"))
    want = fid.compute_fid(sets[0], sets[1], models[64], dims=64)
    got = fid.calculate_fid_given_paths(dirs, 50, "cuda", 64, model=models[64])
    assert got == want
    assert abs(got - float(f["fid_paths"])) <= fid_bar(float(f["fid64"][0]), feature_bar(f["act64"], 64), int(f["n"]),
                                                       64, 2 * np.trace(np.cov(f["act64"][0], rowvar=False)))
    npz = str(tmp_path / "s0.npz")
    fid.save_fid_stats([dirs[0], npz], 50, "cuda", 64, model=models[64])
    assert fid.calculate_fid_given_paths([npz, dirs[1]], 50, "cuda", 64, model=models[64]) == got


def test_batch_invariance(models):
    f = _fix("fid_299x299")
    s = _sets(f)
    imgs = torch.from_numpy(np.concatenate(list(s) * 3)[:50]).cuda()   # 50 images
    m = models[2048]
    alone = fid.get_activations(imgs[7:8], m, device="cuda")
    five = fid.get_activations(imgs[3:8], m, device="cuda")
    fifty = fid.get_activations(imgs, m, device="cuda")
    small_batches = fid.get_activations(imgs, m, batch_size=7, device="cuda")
    assert np.array_equal(alone[0], fifty[7]) and np.array_equal(five[4], fifty[7])
    assert np.array_equal(small_batches, fifty)


def test_vqgan_eval_image_loop_on_device(models):
    """vqgan_eval.py:170-238 without the PNG round trip: encode -> decode_frames(ids, True) -> uint8 images -> Inception
    features -> FID, on the device; the reference's numpy uint8 path gives the same number"""
    from omnitokenizer_amd import OmniTokenizer_VQGAN, make_args
    from omnitokenizer_amd.config import OmniTokConfig
    from omnitokenizer_amd.frames import pixels_to_frames
    args = make_args(2, resolution=64)
    tok = OmniTokenizer_VQGAN(args)
    tok.load_state_dict(synth.synth_state_dict(OmniTokConfig.from_args(args), seed=0), strict=True)
    tok = tok.cuda().eval()
    n = 80    # more images than dims: full-rank covariances
    x = synth.synth_video(n, 1, 64, seed=98, kind="natural")[:, :, 0].contiguous().cuda()
    with torch.no_grad():
        ids = tok.encode(x, True)
        real_u8 = pixels_to_frames(x, "thwc")
        fake_u8 = tok.decode_frames(ids, True)
    assert real_u8.is_cuda and fake_u8.is_cuda and fake_u8.shape == (n, 64, 64, 3) and fake_u8.dtype == torch.uint8
    got = fid.compute_fid(real_u8, fake_u8, models[64], dims=64)
    host = fid.compute_fid(real_u8.cpu().numpy(), fake_u8.cpu().numpy(), models[64], dims=64)
    assert np.isfinite(got) and got > 0
    assert got == host


# ---- the I3D entry points after the conv refactor -----------------------------------------------------------------------

def i3d_digests():
    """sha256 of conv3d_same's outputs on seeded inputs (every tile of the conv3d rule, a split, a slice) and of the I3D
    logits of a fixture set: the bits of the I3D path"""
    from tests.golden.make_golden_fvd import WEIGHT_SEED, case_sets
    out = {}
    for cfg in [(1, 5, 14, 14, 64, 176, (1, 1, 1), (1, 1, 1)), (2, 9, 28, 28, 64, 256, (3, 3, 3), (1, 1, 1)),
                (1, 9, 40, 52, 4, 64, (7, 7, 7), (2, 2, 2)), (2, 4, 7, 7, 832, 48, (3, 3, 3), (1, 1, 1))]:
        B, T, H, W, cin, cout, k, s = cfg
        g = torch.Generator().manual_seed(cin * cout)
        x = torch.randn((B, T, H, W, cin), generator=g).abs().cuda()
        w = torch.randn((cout, cin) + k, generator=g) * (2.0 / (cin * np.prod(k))) ** 0.5
        b = (0.1 * torch.randn(cout, generator=g)).cuda()
        y = i3d.conv3d_same(x, i3d.pack_conv_weight(w).cuda(), b, k, s)
        out[f"conv3d_{cin}-{cout}_k{k[0]}s{s[0]}"] = hashlib.sha256(y.cpu().numpy().tobytes()).hexdigest()[:16]
    from omnitokenizer_amd import fvd
    m = i3d.InceptionI3d(400)
    m.load_state_dict(synth.synth_i3d_state_dict(WEIGHT_SEED))
    m = m.cuda().eval()
    u = case_sets(17, 40, 52, 11, 12, 13, n=4)[0]
    out["i3d_logits"] = hashlib.sha256(fvd.get_fvd_logits(u, m, "cuda").cpu().numpy().tobytes()).hexdigest()[:16]
    return out


# recorded on an MI355X with the library of the commit before csrc/i3d_common.h (the kernel then lived in csrc/i3d.hip)
I3D_DIGESTS = {"conv3d_4-64_k7s2": "a8065e1a95892765", "conv3d_64-176_k1s1": "80d48644261dc9a9",
               "conv3d_64-256_k3s1": "2bfa5f497037c7e3", "conv3d_832-48_k3s1": "e1a6a4323e272feb",
               "i3d_logits": "bfff322b889509b4"}


def test_i3d_bits_unchanged_by_the_shared_conv():
    assert i3d_digests() == I3D_DIGESTS


# ---- Inception V3 and LPIPS after their operators and weight scaffold moved to one module -------------------------------

def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().cpu().numpy().tobytes())
    return h.hexdigest()[:16]


def inception_digests():
    """sha256 of all four block outputs of 2 seeded images, at the least input that reaches block 3 without the resize and
    from 64 x 64 with it: every module kind, every fused 1x1 split and every channel-slice offset of InceptionV3"""
    from tests.golden.make_golden_fid import WEIGHT_SEED
    sd, out = synth.synth_fid_inception_state_dict(WEIGHT_SEED), {}
    for tag, resize, size in (("native", False, inception.min_input_size(3)), ("resized", True, 64)):
        m = inception.InceptionV3((0, 1, 2, 3), resize_input=resize)
        m.load_state_dict(sd)
        x = torch.rand((2, 3, size, size), generator=torch.Generator().manual_seed(size))
        for blk, o in zip(m.output_blocks, m.cuda().eval()(x.cuda())):
            out[f"inception_{tag}_block{blk}"] = _sha(o)
    return out


def lpips_digests():
    """sha256 of the LPIPS distances of 2 seeded pairs at the least frame size and at 32 x 48: the VGG16 trunk's 13 convs
    and 4 pools, the heads and the ScalingLayer constants"""
    m, out = lpips.load_lpips("cuda", synth.synth_lpips_state_dict(7)), {}
    for H, W in ((lpips.MIN_SIZE, lpips.MIN_SIZE), (32, 48)):
        g = torch.Generator().manual_seed(H * W)
        a, b = (torch.rand((2, 3, H, W), generator=g) - 0.5 for _ in range(2))
        out[f"lpips_{H}x{W}"] = _sha(m(a.cuda(), b.cuda()))
    return out


# recorded on an MI355X with the library and the Python of the commit before omnitokenizer_amd/convnet.py
INCEPTION_DIGESTS = {"inception_native_block0": "3328f1e55918f8d9", "inception_native_block1": "8c01f2b873080d76",
                     "inception_native_block2": "64f513b612c2c9eb", "inception_native_block3": "83ab1aec0be55dac",
                     "inception_resized_block0": "1788cf9f17e1471e", "inception_resized_block1": "3a4a4c55429a5158",
                     "inception_resized_block2": "820e12734c78a8cc", "inception_resized_block3": "389fb158df0b8aae"}
LPIPS_DIGESTS = {"lpips_16x16": "5a96543106042317", "lpips_32x48": "dd0099ed48a32cbf"}


def test_inception_bits_unchanged_by_the_shared_module():
    assert inception_digests() == INCEPTION_DIGESTS


def test_lpips_bits_unchanged_by_the_shared_module():
    assert lpips_digests() == LPIPS_DIGESTS
