"""GPU (-m gpu): reconstruction metrics (csrc/metrics.hip, omnitokenizer_amd/metrics.py, reconstruction_metrics)
against the reference's own PSNR / SSIM (tests/golden/metrics_*.npz, make_golden_metrics.py) and an fp64 torch oracle.

Bars (derived, not measured):
  PSNR_BAR = 1e-5 dB.  The reference's mse is numpy's float32 pairwise mean of n = 3 H W squares: 8 accumulators of up to 16
    adds each (16 roundings), their 8-way combine (3 more), the pairwise tree above blocks of 128 (ceil(log2(n / 128))) and
    the division (1): relative error <= (20 + ceil(log2(n / 128))) 2^-24.  At n = 3 * 256^2 that is 31 * 2^-24 = 1.8e-6;
    PSNR = -10 log10(mse) moves by (10 / ln 10) * rel = 4.34 * 1.8e-6 = 8e-6 dB < 1e-5.  The kernel's own sum (fp64 over
    the same fp32 squares) adds nothing visible.
  SSIM_BAR = 1e-9.  Separable (11 + 11 taps) and 2-D (121 products of the rounded outer-product window) filtering differ by
    at most about 121 * 2^-53 = 1.4e-14 per filtered value (every value and weight sum is <= 1).  The map
    N / D = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)) has |dmap/dmu| <= 2 / sqrt(C1) = 200
    (2 mu / (mu^2 + C1) <= 1 / sqrt(C1), |2 s12 + C2| <= s1 + s2 + C2) and |dmap/ds| <= 2 / C2 = 2.3e3 for each of s1, s2,
    s12, whose error is that of E[.] plus that of mu^2: 2 * 200 * 1.4e-14 + 3 * 2.3e3 * 2.8e-14 = 2e-10 per map value at
    worst.  The means over the map and the channels do not grow it; 1e-9 leaves a margin of 5.
"""
import os

import numpy as np
import pytest
import torch

from omnitokenizer_amd import metrics as mt

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U8_FIXTURES = ["metrics_video", "metrics_odd", "metrics_11x11", "metrics_10x12", "metrics_image", "metrics_identical",
               "metrics_offset", "metrics_noise"]
PSNR_BAR, SSIM_BAR = 1e-5, 1e-9


def _unit(u):
    """u / 255 in fp32 with IEEE division: a table divided on the CPU (the bits of the kernel's table; a division by a
    scalar on the GPU may be a multiplication by its reciprocal), gathered on u's device"""
    table = (torch.arange(256, dtype=torch.float32) / 255).to(u.device)
    return table[u.long()]


def _fix(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def _close(got, want, bar, what):
    got = got.cpu().double()
    want = torch.as_tensor(want, dtype=torch.float64)
    assert got.shape == want.shape, what
    assert torch.equal(torch.isnan(got), torch.isnan(want)), what
    fin = ~torch.isnan(want)
    err = (got[fin] - want[fin]).abs().max().item() if fin.any() else 0.0
    assert err <= bar, f"{what}: max |diff| {err:.3e} > {bar:.0e}"


@pytest.mark.parametrize("name", U8_FIXTURES)
def test_fixtures_uint8_and_fp32(name):
    g = _fix(name)
    u8a, u8b = torch.from_numpy(g["u8a"]).cuda(), torch.from_numpy(g["u8b"]).cuda()
    p8, s8 = mt.psnr_ssim(u8a, u8b, layout="bthwc")
    assert p8.dtype == torch.float64 and p8.shape == g["psnr"].shape and p8.device == u8a.device
    _close(p8, g["psnr"], PSNR_BAR, name + " psnr")
    _close(s8, g["ssim"], SSIM_BAR, name + " ssim")
    # the reference's own layout and dtype: u8 / 255 in fp32, [B,T,3,H,W]
    fa, fb = [_unit(u).permute(0, 1, 4, 2, 3).contiguous() for u in (u8a, u8b)]
    pf, sf = mt.psnr_ssim(fa, fb)
    assert torch.equal(pf, p8) and torch.equal(sf.nan_to_num(-7.0), s8.nan_to_num(-7.0)), name
    if name == "metrics_identical":
        assert (p8 == 100).all() and (s8 == 1.0).all()
    if name == "metrics_10x12":
        assert torch.isnan(s8).all() and torch.isfinite(p8).all()
    if name == "metrics_image":   # 4-D images: one frame
        p4, s4 = mt.psnr_ssim(u8a[:, 0], u8b[:, 0], layout="bthwc")
        assert torch.equal(p4, p8) and torch.equal(s4, s8)


def test_fixture_float_fused_shift_and_clamp():
    g = _fix("metrics_float")
    xa, xb = torch.from_numpy(g["xa"]).cuda(), torch.from_numpy(g["xb"]).cuda()
    p, s = mt.reconstruction_psnr_ssim(xa, xb, False)
    _close(p, g["psnr"], PSNR_BAR, "float psnr")
    _close(s, g["ssim"], SSIM_BAR, "float ssim")
    pe, se = mt.psnr_ssim(xa + 0.5, torch.clamp(xb + 0.5, 0, 1), layout="bcthw")
    assert torch.equal(p, pe) and torch.equal(s, se)


@pytest.mark.parametrize("name", ["metrics_video", "metrics_odd", "metrics_noise", "metrics_float"])
def test_drop_in_dicts(name):
    g = _fix(name)
    if "u8a" in g:
        v1, v2 = [_unit(torch.from_numpy(g[k]).cuda()).permute(0, 1, 4, 2, 3) for k in ("u8a", "u8b")]
    else:
        v1 = (torch.from_numpy(g["xa"]).cuda() + 0.5).permute(0, 2, 1, 3, 4)
        v2 = torch.clamp(torch.from_numpy(g["xb"]).cuda() + 0.5, 0, 1).permute(0, 2, 1, 3, 4)
    rp, rs = mt.calculate_psnr(v1, v2), mt.calculate_ssim(v1, v2)
    T = v1.shape[1]
    for r in (rp, rs):
        assert set(r) == {"value", "value_std", "video_setting", "video_setting_name"}
        assert list(r["value"]) == list(range(T)) and list(r["value_std"]) == list(range(T))
        assert tuple(r["video_setting"]) == tuple(v1.shape[1:])
        assert r["video_setting_name"] == "time, channel, heigth, width"
    _close(_vals(rp["value"]), g["psnr_value"], PSNR_BAR, name + " psnr mean")
    _close(_vals(rp["value_std"]), g["psnr_std"], 2 * PSNR_BAR, name + " psnr std")
    _close(_vals(rs["value"]), g["ssim_value"], SSIM_BAR, name + " ssim mean")
    _close(_vals(rs["value_std"]), g["ssim_std"], 2 * SSIM_BAR, name + " ssim std")


def _vals(d):
    return torch.tensor([d[t] for t in range(len(d))], dtype=torch.float64)


# ---- C3-size batch ------------------------------------------------------------------------------------------------------------

def _c3_pair(B=32, seed=7):
    """[B,3,17,256,256] fp32 pair in [0, 1] (the tokenizer's layout): a and a reconstruction-like b"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    a = torch.rand(B, 3, 17, 256, 256, device="cuda", generator=g)
    b = (a + 0.08 * torch.randn(a.shape, device="cuda", generator=g)).clamp_(0, 1)
    return a, b


def _gauss():
    t = [torch.tensor(-0.5 / (1.5 * 1.5) * (i - 5.0) * (i - 5.0), dtype=torch.float64).exp().item() for i in range(11)]
    s = 1.0 / sum(t)
    return [v * s for v in t]


def oracle(a, b):
    """fp64 torch oracle on [n,3,H,W] fp32 planes: 11 shifted-slice weighted sums per axis over the valid region, no
    convolution library; PSNR from the fp32 squares summed in fp64"""
    g = _gauss()
    x, y = a.double(), b.double()
    H, W = x.shape[-2:]
    vh, vw = H - 10, W - 10

    def filt(m):
        h = sum(g[k] * m[..., :, k:k + vw] for k in range(11))
        return sum(g[k] * h[..., k:k + vh, :] for k in range(11))
    mu1, mu2 = filt(x), filt(y)
    s1, s2, s12 = filt(x * x) - mu1 * mu1, filt(y * y) - mu2 * mu2, filt(x * y) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    smap = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))
    ssim = smap.mean(dim=(-1, -2)).mean(dim=-1)
    d = a - b
    mse = (d * d).double().sum(dim=(-1, -2, -3)) / (3 * H * W)
    psnr = torch.where(mse < 1e-10, torch.full_like(mse, 100.0), 20 * torch.log10(1 / mse.sqrt()))
    return psnr, ssim


@pytest.fixture(scope="module")
def c3():
    a, b = _c3_pair()
    p, s = mt.psnr_ssim(a, b, layout="bcthw")
    torch.cuda.synchronize()
    return a, b, p, s


def test_c3_batch_against_fp64_oracle(c3):
    a, b, p, s = c3
    assert p.shape == (32, 17) and s.shape == (32, 17)
    for c0 in range(0, 32, 4):   # the oracle's fp64 maps in chunks of 4 clips
        fa = a[c0:c0 + 4].permute(0, 2, 1, 3, 4).reshape(-1, 3, 256, 256)
        fb = b[c0:c0 + 4].permute(0, 2, 1, 3, 4).reshape(-1, 3, 256, 256)
        po, so = oracle(fa, fb)
        _close(p[c0:c0 + 4].reshape(-1), po.cpu(), PSNR_BAR, f"clips {c0}.. psnr")
        _close(s[c0:c0 + 4].reshape(-1), so.cpu(), SSIM_BAR, f"clips {c0}.. ssim")


def test_scores_do_not_depend_on_the_batch(c3):
    a, b, p, s = c3
    p3, s3 = mt.psnr_ssim(a[5:8], b[5:8], layout="bcthw")
    assert torch.equal(p3, p[5:8]) and torch.equal(s3, s[5:8])
    for i in range(32):
        p1, s1 = mt.psnr_ssim(a[i:i + 1], b[i:i + 1], layout="bcthw")
        assert torch.equal(p1, p[i:i + 1]) and torch.equal(s1, s[i:i + 1]), f"clip {i}"


def test_layouts_agree_bit_for_bit():
    g = torch.Generator(device="cuda").manual_seed(11)
    u8a = torch.randint(0, 256, (3, 4, 70, 300, 3), dtype=torch.uint8, device="cuda", generator=g)   # two column tiles
    u8b = (u8a.int() + torch.randint(-30, 31, u8a.shape, device="cuda", generator=g)).clamp(0, 255).to(torch.uint8)
    fa, fb = [_unit(u) for u in (u8a, u8b)]                                # [B,F,H,W,3] fp32, u / 255
    ref = mt.psnr_ssim(fa.permute(0, 1, 4, 2, 3).contiguous(), fb.permute(0, 1, 4, 2, 3).contiguous(), layout="btchw")
    bcthw = [x.permute(0, 4, 1, 2, 3) for x in (fa, fb)]                  # non-contiguous views, no copy
    assert not bcthw[0].is_contiguous()
    for got in (mt.psnr_ssim(*bcthw, layout="bcthw"), mt.psnr_ssim(u8a, u8b, layout="bthwc"),
                mt.psnr_ssim(fa, fb, layout="bthwc"), mt.psnr_ssim(u8a, fb, layout="bthwc")):
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    # a w-stride other than 1 / 3 is copied, with the same result
    wide = [torch.zeros(3, 4, 3, 70, 600, device="cuda") for _ in range(2)]
    for w, x in zip(wide, (fa, fb)):
        w[..., ::2] = x.permute(0, 1, 4, 2, 3)
    got = mt.psnr_ssim(wide[0][..., ::2], wide[1][..., ::2])
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])


def test_reconstruction_metrics_on_model_encode_decode():
    from omnitokenizer_amd import OmniTokenizer_VQGAN, make_args, synth
    from omnitokenizer_amd.config import OmniTokConfig
    args = make_args(2, resolution=64)
    model = OmniTokenizer_VQGAN(args)
    model.load_state_dict(synth.synth_state_dict(OmniTokConfig.from_args(args), seed=0), strict=True)
    model = model.cuda().eval()
    x = synth.synth_video(2, 5, 64, seed=1234).cuda()
    ids = model.encode(x, False)
    rec = model.decode(ids, False)
    usage = model.codebook.codebook_usage.clone()
    cnt = model.codebook.call_cnt
    p, s = model.reconstruction_metrics(x, rec, False)
    pe, se = mt.psnr_ssim(x + 0.5, torch.clamp(rec + 0.5, 0, 1), layout="bcthw")
    assert p.shape == (2, x.shape[2]) and torch.equal(p, pe) and torch.equal(s, se)
    assert model.codebook.call_cnt == cnt and torch.equal(model.codebook.codebook_usage, usage)
    pi, si = model.reconstruction_metrics(x[:, :, 0], rec[:, :, 0], True)
    assert pi.shape == (2, 1) and torch.equal(pi[:, 0], p[:, 0]) and torch.equal(si[:, 0], s[:, 0])


def test_fake_implementation_matches_real():
    from torch._subclasses.fake_tensor import FakeTensorMode
    a = torch.rand(2, 3, 3, 24, 40, device="cuda")
    b = torch.rand(2, 3, 3, 24, 40, device="cuda")
    real = torch.ops.omnitok.frame_metrics(a, b, 0.0, False, 0.0, False, 3)
    with FakeTensorMode() as mode:
        fa, fb = mode.from_tensor(a), mode.from_tensor(b)
        fake = torch.ops.omnitok.frame_metrics(fa, fb, 0.0, False, 0.0, False, 3)
    for r, f in zip(real, fake):
        assert f.shape == r.shape and f.dtype == r.dtype == torch.float64 and f.device == r.device
