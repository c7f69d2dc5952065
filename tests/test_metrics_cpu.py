"""CPU: the reconstruction metrics layer (csrc/metrics.hip, omnitokenizer_amd/metrics.py) -- exported symbols, argument
validation of the C ABI (it runs before any launch, so no GPU is needed), the Python layer's layout and dtype checks, and a
fp64 numpy restatement of the reference's PSNR / SSIM against the fixtures of tests/golden/make_golden_metrics.py."""
import ctypes
import glob
import math
import os

import numpy as np
import pytest
import torch

from omnitokenizer_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "metrics_*.npz")))
FAKE = 1 << 20   # a non-null pointer that no check dereferences: every call below fails validation first
B, F, H, W = 2, 5, 64, 96


@pytest.fixture(scope="module")
def lib():
    from omnitokenizer_amd import build
    build.build()
    return _lib.load()


def _op(data=FAKE, dtype=0, clamp=0, shift=0.0, stride=None):
    o = _lib.OmnitokMetricsOperand()
    o.data = data
    for k, s in enumerate(stride or (F * 3 * H * W, 3 * H * W, H * W, W, 1)):
        o.stride[k] = s
    o.dtype, o.clamp, o.shift = dtype, clamp, shift
    return o


def _call(lib, a=None, b=None, sizes=(B, F, H, W), flags=3, psnr=FAKE, ssim=FAKE, work=FAKE, work_bytes=None):
    a = _op() if a is None else a
    b = _op() if b is None else b
    if work_bytes is None:
        work_bytes = lib.omnitok_frame_metrics_workspace(*sizes) if min(sizes[1:]) > 0 else 0
    rc = lib.omnitok_frame_metrics(None if a == "null" else ctypes.byref(a), None if b == "null" else ctypes.byref(b),
                                   *sizes, flags, psnr, ssim, work, max(work_bytes, 0), None)
    return rc, lib.omnitok_last_error().decode()


def test_metrics_symbols_exported(lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("omnitok_frame_metrics", "omnitok_frame_metrics_workspace"):
        assert hasattr(raw, name) and name in _lib.EXPORTED_SYMBOLS
    import omnitokenizer_amd
    from omnitokenizer_amd import OmniTokenizer_VQGAN, metrics
    for name in ("psnr_ssim", "calculate_psnr", "calculate_ssim"):
        assert name in omnitokenizer_amd.__all__
        assert getattr(omnitokenizer_amd, name) is getattr(metrics, name)
    assert callable(OmniTokenizer_VQGAN.reconstruction_metrics)
    assert hasattr(torch.ops.omnitok, "frame_metrics")


def test_workspace_size(lib):
    # fixed partition: strips of 32 SSIM rows, tiles of 246 SSIM columns; 2 doubles per (clip, frame, channel, part)
    assert lib.omnitok_frame_metrics_workspace(32, 17, 256, 256) == 32 * 17 * 3 * 8 * 1 * 16
    assert lib.omnitok_frame_metrics_workspace(1, 1, 1000, 600) == 3 * 31 * 3 * 16
    assert lib.omnitok_frame_metrics_workspace(2, 2, 10, 12) == 2 * 2 * 3 * 1 * 1 * 16
    assert lib.omnitok_frame_metrics_workspace(0, 1, 8, 8) == 0
    assert lib.omnitok_frame_metrics_workspace(1, 0, 8, 8) == -1
    assert lib.omnitok_frame_metrics_workspace(1, 1, 0, 8) == -1


@pytest.mark.parametrize("case,kw,needle", [
    ("null operand a", dict(a="null"), "null pointer"),
    ("null operand b", dict(b="null"), "null pointer"),
    ("null data", dict(b=_op(data=None)), "null pointer (data)"),
    ("null psnr output", dict(psnr=None), "null pointer (psnr"),
    ("null ssim output", dict(ssim=None), "null pointer (ssim"),
    ("null work", dict(work=None), "null pointer (work"),
    ("bad element type", dict(a=_op(dtype=2)), "element type 2"),
    ("short workspace", dict(work_bytes=B * F * 3 * 2 * 16 - 8), "workspace of"),
    ("inner stride 2", dict(a=_op(stride=(1, 1, 1, 1, 2))), "w stride 2"),
    ("inner stride 0", dict(b=_op(stride=(1, 1, 1, 1, 0))), "w stride 0"),
    ("negative stride", dict(a=_op(stride=(1, -1, 1, 1, 1))), "negative stride"),
    ("uint8 with shift", dict(a=_op(dtype=1, shift=0.5)), "no shift or clamp"),
    ("uint8 with clamp", dict(b=_op(dtype=1, clamp=1)), "no shift or clamp"),
    ("bad clamp", dict(a=_op(clamp=2)), "clamp 2"),
    ("non-finite shift", dict(a=_op(shift=float("nan"))), "not finite"),
    ("no output", dict(flags=0), "flags"),
    ("unknown flag", dict(flags=4), "flags"),
    ("bad sizes", dict(sizes=(B, F, 0, W)), "bad sizes"),
    ("too many frames", dict(sizes=(B, 30000, H, W)), "bad sizes"),
])
def test_frame_metrics_validation(lib, case, kw, needle):
    rc, msg = _call(lib, **kw)
    assert rc == -1, case
    assert needle in msg, (case, msg)


def test_only_requested_outputs_need_pointers(lib):
    # PSNR alone with a null SSIM pointer gets past validation up to the operands; an empty batch is a no-op
    rc, msg = _call(lib, flags=1, ssim=None, a=_op(dtype=7))
    assert rc == -1 and "element type 7" in msg
    rc, _ = _call(lib, sizes=(0, F, H, W), a="null", b="null", psnr=None, ssim=None, work=None)
    assert rc == 0


def test_python_layer_checks():
    from omnitokenizer_amd import metrics
    x = torch.zeros(2, 5, 3, 16, 16)
    with pytest.raises(ValueError, match="layout"):
        metrics.psnr_ssim(x, x, layout="bhwc")
    with pytest.raises(TypeError, match="dtype"):
        metrics.psnr_ssim(x.double(), x)
    with pytest.raises(TypeError, match="dtype"):
        metrics.psnr_ssim(x, x.half())
    with pytest.raises(TypeError, match="tensor"):
        metrics.psnr_ssim(x.numpy(), x)
    with pytest.raises(ValueError, match="differ in shape"):
        metrics.psnr_ssim(x, x[:, :4])
    with pytest.raises(ValueError, match="channels"):
        metrics.psnr_ssim(x, x, layout="bcthw")                       # [B,3,F,H,W] expected: dim 1 is 5 here
    with pytest.raises(ValueError, match="channels"):
        metrics.psnr_ssim(torch.zeros(2, 5, 16, 16, 4, dtype=torch.uint8), torch.zeros(2, 5, 16, 16, 4, dtype=torch.uint8),
                          layout="bthwc")
    with pytest.raises(ValueError, match="5-D video or a 4-D image"):
        metrics.psnr_ssim(x[0, 0], x[0, 0])
    with pytest.raises(RuntimeError, match="GPU"):
        metrics.psnr_ssim(x, x)
    with pytest.raises(RuntimeError, match="GPU"):
        metrics.psnr_ssim(torch.zeros(2, 16, 16, 3, dtype=torch.uint8), torch.zeros(2, 16, 16, 3, dtype=torch.uint8),
                          layout="bthwc")
    with pytest.raises(TypeError, match="float32"):
        metrics.calculate_psnr(x.to(torch.uint8), x.to(torch.uint8))
    with pytest.raises(ValueError, match="batch"):
        metrics.calculate_ssim(x[:0], x[:0])
    with pytest.raises(ValueError, match="differ in shape"):
        metrics.calculate_ssim(x, x[:1])
    with pytest.raises(ValueError, match="is_image"):
        metrics.reconstruction_psnr_ssim(torch.zeros(2, 3, 5, 16, 16), torch.zeros(2, 3, 5, 16, 16), True)
    with pytest.raises(TypeError, match="float32"):
        metrics.reconstruction_psnr_ssim(torch.zeros(2, 3, 16, 16, dtype=torch.uint8), torch.zeros(2, 3, 16, 16), True)


def test_model_method_refuses_cpu():
    from omnitokenizer_amd import OmniTokenizer_VQGAN, make_args
    m = OmniTokenizer_VQGAN(make_args(2, resolution=64))
    x = torch.zeros(1, 3, 5, 64, 64)
    with pytest.raises(RuntimeError, match="GPU"):
        m.reconstruction_metrics(x, x, False)


# ---- fp64 numpy restatement of calculate_psnr.py / calculate_ssim.py -----------------------------------------------------------

def _window():
    # cv2.getGaussianKernel(11, 1.5): exp((-0.5 / sigma^2) x x) normalised by 1 / sum, outer product as in ssim()
    t = [math.exp(-0.5 / (1.5 * 1.5) * (i - 5.0) * (i - 5.0)) for i in range(11)]
    s = 1.0 / sum(t)
    g = np.array([v * s for v in t])
    return np.outer(g, g)


def np_ssim_plane(p1, p2):
    """ssim() of one [H, W] plane in fp64: the 2-D window over the valid region only (no convolution library)"""
    a, b = p1.astype(np.float64), p2.astype(np.float64)
    H, W = a.shape
    vh, vw = H - 10, W - 10
    if vh <= 0 or vw <= 0:
        return float("nan")
    win = _window()

    def filt(x):
        acc = np.zeros((vh, vw))
        for i in range(11):
            for j in range(11):
                acc += win[i, j] * x[i:i + vh, j:j + vw]
        return acc
    mu1, mu2 = filt(a), filt(b)
    s1, s2, s12 = filt(a * a) - mu1 ** 2, filt(b * b) - mu2 ** 2, filt(a * b) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    return float((((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 ** 2 + mu2 ** 2 + C1) * (s1 + s2 + C2))).mean())


def np_psnr_frame(f1, f2):
    mse = np.mean((f1 - f2) ** 2)   # float32, as img_psnr
    return 100.0 if mse < 1e-10 else 20 * math.log10(1 / math.sqrt(mse))


def fixture_videos(g):
    """the reference's [B,T,3,H,W] fp32 videos of a fixture (make_golden_metrics.videos_of, in numpy)"""
    if "u8a" in g:
        return [np.ascontiguousarray(g[k].transpose(0, 1, 4, 2, 3)).astype(np.float32) / np.float32(255) for k in ("u8a", "u8b")]
    real = g["xa"] + np.float32(0.5)
    fake = np.clip(g["xb"] + np.float32(0.5), np.float32(0), np.float32(1))
    return [np.ascontiguousarray(v.transpose(0, 2, 1, 3, 4)) for v in (real, fake)]


def test_fixture_set_is_complete():
    assert set(FIXTURES) == {"metrics_video", "metrics_odd", "metrics_11x11", "metrics_10x12", "metrics_image",
                             "metrics_identical", "metrics_offset", "metrics_noise", "metrics_float"}
    assert sum(os.path.getsize(os.path.join(GOLDEN, n + ".npz")) for n in FIXTURES) <= 1.5e6


@pytest.mark.parametrize("name", FIXTURES)
def test_numpy_restatement_reproduces_fixture(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    v1, v2 = fixture_videos(g)
    Bn, T = v1.shape[:2]
    psnr = np.array([[np_psnr_frame(v1[b, t], v2[b, t]) for t in range(T)] for b in range(Bn)])
    ssim = np.array([[(np_ssim_plane(v1[b, t, 0], v2[b, t, 0]) + np_ssim_plane(v1[b, t, 1], v2[b, t, 1]) +
                       np_ssim_plane(v1[b, t, 2], v2[b, t, 2])) / 3 for t in range(T)] for b in range(Bn)])
    assert psnr.shape == g["psnr"].shape and ssim.shape == g["ssim"].shape
    # PSNR: both are float32 np.mean, but over different memory orders (the fixture's frames are strided views), hence the
    # float32 summation bar of tests/test_gpu_metrics.py (PSNR_BAR) rather than equality
    np.testing.assert_allclose(psnr, g["psnr"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(ssim, g["ssim"], rtol=0, atol=1e-12, equal_nan=True)
    np.testing.assert_allclose(psnr.mean(0), g["psnr_value"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(psnr.std(0), g["psnr_std"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(ssim.mean(0), g["ssim_value"], rtol=0, atol=1e-12, equal_nan=True)
    np.testing.assert_allclose(ssim.std(0), g["ssim_std"], rtol=0, atol=1e-12, equal_nan=True)
    if name == "metrics_identical":
        assert (g["psnr"] == 100).all() and (g["ssim"] == 1.0).all()
    if name == "metrics_10x12":
        assert np.isnan(g["ssim"]).all() and np.isfinite(g["psnr"]).all()
    if name == "metrics_float":
        fake = fixture_videos(g)[1]
        assert (fake == 0).any() and (fake == 1).any()
