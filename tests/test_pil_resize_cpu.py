"""CPU: the Pillow-exact resize (csrc/resize_pil.hip, omnitokenizer_amd.frames.resize_frames / images_to_pixels /
center_crop_arr) -- exported symbols, the host run of the coefficient text the device runs against the numpy restatement
(tests/pil_resize_oracle.py; the guard against FMA contraction on the host), the C ABI's argument validation (it runs before
any launch, so no GPU is needed), the Python layer's input checks, and the fixtures written by
tests/golden/make_golden_pil_resize.py against the oracle and, where Pillow is installed, against Pillow itself."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

from omnitokenizer_amd import _lib
from tests import pil_resize_oracle as oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FAKE = ctypes.c_void_p(1 << 20)   # a non-null, 16-byte aligned pointer that no check dereferences
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "pilresize_*.npz")))
# every (in, out) axis pair of the fixture shapes (rows, then columns; center_crop_arr's box halvings and bicubic steps
# included), plus the ImageNet-sized ones
AXIS_PAIRS = [(37, 16), (53, 16), (16, 24), (7, 16), (5, 16), (64, 64), (48, 32), (33, 33), (33, 20), (1, 4), (9, 4),
              (1000, 8), (31, 8), (129, 96), (257, 96), (48, 24), (50, 25), (40, 32), (72, 32), (70, 96), (90, 96),
              (150, 75), (97, 48), (75, 50), (48, 32), (64, 32), (500, 256), (375, 256), (1, 4)]


@pytest.fixture(scope="module")
def lib():
    from omnitokenizer_amd import build
    build.build()
    return _lib.load()


def test_fixture_list_is_complete():   # ... and every fixture is within the size of the largest frames fixture
    assert len(FIXTURES) == 30, FIXTURES
    limit = os.path.getsize(os.path.join(GOLDEN, "frames_pre_odd.npz"))
    for name in FIXTURES:
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) <= limit, name


def test_symbols_exported(lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("omnitok_frames_resize_pil_workspace", "omnitok_frames_resize_pil", "omnitok_pil_resize_coeffs"):
        assert hasattr(raw, name) and name in _lib.EXPORTED_SYMBOLS


def _coeffs(lib, n_in, n_out, f):
    ks = ctypes.c_int(-1)
    assert lib.omnitok_pil_resize_coeffs(n_in, n_out, f, ctypes.byref(ks), None, None) == 0
    k = np.full((n_out, ks.value), 12345, np.int32)
    b = np.full((n_out, 2), 12345, np.int32)
    assert lib.omnitok_pil_resize_coeffs(n_in, n_out, f, ctypes.byref(ks), k.ctypes.data_as(ctypes.c_void_p),
                                         b.ctypes.data_as(ctypes.c_void_p)) == 0
    return ks.value, k, b


@pytest.mark.parametrize("f", [0, 1, 2], ids=["bicubic", "bilinear", "box"])
def test_host_coefficients_equal_the_oracle(lib, f):
    for n_in, n_out in sorted(set(AXIS_PAIRS)):
        ks, k, b = _coeffs(lib, n_in, n_out, f)
        want_ks, want_k, want_b = oracle.coeffs(n_in, n_out, f)
        assert ks == want_ks, (n_in, n_out)
        assert np.array_equal(b, want_b), (n_in, n_out)
        assert np.array_equal(k, want_k), (n_in, n_out, int(np.abs(k - want_k).max()))


def test_coefficients_validation(lib):
    ks = ctypes.c_int(0)
    for args, needle in [((0, 4, 0, ctypes.byref(ks), None, None), "bad sizes"), ((4, 0, 0, ctypes.byref(ks), None, None), "bad sizes"),
                         ((4, 4, 3, ctypes.byref(ks), None, None), "filter"), ((4, 4, 0, None, None, None), "null ksize"),
                         ((4, 8, 0, ctypes.byref(ks), FAKE, None), "null bounds")]:
        assert lib.omnitok_pil_resize_coeffs(*args) == -1
        assert needle in lib.omnitok_last_error().decode()


def _desc(F=1, H=72, W=128, start=0, step=1, top=0, left=0, rh=64, rw=64, frames=FAKE):
    d = _lib.OmnitokFramesDesc()
    d.frames = frames.value if frames is not None else None
    d.F, d.H, d.W = F, H, W
    d.row_stride, d.frame_stride = 3 * W, 3 * W * H
    d.frame_start, d.frame_step, d.crop_top, d.crop_left, d.resize_h, d.resize_w = start, step, top, left, rh, rw
    return d


def _arr(descs):
    return (_lib.OmnitokFramesDesc * max(len(descs), 1))(*descs)


def _resize(lib, descs, F_out=1, R_h=64, R_w=64, filt=0, kind=0, work=FAKE, work_bytes=1 << 40, out=FAKE):
    rc = lib.omnitok_frames_resize_pil(_arr(descs), len(descs), F_out, R_h, R_w, filt, kind, work, work_bytes, out, None)
    return rc, lib.omnitok_last_error().decode()


def _small_stride(d):
    d.row_stride = 100
    return d


def _small_frame_stride(d):
    d.frame_stride = d.row_stride * (d.H - 1) + 3 * d.W - 1   # one byte short of a frame
    return d


@pytest.mark.parametrize("case,kw,needle", [
    ("null output", dict(out=None), "null pointer"),
    ("null work", dict(work=None), "null pointer"),
    ("null frames", dict(descs=[_desc(frames=None)]), "clip 0: null frames"),
    ("bad filter", dict(filt=3), "filter 3"),
    ("negative filter", dict(filt=-1), "filter -1"),
    ("bad out kind", dict(kind=2), "out kind 2"),
    ("bad sizes", dict(R_h=0), "bad sizes"),
    ("frames past F", dict(descs=[_desc(start=1)]), "run past F"),
    ("frame step past F", dict(descs=[_desc(F=8, step=2)], F_out=5), "run past F"),
    ("resize_h < 1", dict(descs=[_desc(rh=0)]), "sizes must be >= 1"),
    ("resize_w < 1", dict(descs=[_desc(rw=-3)]), "sizes must be >= 1"),
    ("crop right of resized", dict(descs=[_desc(rw=100, left=40)]), "outside the 64x100 resized"),
    ("crop below resized", dict(descs=[_desc(rh=70, top=7)]), "outside the 70x64 resized"),
    ("negative crop", dict(descs=[_desc(top=-1)]), "outside"),
    ("window larger than resized", dict(R_h=65), "outside the 64x64 resized"),
    ("row stride too small", dict(descs=[_small_stride(_desc())]), "strides"),
    ("frame stride too small", dict(descs=[_small_frame_stride(_desc(F=2))]), "strides"),
    ("workspace too small", dict(work_bytes=1000), "too small"),
    ("unaligned workspace", dict(work=ctypes.c_void_p((1 << 20) + 4)), "16-byte aligned"),
    ("too many taps", dict(descs=[_desc(H=64, W=8000, rh=64, rw=8)], R_h=8, R_w=8), "more than the cap of 2048"),
])
def test_frames_resize_pil_validation(lib, case, kw, needle):
    descs = kw.pop("descs", [_desc()])
    rc, msg = _resize(lib, descs, **kw)
    assert rc == -1, case
    assert needle in msg, (case, msg)


def test_null_desc_and_empty_batch(lib):
    assert lib.omnitok_frames_resize_pil(None, 1, 1, 64, 64, 0, 0, FAKE, 1 << 30, FAKE, None) == -1
    assert "null pointer" in lib.omnitok_last_error().decode()
    assert lib.omnitok_frames_resize_pil(None, 0, 1, 64, 64, 0, 0, None, 0, None, None) == 0


def test_validation_names_the_clip(lib):
    rc, msg = _resize(lib, [_desc(), _desc(H=40, W=48, rh=32, rw=32)])
    assert rc == -1 and "clip 1" in msg and "32x32 resized" in msg


def test_the_tap_cap_admits_a_125_fold_bicubic_downscale(lib):
    ws = lib.omnitok_frames_resize_pil_workspace(_arr([_desc(H=1000, W=1000, rh=8, rw=8)]), 1, 1, 0)
    assert ws > 0
    ks, _, _ = _coeffs(lib, 1000, 8, 0)
    assert ks == 501


def test_workspace_grows_with_the_batch_and_rejects_bad_input(lib):
    ws = lib.omnitok_frames_resize_pil_workspace
    one = ws(_arr([_desc()]), 1, 1, 0)
    two = ws(_arr([_desc(), _desc()]), 2, 1, 0)
    ragged = ws(_arr([_desc(), _desc(H=300, W=301, rh=128, rw=128)]), 2, 1, 0)
    assert 0 < one and two == 2 * one and ragged > two
    # the tables of both axes and an intermediate of H rows of the resized width
    ksw, ksh = oracle.coeffs(128, 64, 0)[0], oracle.coeffs(72, 64, 0)[0]
    assert one >= 4 * 64 * (ksw + 2) + 4 * 64 * (ksh + 2) + 72 * 64 * 3
    assert ws(_arr([_desc(F=3)]), 1, 3, 0) > one
    assert ws(None, 0, 1, 0) == 0
    # the size it reports is accepted, one byte less is not
    assert _resize(lib, [_desc()], work_bytes=one - 1)[0] == -1
    for args, needle in [((None, 1, 1, 0), "null pointer"), ((_arr([_desc()]), 1, 1, 5), "filter 5"),
                         ((_arr([_desc()]), 1, 0, 0), "bad sizes"), ((_arr([_desc(rh=0)]), 1, 1, 0), "sizes must be >= 1"),
                         ((_arr([_desc(frames=None)]), 1, 1, 0), "null frames"),
                         ((_arr([_desc(), _desc(W=9000, rw=8)]), 2, 1, 0), "clip 1")]:
        assert ws(*args) == -1
        assert needle in lib.omnitok_last_error().decode(), needle


def test_python_api_rejects_bad_inputs():
    from omnitokenizer_amd import frames
    import omnitokenizer_amd
    assert omnitokenizer_amd.resize_frames is frames.resize_frames
    assert omnitokenizer_amd.images_to_pixels is frames.images_to_pixels
    assert omnitokenizer_amd.center_crop_arr is frames.center_crop_arr
    u8 = torch.zeros(2, 16, 20, 3, dtype=torch.uint8)
    for fn in (lambda x: frames.resize_frames(x, (8, 8), True), lambda x: frames.images_to_pixels(x, 8),
               lambda x: frames.center_crop_arr(x, 8)):
        with pytest.raises(RuntimeError, match="GPU"):
            fn(u8)
        with pytest.raises(RuntimeError, match="GPU"):
            fn([u8[0], u8[1, :8]])
        with pytest.raises(TypeError, match="uint8"):
            fn(u8.float())
        with pytest.raises(ValueError, match="shape"):
            fn(u8[..., :2])
        with pytest.raises(TypeError):
            fn(u8.numpy())
    with pytest.raises(ValueError):
        frames.resize_frames(u8, (8, 8))                    # [B,H,W,3] is not a batch of clips
    with pytest.raises(ValueError, match="interpolation"):
        frames.resize_frames(u8, (8, 8), True, interpolation="lanczos")
    with pytest.raises(ValueError, match="interpolation"):
        frames.images_to_pixels(u8, 8, interpolation="nearest")
    with pytest.raises(ValueError, match="out"):
        frames.resize_frames(u8, (8, 8), True, out="float")
    with pytest.raises(ValueError, match="resolution"):
        frames.images_to_pixels(u8, 0)
    with pytest.raises(ValueError, match="crop"):
        frames.images_to_pixels(u8, 8, resize_to=12)
    with pytest.raises(ValueError, match="resize_to"):
        frames.images_to_pixels(u8, 8, crop=[(0, 0), (0, 0)])
    with pytest.raises(ValueError, match="image_size"):
        frames.center_crop_arr(u8, 0)


def test_encode_images_exists_and_refuses_cpu():
    from omnitokenizer_amd import OmniTokenizer_VQGAN, make_args
    m = OmniTokenizer_VQGAN(make_args(2, resolution=64))
    with pytest.raises(RuntimeError, match="GPU"):
        m.encode_images(torch.zeros(1, 80, 90, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="GPU"):
        m.encode_images([torch.zeros(80, 90, 3, dtype=torch.uint8)])


def expected_from(g, resize, cca):
    """what a fixture's `out` must equal, from `resize(u8, (h, w), interpolation)` / `cca(u8, image_size)`"""
    kind = str(g["kind"])
    if kind == "center_crop_arr":
        return cca(g["u8"], int(g["image_size"]))
    size, interp = tuple(int(v) for v in g["size"]), str(g["interpolation"])
    if kind == "video":
        c0, w = int(g["col0"]), int(g["width"])
        sel = g["u8"][int(g["frame_start"])::int(g["sample_every_n_frames"]), :, c0:c0 + w]
        return np.stack([resize(np.ascontiguousarray(f), size, interp) for f in sel])
    out = resize(g["u8"], size, interp)
    if "crop" in g:
        (top, left), s = g["crop"], int(g["crop_size"])
        out = np.ascontiguousarray(out[top:top + s, left:left + s])
    return out


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_equals_the_fixture(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    assert g["u8"].dtype == np.uint8 and g["out"].dtype == np.uint8 and str(g["pil_version"])
    assert np.array_equal(expected_from(g, oracle.resize, oracle.center_crop_arr), g["out"])
    if str(g["kind"]) == "imagedataset":
        want = (g["out"].astype(np.float32) / np.float32(255) - np.float32(0.5)).transpose(2, 0, 1)
        assert g["pixels"].dtype == np.float32 and np.array_equal(g["pixels"], want)
        # ... which is torch's ToTensor + Normalize(0.5, 1.0) arithmetic
        t = torch.from_numpy(g["out"]).permute(2, 0, 1).float().div(255).sub(0.5)
        assert torch.equal(t, torch.from_numpy(g["pixels"]))


@pytest.mark.parametrize("name", FIXTURES)
def test_pillow_now_equals_the_fixture(name):
    pytest.importorskip("PIL")
    from tests.golden import make_golden_pil_resize as mk
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    got = expected_from(g, mk.pil_resize, mk.center_crop_arr)
    assert np.array_equal(got, g["out"]), "Pillow's resampler changed: the fixtures (and the kernels) describe " + \
        str(g["pil_version"])
