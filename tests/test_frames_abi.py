"""CPU: the frames in / frames out layer (csrc/frames.hip, omnitokenizer_amd/frames.py) -- exported symbols, argument
validation of the C ABI (it runs before any launch, so no GPU is needed), the Python layer's input checks, and the
reference fixtures written by tests/golden/make_golden_frames.py."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from omnitokenizer_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FAKE = ctypes.c_void_p(1 << 20)   # a non-null pointer that no check dereferences: every call below fails validation first


@pytest.fixture(scope="module")
def lib():
    from omnitokenizer_amd import build
    build.build()
    return _lib.load()


def _desc(F=5, H=72, W=128, start=0, step=1, top=0, left=0, rh=0, rw=0, frames=FAKE):
    d = _lib.OmnitokFramesDesc()
    d.frames = frames.value if frames is not None else None
    d.F, d.H, d.W = F, H, W
    d.row_stride, d.frame_stride = 3 * W, 3 * W * H
    d.frame_start, d.frame_step, d.crop_top, d.crop_left, d.resize_h, d.resize_w = start, step, top, left, rh, rw
    return d


def _f2p(lib, descs, F_out=5, R_h=64, R_w=64, mode=0, flags=0, work=FAKE, out=FAKE):
    arr = (_lib.OmnitokFramesDesc * max(len(descs), 1))(*descs)
    rc = lib.omnitok_frames_to_pixels(arr if descs else None, len(descs), F_out, R_h, R_w, mode, flags, work, out, None)
    return rc, lib.omnitok_last_error().decode()


def test_frames_symbols_exported(lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("omnitok_frames_to_pixels", "omnitok_pixels_to_frames"):
        assert hasattr(raw, name) and name in _lib.EXPORTED_SYMBOLS


@pytest.mark.parametrize("case,kw,needle", [
    ("null desc", dict(descs=None), "null pointer"),
    ("null output", dict(out=None), "null pointer"),
    ("null frames", dict(descs=[_desc(frames=None)]), "null frames"),
    ("null work with videonorm", dict(flags=1, work=None), "null work"),
    ("crop right of source", dict(descs=[_desc(left=65)]), "outside the 72x128 source"),
    ("crop below source", dict(descs=[_desc(top=9)]), "outside the 72x128 source"),
    ("negative crop", dict(descs=[_desc(top=-1)]), "outside"),
    ("frames past F", dict(descs=[_desc(start=1)]), "run past F"),
    ("frame step past F", dict(descs=[_desc(F=8, step=2)], F_out=5), "run past F"),
    ("bilinear crop outside resized", dict(mode=1, descs=[_desc(rh=64, rw=100, left=40)]), "outside the 64x100 resized"),
    ("bilinear without size", dict(mode=1, descs=[_desc()]), "resized"),
    ("bad mode", dict(mode=2), "mode"),
    ("unknown flag", dict(flags=2), "flags"),
    ("videonorm with bilinear", dict(mode=1, flags=1, descs=[_desc(rh=64, rw=113)]), "mode NONE only"),
    ("bad sizes", dict(R_h=0), "bad sizes"),
    ("row stride too small", dict(descs=[(lambda d: (setattr(d, "row_stride", 100), d)[1])(_desc())]), "strides"),
])
def test_frames_to_pixels_validation(lib, case, kw, needle):
    descs = kw.pop("descs", [_desc()])
    if descs is None:
        rc = lib.omnitok_frames_to_pixels(None, 1, 5, 64, 64, 0, 0, FAKE, FAKE, None)
        msg = lib.omnitok_last_error().decode()
    else:
        rc, msg = _f2p(lib, descs, **kw)
    assert rc == -1, case
    assert needle in msg, (case, msg)


def test_ragged_validation_names_the_clip(lib):
    rc, msg = _f2p(lib, [_desc(), _desc(H=40, W=48)], R_h=64, R_w=64)
    assert rc == -1 and "clip 1" in msg and "40x48" in msg


@pytest.mark.parametrize("args,needle", [
    ((FAKE, 2, 4, 5, 8, 8, 0, FAKE), "expected 3 channels"),
    ((FAKE, 2, 1, 5, 8, 8, 1, FAKE), "expected 3 channels"),
    ((None, 2, 3, 5, 8, 8, 0, FAKE), "null pointer"),
    ((FAKE, 2, 3, 5, 8, 8, 0, None), "null pointer"),
    ((FAKE, 2, 3, 5, 8, 8, 2, FAKE), "layout"),
    ((FAKE, 2, 3, 0, 8, 8, 0, FAKE), "bad sizes"),
])
def test_pixels_to_frames_validation(lib, args, needle):
    rc = lib.omnitok_pixels_to_frames(*args, None)
    assert rc == -1 and needle in lib.omnitok_last_error().decode()


def test_python_api_rejects_bad_inputs():
    from omnitokenizer_amd import frames
    u8 = torch.zeros(2, 5, 16, 16, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU"):
        frames.frames_to_pixels(u8)
    with pytest.raises(RuntimeError, match="GPU"):
        frames.frames_to_pixels([u8[0], u8[1, :, :8]], resolution=8)
    with pytest.raises(TypeError, match="uint8"):
        frames.frames_to_pixels(u8.float())
    with pytest.raises(ValueError, match="shape"):
        frames.frames_to_pixels(u8[..., :2])
    with pytest.raises(ValueError):
        frames.frames_to_pixels(u8, is_image=True)          # [B,F,H,W,3] is not an image batch
    with pytest.raises(ValueError, match="resize"):
        frames.frames_to_pixels(u8, resize="bicubic")
    with pytest.raises(ValueError, match="videonorm"):
        frames.frames_to_pixels(u8, resize="bilinear", norm="videonorm", resolution=8)
    with pytest.raises(TypeError):
        frames.frames_to_pixels(u8.numpy())
    x = torch.zeros(2, 3, 5, 8, 8)
    with pytest.raises(RuntimeError, match="GPU"):
        frames.pixels_to_frames(x)
    with pytest.raises(TypeError, match="float32"):
        frames.pixels_to_frames(x.double())
    with pytest.raises(ValueError, match="shape"):
        frames.pixels_to_frames(torch.zeros(2, 4, 5, 8, 8))
    with pytest.raises(ValueError, match="layout"):
        frames.pixels_to_frames(x, layout="hwc")


def test_model_methods_exist_and_refuse_cpu():
    from omnitokenizer_amd import OmniTokenizer_VQGAN, make_args
    m = OmniTokenizer_VQGAN(make_args(2, resolution=64))
    with pytest.raises(RuntimeError, match="GPU"):
        m.encode_frames(torch.zeros(1, 5, 64, 64, 3, dtype=torch.uint8), False)
    with pytest.raises(RuntimeError, match="GPU"):
        m.decode_frames(torch.zeros(1, 2, 8, 8, dtype=torch.int64), False)


def test_preprocess_size_is_the_reference_rule():
    from omnitokenizer_amd.frames import preprocess_size
    for h, w, r in [(72, 128, 64), (96, 80, 128), (300, 301, 128), (360, 640, 256), (48, 48, 64), (301, 300, 128)]:
        scale = r / min(h, w)   # data.py:320-326
        want = (r, math.ceil(w * scale)) if h < w else (math.ceil(h * scale), r)
        assert preprocess_size(h, w, r) == want
    assert preprocess_size(360, 640, 256) == (256, 456)


FIXTURES = {  # name: (u8 [F,H,W,3], ref [3,F_out,R,R])
    "frames_pre_wide_down": ((5, 72, 128), (5, 64)), "frames_pre_tall_up": ((2, 96, 80), (2, 128)),
    "frames_pre_square_up": ((2, 48, 48), (2, 64)), "frames_pre_same": ((2, 64, 128), (2, 64)),
    "frames_pre_odd": ((1, 300, 301), (1, 128)), "frames_pre_seq": ((9, 40, 72), (4, 32)),
    "frames_pre_image": ((1, 72, 128), (1, 64)), "frames_vn_video": ((5, 72, 128), (5, 64)),
    "frames_vn_binary": ((5, 40, 48), (5, 32)), "frames_vn_image": ((1, 64, 96), (1, 64)),
}


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_frames_fixtures_load(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    (fhw, (f_out, r)) = FIXTURES[name]
    assert g["u8"].dtype == np.uint8 and g["u8"].shape == fhw + (3,)
    assert g["ref"].dtype == np.float32 and g["ref"].shape == (3, f_out, r, r)
    assert int(g["resolution"]) == r
    ref = g["ref"]
    if name == "frames_vn_binary":    # VideoNorm's rule: bytes 0 / 1 are not divided by 255
        assert set(np.unique(ref).tolist()) <= {-0.5, 0.5}
    else:
        assert ref.min() >= -0.5 and ref.max() <= 0.5
    if name.startswith("frames_vn_"):
        top, left = int(g["crop_top"]), int(g["crop_left"])
        assert 0 <= top <= fhw[1] - r and 0 <= left <= fhw[2] - r


def test_frames_fixtures_stay_small():
    total = sum(os.path.getsize(os.path.join(GOLDEN, n + ".npz")) for n in FIXTURES)
    assert total < 2_000_000
