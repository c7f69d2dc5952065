"""CPU: the I3D / FVD layer (csrc/i3d.hip, omnitokenizer_amd/i3d.py, omnitokenizer_amd/fvd.py) -- exported symbols, argument
validation of the C ABI (it runs before any launch, so no GPU is needed), the synthetic weights against the reference's
state_dict, the soundness of the logits bar of tests/test_gpu_fvd.py, frechet_distance against the reference's values, and
the Python layer's input checks.

Bars: frechet_distance on the fixture's fp64 logits is the reference's fp64 computation in the same operation order:
1e-9 relative (svd and matmul blocking may differ between builds).  Against the reference's fp32 value: the fp32 run takes the
square root of the D - n + 1 = 393 covariance eigenvalues that are rounding noise, each at most D u max(tr S1, tr S2) in
size, so it is off by at most 2 (D - n + 1) sqrt(D u max tr) plus its own rounding: FVD32_BAR below.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from omnitokenizer_amd import _lib, fvd, i3d, synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FAKE = ctypes.c_void_p(1 << 20)   # a non-null, aligned pointer that no check dereferences
CASES = ["fvd_t17_40x52", "fvd_t16_64x64"]
U = 2.0 ** -24


@pytest.fixture(scope="module")
def lib():
    from omnitokenizer_amd import build
    build.build()
    return _lib.load()


def _fix(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def test_symbols_exported(lib):
    for name in ("omnitok_same_pad", "omnitok_i3d_preprocess", "omnitok_conv3d_packed_ldw", "omnitok_conv3d_same",
                 "omnitok_maxpool3d_same", "omnitok_i3d_head"):
        assert name in _lib.EXPORTED_SYMBOLS and getattr(lib, name)
    import omnitokenizer_amd as pkg
    for name in ("InceptionI3d", "load_fvd_model", "get_fvd_logits", "frechet_distance", "compute_fvd"):
        assert name in pkg.__all__ and getattr(pkg, name)


@pytest.mark.parametrize("s,k,stride,front,out", [(224, 7, 2, 2, 112), (17, 7, 2, 3, 9), (16, 7, 2, 2, 8),
                                                 (112, 3, 2, 0, 56), (113, 3, 2, 1, 57), (9, 3, 2, 1, 5),
                                                 (5, 2, 2, 0, 3), (4, 2, 2, 0, 2), (28, 3, 1, 1, 28), (7, 1, 1, 0, 7)])
def test_same_pad(lib, s, k, stride, front, out):
    """Unit3D.compute_pad: Conv3d_1a on 224 pads 2 / 3 (its padding=(3,3,3) argument is ignored), on 17 pads 3 / 3"""
    f, o = ctypes.c_int(), ctypes.c_int()
    lib.omnitok_same_pad(s, k, stride, ctypes.byref(f), ctypes.byref(o))
    assert (f.value, o.value) == (front, out) == i3d.same_pad(s, k, stride)


def _conv(**kw):
    d = _lib.OmnitokConv3d()
    base = dict(x=FAKE.value, x_cs=64, x_off=0, B=1, T=9, H=28, W=28, Cin=64, w=FAKE.value, bias=FAKE.value, Cout=32,
                kt=3, kh=3, kw=3, st=1, sh=1, sw=1, relu=1, y=FAKE.value, y_cs=32, y_off=0, y2=None, y2_cs=0, y2_off=0,
                split=32)
    base.update(kw)
    for k, v in base.items():
        setattr(d, k, v)
    return d


# every bad descriptor with the full omnitok_last_error() text of the commit before the shared host side
# (conv_args in csrc/convnet_common.h)
CONV_REJECTS = [
    (dict(Cin=3, x_cs=4), "conv3d_same: Cin 3 must be a positive multiple of 4 and the kernel 3 x 3 x 3 within 1..7"),
    (dict(Cin=0), "conv3d_same: Cin 0 must be a positive multiple of 4 and the kernel 3 x 3 x 3 within 1..7"),
    (dict(kt=8), "conv3d_same: Cin 64 must be a positive multiple of 4 and the kernel 8 x 3 x 3 within 1..7"),
    (dict(kw=0), "conv3d_same: Cin 64 must be a positive multiple of 4 and the kernel 3 x 3 x 0 within 1..7"),
    (dict(st=0), "conv3d_same: strides 0 x 1 x 1 outside 1..4"),
    (dict(sh=5), "conv3d_same: strides 1 x 5 x 1 outside 1..4"),
    (dict(relu=2), "conv3d_same: relu 2"),
    (dict(x_off=2), "conv3d_same: input channels [2, 66) outside the 64 per position, or not 16-byte groups"),
    (dict(x_cs=62), "conv3d_same: input channels [0, 64) outside the 62 per position, or not 16-byte groups"),
    (dict(x_off=4), "conv3d_same: input channels [4, 68) outside the 64 per position, or not 16-byte groups"),
    (dict(split=0), "conv3d_same: split 0 outside 1..Cout (32)"),
    (dict(split=33), "conv3d_same: split 33 outside 1..Cout (32)"),
    (dict(y_off=1), "conv3d_same: output channels [1, 33) outside the 32 per position"),
    (dict(y_cs=16), "conv3d_same: output channels [0, 32) outside the 16 per position"),
    (dict(split=16), "conv3d_same: second output channels [0, 16) outside the 0 per position"),
    (dict(split=16, y2=FAKE.value, y2_cs=8), "conv3d_same: second output channels [0, 16) outside the 8 per position"),
    (dict(split=16, y2=FAKE.value, y2_cs=20, y2_off=8),
     "conv3d_same: second output channels [8, 24) outside the 20 per position"),
    (dict(x=None), "conv3d_same: null pointer"),
    (dict(w=None), "conv3d_same: null pointer"),
    (dict(bias=None), "conv3d_same: null pointer"),
    (dict(y=None), "conv3d_same: null pointer"),
    (dict(x=FAKE.value + 4), "conv3d_same: x and w must be 16-byte aligned"),
    (dict(w=FAKE.value + 8), "conv3d_same: x and w must be 16-byte aligned"),
    (dict(T=0), "conv3d_same: bad sizes B 1 T 0 H 28 W 28 Cout 32"),
    (dict(B=-1), "conv3d_same: bad sizes B -1 T 9 H 28 W 28 Cout 32"),
    (dict(Cout=0), "conv3d_same: bad sizes B 1 T 9 H 28 W 28 Cout 0"),
]


@pytest.mark.parametrize("bad,text", CONV_REJECTS, ids=[f"bad{i}" for i in range(len(CONV_REJECTS))])
def test_conv_abi_rejects(lib, bad, text):
    d = _conv(**bad)
    assert lib.omnitok_conv3d_same(ctypes.byref(d), None) == -1
    assert lib.omnitok_last_error().decode().startswith("conv3d_same")
    assert lib.omnitok_last_error().decode() == text
    assert lib.omnitok_conv3d_same(None, None) == -1
    assert lib.omnitok_last_error().decode() == "conv3d_same: null descriptor"


def test_conv_abi_accepts_empty_batch(lib):
    d = _conv(B=0, x=None, w=None, bias=None, y=None)
    assert lib.omnitok_conv3d_same(ctypes.byref(d), None) == 0
    # the empty-batch return comes after the channel-window checks
    d = _conv(B=0, x=None, w=None, bias=None, y=None, split=0)
    assert lib.omnitok_conv3d_same(ctypes.byref(d), None) == -1
    assert lib.omnitok_last_error().decode() == "conv3d_same: split 0 outside 1..Cout (32)"


def test_packed_ldw(lib):
    assert lib.omnitok_conv3d_packed_ldw(4, 7, 7, 7) == 1376          # 343 taps x 4 channels, rounded up to 32
    assert lib.omnitok_conv3d_packed_ldw(64, 1, 1, 1) == 64
    assert lib.omnitok_conv3d_packed_ldw(24, 3, 3, 3) == 672
    assert lib.omnitok_conv3d_packed_ldw(3, 1, 1, 1) == -1 and lib.omnitok_conv3d_packed_ldw(4, 8, 1, 1) == -1
    w = torch.randn(5, 3, 2, 1, 3)
    p = i3d.pack_conv_weight(w)
    assert p.shape == (5, 32)
    assert torch.equal(p[:, :24].view(5, 2, 1, 3, 4)[..., :3], w.permute(0, 2, 3, 4, 1))
    assert (p[:, :24].view(5, 2, 1, 3, 4)[..., 3] == 0).all() and (p[:, 24:] == 0).all()


@pytest.mark.parametrize("args", [(None, 1, 9, 40, 52, 224, 224, FAKE), (FAKE, 1, 9, 40, 52, 224, 224, None),
                                  (FAKE, 1, 0, 40, 52, 224, 224, FAKE), (FAKE, 1, 9, 0, 52, 224, 224, FAKE),
                                  (FAKE, 1, 9, 40, 52, 0, 224, FAKE), (FAKE, -1, 9, 40, 52, 224, 224, FAKE),
                                  (FAKE, 1, 9, 40, 52, 224, 224, ctypes.c_void_p((1 << 20) + 4))])
def test_preprocess_abi_rejects(lib, args):
    assert lib.omnitok_i3d_preprocess(*args, None) == -1
    assert lib.omnitok_last_error().decode().startswith("i3d_preprocess")


@pytest.mark.parametrize("args", [(FAKE, 1, 9, 28, 28, 6, 3, 3, 3, 2, 2, 2, FAKE), (FAKE, 1, 9, 28, 28, 0, 3, 3, 3, 2, 2, 2, FAKE),
                                  (FAKE, 1, 9, 28, 28, 64, 0, 3, 3, 2, 2, 2, FAKE), (FAKE, 1, 9, 28, 28, 64, 3, 3, 3, 0, 2, 2, FAKE),
                                  (None, 1, 9, 28, 28, 64, 3, 3, 3, 2, 2, 2, FAKE), (FAKE, 1, 9, 28, 28, 64, 3, 3, 3, 2, 2, 2, None),
                                  (FAKE, 1, 0, 28, 28, 64, 3, 3, 3, 2, 2, 2, FAKE),
                                  (ctypes.c_void_p((1 << 20) + 4), 1, 9, 28, 28, 64, 3, 3, 3, 2, 2, 2, FAKE)])
def test_maxpool_abi_rejects(lib, args):
    assert lib.omnitok_maxpool3d_same(*args, None) == -1
    assert lib.omnitok_last_error().decode().startswith("maxpool3d_same")


@pytest.mark.parametrize("args", [(FAKE, 1, 1, 7, 7, 1024, FAKE, FAKE, 400, FAKE), (FAKE, 1, 3, 6, 7, 1024, FAKE, FAKE, 400, FAKE),
                                  (FAKE, 1, 3, 7, 6, 1024, FAKE, FAKE, 400, FAKE), (FAKE, 1, 3, 7, 7, 4096, FAKE, FAKE, 400, FAKE),
                                  (FAKE, 1, 3, 7, 7, 1024, FAKE, FAKE, 0, FAKE), (FAKE, 1, 3, 7, 7, 1024, FAKE, FAKE, 2000, FAKE),
                                  (None, 1, 3, 7, 7, 1024, FAKE, FAKE, 400, FAKE), (FAKE, 1, 3, 7, 7, 1024, None, FAKE, 400, FAKE),
                                  (FAKE, 1, 3, 7, 7, 1024, FAKE, None, 400, FAKE), (FAKE, 1, 3, 7, 7, 1024, FAKE, FAKE, 400, None)])
def test_head_abi_rejects(lib, args):
    assert lib.omnitok_i3d_head(*args, None) == -1
    assert lib.omnitok_last_error().decode().startswith("i3d_head")


def test_synth_state_dict_matches_reference_keys():
    keys = np.load(os.path.join(GOLDEN, "fvd_keys.npz"))
    sd = synth.synth_i3d_state_dict(0)
    assert list(sd) == list(keys["keys"])
    assert [",".join(map(str, v.shape)) for v in sd.values()] == list(keys["shapes"])
    assert sd["Mixed_4f.b1b.bn.running_var"].dtype == torch.float32
    assert sd["Conv3d_1a_7x7.bn.num_batches_tracked"].dtype == torch.int64
    assert torch.equal(sd["logits.conv3d.bias"], synth.synth_i3d_state_dict(0)["logits.conv3d.bias"])


def test_fixture_endpoints_stay_order_one():
    for case in CASES:
        f = _fix(case)
        assert list(f["rms_names"]) == i3d.ENDPOINTS[:-1]
        assert (f["rms"] > 0.2).all() and (f["rms"] < 5).all(), f["rms"]


@pytest.mark.parametrize("case", CASES)
def test_logit_bar_holds_the_reference_fp32_run(case):
    from tests.test_gpu_fvd import logit_bar
    f = _fix(case)
    err = np.abs(f["logits32"].astype(np.float64) - f["logits64"]).max()
    bar = logit_bar(f["logits64"])
    assert err <= bar, (err, bar)


@pytest.mark.parametrize("case", CASES)
def test_frechet_distance_matches_reference(case):
    f = _fix(case)
    l32, l64 = torch.from_numpy(f["logits32"]), torch.from_numpy(f["logits64"])
    D, n = l64.shape[2], l64.shape[1]
    for j, (a, b) in enumerate([(0, 1), (0, 2), (0, 0)]):
        got = fvd.frechet_distance(l64[a], l64[b]).item()
        want = float(f["fvd64"][j])
        assert abs(got - want) <= 1e-9 * max(abs(want), 1.0), (j, got, want)
        tr = max(fvd.cov(l64[a].double()).trace().item(), fvd.cov(l64[b].double()).trace().item())
        bar32 = 2 * (D - n + 1) * np.sqrt(D * U * tr) + 1e-5 * abs(want)
        got32 = fvd.frechet_distance(l32[a], l32[b]).item()
        assert abs(got32 - float(f["fvd32"][j])) <= bar32, (j, got32, float(f["fvd32"][j]), bar32)
    assert fvd.frechet_distance(l64[0], l64[0]).abs().item() < 1e-9


def test_model_rejects_unsupported_configurations():
    with pytest.raises(NotImplementedError):
        i3d.InceptionI3d(400, is_coinrun=True)
    with pytest.raises(NotImplementedError):
        i3d.InceptionI3d(400, final_endpoint="Mixed_5c")
    with pytest.raises(NotImplementedError):
        i3d.InceptionI3d(400, in_channels=2)
    with pytest.raises(ValueError):
        i3d.InceptionI3d(400, final_endpoint="nope")
    m = i3d.InceptionI3d(400)
    sd = synth.synth_i3d_state_dict(1)
    m.load_state_dict(sd)
    assert list(m.state_dict()) == list(sd)
    del sd["Mixed_4f.b1b.bn.running_var"]
    with pytest.raises(RuntimeError, match="missing"):
        i3d.InceptionI3d(400).load_state_dict(sd)
    with pytest.raises(RuntimeError, match="GPU"):
        m(torch.zeros(1, 3, 9, 224, 224))


# the full texts of the commit before the shared strict check and weight holder (omnitokenizer_amd/convnet.py)
_PRE = "Error(s) in loading state_dict for InceptionI3d: "
STRICT_TEXT = {
    "missing": _PRE + "missing keys ['Mixed_4f.b1b.bn.running_var'], unexpected keys []",
    "extra": _PRE + "missing keys [], unexpected keys ['Mixed_5c.b3b.conv3d.bias']",
    "shape": _PRE + (
        "size mismatch for Mixed_3b.b1b.conv3d.weight: copying a param with shape (128, 96, 1, 3, 3), the model has "
        "(128, 96, 3, 3, 3)"),
    "truncated": _PRE + ("missing keys ['Mixed_5c.b3b.conv3d.weight', 'Mixed_5c.b3b.bn.weight', 'Mixed_5c.b3b.bn.bias', "
        "'Mixed_5c.b3b.bn.running_mean', 'Mixed_5c.b3b.bn.running_var', 'Mixed_5c.b3b.bn.num_batches_tracked'], "
        "unexpected keys ['extra.0', 'extra.1', 'extra.2', 'extra.3', 'extra.4', 'extra.5', 'extra.6', 'extra.7'] ..."),
}


@pytest.mark.parametrize("edit", list(STRICT_TEXT))
def test_strict_loading_rejects(edit):
    sd = synth.synth_i3d_state_dict(1)
    if edit == "missing":
        del sd["Mixed_4f.b1b.bn.running_var"]
    elif edit == "extra":
        sd["Mixed_5c.b3b.conv3d.bias"] = torch.zeros(128)
    elif edit == "shape":
        sd["Mixed_3b.b1b.conv3d.weight"] = torch.zeros(128, 96, 1, 3, 3)
    else:   # more than 8 unexpected keys: the first 8, then " ..."
        for k in [k for k in sd if k.startswith("Mixed_5c.b3b.")]:
            del sd[k]
        sd.update({f"extra.{j}": torch.zeros(1) for j in range(9)})
    m = i3d.InceptionI3d(400)
    with pytest.raises(RuntimeError) as e:
        m.load_state_dict(sd)
    assert str(e.value) == STRICT_TEXT[edit]
    with pytest.raises(RuntimeError) as e:
        m.state_dict()
    assert str(e.value) == "InceptionI3d: no weights loaded"
    with pytest.raises(RuntimeError) as e:
        m._weights(torch.device("cpu"))
    assert str(e.value) == "InceptionI3d: load_state_dict first"


def test_input_checks():
    m = i3d.InceptionI3d(400)
    m.load_state_dict(synth.synth_i3d_state_dict(0))
    u = np.zeros((2, 9, 32, 32, 3), np.uint8)
    with pytest.raises(TypeError):
        fvd.get_fvd_logits(u.astype(np.float32), m, "cuda")
    with pytest.raises(ValueError, match=r"\[B, T, H, W, 3\]"):
        fvd.get_fvd_logits(np.zeros((2, 9, 32, 32, 4), np.uint8), m, "cuda")
    with pytest.raises(ValueError, match="at least 9 frames"):
        fvd.get_fvd_logits(np.zeros((2, 8, 32, 32, 3), np.uint8), m, "cuda")
    with pytest.raises(RuntimeError, match="GPU"):
        fvd.get_fvd_logits(torch.from_numpy(u), m, None)
    with pytest.raises(RuntimeError, match="GPU"):
        fvd.get_fvd_logits(u, m, "cpu")
    with pytest.raises(ValueError, match="193"):
        i3d.check_input_size(17, 192, 224)
    i3d.check_input_size(9, 193, 193)
    with pytest.raises(ValueError, match="9 frames"):
        i3d.check_input_size(8, 224, 224)
    assert i3d.final_grid(17, 224, 224) == (3, 7, 7) and i3d.final_grid(16, 256, 320) == (2, 8, 10)
