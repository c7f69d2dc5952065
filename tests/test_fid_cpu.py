"""CPU: the Inception V3 / FID layer (csrc/inception.hip, omnitokenizer_amd/inception.py, omnitokenizer_amd/fid.py) --
exported symbols, argument validation of the C ABI (it runs before any launch, so no GPU is needed), the synthetic weights
and both key sets against the reference's state_dicts, the soundness of the feature bar of tests/test_gpu_fid.py,
calculate_frechet_distance and the .npz statistics against the reference's values, and the Python layer's input checks.

Bars: calculate_frechet_distance on the fixture's fp64 activations is the reference's fp64 computation (np.cov, the same
scipy sqrtm): 1e-9 of the traces it sums (sqrtm's blocking may differ between builds).  The fp32 activations give the
reference's fp32 value to the same bar: both sides compute from the same fp32 numbers widened to fp64.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from omnitokenizer_amd import _lib, fid, inception, synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FAKE = ctypes.c_void_p(1 << 20)   # a non-null, aligned pointer that no check dereferences
FEATURE_CASES = ["fid_64x80", "fid_299x299"]
SYMBOLS = ("omnitok_fid_preprocess", "omnitok_conv2d_out", "omnitok_conv2d", "omnitok_maxpool2d", "omnitok_avgpool2d",
           "omnitok_spatial_mean")


@pytest.fixture(scope="module")
def lib():
    from omnitokenizer_amd import build
    build.build()
    return _lib.load()


def _fix(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def test_symbols_exported(lib):
    for name in SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS and getattr(lib, name)
    import omnitokenizer_amd as pkg
    for name in ("InceptionV3", "load_fid_inception", "calculate_activation_statistics", "calculate_frechet_distance",
                 "compute_statistics_of_path", "calculate_fid_given_paths", "save_fid_stats", "compute_fid"):
        assert name in pkg.__all__ and getattr(pkg, name)
    assert pkg.frechet_distance.__module__ == "omnitokenizer_amd.fvd"


@pytest.mark.parametrize("s,k,stride,pad,out", [(299, 3, 2, 0, 149), (149, 3, 1, 0, 147), (147, 3, 1, 1, 147),
                                                (147, 3, 2, 0, 73), (71, 3, 2, 0, 35), (35, 3, 2, 0, 17),
                                                (17, 3, 2, 0, 8), (17, 7, 1, 3, 17), (35, 5, 1, 2, 35), (2, 3, 1, 0, 0)])
def test_out_size(lib, s, k, stride, pad, out):
    assert lib.omnitok_conv2d_out(s, k, stride, pad) == out == inception.out_size(s, k, stride, pad)


def _conv(**kw):
    d = _lib.OmnitokConv2d()
    base = dict(x=FAKE.value, x_cs=64, x_off=0, N=1, H=35, W=35, Cin=64, w=FAKE.value, bias=FAKE.value, Cout=32, kh=3, kw=3,
                sh=1, sw=1, ph=1, pw=1, relu=1, y=FAKE.value, y_cs=32, y_off=0, y2=None, y2_cs=0, y2_off=0, split=32)
    base.update(kw)
    for k, v in base.items():
        setattr(d, k, v)
    return d


# every bad descriptor with the full omnitok_last_error() text of the commit before the shared host side
# (conv_args in csrc/convnet_common.h)
CONV_REJECTS = [
    (dict(Cin=3, x_cs=4), "conv2d: Cin 3 must be a positive multiple of 4 and the kernel 3 x 3 within 1..7"),
    (dict(Cin=0), "conv2d: Cin 0 must be a positive multiple of 4 and the kernel 3 x 3 within 1..7"),
    (dict(kh=8), "conv2d: Cin 64 must be a positive multiple of 4 and the kernel 8 x 3 within 1..7"),
    (dict(kw=0), "conv2d: Cin 64 must be a positive multiple of 4 and the kernel 3 x 0 within 1..7"),
    (dict(sh=0), "conv2d: strides 0 x 1 outside 1..4"),
    (dict(sw=5), "conv2d: strides 1 x 5 outside 1..4"),
    (dict(ph=3), "conv2d: padding 3 x 1 outside 0..kernel - 1"),
    (dict(pw=-1), "conv2d: padding 1 x -1 outside 0..kernel - 1"),
    (dict(relu=2), "conv2d: relu 2"),
    (dict(x_off=2), "conv2d: input channels [2, 66) outside the 64 per position, or not 16-byte groups"),
    (dict(x_cs=62), "conv2d: input channels [0, 64) outside the 62 per position, or not 16-byte groups"),
    (dict(x_off=4), "conv2d: input channels [4, 68) outside the 64 per position, or not 16-byte groups"),
    (dict(split=0), "conv2d: split 0 outside 1..Cout (32)"),
    (dict(split=33), "conv2d: split 33 outside 1..Cout (32)"),
    (dict(y_off=1), "conv2d: output channels [1, 33) outside the 32 per position"),
    (dict(y_cs=16), "conv2d: output channels [0, 32) outside the 16 per position"),
    (dict(split=16), "conv2d: second output channels [0, 16) outside the 0 per position"),
    (dict(split=16, y2=FAKE.value, y2_cs=8), "conv2d: second output channels [0, 16) outside the 8 per position"),
    (dict(split=16, y2=FAKE.value, y2_cs=20, y2_off=8), "conv2d: second output channels [8, 24) outside the 20 per position"),
    (dict(x=None), "conv2d: null pointer"),
    (dict(w=None), "conv2d: null pointer"),
    (dict(bias=None), "conv2d: null pointer"),
    (dict(y=None), "conv2d: null pointer"),
    (dict(x=FAKE.value + 4), "conv2d: x and w must be 16-byte aligned"),
    (dict(w=FAKE.value + 8), "conv2d: x and w must be 16-byte aligned"),
    (dict(H=0), "conv2d: bad sizes N 1 H 0 W 35 Cout 32"),
    (dict(N=-1), "conv2d: bad sizes N -1 H 35 W 35 Cout 32"),
    (dict(Cout=0), "conv2d: bad sizes N 1 H 35 W 35 Cout 0"),
    (dict(H=2, W=2, ph=0, pw=0), "conv2d: empty output (2 x 2 input, kernel 3 x 3, padding 0 x 0)"),
]


@pytest.mark.parametrize("bad,text", CONV_REJECTS, ids=[f"bad{i}" for i in range(len(CONV_REJECTS))])
def test_conv_abi_rejects(lib, bad, text):
    d = _conv(**bad)
    assert lib.omnitok_conv2d(ctypes.byref(d), None) == -1
    assert lib.omnitok_last_error().decode().startswith("conv2d")
    assert lib.omnitok_last_error().decode() == text
    assert lib.omnitok_conv2d(None, None) == -1
    assert lib.omnitok_last_error().decode() == "conv2d: null descriptor"


def test_conv_abi_accepts_empty_batch(lib):
    d = _conv(N=0, x=None, w=None, bias=None, y=None)
    assert lib.omnitok_conv2d(ctypes.byref(d), None) == 0
    # the empty-batch return comes after the channel-window checks and after the empty-output check
    d = _conv(N=0, x=None, w=None, bias=None, y=None, split=0)
    assert lib.omnitok_conv2d(ctypes.byref(d), None) == -1
    assert lib.omnitok_last_error().decode() == "conv2d: split 0 outside 1..Cout (32)"
    d = _conv(N=0, x=None, w=None, bias=None, y=None, H=2, W=2, ph=0, pw=0)
    assert lib.omnitok_conv2d(ctypes.byref(d), None) == -1
    assert lib.omnitok_last_error().decode() == "conv2d: empty output (2 x 2 input, kernel 3 x 3, padding 0 x 0)"


@pytest.mark.parametrize("args", [
    (None, 0, 240, 4, 64, 80, 299, 299, 3, FAKE), (FAKE, 0, 240, 4, 64, 80, 299, 299, 3, None),
    (FAKE, 2, 240, 4, 64, 80, 299, 299, 3, FAKE), (FAKE, 0, 240, 4, 64, 80, 299, 299, 4, FAKE),
    (FAKE, 0, 239, 4, 64, 80, 299, 299, 3, FAKE), (FAKE, 0, 240, -1, 64, 80, 299, 299, 3, FAKE),
    (FAKE, 0, 240, 4, 0, 80, 299, 299, 3, FAKE), (FAKE, 1, 0, 4, 64, 80, 0, 299, 3, FAKE),
    (FAKE, 1, 0, 4, 64, 80, 299, 299, 2, FAKE), (FAKE, 0, 240, 4, 64, 80, 299, 299, 3, ctypes.c_void_p((1 << 20) + 4))])
def test_preprocess_abi_rejects(lib, args):
    """bad pointer, dtype, flags, row stride below 3 W, sizes, and a size change without the resize flag"""
    assert lib.omnitok_fid_preprocess(*args, None) == -1
    assert lib.omnitok_last_error().decode().startswith("fid_preprocess")


@pytest.mark.parametrize("fn", ["omnitok_maxpool2d", "omnitok_avgpool2d"])
@pytest.mark.parametrize("args", [
    (FAKE, 1, 35, 35, 6, 3, 2, 0, FAKE, 8, 0), (FAKE, 1, 35, 35, 0, 3, 2, 0, FAKE, 8, 0),
    (FAKE, 1, 35, 35, 64, 0, 2, 0, FAKE, 64, 0), (FAKE, 1, 35, 35, 64, 3, 0, 0, FAKE, 64, 0),
    (FAKE, 1, 35, 35, 64, 3, 1, 2, FAKE, 64, 0), (FAKE, 1, 2, 2, 64, 3, 1, 0, FAKE, 64, 0),
    (FAKE, 1, 35, 35, 64, 3, 2, 0, FAKE, 64, 4), (FAKE, 1, 35, 35, 64, 3, 2, 0, FAKE, 68, 2),
    (None, 1, 35, 35, 64, 3, 2, 0, FAKE, 64, 0), (FAKE, 1, 35, 35, 64, 3, 2, 0, None, 64, 0),
    (FAKE, -1, 35, 35, 64, 3, 2, 0, FAKE, 64, 0),
    (ctypes.c_void_p((1 << 20) + 4), 1, 35, 35, 64, 3, 2, 0, FAKE, 64, 0)])
def test_pool_abi_rejects(lib, fn, args):
    """C not a multiple of 4, kernel / stride outside range, padding above k / 2, an empty output, an output slice outside
    the row or not 16-byte aligned, null or misaligned pointers"""
    assert getattr(lib, fn)(*args, None) == -1
    assert lib.omnitok_last_error().decode().startswith(fn[len("omnitok_"):])


@pytest.mark.parametrize("args", [(FAKE, 1, 8, 8, 6, FAKE), (FAKE, 1, 0, 8, 2048, FAKE), (FAKE, -1, 8, 8, 2048, FAKE),
                                  (None, 1, 8, 8, 2048, FAKE), (FAKE, 1, 8, 8, 2048, None),
                                  (FAKE, 1, 8, 8, 2048, ctypes.c_void_p((1 << 20) + 8))])
def test_spatial_mean_abi_rejects(lib, args):
    assert lib.omnitok_spatial_mean(*args, None) == -1
    assert lib.omnitok_last_error().decode().startswith("spatial_mean")


def test_synth_state_dict_matches_reference_keys():
    keys = np.load(os.path.join(GOLDEN, "fid_keys.npz"))
    sd = synth.synth_fid_inception_state_dict(0)
    assert list(sd) == list(keys["pth_keys"])
    assert [",".join(map(str, v.shape)) for v in sd.values()] == list(keys["pth_shapes"])
    spec = inception.state_spec(wrapper=True)
    assert list(spec) == list(keys["wrapper_keys"])
    assert [",".join(map(str, s)) for s, _ in spec.values()] == list(keys["wrapper_shapes"])
    assert sd["Mixed_7c.branch_pool.bn.running_var"].dtype == torch.float32
    assert sd["Conv2d_1a_3x3.bn.num_batches_tracked"].dtype == torch.int64
    assert torch.equal(sd["fc.bias"], synth.synth_fid_inception_state_dict(0)["fc.bias"])


def _wrapper_sd(sd, last_block=3):
    """the .pth state_dict under InceptionV3's own names (what the reference's InceptionV3.state_dict() holds)"""
    pth = [p for p, _ in inception._convs_with_keys(False, last_block)]
    own = [p for p, _ in inception._convs_with_keys(True, last_block)]
    out = {}
    for a, b in zip(pth, own):
        for k, v in sd.items():
            if k.startswith(a + "."):
                out[b + k[len(a):]] = v
    return out


def test_strict_loading_accepts_both_key_sets():
    sd = synth.synth_fid_inception_state_dict(3)
    m = inception.InceptionV3([3])
    m.load_state_dict(sd)
    via_pth = m.state_dict()
    keys = np.load(os.path.join(GOLDEN, "fid_keys.npz"))
    assert list(via_pth) == list(keys["wrapper_keys"])
    m2 = inception.InceptionV3([3])
    m2.load_state_dict(_wrapper_sd(sd))
    assert all(torch.equal(via_pth[k], v) for k, v in m2.state_dict().items())
    # a block-0 model holds (and takes) only block 0's wrapper keys; the .pth file always works
    m0 = inception.InceptionV3([0])
    m0.load_state_dict(_wrapper_sd(sd, 0))
    assert len(m0.state_dict()) == 18
    inception.InceptionV3([0]).load_state_dict(sd)
    # checkpoints without num_batches_tracked (torch's BatchNorm accepts them)
    inception.InceptionV3([3]).load_state_dict({k: v for k, v in sd.items() if "num_batches_tracked" not in k})


# the full texts of the commit before the shared strict check (omnitokenizer_amd/convnet.py)
_PRE = "Error(s) in loading state_dict for InceptionV3: "
STRICT_TEXT = {
    "missing": _PRE + "missing keys ['Mixed_6e.branch7x7dbl_4.bn.running_var'], unexpected keys []",
    "extra": _PRE + "missing keys [], unexpected keys ['AuxLogits.fc.weight']",
    "shape": _PRE + (
        "size mismatch for Mixed_5b.branch_pool.conv.weight: copying a param with shape (64, 192, 1, 1), the model has "
        "(32, 192, 1, 1)"),
    "no_fc": _PRE + "missing keys ['fc.weight', 'fc.bias'], unexpected keys []",
    "wrapper_extra_block": _PRE + (
        "missing keys [], unexpected keys ['blocks.2.0.branch1x1.conv.weight', 'blocks.2.0.branch1x1.bn.weight', "
        "'blocks.2.0.branch1x1.bn.bias', 'blocks.2.0.branch1x1.bn.running_mean', "
        "'blocks.2.0.branch1x1.bn.running_var', 'blocks.2.0.branch1x1.bn.num_batches_tracked', "
        "'blocks.2.0.branch5x5_1.conv.weight', 'blocks.2.0.branch5x5_1.bn.weight'] ..."),
    "some_nbt": _PRE + "missing keys ['Conv2d_2a_3x3.bn.num_batches_tracked'], unexpected keys []",
}


@pytest.mark.parametrize("edit", ["missing", "extra", "shape", "no_fc", "wrapper_extra_block", "some_nbt"])
def test_strict_loading_rejects(edit):
    sd = synth.synth_fid_inception_state_dict(3)
    m = inception.InceptionV3([3])
    if edit == "missing":
        del sd["Mixed_6e.branch7x7dbl_4.bn.running_var"]
    elif edit == "extra":
        sd["AuxLogits.fc.weight"] = torch.zeros(1000, 768)
    elif edit == "shape":
        sd["Mixed_5b.branch_pool.conv.weight"] = torch.zeros(64, 192, 1, 1)
    elif edit == "no_fc":
        del sd["fc.weight"], sd["fc.bias"]
    elif edit == "wrapper_extra_block":
        m = inception.InceptionV3([1])
        sd = _wrapper_sd(sd, 2)
    elif edit == "some_nbt":
        del sd["Conv2d_2a_3x3.bn.num_batches_tracked"]
    with pytest.raises(RuntimeError, match="Error") as e:
        m.load_state_dict(sd)
    assert str(e.value) == STRICT_TEXT[edit]


def test_fixture_blocks_stay_order_one():
    for case in FEATURE_CASES:
        f = _fix(case)
        assert list(f["rms_names"]) == ["block0", "block1", "block2", "block3"]
        assert (f["rms"] > 0.2).all() and (f["rms"] < 8).all(), f["rms"]


@pytest.mark.parametrize("case", FEATURE_CASES + ["fid_dist_d64"])
def test_feature_bar_holds_the_reference_fp32_run(case):
    from tests.test_gpu_fid import feature_bar
    f = _fix(case)
    dims = [64] if case == "fid_dist_d64" else [64, 192, 768, 2048]
    for d in dims:
        a32, a64 = (f["act32"], f["act64"]) if case == "fid_dist_d64" else (f[f"act32_{d}"], f[f"act64_{d}"])
        err = np.abs(a32.astype(np.float64) - a64).max()
        bar = feature_bar(a64, d)
        assert err <= bar, (d, err, bar)
        assert err > 0   # the fp32 run does round: the bar is not vacuous


def _stats(a):
    return np.mean(a, axis=0), np.cov(a, rowvar=False)


def test_frechet_distance_matches_reference():
    f = _fix("fid_dist_d64")
    for tag in ("64", "32"):
        act = f["act" + tag].astype(np.float64)
        st = [_stats(a) for a in act]
        for j, (a, b) in enumerate([(0, 1), (0, 2), (0, 0)]):
            got = fid.calculate_frechet_distance(*st[a], *st[b])
            want = float(f["fid" + tag][j])
            tol = 1e-9 * (np.trace(st[a][1]) + np.trace(st[b][1]))
            assert abs(got - want) <= tol, (tag, j, got, want, tol)
    assert abs(float(f["fid_paths"]) - float(f["fid32"][0])) <= 1e-9 * float(f["fid32"][0])
    with pytest.raises(ValueError):
        fid.calculate_frechet_distance(np.zeros(3), np.eye(3), np.zeros(4), np.eye(4))


def test_npz_statistics_round_trip(tmp_path):
    """compute_statistics_of_path and calculate_fid_given_paths on .npz files (no model is needed for them)"""
    f = _fix("fid_dist_d64")
    paths = []
    for i, a in enumerate(f["act64"][:2]):
        mu, sigma = _stats(a)
        p = str(tmp_path / f"s{i}.npz")
        np.savez_compressed(p, mu=mu, sigma=sigma)
        m2, s2 = fid.compute_statistics_of_path(p, None, 50, 64, None)
        assert np.array_equal(m2, mu) and np.array_equal(s2, sigma)
        paths.append(p)
    got = fid.calculate_fid_given_paths(paths, 50, "cuda", 64)
    want = float(f["fid64"][0])
    assert abs(got - want) <= 1e-9 * np.trace(_stats(f["act64"][0])[1]) * 2
    with pytest.raises(RuntimeError, match="Invalid path"):
        fid.calculate_fid_given_paths([paths[0], str(tmp_path / "nope")], 50, "cuda", 64)
    with pytest.raises(ValueError, match="weights"):
        fid.calculate_fid_given_paths([paths[0], str(tmp_path)], 50, "cuda", 64)
    with pytest.raises(RuntimeError, match="Existing"):
        fid.save_fid_stats([str(tmp_path), paths[0]], 50, "cuda", 64)


def test_min_input_size():
    """the reference's forward needs every layer to have an output: 11, 27, 43, 75 pixels for blocks 0..3"""
    assert [inception.min_input_size(b) for b in range(4)] == [11, 27, 43, 75]
    for b, s in enumerate([11, 27, 43, 75]):
        inception.check_input_size(s, s, b)
        with pytest.raises(ValueError, match="too small"):
            inception.check_input_size(s - 1, s + 40, b)
    ext = dict((n, (h, w)) for n, h, w in inception.block_extents(299, 299))
    assert ext["maxpool1"] == (73, 73) and ext["maxpool2"] == (35, 35) and ext["Mixed_6e"] == (17, 17)
    assert ext["Mixed_7c"] == (8, 8)


def test_model_and_input_checks():
    with pytest.raises(NotImplementedError):
        inception.InceptionV3(use_fid_inception=False)
    with pytest.raises(ValueError):
        inception.InceptionV3([4])
    m = inception.InceptionV3([3])
    with pytest.raises(RuntimeError, match="GPU"):
        m(torch.zeros(1, 3, 299, 299))
    m.load_state_dict(synth.synth_fid_inception_state_dict(0))
    with pytest.raises(ValueError, match="dims"):
        fid.get_activations(np.zeros((2, 32, 32, 3), np.uint8), m, dims=100, device="cuda")
    with pytest.raises(ValueError, match="block"):
        fid.get_activations(np.zeros((2, 32, 32, 3), np.uint8), m, dims=64, device="cuda")
    with pytest.raises(ValueError, match="dims"):
        fid.load_fid_inception("cuda", "unused.pth", dims=1000)
    with pytest.raises(RuntimeError, match="GPU"):
        fid.get_activations(np.zeros((2, 32, 32, 3), np.uint8), m, device="cpu")
    small = inception.InceptionV3([3], resize_input=False)
    with pytest.raises(ValueError, match="too small"):
        small(torch.zeros(1, 3, 74, 299))
