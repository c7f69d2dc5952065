"""CPU: LPIPS (csrc/lpips.hip, omnitokenizer_amd/lpips.py) -- exported symbols, argument validation of the C ABI (it runs
before any launch, so no GPU is needed), the synthetic weights against the reference's LPIPS().state_dict() key set, the
three weight sources of load_lpips, the soundness of the bar of tests/test_gpu_lpips.py on the reference's own fp32 run,
and the custom operators' schemas and fake-tensor shapes.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from omnitokenizer_amd import _lib, lpips, synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FAKE = 1 << 20   # a non-null, aligned address that no check dereferences
CASES = ["lpips_16x16", "lpips_50x70", "lpips_64x64", "lpips_256x256", "lpips_same_32x32", "lpips_light_40x40"]
SYMBOLS = ("omnitok_lpips_preprocess", "omnitok_lpips_workspace", "omnitok_lpips_layer", "omnitok_lpips_finalize")


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
    for name in ("LPIPS", "load_lpips", "lpips_frames"):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(lpips, name)


def _operand(**kw):
    d = _lib.OmnitokMetricsOperand()
    d.data = kw.pop("data", FAKE)
    strides = kw.pop("stride", (3 * 32 * 32, 3 * 32 * 32, 32 * 32, 32, 1))
    for k in range(5):
        d.stride[k] = strides[k]
    d.dtype = kw.pop("dtype", 0)
    d.clamp = kw.pop("clamp", 0)
    d.shift = kw.pop("shift", 0.0)
    assert not kw
    return d


def _pre(lib, op=None, B=2, F=1, H=32, W=32, i0=0, n=2, flags=0, shift=(-.03, -.088, -.188), scale=(.458, .448, .45),
         out=FAKE):
    d = op if op is not None else _operand()
    sh = (ctypes.c_float * 3)(*shift) if shift is not None else None
    sc = (ctypes.c_float * 3)(*scale) if scale is not None else None
    return lib.omnitok_lpips_preprocess(ctypes.byref(d) if d is not False else None, B, F, H, W, i0, n, flags, sh, sc,
                                        ctypes.c_void_p(out) if out else None, None)


@pytest.mark.parametrize("bad", [
    dict(op=False), dict(op="data"), dict(H=15), dict(W=8), dict(flags=2), dict(flags=-1), dict(op="dtype"),
    dict(op="stride"), dict(op="clamp"), dict(op="shift"), dict(shift=None), dict(scale=None), dict(scale=(1.0, 0.0, 1.0)),
    dict(shift=(float("nan"), 0.0, 0.0)), dict(i0=1), dict(n=3), dict(i0=-1), dict(n=-1), dict(out=0), dict(out=FAKE + 4),
    dict(B=-1), dict(F=0)])
def test_preprocess_abi_rejects(lib, bad):
    op = bad.pop("op", None)
    if op == "data":
        op = _operand(data=0)
    elif op == "dtype":
        op = _operand(dtype=2)
    elif op == "stride":
        op = _operand(stride=(0, 0, -1024, 32, 1))
    elif op == "clamp":
        op = _operand(clamp=2)
    elif op == "shift":
        op = _operand(shift=float("inf"))
    assert _pre(lib, op, **bad) == -1
    assert lib.omnitok_last_error().decode().startswith("lpips_preprocess")


def test_preprocess_abi_accepts_uint8_shift_and_empty(lib):
    # a uint8 operand may carry a shift here (unlike omnitok_frame_metrics); n = 0 launches nothing
    assert _pre(lib, _operand(dtype=1, shift=-0.5, stride=(3 * 32 * 32, 0, 1, 96, 3)), n=0) == 0
    assert _pre(lib, _operand(data=0), n=0, out=0) == 0


def _layer(lib, feats=FAKE, N=2, h=16, w=16, C=64, lin_w=FAKE, layer=0, work=FAKE, work_bytes=None, res=FAKE):
    need = lib.omnitok_lpips_workspace(max(N, 0), h, w)
    work_bytes = need if work_bytes is None else work_bytes
    p = lambda a: ctypes.c_void_p(a) if a else None  # noqa: E731
    return lib.omnitok_lpips_layer(p(feats), N, h, w, C, p(lin_w), layer, p(work), max(work_bytes, 0), p(res), None)


@pytest.mark.parametrize("bad", [
    dict(C=516), dict(C=1024), dict(C=6), dict(C=0), dict(h=0), dict(w=-1), dict(N=-1), dict(N=65536), dict(layer=5),
    dict(layer=-1), dict(feats=0), dict(lin_w=0), dict(res=0), dict(work=0), dict(work_bytes=8), dict(feats=FAKE + 4),
    dict(lin_w=FAKE + 8)])
def test_layer_abi_rejects(lib, bad):
    assert _layer(lib, **bad) == -1
    assert lib.omnitok_last_error().decode().startswith("lpips_layer")


def test_workspace_and_finalize_abi(lib):
    assert lib.omnitok_lpips_workspace(3, 256, 256) == 3 * 1024 * 8       # strips of 64 pixels
    assert lib.omnitok_lpips_workspace(2, 17, 13) == 2 * 4 * 8
    assert lib.omnitok_lpips_workspace(2, 33, 33) == 2 * 18 * 8
    assert lib.omnitok_lpips_workspace(-1, 16, 16) == -1 and lib.omnitok_lpips_workspace(1, 0, 16) == -1
    assert _layer(lib, C=512, N=0, feats=0, lin_w=0, work=0, res=0) == 0
    assert lib.omnitok_lpips_finalize(None, 2, ctypes.c_void_p(FAKE), None) == -1
    assert lib.omnitok_lpips_finalize(ctypes.c_void_p(FAKE), 2, None, None) == -1
    assert lib.omnitok_lpips_finalize(ctypes.c_void_p(FAKE), -1, ctypes.c_void_p(FAKE), None) == -1
    assert lib.omnitok_lpips_finalize(None, 0, None, None) == 0


def test_synth_state_dict_matches_reference_keys():
    f = _fix("lpips_keys")
    sd = synth.synth_lpips_state_dict(5)
    assert list(sd) == list(f["keys"]) == list(lpips.state_spec())
    assert [",".join(map(str, v.shape)) for v in sd.values()] == list(f["shapes"])
    assert all(v.dtype == torch.float32 for v in sd.values())
    assert all((sd[f"lin{k}.model.1.weight"] >= 0).all() for k in range(5))
    assert torch.equal(sd["scaling_layer.shift"].view(-1), torch.tensor(lpips.SCALING_SHIFT, dtype=torch.float32))
    assert torch.equal(sd["scaling_layer.scale"].view(-1), torch.tensor(lpips.SCALING_SCALE, dtype=torch.float32))
    assert not torch.equal(sd["net.slice1.0.weight"], synth.synth_lpips_state_dict(6)["net.slice1.0.weight"])


def _packed_equal(p, q):
    assert p["shift"] == q["shift"] and p["scale"] == q["scale"]
    assert len(p["convs"]) == len(q["convs"]) == 13
    for (s1, w1, b1), (s2, w2, b2) in zip(p["convs"], q["convs"]):
        assert s1 == s2 and torch.equal(w1, w2) and torch.equal(b1, b2)
    assert all(torch.equal(a, b) for a, b in zip(p["lins"], q["lins"]))


def test_load_lpips_sources_agree(lib, tmp_path):
    sd = synth.synth_lpips_state_dict(7)
    direct = lpips.load_lpips("cpu", sd).packed("cpu")
    ckpt = {"state_dict": {**{f"perceptual_model.{k}": v for k, v in sd.items()},
                           "encoder.conv_first.weight": torch.zeros(1), "image_discriminator.x": torch.zeros(2)}}
    path = tmp_path / "tok.ckpt"
    torch.save(ckpt, path)
    vgg, lin = lpips.to_torchvision(sd)
    vgg = dict(vgg, **{"classifier.0.weight": torch.zeros(4, 2), "classifier.0.bias": torch.zeros(4)})
    torch.save(lin, tmp_path / "vgg.pth")
    for src in (str(path), ckpt["state_dict"], (vgg, str(tmp_path / "vgg.pth")), (vgg, lin)):
        _packed_equal(direct, lpips.load_lpips("cpu", src).packed("cpu"))
    m = lpips.load_lpips("cpu", sd)
    assert list(m.state_dict()) == list(sd) and all(torch.equal(m.state_dict()[k], sd[k]) for k in sd)
    w0 = direct["convs"][0][1]   # the first conv's Cin 3 padded to 4: channel 3 of every tap has weight 0
    assert w0.shape[0] == 64 and w0.shape[1] >= 36 and (w0[:, 3:36:4] == 0).all() and (w0[:, 0:36:4] != 0).any()


# the full texts of the commit before the shared strict check (omnitokenizer_amd/convnet.py)
STRICT_TEXT = {
    "missing": "Error(s) in loading state_dict for LPIPS: missing keys ['lin3.model.1.weight'], unexpected keys []",
    "extra": "Error(s) in loading state_dict for LPIPS: missing keys [], unexpected keys ['net.slice5.30.weight']",
    "shape": ("Error(s) in loading state_dict for LPIPS: size mismatch for net.slice2.5.weight: copying a param with shape "
        "(128, 64, 1, 1), the model has (128, 64, 3, 3)"),
    "vgg16": "Error(s) in loading state_dict for torchvision vgg16: missing keys ['features.28.bias'], unexpected keys []",
}


@pytest.mark.parametrize("edit", ["missing", "extra", "shape"])
def test_load_lpips_is_strict(lib, edit):
    sd = dict(synth.synth_lpips_state_dict(7))
    if edit == "missing":
        del sd["lin3.model.1.weight"]
    elif edit == "extra":
        sd["net.slice5.30.weight"] = torch.zeros(1)
    else:
        sd["net.slice2.5.weight"] = torch.zeros(128, 64, 1, 1)
    with pytest.raises(RuntimeError, match="loading state_dict") as e:
        lpips.load_lpips("cpu", sd)
    assert str(e.value) == STRICT_TEXT[edit]
    vgg, lin = lpips.to_torchvision(synth.synth_lpips_state_dict(7))
    del vgg["features.28.bias"]
    with pytest.raises(RuntimeError, match="vgg16") as e:
        lpips.load_lpips("cpu", (vgg, lin))
    assert str(e.value) == STRICT_TEXT["vgg16"]
    for call, text in ((lpips.LPIPS().state_dict, "LPIPS: no weights loaded"),
                       (lambda: lpips.LPIPS().packed("cpu"), "LPIPS: load_state_dict first (or load_lpips)")):
        with pytest.raises(RuntimeError) as e:
            call()
        assert str(e.value) == text


def test_fixture_slices_stay_order_one():
    for case in CASES:
        f = _fix(case)
        assert (f["rms"] > 0.02).all() and (f["rms"] < 8).all(), (case, f["rms"])


@pytest.mark.parametrize("case", CASES)
def test_val_bar_holds_the_reference_fp32_run(case):
    from tests.golden.make_golden_lpips import WEIGHT_SEED
    from tests.test_gpu_lpips import lin_wmax, res_bars, val_bar
    f = _fix(case)
    wmax = lin_wmax(synth.synth_lpips_state_dict(WEIGHT_SEED))
    err = np.abs(f["val32"].astype(np.float64) - f["val64"])
    assert (err <= val_bar(f["res64"], f["val64"], wmax)).all()
    assert (np.abs(f["res32"].astype(np.float64) - f["res64"]) <= res_bars(f["res64"], wmax)).all()
    np.testing.assert_allclose(f["val64"], f["res64"].sum(1), rtol=1e-12, atol=0)
    if str(f["mode"]) == "same":
        assert (f["val64"] == 0).all() and (f["val32"] == 0).all()
    else:
        assert (err > 0).any() or (f["val32"] != 0).all()


def test_custom_op_schemas_and_fake_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    ops = torch.ops.omnitok
    assert "Tensor(a7!) out" in str(ops.lpips_preprocess.default._schema)
    assert "Tensor(a3!) res" in str(ops.lpips_layer.default._schema)
    assert str(ops.lpips_finalize.default._schema).endswith("-> Tensor")
    with FakeTensorMode():
        res = torch.empty((6, 5), dtype=torch.float64, device="cuda")
        val = ops.lpips_finalize(res)
        assert val.shape == (6,) and val.dtype == torch.float32
        feats = torch.empty((12, 8, 8, 512), device="cuda")
        assert ops.lpips_layer(feats, torch.empty(512, device="cuda"), 3, res) is None
        src = torch.empty((2, 3, 3, 16, 16), dtype=torch.uint8, device="cuda")
        out = torch.empty((6, 16, 16, 4), device="cuda")
        assert ops.lpips_preprocess(src, -0.5, False, True, [0.0] * 3, [1.0] * 3, 0, out) is None


def test_model_and_input_checks():
    m = lpips.LPIPS()
    with pytest.raises(RuntimeError, match="load_state_dict"):
        m.packed("cpu")
    m = lpips.load_lpips("cpu", synth.synth_lpips_state_dict(1))
    x = torch.zeros((2, 3, 32, 32))
    with pytest.raises(RuntimeError, match="GPU"):
        m(x, x)
    with pytest.raises(RuntimeError, match="GPU"):
        lpips.lpips_frames(x, x, m, layout="nchw")
    with pytest.raises(ValueError, match="layout"):
        lpips.lpips_frames(x, x, m, layout="nhwc")
    with pytest.raises(TypeError):
        lpips.lpips_frames(x, x, object(), layout="nchw")
    with pytest.raises(ValueError, match="source"):
        lpips.load_lpips("cpu", None)
