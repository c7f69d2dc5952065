"""Latte video denoiser, the checks that need no GPU: the ABI of include/omnitok_latte.h, the engine's configuration rules, its key
list against the reference's, the fp64 restatement tests/latte_ref.py against the reference's recorded outputs, the temporal sin-cos
table, state_dict names, and every unsupported option."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import dit_ref, latte_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def lib():
    from omnitokenizer_amd import build, _lib
    build.build()
    return _lib.load()


def golden(name):
    return np.load(os.path.join(GOLDEN, name))


def test_latte_header_symbols_exported(lib):
    from omnitokenizer_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "omnitok_latte.h")).read()
    declared = set(re.findall(r"\b(omnitok_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) == 13 and all(n.startswith("omnitok_latte_") for n in declared), declared
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(raw, name), f"{name} declared in omnitok_latte.h but not exported"
    assert declared == set(_lib.LATTE_EXPORTED_SYMBOLS), declared ^ set(_lib.LATTE_EXPORTED_SYMBOLS)
    # the boundaries of the other headers are unchanged
    assert not set(_lib.LATTE_EXPORTED_SYMBOLS) & (set(_lib.EXPORTED_SYMBOLS) | set(_lib.DIT_EXPORTED_SYMBOLS))
    from omnitokenizer_amd import build
    assert {"latte_attn.hip", "latte_ops.hip", "latte_engine.hip"} <= set(build.SOURCES)


GOOD = dict(input_size=32, patch_size=2, in_channels=8, hidden=1152, depth=28, heads=16, mlp_hidden=4608, num_classes=101,
            class_dropout=0.1, learn_sigma=1, num_frames=5, extras=2)


def _create(lib, **over):
    from omnitokenizer_amd._lib import OmnitokLatteConfig
    cfg = OmnitokLatteConfig(**{**GOOD, **over})
    h = ctypes.c_void_p()
    rc = lib.omnitok_latte_create(ctypes.byref(cfg), ctypes.byref(h))
    return rc, h


@pytest.mark.parametrize("over,word", [
    (dict(depth=27), "even"),
    (dict(depth=1), "even"),
    (dict(num_frames=0), "num_frames"),
    (dict(num_frames=33), "num_frames"),
    (dict(extras=78), "not built"),
    (dict(extras=0), "extras"),
    (dict(hidden=1024, heads=8), "head_dim"),            # 128
    (dict(hidden=96, heads=1, mlp_hidden=384), "head_dim"),
    (dict(hidden=1280, heads=16, mlp_hidden=5120), "head_dim"),   # 80
    (dict(input_size=33), "multiple of patch_size"),
    (dict(depth=0), "positive"),
])
def test_config_validation(lib, over, word):
    rc, h = _create(lib, **over)
    assert rc == -1 and not h.value
    assert word in lib.omnitok_last_error().decode()


def test_config_accepts_the_reference_models_and_argument_errors_need_no_gpu(lib):
    for hidden, heads, depth in ((1152, 16, 28), (1024, 16, 24), (768, 12, 12), (384, 6, 12)):   # XL (hd 72), L, B, S (hd 64)
        for frames, extras in ((5, 2), (16, 1), (1, 1), (32, 2)):
            rc, h = _create(lib, hidden=hidden, heads=heads, depth=depth, mlp_hidden=4 * hidden, num_frames=frames, extras=extras)
            assert rc == 0, lib.omnitok_last_error()
            sizes = [lib.omnitok_latte_workspace_bytes(h, b) for b in (1, 2, 3, 8)]
            assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:])), sizes   # monotone in B
            assert lib.omnitok_latte_workspace_bytes(h, 0) == -1
            lib.omnitok_latte_destroy(h)
    rc, h = _create(lib)
    assert lib.omnitok_latte_forward(h, None, None, None, 1, None, None) == -1 and b"null" in lib.omnitok_last_error()
    assert lib.omnitok_latte_finalize(h, None) == -3 and b"missing weight pos_embed" in lib.omnitok_last_error()
    lib.omnitok_latte_destroy(h)
    p16 = ctypes.c_void_p(16)
    assert lib.omnitok_latte_attn_temporal(p16, 1, 33, 4, 2, 64, p16, None) == -1 and b"frames" in lib.omnitok_last_error()
    assert lib.omnitok_latte_attn_temporal(p16, 1, 0, 4, 2, 64, p16, None) == -1 and b"frames" in lib.omnitok_last_error()
    assert lib.omnitok_latte_attn_temporal(p16, 1, 5, 4, 2, 80, p16, None) == -1 and b"head_dim" in lib.omnitok_last_error()
    assert lib.omnitok_latte_attn_temporal(ctypes.c_void_p(8), 1, 5, 4, 2, 64, p16, None) == -1 and b"unaligned" in lib.omnitok_last_error()
    assert lib.omnitok_latte_add_temp_embed(p16, p16, 1, 5, 4, 6, None) == -1
    assert lib.omnitok_latte_cfg_blend(p16, 3, 8, 4, 16, 2.0, None) == -1 and b"even" in lib.omnitok_last_error()


@pytest.mark.parametrize("name", ["a", "b"])
def test_missing_list_after_create_is_the_reference_key_list(lib, name):
    from omnitokenizer_amd.latte import Latte
    g = golden(f"latte_model_{name}.npz")
    cfg = latte_ref.MODELS[name]
    keys = [str(k) for k in g["keys"]]
    assert ("y_embedder.embedding_table.weight" in keys) == (cfg["extras"] == 2) and "temp_embed" in keys
    m = Latte(**cfg)
    assert sorted(m.engine_missing()) == sorted(keys)
    assert list(latte_ref.weight_shapes(cfg)) == m.engine_missing()
    assert set(m.state_dict()) == set(keys)


@pytest.mark.parametrize("name", ["a", "b"])
def test_latte_ref_fp64_equals_the_reference(name):
    """The check on the restatement itself: tests/latte_ref.py in fp64 against the outputs the reference's own model.double() gave."""
    g = golden(f"latte_model_{name}.npz")
    cfg = latte_ref.MODELS[name]
    w = latte_ref.to_dtype(latte_ref.make_weights(cfg, latte_ref.SEEDS[name]), torch.float64)
    x, t, y = latte_ref.make_inputs(name)
    assert np.array_equal(x, g["x"]) and np.array_equal(t, g["t"]) and np.array_equal(y, g["y"])
    assert x.shape == (4, cfg["num_frames"], cfg["in_channels"], cfg["input_size"], cfg["input_size"])
    assert set(t.tolist()) == {0, 1, 500, 999} and cfg["num_classes"] in y.tolist()
    x, t, y = torch.from_numpy(x), torch.from_numpy(t), torch.from_numpy(y)
    for key, out in (("forward", latte_ref.forward(w, cfg, x, t, y)),
                     ("forward_with_cfg", latte_ref.forward_with_cfg(w, cfg, x, t, y, float(g["cfg_scale"])))):
        ref = torch.from_numpy(g[key])
        rel = float((out - ref).abs().max() / ref.abs().max())
        print(name, key, "relative", rel)
        assert out.shape == ref.shape and rel <= 1e-12
    assert float(np.abs(g["forward"]).max()) > 0.5  # every block contributes: not the zero output of the reference's own init


def test_temp_embed_add_happens_in_the_first_pair_only():
    """Model (a) has two pairs: moving the add into the second pair, or into both, is a different function."""
    cfg = latte_ref.MODELS["a"]
    w = latte_ref.to_dtype(latte_ref.make_weights(cfg, latte_ref.SEEDS["a"]), torch.float64)
    x, t, y = (torch.from_numpy(v) for v in latte_ref.make_inputs("a"))
    base = latte_ref.forward(w, cfg, x, t, y)
    w2 = dict(w)
    w2["temp_embed"] = torch.zeros_like(w["temp_embed"])
    assert float((latte_ref.forward(w2, cfg, x, t, y) - base).abs().max()) > 1e-4


def test_latte_ref_p_sample_fp64_equals_the_reference_loop():
    from omnitokenizer_amd.diffusion import create_diffusion
    g = golden("latte_loop.npz")
    d = create_diffusion(str(g["respacing"]))
    coef = d.coefficient_table()
    assert g["x0"].shape == latte_ref.LOOP_SHAPE
    for tag, clip in (("clip", True), ("noclip", False)):
        x = torch.from_numpy(g["x0"])
        for k, i in enumerate(range(d.num_timesteps - 1, -1, -1)):
            tt = torch.full((x.shape[0],), d.timestep_map[i], dtype=torch.int64)
            x, _ = latte_ref.p_sample(coef[i], latte_ref.toy_model(x, tt), x, torch.from_numpy(g["step_noise"][k]), True, clip)
            ref = torch.from_numpy(g[f"trajectory_{tag}"][k])
            assert float((x - ref).abs().max() / ref.abs().max()) <= 1e-9, (tag, k)


@pytest.mark.parametrize("name", ["a", "b"])
def test_temp_embed_is_bit_equal_to_the_recorded_one(name):
    from omnitokenizer_amd.latte import Latte, get_1d_sincos_temp_embed
    g = golden(f"latte_model_{name}.npz")
    cfg = latte_ref.MODELS[name]
    ours = get_1d_sincos_temp_embed(cfg["hidden_size"], cfg["num_frames"])
    assert ours.dtype == np.float64 and ours.shape == (cfg["num_frames"], cfg["hidden_size"])
    assert np.array_equal(ours.astype(np.float32)[None], g["temp_embed"])
    m = Latte(**cfg)
    assert m.temp_embed.dtype == torch.float32 and np.array_equal(m.temp_embed.numpy(), g["temp_embed"])


def test_state_dict_names_round_trip():
    from omnitokenizer_amd.latte import Latte, Latte_models
    names = [f"Latte-{n}/{p}" for n in ("XL", "L", "B", "S") for p in (2, 4, 8)] + ["Latte-XL/2-omnitokenizer"]
    assert sorted(Latte_models) == sorted(names) and len(names) == 13
    for name, cfg in latte_ref.MODELS.items():
        m = Latte(**cfg)
        w = latte_ref.make_weights(cfg, latte_ref.SEEDS[name])
        sd = m.state_dict()
        assert list(sd) and set(sd) == set(w) and all(tuple(sd[k].shape) == tuple(w[k].shape) for k in w)
        out = m.load_state_dict(w, strict=True)
        assert not out.missing_keys and not out.unexpected_keys
        assert all(torch.equal(m.state_dict()[k], w[k]) for k in w)
    xl = Latte_models["Latte-XL/2-omnitokenizer"](input_size=32, num_frames=5, num_classes=101, extras=2)
    assert xl.in_channels == 8 and xl.pos_embed.shape == (1, 256, 1152) and xl.temp_embed.shape == (1, 5, 1152)
    assert xl.y_embedder.embedding_table.weight.shape == (102, 1152) and xl.final_layer.linear.weight.shape == (64, 1152)
    assert len(xl.blocks) == 28 and not xl.training and xl.extras == 2 and xl.num_frames == 5
    plain = Latte_models["Latte-S/2"]()   # the reference's defaults: 16 frames, 4 channels, no labels
    assert plain.num_frames == 16 and plain.in_channels == 4 and plain.extras == 1 and not hasattr(plain, "y_embedder")
    import omnitokenizer_amd
    assert omnitokenizer_amd.Latte is Latte and omnitokenizer_amd.Latte_models is Latte_models
    assert callable(omnitokenizer_amd.generate_videos) and callable(omnitokenizer_amd.load_latte)
    assert callable(omnitokenizer_amd.get_1d_sincos_temp_embed)


def test_load_latte_takes_ema(tmp_path):
    from omnitokenizer_amd.latte import load_latte
    a, b = {"w": torch.ones(2)}, {"w": torch.zeros(2)}
    torch.save({"model": a, "ema": b, "opt": {}}, tmp_path / "train.pt")
    torch.save({"state_dict": a, "epoch": 3}, tmp_path / "lightning.pt")
    torch.save(a, tmp_path / "plain.pt")
    assert torch.equal(load_latte(str(tmp_path / "train.pt"))["w"], b["w"])
    assert torch.equal(load_latte(str(tmp_path / "lightning.pt"))["w"], a["w"])
    assert torch.equal(load_latte(str(tmp_path / "plain.pt"))["w"], a["w"])


def test_unsupported_options_raise():
    from omnitokenizer_amd.latte import Latte
    m = Latte(**latte_ref.MODELS["a"])
    x, t, y = torch.zeros(1, 5, 8, 8, 8), torch.zeros(1, dtype=torch.long), torch.zeros(1, dtype=torch.long)
    with pytest.raises(NotImplementedError, match="inference-only"):
        m.train()
    assert m.eval() is m
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(x, t, y)
    with pytest.raises(NotImplementedError, match=r"use_fp16.*latte\.py"):
        m(x, t, y, use_fp16=True)
    with pytest.raises(NotImplementedError, match=r"use_fp16.*latte\.py"):
        m.forward_with_cfg(x, t, y, cfg_scale=2.0, use_fp16=True)
    with pytest.raises(NotImplementedError, match=r"text_embedding.*latte\.py"):
        m(x, t, y, text_embedding=torch.zeros(1, 77, 768))
    with pytest.raises(NotImplementedError, match="fractional"):
        m(x, torch.full((1,), 0.5), y)
    with pytest.raises(ValueError, match="x must be"):
        m(x[:, 0], t, y)                      # a 4-D image batch is the DiT's input, not Latte's
    with pytest.raises(ValueError, match="y must be"):
        m(x, t, None)                         # extras == 2 needs labels
    with pytest.raises(ValueError, match="not built"):
        Latte(**{**latte_ref.MODELS["a"], "extras": 78})
    with pytest.raises(ValueError, match="even"):
        Latte(**{**latte_ref.MODELS["a"], "depth": 3})
    with pytest.raises(ValueError, match="head_dim"):
        Latte(hidden_size=256, num_heads=2)
    for mode in ("math", "flash", "xformers"):     # accepted: there is one attention
        assert Latte(**{**latte_ref.MODELS["b"], "attention_mode": mode}).attention_mode == mode
    # the DiT class is what it was
    from omnitokenizer_amd.dit import DiT
    d = DiT(**dit_ref.MODELS["a"])
    assert sorted(d.engine_missing()) == sorted(dit_ref.weight_shapes(dit_ref.MODELS["a"]))
