"""DiT denoiser, the checks that need no GPU: the ABI of include/omnitok_dit.h, the engine's configuration rules, the fp64
restatement tests/dit_ref.py against the reference's recorded outputs, the sampler's tables against the reference's, state_dict
names, and every unsupported option."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import dit_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def lib():
    from omnitokenizer_amd import build, _lib
    build.build()
    return _lib.load()


def golden(name):
    return np.load(os.path.join(GOLDEN, name))


def test_dit_header_symbols_exported(lib):
    from omnitokenizer_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "omnitok_dit.h")).read()
    declared = set(re.findall(r"\b(omnitok_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 17 and all(n.startswith("omnitok_dit_") for n in declared), declared
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(raw, name), f"{name} declared in omnitok_dit.h but not exported"
    assert declared == set(_lib.DIT_EXPORTED_SYMBOLS), declared ^ set(_lib.DIT_EXPORTED_SYMBOLS)
    # the drop-in boundary of the other headers is unchanged
    assert not set(_lib.DIT_EXPORTED_SYMBOLS) & set(_lib.EXPORTED_SYMBOLS)


GOOD = dict(input_size=32, patch_size=2, in_channels=8, hidden=1152, depth=28, heads=16, mlp_hidden=4608, num_classes=1000,
            class_dropout=0.1, learn_sigma=1)


def _create(lib, **over):
    from omnitokenizer_amd._lib import OmnitokDitConfig
    cfg = OmnitokDitConfig(**{**GOOD, **over})
    h = ctypes.c_void_p()
    rc = lib.omnitok_dit_create(ctypes.byref(cfg), ctypes.byref(h))
    return rc, h


@pytest.mark.parametrize("over,word", [
    (dict(hidden=1024, heads=8), "head_dim"),            # 128
    (dict(hidden=96, heads=1, mlp_hidden=384), "head_dim"),
    (dict(hidden=1152, heads=10), "head_dim"),           # not a divisor
    (dict(mlp_hidden=4600), "multiples of 32"),
    (dict(patch_size=8, in_channels=9), "<= 512"),       # 576
    (dict(input_size=33), "multiple of patch_size"),
    (dict(depth=0), "positive"),
    (dict(class_dropout=-0.5), "class_dropout"),
])
def test_config_validation(lib, over, word):
    rc, h = _create(lib, **over)
    assert rc == -1 and not h.value
    assert word in lib.omnitok_last_error().decode()


def test_config_accepts_the_reference_models_and_counts_rows(lib):
    for hidden, heads, depth in ((1152, 16, 28), (1024, 16, 24), (768, 12, 12), (384, 6, 12)):   # XL (hd 72), L, B, S (hd 64)
        for p in (2, 4, 8):
            rc, h = _create(lib, hidden=hidden, heads=heads, depth=depth, mlp_hidden=4 * hidden, patch_size=p)
            assert rc == 0, lib.omnitok_last_error()
            assert lib.omnitok_dit_workspace_bytes(h, 2) > 0
            assert lib.omnitok_dit_workspace_bytes(h, 0) == -1
            lib.omnitok_dit_destroy(h)
    # argument errors come before any HIP call
    rc, h = _create(lib)
    assert lib.omnitok_dit_forward(h, None, None, None, 1, None, None) == -1 and b"null" in lib.omnitok_last_error()
    assert lib.omnitok_dit_finalize(h, None) == -3 and b"missing weight" in lib.omnitok_last_error()
    lib.omnitok_dit_destroy(h)
    assert lib.omnitok_dit_attn(ctypes.c_void_p(16), 1, 16, 2, 96, ctypes.c_void_p(16), None) == -1
    assert b"head_dim" in lib.omnitok_last_error()
    assert lib.omnitok_dit_patch_embed(ctypes.c_void_p(16), 1, ctypes.c_void_p(16), ctypes.c_void_p(16), ctypes.c_void_p(16), 1, 4, 9, 2,
                                       64, ctypes.c_void_p(16), None) == -1
    assert lib.omnitok_dit_unpatchify(ctypes.c_void_p(16), 1, 15, 2, 8, ctypes.c_void_p(16), None) == -1


@pytest.mark.parametrize("name", ["a", "b"])
def test_dit_ref_fp64_equals_the_reference(name):
    """The check on the restatement itself: tests/dit_ref.py in fp64 against the outputs the reference's own model.double() gave."""
    g = golden(f"dit_model_{name}.npz")
    cfg = dit_ref.MODELS[name]
    w = dit_ref.to_dtype(dit_ref.make_weights(cfg, dit_ref.SEEDS[name]), torch.float64)
    x, t, y = dit_ref.make_inputs(name)
    assert np.array_equal(x, g["x"]) and np.array_equal(t, g["t"]) and np.array_equal(y, g["y"])
    assert set(t.tolist()) == {0, 1, 500, 999} and cfg["num_classes"] in y.tolist()
    x, t, y = torch.from_numpy(x), torch.from_numpy(t), torch.from_numpy(y)
    for key, out in (("forward", dit_ref.forward(w, cfg, x, t, y)),
                     ("forward_with_cfg", dit_ref.forward_with_cfg(w, cfg, x, t, y, float(g["cfg_scale"])))):
        ref = torch.from_numpy(g[key])
        rel = float((out - ref).abs().max() / ref.abs().max())
        print(name, key, "relative", rel)
        assert out.shape == ref.shape and rel <= 1e-9
    assert float(np.abs(g["forward"]).max()) > 0.5  # every block contributes: not the zero output of the reference's own init


def test_dit_ref_p_sample_fp64_equals_the_reference_loop():
    from omnitokenizer_amd.diffusion import create_diffusion
    g = golden("dit_loop.npz")
    d = create_diffusion(str(g["respacing"]))
    coef = d.coefficient_table()
    for tag, clip in (("clip", True), ("noclip", False)):
        x = torch.from_numpy(g["x0"])
        for k, i in enumerate(range(d.num_timesteps - 1, -1, -1)):
            tt = torch.full((x.shape[0],), d.timestep_map[i], dtype=torch.int64)
            x, _ = dit_ref.p_sample(coef[i], dit_ref.toy_model(x, tt), x, torch.from_numpy(g["step_noise"][k]), True, clip)
            ref = torch.from_numpy(g[f"trajectory_{tag}"][k])
            assert float((x - ref).abs().max() / ref.abs().max()) <= 1e-9, (tag, k)


@pytest.mark.parametrize("key,resp", [("250", "250"), ("50", "50"), ("s10_15_20", "10,15,20")])
def test_tables_equal_the_reference_bit_for_bit(key, resp):
    from omnitokenizer_amd.diffusion import create_diffusion, SpacedDiffusion
    g = golden("dit_tables.npz")
    d = create_diffusion(resp)
    assert d.timestep_map == g[f"{key}/timestep_map"].tolist() and d.num_timesteps == len(d.timestep_map)
    for n in ("betas", "alphas_cumprod", "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_variance",
              "posterior_log_variance_clipped", "posterior_mean_coef1", "posterior_mean_coef2"):
        ours, ref = getattr(d, n).astype(np.float32), g[f"{key}/{n}"].astype(np.float32)
        assert ours.tobytes() == ref.tobytes(), n
    tab = d.coefficient_table()
    names = SpacedDiffusion.COEF_NAMES
    assert tab.dtype == np.float32 and tab.shape == (d.num_timesteps, 8)
    for col, n in ((0, "sqrt_recip_alphas_cumprod"), (1, "sqrt_recipm1_alphas_cumprod"), (2, "posterior_mean_coef1"),
                   (3, "posterior_mean_coef2"), (4, "posterior_log_variance_clipped")):
        assert names[col] == n and tab[:, col].tobytes() == g[f"{key}/{n}"].astype(np.float32).tobytes()
    assert tab[:, 5].tobytes() == np.log(g[f"{key}/betas"]).astype(np.float32).tobytes()
    fixed = np.log(np.append(g[f"{key}/posterior_variance"][1], g[f"{key}/betas"][1:])).astype(np.float32)
    assert tab[:, 6].tobytes() == fixed.tobytes()
    assert tab[0, 7] == 0.0 and (tab[1:, 7] == 1.0).all()


def test_pos_embed_and_timestep_table(lib):
    from omnitokenizer_amd.dit import get_2d_sincos_pos_embed, timestep_frequencies
    assert np.array_equal(get_2d_sincos_pos_embed(128, 6), golden("dit_tables.npz")["pos_embed_128_6"])
    # the engine's table from this torch's frequencies: cos / sin of the reference's fp32 args in fp64, rounded once -- which is
    # within one fp32 ulp of 1 of the reference's own fp32 cos / sin (dit_ref's embedding)
    fr = timestep_frequencies().contiguous()
    tab = np.zeros((1000, 256), np.float32)
    assert lib.omnitok_dit_timestep_table(ctypes.c_void_p(fr.data_ptr()), tab.ctypes.data_as(ctypes.c_void_p)) == 0
    args = (torch.arange(1000)[:, None].float() * fr[None]).double()
    assert np.array_equal(tab, torch.cat([torch.cos(args), torch.sin(args)], dim=-1).float().numpy())
    ref = dit_ref.timestep_embedding(torch.arange(1000), torch.float32).numpy()
    assert np.abs(tab - ref).max() <= 2.0 ** -23
    # the built-in frequencies are the correctly rounded ones: at most one ulp from any fp32 exp
    own = np.zeros((1000, 256), np.float32)
    assert lib.omnitok_dit_timestep_table(None, own.ctypes.data_as(ctypes.c_void_p)) == 0
    assert np.array_equal(own[1], np.concatenate([np.cos(_own_freqs()), np.sin(_own_freqs())]).astype(np.float32))
    assert np.abs(own - tab).max() <= 1e-4


def _own_freqs():
    arg = (np.float32(-np.log(10000.0)) * np.arange(128, dtype=np.float32)) / np.float32(128)
    return np.exp(arg.astype(np.float64)).astype(np.float32).astype(np.float64)


def test_state_dict_names_round_trip():
    from omnitokenizer_amd.dit import DiT, DiT_models
    assert sorted(DiT_models) == sorted(f"DiT-{n}/{p}" for n in ("XL", "L", "B", "S") for p in (2, 4, 8))
    for name, cfg in dit_ref.MODELS.items():
        m = DiT(**cfg)
        w = dit_ref.make_weights(cfg, dit_ref.SEEDS[name])
        sd = m.state_dict()
        assert list(sd) and set(sd) == set(w) and all(tuple(sd[k].shape) == tuple(w[k].shape) for k in w)
        out = m.load_state_dict(w, strict=True)
        assert not out.missing_keys and not out.unexpected_keys
        assert all(torch.equal(m.state_dict()[k], w[k]) for k in w)
        assert sorted(m.engine_missing()) == sorted(w)  # the engine waits for exactly these names
    xl = DiT_models["DiT-XL/2"](input_size=32, in_channels=8)
    assert xl.pos_embed.shape == (1, 256, 1152) and xl.y_embedder.embedding_table.weight.shape == (1001, 1152)
    assert xl.final_layer.linear.weight.shape == (64, 1152) and len(xl.blocks) == 28 and not xl.training


def test_load_dit_takes_ema(tmp_path):
    from omnitokenizer_amd.dit import load_dit
    a, b = {"w": torch.ones(2)}, {"w": torch.zeros(2)}
    torch.save({"model": a, "ema": b, "opt": {}}, tmp_path / "train.pt")
    torch.save(a, tmp_path / "plain.pt")
    assert torch.equal(load_dit(str(tmp_path / "train.pt"))["w"], b["w"])
    assert torch.equal(load_dit(str(tmp_path / "plain.pt"))["w"], a["w"])


def test_unsupported_options_raise():
    from omnitokenizer_amd.dit import DiT
    from omnitokenizer_amd.diffusion import create_diffusion, space_timesteps
    m = DiT(**dit_ref.MODELS["a"])
    with pytest.raises(NotImplementedError, match="inference-only"):
        m.train()
    with pytest.raises(NotImplementedError, match="inference-only"):
        m.train(True)
    assert m.eval() is m
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 8, 12, 12), torch.zeros(1, dtype=torch.long), torch.zeros(1, dtype=torch.long))
    with pytest.raises(NotImplementedError, match="fractional"):
        m(torch.zeros(1, 8, 12, 12), torch.full((1,), 0.5), torch.zeros(1, dtype=torch.long))
    with pytest.raises(ValueError, match="head_dim"):
        DiT(hidden_size=256, num_heads=2)
    for resp in ("ddim50", "ddim25"):
        with pytest.raises(NotImplementedError, match="respace.py"):
            create_diffusion(resp)
        with pytest.raises(NotImplementedError):
            space_timesteps(1000, resp)
    with pytest.raises(NotImplementedError, match="gaussian_diffusion.py"):
        create_diffusion("250", predict_xstart=True)
    with pytest.raises(NotImplementedError, match="gaussian_diffusion.py"):
        create_diffusion("250", noise_schedule="squaredcos_cap_v2")
    with pytest.raises(ValueError):
        create_diffusion("1001")
    d = create_diffusion("10")
    x = torch.zeros(1, 4, 2, 2)
    for kw in (dict(cond_fn=lambda *a, **k: 0), dict(denoised_fn=lambda v: v)):
        with pytest.raises(NotImplementedError, match="gaussian_diffusion.py"):
            d.p_sample(dit_ref.toy_model, x, torch.zeros(1, dtype=torch.long), **kw)
        with pytest.raises(NotImplementedError, match="gaussian_diffusion.py"):
            d.p_sample_loop(dit_ref.toy_model, x.shape, device="cpu", **kw)
    for fn in (d.ddim_sample, d.ddim_sample_loop, d.ddim_reverse_sample, d.ddim_sample_loop_progressive, d.training_losses,
               d.calc_bpd_loop):
        with pytest.raises(NotImplementedError, match="gaussian_diffusion.py"):
            fn(None, None)
    # the defaults of the reference's signature
    assert create_diffusion("").num_timesteps == 1000 and create_diffusion(None).timestep_map == list(range(1000))
    assert create_diffusion("250", learn_sigma=False).learn_sigma is False
