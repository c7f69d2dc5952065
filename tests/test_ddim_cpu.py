"""The DDIM sampler, the checks that need no GPU: the "ddimN" striding and the respaced tables against the reference's
(tests/golden/ddim_loop.npz, written by tests/golden/make_golden_ddim.py), the fp32 coefficient chain against torch's, the ABI of
omnitok_dit_ddim_step with every argument error, tests/ddim_ref.py against the reference's recorded trajectories, and what stays
refused."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import ddim_ref, dit_ref, latte_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "ddim_loop.npz"))


@pytest.fixture(scope="module")
def lib():
    from omnitokenizer_amd import build, _lib
    build.build()
    return _lib.load()


def test_names_are_exported():
    import omnitokenizer_amd as pkg
    from omnitokenizer_amd import diffusion
    for name in ("create_ddim_diffusion", "DDIMDiffusion", "ddim_timesteps"):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(diffusion, name)
    assert issubclass(diffusion.DDIMDiffusion, diffusion.SpacedDiffusion)


def test_ddim_timesteps_equal_the_reference():
    from omnitokenizer_amd.diffusion import ddim_timesteps
    for count in (7, 10, 25, 50, 250):
        got = ddim_timesteps(1000, count)
        assert isinstance(got, set) and sorted(got) == G[f"ddim_timesteps/{count}"].tolist() and len(got) == count
    assert G["ddim_timesteps/no_stride"].tolist() == [300]
    with pytest.raises(ValueError, match="cannot create exactly 1000 steps with an integer stride"):
        ddim_timesteps(1000, 300)


@pytest.mark.parametrize("key,resp", [("ddim10", "ddim10"), ("ddim50", "ddim50"), ("s10_15_20", "10,15,20")])
def test_tables_equal_the_reference(key, resp):
    from omnitokenizer_amd.diffusion import DDIMDiffusion, create_ddim_diffusion
    d = create_ddim_diffusion(resp)
    assert type(d) is DDIMDiffusion
    assert d.timestep_map == G[f"{key}/timestep_map"].tolist() and d.num_timesteps == len(d.timestep_map)
    for n in ("alphas_cumprod", "alphas_cumprod_prev", "alphas_cumprod_next"):
        ours, ref = getattr(d, n), G[f"{key}/{n}"]
        assert ours.dtype == np.float64 and ours.astype(np.float32).tobytes() == ref.astype(np.float32).tobytes(), n
        assert np.abs(ours - ref).max() <= 1e-15, n
    assert d.alphas_cumprod_next[-1] == 0.0 and np.array_equal(d.alphas_cumprod_next[:-1], d.alphas_cumprod[1:])


def _torch_sqrt(v):
    return torch.sqrt(v)


def _ieee_sqrt(v):
    """The correctly rounded fp32 square root: the fp64 root rounded once more (53 >= 2 * 24 + 2 bits: the second rounding cannot
    change the result)."""
    return torch.sqrt(v.double()).float()


# "ddim10" with torch.sqrt is the chain as the reference's CPU run gives it.  torch's vectorised CPU sqrt is not correctly rounded
# (0.5001 ulp): over longer tables it leaves the IEEE result by an ulp in about one element of a hundred, which of them depending on
# the element's position in the vector.  The table is the IEEE chain, so the other respacings are held to it with the correctly
# rounded root -- every other operation of the chain (+ - * /) is correctly rounded in torch and in numpy alike.
@pytest.mark.parametrize("resp,sqrt", [("ddim10", _torch_sqrt), ("ddim10", _ieee_sqrt), ("ddim50", _ieee_sqrt), ("10,15,20", _ieee_sqrt)])
@pytest.mark.parametrize("eta", [0.0, 0.3, 0.5, 1.0])
def test_coefficient_table_is_the_reference_chain_in_fp32(eta, resp, sqrt):
    """gaussian_diffusion.py:543-558, 590-596 written with torch fp32 CPU tensors, as _extract_into_tensor's .float() makes the
    reference run it, in its expression order."""
    from omnitokenizer_amd.diffusion import create_ddim_diffusion
    d = create_ddim_diffusion(resp)
    tab = d.ddim_coefficient_table(eta)
    assert tab.dtype == np.float32 and tab.shape == (d.num_timesteps, 8) and len(d.DDIM_COEF_NAMES) == 8
    alpha_bar, alpha_bar_prev, alpha_bar_next = (torch.from_numpy(v).float() for v in
                                                 (d.alphas_cumprod, d.alphas_cumprod_prev, d.alphas_cumprod_next))
    sigma = (
        eta
        * sqrt((1 - alpha_bar_prev) / (1 - alpha_bar))
        * sqrt(1 - alpha_bar / alpha_bar_prev)
    )
    assert sigma.dtype == torch.float32
    nonzero_mask = (torch.arange(d.num_timesteps) != 0).float()
    want = [torch.from_numpy(d.sqrt_recip_alphas_cumprod).float(), torch.from_numpy(d.sqrt_recipm1_alphas_cumprod).float(),
            sqrt(alpha_bar_prev), sqrt(1 - alpha_bar_prev - sigma ** 2), nonzero_mask * sigma,
            sqrt(alpha_bar_next), sqrt(1 - alpha_bar_next), torch.zeros(d.num_timesteps)]
    got = torch.from_numpy(tab)
    for col, w in enumerate(want):
        assert w.dtype == torch.float32 and torch.equal(got[:, col], w), (col, d.DDIM_COEF_NAMES[col])
    assert tab[0, 4] == 0.0 and tab[0, 3] == 0.0 and tab[0, 2] == 1.0
    assert tab[-1, 5] == 0.0 and tab[-1, 6] == 1.0
    assert (tab[1:, 4] > 0).all() if eta > 0 else (tab[:, 4] == 0).all()
    assert np.isfinite(tab).all()


@pytest.mark.parametrize("eta", [-0.1, float("nan"), 2.0, float("inf")])
def test_refused_eta(eta):
    from omnitokenizer_amd.diffusion import create_ddim_diffusion
    d = create_ddim_diffusion("ddim10")
    with pytest.raises(ValueError):
        d.ddim_coefficient_table(eta)
    with pytest.raises(ValueError):   # ... and the loop refuses it before anything touches the model or a device
        d.ddim_sample_loop(None, (1, 4, 2, 2), device="cpu", eta=eta)


def test_ddim_ref_fp64_equals_the_reference_trajectories():
    """The check on the restatement itself: tests/ddim_ref.py in fp64 with this package's tables against the reference's loops."""
    from omnitokenizer_amd.diffusion import create_ddim_diffusion
    d = create_ddim_diffusion(str(G["respacing"]))
    n = d.num_timesteps
    cases = [(f"dit_eta{e:g}_{'clip' if c else 'noclip'}", "", dit_ref.toy_model, e, c, False) for e in (0.0, 0.5, 1.0) for c in (True, False)]
    cases += [(f"latte_eta{e:g}_noclip", "latte_", latte_ref.toy_model, e, False, False) for e in (0.0, 0.5)]
    cases += [("dit_reverse", "", dit_ref.toy_model, 0.0, False, True)]
    for key, pre, toy, eta, clip, reverse in cases:
        coef = d.ddim_coefficient_table(eta)
        x = torch.from_numpy(G[pre + "x0"])
        for k, i in enumerate(range(n) if reverse else range(n - 1, -1, -1)):
            tt = torch.full((x.shape[0],), d.timestep_map[i], dtype=torch.int64)
            draw = torch.from_numpy(G[pre + "step_noise"][k]) if eta > 0 else None
            x, _ = ddim_ref.ddim_step(coef[i], toy(x, tt), x, draw, True, clip, reverse)
            ref = torch.from_numpy(G[key][k])
            assert float((x - ref).abs().max() / ref.abs().max()) <= 1e-9, (key, k)
        cpu = float(G[f"cpu_fp32_err_{key}"])
        assert np.isfinite(cpu) and cpu > 0


# ---- the C entry ---------------------------------------------------------------------------------------------------------------------
def test_symbol_and_prototype(lib):
    from omnitokenizer_amd import _lib
    assert "omnitok_dit_ddim_step" in _lib.DIT_EXPORTED_SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "omnitok_dit.h")).read()
    m = re.search(r"\bint omnitok_dit_ddim_step\(([^;]*)\);", hdr)
    assert m, "omnitok_dit_ddim_step is not declared in omnitok_dit.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == ["model_out", "x", "noise", "coef", "n_steps", "t", "B", "C", "HW", "learned_range",
                                                            "clip", "reverse", "x_out", "pred_xstart", "stream"]
    P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64

    def ctype(p):
        return P if "*" in p or p.startswith("omnitok_stream_t") else (L if p.startswith("int64_t") else I)

    assert _lib._DIT_PROTOS["omnitok_dit_ddim_step"] == [ctype(p) for p in params]
    fn = lib.omnitok_dit_ddim_step
    assert fn.argtypes == _lib._DIT_PROTOS["omnitok_dit_ddim_step"] and fn.restype is ctypes.c_int
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "omnitok_dit_ddim_step")


def _host_ptr():
    buf = (ctypes.c_float * 64)()     # a host address: never dereferenced, the calls are refused first
    return buf, ctypes.c_void_p(ctypes.addressof(buf))


def test_argument_errors_come_before_any_hip_call(lib):
    buf, p = _host_ptr()
    fn, err = lib.omnitok_dit_ddim_step, lib.omnitok_last_error
    #       mo x  noise coef n_steps t  B  C  HW learned clip reverse x_out xs stream
    good = [p, p, p, p, 10, p, 2, 4, 25, 1, 1, 0, p, p, None]
    for idx, name in ((0, b"model_out"), (1, b"x"), (3, b"coef"), (5, b"t"), (12, b"x_out")):
        args = list(good)
        args[idx] = None
        assert fn(*args) == -1 and name + b" is null" in err(), name
    for idx, name in ((4, b"n_steps"), (6, b"B"), (7, b"C"), (8, b"HW")):
        for bad in (0, -1):
            args = list(good)
            args[idx] = bad
            assert fn(*args) == -1 and b"dit_ddim_step: " + name + b" " in err(), (name, bad)
    # more elements than the grid covers, and a product that would overflow int64: the kernel's one 32-bit grid dimension
    for B, C, HW in ((2 ** 31 - 1, 2 ** 31 - 1, 2 ** 40), (2 ** 20, 2 ** 10, 2 ** 20), (1, 1, 2 ** 39 - 256)):
        args = list(good)
        args[6], args[7], args[8] = B, C, HW
        assert fn(*args) == -1 and b"too many elements" in err(), (B, C, HW)
    del buf


# ---- what stays refused ----------------------------------------------------------------------------------------------------------------
def test_refusals_stay():
    from omnitokenizer_amd.diffusion import (SpacedDiffusion, create_ddim_diffusion, create_diffusion, generate_images, generate_videos,
                                             space_timesteps)
    with pytest.raises(NotImplementedError, match="respace.py"):
        create_diffusion("ddim50")
    with pytest.raises(NotImplementedError):
        space_timesteps(1000, "ddim50")
    plain = create_diffusion("10")
    assert type(plain) is SpacedDiffusion
    for fn in (plain.ddim_sample, plain.ddim_sample_loop, plain.ddim_reverse_sample, plain.ddim_sample_loop_progressive):
        with pytest.raises(NotImplementedError, match="gaussian_diffusion.py"):
            fn(None, None)
    with pytest.raises(NotImplementedError, match="gaussian_diffusion.py"):
        create_ddim_diffusion("ddim50", predict_xstart=True)
    with pytest.raises(NotImplementedError, match="gaussian_diffusion.py"):
        create_ddim_diffusion("ddim50", noise_schedule="squaredcos_cap_v2")
    with pytest.raises(ValueError, match="integer stride"):
        create_ddim_diffusion("ddim300")
    with pytest.raises(ValueError, match="at least two"):
        create_ddim_diffusion("1")
    with pytest.raises(ValueError):
        create_ddim_diffusion("1001")
    d = create_ddim_diffusion("ddim10")
    x, t = torch.zeros(1, 4, 2, 2), torch.zeros(1, dtype=torch.long)
    for kw in (dict(cond_fn=lambda *a, **k: 0), dict(denoised_fn=lambda v: v)):
        for step in (d.ddim_sample, d.ddim_reverse_sample, d.p_sample):
            with pytest.raises(NotImplementedError, match="gaussian_diffusion.py"):
                step(dit_ref.toy_model, x, t, **kw)
        for loop in (d.ddim_sample_loop, d.p_sample_loop):
            with pytest.raises(NotImplementedError, match="gaussian_diffusion.py"):
                loop(dit_ref.toy_model, x.shape, device="cpu", **kw)
        with pytest.raises(NotImplementedError, match="gaussian_diffusion.py"):
            next(d.ddim_sample_loop_progressive(dit_ref.toy_model, x.shape, device="cpu", **kw))
    for step in (d.ddim_sample, d.ddim_reverse_sample):   # a model on the CPU
        with pytest.raises(RuntimeError, match="GPU only"):
            step(dit_ref.toy_model, x, t)
    with pytest.raises(ValueError, match="deterministic"):
        d.ddim_reverse_sample(dit_ref.toy_model, x, t, eta=0.5)
    # the reference's defaults and the respacings it lets ddim_sample_loop run on
    assert create_ddim_diffusion("").num_timesteps == 1000 and create_ddim_diffusion(None).timestep_map == list(range(1000))
    assert create_ddim_diffusion("250").timestep_map == create_diffusion("250").timestep_map
    assert create_ddim_diffusion("ddim50", learn_sigma=False).learn_sigma is False
    assert create_ddim_diffusion("ddim25", diffusion_steps=100).timestep_map == list(range(0, 100, 4))
    # the sample_method switch of generate_images / generate_videos: checked before anything else is touched
    for gen in (generate_images, generate_videos):
        with pytest.raises(TypeError, match="create_ddim_diffusion"):
            gen(None, plain, None, None, sample_method="ddim")
        with pytest.raises(ValueError, match="sample_method"):
            gen(None, plain, None, None, sample_method="plms")
        with pytest.raises(ValueError, match="sample_method"):
            gen(None, d, None, None, sample_method="DDIM")
