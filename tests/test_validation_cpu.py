"""CPU: the validation-loss fixtures are sane, the new entry points validate their arguments before any device work, and the
header, the ctypes table and the built library agree on the new symbols."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests.validation_cases import VAL_CASES, ValCase

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("omnitok_losses_workspace", "omnitok_recon_losses", "omnitok_commitment_sum", "omnitok_kl_sum")
# An fp32 mean of n terms by pairwise / blocked summation carries about log2(n) roundings of 2^-24 each; the scalars below
# also inherit the fp32 run's pixel and latent noise, itself a few roundings per element.  MEAN_C = 4 such budgets.
MEAN_C = 4.0


def mean_bar(n):
    return MEAN_C * math.log2(max(n, 2)) * 2.0 ** -24


@pytest.mark.parametrize("name", VAL_CASES)
def test_reference_fp32_scalars_within_fp32_mean_bound_of_fp64(name):
    c = ValCase(name)
    n_pix = c.x_recon32.numel()
    pairs = [("recon_loss", n_pix)]
    if c.is_vae:
        pairs.append(("kl", c.g["moments32"].size // 2))
    else:
        pairs.append(("perplexity", c.g["ids"].size))
        if not c.is_ext:
            pairs.append(("commitment", c.g["z32"].size))
    for key, n in pairs:
        v32, v64 = c.scalar(key + "32"), c.scalar(key + "64")
        rel = abs(v32 - v64) / abs(v64)
        print(f"{name} {key}: fp32 {v32!r} fp64 {v64!r} rel {rel:.2e} bar {mean_bar(n):.2e}")
        assert rel <= mean_bar(n), (key, v32, v64)
    # the stored raw means reproduce the fp64 run's recon_loss
    a = c.args
    want = c.scalar("l1_64") * a.l1_weight if c.l1_path else \
        c.scalar("mse_64") * a.l1_weight + c.scalar("laplace_64") * a.logitslaplace_weight
    assert abs(want - c.scalar("recon_loss64")) <= (1e-12 if c.fp64_run else mean_bar(n_pix)) * abs(want)
    # 0.25 * mse(z, E[ids]) recomputed from the stored fp64 latents
    if not c.is_vae and not c.is_ext:
        z = c.wide("z")
        E = c.sd["codebook.embeddings"].double()
        ids = torch.from_numpy(c.g["ids"].astype(np.int64))
        assert abs(0.25 * ((z - E[ids]) ** 2).mean().item() - c.scalar("commitment64")) <= 1e-12
    if c.is_vae:
        mom = c.wide("moments")
        mu, lv = torch.chunk(mom, 2, dim=1)
        lv = lv.clamp(-30.0, 20.0)
        kl = 0.5 * (mu ** 2 + lv.exp() - 1.0 - lv).sum().item() / mom.shape[0] * a.kl_weight
        assert abs(kl - c.scalar("kl64")) <= 1e-12 * abs(kl)
    assert c.g["perceptual64"].shape == c.g["perceptual32"].shape and c.g["perceptual64"].ndim == 4
    assert c.g["lpips_res64"].shape == (c.g["perceptual64"].shape[0], 5)


def test_loss_ops_validate_arguments_before_device_work():
    import omnitokenizer_amd as oa
    from omnitokenizer_amd import losses
    f = torch.zeros
    with pytest.raises(ValueError, match="differ in shape"):
        oa.reconstruction_losses(f(2, 3, 4), f(2, 3, 5))
    with pytest.raises(TypeError, match="float32"):
        oa.reconstruction_losses(f(2, 3, dtype=torch.float64), f(2, 3))
    with pytest.raises(TypeError, match="tensor"):
        oa.reconstruction_losses(f(2, 3), [1.0])
    with pytest.raises(RuntimeError, match="one GPU"):
        oa.reconstruction_losses(f(2, 3), f(2, 3, device="meta"))
    with pytest.raises(RuntimeError, match="no CPU path"):
        oa.reconstruction_losses(f(2, 3), f(2, 3))
    with pytest.raises(ValueError, match="flags"):
        losses.recon_sums(f(2, 3), f(2, 3), 8)
    E = f(16, 8)
    with pytest.raises(ValueError, match="channel-last"):
        losses.commitment_sum(f(2, 8, 4, 4), f(2, 4, 4, dtype=torch.int64), E)
    with pytest.raises(TypeError, match="int64"):
        losses.commitment_sum(f(2, 4, 4, 8), f(2, 4, 4, dtype=torch.int32), E)
    with pytest.raises(RuntimeError, match="one GPU"):
        losses.commitment_sum(f(2, 4, 4, 8), f(2, 4, 4, dtype=torch.int64, device="meta"), E)
    with pytest.raises(RuntimeError, match="no CPU path"):
        losses.commitment_sum(f(2, 4, 4, 8), f(2, 4, 4, dtype=torch.int64), E)
    with pytest.raises(ValueError, match="2c"):
        losses.kl_sums(f(2, 7, 4))
    with pytest.raises(TypeError, match="float32"):
        losses.kl_sums(f(2, 8, 4, dtype=torch.float16))
    with pytest.raises(RuntimeError, match="no CPU path"):
        losses.kl_sums(f(2, 8, 4))


def test_forward_validates_arguments_before_device_work():
    from omnitokenizer_amd import OmniTokenizer_VQGAN, make_args
    from omnitokenizer_amd.lpips import LPIPS
    m = OmniTokenizer_VQGAN(make_args(2, resolution=64)).eval()
    x = torch.zeros(1, 3, 64, 64)
    assert m.perceptual_model is None
    for idx in (0, 1):
        with pytest.raises(NotImplementedError, match="training"):
            m(x, optimizer_idx=idx)
    with pytest.raises(RuntimeError, match="load_lpips"):
        m(x)
    with pytest.raises(TypeError, match="LPIPS"):
        m.set_perceptual_model(torch.nn.Identity())
    assert m.set_perceptual_model(LPIPS()) is m
    # an attribute, not a submodule: state_dict() stays the encode/decode path's
    assert "perceptual_model" not in m._modules and not any(k.startswith("perceptual_model") for k in m.state_dict())
    with pytest.raises(TypeError, match="float32"):
        m(x.double())
    with pytest.raises(ValueError, match=r"\[B,C,H,W\]"):
        m(torch.zeros(3, 64, 64))
    with pytest.raises(RuntimeError, match="input on meta"):
        m(torch.zeros(1, 3, 64, 64, device="meta"))
    with pytest.raises(ValueError, match="frame_idx"):
        m(x, frame_idx=torch.zeros(1, dtype=torch.int64))
    for kw in (dict(frame_idx=torch.zeros(1, dtype=torch.int64)), dict(noise=torch.zeros(1, 8, 8, 8))):
        with pytest.raises(ValueError, match="forward\\(x\\) only"):
            m(x, log_image=True, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.validation_step({"video": x}, 0)
    rs = OmniTokenizer_VQGAN(make_args(2, resolution=64, resolution_scale=[0.5, 1.0])).eval()
    rs.perceptual_model = LPIPS()
    with pytest.raises(NotImplementedError, match="resolution_scale"):
        rs(x)


def test_header_binding_and_library_agree_on_the_loss_symbols():
    from omnitokenizer_amd import _lib, build
    build.build()
    hdr = open(os.path.join(ROOT, "include", "omnitok.h")).read()
    declared = set(re.findall(r"\b(omnitok_[a-z0-9_]+)\s*\(", hdr))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} not declared in include/omnitok.h"
        assert name in _lib.EXPORTED_SYMBOLS, f"{name} not bound in _lib.py"
        assert hasattr(raw, name), f"{name} not exported by the library"
    # argument counts of the ctypes table against the header's declarations
    for name in NEW_SYMBOLS:
        decl = re.search(rf"\b{name}\s*\(([^;]*?)\)\s*;", hdr, re.S).group(1)
        assert len(_lib._PROTOS[name]) == len([a for a in decl.split(",") if a.strip()]), name
    assert "losses.hip" in build.SOURCES
    assert build.isa_report()["losses.hip"]["packed_f32"] == 0
    lib = _lib.load()
    assert lib.omnitok_losses_workspace(0) == -1 and lib.omnitok_losses_workspace(70000) == -1
    assert lib.omnitok_losses_workspace(32) >= 32 * 3 * 8
    # host-side validation fires before any HIP call
    one = ctypes.c_void_p(256)
    assert lib.omnitok_recon_losses(None, one, 1, 16, 1, one, None, one, 1 << 20, None) == -1
    assert b"null" in lib.omnitok_last_error()
    assert lib.omnitok_recon_losses(one, one, 1, 16, 8, one, None, one, 1 << 20, None) == -1
    assert b"flags" in lib.omnitok_last_error()
    assert lib.omnitok_recon_losses(one, one, 1, 16, 1, one, None, one, 8, None) == -1
    assert b"workspace" in lib.omnitok_last_error()
    assert lib.omnitok_commitment_sum(one, one, one, 0, 8, 16, one, one, 1 << 20, None) == -1
    assert lib.omnitok_kl_sum(one, 0, 16, one, None, one, 1 << 20, None) == -1


def test_loss_ops_are_registered_with_fakes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from omnitokenizer_amd import losses  # noqa: F401
    with FakeTensorMode():
        x = torch.empty(4, 3, 5, 64, 64, device="cuda")
        sums, total = torch.ops.omnitok.recon_losses(x, x, 7)
        assert tuple(sums.shape) == (4, 3) and tuple(total.shape) == (3,) and sums.dtype == torch.float64
        z, ids = torch.empty(2, 2, 8, 8, 8, device="cuda"), torch.empty(2, 2, 8, 8, dtype=torch.int64, device="cuda")
        assert tuple(torch.ops.omnitok.commitment_sum(z, ids, torch.empty(8192, 8, device="cuda")).shape) == (1,)
        s, t = torch.ops.omnitok.kl_sum(torch.empty(3, 16, 2, 8, 8, device="cuda"))
        assert tuple(s.shape) == (3,) and tuple(t.shape) == (1,) and t.dtype == torch.float64
