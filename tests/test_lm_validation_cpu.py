"""CPU: the LM validation entry points exist with the declared signatures and validate their arguments before any device work;
the lm_validation_* fixtures agree with the oracle's logits; the reference's own fp32 cross-entropy sits inside the derived bar
(tests/lm_validation_bounds.py), so the bar is not tighter than the reference itself."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import gpt_oracle as go
from tests import lm_validation_bounds as lb
from tests.helpers import GOLDEN
from tests.test_oracle_gpt import GPT_CASES, load_gpt_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("omnitok_lm_token_ce_workspace", "omnitok_lm_token_ce", "omnitok_lm_prefill_loss",
               "omnitok_lm_loss_workspace_bytes")


@pytest.fixture(scope="module")
def lib():
    from omnitokenizer_amd import _lib, build
    build.build()
    return _lib.load()


def load_val(name):
    return np.load(os.path.join(GOLDEN, f"lm_validation_{name}.npz"))


def test_header_binding_and_library_agree_on_the_lm_loss_symbols(lib):
    from omnitokenizer_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "omnitok_lm.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib._PROTOS and hasattr(raw, name), name
    P, I64, I = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    assert _lib._PROTOS["omnitok_lm_token_ce"] == [P, I64, P, I64, I, P, P, P, P, I64, P]
    assert _lib._PROTOS["omnitok_lm_prefill_loss"] == [P, P, I, P, I, P, P, P, P, I, P, P, P, P]
    assert lib.omnitok_lm_token_ce_workspace.restype is I64 and lib.omnitok_lm_loss_workspace_bytes.restype is I64
    assert lib.omnitok_lm_token_ce_workspace(0) == -1 and lib.omnitok_lm_token_ce_workspace(2 ** 31 + 1) == -1
    need = lib.omnitok_lm_token_ce_workspace(1)
    assert need > 0 and lib.omnitok_lm_token_ce_workspace(2 ** 31) == need
    assert lib.omnitok_lm_loss_workspace_bytes(None) == 0


def test_c_entry_points_validate_arguments_without_gpu(lib):
    from omnitokenizer_amd import _lib
    buf = (ctypes.c_double * 8)()
    one = ctypes.cast(buf, ctypes.c_void_p)
    need = lib.omnitok_lm_token_ce_workspace(4)
    tc = lib.omnitok_lm_token_ce
    assert tc(None, 8, one, 4, 8, one, one, one, one, need, None) == -1 and b"null" in lib.omnitok_last_error()
    assert tc(one, 8, one, 4, 8, one, one, None, one, need, None) == -1          # no sums
    assert tc(one, 8, one, 4, 8, one, one, one, one, need - 1, None) == -1       # short workspace
    assert tc(one, 7, one, 4, 8, one, one, one, one, need, None) == -1           # ld < V
    assert tc(one, 8, one, 0, 8, one, one, one, one, need, None) == -1           # no rows
    assert tc(one, 8, one, 4, 0, one, one, one, one, need, None) == -1           # V < 1
    assert tc(one.value + 2, 8, one, 4, 8, one, one, one, one, need, None) == -1 and b"aligned" in lib.omnitok_last_error()
    assert lib.omnitok_lm_prefill_loss(None, None, 1, None, 0, None, one, one, one, 1, None, None, one, None) == -1
    # the option: default 2048, readable, at least one row
    assert _lib.get_option("lm_loss_chunk_rows") == 2048
    try:
        _lib.set_option("lm_loss_chunk_rows", 64)
        assert _lib.get_option("lm_loss_chunk_rows") == 64
        with pytest.raises(ValueError, match="at least 1"):
            _lib.set_option("lm_loss_chunk_rows", 0)
        assert _lib.get_option("lm_loss_chunk_rows") == 64
    finally:
        _lib.set_option("lm_loss_chunk_rows", 2048)


def test_python_entry_points_validate_arguments_before_device_work():
    import omnitokenizer_amd as oa
    from omnitokenizer_amd import lm_losses
    assert "token_cross_entropy" in oa.__all__ and oa.token_cross_entropy is lm_losses.token_cross_entropy
    lg, tg = torch.zeros(3, 7), torch.zeros(3, dtype=torch.int64)
    for fn in (lm_losses.token_cross_entropy, lm_losses.token_ce_sums):
        with pytest.raises(TypeError, match="float32"):
            fn(lg.double(), tg)
        with pytest.raises(TypeError, match="tensor"):
            fn([[0.0]], tg)
        with pytest.raises(TypeError, match="int64"):
            fn(lg, tg.int())
        with pytest.raises(ValueError, match=r"logits.shape\[:-1\]"):
            fn(lg, tg[:2])
        with pytest.raises(ValueError, match="V >= 1"):
            fn(torch.zeros(3, 0), tg)
        with pytest.raises(ValueError, match="V >= 1"):
            fn(torch.zeros(()), torch.zeros((), dtype=torch.int64))
        with pytest.raises(RuntimeError, match="one GPU"):
            fn(lg, tg.to("meta"))
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(lg, tg)


def test_token_ce_op_is_registered_with_a_fake():
    from omnitokenizer_amd import lm_losses  # noqa: F401
    assert "Tensor logits, Tensor targets" in str(torch.ops.omnitok.token_ce.default._schema)
    nll, rank, sums = torch.ops.omnitok.token_ce(torch.zeros(2, 5, 9, device="meta"),
                                                 torch.zeros(2, 5, dtype=torch.int64, device="meta"))
    assert (tuple(nll.shape), nll.dtype) == ((2, 5), torch.float32) and (tuple(rank.shape), rank.dtype) == ((2, 5), torch.int32)
    assert (tuple(sums.shape), sums.dtype) == ((4,), torch.float64)


def test_gpt_and_transformer_expose_the_validation_methods():
    import argparse
    from omnitokenizer_amd.gpt import GPT
    from omnitokenizer_amd.lm_transformer import Net2NetTransformer
    for name in ("shared_step", "validation_step", "_teacher_forced_sequence"):
        assert callable(getattr(Net2NetTransformer, name))
    assert not hasattr(Net2NetTransformer, "training_step")
    m = GPT(argparse.Namespace(), 300, 40, n_layer=1, n_head=4, n_embd=256)
    idx = torch.zeros(2, 8, dtype=torch.int64)
    with pytest.raises(TypeError, match="int64"):
        m.token_losses(idx, idx.int())
    with pytest.raises(ValueError, match=r"\[B, T\]"):
        m.token_losses(idx, idx[:, :7])
    big = GPT(argparse.Namespace(), 300, 70000, n_layer=1, n_head=4, n_embd=256)
    wide = torch.zeros(1, 65536, dtype=torch.int64)
    with pytest.raises(ValueError, match="65535"):
        big.token_losses(wide, wide)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.token_losses(idx, idx)
    assert m.loss_workspace_bytes() == 0


@pytest.mark.parametrize("name", GPT_CASES)
def test_fixture_is_consistent_with_the_oracle_logits(name):
    g, sd, (V, BS, L, H, C) = load_gpt_case(name)
    v = load_val(name)
    tg = torch.from_numpy(v["targets"])
    assert tuple(tg.shape) == tuple(g["idx"].shape) and int(tg.min()) >= 0 and int(tg.max()) < V
    with torch.no_grad():
        logits = go.forward(sd, torch.from_numpy(g["idx"]), H)
    flat, tflat = logits.reshape(-1, V), tg.reshape(-1)
    n = tflat.numel()
    # the oracle's logits are within 2e-5 of the reference's (tests/test_oracle_gpt.py): so is every nll (a 1-Lipschitz map
    # of the logits in the max norm, twice: the logsumexp and the target's entry)
    assert (lb.nll64(flat, tflat) - torch.from_numpy(v["nll64"]).reshape(-1)).abs().max().item() < 2 * 2e-5
    assert abs(F.cross_entropy(flat, tflat).item() - float(v["loss"])) < 2 * 2e-5
    # margins: recorded from the reference's logits; no row is near a tie, so the oracle's ranks decide the accuracies
    m1, m5 = torch.from_numpy(v["margin1"]).reshape(-1), torch.from_numpy(v["margin5"]).reshape(-1)
    near = (m1.abs() < 2 * lb.LOGIT_TOL) | (m5.abs() < 2 * lb.LOGIT_TOL)
    assert int(near.sum()) <= 0.02 * n
    rank = lb.rank_of_target(flat, tflat)
    assert torch.equal(rank == 0, m1 > 0) and torch.equal(rank < 5, m5 > 0)
    a1, a5 = lb.reference_accuracy((rank == 0).sum(), n), lb.reference_accuracy((rank < 5).sum(), n)
    assert a1.item() == float(v["acc1"][0]) and a5.item() == float(v["acc5"][0])
    assert 0 < a1.item() < a5.item() < 100     # some rows top-1, some in 2..5, some miss


@pytest.mark.parametrize("name", GPT_CASES)
def test_reference_fp32_cross_entropy_is_inside_the_derived_bar(name):
    g, sd, (V, BS, L, H, C) = load_gpt_case(name)
    v = load_val(name)
    logits = torch.from_numpy(g["logits"]).reshape(-1, V)          # the reference's own fp32 logits
    tg = torch.from_numpy(v["targets"]).reshape(-1)
    ref64 = torch.from_numpy(v["nll64"]).reshape(-1)
    assert torch.equal(lb.nll64(logits, tg), ref64) or (lb.nll64(logits, tg) - ref64).abs().max().item() < 1e-12
    bar = lb.nll_bar(logits, tg)
    nll32 = F.cross_entropy(logits, tg, reduction="none")
    r = float(((nll32.double() - ref64).abs() / bar).max())
    loss64 = float(ref64.mean())
    lbar = lb.loss_bar(bar, tg, loss64)
    print(f"{name}: reference fp32 nll at {r:.3f} of the bar; loss err {abs(float(v['loss']) - loss64):.2e} bar {lbar:.2e}")
    assert r <= 1.0
    assert abs(float(v["loss"]) - loss64) <= lbar


@pytest.mark.parametrize("V", [1, 5, 63, 257, 1025, 9217])
@pytest.mark.parametrize("scale", [1.0, 30.0])
def test_torch_fp32_cross_entropy_is_inside_the_bar_on_the_kernel_test_inputs(V, scale):
    """the inputs of tests/test_gpu_lm_validation.py::test_token_ce_vs_fp64: the bar holds for torch's own fp32 kernel too"""
    for N in (1, 3, 257, 1030):
        logits, tg = lb.ce_case(N, V, scale)
        bar = lb.nll_bar(logits, tg)
        err = (F.cross_entropy(logits, tg, reduction="none").double() - lb.nll64(logits, tg)).abs()
        assert float(torch.where(bar > 0, err / bar, err).max()) <= 1.0, N
