"""CPU: the fp64 restatement and the derived bar of tests/lm_prefill_attn16_ref.py, on the inputs the GPU test uses.  A plain fp32 torch
restatement of the contract (another order of every sum, torch's own expf) has to stay inside the bar, and restatements that break the
contract -- an operand left unrounded, the mask off by one key -- have to leave it: the bar is neither fitted to a kernel nor vacuous."""
import pytest
import torch

from tests import error_bounds as eb
from tests import lm_prefill_attn16_ref as r16
from tests import lm_prefill_attn_ref as ar

FMTS = ["bf16", "fp16"]


def ratio(c, out32):
    return eb.ratio((out32.double() - c["out64"]).abs(), c["bar"])


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("hd", ar.HDS)
@pytest.mark.parametrize("name", list(ar.CASES))
def test_fp32_restatement_is_inside_the_bar(name, hd, fmt):
    c = r16.case(name, hd, fmt)
    r = ratio(c, r16.emulate(c["qkv"], c["B"], c["T"], ar.HEADS, fmt, r16.KT))
    print(f"{name} hd {hd} {fmt}: fp32 torch restatement, worst err / bar {r:.3f}; bar {float(c['bar'].min()):.2e} .. "
          f"{float(c['bar'].max()):.2e}, max |out| {float(c['out64'].abs().max()):.2f}")
    assert r <= 1.0
    assert torch.isfinite(c["bar"]).all() and float(c["bar"].max()) < (0.5 if fmt == "bf16" else 0.1)   # outputs are O(1) .. O(10)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name,left_out", [("q8_3x70", "q"), ("q8_3x70", "k"), ("dom_last_2x300", "k")])
def test_an_unrounded_operand_leaves_the_bar(name, left_out, fmt):
    hd = 96
    c = r16.case(name, hd, fmt)
    kept = tuple(n for n in "qkv" if n != left_out)
    r = ratio(c, r16.emulate(c["qkv"], c["B"], c["T"], ar.HEADS, fmt, r16.KT, rounded=kept))
    print(f"{name} hd {hd} {fmt}: {left_out} left unrounded: worst err / bar {r:.2f}")
    assert r > 1.0


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("shift", [1, -1])
@pytest.mark.parametrize("name", [n for n in ar.CASES if not n.startswith("dom_first")])
def test_a_mask_off_by_one_key_leaves_the_bar(name, shift, fmt):
    """Every case but dom_first: there key 0 outweighs every other key by e^30, so one key more or fewer moves a row by 1e-13 of
    itself by construction -- no bar can see it, and the exact prefix-mean cases on the GPU are what pins the mask there."""
    hd = 96
    c = r16.case(name, hd, fmt)
    r = ratio(c, r16.emulate(c["qkv"], c["B"], c["T"], ar.HEADS, fmt, r16.KT, mask_shift=shift))
    print(f"{name} hd {hd} {fmt}: mask shifted by {shift:+d}: worst err / bar {r:.1f}")
    assert r > 100.0


def test_restatement_row_zero_is_rounded_v():
    hd, fmt = 64, "bf16"
    c = r16.case("rnd_3x70", hd, fmt)
    B, T, C = c["B"], c["T"], ar.HEADS * hd
    v = r16.round_qkv(c["qkv"], fmt).view(B, T, 3, C)[:, :, 2]
    assert torch.equal(c["out64"].view(B, T, C)[:, 0], v[:, 0].double())
    assert torch.equal(r16.emulate(c["qkv"], B, T, ar.HEADS, fmt, r16.KT).view(B, T, C)[:, 0], v[:, 0])
