"""CPU: the fp64 restatement and the derived bar of tests/lm_prefill_attn_ref.py, on the inputs the GPU test uses.  A plain fp32 torch
restatement (another order of every sum, torch's own expf) has to stay inside both bars: the bar is a property of fp32 arithmetic under
the contract, not of one kernel."""
import pytest
import torch

from tests import error_bounds as eb
from tests import lm_prefill_attn_ref as ar


@pytest.mark.parametrize("hd", ar.HDS)
@pytest.mark.parametrize("name", list(ar.CASES))
def test_fp32_restatement_is_inside_the_bar(name, hd):
    c = ar.case(name, hd)
    out32 = ar.attention(c["qkv"], c["B"], c["T"], ar.HEADS, torch.float32)
    err = (out32.double() - c["out64"]).abs()
    r_t, r_r = eb.ratio(err, c["bar"]), eb.ratio(err, c["bar_rows"])
    print(f"{name} hd {hd}: fp32 torch restatement, worst err / bar: tiled bar {r_t:.3f}, rows bar {r_r:.3f}; max err {float(err.max()):.2e}, "
          f"bar {float(c['bar'].min()):.2e} .. {float(c['bar'].max()):.2e}, max |out| {float(c['out64'].abs().max()):.2f}")
    assert r_t <= 1.0 and r_r <= 1.0
    assert torch.isfinite(c["bar"]).all() and float(c["bar"].max()) < 1e-2     # a bar, not a blank cheque (outputs are O(1))


def test_restatement_row_zero_is_v_and_streams_are_separate():
    hd = 64
    c = ar.case("rnd_3x70", hd)
    B, T, C = c["B"], c["T"], ar.HEADS * hd
    v = c["qkv"].view(B, T, 3, C)[:, :, 2].double()
    assert torch.equal(c["out64"].view(B, T, C)[:, 0], v[:, 0])
    alone, _ = ar.reference(c["qkv"].view(B, T, 3 * C)[1].contiguous(), 1, T, ar.HEADS)
    assert torch.equal(alone, c["out64"].view(B, T, C)[1])
