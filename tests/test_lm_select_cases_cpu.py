"""CPU: the expectations of tests/lm_select_cases.py (what tests/test_gpu_lm_select.py holds the selection kernel to)
against the reference's own fp32 filter as the oracle restates it, their preconditions, and the probe counts."""
import numpy as np
import pytest
import torch

from oracle import gpt_oracle as go
from tests import lm_select_cases as sc

N_CASES = 131


def test_no_case_was_dropped():
    names = sc.case_names()
    assert len(names) == N_CASES and len(set(names)) == N_CASES
    for mech in ("bitonic_", "radix_pos_", "radix_neg_", "radix_mixed_", "tie", "zero_", "ninf_", "sortbuf_", "seam_",
                 "nucleus_", "unsorted_", "temp", "cfg_"):
        assert any(n.startswith(mech) for n in names), mech
    for k in (1, 2, 127, 128, 129, 255, 256, 257, 2047, 2048, 2049):
        assert f"bitonic_k{k}" in names
    for k in (None, 0, 300, 307, 200, 201):
        assert f"ninf_k{k}" in names


@pytest.mark.parametrize("name", sc.case_names())
def test_case_against_the_reference_filter(name):
    c = sc.get(name)
    s = c.solve()                                   # asserts the preconditions, n_keep and the probe count
    v = c.values()
    order, n_nuc, cdf, u, want = s["order"], s["n_nuc"], s["cdf"], s["u"], s["want"]
    assert u.dtype == np.float32 and want.dtype == np.int64 and u.size == want.size == c.n_probes
    assert u.size <= 2200 and float(u.min()) == 0.0 and float(u.max()) == np.float32(sc.U_LAST)
    if c.overflow:
        # nothing to draw from: the kernel must raise its flag and return the first maximum
        assert len(order) > sc.SORT_MAX and s["top_p"] < 1.0 and (want == int(v.argmax())).all()
        return
    # the reference's own fp32 filter keeps the same set, and the oracle ranks it the same way
    _, ref_order, ref_cdf = go.select_inverse_cdf(v, c.top_k, s["top_p"], 0.0)
    mine = order[:n_nuc]
    if c.index_order:
        # the oracle ranks by value; the kernel walks these survivors by index (no nucleus, so no order is needed)
        assert np.array_equal(np.sort(ref_order.numpy()), mine) and np.array_equal(np.sort(mine), mine)
    else:
        assert np.array_equal(ref_order.numpy(), mine), "survivor set or order differs from the reference's filter"
        assert np.abs(ref_cdf.numpy() - cdf[:n_nuc] / cdf[n_nuc - 1]).max() < 1e-6
    # every probe sits where it claims to: the oracle's inverse CDF returns the wanted token
    c64 = cdf[:n_nuc] / cdf[n_nuc - 1]
    r = np.searchsorted(c64, u.astype(np.float64), side="right")
    assert np.array_equal(order[np.minimum(r, n_nuc - 1)], want)
    d = sc.delta(s["n_sum"])
    edges = np.concatenate(([0.0], c64))
    mid, rm = u[:-2].astype(np.float64), r[:-2]      # the midpoint probes: delta away from both ends of their interval
    assert (mid - edges[rm]).min() >= d and (edges[rm + 1] - mid).min() >= d
    if c.finite_only:
        assert bool(torch.isfinite(v[torch.from_numpy(want)]).all())
    if c.same_tokens_as:
        o = sc.get(c.same_tokens_as).solve()
        assert np.array_equal(o["u"], u) and np.array_equal(o["want"], want)


def test_expected_on_the_signed_zero_row():
    """the row of the defect: the reference keeps zeros of both signs when the k-th value is a zero"""
    row = torch.tensor([1.0, 0.0, -0.0, -0.0, 0.0, -1.0, -2.0])
    order, n_nuc, _ = sc.expected(row, 2, 1.0)
    assert order.tolist() == [0, 1, 2, 3, 4] and n_nuc == 5
    kept = torch.isfinite(go.top_k_top_p_filtering(row[None], top_k=2)[0]).nonzero()[:, 0]
    assert kept.tolist() == [0, 1, 2, 3, 4]


def test_expected_never_returns_a_rank_without_mass():
    row = torch.tensor([0.5, sc.NEG_INF, 0.25, sc.NEG_INF])
    for top_k in (None, 0, 3, 4, 9):
        order, n_nuc, cdf = sc.expected(row, top_k, 1.0)
        assert order[:n_nuc].tolist() == ([0, 2]) and (top_k is None or len(order) == 4)
        u, want, _ = sc.probes(order, n_nuc, cdf, 4)
        assert want.tolist() == [0, 2, 0, 2]


@pytest.mark.parametrize("V,top_k,top_p,temp", sc.SEMANTICS_PARAMS)
def test_semantics_exclusions_stay_inside_their_caps(V, top_k, top_p, temp):
    """tests/test_gpu_lm.py::test_select_kernel_vs_reference_semantics leaves out hand-placed probes on intervals
    narrower than 1e-5 (it probes the next resolvable rank instead) and random draws within 2e-6 of a CDF value.  Both depend only on the oracle and on u: here the
    same rows and the same uniforms show that the caps that test now asserts (at least 90 % of the random draws counted,
    at most one hand-placed probe per row skipped) hold before any kernel runs."""
    B = 6
    lg = torch.randn(B, V, generator=torch.Generator().manual_seed(V + (top_k or 0))) * 3.0    # that test's rnd(...)
    lg[0, 10] = lg[0, 11]
    lg[1, 5] = lg[1].max() + 4.0
    vals = torch.div(lg, temp)
    oracles = [go.select_inverse_cdf(vals[b], top_k, top_p, 0.0) for b in range(B)]
    for b in range(B):
        skipped = sum(sc.semantics_hand_rank(oracles[b][2], f) is None for f in sc.SEMANTICS_FRACS)
        assert skipped <= sc.SEMANTICS_MAX_HAND_SKIPS, (b, skipped)
    g = torch.Generator().manual_seed(1)
    counted = total = 0
    for _ in range(20):
        u = torch.rand(B, generator=g, dtype=torch.float64)
        for b in range(B):
            total += 1
            counted += not sc.semantics_edge(oracles[b][2], u[b].float())
    print(f"counted {counted} of {total} random draws")
    assert counted >= sc.SEMANTICS_MIN_COUNTED * total
