"""Rows, exact expectations and probes for the token selection kernel (csrc/lm_select.hip); CPU only.

`expected` restates the reference's filter (gpt.py:19-51) on one fp32 row exactly: survivors by FLOAT comparison
(`values >= kth`: +0 and -0 are equal, ties at the k-th value are kept), ranked by descending value with ascending
index among equals, softmax over the survivors in float64, nucleus by the predecessors' mass.  `probes` turns
that into uniforms for ONE launch with one kernel row per probed rank (the same logits row repeated, only u[b]
differs), so a launch returns the kernel's whole rank -> token map and every token is compared, none excluded.

That is only sound where fp32 cannot move a probe across an interval edge, or the nucleus cut across a rank.  The
helper asserts it (it never skips a case over it): every probed interval of the renormalised nucleus CDF, and the
gap a designed top_p sits in the middle of, is at least 2 * delta(n) wide, where

    delta(n) = 8 * (n / 1024 + 24) * 2^-24

bounds the kernel's error on a CDF value relative to the total mass: a thread adds its chunk of at most
ceil(n / 1024) fp32 terms (a few more for the fall-back recomputations), the block scan adds 10 more levels, expf
is good to 1 ulp, the product u * Z rounds once; the sum of those, times 8 as margin.  n is the number of terms the
kernel sums: the survivors on the sorted path, V on the unsorted one.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np
import torch

NEG_INF = float("-inf")
U_LAST = 1.0 - 2.0 ** -24        # the largest fp32 below 1: what torch.rand can return at most
SORT_MAX = 16384                 # survivors the kernel's sort buffer holds


def delta(n: int) -> float:
    return 8.0 * (n / 1024.0 + 24.0) * 2.0 ** -24


def expected(values, top_k, top_p, index_order=False):
    """(order, n_nuc, cdf64) of one fp32 row.  order: the survivors' columns by rank (all of them, zero-mass
    `-inf` survivors last); cdf64: cumulative softmax over them; n_nuc: how many ranks the draw can return -- rank r
    stays iff r == 0 or cdf[r - 1] <= top_p (top_p None or >= 1: no cut, like the reference), and never a rank without
    mass (the reference's multinomial cannot return one either).  top_k None: no filter, the columns with mass in
    index order.  index_order: the survivors in index order instead (what the kernel walks when more than SORT_MAX
    survive and no nucleus is asked for)."""
    v = torch.as_tensor(values)
    assert v.dtype == torch.float32 and v.dim() == 1 and not torch.isnan(v).any()
    V = v.numel()
    if top_k is None:
        keep = torch.nonzero(v > NEG_INF)[:, 0]
        top_p = None
    else:
        if top_k > 0:
            kth = torch.topk(v, min(top_k, V))[0][-1]
            keep = torch.nonzero(v >= kth)[:, 0]                     # float comparison: 0.0 == -0.0, ties kept
        else:
            keep = torch.arange(V)
        if not index_order:
            # stable: ascending index among equals (-0.0 and 0.0 compare equal in the sort as well)
            keep = keep[torch.sort(-v[keep].double(), stable=True)[1]]
    assert keep.numel() > 0
    vk = v[keep].double()
    pr = torch.exp(vk - vk.max())
    pr = pr / pr.sum()
    cdf = torch.cumsum(pr, 0)
    n_mass = int((vk > NEG_INF).sum())
    if index_order or top_k is None:
        assert top_p is None or top_p >= 1.0
        n_nuc = keep.numel() if index_order else n_mass
    elif top_p is None or top_p >= 1.0:
        n_nuc = n_mass
    else:
        n_nuc = min(1 + int((cdf[:-1] <= float(top_p)).sum()), n_mass)     # cdf is non-decreasing: a prefix
    return keep.numpy().astype(np.int64), n_nuc, cdf.numpy()


def nucleus_top_p(values, top_k, n_nuc):
    """top_p (an fp32 value) that leaves exactly n_nuc ranks: the midpoint of the gap of the survivors' CDF that the cut
    must fall into, so its margin is half that gap; asserts the gap is at least 2 * delta wide."""
    order, _, cdf = expected(values, top_k, None)
    assert 1 <= n_nuc <= len(order)
    lo = 0.0 if n_nuc == 1 else float(cdf[n_nuc - 2])      # rank n_nuc - 1 stays: cdf[n_nuc - 2] <= top_p
    hi = float(cdf[n_nuc - 1])                             # rank n_nuc goes:      cdf[n_nuc - 1] >  top_p
    top_p = float(np.float32((lo + hi) / 2))
    assert hi - lo >= 2 * delta(len(order)), (hi - lo, 2 * delta(len(order)))
    assert 0.0 < top_p < 1.0 and lo + delta(len(order)) <= top_p <= hi - delta(len(order))
    return top_p


def probes(order, n_nuc, cdf, n_sum, ranks=None):
    """(u fp32 [P], want int64 [P], min_width): one probe at the float64 midpoint of each rank's interval of the
    renormalised nucleus CDF (ranks None: every rank below n_nuc), then u = 0 (-> order[0]) and u = 1 - 2^-24
    (-> the last rank that can be drawn).  Asserts every probed interval, the first and the last one are at least
    2 * delta(n_sum) wide."""
    c = np.asarray(cdf[:n_nuc], dtype=np.float64) / float(cdf[n_nuc - 1])
    lo = np.concatenate(([0.0], c[:-1]))
    width = c - lo
    mass = np.nonzero(width > 0)[0]
    first, last = int(mass[0]), int(mass[-1])
    if ranks is None:
        ranks = np.arange(n_nuc)
    ranks = np.unique(np.asarray(ranks, dtype=np.int64))
    assert ranks.size and ranks.min() >= 0 and ranks.max() < n_nuc
    need = 2 * delta(n_sum)
    checked = np.unique(np.concatenate((ranks, [first, last])))
    min_width = float(width[checked].min())
    assert min_width >= need, f"narrowest probed interval {min_width:.2e} < 2 delta = {need:.2e}"
    u = np.concatenate(((lo[ranks] + c[ranks]) / 2, [0.0, U_LAST])).astype(np.float32)
    assert u.max() < 1.0
    want = np.concatenate((order[ranks], [order[first], order[last]])).astype(np.int64)
    return u, want, min_width


# ---- rows ------------------------------------------------------------------------------------------------------------
def urow(V, amp, seed):
    """V DISTINCT fp32 values uniform in +-amp (a chance tie would move n_keep off the designed top_k)."""
    rs = np.random.RandomState(seed)
    v = (rs.uniform(-amp, amp, V)).astype(np.float32)
    while True:
        _, first = np.unique(v, return_index=True)
        dup = np.setdiff1d(np.arange(V), first)
        if dup.size == 0:
            return torch.from_numpy(v)
        v[dup] = rs.uniform(-amp, amp, dup.size).astype(np.float32)


def _shuffled(vals, seed):
    v = np.asarray(vals, dtype=np.float32)
    return torch.from_numpy(v[np.random.RandomState(seed).permutation(v.size)])


def radix_groups(sign=1.0, n=24):
    """Four groups of finite values whose keys differ, inside a group, only in byte 0, 1, 2 or 3."""
    j = np.arange(1, n + 1, dtype=np.float64)
    g0 = sign * (1.0 + j * 2.0 ** -23)      # mantissa bits 0..7   -> key byte 0
    g1 = sign * (1.0 + j * 2.0 ** -15)      # mantissa bits 8..15  -> key byte 1
    g2 = sign * (1.0 + j * 2.0 ** -7)       # mantissa bits 16..22 -> key byte 2
    return [g0, g1, g2]


def radix_row(kind):
    """'pos': the three mantissa groups above 1 and byte 3 (sign and exponent) as {+-2, +-1, +-0.5};
    'neg': every value negative (keys are the inverted bits); 'mixed': both signs of every group."""
    if kind == "pos":
        parts = radix_groups(1.0) + [np.array([2.0, 1.0, 0.5, -0.5, -1.0, -2.0])]
    elif kind == "neg":
        parts = radix_groups(-1.0) + [np.array([-4.0, -2.0, -1.0, -0.5, -0.25, -0.125])]
    else:
        parts = radix_groups(1.0) + radix_groups(-1.0) + [np.array([2.0, 1.0, 0.5, -0.5, -1.0, -2.0])]
    row = _shuffled(np.concatenate(parts), seed=len(kind))
    assert np.unique(row.numpy()).size == row.numel()
    # k inside each group and on each group edge: the ranks where the sorted row changes group, +-1, and the middles
    s = np.sort(row.numpy().astype(np.float64))[::-1]
    grp = np.zeros(s.size, dtype=np.int64)
    for gi, part in enumerate(parts):
        grp[np.isin(s, part.astype(np.float32).astype(np.float64))] = gi
    edges = [0] + [i for i in range(1, s.size) if grp[i] != grp[i - 1]] + [s.size]
    ks = set()
    for a, b in zip(edges[:-1], edges[1:]):
        ks.update({a + 1, (a + b) // 2 + 1, b})       # first, middle and last rank of the run, as 1-based k
    return row, sorted(k for k in ks if 1 <= k <= s.size)


def with_ties(row, rank0, m):
    """`row` with the value of (0-based) rank `rank0` copied over the next m - 1 ranks: m equal values at ranks
    rank0 .. rank0 + m - 1."""
    row = row.clone()
    idx = torch.sort(row, descending=True, stable=True)[1]
    row[idx[rank0:rank0 + m]] = float(row[idx[rank0]])
    return row


def zero_row(V, n_pos, n_zero, seed):
    """n_pos positive values, n_zero zeros of both signs, the rest negative, shuffled."""
    rs = np.random.RandomState(seed)
    a = np.abs(urow(V, 1.0, seed).numpy()) + np.float32(0.01)
    a[n_pos:] *= -1
    a[n_pos:n_pos + n_zero] = np.where(np.arange(n_zero) % 3 == 1, 0.0, -0.0).astype(np.float32)
    row = torch.from_numpy(a[rs.permutation(V)])
    assert int((row == 0).sum()) == n_zero and int(torch.signbit(row[row == 0]).sum()) not in (0, n_zero)
    return row


def ninf_row(V, n_inf, amp, seed):
    row = urow(V, amp, seed)
    row[torch.from_numpy(np.random.RandomState(seed + 1).permutation(V)[:n_inf])] = NEG_INF
    return row


def ends_and_stride(n, stride=37, ends=64):
    """the first `ends` ranks, the last `ends` ranks and every `stride`-th one of n"""
    return np.unique(np.concatenate((np.arange(min(ends, n)), np.arange(max(n - ends, 0), n), np.arange(0, n, stride))))


# ---- cases -----------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    logits: torch.Tensor                       # [V] fp32, raw (before the temperature division)
    top_k: Optional[int]
    top_p: Optional[float] = None              # None: 1.0 (no nucleus)
    n_nuc: Optional[int] = None                # design the nucleus instead: top_p = nucleus_top_p(values, top_k, n_nuc)
    ranks: Optional[np.ndarray] = None         # probed ranks (None: all)
    n_probes: Optional[int] = None             # what the table says: probed ranks + 2
    n_keep: Optional[int] = None               # designed number of survivors (checked)
    temperature: float = 1.0
    logits_uncond: Optional[torch.Tensor] = None
    cfg_t: float = 0.0
    index_order: bool = False                  # more than SORT_MAX survivors, no nucleus: drawn in index order
    overflow: bool = False                     # more than SORT_MAX survivors AND a nucleus: flag set, token = argmax
    finite_only: bool = False                  # every returned token must have a finite logit (also asserted)
    same_tokens_as: Optional[str] = None       # another case whose tokens must be identical, probe by probe
    _solved: dict = field(default_factory=dict, repr=False)

    def values(self):
        """what the selection sees: the reference's own sequence of fp32 roundings (gpt.py:347, :428-431)"""
        lc = torch.div(self.logits, self.temperature)
        if self.logits_uncond is None:
            return lc
        lu = torch.div(self.logits_uncond, self.temperature)
        t = self.cfg_t
        return (1 + t) * lc - t * lu

    def solve(self):
        """dict(order, n_nuc, cdf, u, want, top_p, n_sum, min_width); asserts every precondition"""
        if self._solved:
            return self._solved
        v = self.values()
        assert v.dtype == torch.float32
        top_p = self.top_p
        if self.n_nuc is not None:
            top_p = nucleus_top_p(v, self.top_k, self.n_nuc)
        if self.overflow:
            order, _, cdf = expected(v, self.top_k, None)
            assert len(order) > SORT_MAX and top_p is not None and top_p < 1.0
            u = np.array([0.0, 0.25, 0.5, 0.75, U_LAST], dtype=np.float32)
            amax = int(torch.nonzero(v == v.max())[0, 0])
            res = dict(order=order, n_nuc=None, cdf=cdf, u=u, want=np.full(u.size, amax, dtype=np.int64), top_p=top_p,
                       n_sum=v.numel(), min_width=None)
        else:
            order, n_nuc, cdf = expected(v, self.top_k, top_p, index_order=self.index_order)
            unsorted = self.top_k is None or self.index_order
            assert self.index_order == (self.top_k is not None and len(order) > SORT_MAX)
            n_sum = v.numel() if unsorted else len(order)
            if self.n_nuc is not None:
                assert n_nuc == self.n_nuc
            u, want, mw = probes(order, n_nuc, cdf, n_sum, self.ranks)
            res = dict(order=order, n_nuc=n_nuc, cdf=cdf, u=u, want=want, top_p=top_p, n_sum=n_sum, min_width=mw)
        if self.n_keep is not None:
            assert len(res["order"]) == self.n_keep, (len(res["order"]), self.n_keep)
        if self.n_probes is not None:
            assert res["u"].size == self.n_probes, (res["u"].size, self.n_probes)
        if self.finite_only:
            assert bool(torch.isfinite(v[torch.from_numpy(res["want"])]).all())
        self._solved = res
        return res

    def kernel_top_k(self):
        return -1 if self.top_k is None else int(self.top_k)

    def kernel_top_p(self):
        p = self.solve()["top_p"]
        return 1.0 if p is None else float(p)


def _cfg(case, name, t, seed, exact=False):
    """`case` once more through the CFG blend, values = (1 + t) lc - t lu.  exact (t = 1): lu = lc (0 where lc is a zero
    or -inf), so 2 lc - lu is lc bit for bit and the designed row (ties, radix bytes, signed zeros, -inf) reaches the
    selection unchanged; otherwise lu is an independent random row and both are scaled so that the blend keeps the
    amplitude of the original row."""
    lc = case.logits
    if exact:
        assert t == 1.0
        lu = torch.where(torch.isfinite(lc) & (lc != 0), lc, torch.zeros_like(lc))
        new = Case(**{**_fields(case), "name": name, "logits_uncond": lu, "cfg_t": t})
        assert torch.equal(new.values().view(torch.int32), case.values().view(torch.int32))    # signs of zeros too
        return new
    s = 1.0 / (1 + 2 * t)
    amp = float(lc[torch.isfinite(lc)].abs().max())
    lu = urow(lc.numel(), amp, seed) * s
    return Case(**{**_fields(case), "name": name, "logits": lc * s, "logits_uncond": lu, "cfg_t": t})


def _fields(case):
    return {k: getattr(case, k) for k in case.__dataclass_fields__ if k != "_solved"}


def _build():
    cs: List[Case] = []
    add = cs.append
    # bitonic padding (P = 128, 256, 512, 2048, 4096) and the in-wave / LDS stage boundary
    for k in (1, 2, 127, 128, 129, 255, 256, 257):
        add(Case(f"bitonic_k{k}", urow(320, 1.0, 100 + k), k, n_keep=k, n_probes=k + 2))
    for k in (2047, 2048, 2049):
        add(Case(f"bitonic_k{k}", urow(9193, 1.0, 100 + k), k, n_keep=k, n_probes=k + 2))
    # radix passes
    radix_mid = {}
    for kind in ("pos", "neg", "mixed"):
        row, ks = radix_row(kind)
        radix_mid[kind] = f"radix_{kind}_k{ks[len(ks) // 2]}"
        for k in ks:
            add(Case(f"radix_{kind}_k{k}", row, k, n_keep=k, n_probes=k + 2))
    # ties
    add(Case("tie5_k42", with_ties(urow(320, 1.0, 201), 40, 5), 42, n_keep=45, n_probes=47))
    add(Case("tie5_k2046", with_ties(urow(9193, 1.0, 202), 2044, 5), 2046, n_keep=2049, n_probes=2051))
    add(Case("tie_all_equal", torch.full((2048,), 0.375), 1, n_keep=2048, n_probes=2050))
    add(Case("zero_kth_small", torch.tensor([1.0, 0.0, -0.0, -0.0, 0.0, -1.0, -2.0]), 2, n_keep=5, n_probes=7))
    add(Case("zero_kth", zero_row(320, 10, 6, 203), 12, n_keep=16, n_probes=18))
    # (the cut sits after the zeros: where it falls INSIDE a tie the reference's unstable sort decides which copies stay)
    add(Case("zero_kth_nucleus", zero_row(320, 10, 6, 203), 12, n_nuc=16, n_keep=16, n_probes=18))
    add(Case("zero_max_greedy", torch.tensor([-1.0, -0.0, 0.0, -0.0, -3.0]), 1, n_keep=3, n_probes=5))
    zr = zero_row(17385, 16380, 10, 204) * 0.1
    add(Case("zero_kth_overflow", zr, 16383, n_keep=16390, index_order=True, ranks=ends_and_stride(16390),
             n_probes=ends_and_stride(16390).size + 2))
    # -inf
    ni = ninf_row(300, 100, 1.0, 301)
    for k in (None, 0, 300, 307, 200, 201):
        add(Case(f"ninf_k{k}", ni, k, n_keep=200 if k in (None, 200) else 300, n_probes=202, finite_only=True))
    add(Case("ninf_k0_nucleus", ni, 0, n_nuc=200, n_keep=300, n_probes=202, finite_only=True))
    nb = ninf_row(9193, 3064, 1.0, 302)
    for k in (0, 6129, 6130):
        r = ends_and_stride(6129, stride=5)
        add(Case(f"ninf_big_k{k}", nb, k, n_keep=6129 if k == 6129 else 9193, ranks=r, n_probes=r.size + 2,
                 finite_only=True))
    one = torch.full((300,), NEG_INF)
    one[137] = -2.5
    for k in (None, 0, 1, 5):
        add(Case(f"ninf_one_finite_k{k}", one, k, n_probes=3, finite_only=True))
    # sort buffer
    sb = urow(17385, 0.1, 401)
    r = ends_and_stride(16384)
    add(Case("sortbuf_k16384", sb, 16384, n_keep=16384, ranks=r, n_probes=r.size + 2))
    r = ends_and_stride(12000)
    add(Case("sortbuf_k16384_nucleus", sb, 16384, n_nuc=12000, n_keep=16384, ranks=r, n_probes=r.size + 2))
    sbt = with_ties(sb, 16383, 2)
    r = ends_and_stride(16385)
    add(Case("sortbuf_tie_16385", sbt, 16384, n_keep=16385, index_order=True, ranks=r, n_probes=r.size + 2))
    add(Case("sortbuf_tie_16385_nucleus", sbt, 16384, top_p=0.9, n_keep=16385, overflow=True, n_probes=5))
    # the register build / re-reading build seam
    seam = urow(16384, 1.0, 501)
    add(Case("seam_16384", seam, 2048, n_keep=2048, n_probes=2050))
    add(Case("seam_16385", torch.cat((seam, torch.tensor([NEG_INF]))), 2048, n_keep=2048, n_probes=2050,
             same_tokens_as="seam_16384"))
    for V in (1024, 1025, 16385):
        row = urow(V, 1.0, 510 + V % 7)
        row[-1] = row.max() + 0.5             # the last column (alone in its pass of the row when V = 1024 j + 1) ranks first
        add(Case(f"seam_lastmax_{V}", row, 100, n_keep=100, n_probes=102))
    # nucleus count
    for V, k in ((320, 300), (9193, 2049)):
        row = urow(V, 1.0, 600 + V % 11)
        for n in (1, 2, 128, 129, k - 1, k):
            add(Case(f"nucleus_k{k}_n{n}", row, k, n_nuc=n, n_keep=k, n_probes=n + 2))
    # unsorted path
    add(Case("unsorted_1000", urow(1000, 1.0, 701), None, n_probes=1002))
    add(Case("unsorted_1025", urow(1025, 1.0, 702), None, n_probes=1027))
    un = urow(17385, 0.1, 703)
    r = ends_and_stride(17385)
    add(Case("unsorted_17385", un, None, ranks=r, n_probes=r.size + 2))
    un2 = un.clone()
    un2[5000:7000] = NEG_INF               # 17 columns per thread: the run spans whole per-thread chunks
    r = np.unique(np.concatenate((ends_and_stride(15385), np.arange(4990, 5010))))   # ranks over the columns with mass
    add(Case("unsorted_17385_ninf_run", un2, None, n_keep=15385, ranks=r, n_probes=r.size + 2, finite_only=True))
    # temperature
    by = {c.name: c for c in cs}
    add(Case(**{**_fields(by["bitonic_k257"]), "name": "temp07_bitonic_k257", "temperature": 0.7}))
    add(Case(**{**_fields(by["nucleus_k300_n128"]), "name": "temp13_nucleus_k300_n128", "temperature": 1.3}))
    # CFG: each row kind once more
    for i, (src, exact) in enumerate([("bitonic_k129", False), ("bitonic_k2049", False), (radix_mid["mixed"], True),
                                      (radix_mid["neg"], True), ("tie5_k42", True), ("tie_all_equal", True),
                                      ("zero_kth", True), ("zero_kth_small", True), ("ninf_k0", True), ("ninf_kNone", False),
                                      ("ninf_k201", False), ("sortbuf_k16384", False), ("sortbuf_tie_16385", True),
                                      ("sortbuf_tie_16385_nucleus", True), ("seam_16384", False), ("seam_lastmax_16385", False),
                                      ("nucleus_k300_n129", False), ("nucleus_k2049_n2048", False),
                                      ("unsorted_1025", False), ("unsorted_17385_ninf_run", False)]):
        add(_cfg(by[src], "cfg_" + src, 1.0 if exact else 1.5, 800 + i, exact))
    add(Case(**{**_fields(_cfg(by["bitonic_k128"], "cfg_temp07_bitonic_k128", 1.5, 899)), "temperature": 0.7}))
    names = [c.name for c in cs]
    assert len(set(names)) == len(names)
    return cs


_CASES: List[Case] = []


def cases() -> List[Case]:
    if not _CASES:
        _CASES.extend(_build())
    return _CASES


def case_names() -> List[str]:
    return [c.name for c in cases()]


def get(name) -> Case:
    return next(c for c in cases() if c.name == name)


# ---- the exclusions of tests/test_gpu_lm.py::test_select_kernel_vs_reference_semantics -----------------------------------
SEMANTICS_PARAMS = [(320, 50, 0.9, 0.9), (9193, 2048, 0.9, 1.0), (9193, 64, 1.0, 0.7), (300, 300, 0.5, 1.0),
                    (520, 1, 0.3, 1.0), (17385, None, None, 1.0), (9193, 0, 0.7, 1.3), (8193, 8192, 0.95, 1.0),
                    (17385, 100, 0.9, 1.0), (16384, 2048, 0.9, 1.0)]
SEMANTICS_FRACS = (0.0, 0.3, 0.77, 0.999)
SEMANTICS_MIN_WIDTH = 1e-5       # hand-placed probes on a narrower interval are skipped
SEMANTICS_EDGE = 2e-6            # random draws this close to a CDF value are not counted
SEMANTICS_MIN_COUNTED = 0.9      # ... but at least this share of them must be
SEMANTICS_MAX_HAND_SKIPS = 1     # ... and at most this many hand-placed probes per row may be skipped


def semantics_hand_rank(cdf, frac):
    """the rank that test probes for `frac` of a row with this oracle CDF: int(frac * n), or -- where fp32 cannot resolve
    that interval (narrower than SEMANTICS_MIN_WIDTH) -- the next rank, cyclically, whose interval it can; None if the
    row has none, and only then is the probe skipped.  (Probing int(frac * n) alone skipped three of the four probes
    of a row of the V = 17385 unfiltered set: four fifths of its intervals are narrower than 1e-5.)"""
    n = len(cdf)
    r = min(int(frac * n), n - 1)
    c = np.asarray(cdf, dtype=np.float64)
    ok = np.nonzero(np.diff(np.concatenate(([0.0], c))) > SEMANTICS_MIN_WIDTH)[0]
    if ok.size == 0:
        return None
    later = ok[ok >= r]
    return int(later[0] if later.size else ok[0])


def semantics_edge(cdf, u):
    """whether that test leaves the random draw u of a row with this oracle CDF uncounted"""
    return (cdf - float(u)).abs().min().item() < SEMANTICS_EDGE
