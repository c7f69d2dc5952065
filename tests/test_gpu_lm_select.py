"""GPU (-m gpu): token selection (csrc/lm_select.hip) rank by rank against the exact expectations of
tests/lm_select_cases.py, and the stochastic sampling loops of omnitokenizer_amd/gpt.py draw by draw against the
oracle."""
import argparse
import ctypes

import numpy as np
import pytest
import torch

from oracle import gpt_oracle as go
from tests import lm_select_cases as sc
from tests.test_oracle_gpt import f64, load_gpt_case

pytestmark = pytest.mark.gpu
LOGIT_TOL = 1e-4          # tests/test_gpu_lm.py: the engine's logits against the same oracle
# The teacher-forced oracle passes below run in float64 on the same fp32 weights, like tests/test_gpu_lm_wide.py
# (tests/test_oracle_gpt.py pins that form to the reference's golden logits): with scale_cfg the blend at step 11 is
# 17.5 lc - 16.5 lu and multiplies rounding on the logits by up to 34, and the fp32 oracle ALONE is then 5.5e-5 from
# its float64 self on gpt_hd96 (2.3e-5 on gpt_hd64; 8e-6 / 5e-6 without scale_cfg, 6e-6 / 2e-6 on the plain loop) --
# more than half of LOGIT_TOL would be the reference's own error, charged to the engine.


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _select(c, u, sample=1, want_blend=False):
    """one launch of omnitok_lm_select on the case's row repeated once per uniform -> (tokens, err flag, blend)"""
    from omnitokenizer_amd import _lib
    lib = _lib.load()
    B, V = (1 if u is None else int(u.size)), c.logits.numel()
    lc = c.logits.cuda()[None].expand(B, V).contiguous()
    lu = None if c.logits_uncond is None else c.logits_uncond.cuda()[None].expand(B, V).contiguous()
    ud = None if u is None else torch.from_numpy(u).cuda()
    out = torch.full((B,), -1, dtype=torch.int64, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    blend = torch.empty(B, V, dtype=torch.float32, device="cuda") if want_blend else None
    _lib.check(lib.omnitok_lm_select(_p(lc), _p(lu), B, V, float(c.temperature), float(1 + c.cfg_t), float(c.cfg_t),
                                     c.kernel_top_k(), c.kernel_top_p(), sample, _p(ud), _p(out), _p(blend), _p(err),
                                     torch.cuda.current_stream().cuda_stream), "lm_select")
    return out.cpu().numpy(), int(err.item()), None if blend is None else blend.cpu()


@pytest.mark.parametrize("name", sc.case_names())
def test_select_rank_by_rank(name):
    """One launch, one kernel row per probed rank: every token equals the expectation (no probe is excluded; the helper
    asserts that every probed interval is wide enough for that), the overflow flag is raised exactly where a nucleus
    meets more survivors than the sort buffer holds, and greedy returns the lowest index among the maxima."""
    c = sc.get(name)
    s = c.solve()
    v = c.values()
    got, err, _ = _select(c, s["u"])
    bad = np.nonzero(got != s["want"])[0]
    assert bad.size == 0, (f"{bad.size} of {got.size} probes differ; first: probe {bad[0]} u={s['u'][bad[0]]!r} "
                           f"got {got[bad[0]]} (value {float(v[got[bad[0]]]) if 0 <= got[bad[0]] < v.numel() else None})"
                           f" want {s['want'][bad[0]]} (value {float(v[s['want'][bad[0]]])})")
    assert err == (1 if c.overflow else 0)
    if c.finite_only:
        assert bool(torch.isfinite(v[torch.from_numpy(got)]).all())
    if c.same_tokens_as:
        other = sc.get(c.same_tokens_as)
        assert np.array_equal(other.solve()["u"], s["u"])
        assert np.array_equal(_select(other, s["u"])[0], got)
    greedy, gerr, blend = _select(c, None, sample=0, want_blend=True)
    assert int(greedy[0]) == int(torch.nonzero(v == v.max())[0, 0]) and gerr == 0
    # the values the selection saw are the reference's own sequence of roundings, bit for bit (signs of zeros too)
    assert torch.equal(blend[0].view(torch.int32), v.view(torch.int32))


# ---- the stochastic loops, draw by draw ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpts():
    cache = {}

    def get(name):
        if name not in cache:
            from omnitokenizer_amd.gpt import GPT
            g, sd, (V, BS, L, H, C) = load_gpt_case(name)
            m = GPT(argparse.Namespace(), V, BS, n_layer=L, n_head=H, n_embd=C)
            m.load_state_dict(sd, strict=True)
            cache[name] = (m.cuda().eval(), f64(sd), H, V)
        return cache[name]
    return get


def _replay_uniforms(seed, B, steps):
    """The uniforms a loop consumed.  RELIES ON how select_tokens takes them from torch's generator: exactly one
    torch.rand(B, device="cuda") per step from the default generator, and nothing else in the loop draws from it."""
    torch.manual_seed(seed)
    return torch.stack([torch.rand(B, device="cuda") for _ in range(steps)], 1).cpu()     # [B, steps]


def _check_draws(tok, lg, us, top_k, top_p, V):
    """(a): token n of stream b is the oracle's inverse-CDF token for the logits the selection saw and the replayed
    uniform -- unless u lies within delta of a CDF value, or top_p within delta of a value of the survivors' CDF (the
    cut itself could then fall either way).  delta = lm_select_cases.delta(n_keep), n_keep = top_k (V without a filter);
    the expected share of exclusions, n_keep * 2 delta, is under 1.25 % for every setting used here; the cap is 5 %."""
    B, steps = tok.shape
    n_keep = V if top_k is None else min(top_k, V)
    d = sc.delta(n_keep)
    assert n_keep * 2 * d < 0.0125
    excluded = 0
    for b in range(B):
        for n in range(steps):
            u = float(us[b, n])
            want, order, cdf = go.select_inverse_cdf(lg[b, n], top_k, top_p, u)
            near = (cdf - u).abs().min().item() < d
            if top_k is not None and top_p is not None and top_p < 1.0:
                near = near or np.abs(sc.expected(lg[b, n], top_k, None)[2] - top_p).min() < d
            if near:
                excluded += 1
                assert int(tok[b, n]) in set(order.tolist())
                continue
            assert int(tok[b, n]) == want, (b, n, int(tok[b, n]), want, u)
    share = excluded / (B * steps)
    print(f"excluded {excluded} of {B * steps} draws ({100 * share:.2f} %, cap 5 %, expected under "
          f"{100 * n_keep * 2 * d:.2f} %)")
    assert share <= 0.05
    assert len(set(tok.flatten().tolist())) > 1       # draws, not one token over and over


@pytest.mark.parametrize("top_k,top_p", [(8, 1.0), (50, 0.9), (None, None)])
@pytest.mark.parametrize("name", ["gpt_hd64", "gpt_hd96"])
def test_sample_with_past_draw_by_draw(gpts, name, top_k, top_p):
    from omnitokenizer_amd import gpt as og
    m, sd64, H, V = gpts(name)
    B, steps, temp, seed = 8, 12, 0.9, 1234
    x = torch.randint(0, V, (B, 3), generator=torch.Generator().manual_seed(7))
    runs = {}
    for use_graph in (True, False):
        torch.manual_seed(seed)
        tok, lg = og.sample_with_past(x.cuda(), m, steps, temperature=temp, sample_logits=True, top_k=top_k, top_p=top_p,
                                      use_graph=use_graph, return_logits=True)
        runs[use_graph] = (tok.cpu(), lg.cpu())
    assert torch.equal(runs[True][0], runs[False][0]), "graph and non-graph loops drew different tokens"
    us = _replay_uniforms(seed, B, steps)
    for use_graph, (tok, lg) in runs.items():
        _check_draws(tok, lg, us, top_k, top_p, V)
        # (b) the loop fed back the token it drew, at the right position: a teacher-forced oracle pass over the GPU's
        # own tokens reproduces the logits every draw was made from
        with torch.no_grad():
            ref_tok, ref_lg = go.sample_with_past(sd64, x, H, steps, temperature=temp, return_logits=True, forced=tok)
        assert torch.equal(ref_tok, tok) and ref_lg.dtype == torch.float64
        e = (lg.double() - ref_lg).abs().max().item()
        print(f"{name} graph={use_graph}: logits vs the teacher-forced oracle {e:.2e}")
        assert e < LOGIT_TOL


@pytest.mark.parametrize("scale_cfg", [False, True])
@pytest.mark.parametrize("name", ["gpt_hd64", "gpt_hd96"])
def test_sample_with_past_cfg_draw_by_draw(gpts, name, scale_cfg):
    from omnitokenizer_amd import gpt as og
    m, sd64, H, V = gpts(name)
    B, steps, seed, top_k, top_p = 6, 12, 4321, 50, 0.9
    cls = torch.randint(0, V - 1, (B, 1), generator=torch.Generator().manual_seed(9))
    kw = dict(cfg_ratio=1.5, class_first=scale_cfg, scale_cfg=scale_cfg)
    runs = {}
    for use_graph in (True, False):
        torch.manual_seed(seed)
        tok, lg = og.sample_with_past_cfg(cls.cuda(), m, steps, sample_logits=True, top_k=top_k, top_p=top_p,
                                          use_graph=use_graph, return_logits=True, **kw)
        runs[use_graph] = (tok.cpu(), lg.cpu())
    assert torch.equal(runs[True][0], runs[False][0]), "graph and non-graph loops drew different tokens"
    us = _replay_uniforms(seed, B, steps)
    for use_graph, (tok, lg) in runs.items():
        _check_draws(tok, lg, us, top_k, top_p, V)
        # (b) on the conditional AND the unconditional rows: the blend mixes both streams' logits
        with torch.no_grad():
            ref_tok, ref_lg = go.sample_with_past_cfg(sd64, cls, H, steps, return_logits=True, forced=tok, **kw)
        assert torch.equal(ref_tok, tok) and ref_lg.dtype == torch.float64
        e = (lg.double() - ref_lg).abs().max().item()
        print(f"{name} graph={use_graph} scale_cfg={scale_cfg}: blend vs the teacher-forced oracle {e:.2e}")
        assert e < LOGIT_TOL
