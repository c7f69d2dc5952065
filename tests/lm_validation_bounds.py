"""Derived error bars of the LM validation kernels (csrc/lm_loss.hip), from tests/error_bounds.py.

Per row, against the fp64 evaluation of the same fp32 logits l_j (m = max_j l_j, d_j = l_j - m <= 0, s = sum_j exp(d_j),
p_j = exp(d_j) / s, nll = (m + log s) - l_t):

  * one rounding of each d_j:  |delta d_j| <= u |d_j|, a relative error expm1(u |d_j|) of term j, p-weighted in s.
    In the wide-row kernel a term reaches the row maximum in steps (its lane's running maximum, then the row's): the steps'
    arguments are all <= 0 and add up to d_j, so their roundings add up to at most the same u |d_j|;
  * expf within EXPF_ULPS of the true value: at most EXPF_ULPS * 2u relative per term;
  * the sum of V positive terms: gamma(V).  Adding an exact zero rounds nothing, so a row of V terms has at most V - 1 inexact
    additions however the lanes and waves share it.  In the wide-row kernel (V > 1024) a term's path has V / 256 adds in its lane,
    at most V / 4096 + 1 rescales of 3u each (an expf and a product), the final rescale and 8 adds across lanes and waves: under
    30 + V / 200 roundings, inside gamma(V) for every V > 1024;
  * logf within LOGF_ULPS of the true value: LOGF_ULPS * 2u |log s|;
  * the two fp32 additions of the three-term sum, in either association: the kernel forms (m + log s) - l_t, torch's
    log_softmax forms (l_t - m) - log s; the first partial is rounded at u |m + log s| or u |l_t - m|, the result at u |nll|.
    The bar takes the larger partial, so that it holds for the reference's own fp32 cross-entropy as well (the issue's check
    that the bar is not tighter than the reference itself): u max(|m + log s|, |l_t - m|) + u |nll|.

The loss is the fp64 sum of the counted rows' nll over their count, rounded to fp32 once: the mean of the rows' bars plus
u |loss|.
"""
import torch

from omnitokenizer_amd.lm_losses import MAX_ROWS
from tests import error_bounds as eb
from tests.test_gpu_lm import LOGIT_TOL  # noqa: F401  (1e-4: the logits' own tolerance against the reference)

U = eb.U
# HIP math API, single precision accuracy table: expf 1 ulp, logf 1 ulp (full range); 1 ulp <= 2u relative
EXPF_ULPS = 1
LOGF_ULPS = 1


def nll64(logits, targets):
    """fp64 logsumexp(l) - l_t of fp32 logits [N, V]; rows with a target < 0 give 0"""
    l = logits.double()
    t = targets.clamp(min=0)
    out = torch.logsumexp(l, -1) - l.gather(-1, t[:, None]).squeeze(-1)
    return torch.where(targets >= 0, out, torch.zeros_like(out))


def nll_bar(logits, targets):
    """[N] bound on |nll_kernel - nll64| for fp32 logits [N, V] and valid targets (rows with a target < 0: 0)"""
    l = logits.double()
    V = l.shape[-1]
    m = l.amax(-1, keepdim=True)
    d = l - m
    e = torch.exp(d)
    s = e.sum(-1, keepdim=True)
    arg = (e / s * torch.expm1(U * d.abs())).sum(-1)
    rel_s = (1 + arg) * (1 + EXPF_ULPS * 2 * U) * (1 + eb.gamma(V)) - 1
    log_s = torch.log(s).squeeze(-1)
    d_log = -torch.log1p(-rel_s) + LOGF_ULPS * 2 * U * log_s.abs()
    a = m.squeeze(-1) + log_s
    lt = l.gather(-1, targets.clamp(min=0)[:, None]).squeeze(-1)
    nll = a - lt
    partial = torch.maximum(a.abs(), (lt - m.squeeze(-1)).abs())
    bar = (d_log + U * (partial + d_log) + U * nll.abs()) * (1 + 2 * U)
    return torch.where(targets >= 0, bar, torch.zeros_like(bar))


def loss_bar(row_bars, targets, loss):
    """bound on |loss_kernel - loss64|: the counted rows' mean bar plus one fp32 rounding of the loss"""
    keep = targets >= 0
    return float(row_bars[keep].mean()) + U * abs(float(loss))


def rank_of_target(logits, targets):
    """#{j : l_j > l_t} + #{j < t : l_j == l_t} per row, by torch on the same tensor (valid targets)"""
    lt = logits.gather(-1, targets[:, None])
    j = torch.arange(logits.shape[-1], device=logits.device)[None, :]
    return ((logits > lt).sum(-1) + ((logits == lt) & (j < targets[:, None])).sum(-1)).to(torch.int32)


def reference_accuracy(correct_k, count):
    """the reference's `correct_k.mul_(100.0 / batch_size)` (utils.py:203-204): an fp32 tensor times a Python double"""
    return torch.tensor([float(correct_k)], dtype=torch.float32).mul_(100.0 / count)


def ce_case(N, V, scale, seed=0):
    """seeded fp32 logits [N, V] (standard normal times `scale`) and valid targets [N]"""
    assert 1 <= N <= MAX_ROWS and V >= 1
    g = torch.Generator().manual_seed(1000 * seed + 7 * V + N)
    logits = torch.randn(N, V, generator=g) * scale
    return logits, torch.randint(0, V, (N,), generator=g)
