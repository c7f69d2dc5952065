"""LM validation numbers on the device: the token cross-entropy and the top-1 / top-5 accuracy of the reference's
`Net2NetTransformer.shared_step` (lm_transformer.py:308-321: F.cross_entropy and utils.accuracy(topk=(1, 5)), utils.py:191-205),
computed by one read of the logits in csrc/lm_loss.hip (include/omnitok_lm.h omnitok_lm_token_ce):

  token_cross_entropy(logits, targets)   {"loss", "acc1", "acc5", "nll", "rank", "count"}
  token_ce_sums(logits, targets)         (nll, rank, sums [4] float64): the raw outputs, omnitok::token_ce

`GPT.token_losses` returns the same dict without ever holding the [B, T, V] logits (omnitok_lm_prefill_loss).

Per row: nll = logsumexp(logits) - logits[target] in fp32; rank = how many entries come before the target in a descending order
with the lowest index first among equals (torch.topk leaves the order of equal values open; this is omnitok_lm_select's argmax
convention).  A target < 0 is an ignored row (nll 0, rank -1, counted nowhere); a target >= V gives nll NaN and rank V and makes
the loss NaN (torch's device assert would end the process instead).  The sums are added in fp64 in a fixed order: two calls
give equal bits.  The operands are only read.  There is no CPU path.
"""
from __future__ import annotations

from typing import Dict, Tuple

import torch

from . import _lib
from ._lib import check
from .losses import _check_fp32, _check_one_gpu, _ptr, _stream

MAX_ROWS = 1 << 31


def _check_ce(logits, targets, what: str):
    _check_fp32(logits, "logits", what)
    if not isinstance(targets, torch.Tensor) or targets.dtype != torch.int64:
        raise TypeError(f"{what}: targets must be an int64 tensor, got {getattr(targets, 'dtype', type(targets).__name__)}")
    if logits.dim() < 1 or logits.shape[-1] < 1:
        raise ValueError(f"{what}: logits must be [..., V] with V >= 1, got {tuple(logits.shape)}")
    if tuple(targets.shape) != tuple(logits.shape[:-1]):
        raise ValueError(f"{what}: targets must be logits.shape[:-1] = {tuple(logits.shape[:-1])}, got {tuple(targets.shape)}")
    if targets.numel() > MAX_ROWS:
        raise ValueError(f"{what}: {targets.numel()} rows, at most {MAX_ROWS}")
    _check_one_gpu(what, logits=logits, targets=targets)


def _rows(logits):
    """[N, V] view with unit column stride and a row stride >= V (a column slice of a wider buffer stays a view)"""
    V = logits.shape[-1]
    lg = logits if logits.dim() == 2 else logits.reshape(-1, V)
    if not ((V == 1 or lg.stride(1) == 1) and (lg.shape[0] <= 1 or lg.stride(0) >= V)):
        lg = lg.contiguous()
    return lg


def _register_ops():
    from torch.library import custom_op

    @custom_op("omnitok::token_ce", mutates_args=(), device_types="cuda")
    def _ce(logits: torch.Tensor, targets: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        _check_ce(logits, targets, "token_ce")
        V = logits.shape[-1]
        N = targets.numel()
        nll = torch.empty(targets.shape, device=logits.device, dtype=torch.float32)
        rank = torch.empty(targets.shape, device=logits.device, dtype=torch.int32)
        sums = torch.zeros(4, device=logits.device, dtype=torch.float64)
        if N == 0:   # torch's mean of nothing: the caller divides 0 by 0
            return nll, rank, sums
        lg, tg = _rows(logits), targets.contiguous()
        ld = lg.stride(0) if N > 1 else V
        lib = _lib.load()
        with torch.cuda.device(logits.device):
            need = lib.omnitok_lm_token_ce_workspace(N)
            work = torch.empty(need, device=logits.device, dtype=torch.uint8)
            check(lib.omnitok_lm_token_ce(_ptr(lg), ld, _ptr(tg), N, V, _ptr(nll), _ptr(rank), _ptr(sums), _ptr(work), need,
                                          _stream()), "token_ce")
        return nll, rank, sums

    @_ce.register_fake
    def _(logits, targets):
        return (logits.new_empty(targets.shape, dtype=torch.float32), logits.new_empty(targets.shape, dtype=torch.int32),
                logits.new_empty((4,), dtype=torch.float64))


_register_ops()


def results(nll: torch.Tensor, rank: torch.Tensor, sums: torch.Tensor) -> Dict[str, torch.Tensor]:
    """The dict of token_cross_entropy from the kernel's outputs (no host synchronisation):
      loss   0-dim fp32: the fp64 sum / count (one correctly rounded fp64 division of two device scalars, as losses.mean_of
             does with a host count), rounded to fp32 once; NaN for count 0 (torch's mean of nothing)
      acc1, acc5   [1] fp32: float32(correct_k) * float32(100.0 / count), the reference's `correct_k.mul_(100.0 / batch_size)`
      count  0-dim int64: the rows that are not ignored."""
    count = sums[1]
    scale = (torch.full((), 100.0, device=sums.device, dtype=torch.float64) / count).to(torch.float32)
    return {"loss": (sums[0] / count).to(torch.float32),
            "acc1": sums[2:3].to(torch.float32) * scale, "acc5": sums[3:4].to(torch.float32) * scale,
            "nll": nll, "rank": rank, "count": count.to(torch.int64)}


def token_ce_sums(logits: torch.Tensor, targets: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(nll fp32, rank int32, both of targets' shape; sums [4] float64 = sum of nll, counted rows, rows with rank 0, rows with
    rank < 5) on the device.  logits fp32 [..., V], targets int64 logits.shape[:-1], one GPU."""
    _check_ce(logits, targets, "token_ce_sums")
    return torch.ops.omnitok.token_ce(logits, targets)


def token_cross_entropy(logits: torch.Tensor, targets: torch.Tensor) -> Dict[str, torch.Tensor]:
    """{"loss", "acc1", "acc5", "nll", "rank", "count"} of fp32 logits [..., V] against int64 targets [...] on one GPU: what the
    reference's shared_step computes with F.cross_entropy(logits.reshape(-1, V), target.reshape(-1)) and
    accuracy(..., topk=(1, 5)), from one read of the logits.  A [N, V] column slice of a wider buffer is read in place."""
    _check_ce(logits, targets, "token_cross_entropy")
    return results(*torch.ops.omnitok.token_ce(logits, targets))
