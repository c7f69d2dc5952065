"""Validation losses on the device: the sums behind the reference's VQGAN.forward(x) and validation_step
(omnitokenizer.py:388-394, 372-377, 608-618; INTEGRATION.md "validation losses"), each one read of its operands in
csrc/losses.hip (include/omnitok.h "validation losses"):

  reconstruction_losses(x, x_recon)   {"l1", "mse", "logits_laplace"}: per-item means [B] float64 of |x_recon - x|,
                                      (x_recon - x)^2 and the logit-Laplace distance (eps = 0.1)
  recon_sums(x, x_recon, flags)       (sums [B, 3], total [3]) float64: the raw sums, omnitok::recon_losses
  commitment_sum(z, ids, codebook)    [1] float64: sum (z - codebook[ids])^2, the row gathered in the kernel,
                                      omnitok::commitment_sum
  kl_sums(moments)                    (sums [B], total [1]) float64: sum mu^2 + exp(lv) - 1 - lv, lv = clamp(logvar, -30, 20),
                                      omnitok::kl_sum

Every summand is formed in fp32 exactly as torch's fp32 ops form it and accumulated in fp64 in a fixed order: two calls
give equal bits, and a mean over 10^8 elements does not lose its tail.  The operands are only read.  There is no CPU path.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Tuple

import torch

from . import _lib
from ._lib import check

FLAG_L1, FLAG_MSE, FLAG_LAPLACE = 1, 2, 4          # OMNITOK_LOSS_*
FLAG_ALL = FLAG_L1 | FLAG_MSE | FLAG_LAPLACE
MAX_BATCH = 65535


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _work(lib, B: int, device, what: str):
    need = lib.omnitok_losses_workspace(B)
    if need < 0:
        raise ValueError(f"{what}: batch of {B} items, expected 1 .. {MAX_BATCH}")
    return torch.empty(need, device=device, dtype=torch.uint8), need


def _check_fp32(t, name: str, what: str):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: {name} must be a tensor, got {type(t).__name__}")
    if t.dtype != torch.float32:
        raise TypeError(f"{what}: {name}: dtype {t.dtype}, expected torch.float32")


def _check_one_gpu(what: str, **tensors):
    """after the shape checks: every operand on the same GPU"""
    devs = {name: t.device for name, t in tensors.items()}
    if len(set(devs.values())) > 1:
        raise RuntimeError(f"{what}: " + ", ".join(f"{k} on {v}" for k, v in devs.items()) + ": all must be on one GPU")
    for name, d in devs.items():
        if d.type != "cuda":
            raise RuntimeError(f"{what}: {name} is on {d}: the losses run on the GPU (there is no CPU path)")


def _check_pair(x, x_recon, what: str):
    _check_fp32(x, "x", what)
    _check_fp32(x_recon, "x_recon", what)
    if x.shape != x_recon.shape:
        raise ValueError(f"{what}: x and x_recon differ in shape: {tuple(x.shape)} vs {tuple(x_recon.shape)}")
    if x.dim() < 1:
        raise ValueError(f"{what}: x must be [B, ...], got a 0-dim tensor")
    if x.shape[0] > MAX_BATCH:
        raise ValueError(f"{what}: batch of {x.shape[0]} items, at most {MAX_BATCH}")
    _check_one_gpu(what, x=x, x_recon=x_recon)


def _register_ops():
    from torch.library import custom_op

    @custom_op("omnitok::recon_losses", mutates_args=(), device_types="cuda")
    def _recon(x: torch.Tensor, x_recon: torch.Tensor, flags: int) -> Tuple[torch.Tensor, torch.Tensor]:
        _check_pair(x, x_recon, "recon_losses")
        if flags < 1 or flags & ~FLAG_ALL:
            raise ValueError(f"recon_losses: flags 0x{flags:x}")
        B = x.shape[0]
        n = x[0].numel() if B else 0
        sums = torch.empty((B, 3), device=x.device, dtype=torch.float64)
        total = torch.empty(3, device=x.device, dtype=torch.float64)
        if B == 0 or n == 0:   # torch's mean of nothing
            return sums.fill_(0.0), total.fill_(0.0)
        x, x_recon = x.contiguous(), x_recon.contiguous()
        lib = _lib.load()
        with torch.cuda.device(x.device):
            work, need = _work(lib, B, x.device, "recon_losses")
            check(lib.omnitok_recon_losses(_ptr(x), _ptr(x_recon), B, n, flags, _ptr(sums), _ptr(total), _ptr(work), need,
                                           _stream()), "recon_losses")
        return sums, total

    @_recon.register_fake
    def _(x, x_recon, flags):
        return x.new_empty((x.shape[0], 3), dtype=torch.float64), x.new_empty((3,), dtype=torch.float64)

    @custom_op("omnitok::commitment_sum", mutates_args=(), device_types="cuda")
    def _commit(z: torch.Tensor, ids: torch.Tensor, codebook: torch.Tensor) -> torch.Tensor:
        _check_commitment(z, ids, codebook)
        out = torch.zeros(1, device=z.device, dtype=torch.float64)
        if ids.numel() == 0:
            return out
        z, ids, codebook = z.contiguous(), ids.contiguous(), codebook.contiguous()
        lib = _lib.load()
        with torch.cuda.device(z.device):
            work, need = _work(lib, 1, z.device, "commitment_sum")
            check(lib.omnitok_commitment_sum(_ptr(z), _ptr(ids), _ptr(codebook), ids.numel(), codebook.shape[1],
                                             codebook.shape[0], _ptr(out), _ptr(work), need, _stream()), "commitment_sum")
        return out

    @_commit.register_fake
    def _(z, ids, codebook):
        return z.new_empty((1,), dtype=torch.float64)

    @custom_op("omnitok::kl_sum", mutates_args=(), device_types="cuda")
    def _kl(moments: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        _check_moments(moments)
        B = moments.shape[0]
        sums = torch.zeros(B, device=moments.device, dtype=torch.float64)
        total = torch.zeros(1, device=moments.device, dtype=torch.float64)
        m = moments[0].numel() // 2 if B else 0
        if B == 0 or m == 0:
            return sums, total
        moments = moments.contiguous()
        lib = _lib.load()
        with torch.cuda.device(moments.device):
            work, need = _work(lib, B, moments.device, "kl_sum")
            check(lib.omnitok_kl_sum(_ptr(moments), B, m, _ptr(sums), _ptr(total), _ptr(work), need, _stream()), "kl_sum")
        return sums, total

    @_kl.register_fake
    def _(moments):
        return moments.new_empty((moments.shape[0],), dtype=torch.float64), moments.new_empty((1,), dtype=torch.float64)


def _check_commitment(z, ids, codebook):
    what = "commitment_sum"
    _check_fp32(z, "z", what)
    _check_fp32(codebook, "codebook", what)
    if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int64:
        raise TypeError(f"{what}: ids must be an int64 tensor, got {getattr(ids, 'dtype', type(ids).__name__)}")
    if codebook.dim() != 2:
        raise ValueError(f"{what}: codebook must be [n_codes, c], got {tuple(codebook.shape)}")
    if z.dim() < 1 or z.shape[-1] != codebook.shape[1] or tuple(z.shape[:-1]) != tuple(ids.shape):
        raise ValueError(f"{what}: z must be ids.shape + (c,) = {tuple(ids.shape) + (codebook.shape[1],)} (channel-last, "
                         f"what encode(return_latents=True) returns), got {tuple(z.shape)}")
    _check_one_gpu(what, z=z, ids=ids, codebook=codebook)


def _check_moments(moments):
    what = "kl_sum"
    _check_fp32(moments, "moments", what)
    if moments.dim() < 2 or moments.shape[1] % 2:
        raise ValueError(f"{what}: moments must be [B, 2c, ...] (mean | logvar along dim 1), got {tuple(moments.shape)}")
    if moments.shape[0] > MAX_BATCH:
        raise ValueError(f"{what}: batch of {moments.shape[0]} items, at most {MAX_BATCH}")
    _check_one_gpu(what, moments=moments)


_register_ops()


def mean_of(total: torch.Tensor, n: int) -> torch.Tensor:
    """total / n as ONE correctly rounded fp64 division (a tensor divided by a Python scalar is multiplied by the rounded
    reciprocal on the device); NaN for n = 0, torch's mean of nothing"""
    return total / torch.full((), float(n) if n else float("nan"), device=total.device, dtype=torch.float64)


def recon_sums(x: torch.Tensor, x_recon: torch.Tensor, flags: int = FLAG_ALL) -> Tuple[torch.Tensor, torch.Tensor]:
    """(sums [B, 3], total [3]) float64 on the device: per item sum |d|, sum d^2, sum of the logit-Laplace distance
    (d = x_recon - x; a column not in `flags` is 0), and their index-ordered batch totals.  x, x_recon: fp32, equal shape
    [B, ...], one GPU."""
    if not isinstance(flags, int) or flags < 1 or flags & ~FLAG_ALL:
        raise ValueError(f"recon_sums: flags {flags!r}, expected a combination of FLAG_L1 | FLAG_MSE | FLAG_LAPLACE")
    _check_pair(x, x_recon, "recon_sums")
    return torch.ops.omnitok.recon_losses(x, x_recon, flags)


def reconstruction_losses(x: torch.Tensor, x_recon: torch.Tensor) -> Dict[str, torch.Tensor]:
    """{"l1", "mse", "logits_laplace"}: each [B] float64 on the device, the per-item means of the three reconstruction
    losses of the reference (F.l1_loss, F.mse_loss and logits_laplace of omnitokenizer.py:23-30 on one item).  x, x_recon:
    fp32 [B, ...] of equal shape on one GPU, in the model's [-0.5, 0.5] convention; neither is modified (the reference's
    logits_laplace shifts its arguments in place)."""
    _check_pair(x, x_recon, "reconstruction_losses")
    sums, _ = torch.ops.omnitok.recon_losses(x, x_recon, FLAG_ALL)
    n = x[0].numel() if x.shape[0] else 0
    means = mean_of(sums, n)
    return {"l1": means[:, 0], "mse": means[:, 1], "logits_laplace": means[:, 2]}


def commitment_sum(z: torch.Tensor, ids: torch.Tensor, codebook: torch.Tensor) -> torch.Tensor:
    """[1] float64: sum over tokens and channels of (z - codebook[ids])^2.  z: fp32 ids.shape + (c,) (the channel-last latents
    of encode(return_latents=True)), ids int64, codebook fp32 [n_codes, c].  Codebook.forward's commitment_loss is
    0.25 * this / z.numel()."""
    _check_commitment(z, ids, codebook)
    return torch.ops.omnitok.commitment_sum(z, ids, codebook)


def kl_sums(moments: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(sums [B], total [1]) float64: per item the sum of mu^2 + exp(lv) - 1 - lv over the posterior's elements, lv =
    clamp(logvar, -30, 20), and the batch total.  moments: fp32 [B, 2c, ...], what encode(return_moments=True) returns.
    The reference's kl_loss is 0.5 * total / B * kl_weight."""
    _check_moments(moments)
    return torch.ops.omnitok.kl_sum(moments)
