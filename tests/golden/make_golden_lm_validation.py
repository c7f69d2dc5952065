"""Generates tests/golden/lm_validation_<case>.npz: the LM validation numbers of the reference on the gpt_hd64 / gpt_hd96 /
gpt_hd128 cases of make_golden.py (same seeded weights, same idx).

Run in the build container only:   python tests/golden/make_golden_lm_validation.py

What is the reference's and what is ours.  The reference's `Net2NetTransformer` is a Lightning module and does not import here
(no pytorch_lightning), so its `shared_step` (lm_transformer.py:308-321) is pinned as the arithmetic it performs on the GPT's
logits: the logits come from the reference's own `GPT` class (OmniTokenizer/modules/gpt.py, imported unmodified), the loss from
`F.cross_entropy(logits.reshape(-1, V), target.reshape(-1))` and the accuracies from the reference's own `accuracy`
(OmniTokenizer/utils.py:191-205, imported unmodified under the harness's stubs; the generator fails if it does not import).  The
token sequence that a
Net2NetTransformer would build is built by our mirror in the tests (tests/test_gpu_lm_validation.py), not recorded here.

Targets: seeded, one third of the rows each the top-1 entry, an entry of rank 2..5 and an entry of rank > 5 (so acc1 < acc5 <
100).  The seed of a case is the first one for which no row has a margin below MIN_MARGIN (the tests exclude such rows from
the accuracy comparison and cap their share at 2 %: with 32 rows that means none).

Stored per case (data only):
  targets [B, T] int64, target_seed
  loss, acc1, acc5          fp32, as the reference computes them
  nll64 [B, T]              float64 logsumexp(l) - l_t of the reference's fp32 logits
  margin1, margin5 [B, T]   float64: l_t minus the largest / the 5th-largest logit other than the target's
"""
import argparse
import importlib
import os
import sys
import warnings

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
warnings.filterwarnings("ignore")

from oracle import gpt_oracle as go  # noqa: E402
from oracle import ref_harness as rh  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
CASES = ("gpt_hd64", "gpt_hd96", "gpt_hd128")
MIN_MARGIN = 1e-3     # five times the 2 * LOGIT_TOL below which the GPU tests exclude a row


def pick_targets(logits, seed):
    """[B, T] targets by rank class: row r takes class (r + seed) % 3 -- 0: the top-1 entry, 1: rank 2..5, 2: rank > 5"""
    B, T, V = logits.shape
    order = logits.reshape(-1, V).argsort(dim=-1, descending=True, stable=True)
    rng = np.random.default_rng(seed)
    tg = np.empty(B * T, dtype=np.int64)
    for r in range(B * T):
        cls = (r + seed) % 3
        k = 0 if cls == 0 else int(rng.integers(1, 5)) if cls == 1 else int(rng.integers(5, V))
        tg[r] = int(order[r, k])
    return torch.from_numpy(tg).reshape(B, T)


def margins(logits, targets):
    l64 = logits.double()
    lt = l64.gather(-1, targets[..., None])
    others = l64.scatter(-1, targets[..., None], -float("inf"))
    top = others.topk(5, -1).values
    return (lt - top[..., :1]).squeeze(-1), (lt - top[..., 4:5]).squeeze(-1)


def main():
    rh.install_stubs()
    gpt = importlib.import_module("OmniTokenizer.modules.gpt")
    accuracy = importlib.import_module("OmniTokenizer.utils").accuracy
    for name in CASES:
        g = np.load(os.path.join(OUT, name + ".npz"))
        V, BS, L, H, C = (int(g[k]) for k in ("vocab", "block_size", "n_layer", "n_head", "n_embd"))
        sd = go.synth_gpt_state(V, BS, L, H, C, seed=int(g["weight_seed"]))
        m = gpt.GPT(argparse.Namespace(), V, BS, n_layer=L, n_head=H, n_embd=C).eval()
        m.load_state_dict(sd, strict=False)
        idx = torch.from_numpy(g["idx"])
        with torch.no_grad():
            logits, _ = m(idx)
        assert np.array_equal(logits.numpy(), g["logits"]), "the reference's logits differ from gpt_*.npz"
        for seed in range(100):
            tg = pick_targets(logits, seed)
            m1, m5 = margins(logits, tg)
            if min(m1.abs().min().item(), m5.abs().min().item()) >= MIN_MARGIN:
                break
        else:
            raise RuntimeError(f"{name}: no target seed with all margins >= {MIN_MARGIN}")
        flat, tflat = logits.reshape(-1, V), tg.reshape(-1)
        loss = F.cross_entropy(flat, tflat)
        acc1, acc5 = accuracy(flat, tflat, topk=(1, 5))
        nll64 = torch.logsumexp(logits.double(), -1) - logits.double().gather(-1, tg[..., None]).squeeze(-1)
        np.savez_compressed(os.path.join(OUT, f"lm_validation_{name}.npz"), case=name, targets=tg.numpy(), target_seed=seed,
                            loss=loss.numpy(), acc1=acc1.numpy(), acc5=acc5.numpy(), nll64=nll64.numpy(),
                            margin1=m1.numpy(), margin5=m5.numpy())
        print(f"{name}: seed {seed} loss {loss.item():.6f} acc1 {acc1.item():.3f} acc5 {acc5.item():.3f} "
              f"min |margin| {min(m1.abs().min().item(), m5.abs().min().item()):.2e}")


if __name__ == "__main__":
    main()
