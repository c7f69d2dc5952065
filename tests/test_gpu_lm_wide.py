"""GPU (-m gpu): the LM decode engine (csrc/lm_*.hip) at the reference's widths against the oracle run in float64.

Two-layer models at n_embd 1536 (24 / 16 / 12 heads: head_dim 64 / 96 / 128) and 2048 (32 / 16 heads) take the K-sliced GEMV for
every decode projection (K = C and the FC2 input K = 4 C), with the flash-decode merge in the attention projection's prologue, and
the 128- and 256-key attention chunk forms up to 32 chunks.  Vocabularies of 1000 and 8193 rows split unevenly over the head GEMV's
workgroups.  Every stream has a token sequence of its own, so that mixing streams up cannot pass.

The reference is oracle/gpt_oracle.forward on the same fp32 weights cast to float64, run on the GPU (tests/test_oracle_gpt.py pins
it to the reference's golden logits).  Logits of a causal model at position t depend on tokens <= t only, so one forward per stream
gives the expected logits of every prefill position and of every decode step at every cache length.

Bar: LOGIT_TOL = 1e-4 absolute (the suite's).  The logits have a standard deviation of about 2; the fp32 oracle is 2.1e-5 - 2.5e-5
from float64 at C = 1536, masking a single key of 2300 moves a logit by 1.5e-3 and masking a 128-key chunk by more than 1."""
import argparse
import math

import pytest
import torch

from oracle import gpt_oracle as go

pytestmark = pytest.mark.gpu
LOGIT_TOL = 1e-4
N_LAYER = 2
N_STREAM = 16         # the engine's maximum batch
NSTEP = 4             # teacher-forced decode steps per stream and option arm
MAX_ROWS = 65535      # B * T of one prefill call (omnitok_lm_prefill_ex)

# (n_embd, n_head, vocab, block_size): the 8192-token arms only where the float64 scores [H, T, T] stay <= 8.6 GB
MODELS = [(1536, 24, 1000, 4097), (1536, 16, 8193, 8192), (1536, 12, 1000, 8192), (2048, 32, 1000, 4097),
          (2048, 16, 8193, 8192)]

# every lm_* option at a fixed value, so that an arm changes exactly what it names (whatever the process defaults are)
BASE = dict(lm_ksliced=2, lm_ks_deep=0, lm_balance=1, lm_wide_u=2, lm_mfma=0, lm_mfma_mult=1, lm_attn_waves=8)
LM_OPTIONS = tuple(BASE) + ("lm_attn_short",)


def stream_groups(B):
    """the VALU kernels' stream groups (csrc/lm_gemv.hip lm_gemv_any): 8 while 8 are left, then 4, 2, 1"""
    out, b0 = [], 0
    while b0 < B:
        left = B - b0
        n = 8 if left >= 8 else (4 if left >= 4 else (2 if left >= 2 else 1))
        out.append((b0, n))
        b0 += n
    return out


def decode_arms(B, chunk):
    """(name, options) of each arm that selects another kernel for B streams; groups of <= 2 streams ("small") and of 4 or 8
    ("big") take different forms."""
    small = any(n <= 2 for _, n in stream_groups(B))
    big = B >= 4
    arms = [("K-sliced", {}),                                                    # lm_gemv_ks_kernel, merge in its prologue
            ("rows", dict(lm_ksliced=0))]                                        # lm_gemv_kernel for every GEMV
    if chunk == 256:
        arms.append(("attn 4 waves", dict(lm_attn_waves=4)))
    if small:
        arms += [("K-sliced deep", dict(lm_ks_deep=1)),                          # 16 KiB of weights in flight (groups <= 2)
                 ("rows, balance 0", dict(lm_ksliced=0, lm_balance=0)),          # 4 waves instead of 6 (groups <= 2)
                 ("rows, balance 0, wide_u 4", dict(lm_ksliced=0, lm_balance=0, lm_wide_u=4))]
    if big:
        arms += [("K-sliced only for <= 2", dict(lm_ksliced=1)),                 # groups of 4 / 8 on the row kernel
                 ("rows, wide_u 4", dict(lm_ksliced=0, lm_wide_u=4)),            # the wide GEMVs of groups of 4 / 8
                 ("mfma", dict(lm_mfma=1)),                                      # lm_attn_merge_kernel + lm_gemm4_kernel
                 ("mfma, mult 2", dict(lm_mfma=1, lm_mfma_mult=2))]
    return arms


class Options:
    """sets lm_* options and restores what get_option read before"""

    def __init__(self, **opts):
        from omnitokenizer_amd import _lib
        self.lib, self.opts = _lib, opts

    def __enter__(self):
        self.saved = {k: self.lib.get_option(k) for k in LM_OPTIONS}
        for k, v in self.opts.items():
            self.lib.set_option(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            self.lib.set_option(k, v)


class Wide:
    def __init__(self, C, H, V, BS):
        from omnitokenizer_amd.gpt import GPT
        self.C, self.H, self.V, self.BS = C, H, V, BS
        self.name = f"C{C}H{H}V{V}"
        sd = go.synth_gpt_state(V, BS, N_LAYER, H, C, seed=C + H)
        m = GPT(argparse.Namespace(), V, BS, n_layer=N_LAYER, n_head=H, n_embd=C)
        res = m.load_state_dict(sd, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        self.m = m.cuda().eval()
        self.seqs = torch.randint(0, V, (N_STREAM, BS), generator=torch.Generator().manual_seed(C * 100 + H)).cuda()
        sd64 = {k: v.cuda().double() for k, v in sd.items()}
        with torch.no_grad():   # [BS, V] float64 per stream: one causal forward covers every position
            self.ref = [go.forward(sd64, self.seqs[b:b + 1], H)[0] for b in range(N_STREAM)]
        del sd64

    def alloc(self, B, max_len):
        """a fresh cache of exactly max_len tokens: the engine's cache otherwise only grows, and "lm_attn_short" is read when it is
        allocated"""
        self.m._cache_shape = (0, 0)
        self.m.reset_streams(B, max_len)
        assert self.m._cache_shape == (B, max_len)

    def prefill_error(self, B, T):
        """prefill streams 0..B-1 with T tokens of their sequences; max |logits - fp64| over every position"""
        lg = self.m.prefill(self.seqs[:B, :T].contiguous(), want_logits=True)
        return max(err(lg[b], self.ref[b][:T]) for b in range(B))


def err(got, want):
    d = (got.double() - want).abs()
    return float(torch.nan_to_num(d, nan=math.inf).max())


@pytest.fixture(scope="module", params=MODELS, ids=lambda p: f"C{p[0]}H{p[1]}")
def wide(request):
    w = Wide(*request.param)
    yield w
    del w.m, w.ref
    torch.cuda.empty_cache()


ERRORS = {}   # (model, case, arm) -> max error: printed at the end of the module (pytest -s) for the record


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for k, v in sorted(ERRORS.items()):
        print("lm_wide", *k, f"{v:.2e}")


@pytest.mark.parametrize("waves", [8, 4])
@pytest.mark.parametrize("B,T", [(3, 255), (4, 256), (2, 257), (5, 513), (16, 4095), (7, None)])
def test_prefill_vs_fp64(wide, B, T, waves):
    """Teacher-forced logits of every position of a batched prefill (GEMMs + causal chunked attention) against float64: around
    256-key chunk boundaries, at B * T = 65520 rows (16 x 4095) and at the whole block (7 x 8192 or 7 x 4097)."""
    T = T or wide.BS
    assert B * T <= MAX_ROWS
    with Options(lm_attn_waves=waves):
        wide.alloc(B, T)
        e = wide.prefill_error(B, T)
    ERRORS[wide.name, f"prefill B={B} T={T}", f"attn {waves} waves"] = e
    assert e < LOGIT_TOL, f"prefill B={B} T={T}: logits differ from float64 by {e:.2e}"


def ragged_lengths(B, chunk, max_len):
    """Two sets of start lengths L[b] (the cache holds positions < L[b]; the NSTEP steps run at cache lengths L .. L + NSTEP - 1).
    Round 0: spread over the whole cache, one per chunk boundary X (L = X - 2: the key count L + 1 + s passes X at step 2), the
    longest being max_len - NSTEP (the last step writes slot max_len - 1) when one prefill can hold it; interleaved so that every
    group of 8 streams holds short and long caches.  Round 1: the K-sliced merge's register rounds -- 8 chunks for groups of <= 2
    streams, 2 for groups of 4 and 8 -- crossed at every step."""
    lmax = min(max_len - NSTEP, MAX_ROWS // B)
    cand = sorted({1} | {x - 2 for x in range(chunk, lmax + 3, chunk)} | ({max_len - NSTEP} if max_len - NSTEP <= lmax else set()))
    if B == 1:
        picks = [cand[-1]]
    else:
        picks = [cand[round(i * (len(cand) - 1) / (B - 1))] for i in range(B)]
    round0 = picks[0::2] + picks[1::2]
    round1 = []
    for _, n in stream_groups(B):
        for j in range(n):
            round1.append(8 * chunk - 2 + j if n <= 2 else 2 * chunk - 2 - (j % 2) + 4 * (j // 2))
    assert max(round0 + round1) <= lmax
    return [round0, round1]


# cache configurations: (max_len, "lm_attn_short") -> attention chunk; "max" = the model's block size (4097 or 8192)
CACHES = {"128-key chunks": (4096, 1, 128), "256-key chunks": (4096, 0, 256), "block size": (None, 1, 256)}
DECODE_CASES = ([("128-key chunks", B) for B in (1, 2, 3, 4, 5, 8, 9, 13, 16)] + [("256-key chunks", B) for B in (2, 5, 13)]
                + [("block size", B) for B in (1, 2, 3, 5, 8, 9, 13, 16)])


@pytest.mark.parametrize("cache,B", DECODE_CASES)
def test_decode_ragged_lengths_vs_fp64(wide, cache, B):
    """Decode steps of B streams with a different cache length each, under every option arm that changes a kernel for B, against
    the float64 logits of the same positions.  The caches are filled by one prefill (itself checked against float64); each arm
    restarts the streams at the same lengths.  The overflow flag stays clear, also after a step into slot max_len - 1."""
    max_len, short, chunk = CACHES[cache]
    max_len = max_len or wide.BS
    m = wide.m
    rounds = ragged_lengths(B, chunk, max_len)
    T = max(max(r) for r in rounds)
    failures = []
    with Options(lm_attn_short=short, **BASE):
        wide.alloc(B, max_len)
        e = wide.prefill_error(B, T)
        if not e < LOGIT_TOL:
            failures.append(f"prefill T={T}: {e:.2e}")
        for r, lens in enumerate(rounds):
            L = torch.tensor(lens, dtype=torch.int32, device="cuda")
            steps = torch.arange(NSTEP, device="cuda")
            toks = wide.seqs[torch.arange(B, device="cuda")[:, None], L[:, None].long() + steps]          # [B, NSTEP]
            want = [torch.stack([wide.ref[b][lens[b] + s] for b in range(B)]) for s in range(NSTEP)]   # [B, V] per step
            for name, opts in decode_arms(B, chunk):
                with Options(**opts):
                    m._len[:B] = L
                    m._pos[:B] = L
                    errs = [err(m.step(toks[:, s].contiguous()), want[s]) for s in range(NSTEP)]
                    m.check_overflow()
                e = max(errs)
                ERRORS[wide.name, f"decode {cache} max_len={max_len} B={B} round {r}", name] = e
                if not e < LOGIT_TOL:
                    failures.append(f"round {r} lengths {lens}, {name}: per step {['%.2e' % x for x in errs]}")
    assert not failures, f"{wide.name} {cache} B={B}: logits differ from float64 by more than {LOGIT_TOL}:\n" + "\n".join(failures)
