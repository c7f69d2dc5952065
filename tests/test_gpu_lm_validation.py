"""GPU: the LM validation path -- omnitok_lm_token_ce against fp64 torch on the same logits (bars: tests/lm_validation_bounds.py),
its edge cases, omnitok_lm_prefill_loss against prefill(want_logits) + token_ce, GPT.token_losses against the reference's recorded
numbers, Net2NetTransformer.shared_step / validation_step, and the memory the path does not allocate."""
import argparse
import math
import os

import numpy as np
import pytest
import torch

from oracle import gpt_oracle as go
from tests import lm_validation_bounds as lb
from tests.helpers import GOLDEN
from tests.test_oracle_gpt import GPT_CASES, load_gpt_case

pytestmark = pytest.mark.gpu
LOGIT_TOL = lb.LOGIT_TOL


@pytest.fixture(scope="module")
def ll():
    from omnitokenizer_amd import lm_losses
    return lm_losses


class ChunkRows:
    def __init__(self, rows):
        self.rows = rows

    def __enter__(self):
        from omnitokenizer_amd import _lib
        self.before = _lib.get_option("lm_loss_chunk_rows")
        _lib.set_option("lm_loss_chunk_rows", self.rows)

    def __exit__(self, *a):
        from omnitokenizer_amd import _lib
        _lib.set_option("lm_loss_chunk_rows", self.before)


def strided(logits, pad):
    """the same values as a column slice of a buffer `pad` floats wider (rows at every 4-byte alignment)"""
    if pad == 0:
        return logits.contiguous()
    N, V = logits.shape
    buf = torch.full((N, V + pad), float("nan"), device=logits.device)
    buf[:, :V] = logits
    return buf[:, :V]


# ---- the kernel against fp64 torch --------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 30.0])
@pytest.mark.parametrize("V", [1, 5, 63, 257, 1025, 9217])
def test_token_ce_vs_fp64(ll, V, scale):
    for N in (1, 3, 257, 1030):
        cpu_logits, cpu_tg = lb.ce_case(N, V, scale)
        logits, tg = cpu_logits.cuda(), cpu_tg.cuda()
        ref, bar, want_rank = lb.nll64(logits, tg), lb.nll_bar(logits, tg), lb.rank_of_target(logits, tg)
        for pad in (0, 3):
            lg = strided(logits, pad)
            assert lg.stride(0) == V + pad
            out = ll.token_cross_entropy(lg, tg)
            err = (out["nll"].double() - ref).abs()
            r = float(torch.where(bar > 0, err / bar, torch.where(err > 0, torch.full_like(err, math.inf), err)).max())
            print(f"V {V} N {N} ld {V + pad} x{scale:g}: nll err {float(err.max()):.2e} = {r:.3f} of the bar")
            assert r <= 1.0
            assert torch.equal(out["rank"], want_rank)
            loss64 = float(ref.mean())
            assert abs(float(out["loss"]) - loss64) <= lb.loss_bar(bar, tg, loss64)
            assert int(out["count"]) == N
            assert out["acc1"].item() == lb.reference_accuracy((want_rank == 0).sum(), N).item()
            assert out["acc5"].item() == lb.reference_accuracy((want_rank < 5).sum(), N).item()


def test_token_ce_shapes_and_dict(ll):
    logits, tg = lb.ce_case(10, 300, 3.0)
    out = ll.token_cross_entropy(logits.reshape(2, 5, 300).cuda(), tg.reshape(2, 5).cuda())
    assert set(out) == {"loss", "acc1", "acc5", "nll", "rank", "count"}
    assert tuple(out["nll"].shape) == (2, 5) and out["nll"].dtype == torch.float32
    assert tuple(out["rank"].shape) == (2, 5) and out["rank"].dtype == torch.int32
    assert out["loss"].dim() == 0 and out["loss"].dtype == torch.float32 and tuple(out["acc1"].shape) == (1,)
    flat = ll.token_cross_entropy(logits.cuda(), tg.cuda())
    assert torch.equal(flat["nll"], out["nll"].reshape(-1)) and torch.equal(flat["loss"], out["loss"])
    # a transposed view is copied, not misread
    t = ll.token_cross_entropy(logits.t().contiguous().cuda().t(), tg.cuda())
    assert torch.equal(t["nll"], flat["nll"]) and torch.equal(t["rank"], flat["rank"])
    nll, rank, sums = ll.token_ce_sums(logits.cuda(), tg.cuda())
    assert torch.equal(nll, flat["nll"]) and sums.dtype == torch.float64 and float(sums[1]) == 10.0
    assert float(sums[0]) == float(flat["nll"].double().sum()) or abs(float(sums[0]) - float(flat["nll"].double().sum())) < 1e-12


@pytest.mark.parametrize("V", [40, 1500])
def test_ties_rank_lowest_index_first(ll, V):
    """duplicated maxima before and after the target: rank counts the larger entries and the equal ones at a lower index"""
    l = torch.zeros(5, V)
    l[:, [3, 10, 20]] = 5.0
    tg = torch.tensor([3, 10, 20, 0, 30])
    out = ll.token_cross_entropy(l.cuda(), tg.cuda())
    assert out["rank"].tolist() == [0, 1, 2, 3, 3 + 27]
    assert torch.equal(out["rank"], lb.rank_of_target(l.cuda(), tg.cuda()))
    assert out["acc1"].item() == lb.reference_accuracy(1, 5).item() and out["acc5"].item() == lb.reference_accuracy(4, 5).item()
    # a constant row: every entry ties, the target's index is its rank
    c = ll.token_cross_entropy(torch.full((2, V), -2.5).cuda(), torch.tensor([0, V - 1]).cuda())
    assert c["rank"].tolist() == [0, V - 1]
    assert (c["nll"].double().cpu() - math.log(V)).abs().max().item() <= float(lb.nll_bar(torch.full((2, V), -2.5), tg[:2]).max())


@pytest.mark.parametrize("V", [63, 1025])
def test_ignored_invalid_and_repeatable(ll, V):
    N = 300
    cpu_logits, cpu_tg = lb.ce_case(N, V, 4.0, seed=3)
    logits, tg = cpu_logits.cuda(), cpu_tg.cuda()
    full = ll.token_cross_entropy(logits, tg)
    again = ll.token_cross_entropy(logits, tg)
    for k in full:
        assert torch.equal(full[k], again[k]), k                     # two calls: equal bits
    # ignored rows contribute nothing
    ign = tg.clone()
    ign[::3] = -1
    ign[5] = -7
    keep = ign >= 0
    out = ll.token_cross_entropy(logits, ign)
    assert torch.equal(out["nll"][keep], full["nll"][keep]) and torch.equal(out["rank"][keep], full["rank"][keep])
    assert (out["nll"][~keep] == 0).all() and (out["rank"][~keep] == -1).all()
    n = int(keep.sum())
    assert int(out["count"]) == n
    sub = ll.token_cross_entropy(logits[keep], tg[keep])
    assert abs(float(out["loss"]) - float(sub["loss"])) <= 2 * lb.U * abs(float(sub["loss"]))   # another partition of the fp64 sum
    assert torch.equal(out["acc1"], sub["acc1"]) and torch.equal(out["acc5"], sub["acc5"])
    # every row ignored: count 0, NaN loss (torch's mean of nothing)
    none = ll.token_cross_entropy(logits, torch.full_like(tg, -1))
    assert int(none["count"]) == 0 and math.isnan(float(none["loss"])) and math.isnan(none["acc1"].item())
    # an invalid target: NaN and rank V, no fault, the other rows untouched
    bad = tg.clone()
    bad[7], bad[100] = V, V + 12345
    inv = ll.token_cross_entropy(logits, bad)
    torch.cuda.synchronize()
    assert torch.isnan(inv["nll"][[7, 100]]).all() and inv["rank"][[7, 100]].tolist() == [V, V]
    ok = torch.ones(N, dtype=torch.bool, device="cuda")
    ok[[7, 100]] = False
    assert torch.equal(inv["nll"][ok], full["nll"][ok]) and torch.equal(inv["rank"][ok], full["rank"][ok])
    assert math.isnan(float(inv["loss"])) and int(inv["count"]) == N
    hits = full["rank"][ok]
    assert inv["acc1"].item() == lb.reference_accuracy((hits == 0).sum(), N).item()
    assert inv["acc5"].item() == lb.reference_accuracy((hits < 5).sum(), N).item()


# ---- the prefill without the logits tensor ------------------------------------------------------------------------------
LM = dict(V=1100, BS=80, L=1, H=4, C=256)     # V > 1024: the wide-row kernel; 3 x 70 rows: four blocks of 64, three of 100


def synth_gpt(seed=31):
    from omnitokenizer_amd import gpt as og
    sd = go.synth_gpt_state(LM["V"], LM["BS"], LM["L"], LM["H"], LM["C"], seed=seed)
    m = og.GPT(argparse.Namespace(), LM["V"], LM["BS"], n_layer=LM["L"], n_head=LM["H"], n_embd=LM["C"])
    m.load_state_dict(sd, strict=True)
    return m.cuda().eval()


@pytest.fixture(scope="module")
def prefill_case(ll):
    """model, idx, targets [3, 70] (the first two positions of every stream ignored) and, computed once: the logits of
    prefill(want_logits), token_cross_entropy on them, their fp64 nll, bar, and margins"""
    m = synth_gpt()
    g = torch.Generator().manual_seed(41)
    idx = torch.randint(0, LM["V"], (3, 70), generator=g).cuda()
    tg = torch.randint(0, LM["V"], (3, 70), generator=g)
    tg[:, :2] = -1
    tg = tg.cuda()
    m._sync_engine()
    m.reset_streams(3, 70)
    logits = m.prefill(idx, want_logits=True)
    flat, tflat = logits.reshape(-1, LM["V"]), tg.reshape(-1)
    ref = ll.token_cross_entropy(logits, tg)
    l64 = flat.double()
    lt = l64.gather(-1, tflat.clamp(min=0)[:, None])
    top = l64.scatter(-1, tflat.clamp(min=0)[:, None], -math.inf).topk(5, -1).values
    margin = torch.minimum((lt - top[:, :1]).abs(), (lt - top[:, 4:5]).abs()).squeeze(-1)
    return dict(m=m, idx=idx, tg=tg, ref=ref, nll64=lb.nll64(flat, tflat), bar=lb.nll_bar(flat, tflat), margin=margin)


def test_prefill_loss_one_block_is_bit_equal(prefill_case):
    c = prefill_case
    assert 2048 >= c["idx"].numel()
    c["m"].reset_streams(3, 72)     # room for the step below (the cache only grows)
    with ChunkRows(2048):
        out = c["m"].token_losses(c["idx"], c["tg"])
    for k in c["ref"]:
        assert torch.equal(out[k], c["ref"][k]), k
    # ... and it leaves the prefill's cache behind: the next step's logits are the prefill's
    nxt = torch.randint(0, LM["V"], (3,), generator=torch.Generator().manual_seed(42)).cuda()
    after = c["m"].step(nxt)
    c["m"].reset_streams(3, 71)
    c["m"].prefill(c["idx"])
    assert torch.equal(after, c["m"].step(nxt))


@pytest.mark.parametrize("R", [64, 100])
def test_prefill_loss_in_blocks(prefill_case, R):
    c = prefill_case
    with ChunkRows(R):
        out = c["m"].token_losses(c["idx"], c["tg"])
    keep = (c["tg"] >= 0).reshape(-1)
    err = (out["nll"].reshape(-1).double() - c["nll64"]).abs()
    tol = c["bar"] + 2 * LOGIT_TOL
    print(f"R {R}: nll err {float(err.max()):.2e} (bar + 2 LOGIT_TOL >= {float(tol.min()):.2e}); "
          f"rows with a margin below 2 LOGIT_TOL: {int((c['margin'] < 2 * LOGIT_TOL)[keep].sum())}")
    assert (err[keep] <= tol[keep]).all()
    assert (out["nll"].reshape(-1)[~keep] == 0).all() and (out["rank"].reshape(-1)[~keep] == -1).all()
    clear = keep & (c["margin"] >= 2 * LOGIT_TOL)
    assert torch.equal(out["rank"].reshape(-1)[clear], c["ref"]["rank"].reshape(-1)[clear])
    assert int(clear.sum()) >= 0.98 * int(keep.sum())
    assert int(out["count"]) == int(keep.sum())
    if bool((clear == keep).all()):
        assert torch.equal(out["acc1"], c["ref"]["acc1"]) and torch.equal(out["acc5"], c["ref"]["acc5"])
    n = int(keep.sum())
    assert abs(float(out["loss"]) - float(c["nll64"][keep].mean())) <= float(tol[keep].mean()) + lb.U * abs(float(out["loss"]))
    assert n == 3 * 68


def test_prefill_loss_skips_blocks_of_ignored_rows(prefill_case):
    """the first 64 rows (one block at R = 64) all ignored: their GEMM is skipped, their outputs are the ignored row's"""
    c = prefill_case
    tg = c["tg"].clone().reshape(-1)
    tg[:64] = -1
    tg = tg.reshape(3, 70)
    with ChunkRows(64):
        out = c["m"].token_losses(c["idx"], tg)
    nll, rank = out["nll"].reshape(-1), out["rank"].reshape(-1)
    assert (nll[:64] == 0).all() and (rank[:64] == -1).all()
    keep = (tg >= 0).reshape(-1)
    err = (nll.double() - c["nll64"]).abs()
    assert (err[keep] <= (c["bar"] + 2 * LOGIT_TOL)[keep]).all()
    assert int(out["count"]) == int(keep.sum())


def test_token_losses_does_not_hold_the_logits():
    m = synth_gpt(seed=32)          # a fresh engine: the workspace only grows
    g = torch.Generator().manual_seed(43)
    idx = torch.randint(0, LM["V"], (3, 70), generator=g).cuda()
    tg = torch.randint(0, LM["V"], (3, 70), generator=g).cuda()
    logits_bytes = 3 * 70 * LM["V"] * 4
    with ChunkRows(64):
        m._sync_engine()
        m.reset_streams(3, 70)
        assert m.loss_workspace_bytes() == 0
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.max_memory_allocated()
        out = m.token_losses(idx, tg)
        torch.cuda.synchronize()
        grown = torch.cuda.max_memory_allocated() - before
    ws = m.loss_workspace_bytes()
    print(f"torch allocations grew by {grown} B, library workspace {ws} B, logits would be {logits_bytes} B")
    assert grown < logits_bytes // 8
    assert 64 * LM["V"] * 4 <= ws < logits_bytes // 2
    assert math.isfinite(float(out["loss"]))


# ---- the reference's recorded numbers -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GPT_CASES)
def test_token_losses_vs_reference_golden(name):
    from omnitokenizer_amd.gpt import GPT
    g, sd, (V, BS, L, H, C) = load_gpt_case(name)
    v = np.load(os.path.join(GOLDEN, f"lm_validation_{name}.npz"))
    m = GPT(argparse.Namespace(), V, BS, n_layer=L, n_head=H, n_embd=C)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    idx, tg = torch.from_numpy(g["idx"]).cuda(), torch.from_numpy(v["targets"]).cuda()
    out = m.token_losses(idx, tg)
    ref_logits = torch.from_numpy(g["logits"]).reshape(-1, V)
    bar = lb.nll_bar(ref_logits, tg.reshape(-1).cpu())
    nll_ref = torch.from_numpy(v["nll64"]).reshape(-1)
    err = (out["nll"].reshape(-1).double().cpu() - nll_ref).abs()
    assert (err <= bar + 2 * LOGIT_TOL).all()
    lbar = lb.loss_bar(bar, tg.reshape(-1).cpu(), float(v["loss"])) + LOGIT_TOL
    dl = abs(float(out["loss"]) - float(v["loss"]))
    print(f"{name}: loss {float(out['loss']):.6f} vs {float(v['loss']):.6f} (diff {dl:.2e}, bar {lbar:.2e}); nll err {float(err.max()):.2e}")
    assert dl <= lbar
    m1, m5 = torch.from_numpy(v["margin1"]).reshape(-1), torch.from_numpy(v["margin5"]).reshape(-1)
    near = (m1.abs() < 2 * LOGIT_TOL) | (m5.abs() < 2 * LOGIT_TOL)
    n = near.numel()
    assert int(near.sum()) <= 0.02 * n
    rank = out["rank"].reshape(-1).cpu()
    assert torch.equal((rank == 0)[~near], (m1 > 0)[~near]) and torch.equal((rank < 5)[~near], (m5 > 0)[~near])
    if not bool(near.any()):
        assert out["acc1"].item() == float(v["acc1"][0]) and out["acc5"].item() == float(v["acc5"][0])
    assert int(out["count"]) == n


# ---- Net2NetTransformer.shared_step / validation_step -------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_tokenizer():
    from omnitokenizer_amd import OmniTokenizer_VQGAN, make_args, synth
    from omnitokenizer_amd.config import OmniTokConfig
    targs = make_args(2, resolution=64)
    cfg = OmniTokConfig.from_args(targs)
    tok = OmniTokenizer_VQGAN(targs)
    tok.load_state_dict(synth.synth_state_dict(cfg, seed=0), strict=True)
    return tok, cfg


@pytest.mark.parametrize("starts_with_sos,class_first,unconditional",
                         [(False, False, False), (True, False, False), (True, True, False), (False, False, True)])
def test_shared_step_and_validation_step(ll, tiny_tokenizer, starts_with_sos, class_first, unconditional):
    from omnitokenizer_amd import synth
    from omnitokenizer_amd.lm_transformer import Net2NetTransformer
    tok, cfg = tiny_tokenizer
    n_cls, L, H, C = 10, 2, 4, 256
    args = argparse.Namespace(class_cond_dim=None if unconditional else n_cls, unconditional=unconditional, vtokens=False,
                              block_size=80, n_layer=L, n_head=H, n_embd=C, vtokens_pos=False, n_unmasked=0,
                              starts_with_sos=starts_with_sos, class_first=class_first)
    net = Net2NetTransformer(args, first_stage_model=tok, first_stage_key="video", cond_stage_key="label")
    V = net.transformer.vocab_size
    assert V == cfg.n_codes + (0 if unconditional else n_cls) + (1 if starts_with_sos else 0)
    net.load_state_dict({f"transformer.{k}": v for k, v in go.synth_gpt_state(V, 80, L, H, C, seed=6).items()}, strict=True)
    net = net.cuda().eval()
    x = synth.synth_image(2, 64, seed=21).cuda()                   # 8 x 8 = 64 latent tokens
    batch = {"video": x, "label": torch.tensor([3, 7]).cuda()}
    xx, c = net.get_xc(batch)                                      # unconditional: the conditioning key is the video's
    logits, target = net(xx, c)
    want = ll.token_cross_entropy(logits, target)
    flat, tflat = logits.reshape(-1, V), target.reshape(-1)
    bar = lb.loss_bar(lb.nll_bar(flat, tflat), tflat, float(want["loss"]))
    loss, acc1, acc5 = net.shared_step(batch, 0)
    print(f"loss {float(loss):.6f} vs {float(want['loss']):.6f}, bar {bar:.2e}; acc1 {acc1.item():.3f} acc5 {acc5.item():.3f}")
    assert abs(float(loss) - float(want["loss"])) <= bar
    assert torch.equal(acc1, want["acc1"]) and torch.equal(acc5, want["acc5"])
    logged = []
    net.log = lambda name, value, **kw: logged.append((name, value))
    out = net.validation_step(batch, 0)
    assert set(out) == {"val/loss", "val/acc1", "val/acc5"} and [n for n, _ in logged] == ["val/loss", "val/acc1", "val/acc5"]
    assert torch.equal(out["val/loss"], loss) and torch.equal(out["val/acc1"], acc1) and torch.equal(out["val/acc5"], acc5)
    assert all(v is out[n] for n, v in logged)
