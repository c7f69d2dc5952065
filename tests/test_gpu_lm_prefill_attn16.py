"""GPU (-m gpu): the tiled prefill attention with bf16 / fp16 operands (omnitok_lm_set_prefill_attention_operands,
GPT.set_prefill_attention_operands): the kernel omnitok_lm_attn_prefill16 on the 16-bit MFMA and the engine's prefill routed through it.

Exact cases pin the operand rounding, the mask and the tiling where the arithmetic is exact; random cases are held to the bar of
tests/lm_prefill_attn16_ref.py against fp64 attention over the rounded operands (derived from the contract, checked on the CPU against a
plain restatement and against broken ones: tests/test_lm_prefill_attn16_ref.py); 16-bit outputs to the rounded ends of that bar;
independence and repeatability to torch.equal; the engine to 3 Y, Y the distance between the CPU restatement in its fp32-tile and
fp64-exact forms (never taken from the code under test)."""
import ctypes

import pytest
import torch

from oracle import gpt_oracle as go
from tests import error_bounds as eb
from tests import lm_prefill_attn16_ref as r16
from tests import lm_prefill_attn_ref as ar
from tests.test_gpu_lm import LOGIT_TOL, rnd
from tests.test_gpu_lm_prefill_attn import between, dmax, make_gpt
from tests.test_oracle_gpt import GPT_CASES, load_gpt_case

pytestmark = pytest.mark.gpu
H = ar.HEADS
FMT = r16.FMT
FMTS = ["bf16", "fp16"]
BAR_FACTOR = 3.0   # of Y, as tests/test_gpu_lm_prefill16.py: roundings that last-bit differences upstream may flip


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def lib():
    from omnitokenizer_amd import _lib
    return _lib.load()


def tiled16(lib, qkv, B, T, hd, op, out_fmt=None, flag=None):
    """omnitok_lm_attn_prefill16 of qkv [B * T, 3C] (device) with operands `op` into a fresh fp32 or 16-bit [B * T, C]"""
    C = H * hd
    assert qkv.shape == (B * T, 3 * C) and qkv.is_cuda and qkv.is_contiguous()
    out = torch.full((B * T, C), float("nan"), device="cuda", dtype=torch.float32 if out_fmt is None else FMT[out_fmt][1])
    rc = lib.omnitok_lm_attn_prefill16(_p(qkv), B, T, H, hd, FMT[op][0], _p(out) if out_fmt is None else None,
                                       None if out_fmt is None else _p(out), 0 if out_fmt is None else FMT[out_fmt][0], _p(flag),
                                       torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.omnitok_last_error()
    return out


# ---- 1: exact cases --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", FMTS)
@pytest.mark.parametrize("hd", ar.HDS)
def test_single_key_rows_are_rounded_v_bit_for_bit(lib, hd, op):
    """One key: p = l = 1 exactly, so the row is V as the kernel rounded it -- torch's .to(fmt), bit for bit."""
    C = H * hd
    one = rnd(1, 3 * C, seed=3).cuda()                                    # T = 1
    assert torch.equal(tiled16(lib, one, 1, 1, hd, op), one[:, 2 * C:].to(FMT[op][1]).float())
    B, T = 3, 70                                                          # row 0 of every stream
    qkv = ar.case("rnd_3x70", hd)["qkv"].cuda()
    out = tiled16(lib, qkv, B, T, hd, op).view(B, T, C)
    assert torch.equal(out[:, 0], qkv.view(B, T, 3 * C)[:, 0, 2 * C:].to(FMT[op][1]).float())


@pytest.mark.parametrize("op", FMTS)
@pytest.mark.parametrize("T", [31, 32, 33, 129, 257])
@pytest.mark.parametrize("hd", ar.HDS)
def test_zero_queries_give_exact_prefix_means(lib, hd, T, op):
    """q = 0: every score is 0, every weight 1 (exact in both formats), l = t + 1 and O the exact sum of small integers (exact in both
    formats): out[t] is one fp32 division, torch's.  A key too many or too few at any tile or block edge changes the sum."""
    B, C = 2, H * hd
    g = torch.Generator().manual_seed(7 + T)
    qkv = torch.zeros(B, T, 3, C)
    qkv[:, :, 1] = rnd(B, T, C, seed=T)                                   # keys: anything finite
    qkv[:, :, 2] = torch.randint(-8, 9, (B, T, C), generator=g).float()
    want = qkv[:, :, 2].cumsum(1) / torch.arange(1, T + 1, dtype=torch.float32)[None, :, None]
    out = tiled16(lib, qkv.view(B * T, 3 * C).cuda(), B, T, hd, op)
    assert torch.equal(out.cpu().view(B, T, C), want)


# ---- 2: against fp64 within the derived bar -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", FMTS)
@pytest.mark.parametrize("hd", ar.HDS)
@pytest.mark.parametrize("name", list(ar.CASES))
def test_against_fp64(lib, name, hd, op):
    c = r16.case(name, hd, op)
    out = tiled16(lib, c["qkv"].cuda(), c["B"], c["T"], hd, op).cpu().double()
    err = (out - c["out64"]).abs()
    r = eb.ratio(err, c["bar"])
    print(f"{name} hd {hd} {op}: worst err / bar {r:.4f}; max |out - fp64| {float(err.max()):.2e}")
    assert r <= 1.0


# ---- 3: 16-bit output and the flags ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_fmt", FMTS)
@pytest.mark.parametrize("op", FMTS)
@pytest.mark.parametrize("hd", ar.HDS)
def test_16bit_output(lib, hd, op, out_fmt):
    c = r16.case("rnd_2x300", hd, op)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    y16 = tiled16(lib, c["qkv"].cuda(), c["B"], c["T"], hd, op, out_fmt, flag)
    assert between(y16, c["out64"] - c["bar"], c["out64"] + c["bar"], FMT[out_fmt][1])
    assert int(flag.item()) == 0
    assert torch.equal(tiled16(lib, c["qkv"].cuda(), c["B"], c["T"], hd, op, out_fmt, None), y16)        # flag may be NULL


@pytest.mark.parametrize("hd", ar.HDS)
def test_fp16_operand_and_output_overflows_are_flagged_apart_and_bf16_never(lib, hd):
    B, T, C = 1, 40, H * hd

    def flag_of(qkv, op, out_fmt):
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        out = tiled16(lib, qkv.cuda(), B, T, hd, op, out_fmt, flag)
        return int(flag.item()), out

    base = rnd(B * T, 3 * C, seed=5)
    k_big = base.clone()
    k_big[:, C + 3] = 7.0e4                                               # one K column beyond fp16's 65504
    assert flag_of(k_big, "fp16", None)[0] == 8
    got, out = flag_of(k_big, "bf16", None)
    assert got == 0 and torch.isfinite(out).all()
    v_big = base.clone()
    v_big[:, 2 * C + 3] = 7.0e4                                           # one V column: every mean of it is 7.0e4
    assert flag_of(v_big, "fp16", None)[0] == 8                           # the operand
    got, out = flag_of(v_big, "bf16", "fp16")                             # a finite bf16 operand, an fp16 output of inf: bit 4 alone
    assert got == 4 and bool(torch.isinf(out[:, 3].float()).all())
    assert flag_of(v_big, "fp16", "fp16")[0] == 12                        # both
    got, out = flag_of(v_big, "bf16", "bf16")
    assert got == 0 and torch.isfinite(out.float()).all()
    q_big = base.clone()
    q_big[:, 3] = -7.0e4                                                  # ... and a Q column
    assert flag_of(q_big, "fp16", None)[0] == 8 and flag_of(q_big, "bf16", None)[0] == 0


# ---- 4: independence ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", FMTS)
@pytest.mark.parametrize("others", ["random", "nan"])
@pytest.mark.parametrize("hd", ar.HDS)
def test_a_stream_does_not_depend_on_the_batch(lib, hd, others, op):
    C = H * hd
    mine = rnd(100, 3 * C, seed=21)                                       # the stream: 100 rows, the first 70 of them alone below
    batch = rnd(3, 100, 3 * C, seed=22) if others == "random" else torch.full((3, 100, 3 * C), float("nan"))
    batch[1] = mine
    alone = tiled16(lib, mine[:70].contiguous().cuda(), 1, 70, hd, op)
    full = tiled16(lib, batch.view(300, 3 * C).cuda(), 3, 100, hd, op)
    assert torch.isfinite(alone).all()
    assert torch.equal(full.view(3, 100, C)[1, :70], alone)
    assert torch.equal(tiled16(lib, batch.view(300, 3 * C).cuda(), 3, 100, hd, op).view(3, 100, C)[1], full.view(3, 100, C)[1])   # two calls
    if others == "nan":
        assert torch.isnan(full.view(3, 100, C)[[0, 2]]).all()


# ---- 5: the engine on the golden models -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", FMTS)
@pytest.mark.parametrize("name", GPT_CASES)
def test_engine_fp32_weights_16bit_operands_vs_restatement(name, op):
    """3 streams x min(BS, 40) tokens, fp32 weights + tiled + operands `op`: the forward within 3 Y of the fp64 restatement; the switch
    is live and goes back to the tiled fp32 engine's bits; a prefill of the first T - 3 tokens gives the forward's rows, and the three
    decode steps after it (fp32 arithmetic over a cache the prefill filled) stay within LOGIT_TOL + 3 Y of the oracle."""
    from omnitokenizer_amd import _lib
    g, sd, dims = load_gpt_case(name)
    V, BS, L, Hh, C = dims
    T = min(BS, 40)
    idx = torch.randint(0, V, (3, T), generator=torch.Generator().manual_seed(11))
    l64, Y = r16.engine_reference(sd, idx, Hh, op)
    oracle = go.forward(sd, idx, Hh)
    idx = idx.cuda()
    fp32_tiled, _ = make_gpt(sd, dims, attention="tiled")(idx)            # a fresh tiled engine, fp32 operands
    m = make_gpt(sd, dims, attention="tiled").set_prefill_attention_operands(op)
    logits, _ = m(idx)
    assert m.prefill_attention_operands == op
    assert _lib.load().omnitok_lm_prefill_attention_operands(m._engine) == FMT[op][0]
    e = dmax(logits, l64)
    m.reset_streams(3, T)
    pre = m.prefill(idx[:, :T - 3].contiguous(), want_logits=True)
    e_steps = [dmax(m.step(idx[:, T - 3 + i].contiguous()), oracle[:, T - 3 + i]) for i in range(3)]
    m.check_overflow()
    print(f"{name} {op}: forward vs the fp64 restatement e = {e:.3e}, Y = {Y:.3e}, e / Y = {e / Y:.2f} (bar {BAR_FACTOR}); 3 steps after a "
          f"prefill vs the oracle {max(e_steps):.2e}; |16-bit operands - fp32 operands| {dmax(logits, fp32_tiled):.2e}")
    assert torch.isfinite(logits).all() and e <= BAR_FACTOR * Y
    assert not torch.equal(logits, fp32_tiled)                            # the switch is live
    assert torch.equal(pre, logits[:, :T - 3])                            # a row does not depend on how many rows follow it
    assert max(e_steps) <= LOGIT_TOL + BAR_FACTOR * Y
    back, _ = m.set_prefill_attention_operands("fp32")(idx)               # ... and goes back
    assert torch.equal(back, fp32_tiled)


def test_engine_w16_prefill_with_bf16_operands_vs_restatement():
    """bf16 weights + w16 + tiled + bf16 operands on gpt_hd96, against the restatement with the roundings of both."""
    g, sd, dims = load_gpt_case("gpt_hd96")
    V, BS, L, Hh, C = dims
    T = min(BS, 40)
    idx = torch.randint(0, V, (3, T), generator=torch.Generator().manual_seed(11))
    l64, Y = r16.engine_reference(sd, idx, Hh, "bf16", wfmt="bf16")
    idx = idx.cuda()
    w16_tiled, _ = make_gpt(sd, dims, "bf16", "w16", "tiled")(idx)
    m = make_gpt(sd, dims, "bf16", "w16", "tiled").set_prefill_attention_operands("bf16")
    logits, _ = m(idx)
    m.check_overflow()
    e = dmax(logits, l64)
    print(f"gpt_hd96 bf16 weights + w16 + bf16 operands: e = {e:.3e}, Y = {Y:.3e}, e / Y = {e / Y:.2f} (bar {BAR_FACTOR})")
    assert torch.isfinite(logits).all() and e <= BAR_FACTOR * Y
    assert not torch.equal(logits, w16_tiled)
    back, _ = m.set_prefill_attention_operands("fp32")(idx)
    assert torch.equal(back, w16_tiled)


def test_engine_16bit_operands_need_the_tiled_attention():
    g, sd, dims = load_gpt_case("gpt_hd64")
    V, BS = dims[0], dims[1]
    T = min(BS, 40)
    idx = torch.randint(0, V, (3, T), generator=torch.Generator().manual_seed(11)).cuda()
    m = make_gpt(sd, dims, attention="rows").set_prefill_attention_operands("bf16")
    m.reset_streams(3, T)
    with pytest.raises(RuntimeError) as ei:
        m.prefill(idx, want_logits=True)
    assert "set_prefill_attention_operands" in str(ei.value) and "omnitok_lm_set_prefill_attention to" in str(ei.value)
    m.set_prefill_attention("tiled")
    m.reset_streams(3, T)
    assert torch.isfinite(m.prefill(idx, want_logits=True)).all()
    m.check_overflow()
