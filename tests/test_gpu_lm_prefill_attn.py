"""GPU (-m gpu): the opt-in tiled prefill attention (omnitok_lm_set_prefill_attention, GPT.set_prefill_attention("tiled")): the kernel
omnitok_lm_attn_prefill on the fp32-input MFMA and the engine's prefill routed through it.

Exact cases pin the mask and the tiling where the arithmetic is exact; random cases are held to the bar of tests/lm_prefill_attn_ref.py
against fp64 (derived from the contract, checked on the CPU against a plain fp32 restatement: tests/test_lm_prefill_attn_ref.py);
16-bit outputs to the rounded ends of that bar; independence and repeatability to torch.equal; the engine to the bars the rows mode
is held to (1e-4 against the oracle in fp32, 3 d_ref of tests/lm_prefill16_ref.py under the 16-bit prefill format).
"""
import argparse
import ctypes
import math

import pytest
import torch

from oracle import gpt_oracle as go
from tests import error_bounds as eb
from tests import lm_prefill16_ref as pr
from tests import lm_prefill_attn_ref as ar
from tests.test_gpu_lm import LOGIT_TOL, rnd
from tests.test_oracle_gpt import GPT_CASES, load_gpt_case

pytestmark = pytest.mark.gpu
H = ar.HEADS
FMT = pr.FMT
FMTS = ["bf16", "fp16"]
BAR_FACTOR = 3.0   # of d_ref, as tests/test_gpu_lm_prefill16.py


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def lib():
    from omnitokenizer_amd import _lib
    return _lib.load()


def tiled(lib, qkv, B, T, hd, fmt=None, flag=None):
    """omnitok_lm_attn_prefill of qkv [B * T, 3C] (device) into a fresh fp32 or 16-bit [B * T, C]"""
    C = H * hd
    assert qkv.shape == (B * T, 3 * C) and qkv.is_cuda and qkv.is_contiguous()
    out = torch.full((B * T, C), float("nan"), device="cuda", dtype=torch.float32 if fmt is None else FMT[fmt][1])
    rc = lib.omnitok_lm_attn_prefill(_p(qkv), B, T, H, hd, _p(out) if fmt is None else None, None if fmt is None else _p(out),
                                     0 if fmt is None else FMT[fmt][0], _p(flag), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.omnitok_last_error()
    return out


def rows_path(lib, qkv, B, T, hd):
    """The rows mode's arithmetic from its exported building block: T decode steps of omnitok_lm_attn_decode over an fp32 cache
    (step t appends row t of every stream and attends to keys 0 .. t)."""
    C = H * hd
    steps = qkv.view(B, T, 3 * C).transpose(0, 1).contiguous()            # [T, B, 3C]
    lens = torch.arange(T, dtype=torch.int32, device="cuda")[:, None].expand(T, B).contiguous()
    kc = torch.zeros(B, H, T, hd, device="cuda")
    vc = torch.zeros(B, H, T, hd, device="cuda")
    scratch = torch.empty(B * H * ((T + 255) // 256) * (2 + hd), device="cuda")
    out = torch.empty(T, B, C, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    for t in range(T):
        rc = lib.omnitok_lm_attn_decode(_p(steps[t]), _p(kc), _p(vc), _p(lens[t]), B, H, hd, T, _p(scratch), _p(out[t]), s)
        assert rc == 0, lib.omnitok_last_error()
    return out.transpose(0, 1).reshape(B * T, C)


# ---- 1: exact cases --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd", ar.HDS)
def test_single_key_rows_are_v_bit_for_bit(lib, hd):
    C = H * hd
    one = rnd(1, 3 * C, seed=3).cuda()                                    # T = 1
    assert torch.equal(tiled(lib, one, 1, 1, hd), one[:, 2 * C:])
    B, T = 3, 70                                                          # row 0 of every stream
    qkv = ar.case("rnd_3x70", hd)["qkv"].cuda()
    out = tiled(lib, qkv, B, T, hd).view(B, T, C)
    assert torch.equal(out[:, 0], qkv.view(B, T, 3 * C)[:, 0, 2 * C:])


@pytest.mark.parametrize("T", [31, 32, 33, 129, 257])
@pytest.mark.parametrize("hd", ar.HDS)
def test_zero_queries_give_exact_prefix_means(lib, hd, T):
    """q = 0: every score is 0, every weight expf(0) = 1, l = t + 1 and O the exact sum of small integers: out[t] is one fp32 division,
    torch's.  A key too many or too few at any tile or block edge changes the sum."""
    B, C = 2, H * hd
    g = torch.Generator().manual_seed(7 + T)
    qkv = torch.zeros(B, T, 3, C)
    qkv[:, :, 1] = rnd(B, T, C, seed=T)                                   # keys: anything finite
    qkv[:, :, 2] = torch.randint(-8, 9, (B, T, C), generator=g).float()
    want = qkv[:, :, 2].cumsum(1) / torch.arange(1, T + 1, dtype=torch.float32)[None, :, None]
    out = tiled(lib, qkv.view(B * T, 3 * C).cuda(), B, T, hd)
    assert torch.equal(out.cpu().view(B, T, C), want)


# ---- 2: against fp64 within the derived bar, and the rows path within the sum of both ---------------------------------------------------
@pytest.mark.parametrize("hd", ar.HDS)
@pytest.mark.parametrize("name", list(ar.CASES))
def test_against_fp64_and_the_rows_path(lib, name, hd):
    c = ar.case(name, hd)
    B, T = c["B"], c["T"]
    qkv = c["qkv"].cuda()
    out = tiled(lib, qkv, B, T, hd).cpu().double()
    rows = rows_path(lib, qkv, B, T, hd).cpu().double()
    r_t = eb.ratio((out - c["out64"]).abs(), c["bar"])
    r_r = eb.ratio((rows - c["out64"]).abs(), c["bar_rows"])
    r_b = eb.ratio((out - rows).abs(), c["bar"] + c["bar_rows"])
    print(f"{name} hd {hd}: worst err / bar: tiled vs fp64 {r_t:.4f}, rows vs fp64 {r_r:.4f}, tiled vs rows / (sum of bars) {r_b:.4f}; "
          f"max |tiled - fp64| {float((out - c['out64']).abs().max()):.2e}, max |tiled - rows| {float((out - rows).abs().max()):.2e}")
    assert r_t <= 1.0
    assert r_r <= 1.0
    assert r_b <= 1.0


# ---- 3: 16-bit output -------------------------------------------------------------------------------------------------------------------
def between(y16, lo64, hi64, dt):
    """round16(lo) <= y16 <= round16(hi) elementwise, the ends rounded by torch"""
    y = y16.cpu().double()
    return bool(((y >= lo64.to(dt).double()) & (y <= hi64.to(dt).double())).all())


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("hd", ar.HDS)
def test_16bit_output(lib, hd, fmt):
    c = ar.case("rnd_2x300", hd)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    y16 = tiled(lib, c["qkv"].cuda(), c["B"], c["T"], hd, fmt, flag)
    assert between(y16, c["out64"] - c["bar"], c["out64"] + c["bar"], FMT[fmt][1])
    assert int(flag.item()) == 0
    assert torch.equal(tiled(lib, c["qkv"].cuda(), c["B"], c["T"], hd, fmt, None), y16)          # flag may be NULL


@pytest.mark.parametrize("hd", ar.HDS)
def test_fp16_output_overflow_is_flagged_and_bf16_never(lib, hd):
    B, T, C = 1, 40, H * hd
    qkv = rnd(B * T, 3 * C, seed=5).clone()
    qkv[:, 2 * C + 3] = 7.0e4                                             # one V column beyond fp16's 65504: every mean of it is
    qkv = qkv.cuda()
    for fmt, want in (("fp16", 4), ("bf16", 0)):
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        y16 = tiled(lib, qkv, B, T, hd, fmt, flag)
        assert int(flag.item()) == want, fmt
        col = y16[:, 3].float()
        assert bool(torch.isinf(col).all()) if fmt == "fp16" else bool(torch.isfinite(col).all())
        other = torch.ones(C, dtype=torch.bool)
        other[3] = False
        assert torch.isfinite(y16.float()[:, other.cuda()]).all()


# ---- 4: independence ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("others", ["random", "nan"])
@pytest.mark.parametrize("hd", ar.HDS)
def test_a_stream_does_not_depend_on_the_batch(lib, hd, others):
    C = H * hd
    mine = rnd(100, 3 * C, seed=21)                                       # the stream: 100 rows, the first 70 of them alone below
    batch = rnd(3, 100, 3 * C, seed=22) if others == "random" else torch.full((3, 100, 3 * C), float("nan"))
    batch[1] = mine
    alone = tiled(lib, mine[:70].contiguous().cuda(), 1, 70, hd)
    full = tiled(lib, batch.view(300, 3 * C).cuda(), 3, 100, hd)
    assert torch.isfinite(alone).all()
    assert torch.equal(full.view(3, 100, C)[1, :70], alone)
    assert torch.equal(tiled(lib, batch.view(300, 3 * C).cuda(), 3, 100, hd).view(3, 100, C)[1], full.view(3, 100, C)[1])   # two calls
    if others == "nan":
        assert torch.isnan(full.view(3, 100, C)[[0, 2]]).all()


# ---- 5: the engine on the golden models -------------------------------------------------------------------------------------------------
def make_gpt(sd, dims, fmt="fp32", prefill="fp32", attention="rows"):
    from omnitokenizer_amd.gpt import GPT
    V, BS, L, Hh, C = dims
    m = GPT(argparse.Namespace(), V, BS, n_layer=L, n_head=Hh, n_embd=C)
    res = m.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    m = m.cuda().eval().set_weight_format(fmt).set_prefill_format(prefill)
    return m if attention is None else m.set_prefill_attention(attention)


def dmax(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


def golden_idx(V, BS):
    T = min(BS - 3, 37)
    return T, torch.randint(0, V, (3, T + 3), generator=torch.Generator().manual_seed(11))


@pytest.mark.parametrize("name", GPT_CASES)
def test_engine_fp32_tiled_prefill_and_steps_vs_oracle(name):
    """3 streams x 40 tokens: forward in tiled mode within the project's fp32 bar of the oracle; a tiled prefill of the first T tokens
    followed by 3 decode steps, each within the same bar; the switch is live and goes back to the default engine's bits."""
    from omnitokenizer_amd import _lib
    g, sd, dims = load_gpt_case(name)
    V, BS = dims[0], dims[1]
    T, idx = golden_idx(V, BS)
    ref = go.forward(sd, idx, dims[3])
    idx = idx.cuda()
    base, _ = make_gpt(sd, dims, attention=None)(idx)                     # a fresh default engine
    m = make_gpt(sd, dims, attention="tiled")
    logits, _ = m(idx)
    assert m.prefill_attention == "tiled" and _lib.load().omnitok_lm_prefill_attention(m._engine) == 1
    e_fwd = dmax(logits, ref)
    m.reset_streams(3, T + 3)
    pre = m.prefill(idx[:, :T].contiguous(), want_logits=True)
    e_pre = dmax(pre, ref[:, :T])
    e_steps = [dmax(m.step(idx[:, T + i].contiguous()), ref[:, T + i]) for i in range(3)]
    m.check_overflow()
    print(f"{name}: tiled forward vs oracle {e_fwd:.2e}, prefill {e_pre:.2e}, 3 steps after it {max(e_steps):.2e}; "
          f"|tiled - rows| {dmax(logits, base):.2e}; rows vs oracle {dmax(base, ref):.2e}")
    assert e_fwd < LOGIT_TOL and e_pre < LOGIT_TOL and max(e_steps) < LOGIT_TOL
    assert torch.equal(pre, logits[:, :T])                                # a row does not depend on how many rows follow it
    assert not torch.equal(logits, base)                                  # the switch is live
    back, _ = m.set_prefill_attention("rows")(idx)                        # tiled -> rows: the default engine's bits
    assert torch.equal(back, base)
    explicit, _ = make_gpt(sd, dims, attention="rows")(idx)
    assert torch.equal(explicit, base)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", GPT_CASES)
def test_engine_w16_tiled_prefill_vs_restatement(name, fmt):
    g, sd, dims = load_gpt_case(name)
    V, BS, L, Hh, C = dims
    T = min(BS, 40)
    idx = torch.randint(0, V, (3, T), generator=torch.Generator().manual_seed(11))
    l64, _, _, d_ref = pr.reference(sd, idx, Hh, fmt)
    m = make_gpt(sd, dims, fmt, "w16", "tiled")
    logits, _ = m(idx.cuda())
    m.check_overflow()
    e = dmax(logits, l64)
    print(f"{name} {fmt}: w16 + tiled forward vs the fp64 restatement {e:.3e} = {e / d_ref:.2f} d_ref (bar {BAR_FACTOR} d_ref)")
    assert torch.isfinite(logits).all() and e <= BAR_FACTOR * d_ref


def test_engine_tiled_token_losses_do_not_depend_on_the_chunking():
    from omnitokenizer_amd import _lib
    g, sd, dims = load_gpt_case("gpt_hd96")
    T, idx = golden_idx(dims[0], dims[1])
    idx = idx.cuda()
    m = make_gpt(sd, dims, attention="tiled")
    tg = torch.randint(0, m.vocab_size, tuple(idx.shape), generator=torch.Generator().manual_seed(13))
    tg[:, :2] = -1
    tg = tg.cuda()
    before = _lib.get_option("lm_loss_chunk_rows")
    got = {}
    try:
        for rows in (16, 2048):
            _lib.set_option("lm_loss_chunk_rows", rows)
            got[rows] = m.token_losses(idx, tg)
    finally:
        _lib.set_option("lm_loss_chunk_rows", before)
    assert set(got[16]) == set(got[2048])
    for k in got[16]:
        assert torch.equal(torch.as_tensor(got[16][k]), torch.as_tensor(got[2048][k])), k
    assert m.loss_workspace_bytes() > 0


def test_engine_tiled_prefill_of_300_tokens_with_a_bf16_cache():
    """The tiled attention reads K/V from qkv: the prefill's logits do not depend on the cache format (the rows mode's do), the
    scatter still rounds what the next step reads, and the loss workspace is reported."""
    from omnitokenizer_amd import gpt as og
    V, BS, L, Hh, C = 256, 320, 1, 4, 256
    sd = go.synth_gpt_state(V, BS, L, Hh, C, seed=21)
    x = torch.randint(0, V, (2, 301), generator=torch.Generator().manual_seed(22))
    ref = go.forward(sd, x, Hh)
    x = x.cuda()
    m = og.GPT(argparse.Namespace(), V, BS, n_layer=L, n_head=Hh, n_embd=C)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval().set_prefill_attention("tiled")
    m.reset_streams(2, 301)
    l32 = m.prefill(x[:, :300].contiguous(), want_logits=True).clone()
    s32 = m.step(x[:, 300].contiguous()).clone()
    assert dmax(l32, ref[:, :300]) < LOGIT_TOL and dmax(s32, ref[:, 300]) < LOGIT_TOL
    m.set_cache_format("bf16")
    assert m.prefill_attention == "tiled"
    m.reset_streams(2, 301)
    l16 = m.prefill(x[:, :300].contiguous(), want_logits=True)
    assert torch.equal(l16, l32)
    s16 = m.step(x[:, 300].contiguous())
    m.check_overflow()
    assert torch.isfinite(s16).all() and not torch.equal(s16, s32)        # the step reads the rounded rows
    k, v = m.cache_rows(0, 1, 0, 300)
    assert torch.equal(k, k.to(torch.bfloat16).float()) and torch.isfinite(v).all()
    tg = x[:, 1:301].contiguous()
    out = m.token_losses(x[:, :300].contiguous(), tg)
    assert m.loss_workspace_bytes() > 0 and math.isfinite(float(out["loss"])) and torch.isfinite(out["nll"]).all()
