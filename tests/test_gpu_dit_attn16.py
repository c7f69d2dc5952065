"""omnitok_dit_attn16 on the GPU (include/omnitok_dit.h: the DiT's attention with bf16 / fp16 operands on the 16-bit MFMA): exact cases
(one key, zero queries, a row of one dominant key), every element against fp64 within the bar derived in tests/dit_attn16_ref.py, what
head_dim 72 must not read, bitwise batch independence, the packed output against omnitok_dit_round16 and the range flags.  The shapes
are the smallest that cross every edge: a key tail, a whole tile, a tile plus one key, the 128-query block edge on both sides."""
import ctypes
import math

import pytest
import torch

from tests import dit_attn16_ref as a16
from tests import error_bounds as eb
from tests import lm_prefill_attn_ref as ar

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
FMT = {"bf16": (1, torch.bfloat16), "fp16": (2, torch.float16)}
FMTS = a16.FMTS
F16_RANGE, ATTN16_RANGE = 4, 8  # DIT_FLAG_F16_RANGE, DIT_FLAG_ATTN16_RANGE


@pytest.fixture(scope="module")
def lib():
    from omnitokenizer_amd import build, _lib
    build.build()
    return _lib.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


def ok(lib, rc):
    assert rc == 0, lib.omnitok_last_error().decode()


def run(lib, qkv, B, N, heads, hd, op, out=None, flag=None):
    """out None: the fp32 result; else the result packed in format `out`.  flag: an int32 device tensor, or None = NULL."""
    qkv = qkv.cuda().contiguous()
    assert qkv.shape == (B * N, 3 * heads * hd)
    fp = None if flag is None else P(flag.data_ptr())
    if out is None:
        o = torch.full((B * N, heads * hd), float("nan"), device="cuda")
        ok(lib, lib.omnitok_dit_attn16(P(qkv.data_ptr()), B, N, heads, hd, FMT[op][0], P(o.data_ptr()), None, 0, fp, stream()))
    else:
        o = torch.full((B * N, heads * hd), float("nan"), device="cuda", dtype=FMT[out][1])
        ok(lib, lib.omnitok_dit_attn16(P(qkv.data_ptr()), B, N, heads, hd, FMT[op][0], None, P(o.data_ptr()), FMT[out][0], fp, stream()))
    return o


def new_flag():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


def heads_view(qkv, B, N, heads, hd):
    return qkv.view(B, N, 3, heads, hd)


# ---- exact cases -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd", a16.HDS)
@pytest.mark.parametrize("fmt", FMTS)
def test_single_key_is_v_rounded_once(lib, fmt, hd):
    B, heads = 3, 2
    qkv = ar.rnd(B, 3 * heads * hd, seed=11 + hd)
    out = run(lib, qkv, B, 1, heads, hd, fmt)
    assert torch.equal(out.cpu(), qkv[:, 2 * heads * hd:].to(FMT[fmt][1]).float())


@pytest.mark.parametrize("hd", a16.HDS)
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("N", [31, 32, 33, 36, 81, 127, 128, 129, 257])
def test_zero_queries_give_the_exact_mean_of_v(lib, N, fmt, hd):
    """q = 0: every score is 0, every weight exactly 1, l = N, O the exact integer sum of V: a key too many or too few anywhere
    changes it.  One fp32 division."""
    B, heads = 2, 2
    g = torch.Generator().manual_seed(1000 + N + hd)
    qkv = heads_view(torch.randn(B * N, 3 * heads * hd, generator=g), B, N, heads, hd).clone()
    qkv[:, :, 0] = 0.0
    qkv[:, :, 2] = torch.randint(-8, 9, (B, N, heads, hd), generator=g).float()
    want = (qkv[:, :, 2].sum(1, keepdim=True) / float(N)).expand(B, N, heads, hd).reshape(B * N, heads * hd)
    out = run(lib, qkv.view(B * N, -1), B, N, heads, hd, fmt)
    assert torch.equal(out.cpu(), want)


@pytest.mark.parametrize("hd", a16.HDS)
@pytest.mark.parametrize("fmt", FMTS)
def test_row_of_large_logits(lib, fmt, hd):
    """tests/test_gpu_dit.py::test_attention_row_of_large_logits for 16-bit operands: q, k are bf16 values (exact under both formats;
    the x 32 is a power of two), a query row and two key rows 32 x larger, the large keys in the second and the last tile so that the
    running max moves from tile to tile: logits in the hundreds, every element within the bar.  And a row whose expected value is
    known: query 7 = 16 e_0, key 40 = 64 e_0 + (its random rest x 0): score 1024 / sqrt(hd) >= 120 above every other (|other| <= 16 x 5
    / sqrt(hd)), so every other weight underflows to 0 and the row is V[40] rounded once, bit for bit."""
    B, heads, N = 1, 2, 81
    qkv = heads_view(ar.rnd(B * N, 3 * heads * hd, seed=7 + hd), B, N, heads, hd).clone()
    qkv[:, :, :2] = qkv[:, :, :2].to(torch.bfloat16).float()
    qkv[0, 5, 0] *= 32.0
    qkv[0, 40, 1] *= 32.0
    qkv[0, 80, 1] *= 32.0
    qkv[0, 7, 0] = 0.0
    qkv[0, 7, 0, :, 0] = 16.0
    qkv[0, :, 1, :, 0] = qkv[0, :, 1, :, 0].clamp(-5.0, 5.0)
    qkv[0, 40, 1, :, 0] = 64.0
    flat = qkv.view(B * N, -1)
    out = run(lib, flat, B, N, heads, hd, fmt).cpu()
    ref, bar = a16.reference16(flat, B, N, heads, fmt)
    s_max = float((qkv.double()[0, :, 0].transpose(0, 1) @ qkv.double()[0, :, 1].permute(1, 2, 0)).abs().max() / math.sqrt(hd))
    assert s_max > 100.0
    err = (out.double() - ref).abs()
    print(f"large logits hd {hd} {fmt}: max |s| {s_max:.0f}, max err {float(err.max()):.2e}, err / bar {eb.ratio(err, bar):.3f}")
    assert torch.isfinite(out).all() and eb.ratio(err, bar) <= 1.0
    assert torch.equal(out[7], qkv[0, 40, 2].reshape(-1).to(FMT[fmt][1]).float())


# ---- against fp64 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("bh", list(a16.BH))
@pytest.mark.parametrize("hd", a16.HDS)
@pytest.mark.parametrize("N", a16.NS)
def test_against_fp64_within_the_bar(lib, N, hd, bh, fmt):
    c = a16.case(N, hd, bh, fmt)
    out = run(lib, c["qkv"], c["B"], N, c["H"], hd, fmt).cpu()
    r = eb.ratio((out.double() - c["out64"]).abs(), c["bar"])
    print(f"dit_attn16 N {N} hd {hd} B {c['B']} heads {c['H']} {fmt}: worst err / bar over all elements {r:.3f}")
    assert r <= 1.0


# ---- what the kernel must not read ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_hd72_reads_nothing_behind_column_71(lib, fmt):
    """The half k-step of S and the dead dims of O multiply zeros, not the neighbouring head's q / k / v -- NaN here -- nor, for the
    LAST head, the k / v section (the next row's q for V) that lies behind it."""
    B, N, hd = 2, 36, 72
    heads = 3
    base = heads_view(ar.rnd(B * N, 3 * heads * hd, seed=31), B, N, heads, hd)
    poisoned = base.clone()
    poisoned[:, :, :, 0] = float("nan")
    poisoned[:, :, :, 2] = float("nan")
    clean = run(lib, base.reshape(B * N, -1), B, N, heads, hd, fmt).view(B * N, heads, hd)
    out = run(lib, poisoned.reshape(B * N, -1), B, N, heads, hd, fmt).view(B * N, heads, hd)
    assert torch.isfinite(out[:, 1]).all() and torch.equal(out[:, 1], clean[:, 1])
    assert torch.isnan(out[:, 0]).all() and torch.isnan(out[:, 2]).all()   # those heads themselves multiply the NaNs
    # head 1 as the last head
    heads = 2
    base = heads_view(ar.rnd(B * N, 3 * heads * hd, seed=32), B, N, heads, hd)
    poisoned = base.clone()
    poisoned[:, :, :, 0] = float("nan")
    clean = run(lib, base.reshape(B * N, -1), B, N, heads, hd, fmt).view(B * N, heads, hd)
    out = run(lib, poisoned.reshape(B * N, -1), B, N, heads, hd, fmt).view(B * N, heads, hd)
    assert torch.isfinite(out[:, 1]).all() and torch.equal(out[:, 1], clean[:, 1])
    assert torch.isnan(out[:, 0]).all()


@pytest.mark.parametrize("hd", a16.HDS)
@pytest.mark.parametrize("fmt", FMTS)
def test_a_sample_does_not_depend_on_the_batch(lib, fmt, hd):
    N, heads = 161, 2   # two query blocks, a tail of one key
    C3 = 3 * heads * hd
    mine = ar.rnd(N, C3, seed=41 + hd)
    alone = run(lib, mine, 1, N, heads, hd, fmt)
    assert torch.equal(run(lib, mine, 1, N, heads, hd, fmt), alone)   # two calls on the same input
    for others in (ar.rnd(2 * N, C3, seed=42), torch.full((2 * N, C3), float("nan"))):
        batch = torch.cat([others[:N], mine, others[N:]])
        out = run(lib, batch, 3, N, heads, hd, fmt)
        assert torch.equal(out[N:2 * N], alone)
    assert torch.isnan(out[:N]).all() and torch.isnan(out[2 * N:]).all()


# ---- the packed output and the flags -------------------------------------------------------------------------------------------------------
def rounded(lib, out32, fmt):
    out16 = torch.empty(out32.shape, device="cuda", dtype=FMT[fmt][1])
    flag = new_flag()
    ok(lib, lib.omnitok_dit_round16(P(out32.data_ptr()), FMT[fmt][0], P(out16.data_ptr()), out32.numel(), P(flag.data_ptr()), stream()))
    return out16, int(flag.item())


@pytest.mark.parametrize("hd", a16.HDS)
@pytest.mark.parametrize("out_fmt", FMTS)
@pytest.mark.parametrize("op_fmt", FMTS)
def test_packed_output_is_round16_of_the_fp32_output(lib, op_fmt, out_fmt, hd):
    B, N, heads = 2, 36, 2
    qkv = heads_view(ar.rnd(B * N, 3 * heads * hd, seed=61 + hd), B, N, heads, hd).clone()
    for big in (None, 6.0e4):   # plain; then a V column past fp16's largest finite value under bf16 operands, still inside under fp16
        if big is not None:
            qkv[1, :, 2, 1, 3] = big * (1.2 if op_fmt == "bf16" else 1.0)
        f32, f16 = new_flag(), new_flag()
        out32 = run(lib, qkv.view(B * N, -1), B, N, heads, hd, op_fmt, flag=f32)
        out16 = run(lib, qkv.view(B * N, -1), B, N, heads, hd, op_fmt, out=out_fmt, flag=f16)
        want, want_flag = rounded(lib, out32, out_fmt)
        assert torch.equal(out16.view(torch.int16), want.view(torch.int16))
        assert int(f32.item()) == 0 and int(f16.item()) == want_flag
        assert want_flag == (F16_RANGE if (big is not None and op_fmt == "bf16" and out_fmt == "fp16") else 0)
    # flag NULL: the same bits, nothing written anywhere
    assert torch.equal(run(lib, qkv.view(B * N, -1), B, N, heads, hd, op_fmt, out=out_fmt).view(torch.int16), out16.view(torch.int16))
    assert torch.equal(run(lib, qkv.view(B * N, -1), B, N, heads, hd, op_fmt), out32)


@pytest.mark.parametrize("hd", a16.HDS)
def test_range_flags(lib, hd):
    """fp16 operands: a finite q, k or v that rounds to +-inf raises bit 8; bf16 never does.  An fp16 OUTPUT that rounds from a finite
    value to +-inf raises bit 4.  Under fp16 operands an output is a convex combination of fp16 values, so one launch cannot raise
    both: the two bits meet in a range word that two launches share (they are ORed into it, not written)."""
    B, N, heads = 2, 36, 2
    base = heads_view(ar.rnd(B * N, 3 * heads * hd, seed=71 + hd), B, N, heads, hd)
    for which in range(3):   # a Q, a K and a V column of the last head of sample 1: its last column, the last the kernel reads
        qkv = base.clone()
        qkv[1, :, which, heads - 1, hd - 1] = 7.0e4
        flat = qkv.view(B * N, -1)
        flag = new_flag()
        run(lib, flat, B, N, heads, hd, "fp16", flag=flag)
        assert int(flag.item()) == ATTN16_RANGE, which
        flag = new_flag()
        out = run(lib, flat, B, N, heads, hd, "bf16", flag=flag)
        assert int(flag.item()) == 0 and torch.isfinite(out).all(), which
    # which == 2 still: the V column.  bf16 operands keep it finite, the fp16 output does not
    flag = new_flag()
    out16 = run(lib, flat, B, N, heads, hd, "bf16", out="fp16", flag=flag)
    assert int(flag.item()) == F16_RANGE and torch.isinf(out16[N:, -1].float()).all()
    run(lib, flat, B, N, heads, hd, "fp16", flag=flag)
    assert int(flag.item()) == (F16_RANGE | ATTN16_RANGE) == 12
    # an operand that is infinite already is not a range error
    qkv = base.clone()
    qkv[0, 3, 2, 0, 0] = float("inf")
    flag = new_flag()
    run(lib, qkv.view(B * N, -1), B, N, heads, hd, "fp16", out="fp16", flag=flag)
    assert int(flag.item()) == 0
