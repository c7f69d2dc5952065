"""GPU (-m gpu): omnitok_attn_desc through the C ABI for the one output field the Python layer never varies -- ldo.  Every
attention kernel writes fp32 rows of heads * 64 columns at a row stride of ldo: into the left columns of a wider tensor it must
store bit for bit what it stores densely (the same kernel and arithmetic, only the addresses differ) and leave the pad columns
alone."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

HEADS = 2
HD = HEADS * 64
SENTINEL = -12345.0


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "needs the MI355X"
    from omnitokenizer_amd import ops as _ops
    return _ops


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).cuda()


def rows_qkv(rows, seed):
    """q [rows, HD] and k, v as the two halves of one [rows, 2 HD] tensor (ldkv = 2 HD)."""
    kv = rnd(rows, 2 * HD, seed=seed + 1)
    return dict(q=rnd(rows, HD, seed=seed), ldq=HD, k=kv[:, :HD], v=kv[:, HD:], ldkv=2 * HD)


def spatial_case(ops):
    return "omnitok_attn_spatial", 128, dict(rows_qkv(128, 10), seqs=2, n_tokens=64, heads=HEADS)


def spatial_h2_case(ops):
    r = rows_qkv(128, 20)
    packed, bounds = ops.attn_pack(r["q"], r["k"], r["v"], 64, HEADS, rnd(64, seed=22).abs() + 0.5, rnd(64, seed=23).abs() + 0.5)
    return "omnitok_attn_spatial_h2", 128, dict(qp=packed[0], kp=packed[1], vp=packed[2], q_bound=bounds[0], k_bound=bounds[1],
                                                v_bound=bounds[2], seqs=2, n_tokens=64, heads=HEADS)


def window_case(ops):
    return "omnitok_attn_window", 64, dict(q=rnd(64, 3 * HD, seed=30), ldq=3 * HD, bias_dense=rnd(HEADS, 64, 64, seed=31, scale=0.5),
                                           seqs=1, gh=8, gw=8, heads=HEADS)


def window_h2_case(ops):
    """Packed operands as the engine makes them (tests/test_gpu_gemm_pl.py::test_window_attention_from_packed_operands_vs_fp64):
    centred planes in window-major order -> plane GEMM with the LayerNorm folded into the weight and the packing epilogues."""
    rows, K = 64, 512
    x = rnd(rows, K, seed=40, scale=1.5) + 0.3
    gamma, beta = rnd(K, seed=41) * 0.1 + 1.0, rnd(K, seed=42) * 0.1
    w = rnd(3 * HD, K, seed=43, scale=0.04)
    planes, scales, stats = ops.stats_pack_windows(x, 8, 8, center=True)
    wf, fb, _ = ops.fold_layernorm_weight(w, gamma, beta, rows_fold=3 * HD)
    l2 = 1.01 * float(torch.nn.functional.layer_norm(x.double(), (K,), gamma.double(), beta.double(), 1e-5).norm(dim=1).max())
    qb, kb, vb = (l2 * float(w[i * HD:(i + 1) * HD].norm(dim=1).max()) * s for i, s in ((0, 0.125), (1, 1.0), (2, 1.0)))
    attn = dict(n_tokens=64, heads=HEADS, q_scale=None, k_scale=None, q_mul=0.125, q_bound=qb, k_bound=kb, v_bound=vb)
    qp, kp = ops.linear_pl(planes, ops.pl_pack_weight(wf), rows, 2 * HD, K, a_scale=scales, epilogue=4,
                           fold=(stats, fb, None, 2 * HD), attn=attn)
    vp = ops.linear_pl(planes, ops.pl_pack_weight(wf[2 * HD:].contiguous()), rows, HD, K, a_scale=scales, epilogue=3,
                       fold=(stats, fb[2 * HD:].contiguous(), None, HD), attn=attn)
    return "omnitok_attn_window_h2", rows, dict(qp=qp, kp=kp, vp=vp, q_bound=qb, k_bound=kb, v_bound=vb,
                                                bias_dense=rnd(HEADS, 64, 64, seed=44, scale=0.5), seqs=1, gh=8, gw=8, heads=HEADS)


def temporal_case(ops):
    return "omnitok_attn_temporal", 80, dict(rows_qkv(80, 50), q_scale=rnd(64, seed=52).abs() + 0.5, k_scale=rnd(64, seed=53).abs() + 0.5,
                                             scale=8.0, seqs=16, n_tokens=5, heads=HEADS, causal=1)


def call(name, rows, ldo, fields):
    """The entry point on `fields` with out = a sentinel-filled [rows, ldo] tensor, which is returned."""
    from omnitokenizer_amd import _lib
    out = torch.full((rows, ldo), SENTINEL, device="cuda", dtype=torch.float32)
    d = _lib.OmnitokAttnDesc(out=out.data_ptr(), ldo=ldo)
    for k, v in fields.items():
        setattr(d, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    _lib.check(getattr(_lib.load(), name)(ctypes.byref(d), torch.cuda.current_stream().cuda_stream), name)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", [spatial_case, spatial_h2_case, window_case, window_h2_case, temporal_case],
                         ids=["attn_spatial", "attn_spatial_h2", "attn_window", "attn_window_h2", "attn_temporal"])
def test_padded_ldo_stores_the_dense_result_and_nothing_else(ops, case):
    name, rows, fields = case(ops)
    dense = call(name, rows, HD, fields)
    wide = call(name, rows, HD + 64, fields)
    assert torch.isfinite(dense).all() and not (dense == SENTINEL).any()   # every element written, with a number
    assert torch.equal(wide[:, :HD], dense)
    assert (wide[:, HD:] == SENTINEL).all()
