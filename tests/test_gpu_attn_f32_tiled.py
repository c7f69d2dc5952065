"""GPU (-m gpu): the causal and the non-causal tiled fp32-MFMA attention are one body (csrc/attn_f32_tiled.h).

The last row of a stream sees every key under the causal mask too, in the same tiles and the same order, and at head_dim 64 the two
scale formulas give the same fp32 value: row T - 1 of omnitok_lm_attn_prefill (fp32 output) and row N - 1 of omnitok_dit_attn on the
same qkv, N = T, are the same bits."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
P = ctypes.c_void_p


@pytest.mark.parametrize("T", [1, 31, 32, 33, 129, 257])
def test_last_row_of_the_causal_kernel_is_the_non_causal_kernels(T):
    from omnitokenizer_amd import _lib
    lib = _lib.load()
    B, heads, hd = 2, 2, 64
    C = heads * hd
    qkv = torch.randn(B * T, 3 * C, generator=torch.Generator().manual_seed(T)).cuda()
    lm = torch.full((B * T, C), float("nan"), device="cuda")
    dit = torch.full((B * T, C), float("nan"), device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    assert lib.omnitok_lm_attn_prefill(P(qkv.data_ptr()), B, T, heads, hd, P(lm.data_ptr()), None, 0, None, s) == 0, lib.omnitok_last_error()
    assert lib.omnitok_dit_attn(P(qkv.data_ptr()), B, T, heads, hd, P(dit.data_ptr()), s) == 0, lib.omnitok_last_error()
    torch.cuda.synchronize()
    assert torch.isfinite(lm).all() and torch.isfinite(dit).all()
    assert torch.equal(lm.view(B, T, C)[:, T - 1], dit.view(B, T, C)[:, T - 1])
