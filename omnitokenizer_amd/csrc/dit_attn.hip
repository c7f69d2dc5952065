// DiT denoiser: non-causal attention on the fp32-input MFMA (omnitok_dit_attn; index: dit_common.h).
//
// dit_attn_kernel is attn_f32_tiled (csrc/attn_f32_tiled.h, where the layout, the order of every sum and what a row depends on are
// written down) without the causal mask: the body lm_attn_prefill_kernel runs.  What is the DiT's own: N is any (input_size / p)^2, so
// the last key tile has a tail; head_dim 72 (DiT-XL/2), whose third block of 32 dims is one quarter live; query blocks in ascending
// order; scale = fl(hd^-0.5) rounded once from fp64; fp32 output.  LDS 18 / 22 KB per workgroup at head_dim 64 / 72.
#include "attn_f32_tiled.h"
#include "dit_common.h"

namespace omnitok {

template <int HD>
__global__ __launch_bounds__(256, 2) void dit_attn_kernel(const float *__restrict__ qkv, int N, int heads, float *__restrict__ out) {
    attn_f32_tiled<HD, false>(qkv, N, heads, blockIdx.y, (float)(1.0 / sqrt((double)HD)),
                              [&](int64_t i, const f32x4 &o) { *reinterpret_cast<f32x4 *>(out + i) = o; });
}

}  // namespace omnitok

using namespace omnitok;

extern "C" int omnitok_dit_attn(const float *qkv, int B, int N, int heads, int head_dim, float *out, omnitok_stream_t stream) {
    OT_CHECK_ARG(qkv && out, "dit_attn: null pointer");
    OT_CHECK_ARG(aligned16(qkv) && aligned16(out), "dit_attn: unaligned pointer (16 bytes)");
    OT_CHECK_ARG(head_dim == 64 || head_dim == 72, "dit_attn: head_dim %d (64 | 72)", head_dim);
    OT_CHECK_ARG(B >= 1 && N >= 1 && heads >= 1 && heads <= 1024 && (int64_t)B * heads < (1ll << 31) && N <= 65535 * TA_BQ,
                 "dit_attn: B %d, N %d, heads %d (1 .. 1024)", B, N, heads);
    const dim3 grid((unsigned)(B * heads), (unsigned)((N + TA_BQ - 1) / TA_BQ));
    if (head_dim == 64)
        hipLaunchKernelGGL((dit_attn_kernel<64>), grid, dim3(256), 0, static_cast<hipStream_t>(stream), qkv, N, heads, out);
    else
        hipLaunchKernelGGL((dit_attn_kernel<72>), grid, dim3(256), 0, static_cast<hipStream_t>(stream), qkv, N, heads, out);
    OT_LAUNCH_CHECK("dit_attn");
    return OMNITOK_OK;
}
