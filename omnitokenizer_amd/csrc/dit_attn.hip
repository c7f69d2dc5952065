// DiT denoiser: non-causal attention on the fp32-input MFMA (omnitok_dit_attn; index: dit_common.h).
//
// dit_attn_kernel is attn_f32_tiled (csrc/attn_f32_tiled.h, where the layout, the order of every sum and what a row depends on are
// written down) without the causal mask: the body lm_attn_prefill_kernel runs.  What is the DiT's own: N is any (input_size / p)^2, so
// the last key tile has a tail; head_dim 72 (DiT-XL/2), whose third block of 32 dims is one quarter live; query blocks in ascending
// order; scale = fl(hd^-0.5) rounded once from fp64; fp32 output.  LDS 18 / 22 KB per workgroup at head_dim 64 / 72.
//
// dit_attn16_kernel (omnitok_dit_attn16; the attention format of the engines) is the same for attn16_tiled (csrc/attn16_tiled.h): Q, K,
// V and P rounded once to bf16 / fp16, both products on v_mfma_f32_32x32x16_{bf16,f16}; scale fl(log2(e) / sqrt(hd)); output fp32 or
// rounded once more (dit_round16x4: the bits and the flag of omnitok_dit_round16 over the fp32 result) into the packed operand of
// attn.proj.  LDS 9 / 12.25 KB.
#include "attn16_tiled.h"
#include "attn_f32_tiled.h"
#include "dit_common.h"

namespace omnitok {

template <int HD>
__global__ __launch_bounds__(256, 2) void dit_attn_kernel(const float *__restrict__ qkv, int N, int heads, float *__restrict__ out) {
    attn_f32_tiled<HD, false>(qkv, N, heads, blockIdx.y, (float)(1.0 / sqrt((double)HD)),
                              [&](int64_t i, const f32x4 &o) { *reinterpret_cast<f32x4 *>(out + i) = o; });
}

// OP: the operand format; OT: float, or the 16-bit type of the output
template <int HD, typename OP, typename OT>
__global__ __launch_bounds__(256, 2) void dit_attn16_kernel(const float *__restrict__ qkv, int N, int heads, OT *__restrict__ out,
                                                         int *__restrict__ flag) {
    bool op_inf = false, out_inf = false;
    attn16_tiled<HD, false, OP>(qkv, N, heads, blockIdx.y, op_inf, [&](int64_t i, const f32x4 &o) {
        if constexpr (__is_same(OT, float))
            *reinterpret_cast<f32x4 *>(out + i) = o;
        else
            *reinterpret_cast<u32x2 *>(reinterpret_cast<unsigned short *>(out) + i) = dit_round16x4<OT>(o, out_inf);
    });
    if constexpr (__is_same(OP, lm_fp16))
        if (op_inf && flag) atomicOr(flag, DIT_FLAG_ATTN16_RANGE);
    if constexpr (__is_same(OT, lm_fp16))
        if (out_inf && flag) atomicOr(flag, DIT_FLAG_F16_RANGE);
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

extern "C" int omnitok_dit_attn16(const float *qkv, int B, int N, int heads, int head_dim, int op_fmt, float *out32, void *out16, int out_fmt,
                                  int *flag, omnitok_stream_t stream) {
    OT_CHECK_ARG(qkv, "dit_attn16: null pointer");
    OT_CHECK_ARG(op_fmt == OMNITOK_DIT_LIN_BF16 || op_fmt == OMNITOK_DIT_LIN_FP16, "dit_attn16: op_fmt %d (OMNITOK_DIT_LIN_BF16 | _FP16)",
                 op_fmt);
    OT_CHECK_ARG((out32 != nullptr) != (out16 != nullptr), "dit_attn16: exactly one of out32 / out16");
    OT_CHECK_ARG(!out16 || out_fmt == OMNITOK_DIT_LIN_BF16 || out_fmt == OMNITOK_DIT_LIN_FP16,
                 "dit_attn16: out_fmt %d (OMNITOK_DIT_LIN_BF16 | _FP16)", out_fmt);
    OT_CHECK_ARG(aligned16(qkv) && aligned16(out32) && aligned16(out16), "dit_attn16: unaligned pointer (16 bytes)");
    OT_CHECK_ARG((reinterpret_cast<uintptr_t>(flag) & 3) == 0, "dit_attn16: unaligned flag");
    OT_CHECK_ARG(head_dim == 64 || head_dim == 72, "dit_attn16: head_dim %d (64 | 72)", head_dim);
    OT_CHECK_ARG(B >= 1 && N >= 1 && heads >= 1 && heads <= 1024 && (int64_t)B * heads < (1ll << 31) && N <= 65535 * TA_BQ,
                 "dit_attn16: B %d, N %d, heads %d (1 .. 1024)", B, N, heads);
    const dim3 grid((unsigned)(B * heads), (unsigned)((N + TA_BQ - 1) / TA_BQ));
    // the one dispatch over (head_dim, operands, output type)
    auto launch = [&](auto hd, auto op, auto *out) {
        constexpr int HD = decltype(hd)::value;
        typedef decltype(op) OP;
        typedef std::remove_pointer_t<decltype(out)> OT;
        hipLaunchKernelGGL((dit_attn16_kernel<HD, OP, OT>), grid, dim3(256), 0, static_cast<hipStream_t>(stream), qkv, N, heads, out, flag);
    };
    auto with_out = [&](auto hd, auto op) {
        if (out32) launch(hd, op, out32);
        else if (out_fmt == OMNITOK_DIT_LIN_BF16) launch(hd, op, static_cast<lm_bf16 *>(out16));
        else launch(hd, op, static_cast<lm_fp16 *>(out16));
    };
    auto with_op = [&](auto hd) {
        if (op_fmt == OMNITOK_DIT_LIN_BF16) with_out(hd, lm_bf16{});
        else with_out(hd, lm_fp16{});
    };
    if (head_dim == 64) with_op(std::integral_constant<int, 64>{});
    else with_op(std::integral_constant<int, 72>{});
    OT_LAUNCH_CHECK("dit_attn16");
    return OMNITOK_OK;
}
