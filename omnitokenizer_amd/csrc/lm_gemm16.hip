// LM prefill: the 16-bit MFMA GEMM of a PF_W16 prefill (omnitok_lm_set_prefill_format) -- lm_gemm16_kernel, lm_gemm16 and the
// exported omnitok_lm_gemm16 (index: lm_common.h)
#include "gemm16_tile.h"
#include "gemm_x_common.h"  // gelu_erf

namespace omnitok {

// y[M, N] = act(a16[M, K] . w16[N, K]^T + bias) (+ residual): the tile, the staging, the fragment maps and the order of a dot
// product's partial sums are gemm16_tile's (csrc/gemm16_tile.h, shared with the DiT's block linears); w16 is the image
// lm_round_w16_kernel writes.  The kernel's own part is the epilogue, in fp32 on the accumulators: + bias, exact-erf GELU, + residual
// (may alias y32), or -- Y16 -- rounded with lm_round16<WT> into the packed operand of the next GEMM; an fp16 element that rounds to
// +-inf ORs LM_FLAG_PF16_RANGE into *flag.
template <typename WT, bool Y16>
__global__ __launch_bounds__(256, 2) void lm_gemm16_kernel(const unsigned short *__restrict__ a, const unsigned short *__restrict__ w,
                                                           const float *__restrict__ bias, const float *residual, float *y32,
                                                           unsigned short *__restrict__ y16, int M, int N, int K, int act, int mt,
                                                           int nt, int *__restrict__ flag) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = wave >> 1, wc = wave & 1, r = lane & 31, h = lane >> 5;
    int m0, n0;
    f32x16 acc[2][2];
    gemm16_tile<WT>(a, w, M, N, K, mt, nt, m0, n0, acc);
    // acc[i][j][e] of lane (r, h): row m0 + 64 wr + 32 i + mfma32_row(e, h), column n0 + 64 wc + 32 j + r
    bool inf = false;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = n0 + wc * 64 + j * 32 + r;
        if (n >= N) continue;
        const float bn = bias ? bias[n] : 0.0f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int m = m0 + wr * 64 + i * 32 + mfma32_row(e, h);
                if (m >= M) continue;
                float v = acc[i][j][e];
                if (bias) v += bn;
                if (act == 1) v = gelu_erf(v);
                const int64_t o = (int64_t)m * N + n;
                if constexpr (Y16) {
                    const unsigned short hv = lm_round16<WT>(v);
                    if constexpr (__is_same(WT, lm_fp16)) inf = inf || lm_f16_is_inf(hv);
                    y16[o] = hv;
                } else {
                    if (residual) v += residual[o];
                    y32[o] = v;
                }
            }
    }
    if constexpr (Y16 && __is_same(WT, lm_fp16))
        if (inf && flag) atomicOr(flag, LM_FLAG_PF16_RANGE);
}

template <typename WT>
static void lm_gemm16_launch(const void *a16, const void *w16, const float *bias, const float *residual, float *y32, void *y16, int M,
                             int N, int K, int act, int *flag, hipStream_t stream) {
    const int mt = (M + G16_BM - 1) / G16_BM, nt = (N + G16_BN - 1) / G16_BN;
    const dim3 grid((unsigned)((int64_t)mt * nt));
    const unsigned short *a = static_cast<const unsigned short *>(a16), *w = static_cast<const unsigned short *>(w16);
    if (y16)
        hipLaunchKernelGGL((lm_gemm16_kernel<WT, true>), grid, dim3(256), 0, stream, a, w, bias, residual, y32,
                           static_cast<unsigned short *>(y16), M, N, K, act, mt, nt, flag);
    else
        hipLaunchKernelGGL((lm_gemm16_kernel<WT, false>), grid, dim3(256), 0, stream, a, w, bias, residual, y32,
                           static_cast<unsigned short *>(y16), M, N, K, act, mt, nt, flag);
}

int lm_gemm16(const void *a16, const void *w16, int fmt, const float *bias, const float *residual, float *y32, void *y16, int64_t M,
              int N, int K, int act, int *flag, hipStream_t stream) {
    OT_CHECK_ARG(fmt == OMNITOK_LM_W_BF16 || fmt == OMNITOK_LM_W_FP16, "lm_gemm16: fmt %d (OMNITOK_LM_W_BF16 | OMNITOK_LM_W_FP16)", fmt);
    OT_CHECK_ARG(a16 && w16, "lm_gemm16: null pointer");
    OT_CHECK_ARG((y32 != nullptr) != (y16 != nullptr), "lm_gemm16: exactly one of y32 / y16");
    OT_CHECK_ARG(!(y16 && residual), "lm_gemm16: no residual with a 16-bit output");
    OT_CHECK_ARG(aligned16(a16) && aligned16(w16), "lm_gemm16: unaligned operand (16 bytes)");
    OT_CHECK_ARG((reinterpret_cast<uintptr_t>(y32) & 3) == 0 && (reinterpret_cast<uintptr_t>(y16) & 1) == 0 &&
                     (reinterpret_cast<uintptr_t>(bias) & 3) == 0 && (reinterpret_cast<uintptr_t>(residual) & 3) == 0,
                 "lm_gemm16: unaligned y / bias / residual");
    OT_CHECK_ARG(M >= 1 && M <= 65535 && N >= 1 && K >= 32 && K % 32 == 0, "lm_gemm16: M %lld (1 .. 65535), N %d (>= 1), K %d (K %% 32 == 0)",
                 (long long)M, N, K);
    OT_CHECK_ARG((int64_t)((M + G16_BM - 1) / G16_BM) * ((N + G16_BN - 1) / G16_BN) <= 0x7fffffffLL, "lm_gemm16: too many tiles");
    OT_CHECK_ARG(act == 0 || act == 1, "lm_gemm16: act %d (0 | 1)", act);
    if (fmt == OMNITOK_LM_W_BF16)
        lm_gemm16_launch<lm_bf16>(a16, w16, bias, residual, y32, y16, (int)M, N, K, act, flag, stream);
    else
        lm_gemm16_launch<lm_fp16>(a16, w16, bias, residual, y32, y16, (int)M, N, K, act, flag, stream);
    OT_LAUNCH_CHECK("lm_gemm16");
    return OMNITOK_OK;
}

}  // namespace omnitok

using namespace omnitok;

extern "C" int omnitok_lm_gemm16(const void *a16, const void *w16, int fmt, const float *bias, const float *residual, float *y32,
                                 void *y16, int64_t M, int N, int K, int act, int *flag, omnitok_stream_t stream) {
    return lm_gemm16(a16, w16, fmt, bias, residual, y32, y16, M, N, K, act, flag, static_cast<hipStream_t>(stream));
}
