// DiT / Latte denoiser: the four block linears of a 16-bit linear format (omnitok_dit_set_linear_format) -- dit_gemm16_kernel and the
// exported omnitok_dit_gemm16 (index: dit_common.h)
#include "gemm16_tile.h"
#include "dit_common.h"

namespace omnitok {

// acc = a16[M, K] . w16[N, K]^T is gemm16_tile (csrc/gemm16_tile.h: the tile, the staging, the fragment maps, the M / N tails and the
// order of a dot product's partial sums, shared with the LM's lm_gemm16_kernel).  The kernel's own part is the epilogue, in fp32 on
// the accumulators, one of
//   EPI_BIAS  (qkv)        y32[m, n] = acc + bias[n]
//   EPI_GELU  (fc1)        y16[m, n] = round16(gelu_tanh(acc + bias[n])): dit_gelu_tanh_f, the arithmetic of omnitok_dit_gelu_tanh,
//                          rounded once into the packed operand of fc2; a finite value that leaves the fp16 range raises
//                          DIT_FLAG_F16_RANGE in *flag
//   EPI_GATE  (proj, fc2)  y = acc + bias[n];  x[m, n] = fmaf(gate[m / n_tokens][n], y, x[m, n]): the arithmetic of
//                          omnitok_dit_gate_residual (y rounded on its own, the gate fused into the add) without a Y in memory.
// A lane owns column n0 + 64 wc + 32 j + r of 32 rows: row m reads its own row of a16, x[m, :] and the gate row of its own sample,
// nothing of another row; m / n_tokens is taken once per row.
enum { EPI_BIAS = OMNITOK_DIT_EPI_BIAS, EPI_GELU = OMNITOK_DIT_EPI_GELU16, EPI_GATE = OMNITOK_DIT_EPI_GATE_RESIDUAL };

template <typename WT, int EPI>
__global__ __launch_bounds__(256, 2) void dit_gemm16_kernel(const unsigned short *__restrict__ a, const unsigned short *__restrict__ w,
                                                            const float *__restrict__ bias, float *__restrict__ y32,
                                                            unsigned short *__restrict__ y16, const float *__restrict__ gate,
                                                            int64_t ld_gate, int n_tokens, float *__restrict__ x, int M, int N, int K,
                                                            int mt, int nt, int *__restrict__ flag) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = wave >> 1, wc = wave & 1, r = lane & 31, h = lane >> 5;
    int m0, n0;
    f32x16 acc[2][2];
    gemm16_tile<WT>(a, w, M, N, K, mt, nt, m0, n0, acc);
    const int nA = n0 + wc * 64 + r, nB = nA + 32;  // the lane's two columns (j = 0, 1)
    const bool inA = nA < N, inB = nB < N;
    const float bA = inA ? bias[nA] : 0.0f, bB = inB ? bias[nB] : 0.0f;
    bool inf = false;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int m = m0 + wr * 64 + i * 32 + mfma32_row(e, h);
            if (m >= M) continue;
            const int64_t o = (int64_t)m * N;
            const float *g = nullptr;
            if constexpr (EPI == EPI_GATE) g = gate + (int64_t)(m / n_tokens) * ld_gate;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int n = j ? nB : nA;
                if (!(j ? inB : inA)) continue;
                const float v = acc[i][j][e] + (j ? bB : bA);
                if constexpr (EPI == EPI_BIAS) {
                    y32[o + n] = v;
                } else if constexpr (EPI == EPI_GELU) {
                    y16[o + n] = dit_round16<WT>(dit_gelu_tanh_f(v), inf);
                } else {
                    x[o + n] = fmaf(g[n], v, x[o + n]);
                }
            }
        }
    if constexpr (EPI == EPI_GELU && __is_same(WT, lm_fp16))
        if (inf) atomicOr(flag, DIT_FLAG_F16_RANGE);
}

template <typename WT, int EPI>
static void dit_gemm16_launch(const void *a16, const void *w16, const float *bias, float *y32, void *y16, const float *gate, int64_t ld_gate,
                              int n_tokens, float *x, int M, int N, int K, int *flag, hipStream_t stream) {
    const int mt = (M + G16_BM - 1) / G16_BM, nt = (N + G16_BN - 1) / G16_BN;
    hipLaunchKernelGGL((dit_gemm16_kernel<WT, EPI>), dim3((unsigned)((int64_t)mt * nt)), dim3(256), 0, stream,
                       static_cast<const unsigned short *>(a16), static_cast<const unsigned short *>(w16), bias, y32,
                       static_cast<unsigned short *>(y16), gate, ld_gate, n_tokens, x, M, N, K, mt, nt, flag);
}

template <typename WT>
static void dit_gemm16_epi(int epi, const void *a16, const void *w16, const float *bias, float *y32, void *y16, const float *gate,
                           int64_t ld_gate, int n_tokens, float *x, int M, int N, int K, int *flag, hipStream_t stream) {
    if (epi == EPI_BIAS)
        dit_gemm16_launch<WT, EPI_BIAS>(a16, w16, bias, y32, y16, gate, ld_gate, n_tokens, x, M, N, K, flag, stream);
    else if (epi == EPI_GELU)
        dit_gemm16_launch<WT, EPI_GELU>(a16, w16, bias, y32, y16, gate, ld_gate, n_tokens, x, M, N, K, flag, stream);
    else
        dit_gemm16_launch<WT, EPI_GATE>(a16, w16, bias, y32, y16, gate, ld_gate, n_tokens, x, M, N, K, flag, stream);
}

}  // namespace omnitok

using namespace omnitok;

extern "C" int omnitok_dit_gemm16(const void *a16, const void *w16, int fmt, const float *bias, int epilogue, float *y32, void *y16,
                                  const float *gate, int64_t ld_gate, int n_tokens, float *x, int64_t M, int N, int K, int *flag,
                                  omnitok_stream_t stream) {
    OT_CHECK_ARG(fmt == OMNITOK_DIT_LIN_BF16 || fmt == OMNITOK_DIT_LIN_FP16, "dit_gemm16: fmt %d (OMNITOK_DIT_LIN_BF16 | _FP16)", fmt);
    OT_CHECK_ARG(epilogue == EPI_BIAS || epilogue == EPI_GELU || epilogue == EPI_GATE,
                 "dit_gemm16: epilogue %d (OMNITOK_DIT_EPI_BIAS | _GELU16 | _GATE_RESIDUAL)", epilogue);
    OT_CHECK_ARG(a16 && w16 && bias, "dit_gemm16: null pointer");
    OT_CHECK_ARG(aligned16(a16) && aligned16(w16) && aligned16(bias), "dit_gemm16: unaligned operand (16 bytes)");
    OT_CHECK_ARG(M >= 1 && M <= (1ll << 24) && N >= 1 && K >= 32 && K % 32 == 0,
                 "dit_gemm16: M %lld (1 .. 2^24), N %d (>= 1), K %d (K %% 32 == 0)", (long long)M, N, K);
    OT_CHECK_ARG((int64_t)((M + G16_BM - 1) / G16_BM) * ((N + G16_BN - 1) / G16_BN) <= 0x7fffffffLL, "dit_gemm16: too many tiles");
    // exactly the outputs of the epilogue
    OT_CHECK_ARG((y32 != nullptr) == (epilogue == EPI_BIAS) && (y16 != nullptr) == (epilogue == EPI_GELU) &&
                     (x != nullptr) == (epilogue == EPI_GATE) && (gate != nullptr) == (epilogue == EPI_GATE),
                 "dit_gemm16: the outputs do not match epilogue %d (0: y32; 1: y16; 2: gate and x)", epilogue);
    OT_CHECK_ARG(aligned16(y32) && aligned16(y16) && aligned16(gate) && aligned16(x), "dit_gemm16: unaligned output / gate (16 bytes)");
    OT_CHECK_ARG(epilogue != EPI_GATE || (n_tokens >= 1 && ld_gate >= 0), "dit_gemm16: n_tokens %d (>= 1), ld_gate %lld (>= 0)", n_tokens,
                 (long long)ld_gate);
    OT_CHECK_ARG(flag || !(epilogue == EPI_GELU && fmt == OMNITOK_DIT_LIN_FP16), "dit_gemm16: null flag (an fp16 output needs one)");
    OT_CHECK_ARG((reinterpret_cast<uintptr_t>(flag) & 3) == 0, "dit_gemm16: unaligned flag");
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (fmt == OMNITOK_DIT_LIN_BF16)
        dit_gemm16_epi<lm_bf16>(epilogue, a16, w16, bias, y32, y16, gate, ld_gate, n_tokens, x, (int)M, N, K, flag, s);
    else
        dit_gemm16_epi<lm_fp16>(epilogue, a16, w16, bias, y32, y16, gate, ld_gate, n_tokens, x, (int)M, N, K, flag, s);
    OT_LAUNCH_CHECK("dit_gemm16");
    return OMNITOK_OK;
}
