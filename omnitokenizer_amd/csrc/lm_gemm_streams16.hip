// LM decode: the 16-bit MFMA GEMM of an SF_W16 many-stream step (omnitok_lm_set_streams_format) -- lm_gemm_streams16_kernel,
// lm_streams16_reduce_kernel, lm_gemm_streams16 and the exported omnitok_lm_gemm_streams16 (index: lm_common.h)
#include "gemm16_tile.h"    // g16_mfma, u32x4
#include "gemm_x_common.h"  // gelu_erf

#include <mutex>

namespace omnitok {

// y[B, N] = act(x16[B, K] . w16[N, K]^T + bias) (+ residual) for 1 <= B <= 128 streams in ONE pass over the packed 16-bit weights, on
// v_mfma_f32_32x32x16_{bf16,f16}: both operands 16-bit, every product exact in fp32 inside the instruction, fp32 accumulators.  It keeps
// what the contract of lm_gemm_streams_kernel (lm_gemm_mfma.hip) rests on:
//   * workgroup = 4 waves = one tile of 32 weight rows x one K split (blockIdx.y of KS); the 4 waves cut the split's k blocks (64 k
//     each) into 4 contiguous slices of at most CH blocks (a slice may be empty: K = 128 has two blocks), so a tile is reduced over
//     KS * 4 slices.  KS depends on K only (lm_streams16_ksplit): the summation order of an output never depends on the number of
//     streams, the stream's slot or the CU count;
//   * operands go straight from global memory into fragments, no LDS staging: lane (i = lane & 31, h = lane >> 5) holds
//     w[n0 + i][kb + 16 c + 8 h + j] (A) and x[32 t + i][the same k] (B), j = 0 .. 7 -- one 16-byte load each, the operand map of the
//     instruction (gemm16_tile.h) -- so four loads cover one 128-byte line of a row and MFMA c multiplies k = kb + 16 c .. + 15.
//     Stream tile t of NT = ceil(B / 32) has its own 16-register accumulator; rows past N and streams past B are clamped duplicates
//     that are computed and never stored (a column of the product depends on its own stream only: NaN / Inf stay in their row);
//   * ALL of a wave's weights (<= CH blocks x 4 loads of 16 B per lane = 24 KiB per wave) are requested in one burst behind the first
//     block's activations, as lm_gemm4_kernel does, and the next block's activations (L2 hits) before the current block's MFMAs; loads
//     return in order, so the wait for a block's activations never waits for anything younger.  (A first form kept the fp32 kernel's
//     shape, one block of weights in flight per wave.  Both measure the same, 8.6 - 9.1 us at 32 streams and 19.8 - 20.0 us at 128 for
//     N = 4608, K = 1536: the weights' latency is not what bounds the kernel.  A call costs about 3.9 us per stream tile at every N and
//     K of the model -- the activation fetch of a workgroup, 32 rows x 32 bytes per load instruction, is the suspect; not taken apart);
//   * the 4 wave partials meet in LDS and are added in wave order; with KS == 1 bias / exact GELU / residual follow at once,
//     otherwise the tile's partial goes to part[split][B][N] and lm_streams16_reduce_kernel adds the splits in split order and applies
//     the epilogue.  No atomics on the result: two calls give equal bits.
// Output: fp32 into y32, or -- y16 -- rounded once with lm_round16<WT> into the packed operand of the next GEMM (FC1); an fp16 element
// that rounds to +-inf ORs LM_FLAG_SF16_RANGE into *flag.  Sizes: K % 64 == 0, any N >= 1, 1 <= B <= 128.
constexpr int LMS16_NW = 4;
constexpr int LMS16_CH = 6;  // the most 64-k blocks a wave owns: 96 weight registers

// bias, exact GELU, then residual into y32, or the rounding into y16 (no residual in that form); o = b * N + n
template <typename WT>
__device__ __forceinline__ void lms16_epilogue(float v, int64_t o, int n, const float *__restrict__ bias, const float *residual,
                                               float *y32, unsigned short *__restrict__ y16, int act, bool &inf) {
    if (bias) v += bias[n];
    if (act == 1) v = gelu_erf(v);
    if (y16) {
        const unsigned short hv = lm_round16<WT>(v);
        if constexpr (__is_same(WT, lm_fp16)) inf = inf || lm_f16_is_inf(hv);
        y16[o] = hv;
    } else {
        if (residual) v += residual[o];
        y32[o] = v;
    }
}

template <typename WT, int NT, int CH>
__global__ __launch_bounds__(LMS16_NW * 64) void lm_gemm_streams16_kernel(const unsigned short *__restrict__ x,
                                                                          const unsigned short *__restrict__ w,
                                                                          const float *__restrict__ bias, const float *residual,
                                                                          float *y32, unsigned short *__restrict__ y16,
                                                                          float *__restrict__ part, int B, int N, int K, int act, int KS,
                                                                          int *__restrict__ flag) {
    __shared__ float red[LMS16_NW][32][33];  // [wave][stream of the tile][weight row] (+1: the writes stride over streams)
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, h = lane >> 5;
    const int n0 = blockIdx.x * 32, split = blockIdx.y;
    const int nblk = K >> 6, slices = KS * LMS16_NW, slice = split * LMS16_NW + wave;
    const int b_begin = (int)((int64_t)slice * nblk / slices), b_end = (int)((int64_t)(slice + 1) * nblk / slices);
    const int cnt = b_end - b_begin;  // <= CH by the launcher's KS; wave-uniform
    const unsigned short *wp = w + (int64_t)(n0 + i < N ? n0 + i : N - 1) * K + 8 * h;
    const unsigned short *xp[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) xp[t] = x + (int64_t)(t * 32 + i < B ? t * 32 + i : B - 1) * K + 8 * h;
    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
    if (cnt > 0) {
        u32x4 wq[CH][4], xq[2][NT][4];
        // (blocks past the slice ask for its last block again: cache hits, no branch around a load)
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int c = 0; c < 4; ++c) xq[0][t][c] = *reinterpret_cast<const u32x4 *>(xp[t] + b_begin * 64 + 16 * c);
#pragma unroll
        for (int b = 0; b < CH; ++b) {
            const int kb = (b_begin + (b < cnt ? b : cnt - 1)) * 64;
#pragma unroll
            for (int c = 0; c < 4; ++c) wq[b][c] = *reinterpret_cast<const u32x4 *>(wp + kb + 16 * c);
        }
        __builtin_amdgcn_sched_barrier(0);  // the burst stays a burst: the scheduler otherwise sinks each load to its first use
#pragma unroll
        for (int b = 0; b < CH; ++b) {
            if (b < cnt) {
                if (b + 1 < CH) {
                    const int kn = (b_begin + (b + 1 < cnt ? b + 1 : cnt - 1)) * 64;
#pragma unroll
                    for (int t = 0; t < NT; ++t)
#pragma unroll
                        for (int c = 0; c < 4; ++c) xq[(b + 1) & 1][t][c] = *reinterpret_cast<const u32x4 *>(xp[t] + kn + 16 * c);
                    __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
                for (int c = 0; c < 4; ++c)
#pragma unroll
                    for (int t = 0; t < NT; ++t) acc[t] = g16_mfma<WT>(wq[b][c], xq[b & 1][t][c], acc[t]);
            }
        }
    }
    // acc[t][r] of lane (i, h): weight row n0 + mfma32_row(r, h), stream 32 t + i
    bool inf = false;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if (t) __syncthreads();  // the previous tile was read
#pragma unroll
        for (int r = 0; r < 16; ++r) red[wave][i][mfma32_row(r, h)] = acc[t][r];
        __syncthreads();
        for (int o = tid; o < 32 * 32; o += LMS16_NW * 64) {
            const int j = o >> 5, ii = o & 31, b = t * 32 + j, n = n0 + ii;
            const float v = ((red[0][j][ii] + red[1][j][ii]) + red[2][j][ii]) + red[3][j][ii];
            if (b < B && n < N) {
                if (KS > 1) part[((int64_t)split * B + b) * N + n] = v;
                else lms16_epilogue<WT>(v, (int64_t)b * N + n, n, bias, residual, y32, y16, act, inf);
            }
        }
    }
    if constexpr (__is_same(WT, lm_fp16))
        if (inf && flag) atomicOr(flag, LM_FLAG_SF16_RANGE);
}

// y = act(part[0] + part[1] + ... + part[KS - 1] + bias) (+ residual) or its rounding into y16, the splits in split order
template <typename WT>
__global__ __launch_bounds__(256) void lm_streams16_reduce_kernel(const float *__restrict__ part, const float *__restrict__ bias,
                                                                  const float *residual, float *y32, unsigned short *__restrict__ y16,
                                                                  int64_t total, int N, int KS, int act, int *__restrict__ flag) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= total) return;
    float v = part[o];
    for (int s = 1; s < KS; ++s) v += part[(int64_t)s * total + o];
    bool inf = false;
    lms16_epilogue<WT>(v, o, (int)(o % N), bias, residual, y32, y16, act, inf);
    if constexpr (__is_same(WT, lm_fp16))
        if (inf && flag) atomicOr(flag, LM_FLAG_SF16_RANGE);
}

// K splits across workgroups: the fewest that leave a wave at most LMS16_CH blocks, so K <= 1536 runs as one launch.  By measurement
// (MI355X, bf16, 20 back-to-back calls, KS forced in the form with one block in flight): the reduce launch a split adds costs more
// than the workgroups it adds bring back wherever one launch fits -- N = 4608 / 6144 / 8192 at K = 1536: 9.1 / 9.2 / 9.3 us with KS 1
// against 11.0 - 14.5 us with KS 2 .. 3 at 32 streams, 19.8 - 20.9 against 22.1 - 28.6 us at 128 -- while K = 6144 needs the split
// (64 us with KS 1, 24 us with KS 4, 26 - 32 us beyond).  The one shape a split served there is N = 1536 x K = 1536 (48 workgroups:
// 13.1 us with KS 4 against 19.4 us at 128 streams, 8.2 against 8.9 us at 32); it is left at one launch, a rule of K alone, and is the
// cell that gains least (profiles/lm_streams16_bench.json).
// A function of K ONLY -- not of N, not of B, not of the device: the bits of an output do not depend on who shares its batch.
static int lm_streams16_ksplit(int N, int K) {
    (void)N;
    const int nblk = K / 64;
    return (nblk + LMS16_NW * LMS16_CH - 1) / (LMS16_NW * LMS16_CH);
}
int64_t lm_streams16_part_floats(int B, int N, int K) {
    const int ks = lm_streams16_ksplit(N, K);
    return ks > 1 ? (int64_t)ks * B * N : 0;
}

template <typename WT>
static void lm_streams16_launch(const unsigned short *x, const unsigned short *w, const float *bias, const float *residual, float *y32,
                                unsigned short *y16, float *part, int B, int N, int K, int act, int *flag, hipStream_t stream) {
    const int KS = lm_streams16_ksplit(N, K);
    const dim3 grid((N + 31) / 32, KS);
    const int slices = KS * LMS16_NW, ch = (K / 64 + slices - 1) / slices;  // the longest slice: 1 .. LMS16_CH
    auto launch = [&](auto nt, auto chc) {
        hipLaunchKernelGGL((lm_gemm_streams16_kernel<WT, decltype(nt)::value, decltype(chc)::value>), grid, dim3(LMS16_NW * 64), 0, stream, x, w,
                           bias, residual, y32, y16, part, B, N, K, act, KS, flag);
    };
    auto with_ch = [&](auto nt) {
        switch (ch) {
            case 1: launch(nt, std::integral_constant<int, 1>{}); break;
            case 2: launch(nt, std::integral_constant<int, 2>{}); break;
            case 3: launch(nt, std::integral_constant<int, 3>{}); break;
            case 4: launch(nt, std::integral_constant<int, 4>{}); break;
            case 5: launch(nt, std::integral_constant<int, 5>{}); break;
            default: launch(nt, std::integral_constant<int, LMS16_CH>{}); break;
        }
    };
    switch ((B + 31) / 32) {
        case 1: with_ch(std::integral_constant<int, 1>{}); break;
        case 2: with_ch(std::integral_constant<int, 2>{}); break;
        case 3: with_ch(std::integral_constant<int, 3>{}); break;
        default: with_ch(std::integral_constant<int, 4>{}); break;
    }
    if (KS > 1) {
        const int64_t total = (int64_t)B * N;
        hipLaunchKernelGGL(lm_streams16_reduce_kernel<WT>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, part, bias, residual,
                           y32, y16, total, N, KS, act, flag);
    }
}

int lm_gemm_streams16(const void *a16, const void *w16, int fmt, const float *bias, const float *residual, float *y32, void *y16, int B,
                      int N, int K, int act, float *part, int *flag, hipStream_t stream) {
    const unsigned short *x = static_cast<const unsigned short *>(a16), *w = static_cast<const unsigned short *>(w16);
    unsigned short *o16 = static_cast<unsigned short *>(y16);
    if (fmt == OMNITOK_LM_W_BF16) lm_streams16_launch<lm_bf16>(x, w, bias, residual, y32, o16, part, B, N, K, act, flag, stream);
    else lm_streams16_launch<lm_fp16>(x, w, bias, residual, y32, o16, part, B, N, K, act, flag, stream);
    OT_LAUNCH_CHECK("lm_gemm_streams16");
    return OMNITOK_OK;
}

}  // namespace omnitok

using namespace omnitok;

// process-wide grow-only scratch of omnitok_lm_gemm_streams16 (an engine has its own): split partials
static std::mutex g_streams16_ws_mu;
static float *g_streams16_ws = nullptr;
static int64_t g_streams16_ws_bytes = 0;
static int g_streams16_ws_dev = -1;

extern "C" int omnitok_lm_gemm_streams16(const void *a16, const void *w16, int fmt, const float *bias, const float *residual, float *y32,
                                         void *y16, int B, int N, int K, int act, int *flag, omnitok_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    OT_CHECK_ARG(fmt == OMNITOK_LM_W_BF16 || fmt == OMNITOK_LM_W_FP16, "lm_gemm_streams16: fmt %d (OMNITOK_LM_W_BF16 | OMNITOK_LM_W_FP16)",
                 fmt);
    OT_CHECK_ARG(a16 && w16, "lm_gemm_streams16: null pointer");
    OT_CHECK_ARG((y32 != nullptr) != (y16 != nullptr), "lm_gemm_streams16: exactly one of y32 / y16");
    OT_CHECK_ARG(!(y16 && residual), "lm_gemm_streams16: no residual with a 16-bit output");
    OT_CHECK_ARG(aligned16(a16) && aligned16(w16) && aligned16(y32) && aligned16(y16) && aligned16(bias) && aligned16(residual),
                 "lm_gemm_streams16: unaligned pointer (16 bytes)");
    OT_CHECK_ARG(B >= 1 && B <= 128 && N >= 1 && K >= 64 && K % 64 == 0, "lm_gemm_streams16: B %d (1 .. 128), N %d (>= 1), K %d (K %% 64 == 0)",
                 B, N, K);
    OT_CHECK_ARG(act == 0 || act == 1, "lm_gemm_streams16: act %d (0 | 1)", act);
    const int64_t need = lm_streams16_part_floats(B, N, K);
    std::lock_guard<std::mutex> lk(g_streams16_ws_mu);
    if (need > 0) {
        int dev = 0;
        OT_HIP(hipGetDevice(&dev));
        if (g_streams16_ws_dev != dev) g_streams16_ws_bytes = 0;  // another device's memory: never reused, whatever its size
        if (int rc = lm_grow(reinterpret_cast<void **>(&g_streams16_ws), &g_streams16_ws_bytes, need * 4)) return rc;
        g_streams16_ws_dev = dev;
    }
    return lm_gemm_streams16(a16, w16, fmt, bias, residual, y32, y16, B, N, K, act, g_streams16_ws, flag, stream);
}
