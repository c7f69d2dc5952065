// LM prefill: the 16-bit MFMA GEMM of a PF_W16 prefill (omnitok_lm_set_prefill_format) -- lm_gemm16_kernel, lm_gemm16 and the
// exported omnitok_lm_gemm16 (index: lm_common.h)
#include "lm_common.h"
#include "gemm_x_common.h"  // gelu_erf

namespace omnitok {

// y[M, N] = act(a16[M, K] . w16[N, K]^T + bias) (+ residual) on v_mfma_f32_32x32x16_{bf16,f16}: both operands packed 16-bit and
// row-major (w16 is the image lm_round_w16_kernel writes), products exact in fp32 inside the instruction, fp32 accumulators.
//   * workgroup = 4 waves (2 x 2) = one 128 x 128 tile of y, wave (wr, wc) owns 64 x 64 of it as 2 x 2 accumulators of 32 x 32; the K
//     loop walks 64 k per trip (four 16-k MFMA steps; two on the last trip when K % 64 == 32).  ONE tile shape for every M: the order
//     in which a dot product's partial sums are joined is k order in steps of 16, a function of K alone;
//   * staging: a thread's share of a 128 x 64 operand tile is four 16-byte pieces (rows srow + 32 i, the same 8 k), loaded into
//     registers one trip ahead -- they fly during the current trip's MFMAs -- and written to LDS rows padded to 72 halves (144 B:
//     16-byte aligned pieces, consecutive rows 4 banks apart mod 32).  Rows past M and weight rows past N are clamped duplicates that are
//     computed and never stored: a row of y is a function of its own row of a16 only, so NaN / Inf elsewhere cannot reach it;
//   * fragments (cdna_hip_programming.md 3, "A/B operand lane maps"): lane (r = lane & 31, h = lane >> 5) holds A[row r][k = 8 h + j]
//     and B[k = 8 h + j][col r] = w[col r][8 h + j], j = 0 .. 7 -- one 16-byte LDS read each; the f16 form uses the same maps
//     (tests/test_gpu_lm_prefill16.py, one-hot exactness, checks every lane, half and k step of both);
//   * C: lane holds column n = lane & 31 in 16 registers of rows mfma32_row(reg, h): 32 lanes store 128 contiguous bytes of a y32 row;
//   * epilogue in fp32 on the accumulators: + bias, exact-erf GELU, + residual (may alias y32), or -- Y16 -- rounded with lm_round16<WT>
//     into the packed operand of the next GEMM; an fp16 element that rounds to +-inf ORs LM_FLAG_PF16_RANGE into *flag.
// Tile order: groups of G16_GM tile rows, inside a group the tile row runs fastest -- the workgroups in flight share a few weight
// tiles and G16_GM activation panels (L2).  A speed choice only.
constexpr int G16_BM = 128, G16_BN = 128, G16_BK = 64, G16_LD = 72, G16_GM = 16;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

template <typename WT>
__device__ __forceinline__ f32x16 g16_mfma(const u32x4 &a, const u32x4 &b, const f32x16 &c) {
    if constexpr (__is_same(WT, lm_bf16))
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

template <typename WT, bool Y16>
__global__ __launch_bounds__(256, 2) void lm_gemm16_kernel(const unsigned short *__restrict__ a, const unsigned short *__restrict__ w,
                                                           const float *__restrict__ bias, const float *residual, float *y32,
                                                           unsigned short *__restrict__ y16, int M, int N, int K, int act, int mt,
                                                           int nt, int *__restrict__ flag) {
    __shared__ __attribute__((aligned(16))) unsigned short lds[2 * G16_BM * G16_LD];  // A tile | B tile: 36 KiB
    unsigned short *sa = lds, *sb = lds + G16_BM * G16_LD;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1, r = lane & 31, h = lane >> 5;
    const int per = G16_GM * nt, first = (int)(blockIdx.x / per) * G16_GM, in_grp = (int)(blockIdx.x % per);
    const int gsz = mt - first < G16_GM ? mt - first : G16_GM;
    const int m0 = (first + in_grp % gsz) * G16_BM, n0 = (in_grp / gsz) * G16_BN;
    const int srow = tid >> 3, skc = (tid & 7) * 8;
    const unsigned short *ap[4], *wp[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + srow + 32 * i, n = n0 + srow + 32 * i;
        ap[i] = a + (int64_t)(m < M ? m : M - 1) * K + skc;
        wp[i] = w + (int64_t)(n < N ? n : N - 1) * K + skc;
    }
    u32x4 ra[4], rb[4];
    auto load = [&](int k0) {
        const bool in = k0 + skc < K;  // (K % 32 == 0: a piece of 8 k lies inside K or past it as a whole)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ra[i] = in ? *reinterpret_cast<const u32x4 *>(ap[i] + k0) : u32x4{0u, 0u, 0u, 0u};
            rb[i] = in ? *reinterpret_cast<const u32x4 *>(wp[i] + k0) : u32x4{0u, 0u, 0u, 0u};
        }
    };
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;
    load(0);
    for (int k0 = 0; k0 < K; k0 += G16_BK) {
        __syncthreads();  // the previous trip's fragment reads are done
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *reinterpret_cast<u32x4 *>(sa + (srow + 32 * i) * G16_LD + skc) = ra[i];
            *reinterpret_cast<u32x4 *>(sb + (srow + 32 * i) * G16_LD + skc) = rb[i];
        }
        __syncthreads();
        if (k0 + G16_BK < K) load(k0 + G16_BK);
        const int steps = K - k0 >= G16_BK ? 4 : 2;  // (wave-uniform: the half trip at the end of a K with K % 64 == 32)
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            if (kk < steps) {
                u32x4 fa[2], fb[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    fa[i] = *reinterpret_cast<const u32x4 *>(sa + (wr * 64 + i * 32 + r) * G16_LD + kk * 16 + 8 * h);
                    fb[i] = *reinterpret_cast<const u32x4 *>(sb + (wc * 64 + i * 32 + r) * G16_LD + kk * 16 + 8 * h);
                }
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = g16_mfma<WT>(fa[i], fb[j], acc[i][j]);
            }
        }
    }
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
