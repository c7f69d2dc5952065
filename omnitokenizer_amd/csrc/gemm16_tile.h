// The 128 x 128 tile of a 16-bit MFMA GEMM: the one K loop of lm_gemm16_kernel (csrc/lm_gemm16.hip, the LM's PF_W16 prefill) and
// dit_gemm16_kernel (csrc/dit_gemm16.hip, the DiT / Latte block linears).  The kernels differ in their epilogues only, which they
// write themselves on the accumulators this body leaves.
//
// acc = a16[M, K] . w16[N, K]^T on v_mfma_f32_32x32x16_{bf16,f16}: both operands packed 16-bit and row-major, products exact in fp32
// inside the instruction, fp32 accumulators.
//   * workgroup = 4 waves (2 x 2) = one 128 x 128 tile, wave (wr, wc) owns 64 x 64 of it as 2 x 2 accumulators of 32 x 32; the K
//     loop walks 64 k per trip (four 16-k MFMA steps; two on the last trip when K % 64 == 32).  ONE tile shape for every M: the order
//     in which a dot product's partial sums are joined is k order in steps of 16, a function of K alone;
//   * staging: a thread's share of a 128 x 64 operand tile is four 16-byte pieces (rows srow + 32 i, the same 8 k), loaded into
//     registers one trip ahead -- they fly during the current trip's MFMAs -- and written to LDS rows padded to 72 halves (144 B:
//     16-byte aligned pieces, consecutive rows 4 banks apart mod 32).  Rows past M and weight rows past N are clamped duplicates that are
//     computed and never stored: a row of the result is a function of its own row of a16 only, so NaN / Inf elsewhere cannot reach it;
//   * fragments (cdna_hip_programming.md 3, "A/B operand lane maps"): lane (r = lane & 31, h = lane >> 5) holds A[row r][k = 8 h + j]
//     and B[k = 8 h + j][col r] = w[col r][8 h + j], j = 0 .. 7 -- one 16-byte LDS read each; the f16 form uses the same maps
//     (tests/test_gpu_lm_prefill16.py, one-hot exactness, checks every lane, half and k step of both);
//   * C: acc[i][j][e] of lane (r, h) is row m0 + 64 wr + 32 i + mfma32_row(e, h), column n0 + 64 wc + 32 j + r: 32 lanes of one
//     register cover 128 contiguous bytes of an fp32 row.
// Tile order: groups of G16_GM tile rows, inside a group the tile row runs fastest -- the workgroups in flight share a few weight
// tiles and G16_GM activation panels (L2).  A speed choice only.
// Contract of the callers: 256 threads, grid = mt * nt, K % 32 == 0, a16 / w16 16-byte aligned.  LDS 36 KiB.
#pragma once
#include "lm_common.h"  // lm_bf16, lm_fp16, lm_round16

namespace omnitok {

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

// The tile of this workgroup: its first row m0 and column n0, and acc as above.
template <typename WT>
__device__ __forceinline__ void gemm16_tile(const unsigned short *__restrict__ a, const unsigned short *__restrict__ w, int M, int N, int K,
                                            int mt, int nt, int &m0, int &n0, f32x16 (&acc)[2][2]) {
    __shared__ __attribute__((aligned(16))) unsigned short lds[2 * G16_BM * G16_LD];  // A tile | B tile: 36 KiB
    unsigned short *sa = lds, *sb = lds + G16_BM * G16_LD;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1, r = lane & 31, h = lane >> 5;
    const int per = G16_GM * nt, first = (int)(blockIdx.x / per) * G16_GM, in_grp = (int)(blockIdx.x % per);
    const int gsz = mt - first < G16_GM ? mt - first : G16_GM;
    m0 = (first + in_grp % gsz) * G16_BM;
    n0 = (in_grp / gsz) * G16_BN;
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
}

}  // namespace omnitok
