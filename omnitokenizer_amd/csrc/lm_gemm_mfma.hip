// LM decode: the two matrix-core kernels -- lm_gemm4_kernel (4 .. 8 streams, "lm_mfma" 1) and lm_gemm_streams_kernel (17 .. 128
// streams) -- and omnitok_lm_gemm_streams (index: lm_common.h)
#include "lm_common.h"
#include "gemm_x_common.h"  // gelu_erf, x3_rsrc

#include <mutex>

namespace omnitok {

// ---------------------------------------------------------------------------------------------------------------------
// Multi-stream decode GEMV on the matrix cores (r06): y[b][n] = act(LN(x_b) . w_n + bias_n) (+ residual) for 4 .. 8 streams in ONE
// pass over the weights.  The K-sliced VALU kernel above spends, per weight float4, 4 FMAs per stream plus a cross-lane
// transpose-sum per row and stream: 8 streams cost 1.43 ms per decode step against 0.85 ms for one, although the weight bytes are
// the same.  Here v_mfma_f32_4x4x1_16B_f32 does the work: 16 independent 4 x 4 outer products per instruction, fp32 in, fp32
// accumulate -- block b of a lane group holds k = k0 + 4 b + e, so one instruction multiplies 4 weight rows x 16 k by 16 k x 4 streams.
//   * workgroup = 8 waves = a contiguous slice of the weight rows (grid = a multiple of the CUs: every CU streams the same bytes,
//     as in lm_gemv_ks_kernel), in quads of 4 rows; lane (blk = lane / 4, r = lane % 4) loads w[row 4 q + r][k0 + 64 c + 4 blk .. + 3]:
//     256 contiguous bytes per row and instruction.  Wave w owns k in [w K / 8, (w + 1) K / 8) = CH chunks of 64;
//   * ALL of the workgroup's weights (<= 24 loads of 16 B per lane = 24 KiB per wave) are requested in one burst at the start --
//     rows beyond the slice are cut off by the buffer descriptor -- and land while the LayerNorm statistics are computed.
//     (A first form on 16-row v_mfma_f32_16x16x4_f32 tiles kept one 1536-k pass of a 16-row group in flight per wave: with 6 live
//     rows of 16 per workgroup at N = 1536 it streamed 1.3 TB/s, 2.2 ms per step -- profiles/r06_lm_mfma.txt);
//   * activations: lane (blk, c) holds x[stream 4 sq + c][the same k] for sq = 0, 1; with a LayerNorm (K = 1536: 24 registers) they
//     are loaded BEFORE the weights, normalised in registers (two-pass statistics across the workgroup) and kept; without one they
//     are read chunk by chunk (L2) behind the weights;
//   * per row quad and stream quad one 4-register accumulator; at the end the 16 k blocks are summed across lanes (4 xor steps),
//     the 8 waves through LDS in wave order (deterministic), then bias / GELU / residual.
// Same fp32 products as the VALU kernels, another summation order (tests/test_gpu_lm.py::test_gemv_mfma_path_equals_valu_path).
constexpr int LMM_NW = 8;
int g_lm_mfma_mult = 1;  // "lm_mfma_mult": workgroups per CU of lm_gemm4_kernel (at least; more when a slice would exceed QMAX quads)

template <int ACT, bool LN, int CH, int QMAX>
__global__ __launch_bounds__(LMM_NW * 64, 2) void lm_gemm4_kernel(const float *__restrict__ x, const float *__restrict__ w,
                                                                  const float *__restrict__ bias, const float *residual,
                                                                  const float *__restrict__ g, const float *__restrict__ beta,
                                                                  float *y, int B, int N, int K) {
    static_assert(CH * QMAX <= 24 && (!LN || CH <= 4), "registers: weights in one burst, LayerNorm activations resident");
    // LDS: [NW * 4 lane rows][QMAX * 4 weight rows][8 streams] partial sums | [NW * 4][8] LayerNorm partials
    extern __shared__ float mm_lds[];
    constexpr int NP = LMM_NW * 4;               // partial sums per output: 8 waves x the 4 sixteen-lane rows of a wave
    float *part = mm_lds, *red = mm_lds + NP * QMAX * 32;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int blk = lane >> 2, r = lane & 3, lrow = lane >> 4;
    const int r_begin = (int)((int64_t)blockIdx.x * N / gridDim.x), r_end = (int)((int64_t)(blockIdx.x + 1) * N / gridDim.x);
    const int nrows = r_end - r_begin, Q = (nrows + 3) >> 2;   // <= QMAX by the launcher's grid
    const int k0 = wave * (CH * 64) + blk * 4;                 // this lane's first k
    typedef float f32x4v __attribute__((ext_vector_type(4)));
    // streams of this lane: r and r + 4 (those beyond B repeat the last one and are never stored)
    const float *x0 = x + (int64_t)(r < B ? r : B - 1) * K + k0, *x1 = x + (int64_t)(r + 4 < B ? r + 4 : B - 1) * K + k0;
    // every load of the kernel goes out here, activations and LayerNorm constants first (they are needed first)
    f32x4v xa[CH][2], gv[LN ? CH : 1], bv[LN ? CH : 1];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        xa[c][0] = *reinterpret_cast<const f32x4v *>(x0 + c * 64);
        xa[c][1] = *reinterpret_cast<const f32x4v *>(x1 + c * 64);
        if constexpr (LN) {
            gv[c] = *reinterpret_cast<const f32x4v *>(g + k0 + c * 64);
            bv[c] = *reinterpret_cast<const f32x4v *>(beta + k0 + c * 64);
        }
    }
    // weights: rows beyond the workgroup's slice (and whole quads beyond Q) lie outside the descriptor -- zeros, no traffic, no branch
    const auto w_rs = x3_rsrc(w + (int64_t)r_begin * K, nrows * K * 4);
    f32x4v wv[QMAX][CH];
#pragma unroll
    for (int q = 0; q < QMAX; ++q)
#pragma unroll
        for (int c = 0; c < CH; ++c)
            wv[q][c] = __builtin_bit_cast(f32x4v, __builtin_amdgcn_raw_buffer_load_b128(w_rs, ((q * 4 + r) * K + k0 + c * 64) * 4, 0, 2));
    __builtin_amdgcn_sched_barrier(0);   // the burst stays a burst: the scheduler otherwise sinks each load to its first use
    if constexpr (LN) {
        // two-pass statistics of streams r, r + 4 over all K: the 4 blocks of a 16-lane row by DPP, the 32 rows of the workgroup
        // through LDS.  lds_barrier (lgkmcnt only): __syncthreads() would drain vmcnt -- the weight burst -- in front of the first one
        float s[2] = {0.0f, 0.0f};
#pragma unroll
        for (int c = 0; c < CH; ++c)
#pragma unroll
            for (int sq = 0; sq < 2; ++sq) s[sq] += (xa[c][sq][0] + xa[c][sq][1]) + (xa[c][sq][2] + xa[c][sq][3]);
#pragma unroll
        for (int sq = 0; sq < 2; ++sq) {
            s[sq] += dpp_f32<0x128>(s[sq]);   // row_ror:8, row_ror:4
            s[sq] += dpp_f32<0x124>(s[sq]);
            if ((lane & 12) == 0) red[(wave * 4 + lrow) * 8 + sq * 4 + r] = s[sq];
        }
        lds_barrier();
        float mean[2], rstd[2];
#pragma unroll
        for (int sq = 0; sq < 2; ++sq) {
            float t = 0.0f;
#pragma unroll
            for (int i = 0; i < NP; ++i) t += red[i * 8 + sq * 4 + r];
            mean[sq] = t / (float)K;
        }
        lds_barrier();
        float qs[2] = {0.0f, 0.0f};
#pragma unroll
        for (int c = 0; c < CH; ++c)
#pragma unroll
            for (int sq = 0; sq < 2; ++sq)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float d = xa[c][sq][e] - mean[sq];
                    qs[sq] = fmaf(d, d, qs[sq]);
                }
#pragma unroll
        for (int sq = 0; sq < 2; ++sq) {
            qs[sq] += dpp_f32<0x128>(qs[sq]);
            qs[sq] += dpp_f32<0x124>(qs[sq]);
            if ((lane & 12) == 0) red[(wave * 4 + lrow) * 8 + sq * 4 + r] = qs[sq];
        }
        lds_barrier();
#pragma unroll
        for (int sq = 0; sq < 2; ++sq) {
            float t = 0.0f;
#pragma unroll
            for (int i = 0; i < NP; ++i) t += red[i * 8 + sq * 4 + r];
            rstd[sq] = 1.0f / sqrtf(t / (float)K + 1e-5f);
        }
#pragma unroll
        for (int c = 0; c < CH; ++c)
#pragma unroll
            for (int sq = 0; sq < 2; ++sq)
#pragma unroll
                for (int e = 0; e < 4; ++e) xa[c][sq][e] = (xa[c][sq][e] - mean[sq]) * rstd[sq] * gv[c][e] + bv[c][e];
    }
    f32x4v acc[QMAX][2];
#pragma unroll
    for (int q = 0; q < QMAX; ++q)
#pragma unroll
        for (int sq = 0; sq < 2; ++sq) acc[q][sq] = f32x4v{0.0f, 0.0f, 0.0f, 0.0f};
    // (e before q: consecutive MFMAs go to the 2 QMAX different accumulators, none waits for its predecessor's result;
    //  quads beyond Q multiply zeros -- cheaper than a branch per pair of MFMAs)
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int q = 0; q < QMAX; ++q)
#pragma unroll
                for (int sq = 0; sq < 2; ++sq)
                    acc[q][sq] = __builtin_amdgcn_mfma_f32_4x4x1f32(wv[q][c][e], xa[c][sq][e], acc[q][sq], 0, 0, 0);
    // acc[q][sq][v] (lane = (blk, c)): row 4 q + v, stream 4 sq + c, partial over the k = 4 blk + e (mod 64) of this wave's slice.
    // The 4 blocks of each 16-lane row are summed by DPP; the 4 rows of the wave and the 8 waves meet in LDS.
#pragma unroll
    for (int q = 0; q < QMAX; ++q)
#pragma unroll
        for (int sq = 0; sq < 2; ++sq)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                float t = acc[q][sq][v];
                t += dpp_f32<0x128>(t);
                t += dpp_f32<0x124>(t);
                if ((lane & 12) == 0) part[((wave * 4 + lrow) * QMAX * 4 + q * 4 + v) * 8 + sq * 4 + r] = t;
            }
    lds_barrier();
    for (int o = tid; o < Q * 32; o += LMM_NW * 64) {
        const int row = o >> 3, st = o & 7, n = r_begin + row;
        float v = 0.0f;
#pragma unroll
        for (int i = 0; i < NP; ++i) v += part[i * QMAX * 32 + o];
        if (st < B && n < r_end) {
            if (bias) v += bias[n];
            if (ACT == 1) v = gelu_erf(v);
            if (residual) v += residual[(int64_t)st * N + n];
            y[(int64_t)st * N + n] = v;
        }
    }
}

template <int ACT, bool LN, int CH, int QMAX>
static void launch_gemm4_cfg(const LmLinear &c, hipStream_t stream) {
    const int N = c.N;
    int n_cu = 256;
    (void)current_device_cus(&n_cu);
    const int per = QMAX * 4;                               // rows a workgroup can own
    int mult = g_lm_mfma_mult > 1 ? g_lm_mfma_mult : 1;
    while ((int64_t)n_cu * mult * per < (int64_t)N + n_cu * mult) ++mult;   // ceil(N / grid) <= per
    int grid = n_cu * mult;
    if (grid > N) grid = N;
    hipLaunchKernelGGL((lm_gemm4_kernel<ACT, LN, CH, QMAX>), dim3(grid), dim3(LMM_NW * 64), (LMM_NW * 4 * QMAX * 32 + LMM_NW * 4 * 8) * 4, stream,
                       c.x, c.w.w32, c.bias, c.residual, c.ln_g, c.ln_b, c.y, c.B, c.N, c.K);
}

// K / 512 chunks of 64 k per wave: 3 (K = 1536), 4 (2048), 12 (6144), 16 (8192); false: no MFMA form for this call
template <int ACT, bool LN>
static bool launch_gemm4(const LmLinear &c, hipStream_t stream) {
    switch (c.K) {
        case 1536: launch_gemm4_cfg<ACT, LN, 3, 8>(c, stream); return true;
        case 2048: launch_gemm4_cfg<ACT, LN, 4, 6>(c, stream); return true;
        default: break;
    }
    if constexpr (!LN) {   // (the wide inputs -- FC2's 4 C -- carry no LayerNorm)
        switch (c.K) {
            case 6144: launch_gemm4_cfg<ACT, false, 12, 2>(c, stream); return true;
            case 8192: launch_gemm4_cfg<ACT, false, 16, 1>(c, stream); return true;
            default: break;
        }
    }
    return false;
}

bool lm_gemm4_try(const LmLinear &c, hipStream_t stream) {  // (fp32 weights only: lm_gemv_any asks for no other)
    if (c.ln_g) return c.act ? launch_gemm4<1, true>(c, stream) : launch_gemm4<0, true>(c, stream);
    return c.act ? launch_gemm4<1, false>(c, stream) : launch_gemm4<0, false>(c, stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// Many-stream decode GEMM (omnitok_lm_set_max_streams; B >= "lm_streams_min"): y[B, N] = act(x[B, K] . w[N, K]^T + bias) (+ residual)
// for up to 128 streams in ONE pass over the weights, on v_mfma_f32_32x32x2_f32 -- fp32 in, fp32 accumulate, bit for bit an fmaf chain
// in k order, so every product is still an fp32 product of an fp32 activation and the weight's exact (widened) fp32 value.
//   * workgroup = 4 waves = one tile of 32 weight rows x one K split (blockIdx.y of KS); the 4 waves cut the split's k blocks (32 k
//     each) into 4 contiguous slices, so a tile is reduced over KS * 4 slices.  KS depends on (N, K) only (lm_streams_ksplit): the
//     summation order of an output never depends on the number of streams, the stream's slot or the CU count;
//   * operands: lane (i = lane & 31, h = lane >> 5) holds w[n0 + i][kb + 8 c + 4 h + e] (A) and x[32 t + i][the same k] (B), c, e in
//     0 .. 3: four 16-byte loads (8-byte for 16-bit weights, widened in registers) cover one 128-byte line of a row, and MFMA (c, e)
//     multiplies k = kb + 8 c + e and kb + 8 c + 4 + e.  Stream tile t of NT = ceil(B / 32) has its own 16-register accumulator;
//     rows past N and streams past B are clamped duplicates that are computed and never stored (a column of the product depends on
//     its own stream only: NaN / Inf of one stream stay in its row);
//   * the next block's weights and first-tile activations are requested before the current block's MFMAs, the next stream tile's
//     activations (L2 hits: the activations are a few hundred KB) before the current tile's;
//   * the 4 wave partials meet in LDS and are added in wave order; with KS == 1 bias / exact GELU / residual follow at once,
//     otherwise the tile's partial goes to part[split][B][N] and lm_streams_reduce_kernel adds the splits in split order and applies
//     the epilogue.  No atomics anywhere: two calls give equal bits.
// LayerNorm is a pass of its own in front (lm_layernorm_rows_kernel: one wave per stream).
// Sizes: the kernel itself needs K % 32 == 0 (whole 32-k blocks; any N >= 1, 1 <= B <= 128).  The exported omnitok_lm_gemm_streams asks
// for K % 256 == 0 only because its small batches go to the VALU kernels, which need that; the engine's K is n_embd or 4 n_embd with
// n_embd % 256 == 0 (omnitok_lm_create).
constexpr int LMS_NW = 4;
int g_lm_streams_min = 17;  // "lm_streams_min": the smallest number of streams that takes lm_gemm_streams_kernel (engine steps and
                            // omnitok_lm_gemm_streams); below it the VALU kernels serve the streams in groups of 8 / 4 / 2 / 1

template <typename WT, int NT>
__global__ __launch_bounds__(LMS_NW * 64) void lm_gemm_streams_kernel(const float *__restrict__ x, const WT *__restrict__ w,
                                                                       const float *__restrict__ bias, const float *residual,
                                                                       float *y, float *__restrict__ part, int B, int N, int K,
                                                                       int act, int KS) {
    __shared__ float red[LMS_NW][32][33];  // [wave][stream of the tile][weight row] (+1: the writes stride over streams)
    typedef typename LmW<WT>::quad wquad;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 31, h = lane >> 5;
    const int n0 = blockIdx.x * 32, split = blockIdx.y;
    const int nblk = K >> 5, slices = KS * LMS_NW, slice = split * LMS_NW + wave;
    const int b_begin = (int)((int64_t)slice * nblk / slices), b_end = (int)((int64_t)(slice + 1) * nblk / slices);
    const WT *wp = w + (int64_t)(n0 + i < N ? n0 + i : N - 1) * K + 4 * h;
    const float *xp[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) xp[t] = x + (int64_t)(t * 32 + i < B ? t * 32 + i : B - 1) * K + 4 * h;
    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
    // plain loads, not nontemporal ones: a lane pair takes 32 bytes of a row's 128-byte line per instruction, so the line has to stay
    // in the cache for the three loads that follow
    wquad wq[4], wn[4];
    f32x4 x0[4], x0n[4];  // the first stream tile's activations of this block / the next one
    if (b_begin < b_end) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            wq[c] = *reinterpret_cast<const wquad *>(wp + b_begin * 32 + 8 * c);
            x0[c] = *reinterpret_cast<const f32x4 *>(xp[0] + b_begin * 32 + 8 * c);
        }
    }
    for (int blk = b_begin; blk < b_end; ++blk) {
        const int kb = blk * 32, kn = (blk + 1 < b_end ? blk + 1 : blk) * 32;  // (the last block asks for itself again: no branch)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            wn[c] = *reinterpret_cast<const wquad *>(wp + kn + 8 * c);
            x0n[c] = *reinterpret_cast<const f32x4 *>(xp[0] + kn + 8 * c);
        }
        f32x4 wf[4], xq[2][4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            wf[c] = LmW<WT>::widen(wq[c]);
            xq[0][c] = x0[c];
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if (t + 1 < NT) {
#pragma unroll
                for (int c = 0; c < 4; ++c) xq[(t + 1) & 1][c] = *reinterpret_cast<const f32x4 *>(xp[t + 1] + kb + 8 * c);
            }
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[c][e], xq[t & 1][c][e], acc[t], 0, 0, 0);
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            wq[c] = wn[c];
            x0[c] = x0n[c];
        }
    }
    // acc[t][r] of lane (i, h): weight row n0 + mfma32_row(r, h), stream 32 t + i
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if (t) __syncthreads();  // the previous tile was read
#pragma unroll
        for (int r = 0; r < 16; ++r) red[wave][i][mfma32_row(r, h)] = acc[t][r];
        __syncthreads();
        for (int o = tid; o < 32 * 32; o += LMS_NW * 64) {
            const int j = o >> 5, ii = o & 31, b = t * 32 + j, n = n0 + ii;
            float v = ((red[0][j][ii] + red[1][j][ii]) + red[2][j][ii]) + red[3][j][ii];
            if (b < B && n < N) {
                if (KS > 1) {
                    part[((int64_t)split * B + b) * N + n] = v;
                } else {
                    if (bias) v += bias[n];
                    if (act == 1) v = gelu_erf(v);
                    if (residual) v += residual[(int64_t)b * N + n];
                    y[(int64_t)b * N + n] = v;
                }
            }
        }
    }
}

// y = act(part[0] + part[1] + ... + part[KS - 1] + bias) (+ residual), the splits in split order; residual may alias y
__global__ __launch_bounds__(256) void lm_streams_reduce_kernel(const float *__restrict__ part, const float *__restrict__ bias,
                                                                const float *residual, float *y, int64_t total, int N, int KS,
                                                                int act) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= total) return;
    float v = part[o];
    for (int s = 1; s < KS; ++s) v += part[(int64_t)s * total + o];
    if (bias) v += bias[(int)(o % N)];
    if (act == 1) v = gelu_erf(v);
    if (residual) v += residual[o];
    y[o] = v;
}

// K splits across workgroups: enough workgroups for two per CU of a 256-CU device while a wave keeps at least 4 blocks of 32 k.
// A function of (N, K) ONLY -- not of B, not of the device: the bits of an output do not depend on who shares its batch.
static int lm_streams_ksplit(int N, int K) {
    const int tiles = (N + 31) / 32, nblk = K / 32;
    int ks = 512 / tiles, cap = nblk / (LMS_NW * 4);
    if (cap > 16) cap = 16;
    if (ks > cap) ks = cap;
    return ks < 1 ? 1 : ks;
}
// floats of split partials a call needs (0: the epilogue runs inside the GEMM kernel)
int64_t lm_streams_part_floats(int B, int N, int K) {
    const int ks = lm_streams_ksplit(N, K);
    return ks > 1 ? (int64_t)ks * B * N : 0;
}

template <typename WT>
static void lm_streams_launch(const float *x, const WT *w, const LmLinear &c, float *part, hipStream_t stream) {
    const float *bias = c.bias, *residual = c.residual;
    float *y = c.y;
    const int B = c.B, N = c.N, K = c.K, act = c.act;
    const int KS = lm_streams_ksplit(N, K);
    const dim3 grid((N + 31) / 32, KS);
#define OT_LMS(NT_)                                                                                                          \
    hipLaunchKernelGGL((lm_gemm_streams_kernel<WT, NT_>), grid, dim3(LMS_NW * 64), 0, stream, x, w, bias, residual, y, part, B, N, K, \
                       act, KS)
    switch ((B + 31) / 32) {
        case 1: OT_LMS(1); break;
        case 2: OT_LMS(2); break;
        case 3: OT_LMS(3); break;
        default: OT_LMS(4); break;
    }
#undef OT_LMS
    if (KS > 1) {
        const int64_t total = (int64_t)B * N;
        hipLaunchKernelGGL(lm_streams_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, part, bias, residual,
                           y, total, N, KS, act);
    }
}

int lm_gemm_streams_any(const LmLinear &c, float *xn, float *part, hipStream_t stream) {
    const float *x = c.x;
    if (c.ln_g) {
        if (int rc = lm_layernorm_rows(x, c.ln_g, c.ln_b, xn, nullptr, 0, c.B, c.K, nullptr, stream)) return rc;
        x = xn;
    }
    lm_with_wt(c.w, [&](auto *w) { lm_streams_launch(x, w, c, part, stream); });
    OT_LAUNCH_CHECK("lm_gemm_streams");
    return OMNITOK_OK;
}

}  // namespace omnitok

using namespace omnitok;

// process-wide grow-only scratch of omnitok_lm_gemm_streams (an engine has its own): normalised activations | split partials
static std::mutex g_streams_ws_mu;
static float *g_streams_ws = nullptr;
static int64_t g_streams_ws_bytes = 0;
static int g_streams_ws_dev = -1;

extern "C" int omnitok_lm_gemm_streams(const float *x, const void *w, int fmt, const float *bias, const float *residual,
                                       const float *ln_gamma, const float *ln_beta, float *y, int B, int N, int K, int act,
                                       omnitok_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    OT_CHECK_ARG(fmt == OMNITOK_LM_W_FP32 || fmt == OMNITOK_LM_W_BF16 || fmt == OMNITOK_LM_W_FP16,
                 "lm_gemm_streams: fmt %d (OMNITOK_LM_W_FP32 | OMNITOK_LM_W_BF16 | OMNITOK_LM_W_FP16)", fmt);
    OT_CHECK_ARG(x && w && y, "lm_gemm_streams: null pointer");
    const LmMat m{fmt == OMNITOK_LM_W_FP32 ? static_cast<const float *>(w) : nullptr, fmt == OMNITOK_LM_W_FP32 ? nullptr : w, fmt};
    const LmLinear c{x, m, bias, residual, ln_gamma, ln_beta, y, B, N, K, act};
    if (int rc = lm_linear_check("lm_gemm_streams", 128, c, true)) return rc;
    if (B < g_lm_streams_min)  // the VALU kernels, in groups of 8 / 4 / 2 / 1 streams
        return lm_gemv_any(c, nullptr, stream);
    const int64_t xn_floats = ln_gamma ? (int64_t)B * K : 0, need = xn_floats + lm_streams_part_floats(B, N, K);
    std::lock_guard<std::mutex> lk(g_streams_ws_mu);
    int dev = 0;
    OT_HIP(hipGetDevice(&dev));
    if (need > 0) {
        if (g_streams_ws_dev != dev) g_streams_ws_bytes = 0;  // another device's memory: never reused, whatever its size
        if (int rc = lm_grow(reinterpret_cast<void **>(&g_streams_ws), &g_streams_ws_bytes, need * 4)) return rc;
        g_streams_ws_dev = dev;
    }
    return lm_gemm_streams_any(c, g_streams_ws, g_streams_ws + xn_floats, stream);
}
