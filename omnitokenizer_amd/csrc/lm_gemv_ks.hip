// LM decode: the K-sliced GEMV kernel, its shape selection and its LM_TRACE slots (index of the units: lm_common.h)
#include "lm_common.h"
#include "gemm_x_common.h"  // gelu_erf, x3_rsrc

namespace omnitok {

// K-sliced GEMV (r05; B <= 2, K = NW * CW * 256): wave w of a workgroup owns columns [w * CW * 256, (w + 1) * CW * 256) of EVERY row the
// workgroup computes, so its slice of the activations lives in registers (no LDS staging, no panel barriers), a row's 6 (or 8) KiB
// are one contiguous request of the workgroup, and the grid is exactly one workgroup per CU with N / grid rows each.
// Per row: lane dot over its CW float4 -> wave sum -> one LDS word per (row, wave); one barrier at the end, then the first rows x BQ
// threads add the NW wave sums in wave order and apply bias / GELU / residual.
// What the timeline of a decode step (tools/r05/lm_timeline.py, profiles/r05_lm_timeline.txt) taught this kernel:
//   * loads return in order: what the prologue needs (activations, LayerNorm weights, the attention partials) is requested BEFORE the
//     weights, or it arrives behind 96 KiB of them;
//   * no load sits inside a branch -- not a uniform one either: at the join the compiler's counter model only knows "something may
//     be pending" and waits for vmcnt(0), i.e. for every weight in flight.  Short row groups clamp their row index instead (the
//     duplicate requests are L2 hits), bias / residual are loaded by every thread from a clamped index;
//   * the barriers order LDS only (lds_barrier): __syncthreads() drains vmcnt as well.
// Sums N = 2^k values over the 64 lanes of a wave in N - 1 + (6 - k) exchanges instead of 6 N: every halving step keeps half of the
// values (which half: one bit of the lane index, from bit 5 down) and adds the partner lane's copy of the kept half.  On return a[0] of
// lane l is the wave total of value (l >> (6 - k)); lanes with equal (l >> (6 - k)) hold the same total.
// partner lane's value for exchange distance S: DPP inside a row of 16 (S <= 8; S = 4 pairs lane j with j ^ 7, which differs in bit 2 --
// all a halving step needs), the LDS crossbar across rows
template <int S>
__device__ __forceinline__ float wave_xchg(float v) {
    if constexpr (S == 1) return dpp_f32<0xB1>(v);        // quad_perm [1, 0, 3, 2]
    else if constexpr (S == 2) return dpp_f32<0x4E>(v);   // quad_perm [2, 3, 0, 1]
    else if constexpr (S == 4) return dpp_f32<0x141>(v);  // row_half_mirror
    else if constexpr (S == 8) return dpp_f32<0x128>(v);  // row_ror:8
    else return __shfl_xor(v, S);
}
template <int N, int S>
__device__ __forceinline__ void wave_transpose_step(float (&a)[N], int lane, int n) {  // n live values -> n / 2
    const bool up = (lane & S) != 0;
    const int half = n >> 1;
#pragma unroll
    for (int i = 0; i < N / 2; ++i) {
        if (i < half) {
            const float keep = up ? a[i + half] : a[i], send = up ? a[i] : a[i + half];
            a[i] = keep + wave_xchg<S>(send);
        }
    }
}
template <int N>
__device__ __forceinline__ void wave_transpose_sum(float (&a)[N], int lane) {
    static_assert(N >= 1 && N <= 64 && (N & (N - 1)) == 0, "power of two");
    if constexpr (N >= 2) wave_transpose_step<N, 32>(a, lane, N);
    if constexpr (N >= 4) wave_transpose_step<N, 16>(a, lane, N / 2);
    if constexpr (N >= 8) wave_transpose_step<N, 8>(a, lane, N / 4);
    if constexpr (N >= 16) wave_transpose_step<N, 4>(a, lane, N / 8);
    if constexpr (N >= 32) wave_transpose_step<N, 2>(a, lane, N / 16);
    if constexpr (N >= 64) wave_transpose_step<N, 1>(a, lane, N / 32);
    // the 64 / N lanes that now hold partial sums of the same value: plain all-reduce (any pairing)
    if constexpr (N <= 32) a[0] += wave_xchg<1>(a[0]);
    if constexpr (N <= 16) a[0] += wave_xchg<2>(a[0]);
    if constexpr (N <= 8) a[0] += wave_xchg<4>(a[0]);
    if constexpr (N <= 4) a[0] += wave_xchg<8>(a[0]);
    if constexpr (N <= 2) a[0] += wave_xchg<16>(a[0]);
    if constexpr (N <= 1) a[0] += wave_xchg<32>(a[0]);
}

#ifndef LM_TRACE
#define LM_TRACE 0  // 1: s_memrealtime stamps per workgroup (tools/r05/lm_timeline.py; build with OMNITOK_EXTRA_FLAGS=-DLM_TRACE=1)
#endif
template <typename WT, int BQ, int CW, int RG, int ACT, bool LN, bool XM, int NW>
__global__ __launch_bounds__(NW * 64) void lm_gemv_ks_kernel(const float *__restrict__ x, const WT *__restrict__ w,
                                                             const float *__restrict__ bias, const float *residual,
                                                             const float *__restrict__ g, const float *__restrict__ beta,
                                                             float *y, int N, int K, LmMerge mg, long long *trace,
                                                             const float *__restrict__ scale) {
    // scale [N]: the row scales of an fp8 matrix (WT = lm_fp8), multiplied onto the finished dot product in front of the bias (powers
    // of two: exact); no other instantiation reads it
    constexpr bool W8 = __is_same(WT, lm_fp8);
    extern __shared__ float ks_part[];  // [rows of this workgroup][BQ][NW]
    auto stamp = [&](int k) {
        if constexpr (LM_TRACE)
            if (trace && threadIdx.x == 0) trace[(int64_t)blockIdx.x * 8 + k] = __builtin_amdgcn_s_memrealtime();
    };
    stamp(0);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r_begin = (int)((int64_t)blockIdx.x * N / gridDim.x), r_end = (int)((int64_t)(blockIdx.x + 1) * N / gridDim.x);
    const int nrows = r_end - r_begin, ngroups = (nrows + RG - 1) / RG;
    const int col0 = wave * CW * 256 + lane * 4;  // + cw * 256
    // the workgroup's rows through a buffer descriptor that ends with them: a request past the last row (short last group, the
    // prefetch of the groups after the last) returns zeros without touching memory -- no branch, no wasted traffic.  aux = 2: nt
    typedef typename LmW<WT>::quad wquad;
    constexpr int ES = (int)sizeof(WT);  // bytes per weight
    const auto w_rs = x3_rsrc(w + (int64_t)r_begin * K, nrows * K * ES);
    const int w_vo = col0 * ES;
    auto load_w = [&](wquad (&dst)[RG][CW], int grp) {
#pragma unroll
        for (int r = 0; r < RG; ++r)
#pragma unroll
            for (int cw = 0; cw < CW; ++cw)
                // the row offset rides in the VECTOR offset: that operand (+ the instruction offset) is what the descriptor's range
                // check covers on every generation; an soffset is documented as outside it on some
                dst[r][cw] = LmW<WT>::load(w_rs, w_vo + ((grp * RG + r) * K + cw * 256) * ES);
    };
    wquad wa[RG][CW], wb[RG][CW];
    f32x4 xr[BQ][CW];
    // the finishing thread of output (row r, stream b) is thread r * BQ + b; every thread loads from a clamped index
    const int fr = tid / BQ < nrows ? tid / BQ : nrows - 1, fb = tid % BQ, fn = r_begin + fr;
    const float *w_any = reinterpret_cast<const float *>(w);  // (a valid address for the loads whose value is not used)
    const float *bias_p = bias ? bias + fn : w_any, *res_p = residual ? residual + (int64_t)fb * N + fn : w_any;
    float e_bias, e_res, e_scale = 1.0f;
    // ---- this wave's slice of the activations -> registers, then the weights of the first two row groups ----
    if constexpr (XM) {
        // merged attention partials (see lm_gemv_kernel): every lane merges the head its 4 columns belong to.  The partials of the
        // first XC chunks (1024 or 2048 keys) are requested before the weights, whether or not they hold keys (selected afterwards: their
        // addresses exist for every launch); only contexts beyond that take a second round of loads behind the weights.
        constexpr int XC = BQ <= 2 ? 8 : 2;  // (registers: 6 per chunk, stream and column group)
        const int S = 2 + mg.hd;
        const float *p0[BQ][CW];  // this head's partials: [M, L, o[hd]] per chunk
        int dd[CW];
        float Mc[BQ][CW][XC], Lc[BQ][CW][XC];
        f32x4 qc[BQ][CW][XC];
        int used[BQ];
#pragma unroll
        for (int b = 0; b < BQ; ++b) {
            used[b] = mg.cache_len[b];
#pragma unroll
            for (int cw = 0; cw < CW; ++cw) {
                const int col = col0 + cw * 256, h = col / mg.hd;
                dd[cw] = col - h * mg.hd;
                p0[b][cw] = mg.part + ((int64_t)b * mg.n_head + h) * mg.nchunk * S;
#pragma unroll
                for (int c = 0; c < XC; ++c) {
                    const float *pc = p0[b][cw] + (c < mg.nchunk ? c : mg.nchunk - 1) * S;
                    Mc[b][cw][c] = pc[0];
                    Lc[b][cw][c] = pc[1];
                    qc[b][cw][c] = f32x4{pc[2 + dd[cw]], pc[3 + dd[cw]], pc[4 + dd[cw]], pc[5 + dd[cw]]};
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);  // the requests above go out first (the scheduler otherwise hoists the address-ready weight loads)
        load_w(wa, 0);
        load_w(wb, 1);
        e_bias = *bias_p;
        e_res = *res_p;
        if constexpr (W8) e_scale = scale[fn];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int b = 0; b < BQ; ++b) {
            int nu = (used[b] + 1 + mg.chunk - 1) / mg.chunk;
            if (nu > mg.nchunk) nu = mg.nchunk;
#pragma unroll
            for (int cw = 0; cw < CW; ++cw) {
                const float *pb = p0[b][cw];
                float M = Mc[b][cw][0];
#pragma unroll
                for (int c = 1; c < XC; ++c) M = c < nu ? fmaxf(M, Mc[b][cw][c]) : M;
                for (int c = XC; c < nu; ++c) M = fmaxf(M, pb[c * S]);
                float L = 0.0f;
                L += Lc[b][cw][0] * expf(Mc[b][cw][0] - M);
#pragma unroll
                for (int c = 1; c < XC; ++c) L += c < nu ? Lc[b][cw][c] * expf(Mc[b][cw][c] - M) : 0.0f;
                for (int c = XC; c < nu; ++c) L += pb[c * S + 1] * expf(pb[c * S] - M);
                const float f0 = expf(Mc[b][cw][0] - M) / L;
                f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
                v[0] += qc[b][cw][0][0] * f0;
                v[1] += qc[b][cw][0][1] * f0;
                v[2] += qc[b][cw][0][2] * f0;
                v[3] += qc[b][cw][0][3] * f0;
#pragma unroll
                for (int c = 1; c < XC; ++c) {
                    if (c < nu) {  // (no loads inside: a select of registers)
                        const float f = expf(Mc[b][cw][c] - M) / L;
                        v[0] += qc[b][cw][c][0] * f;
                        v[1] += qc[b][cw][c][1] * f;
                        v[2] += qc[b][cw][c][2] * f;
                        v[3] += qc[b][cw][c][3] * f;
                    }
                }
                for (int c = XC; c < nu; ++c) {
                    const float f = expf(pb[c * S] - M) / L;
                    const float *q = pb + c * S + 2 + dd[cw];
                    v[0] += q[0] * f;
                    v[1] += q[1] * f;
                    v[2] += q[2] * f;
                    v[3] += q[3] * f;
                }
                xr[b][cw] = v;
            }
        }
    } else {
        f32x4 g4[CW], b4[CW];
        constexpr bool WAVE_LN = LN && BQ * NW * CW <= 16;  // statistics per wave over the whole row (while it fits registers) | LDS partials
        f32x4 xf[WAVE_LN ? BQ : 1][WAVE_LN ? NW * CW : 1];
        if constexpr (WAVE_LN) {
#pragma unroll
            for (int b = 0; b < BQ; ++b)
#pragma unroll
                for (int c = 0; c < NW * CW; ++c) xf[b][c] = *reinterpret_cast<const f32x4 *>(x + (int64_t)b * K + c * 256 + lane * 4);
        }
#pragma unroll
        for (int cw = 0; cw < CW; ++cw) {
#pragma unroll
            for (int b = 0; b < BQ; ++b) xr[b][cw] = *reinterpret_cast<const f32x4 *>(x + (int64_t)b * K + col0 + cw * 256);
            if constexpr (LN) {
                g4[cw] = *reinterpret_cast<const f32x4 *>(g + col0 + cw * 256);
                b4[cw] = *reinterpret_cast<const f32x4 *>(beta + col0 + cw * 256);
            }
        }
        __builtin_amdgcn_sched_barrier(0);  // the requests above go out first (the scheduler otherwise hoists the address-ready weight loads)
        load_w(wa, 0);
        load_w(wb, 1);
        e_bias = *bias_p;
        e_res = *res_p;
        if constexpr (W8) e_scale = scale[fn];
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (WAVE_LN) {
            // nn.LayerNorm, two-pass like ATen.  Every wave reduces the WHOLE row itself (xf: NW * CW float4 per lane, L2 hits for all but
            // the first wave to ask) instead of exchanging wave partials through LDS (no workgroup barrier in the prologue)
#pragma unroll
            for (int b = 0; b < BQ; ++b) {
                f32x4 t = xf[b][0];
#pragma unroll
                for (int c = 1; c < NW * CW; ++c) t = t + xf[b][c];
                const float mean = wave_allsum((t[0] + t[1]) + (t[2] + t[3])) / (float)K;
                float q = 0.0f;
#pragma unroll
                for (int c = 0; c < NW * CW; ++c) {
                    const f32x4 a = xf[b][c] - mean;
                    q += (a[0] * a[0] + a[1] * a[1]) + (a[2] * a[2] + a[3] * a[3]);
                }
                const float rstd = 1.0f / sqrtf(wave_allsum(q) / (float)K + 1e-5f);
#pragma unroll
                for (int cw = 0; cw < CW; ++cw)
#pragma unroll
                    for (int e = 0; e < 4; ++e) xr[b][cw][e] = (xr[b][cw][e] - mean) * rstd * g4[cw][e] + b4[cw][e];
            }
        } else if constexpr (LN) {
            // more streams than whole rows fit the registers of: wave sums of the slices -> LDS -> every thread adds the NW partials
            __shared__ float s_red[2][BQ][NW];
            float part[BQ];
#pragma unroll
            for (int b = 0; b < BQ; ++b) {
                f32x4 t = xr[b][0];
#pragma unroll
                for (int cw = 1; cw < CW; ++cw) t = t + xr[b][cw];
                part[b] = (t[0] + t[1]) + (t[2] + t[3]);
            }
            wave_transpose_sum<BQ>(part, lane);
            if ((lane & (64 / BQ - 1)) == 0) s_red[0][lane / (64 / BQ)][wave] = part[0];
            lds_barrier();
            float mean[BQ];
#pragma unroll
            for (int b = 0; b < BQ; ++b) {
                float tot = 0.0f;
#pragma unroll
                for (int w8 = 0; w8 < NW; ++w8) tot += s_red[0][b][w8];
                mean[b] = tot / (float)K;
                float q = 0.0f;
#pragma unroll
                for (int cw = 0; cw < CW; ++cw) {
                    const f32x4 a = xr[b][cw] - mean[b];
                    q += (a[0] * a[0] + a[1] * a[1]) + (a[2] * a[2] + a[3] * a[3]);
                }
                part[b] = q;
            }
            wave_transpose_sum<BQ>(part, lane);
            if ((lane & (64 / BQ - 1)) == 0) s_red[1][lane / (64 / BQ)][wave] = part[0];
            lds_barrier();
#pragma unroll
            for (int b = 0; b < BQ; ++b) {
                float tot = 0.0f;
#pragma unroll
                for (int w8 = 0; w8 < NW; ++w8) tot += s_red[1][b][w8];
                const float rstd = 1.0f / sqrtf(tot / (float)K + 1e-5f);
#pragma unroll
                for (int cw = 0; cw < CW; ++cw)
#pragma unroll
                    for (int e = 0; e < 4; ++e) xr[b][cw][e] = (xr[b][cw][e] - mean[b]) * rstd * g4[cw][e] + b4[cw][e];
            }
        }
    }
    stamp(1);
    // ---- rows, RG at a time, two groups of weights in flight ----
    auto consume = [&](const wquad (&wv)[RG][CW], int grp) {
        float acc[RG * BQ];
#pragma unroll
        for (int r = 0; r < RG; ++r) {
            f32x4 wf[CW];  // widened once, used by every stream
#pragma unroll
            for (int cw = 0; cw < CW; ++cw) wf[cw] = LmW<WT>::widen(wv[r][cw]);
#pragma unroll
            for (int b = 0; b < BQ; ++b) {
                float a = 0.0f;
#pragma unroll
                for (int cw = 0; cw < CW; ++cw) {
                    a = fmaf(wf[cw][0], xr[b][cw][0], a);
                    a = fmaf(wf[cw][1], xr[b][cw][1], a);
                    a = fmaf(wf[cw][2], xr[b][cw][2], a);
                    a = fmaf(wf[cw][3], xr[b][cw][3], a);
                }
                acc[r * BQ + b] = a;
            }
        }
        wave_transpose_sum<RG * BQ>(acc, lane);  // lane l: the wave's sum for (row, stream) number l / (64 / (RG BQ))
        constexpr int LPV = 64 / (RG * BQ);      // lanes per value
        const int id = lane / LPV, r = id / BQ;
        if ((lane & (LPV - 1)) == 0 && grp * RG + r < nrows) ks_part[((grp * RG) * BQ + id) * NW + wave] = acc[0];
    };
    for (int grp = 0; grp < ngroups; grp += 2) {
        consume(wa, grp);
        if (grp == 0) stamp(2);
        load_w(wa, grp + 2);
        consume(wb, grp + 1);  // past the last group: nothing is written
        load_w(wb, grp + 3);
    }
    stamp(3);
    lds_barrier();
    if (tid < nrows * BQ) {
        float v = 0.0f;
#pragma unroll
        for (int w8 = 0; w8 < NW; ++w8) v += ks_part[(fr * BQ + fb) * NW + w8];
        if constexpr (W8) v *= e_scale;
        if (bias) v += e_bias;
        if (ACT == 1) v = gelu_erf(v);
        if (residual) v += e_res;
        y[(int64_t)fb * N + fn] = v;
    }
    if constexpr (LM_TRACE) {
        __builtin_amdgcn_s_waitcnt(0);
        stamp(4);
    }
}

int g_lm_ks_deep = 0;   // "lm_ks_deep": weights in flight per wave of the K-sliced GEMV: 1 = 16 KiB | 0 = 8 KiB
int g_lm_ksliced = 2;  // "lm_ksliced": 2 = lm_gemv_ks_kernel for K in {1536, 2048, 6144, 8192} | 1 = only for B <= 2 | 0 = lm_gemv_kernel

extern long long *g_gemm_trace;
static int g_lm_trace_launch = 0;  // launches since the trace buffer was set (omnitok_debug_set_gemm_trace resets it through lm_trace_reset)
void lm_trace_reset() { g_lm_trace_launch = 0; }
static long long *lm_trace_slot(int grid) {  // 8 stamps per workgroup, 1024 workgroups per launch slot, 256 slots
    if (!g_gemm_trace || g_lm_trace_launch >= 256 || grid > 1024) return nullptr;
    return g_gemm_trace + (int64_t)(g_lm_trace_launch++) * 1024 * 8;
}

// 16-bit weights in the K-sliced kernel keep the fp32 form's rows per group: 4 KiB of weights in flight per wave.  Doubling the rows
// per group (8 KiB, the fp32 form's bytes) measured SLOWER at every batch size -- bf16 decode step at 1 / 2 / 4 / 8 streams
// 0.737 / 0.856 / 0.972 / 1.311 ms against 0.708 / 0.792 / 0.855 / 1.160 ms, fp32 0.849 / 0.918 / 1.010 / 1.268 ms in the same session
// (the A/B lines of profiles/lm_w16_bench.json): the transpose-sum of 64 accumulators per group outweighs the deeper queue.
// true: launched | false: not a shape of this kernel (B, K, the rows per workgroup), nothing launched
template <int BQ, int ACT, bool LN, bool XM, typename WT>
static bool launch_gemv_ks(const WT *w, const LmLinear &c, const LmMerge &mg, hipStream_t stream) {
    const int N = c.N, K = c.K;
    int n_cu = 256;
    (void)current_device_cus(&n_cu);
    if (BQ <= 2 ? g_lm_ksliced >= 1 : g_lm_ksliced >= 2) {
        // K-sliced kernel: one workgroup per CU (more only when a workgroup would own more than 64 rows or 384 outputs)
        int mult = 1;  // workgroups per CU: 2 and 3 measured 7 % and 15 % slower per token (every workgroup repeats the prologue)
        while (N / (n_cu * mult) > 64 / (BQ > 4 ? 2 : 1)) ++mult;
        while (mult > 1 && N < n_cu * mult) --mult;
        const int grid = n_cu * mult;
        const int max_rows = (N + grid - 1) / grid + 1;
        if (N >= grid && max_rows * BQ <= 6 * 64) {
            const int lds = max_rows * BQ * 8 * 4;
            constexpr bool W16 = sizeof(WT) < 4;  // a packed format: bf16 / fp16, or the fp8 image (1 KiB per row group and chunk; not A/B'd)
#define OT_KS1(CW_, RG_, NW_)                                                                                                        \
    hipLaunchKernelGGL((lm_gemv_ks_kernel<WT, BQ, CW_, RG_, ACT, LN, XM, NW_>), dim3(grid), dim3(NW_ * 64), lds, stream, c.x, w, c.bias, c.residual, \
                       c.ln_g, c.ln_b, c.y, N, K, mg, lm_trace_slot(grid), c.w.scale)
#define OT_KS(CW_, RG_, NW_)                        \
    {                                               \
        if (deep) OT_KS1(CW_, RG_ * DEEP, NW_);     \
        else OT_KS1(CW_, RG_, NW_);                 \
        return true;                                \
    }
            // rows per group: 2 groups in flight per wave = 8 KiB ("lm_ks_deep" 1: 16 KiB, measured slower: profiles/r05_lm_timeline.txt)
            constexpr int DEEP = BQ <= 2 && !W16 ? 2 : 1;  // (the deep variants exist for B <= 2 and fp32 weights only)
            const bool deep = g_lm_ks_deep == 1 && BQ <= 2 && !W16;
            if (K == 6 * 256) OT_KS(1, 4, 6)
            if constexpr (!XM) {  // (the attention merge only feeds the C x C projection)
                if (K == 6 * 4 * 256) OT_KS(4, 1, 6)
                if (K == 8 * 4 * 256) OT_KS(4, 1, 8)
            }
            if (K == 8 * 256) OT_KS(1, 4, 8)
#undef OT_KS
#undef OT_KS1
        }
    }
    return false;
}

bool lm_gemv_ks_try(const LmLinear &c, const LmMerge &mg, bool xm, hipStream_t stream) {
    return lm_with_wt_dq(c.w, [&](auto *w) {
        return lm_with_gemv_cfg(c, xm, [&](auto bq, auto act, auto ln, auto xm_) {
            return launch_gemv_ks<decltype(bq)::value, decltype(act)::value, decltype(ln)::value, decltype(xm_)::value>(w, c, mg, stream);
        });
    });
}

}  // namespace omnitok
