// LM decode: the row GEMV kernel, the loop over groups of streams, omnitok_lm_gemv / _gemv_w16 / _gemv_fp8 (index: lm_common.h)
#include "lm_common.h"
#include "gemm_x_common.h"  // gelu_erf

namespace omnitok {

// One workgroup = 4 waves x ROWS weight rows.  The activations (BQ rows of K floats, a few KB, L2-
// resident) are staged once per workgroup in LDS in panels of LM_KP floats -- layer-normalised on the
// way in when LN -- so the waves only stream weights from HBM: U chunks (256 floats) of each of the
// wave's ROWS rows are in flight while the previous U are multiplied (register double buffer).
//
// attention-merge staging (XM): x is not a tensor but the flash-decode chunk partials of
// lm_attn_decode_kernel; the workgroup merges them while it stages its activations, so the chunked
// attention needs neither a merge launch nor cross-workgroup fences.
int g_lm_wide_u = 2;  // "lm_wide_u": chunks per register buffer of the wide GEMVs (4 measured slower: 1.134 vs 1.114 ms / token)

template <typename WT, int BQ, int ROWS, int U, int ACT, bool LN, bool XM, int NW>
__global__ __launch_bounds__(NW * 64) void lm_gemv_kernel(const float *__restrict__ x, const WT *__restrict__ w,
                                                      const float *__restrict__ bias, const float *residual,
                                                      const float *__restrict__ g, const float *__restrict__ beta,
                                                      float *y, int N, int K, LmMerge mg, const float *__restrict__ scale) {
    // scale [N]: the row scales of an fp8 matrix (WT = lm_fp8, powers of two: an exact multiplication of the finished dot product in
    // front of the bias); not read by any other instantiation
    extern __shared__ __attribute__((aligned(16))) float xs[];  // [BQ][kp]
    __shared__ float s_mean[BQ], s_rstd[BQ];
    constexpr int NT = NW * 64;  // NW waves per workgroup: the launcher picks NW and ROWS so that the grid is a whole number of
                                 // workgroups per CU (a CU that gets one workgroup more than its neighbour streams that much longer)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row0 = (blockIdx.x * NW + wave) * ROWS;
    const int kp = K < LM_KP ? K : LM_KP;
    const int nch = K >> 8;  // 256-float chunks
    typedef typename LmW<WT>::quad wquad;
    const WT *wr[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) wr[r] = w + (int64_t)(row0 + r < N ? row0 + r : N - 1) * K + lane * 4;
    auto load_w = [&](wquad (&dst)[ROWS][U], int c0) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (c0 + u < nch) {  // uniform; chunks past the row are neither loaded nor consumed
#pragma unroll
                for (int r = 0; r < ROWS; ++r)
                    dst[r][u] = __builtin_nontemporal_load(reinterpret_cast<const wquad *>(wr[r] + (c0 + u) * 256));
            }
        }
    };
    wquad wa[ROWS][U], wb[ROWS][U];
    load_w(wa, 0);  // in flight while the LayerNorm statistics / merge weights are computed
    // LayerNorm with the whole row in one LDS panel (K <= LM_KP, every GPT block): x, gamma and beta are requested
    // together at kernel start (one memory round trip instead of three dependent ones), the two-pass statistics are
    // block-wide reductions over registers, and the normalised row goes straight to LDS.
    const bool ln_fast = LN && K <= LM_KP;
    if (ln_fast) {
        __shared__ float s_part[2][BQ][NW];
        const int k4n = K >> 2;  // float4 per row (<= 512: NJ per thread)
        constexpr int NJ = (LM_KP / 4 + NT - 1) / NT;
        f32x4 xv[BQ][NJ], g4[NJ], b4[NJ];
        const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const bool has = tid + NT * j < k4n;
            g4[j] = has ? *reinterpret_cast<const f32x4 *>(g + (tid + NT * j) * 4) : zero4;
            b4[j] = has ? *reinterpret_cast<const f32x4 *>(beta + (tid + NT * j) * 4) : zero4;
#pragma unroll
            for (int b = 0; b < BQ; ++b)
                xv[b][j] = has ? *reinterpret_cast<const f32x4 *>(x + (int64_t)b * K + (tid + NT * j) * 4) : zero4;
        }
#pragma unroll
        for (int b = 0; b < BQ; ++b) {
            f32x4 t = xv[b][0];
#pragma unroll
            for (int j = 1; j < NJ; ++j) t = t + xv[b][j];
            const float sum = wave_allsum((t[0] + t[1]) + (t[2] + t[3]));
            if (lane == 0) s_part[0][b][wave] = sum;
        }
        lds_barrier();  // LDS traffic only: __syncthreads() would also wait for every weight load in flight
        float mean[BQ];
#pragma unroll
        for (int b = 0; b < BQ; ++b) {
            float tot = 0.0f;
            if constexpr (NW == 4) tot = (s_part[0][b][0] + s_part[0][b][1]) + (s_part[0][b][2] + s_part[0][b][3]);
            else
#pragma unroll
                for (int w8 = 0; w8 < NW; ++w8) tot += s_part[0][b][w8];
            mean[b] = tot / (float)K;
            float q = 0.0f;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                if (tid + NT * j < k4n) {
                    const f32x4 a = xv[b][j] - mean[b];
                    q += (a[0] * a[0] + a[1] * a[1]) + (a[2] * a[2] + a[3] * a[3]);
                }
            }
            q = wave_allsum(q);
            if (lane == 0) s_part[1][b][wave] = q;
        }
        lds_barrier();  // LDS traffic only: __syncthreads() would also wait for every weight load in flight
#pragma unroll
        for (int b = 0; b < BQ; ++b) {
            float tot = 0.0f;
            if constexpr (NW == 4) tot = (s_part[1][b][0] + s_part[1][b][1]) + (s_part[1][b][2] + s_part[1][b][3]);
            else
#pragma unroll
                for (int w8 = 0; w8 < NW; ++w8) tot += s_part[1][b][w8];
            const float var = tot / (float)K;
            const float rstd = 1.0f / sqrtf(var + 1e-5f);
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                if (tid + NT * j < k4n) {
                    f32x4 v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = (xv[b][j][e] - mean[b]) * rstd * g4[j][e] + b4[j][e];
                    *reinterpret_cast<f32x4 *>(xs + b * kp + (tid + NT * j) * 4) = v;
                }
            }
        }
    } else if (LN) {
        // nn.LayerNorm statistics (two-pass, like ATen): wave w owns activation rows w and w + 4
        for (int b = wave; b < BQ; b += NW) {
            float sum = 0.0f;
            for (int k = lane * 4; k < K; k += 256) {
                const f32x4 v = *reinterpret_cast<const f32x4 *>(x + (int64_t)b * K + k);
                sum += (v[0] + v[1]) + (v[2] + v[3]);
            }
            const float mean = wave_allsum(sum) / (float)K;
            float q = 0.0f;
            for (int k = lane * 4; k < K; k += 256) {
                const f32x4 v = *reinterpret_cast<const f32x4 *>(x + (int64_t)b * K + k);
                const float a0 = v[0] - mean, a1 = v[1] - mean, a2 = v[2] - mean, a3 = v[3] - mean;
                q += (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
            }
            const float var = wave_allsum(q) / (float)K;
            if (lane == 0) {
                s_mean[b] = mean;
                s_rstd[b] = 1.0f / sqrtf(var + 1e-5f);
            }
        }
    }
    float acc[ROWS][BQ];
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
#pragma unroll
        for (int b = 0; b < BQ; ++b) acc[r][b] = 0.0f;

    auto consume = [&](const wquad (&wv)[ROWS][U], int c0, int cbase) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (c0 + u < nch) {
                const int off = (c0 + u - cbase) * 256 + lane * 4;
                f32x4 wf[ROWS];  // widened once, used by every stream
#pragma unroll
                for (int r = 0; r < ROWS; ++r) wf[r] = LmW<WT>::widen(wv[r][u]);
#pragma unroll
                for (int b = 0; b < BQ; ++b) {
                    const f32x4 xv = *reinterpret_cast<const f32x4 *>(xs + b * kp + off);
#pragma unroll
                    for (int r = 0; r < ROWS; ++r) {
                        acc[r][b] = fmaf(wf[r][0], xv[0], acc[r][b]);
                        acc[r][b] = fmaf(wf[r][1], xv[1], acc[r][b]);
                        acc[r][b] = fmaf(wf[r][2], xv[2], acc[r][b]);
                        acc[r][b] = fmaf(wf[r][3], xv[3], acc[r][b]);
                    }
                }
            }
        }
    };

    constexpr int CPP = LM_KP / 256;  // chunks per panel (a multiple of 2 * U)
    for (int p0 = 0; p0 < nch; p0 += CPP) {
        lds_barrier();  // LDS traffic only: __syncthreads() would also wait for every weight load in flight  // previous panel fully consumed (and s_mean / s_rstd / s_f visible)
        const int pk = (nch - p0 < CPP ? nch - p0 : CPP) * 256;  // floats in this panel
        for (int i = tid * 4; i < BQ * pk && !ln_fast; i += NT * 4) {
            const int b = i / pk, k = i - b * pk;
            f32x4 v;
            if (XM) {
                // every staging thread merges its own head: global max over the chunks that hold keys, then
                // f_c = e^(M_c - M) / sum_c L_c e^(M_c - M).  Chunk 0 always holds keys, so its partial is requested
                // together with cache_len: up to 256 cached tokens the whole merge is one memory round trip (the
                // per-head weight table in LDS, its three dependent passes and its barrier are gone).
                const int col = p0 * 256 + k, h = col / mg.hd, d = col - h * mg.hd;  // hd % 4 == 0: one head per float4
                const int S = 2 + mg.hd;
                const float *pp = mg.part + ((int64_t)b * mg.n_head + h) * mg.nchunk * S;
                const float M0 = pp[0], L0 = pp[1];
                const float q00 = pp[2 + d], q01 = pp[3 + d], q02 = pp[4 + d], q03 = pp[5 + d];
                int used = (mg.cache_len[b] + 1 + mg.chunk - 1) / mg.chunk;
                if (used > mg.nchunk) used = mg.nchunk;  // a stream stepped past max_len (flagged by the attention kernel,
                                                         // which clamps the same way): never read past this head's partials
                float M = M0;
                for (int c = 1; c < used; ++c) M = fmaxf(M, pp[c * S]);
                float L = 0.0f;
                L += L0 * expf(M0 - M);
                for (int c = 1; c < used; ++c) L += pp[c * S + 1] * expf(pp[c * S] - M);
                const float f0 = expf(M0 - M) / L;
                v = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                v[0] += q00 * f0;
                v[1] += q01 * f0;
                v[2] += q02 * f0;
                v[3] += q03 * f0;
                for (int c = 1; c < used; ++c) {
                    const float f = expf(pp[c * S] - M) / L;
                    const float *q = pp + c * S + 2 + d;
                    v[0] += q[0] * f;
                    v[1] += q[1] * f;
                    v[2] += q[2] * f;
                    v[3] += q[3] * f;
                }
            } else {
                v = *reinterpret_cast<const f32x4 *>(x + (int64_t)b * K + p0 * 256 + k);
            }
            if (LN) {
                const f32x4 g4 = *reinterpret_cast<const f32x4 *>(g + p0 * 256 + k);
                const f32x4 b4 = *reinterpret_cast<const f32x4 *>(beta + p0 * 256 + k);
                const float mean = s_mean[b], rstd = s_rstd[b];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = (v[e] - mean) * rstd * g4[e] + b4[e];
            }
            *reinterpret_cast<f32x4 *>(xs + b * kp + k) = v;
        }
        lds_barrier();  // LDS traffic only: __syncthreads() would also wait for every weight load in flight
        const int pend = p0 + CPP < nch ? p0 + CPP : nch;
        for (int c0 = p0; c0 < pend; c0 += 2 * U) {
            load_w(wb, c0 + U);  // may belong to the next panel: only the weights are prefetched
            consume(wa, c0, p0);
            if (c0 + U < pend) {
                load_w(wa, c0 + 2 * U);
                consume(wb, c0 + U, p0);
            } else {
                // wb holds the first group of the next panel: rotate it into wa
#pragma unroll
                for (int r = 0; r < ROWS; ++r)
#pragma unroll
                    for (int u = 0; u < U; ++u) wa[r][u] = wb[r][u];
            }
        }
    }
    if (row0 >= N) return;
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
#pragma unroll
        for (int b = 0; b < BQ; ++b) acc[r][b] = wave_allsum(acc[r][b]);
    // lane (r * BQ + b) finishes and stores output (b, row0 + r)
    float mine = 0.0f;
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
#pragma unroll
        for (int b = 0; b < BQ; ++b)
            if (lane == r * BQ + b) mine = acc[r][b];
    if (lane < ROWS * BQ) {
        const int r = lane / BQ, b = lane % BQ, n = row0 + r;
        if (n < N) {
            float v = mine;
            if constexpr (__is_same(WT, lm_fp8)) v *= scale[n];
            if (bias) v += bias[n];
            if (ACT == 1) v = gelu_erf(v);
            if (residual) v += residual[(int64_t)b * N + n];
            y[(int64_t)b * N + n] = v;
        }
    }
}

// "lm_mfma": 0 (default) = the VALU kernels | 1 = groups of 4 .. 8 streams take lm_gemm4_kernel when K / 512 is 3, 4, 12 or 16.
// Measured (profiles/r06_lm_mfma.txt): 8 streams 1.73 - 1.83 ms per decode step against 1.42 ms for the VALU kernels -- the one-burst
// form pays transfer + compute in series (13 - 14 us per GEMV whatever its bytes) where the K-sliced VALU kernel overlaps them, and
// the merged attention output costs a launch of its own; correct (tests) and kept as an A/B arm, not the default.
int g_lm_mfma = 0;
int g_lm_balance = 1;  // "lm_balance": 1 = waves per workgroup and rows per wave chosen so that every CU gets the same number of
                       // workgroups | 0 = 4 waves, 1 row (N <= 2048) or 2 rows per wave

template <int BQ, int ROWS, int U, int ACT, bool LN, bool XM, int NW, typename WT>
static void launch_gemv_cfg(const WT *w, const LmLinear &c, const LmMerge &mg, hipStream_t stream) {
    const int kp = c.K < LM_KP ? c.K : LM_KP;
    const int lds = BQ * kp * 4;
    const int rows_per_wg = NW * ROWS;
    if (lds > 65536) (void)set_max_dynamic_lds(reinterpret_cast<const void *>(lm_gemv_kernel<WT, BQ, ROWS, U, ACT, LN, XM, NW>), lds);
    hipLaunchKernelGGL((lm_gemv_kernel<WT, BQ, ROWS, U, ACT, LN, XM, NW>), dim3((c.N + rows_per_wg - 1) / rows_per_wg), dim3(NW * 64),
                       lds, stream, c.x, w, c.bias, c.residual, c.ln_g, c.ln_b, c.y, c.N, c.K, mg, c.w.scale);
}

template <int BQ, int ACT, bool LN, bool XM, typename WT>
static void launch_gemv_rows(const WT *w, const LmLinear &c, const LmMerge &mg, hipStream_t stream) {
    // ROWS weight rows x U chunks (x2 register buffers) per wave = 8 KiB of fp32 weights in flight per wave.  The 16-bit
    // instantiations keep ROWS and U (4 KiB in flight; 2 KiB of fp8): the row kernel serves no GEMV of the reference's LM, it was taken as it is
    // and not A/B'd -- the rows-per-group A/B (lm_gemv_ks.hip) is about the K-sliced kernel only.
    // Narrow outputs (N <= 2048: the C x C and C x 4C projections) take one row per wave so that the
    // launch still covers every CU.  Wide outputs: 2 rows x 2 chunks x 2 buffers per wave, i.e. a whole K = 1536 row pair is
    // requested before the LayerNorm prologue finishes (the matrix streams from HBM while x is normalised).
    // Balance (r05): a decode GEMV lasts 5-10 us and every CU streams at its own ~25-30 GB/s, so the launch takes as long as the
    // CU with the most workgroups: 384 workgroups on 256 CUs (N = 1536 at 4 rows per workgroup) run like 512.  With 6 waves per
    // workgroup N = 1536 is exactly one workgroup per CU and N = 4608 exactly three (profiles/r05_lm_balance.txt).
    int n_cu = 256;
    (void)current_device_cus(&n_cu);
    const int N = c.N, K = c.K;
    auto waste = [&](int rows_per_wg) {  // workgroup slots of the last round that stay empty, as a fraction of the launch
        const int wgs = (N + rows_per_wg - 1) / rows_per_wg;
        const int rounds = (wgs + n_cu - 1) / n_cu;
        return (double)(rounds * n_cu - wgs) / (double)(rounds * n_cu);
    };
    const bool six = g_lm_balance && BQ <= 2 && K % 256 == 0;
    if (N <= 2048) {
        if (six && waste(6) + 0.05 < waste(4)) launch_gemv_cfg<BQ, 1, 4, ACT, LN, XM, 6>(w, c, mg, stream);
        else launch_gemv_cfg<BQ, 1, 4, ACT, LN, XM, 4>(w, c, mg, stream);
    } else if (six && waste(6) + 0.05 < waste(8)) {
        launch_gemv_cfg<BQ, 1, 4, ACT, LN, XM, 6>(w, c, mg, stream);
    } else if (g_lm_wide_u == 2) {
        launch_gemv_cfg<BQ, 2, 2, ACT, LN, XM, 4>(w, c, mg, stream);
    } else {
        launch_gemv_cfg<BQ, 2, 4, ACT, LN, XM, 4>(w, c, mg, stream);
    }
}

int lm_gemv_any(const LmLinear &c, const LmMerge *mg, hipStream_t stream) {
    const int N = c.N, K = c.K;
    for (int b0 = 0; b0 < c.B;) {
        const int left = c.B - b0;
        LmLinear g = c;  // this group's rows
        g.x = c.x ? c.x + (int64_t)b0 * K : nullptr;
        g.residual = c.residual ? c.residual + (int64_t)b0 * N : nullptr;
        g.y = c.y + (int64_t)b0 * N;
        LmMerge m2{nullptr, nullptr, 0, 0, 0, LM_CHUNK};  // this group's partials
        if (mg) {
            m2 = *mg;
            m2.part += (int64_t)b0 * mg->n_head * mg->nchunk * (2 + mg->hd);
            m2.cache_len += b0;
        }
        const bool mfma_k = K == 1536 || K == 2048 || (!c.ln_g && (K == 6144 || K == 8192));
        if (g_lm_mfma && !c.w.w16 && !c.w.w8 && left >= 4 && mfma_k && N >= 16 && (int64_t)N * K < (1ll << 29) && (!mg || mg->merged)) {
            // 4 .. 8 streams in one pass over the weights on the matrix cores (lm_gemm4_kernel)
            g.B = left > 8 ? 8 : left;
            if (mg) {   // the merged attention output as a tensor first (the VALU path merges inside its prologue)
                float *merged = mg->merged + (int64_t)b0 * K;
                lm_attn_merge(m2.part, m2.cache_len, mg->n_head, mg->hd, mg->nchunk, 0, merged, nullptr, 0, g.B, nullptr, mg->chunk, stream);
                g.x = merged;
            }
            if (lm_gemm4_try(g, stream)) {
                OT_LAUNCH_CHECK("lm_gemm4");
                b0 += g.B;
                continue;
            }
        }
        g.B = left >= 8 ? 8 : (left >= 4 ? 4 : (left >= 2 ? 2 : 1));
        // the K-sliced kernel where it has the shape, the row kernel for every other
        if (!lm_gemv_ks_try(g, m2, mg != nullptr, stream))
            lm_with_wt_dq(g.w, [&](auto *w) {
                lm_with_gemv_cfg(g, mg != nullptr, [&](auto bq, auto act, auto ln, auto xm) {
                    launch_gemv_rows<decltype(bq)::value, decltype(act)::value, decltype(ln)::value, decltype(xm)::value>(w, g, m2, stream);
                });
            });
        OT_LAUNCH_CHECK("lm_gemv");
        b0 += g.B;
    }
    return OMNITOK_OK;
}

int lm_linear_check(const char *who, int bmax, const LmLinear &c, bool y16) {
    OT_CHECK_ARG(c.B > 0 && c.B <= bmax && c.N > 0 && c.K > 0 && c.K % 256 == 0,
                 bmax > 16 ? "%s: bad sizes B=%d N=%d K=%d (1 <= B <= %d, K %% 256 == 0)" : "%s: bad sizes B=%d N=%d K=%d", who, c.B, c.N,
                 c.K, bmax);
    OT_CHECK_ARG((c.ln_g != nullptr) == (c.ln_b != nullptr), "%s: ln_gamma / ln_beta must come together", who);
    OT_CHECK_ARG(c.act == 0 || c.act == 1, "%s: act %d", who, c.act);
    OT_CHECK_ARG(aligned16(c.x) && aligned16(c.w.w8 ? c.w.w8 : c.w.w16 ? c.w.w16 : c.w.w32) && (!y16 || aligned16(c.y)), "%s: unaligned", who);
    return OMNITOK_OK;
}

}  // namespace omnitok

using namespace omnitok;

extern "C" int omnitok_lm_gemv(const float *x, const float *w, const float *bias, const float *residual,
                               const float *ln_gamma, const float *ln_beta, float *y, int B, int N, int K, int act,
                               omnitok_stream_t stream_) {
    if (B == 0) return OMNITOK_OK;
    OT_CHECK_ARG(x && w && y, "lm_gemv: null pointer");
    const LmLinear c{x, {w, nullptr, OMNITOK_LM_W_FP32}, bias, residual, ln_gamma, ln_beta, y, B, N, K, act};
    if (int rc = lm_linear_check("lm_gemv", 16, c, false)) return rc;
    return lm_gemv_any(c, nullptr, static_cast<hipStream_t>(stream_));
}

extern "C" int omnitok_lm_gemv_w16(const float *x, const void *w16, int fmt, const float *bias, const float *residual,
                                   const float *ln_gamma, const float *ln_beta, float *y, int B, int N, int K, int act,
                                   omnitok_stream_t stream_) {
    OT_CHECK_ARG(fmt == OMNITOK_LM_W_BF16 || fmt == OMNITOK_LM_W_FP16, "lm_gemv_w16: fmt %d (OMNITOK_LM_W_BF16 | OMNITOK_LM_W_FP16)", fmt);
    OT_CHECK_ARG(x && w16 && y, "lm_gemv_w16: null pointer");
    if (B == 0) return OMNITOK_OK;
    const LmLinear c{x, {nullptr, w16, fmt}, bias, residual, ln_gamma, ln_beta, y, B, N, K, act};
    if (int rc = lm_linear_check("lm_gemv_w16", 16, c, false)) return rc;
    return lm_gemv_any(c, nullptr, static_cast<hipStream_t>(stream_));
}

extern "C" int omnitok_lm_gemv_fp8(const float *x, const void *q8, const float *scale, const float *bias, const float *residual,
                                   const float *ln_gamma, const float *ln_beta, float *y, int B, int N, int K, int act,
                                   omnitok_stream_t stream_) {
    OT_CHECK_ARG(x && q8 && scale && y, "lm_gemv_fp8: null pointer");
    if (B == 0) return OMNITOK_OK;
    const LmLinear c{x, {nullptr, nullptr, OMNITOK_LM_W_FP32, q8, scale}, bias, residual, ln_gamma, ln_beta, y, B, N, K, act};
    if (int rc = lm_linear_check("lm_gemv_fp8", 16, c, false)) return rc;
    return lm_gemv_any(c, nullptr, static_cast<hipStream_t>(stream_));
}
