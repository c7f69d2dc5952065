// Tiled attention on the fp32-input MFMA: the one body of lm_attn_prefill_kernel (causal, csrc/lm_attn_prefill.hip) and
// dit_attn_kernel (non-causal, csrc/dit_attn.hip), and the geometry constants that lm_attn_prefill16_kernel and both host sides share.
//
// A workgroup of 4 waves owns one (stream, head, TA_BQ = 128 query block), a wave 32 of its query rows; the K/V rows of the stream are
// staged in LDS TA_KT = 32 keys at a time, ONCE for the 128 queries, and both products run on v_mfma_f32_32x32x2_f32 (fp32 in, fp32
// accumulate: bit for bit an fmaf chain in k order, no rounding an fmaf does not have).
//
//   S^T = K . Q^T   A = K tile (lane (key, hi) supplies K[key][8u + 4hi + e]), B = Q (lane (query, hi) holds Q[query][8u + 4hi + e] in
//                   HD / 2 registers for the whole block).  The dot product of one score is ONE chain from 0 over the dims in the order
//                   0 4 1 5 2 6 3 7 | 8 12 ...: HD / 2 k-steps.  `scale` (the caller's own rounding of hd^-0.5) multiplies the finished dot.
//   C/D map         register r of lane (query, hi) is key (r & 3) + 8 (r >> 2) + 4 hi of the tile (mfma32_row): a lane holds 16 keys of
//                   ITS query, so the row max / sum is in-lane plus one v_permlane32_swap (halves_max / halves_sum, both halves get
//                   the same bits), and register r is as it stands the B operand of
//   O^T += V^T . P^T  with the key pair (mfma32_row(r, 0), mfma32_row(r, 1)) as the MFMA's two k: P never leaves its registers.  Per
//                   output element the 32 keys of a tile are added in the fixed order 0 4 1 5 2 6 3 7 | 8 12 ..., tiles ascending.
//   online softmax  over key tiles of 32, ascending, anchored at key 0 of the stream; expf in fp32; the keys a query does not see are
//                   -inf before the max; out = O / l, one division per element.
//   mask            CAUSAL: the keys after the query's position.  Only the wave's diagonal tile has any; a wave skips the tiles above
//                   it (it still helps to stage them for the waves below it), and the workgroup's tiles end at its last query's.
//                   Otherwise: the keys past T - 1, in the last of the ceil(T / 32) tiles.  Every tile a wave multiplies has at least
//                   one key its queries see, so the max stays finite.
//   head_dim        any multiple of 8.  O has its dims in NDB = ceil(HD / 32) blocks of 32, and the V image in LDS is NDB * 32 columns
//                   wide.  Where HD is no multiple of 32 (72: the third block is one quarter live) the dead columns are written ONCE
//                   with zeros and never staged, so the dead lanes of the last block multiply zeros -- not the neighbouring head's V,
//                   which is what lies behind column HD - 1 in memory -- and the store skips them; the last staging step of a thread
//                   is guarded.  At a multiple of 32 all of that folds away at compile time.
//
// LDS: Ks[32][HD + 4] (16 consecutive keys' b128 reads cover the 64 banks once: the row stride is 4 mod 8 dwords), Vs[32][NDB * 32 + 4].
// Registers at HD = 72: 36 of Q, 48 of O, 16 of S, 24 of prefetch; at 128: 64, 64, 16, 32.  The callers' __launch_bounds__(256, 2) budget
// of 256 holds them without scratch (build.py's ISA report counts scratch instructions).
//
// No atomics on the result, no split over keys across workgroups, no partials tensor.
//
// What row (b, t) depends on: t, and rows b*T .. b*T + kmax of qkv, kmax = min(32 (t / 32) + 31, T - 1) if CAUSAL, else T - 1 -- not B,
// T (CAUSAL), the stream's slot or another stream (the tile rows past T are clamped duplicates of row T - 1: masked keys, queries that
// are computed and never stored).
// One limit: a masked key still enters the P.V MFMA, with weight exactly 0.  0 * v only ever changes the sign of a zero sum -- unless v
// is not finite: CAUSAL, a NaN / Inf in the V of row u makes rows 32 (u / 32) .. u - 1 of the same stream NaN.  (Not CAUSAL, every row
// of a stream reads every V row of it anyway, and a clamped duplicate is a copy of row T - 1.)
#pragma once
#include "common.h"

#include <cmath>

namespace omnitok {

constexpr int TA_BQ = 128;  // query rows per workgroup (4 waves x 32)
constexpr int TA_KT = 32;   // keys per tile: the width of one online-softmax step

// qkv [B * T, 3C] with C = n_head * HD; blockIdx.x = b * n_head + h; qb: the workgroup's query block (the caller's block order).
// store(i, o): the caller's write of the f32x4 o, elements i .. i + 3 of out [B * T, C].  Call it from __launch_bounds__(256, 2)
// kernels of 256 threads, once.
template <int HD, bool CAUSAL, typename Store>
__device__ __forceinline__ void attn_f32_tiled(const float *__restrict__ qkv, int T, int n_head, int qb, float scale, Store store) {
    constexpr int LDK = HD + 4;          // LDS row stride of K in floats
    constexpr int NU = HD / 8;           // f32x4 of Q per lane
    constexpr int NDB = (HD + 31) / 32;  // 32-dim blocks of O
    constexpr int LDV = NDB * 32 + 4;    // LDS row stride of V
    constexpr int C4 = HD / 4;           // f32x4 per K / V row
    constexpr int NLD = (TA_KT * C4 + 255) / 256;          // f32x4 per thread, matrix and tile
    constexpr bool WHOLE = NLD * 256 == TA_KT * C4;        // else the last one is guarded
    static_assert(HD % 8 == 0, "a lane holds whole f32x4 of Q");
    __shared__ __attribute__((aligned(16))) float Ks[TA_KT * LDK];
    __shared__ __attribute__((aligned(16))) float Vs[TA_KT * LDV];

    const int b = blockIdx.x / n_head, h = blockIdx.x - b * n_head;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r32 = lane & 31, hi = lane >> 5;
    const int C = n_head * HD;
    const float *base = qkv + (int64_t)b * T * 3 * C + h * HD;  // row t of this stream and head: base + t * 3C (q), + C (k), + 2C (v)
    const int q0 = qb * TA_BQ + wave * 32;                      // first query of the wave
    const int tq = q0 + r32;                                    // this lane's query position
    const int nkt = (CAUSAL ? min(qb * TA_BQ + TA_BQ - 1, T - 1) : T - 1) / TA_KT + 1;  // key tiles of the workgroup
    const int mkt = CAUSAL ? q0 / TA_KT : nkt - 1;              // the wave's last tile, the one with masked keys: the diagonal / the tail
    const int kmax = CAUSAL ? tq : T - 1;                       // the last key this lane's query sees
    const bool wave_active = q0 < T;

    if constexpr (NDB * 32 > HD) {  // the dead columns of the V image: zeros, written once (the first barrier of the loop orders them)
        constexpr int PADW = NDB * 32 - HD;
        for (int id = tid; id < TA_KT * PADW; id += 256) Vs[(id / PADW) * LDV + HD + id % PADW] = 0.0f;
    }

    f32x4 qf[NU];
    {
        const float *qrow = base + (int64_t)min(tq, T - 1) * 3 * C + 4 * hi;
#pragma unroll
        for (int u = 0; u < NU; ++u) qf[u] = *reinterpret_cast<const f32x4 *>(qrow + 8 * u);
    }
    f32x4 rk[NLD], rv[NLD];
    auto gload = [&](int kt) {
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int id = tid + 256 * j;
            if (WHOLE || id < TA_KT * C4) {
                const int key = id / C4, c4 = id - key * C4;
                const float *krow = base + (int64_t)min(kt * TA_KT + key, T - 1) * 3 * C + C + c4 * 4;
                rk[j] = *reinterpret_cast<const f32x4 *>(krow);
                rv[j] = *reinterpret_cast<const f32x4 *>(krow + C);
            }
        }
    };
    auto lstore = [&]() {
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int id = tid + 256 * j;
            if (WHOLE || id < TA_KT * C4) {
                const int key = id / C4, c4 = id - key * C4;
                *reinterpret_cast<f32x4 *>(Ks + key * LDK + c4 * 4) = rk[j];
                *reinterpret_cast<f32x4 *>(Vs + key * LDV + c4 * 4) = rv[j];
            }
        }
    };

    f32x16 ot[NDB];
#pragma unroll
    for (int d = 0; d < NDB; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) ot[d][r] = 0.0f;
    float m_run = -INFINITY, l_run = 0.0f;

    gload(0);
    for (int kt = 0; kt < nkt; ++kt) {
        if (kt > 0) __syncthreads();  // every wave is done with the tile before
        lstore();
        __syncthreads();
        if (kt + 1 < nkt) gload(kt + 1);  // in flight under this tile's MFMAs
        if (!wave_active || (CAUSAL && kt > mkt)) continue;  // wave-uniform: no query / above the diagonal (the barriers above are still taken)
        // ---- S^T = K . Q^T for 32 keys x 32 queries
        f32x16 st;
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] = 0.0f;
        const float *kp = Ks + r32 * LDK + 4 * hi;
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const f32x4 kf = *reinterpret_cast<const f32x4 *>(kp + 8 * u);
#pragma unroll
            for (int e = 0; e < 4; ++e) st = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[e], qf[u][e], st, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] *= scale;
        if (kt == mkt) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (kt * TA_KT + mfma32_row(r, hi) > kmax) st[r] = -INFINITY;
        }
        // ---- online softmax: the lane's 16 keys, then the other half's
        float mx = st[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) mx = fmaxf(mx, st[r]);
        mx = halves_max(mx);
        const float m_new = fmaxf(m_run, mx);
        float ps = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            st[r] = expf(st[r] - m_new);
            ps += st[r];
        }
        ps = halves_sum(ps);
        if (__any(m_new != m_run)) {  // wave-uniform; exact: the factor is expf(0) = 1 for a lane whose max stayed
            const float alpha = expf(m_run - m_new);  // 0 on the first tile (m_run = -inf)
            l_run *= alpha;
#pragma unroll
            for (int d = 0; d < NDB; ++d)
#pragma unroll
                for (int r = 0; r < 16; ++r) ot[d][r] *= alpha;
        }
        l_run += ps;
        m_run = m_new;
        // ---- O^T += V^T . P^T: step r takes the keys mfma32_row(r, 0) and mfma32_row(r, 1)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float *vrow = Vs + mfma32_row(r, hi) * LDV + r32;
#pragma unroll
            for (int d = 0; d < NDB; ++d) ot[d] = __builtin_amdgcn_mfma_f32_32x32x2f32(vrow[32 * d], st[r], ot[d], 0, 0, 0);
        }
    }

    // ---- out[q][d] = O^T[d][q] / l; the lane owns query tq and dims 32 db + 8 g + 4 hi + (0 .. 3)
    if (tq >= T) return;
    const int64_t o0 = ((int64_t)b * T + tq) * C + h * HD + 4 * hi;
#pragma unroll
    for (int d = 0; d < NDB; ++d)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            if (32 * d + 8 * g >= HD) continue;  // compile-time: the dead part of the last block (HD % 8 == 0: a group is live or dead as a whole)
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = ot[d][4 * g + e] / l_run;
            store(o0 + 32 * d + 8 * g, o);
        }
}

}  // namespace omnitok
