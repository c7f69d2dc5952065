// DiT denoiser: non-causal attention on the fp32-input MFMA (omnitok_dit_attn; index: dit_common.h).
//
// The geometry of lm_attn_prefill_kernel (csrc/lm_attn_prefill.hip) without its causal mask: a workgroup of 4 waves owns one
// (sample, head, 128-query block), a wave 32 of its query rows; the K/V rows of the sample are staged in LDS 32 keys at a time, ONCE
// for the 128 queries, and both products run on v_mfma_f32_32x32x2_f32 (fp32 in, fp32 accumulate).
//
//   S^T = K . Q^T   A = K tile (lane (key, hi) supplies K[key][8u + 4hi + e]), B = Q (lane (query, hi) holds Q[query][8u + 4hi + e] in
//                   HD / 2 registers for the whole block): HD / 2 k-steps, 32 at head_dim 64 and 36 at 72.  scale = hd^-0.5
//                   multiplies the finished dot.
//   C/D map         register r of lane (query, hi) is key mfma32_row(r, hi) of the tile: the row max / sum is in-lane plus one
//                   v_permlane32_swap, and register r is as it stands the B operand of
//   O^T += V^T . P^T  with the key pair (mfma32_row(r, 0), mfma32_row(r, 1)) as the MFMA's two k: P never leaves its registers.
//   online softmax  over key tiles of 32, ascending; expf in fp32; out = O / l, one division per element.
//
// The two things the prefill kernel never needed:
//   key tail        N is any (input_size / p)^2.  The rows of the last tile past N are clamped duplicates of row N - 1; as keys they
//                   are -inf before the max (every tile has at least one real key, so the max stays finite), as queries they are
//                   computed and never stored.  A masked key still enters the P.V MFMA with weight exactly 0.
//   head_dim 72     O has 72 dims in blocks of 32: the third block is one quarter live.  The V image in LDS is NDB * 32 columns wide;
//                   columns 72 .. 95 are written ONCE with zeros and never staged, so the dead lanes of the third block multiply
//                   zeros -- not the neighbouring head's V, which is what lies behind column 71 in memory -- and the store skips them.
//
// LDS: Ks[32][HD + 4] (16 consecutive keys' b128 reads cover the 64 banks once: the row stride is 4 mod 8 dwords at both head
// dims), Vs[32][NDB * 32 + 4]; 18 / 22 KB per workgroup.  Registers at HD = 72: 36 of Q, 48 of O, 16 of S, 24 of prefetch; the
// __launch_bounds__(256, 2) budget of 256 holds them without scratch (build.py's ISA report counts scratch instructions).
//
// No atomics, no split over keys across workgroups.  What row (b, n) depends on: rows b N .. b N + N - 1 of qkv and nothing else.
#include "dit_common.h"

#include <cmath>
#include <type_traits>

namespace omnitok {

constexpr int DA_BQ = 128;  // query rows per workgroup (4 waves x 32)
constexpr int DA_KT = 32;   // keys per tile

template <int HD>
__global__ __launch_bounds__(256, 2) void dit_attn_kernel(const float *__restrict__ qkv, int N, int heads, float *__restrict__ out) {
    constexpr int LDK = HD + 4;
    constexpr int NU = HD / 8;            // f32x4 of Q per lane
    constexpr int NDB = (HD + 31) / 32;   // 32-dim blocks of O
    constexpr int LDV = NDB * 32 + 4;
    constexpr int C4 = HD / 4;            // f32x4 per K / V row
    constexpr int NLD = (DA_KT * C4 + 255) / 256;  // f32x4 per thread, matrix and tile (the last one guarded)
    static_assert(HD % 8 == 0, "a lane holds whole f32x4 of Q");
    __shared__ __attribute__((aligned(16))) float Ks[DA_KT * LDK];
    __shared__ __attribute__((aligned(16))) float Vs[DA_KT * LDV];

    const int b = blockIdx.x / heads, h = blockIdx.x - b * heads;
    const int qb = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r32 = lane & 31, hi = lane >> 5;
    const int C = heads * HD;
    const float *base = qkv + (int64_t)b * N * 3 * C + h * HD;  // row n of this sample and head: base + n * 3C (q), + C (k), + 2C (v)
    const int q0 = qb * DA_BQ + wave * 32;
    const int tq = q0 + r32;
    const int nkt = (N + DA_KT - 1) / DA_KT;
    const bool wave_active = q0 < N;

    if constexpr (NDB * 32 > HD) {  // the dead columns of the V image: zeros, written once (the first barrier of the loop orders them)
        constexpr int PADW = NDB * 32 - HD;
        for (int id = tid; id < DA_KT * PADW; id += 256) Vs[(id / PADW) * LDV + HD + id % PADW] = 0.0f;
    }

    f32x4 qf[NU];
    {
        const float *qrow = base + (int64_t)min(tq, N - 1) * 3 * C + 4 * hi;
#pragma unroll
        for (int u = 0; u < NU; ++u) qf[u] = *reinterpret_cast<const f32x4 *>(qrow + 8 * u);
    }
    f32x4 rk[NLD], rv[NLD];
    auto gload = [&](int kt) {
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int id = tid + 256 * j;
            if (id < DA_KT * C4) {
                const int key = id / C4, c4 = id - key * C4;
                const float *krow = base + (int64_t)min(kt * DA_KT + key, N - 1) * 3 * C + C + c4 * 4;
                rk[j] = *reinterpret_cast<const f32x4 *>(krow);
                rv[j] = *reinterpret_cast<const f32x4 *>(krow + C);
            }
        }
    };
    auto lstore = [&]() {
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int id = tid + 256 * j;
            if (id < DA_KT * C4) {
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
    const float scale = (float)(1.0 / sqrt((double)HD));

    gload(0);
    for (int kt = 0; kt < nkt; ++kt) {
        if (kt > 0) __syncthreads();  // every wave is done with the tile before
        lstore();
        __syncthreads();
        if (kt + 1 < nkt) gload(kt + 1);  // in flight under this tile's MFMAs
        if (!wave_active) continue;       // wave-uniform (the barriers above are still taken)
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
        if (kt == nkt - 1) {  // the key tail
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (kt * DA_KT + mfma32_row(r, hi) >= N) st[r] = -INFINITY;
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
    if (tq >= N) return;
    const int64_t o0 = ((int64_t)b * N + tq) * C + h * HD + 4 * hi;
#pragma unroll
    for (int d = 0; d < NDB; ++d)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            if (32 * d + 8 * g >= HD) continue;  // compile-time: the dead part of the last block (HD % 8 == 0: a group is live or dead as a whole)
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = ot[d][4 * g + e] / l_run;
            *reinterpret_cast<f32x4 *>(out + o0 + 32 * d + 8 * g) = o;
        }
}

}  // namespace omnitok

using namespace omnitok;

extern "C" int omnitok_dit_attn(const float *qkv, int B, int N, int heads, int head_dim, float *out, omnitok_stream_t stream) {
    OT_CHECK_ARG(qkv && out, "dit_attn: null pointer");
    OT_CHECK_ARG(aligned16(qkv) && aligned16(out), "dit_attn: unaligned pointer (16 bytes)");
    OT_CHECK_ARG(head_dim == 64 || head_dim == 72, "dit_attn: head_dim %d (64 | 72)", head_dim);
    OT_CHECK_ARG(B >= 1 && N >= 1 && heads >= 1 && heads <= 1024 && (int64_t)B * heads < (1ll << 31) && N <= 65535 * DA_BQ,
                 "dit_attn: B %d, N %d, heads %d (1 .. 1024)", B, N, heads);
    const dim3 grid((unsigned)(B * heads), (unsigned)((N + DA_BQ - 1) / DA_BQ));
    if (head_dim == 64)
        hipLaunchKernelGGL((dit_attn_kernel<64>), grid, dim3(256), 0, static_cast<hipStream_t>(stream), qkv, N, heads, out);
    else
        hipLaunchKernelGGL((dit_attn_kernel<72>), grid, dim3(256), 0, static_cast<hipStream_t>(stream), qkv, N, heads, out);
    OT_LAUNCH_CHECK("dit_attn");
    return OMNITOK_OK;
}
