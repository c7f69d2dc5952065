// LM prefill: tiled causal attention on the fp32-input MFMA (omnitok_lm_set_prefill_attention(OMNITOK_LM_PA_TILED)),
// omnitok_lm_attn_prefill (index: lm_common.h)
//
// The rows mode of the prefill launches the decode kernel once per query row, head and 256-key chunk: every row re-reads its whole
// K/V prefix and multiplies it on the VALU.  Here a workgroup of 4 waves owns one (stream, head, 128-query block), a wave 32 of its
// query rows; the K/V rows of the stream are staged in LDS 32 keys at a time, ONCE for the 128 queries, and both products run on
// v_mfma_f32_32x32x2_f32 (fp32 in, fp32 accumulate: bit for bit an fmaf chain in k order, no rounding an fmaf does not have).
//
//   S^T = K . Q^T   A = K tile (lane (key, hi) supplies K[key][8u + 4hi + e]), B = Q (lane (query, hi) holds Q[query][8u + 4hi + e] in
//                   HD / 2 registers for the whole block).  The dot product of one score is ONE chain from 0 over the dims in the order
//                   0 4 1 5 2 6 3 7 | 8 12 ...; scale = 1 / sqrtf(hd) multiplies the finished dot, as in lm_attn_decode_kernel.
//   C/D map         register r of lane (query, hi) is key (r & 3) + 8 (r >> 2) + 4 hi of the tile (mfma32_row): a lane holds 16 keys of
//                   ITS query, so the row max / sum is in-lane plus one v_permlane32_swap (halves_max / halves_sum, both halves get
//                   the same bits), and register r is as it stands the B operand of
//   O^T += V^T . P^T  with the key pair (mfma32_row(r, 0), mfma32_row(r, 1)) as the MFMA's two k: P never leaves its registers.  Per
//                   output element the 32 keys of a tile are added in the fixed order 0 4 1 5 2 6 3 7 | 8 12 ..., tiles ascending.
//   online softmax  over key tiles of 32, ascending, anchored at key 0 of the stream; expf in fp32; keys after the query's position
//                   are -inf before the max (only the diagonal tile has any); out = O / l, one division per element.
//
// No atomics on the result, no split over keys across workgroups, no partials tensor.  A wave skips the key tiles above its own
// diagonal (it still helps to stage them for the waves below it); the longest query blocks are launched first.
//
// What row (b, t) depends on: t, and rows b*T .. b*T + min(32 (t / 32) + 31, T - 1) of qkv -- not B, T, the stream's slot or another
// stream (the tile rows past T are clamped duplicates of row T - 1: masked keys, queries that are computed and never stored).
// One limit: a masked key still enters the P.V MFMA, with weight 0.  0 * v only ever changes the sign of a zero sum -- unless v is
// not finite: a NaN / Inf in the V of row u makes rows 32 (u / 32) .. u - 1 of the same stream NaN, where the rows kernel skips it.
#include "lm_common.h"

#include <cmath>

namespace omnitok {

constexpr int PA_BQ = 128;  // query rows per workgroup (4 waves x 32)
constexpr int PA_KT = 32;   // keys per tile: the width of one online-softmax step

template <int HD, typename OT>
__global__ __launch_bounds__(256, 2) void lm_attn_prefill_kernel(const float *__restrict__ qkv, int T, int n_head, OT *__restrict__ out,
                                                              int *__restrict__ flag) {
    constexpr int LD = HD + 4;    // LDS row stride in floats: 16 consecutive keys' b128 reads cover the banks once
    constexpr int NU = HD / 8;    // f32x4 of Q per lane
    constexpr int NDB = HD / 32;  // 32-dim blocks of O
    constexpr int C4 = HD / 4;    // f32x4 per K / V row
    constexpr int NLD = PA_KT * C4 / 256;  // f32x4 per thread, matrix and tile
    static_assert(PA_KT * C4 % 256 == 0, "a tile is a whole number of f32x4 per thread");
    __shared__ __attribute__((aligned(16))) float Ks[PA_KT * LD];
    __shared__ __attribute__((aligned(16))) float Vs[PA_KT * LD];

    const int b = blockIdx.x / n_head, h = blockIdx.x - b * n_head;
    const int qb = (int)gridDim.y - 1 - (int)blockIdx.y;  // long blocks first
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r32 = lane & 31, hi = lane >> 5;
    const int C = n_head * HD;
    const float *base = qkv + (int64_t)b * T * 3 * C + h * HD;  // row t of this stream and head: base + t * 3C (q), + C (k), + 2C (v)
    const int q0 = qb * PA_BQ + wave * 32;                      // first query of the wave
    const int tq = q0 + r32;                                    // this lane's query position
    const int last = min(qb * PA_BQ + PA_BQ - 1, T - 1);
    const int nkt = last / PA_KT + 1;                           // key tiles of the workgroup
    const int diag = q0 / PA_KT;                                // the wave's diagonal tile
    const bool wave_active = q0 < T;

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
            const int id = tid + 256 * j, key = id / C4, c4 = id - key * C4;
            const float *krow = base + (int64_t)min(kt * PA_KT + key, T - 1) * 3 * C + C + c4 * 4;
            rk[j] = *reinterpret_cast<const f32x4 *>(krow);
            rv[j] = *reinterpret_cast<const f32x4 *>(krow + C);
        }
    };
    auto lstore = [&]() {
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int id = tid + 256 * j, key = id / C4, c4 = id - key * C4;
            *reinterpret_cast<f32x4 *>(Ks + key * LD + c4 * 4) = rk[j];
            *reinterpret_cast<f32x4 *>(Vs + key * LD + c4 * 4) = rv[j];
        }
    };

    f32x16 ot[NDB];
#pragma unroll
    for (int d = 0; d < NDB; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) ot[d][r] = 0.0f;
    float m_run = -INFINITY, l_run = 0.0f;
    const float scale = 1.0f / sqrtf((float)HD);

    gload(0);
    for (int kt = 0; kt < nkt; ++kt) {
        if (kt > 0) __syncthreads();  // every wave is done with the tile before
        lstore();
        __syncthreads();
        if (kt + 1 < nkt) gload(kt + 1);  // in flight under this tile's MFMAs
        if (!wave_active || kt > diag) continue;  // wave-uniform: above the diagonal (the barriers above are still taken)
        // ---- S^T = K . Q^T for 32 keys x 32 queries
        f32x16 st;
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] = 0.0f;
        const float *kp = Ks + r32 * LD + 4 * hi;
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const f32x4 kf = *reinterpret_cast<const f32x4 *>(kp + 8 * u);
#pragma unroll
            for (int e = 0; e < 4; ++e) st = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[e], qf[u][e], st, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] *= scale;
        if (kt == diag) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (kt * PA_KT + mfma32_row(r, hi) > tq) st[r] = -INFINITY;
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
            const float *vrow = Vs + mfma32_row(r, hi) * LD + r32;
#pragma unroll
            for (int d = 0; d < NDB; ++d) ot[d] = __builtin_amdgcn_mfma_f32_32x32x2f32(vrow[32 * d], st[r], ot[d], 0, 0, 0);
        }
    }

    // ---- out[q][d] = O^T[d][q] / l; the lane owns query tq and dims 32 db + 8 g + 4 hi + (0 .. 3)
    if (tq >= T) return;
    const int64_t o0 = ((int64_t)b * T + tq) * C + h * HD + 4 * hi;
    bool inf = false;
#pragma unroll
    for (int d = 0; d < NDB; ++d)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = ot[d][4 * g + e] / l_run;
            if constexpr (__is_same(OT, float)) {
                *reinterpret_cast<f32x4 *>(out + o0 + 32 * d + 8 * g) = o;
            } else {
                *reinterpret_cast<u32x2 *>(out + o0 + 32 * d + 8 * g) = LmKV<OT>::store4(o, inf);
            }
        }
    if constexpr (LmKV<OT>::CAN_OVERFLOW)
        if (inf && flag) atomicOr(flag, LM_FLAG_PF16_RANGE);
}

template <typename OT>
static void lm_attn_prefill_launch(const float *qkv, int B, int T, int n_head, int head_dim, OT *out, int *flag, hipStream_t stream) {
    const dim3 grid((unsigned)(B * n_head), (unsigned)((T + PA_BQ - 1) / PA_BQ));
    switch (head_dim) {
        case 64: hipLaunchKernelGGL((lm_attn_prefill_kernel<64, OT>), grid, dim3(256), 0, stream, qkv, T, n_head, out, flag); break;
        case 96: hipLaunchKernelGGL((lm_attn_prefill_kernel<96, OT>), grid, dim3(256), 0, stream, qkv, T, n_head, out, flag); break;
        default: hipLaunchKernelGGL((lm_attn_prefill_kernel<128, OT>), grid, dim3(256), 0, stream, qkv, T, n_head, out, flag); break;
    }
}

int lm_attn_prefill(const float *qkv, int B, int T, int n_head, int head_dim, float *out32, void *out16, int fmt, int *flag,
                    hipStream_t stream) {
    OT_CHECK_ARG(qkv, "lm_attn_prefill: null pointer");
    OT_CHECK_ARG((out32 != nullptr) != (out16 != nullptr), "lm_attn_prefill: exactly one of out32 / out16");
    OT_CHECK_ARG(!out16 || fmt == OMNITOK_LM_W_BF16 || fmt == OMNITOK_LM_W_FP16,
                 "lm_attn_prefill: fmt %d (OMNITOK_LM_W_BF16 | OMNITOK_LM_W_FP16)", fmt);
    OT_CHECK_ARG(aligned16(qkv) && aligned16(out32) && aligned16(out16), "lm_attn_prefill: unaligned pointer (16 bytes)");
    OT_CHECK_ARG((reinterpret_cast<uintptr_t>(flag) & 3) == 0, "lm_attn_prefill: unaligned flag");
    OT_CHECK_ARG(head_dim == 64 || head_dim == 96 || head_dim == 128, "lm_attn_prefill: head_dim %d (64 | 96 | 128)", head_dim);
    OT_CHECK_ARG(B >= 1 && T >= 1 && (int64_t)B * T <= 65535 && n_head >= 1 && n_head <= 1024,
                 "lm_attn_prefill: B %d, T %d (>= 1, B * T <= 65535), n_head %d (1 .. 1024)", B, T, n_head);
    if (out32) lm_attn_prefill_launch<float>(qkv, B, T, n_head, head_dim, out32, nullptr, stream);
    else if (fmt == OMNITOK_LM_W_BF16) lm_attn_prefill_launch<lm_bf16>(qkv, B, T, n_head, head_dim, static_cast<lm_bf16 *>(out16), flag, stream);
    else lm_attn_prefill_launch<lm_fp16>(qkv, B, T, n_head, head_dim, static_cast<lm_fp16 *>(out16), flag, stream);
    OT_LAUNCH_CHECK("lm_attn_prefill");
    return OMNITOK_OK;
}

}  // namespace omnitok

extern "C" int omnitok_lm_attn_prefill(const float *qkv, int B, int T, int n_head, int head_dim, float *out32, void *out16, int fmt,
                                       int *flag, omnitok_stream_t stream) {
    return omnitok::lm_attn_prefill(qkv, B, T, n_head, head_dim, out32, out16, fmt, flag, static_cast<hipStream_t>(stream));
}
