// Tiled attention with bf16 / fp16 operands on v_mfma_f32_32x32x16_{bf16,f16}: the body of dit_attn16_kernel (non-causal,
// csrc/dit_attn.hip), in the shape of attn_f32_tiled.h, and the small helpers (pa16_*) it shares with lm_attn_prefill16_kernel
// (csrc/lm_attn_prefill.hip), whose geometry, operand layout and arithmetic this body restates (that kernel keeps its own copy of
// the loop; its header comment is the longer description of the layout).
//
// A workgroup of 4 waves owns one (stream, head, TA_BQ = 128 query block), a wave 32 of its query rows; the K/V rows of the stream are
// staged in LDS TA_KT = 32 keys at a time, ONCE for the 128 queries.  Q, K and V are rounded ONCE to the operand format OP, to nearest
// even (the bits of tensor.to(dtype)), where they are staged -- K and V on their way from the prefetch registers into LDS, Q on its
// way into the B fragments: no packed copy of qkv, no workspace.
//
//   S^T = K . Q^T   A = K tile (lane (key, hi) reads K[key][16 s + 8 hi + (0 .. 7)], one ds_read_b128 of the row-major image), B = Q
//                   (lane (query, hi) holds Q[query][16 s + 8 hi + (0 .. 7)] in NS = ceil(HD / 16) fragments for the whole block).
//                   Products exact, the sum is the MFMA's fp32 accumulation.  The finished dot is multiplied by
//                   fl(log2(e) / sqrt(hd)), one constant rounded once from fp64: hd^-0.5 with the exponential's base change folded in.
//   C/D map         register r of lane (query, hi) is key mfma32_row(r, hi) of the tile, so registers 8 n .. 8 n + 7, rounded to OP,
//                   are as they stand the B fragment of
//   O^T += V^T . P^T  k-step n (n = 0, 1): keys 16 n + 4 hi + {0 .. 3, 8 .. 11}.  P never leaves its registers.  The A fragment of
//                   lane (dim, hi) is two ds_read_b64 of a TRANSPOSED image Vt[dim][key], which the staging threads write after a
//                   4 x 4 transpose in registers (a thread owns 4 keys x 4 dims of V).
//   online softmax  over key tiles of 32, ascending, anchored at key 0 of the stream; running max, sum and rescale in fp32; the keys a
//                   query does not see are -inf before the max.  The weight is v_exp_f32 of the base-2 score difference (documented
//                   error 1 ulp).  l sums the weights BEFORE their rounding; P is rounded once to OP on its way into the MFMA;
//                   out = O / l, one division per element.
//   mask            CAUSAL: the keys after the query's position (the wave's diagonal tile; the tiles above it are skipped).  Otherwise:
//                   the keys past T - 1, in the last of the ceil(T / 32) tiles.  Every tile a wave multiplies has at least one key its
//                   queries see, so the max stays finite.
//   head_dim        any multiple of 8.  Where HD is no multiple of 16 (72: 4 1/2 k-steps of S) the half k-step multiplies ZEROS on both
//                   sides: lane half hi = 1 of Q's last fragment is zero and the columns HD .. HD + 7 of the K image are written once
//                   with zeros; neither is ever loaded -- what lies behind column HD - 1 in memory is the next head, the next section
//                   of the row or the end of the buffer.  Where HD is no multiple of 32 (72: 2 1/4 blocks of O) the dead rows
//                   HD .. 32 NDB - 1 of the transposed V image are written once with zeros, and the store skips the dead dims.  The
//                   products with zeros are exact.  The last staging step of a thread is guarded where 32 keys x HD / 4 f32x4 is no
//                   multiple of 256.  At a multiple of 32 all of that folds away at compile time.
//
// LDS images (16-bit elements): Ks[32][LDK], LDK = 16 NS + 8: 72 elements = 36 dwords at HD 64, 88 elements = 44 dwords at HD 72.  Both
// are 4 mod 8 dwords, so 16 consecutive keys' b128 reads cover the 64 banks once (HD + 8 at 72 would be 40 dwords = 0 mod 8: every
// eighth key on the same banks).  Vt[32 NDB][PA16_LDT = 36] (row stride 18 dwords: the b64 reads of 32 dims cover the 64 banks once).
// 9 / 12.25 KB per workgroup at HD 64 / 72.
// Registers at HD = 72: 20 of Q, 48 of O, 16 of S, 28 of prefetch; dit_attn16_kernel compiles to 118 / 146 VGPRs (bf16 operands, HD 64 /
// 72) and 119 / 162 (fp16: the range checks of the operand roundings), inside the callers' __launch_bounds__(256, 2) budget without
// scratch (build.py's ISA report counts scratch instructions).
//
// No atomics on the result, no split over keys across workgroups, no partials tensor.
// What row (b, t) depends on: as attn_f32_tiled.h -- t, and rows b*T .. b*T + kmax of qkv, not B or another stream (the tile rows
// past T are clamped duplicates of row T - 1: masked keys, queries that are computed and never stored).
// op_inf: set where a FINITE element of Q, K or V rounds to +-inf (fp16 only: dit_round16's convention).
#pragma once
#include "attn_f32_tiled.h"  // TA_BQ, TA_KT
#include "lm_common.h"       // lm_bf16, lm_fp16, lm_round16

namespace omnitok {

constexpr int PA16_LDT = 36;  // row stride of the transposed V image in 16-bit elements

typedef unsigned pa16_u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 pa16_bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 pa16_f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 pa16_bf16x2 __attribute__((ext_vector_type(2)));
typedef float pa16_f32x2 __attribute__((ext_vector_type(2)));

template <typename OP>
__device__ __forceinline__ f32x16 pa16_mfma(const pa16_u32x4 &a, const pa16_u32x4 &b, const f32x16 &c) {
    if constexpr (__is_same(OP, lm_bf16))
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(pa16_bf16x8, a), __builtin_bit_cast(pa16_bf16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(pa16_f16x8, a), __builtin_bit_cast(pa16_f16x8, b), c, 0, 0, 0);
}

// Two fp32 values rounded to OP, packed low | high; inf: an fp16 result of +-inf.  bf16: one v_cvt_pk_bf16_f32 (the compiler's
// conversion of a float pair) instead of two integer roundings of 5 instructions each.  Its bits equal lm_round16<lm_bf16>'s for every
// non-NaN input -- compared over all 2^32 patterns in both halves of the pair on an MI355X, subnormals included; a NaN keeps its
// payload where lm_round16 gives 0x7FC0 (NaN either way).
template <typename OP>
__device__ __forceinline__ unsigned pa16_pack2(float lo, float hi, bool &inf) {
    if constexpr (__is_same(OP, lm_bf16)) {
        return __builtin_bit_cast(unsigned, __builtin_convertvector(pa16_f32x2{lo, hi}, pa16_bf16x2));
    } else {
        const unsigned short a = lm_round16<OP>(lo), b = lm_round16<OP>(hi);
        inf = inf || lm_f16_is_inf(a) || lm_f16_is_inf(b);
        return (unsigned)a | ((unsigned)b << 16);
    }
}

// pa16_pack2 for an operand: `inf` records only a FINITE value that became +-inf (an infinite input is not a range error)
template <typename OP>
__device__ __forceinline__ unsigned a16_pack2(float lo, float hi, bool &inf) {
    bool any = false;
    const unsigned p = pa16_pack2<OP>(lo, hi, any);
    if constexpr (__is_same(OP, lm_fp16))
        if (any)
            inf = inf || (lm_f16_is_inf((unsigned short)p) && fabsf(lo) <= 3.402823466e38f) ||
                  (lm_f16_is_inf((unsigned short)(p >> 16)) && fabsf(hi) <= 3.402823466e38f);
    return p;
}

// qkv [B * T, 3C] with C = n_head * HD; blockIdx.x = b * n_head + h; qb: the workgroup's query block (the caller's block order).
// store(i, o): the caller's write of the f32x4 o, elements i .. i + 3 of out [B * T, C].  Call it from __launch_bounds__(256, 2)
// kernels of 256 threads, once.
template <int HD, bool CAUSAL, typename OP, typename Store>
__device__ __forceinline__ void attn16_tiled(const float *__restrict__ qkv, int T, int n_head, int qb, bool &op_inf, Store store) {
    constexpr int KT = TA_KT, LDT = PA16_LDT;
    constexpr int NS = (HD + 15) / 16;   // k-steps of S: B fragments of Q per lane
    constexpr int LDK = 16 * NS + 8;     // row stride of the K image in 16-bit elements (4 mod 8 dwords at 64 and 72)
    constexpr int NDB = (HD + 31) / 32;  // 32-dim blocks of O
    constexpr int C4 = HD / 4;           // f32x4 per K / V row
    constexpr int NLD = (KT * C4 + 255) / 256;    // f32x4 of K per thread and tile
    constexpr bool WHOLE = NLD * 256 == KT * C4;  // else the last one is guarded
    constexpr int NVU = 8 * C4;                   // threads that stage V: 4 keys x 4 dims each
    constexpr bool HALF = NS * 16 > HD;           // the last k-step of S is half live
    static_assert(HD % 8 == 0 && NVU <= 256, "a lane holds whole halves of a fragment; one V unit per thread");
    static_assert(!HALF || NS * 16 - HD == 8, "the dead part of the last k-step is lane half hi = 1");
    static_assert((LDK / 2) % 8 == 4, "K image row stride: 4 mod 8 dwords");
    __shared__ __attribute__((aligned(16))) unsigned short Ks[KT * LDK];
    __shared__ __attribute__((aligned(16))) unsigned short Vt[NDB * 32 * LDT];

    const int b = blockIdx.x / n_head, h = blockIdx.x - b * n_head;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r32 = lane & 31, hi = lane >> 5;
    const int C = n_head * HD;
    const float *base = qkv + (int64_t)b * T * 3 * C + h * HD;  // row t of this stream and head: base + t * 3C (q), + C (k), + 2C (v)
    const int q0 = qb * TA_BQ + wave * 32;                      // first query of the wave
    const int tq = q0 + r32;                                    // this lane's query position
    const int nkt = (CAUSAL ? min(qb * TA_BQ + TA_BQ - 1, T - 1) : T - 1) / KT + 1;  // key tiles of the workgroup
    const int mkt = CAUSAL ? q0 / KT : nkt - 1;                 // the wave's last tile, the one with masked keys: the diagonal / the tail
    const int kmax = CAUSAL ? tq : T - 1;                       // the last key this lane's query sees
    const bool wave_active = q0 < T;

    // the dead parts of both images: zeros, written once (the first barrier of the loop orders them)
    if constexpr (HALF) {
        if (tid < KT) *reinterpret_cast<pa16_u32x4 *>(Ks + tid * LDK + HD) = pa16_u32x4{0u, 0u, 0u, 0u};
    }
    if constexpr (NDB * 32 > HD) {
        constexpr int DEAD2 = (NDB * 32 - HD) * LDT / 2;  // dwords
        unsigned *dead = reinterpret_cast<unsigned *>(Vt + HD * LDT);
        for (int id = tid; id < DEAD2; id += 256) dead[id] = 0u;
    }

    pa16_u32x4 qf[NS];
    {
        const float *qrow = base + (int64_t)min(tq, T - 1) * 3 * C + 8 * hi;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            if (HALF && s == NS - 1 && hi) {  // dims HD .. HD + 7: zeros, not loaded
                qf[s] = pa16_u32x4{0u, 0u, 0u, 0u};
                continue;
            }
            const f32x4 a = *reinterpret_cast<const f32x4 *>(qrow + 16 * s), c = *reinterpret_cast<const f32x4 *>(qrow + 16 * s + 4);
            qf[s] = pa16_u32x4{a16_pack2<OP>(a[0], a[1], op_inf), a16_pack2<OP>(a[2], a[3], op_inf),
                               a16_pack2<OP>(c[0], c[1], op_inf), a16_pack2<OP>(c[2], c[3], op_inf)};
        }
    }
    // staging: K as the fp32 body (thread: f32x4 number tid + 256 j of the tile); V in units of 4 keys x 4 dims (thread tid < NVU:
    // keys 4 vg .. 4 vg + 3, dims 4 vc .. 4 vc + 3), so that a thread writes four 8-byte runs of the transposed image
    const int vg = tid & 7, vc = tid >> 3;
    const bool stages_v = tid < NVU;
    f32x4 rk[NLD], rv[4];
    auto gload = [&](int kt) {
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int id = tid + 256 * j;
            if (WHOLE || id < KT * C4) {
                const int key = id / C4, c4 = id - key * C4;
                rk[j] = *reinterpret_cast<const f32x4 *>(base + (int64_t)min(kt * KT + key, T - 1) * 3 * C + C + c4 * 4);
            }
        }
        if (stages_v) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                rv[i] = *reinterpret_cast<const f32x4 *>(base + (int64_t)min(kt * KT + 4 * vg + i, T - 1) * 3 * C + 2 * C + vc * 4);
        }
    };
    auto lstore = [&]() {
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int id = tid + 256 * j;
            if (WHOLE || id < KT * C4) {
                const int key = id / C4, c4 = id - key * C4;
                const f32x4 k = rk[j];
                *reinterpret_cast<u32x2 *>(Ks + key * LDK + c4 * 4) = u32x2{a16_pack2<OP>(k[0], k[1], op_inf), a16_pack2<OP>(k[2], k[3], op_inf)};
            }
        }
        if (stages_v) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                *reinterpret_cast<u32x2 *>(Vt + (vc * 4 + e) * LDT + 4 * vg) =
                    u32x2{a16_pack2<OP>(rv[0][e], rv[1][e], op_inf), a16_pack2<OP>(rv[2][e], rv[3][e], op_inf)};
        }
    };

    f32x16 ot[NDB];
#pragma unroll
    for (int d = 0; d < NDB; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) ot[d][r] = 0.0f;
    float m_run = -INFINITY, l_run = 0.0f;
    const float scale2 = (float)(1.4426950408889634 / sqrt((double)HD));  // log2(e) / sqrt(hd), folded at build time

    gload(0);
    for (int kt = 0; kt < nkt; ++kt) {
        if (kt > 0) __syncthreads();  // every wave is done with the tile before
        lstore();
        __syncthreads();
        if (kt + 1 < nkt) gload(kt + 1);  // in flight under this tile's work
        if (!wave_active || (CAUSAL && kt > mkt)) continue;  // wave-uniform: no query / above the diagonal (the barriers above are still taken)
        // ---- S^T = K . Q^T for 32 keys x 32 queries
        f32x16 st;
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] = 0.0f;
        const unsigned short *kp = Ks + r32 * LDK + 8 * hi;
#pragma unroll
        for (int s = 0; s < NS; ++s) st = pa16_mfma<OP>(*reinterpret_cast<const pa16_u32x4 *>(kp + 16 * s), qf[s], st);
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] *= scale2;
        if (kt == mkt) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (kt * KT + mfma32_row(r, hi) > kmax) st[r] = -INFINITY;
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
            st[r] = __builtin_amdgcn_exp2f(st[r] - m_new);
            ps += st[r];
        }
        ps = halves_sum(ps);
        if (__any(m_new != m_run)) {  // wave-uniform; exact: the factor is 2^0 = 1 for a lane whose max stayed
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);  // 0 on the first tile (m_run = -inf)
            l_run *= alpha;
#pragma unroll
            for (int d = 0; d < NDB; ++d)
#pragma unroll
                for (int r = 0; r < 16; ++r) ot[d][r] *= alpha;
        }
        l_run += ps;
        m_run = m_new;
        // ---- O^T += V^T . P^T: k-step n takes registers 8 n .. 8 n + 7, the keys 16 n + 4 hi + {0 .. 3, 8 .. 11}
        bool p_inf = false;  // (a weight is <= 1: never set)
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const pa16_u32x4 pf = {pa16_pack2<OP>(st[8 * n], st[8 * n + 1], p_inf), pa16_pack2<OP>(st[8 * n + 2], st[8 * n + 3], p_inf),
                                   pa16_pack2<OP>(st[8 * n + 4], st[8 * n + 5], p_inf), pa16_pack2<OP>(st[8 * n + 6], st[8 * n + 7], p_inf)};
            const unsigned short *vp = Vt + r32 * LDT + 16 * n + 4 * hi;
#pragma unroll
            for (int d = 0; d < NDB; ++d) {
                const u32x2 lo = *reinterpret_cast<const u32x2 *>(vp + 32 * d * LDT), up = *reinterpret_cast<const u32x2 *>(vp + 32 * d * LDT + 8);
                ot[d] = pa16_mfma<OP>(pa16_u32x4{lo[0], lo[1], up[0], up[1]}, pf, ot[d]);
            }
        }
    }

    // ---- out[q][d] = O^T[d][q] / l; the lane owns query tq and dims 32 db + 8 g + 4 hi + (0 .. 3)
    if (tq >= T) return;
    const int64_t o0 = ((int64_t)b * T + tq) * C + h * HD + 4 * hi;
#pragma unroll
    for (int d = 0; d < NDB; ++d)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            if (32 * d + 8 * g >= HD) continue;  // compile-time: the dead part of the last block
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = ot[d][4 * g + e] / l_run;
            store(o0 + 32 * d + 8 * g, o);
        }
}

}  // namespace omnitok
