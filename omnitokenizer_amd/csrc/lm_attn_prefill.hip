// LM prefill: tiled causal attention (omnitok_lm_set_prefill_attention(OMNITOK_LM_PA_TILED)) on the fp32-input MFMA, omnitok_lm_attn_prefill,
// or with bf16 / fp16 operands on the 16-bit MFMA (omnitok_lm_set_prefill_attention_operands), omnitok_lm_attn_prefill16: two kernels, one
// geometry and one host side (index: lm_common.h)
//
// The rows mode of the prefill launches the decode kernel once per query row, head and 256-key chunk: every row re-reads its whole
// K/V prefix and multiplies it on the VALU.  Here the K/V rows of a stream are staged once per 128 query rows and both products run on
// the MFMA.  The fp32 kernel is the CAUSAL form of attn_f32_tiled (csrc/attn_f32_tiled.h: the operand layout, the order of every sum,
// what a row depends on and the non-finite-V limit of a masked key are written down there; the rows kernel skips such a key).  What is
// the LM's own: the longest query blocks are launched first, scale = 1 / sqrtf(hd) as in lm_attn_decode_kernel, and the output format.
#include "attn16_tiled.h"
#include "attn_f32_tiled.h"
#include "lm_common.h"

namespace omnitok {

template <int HD, typename OT>
__global__ __launch_bounds__(256, 2) void lm_attn_prefill_kernel(const float *__restrict__ qkv, int T, int n_head, OT *__restrict__ out,
                                                              int *__restrict__ flag) {
    bool inf = false;
    attn_f32_tiled<HD, true>(qkv, T, n_head, (int)gridDim.y - 1 - (int)blockIdx.y /* long blocks first */, 1.0f / sqrtf((float)HD),
                             [&](int64_t i, const f32x4 &o) {
                                 if constexpr (__is_same(OT, float)) {
                                     *reinterpret_cast<f32x4 *>(out + i) = o;
                                 } else {
                                     *reinterpret_cast<u32x2 *>(out + i) = LmKV<OT>::store4(o, inf);
                                 }
                             });
    if constexpr (LmKV<OT>::CAN_OVERFLOW)
        if (inf && flag) atomicOr(flag, LM_FLAG_PF16_RANGE);
}

// ---- bf16 / fp16 operands --------------------------------------------------------------------------------------------------------------
// The tiling above with both products on v_mfma_f32_32x32x16_bf16 / _f16 (16 x the rate of the fp32-input MFMA): the same workgroup of 4
// waves per (stream, head, 128-query block), a wave 32 of its query rows, the K/V rows staged in LDS KT = 32 keys at a time, ONCE for
// the 128 queries.  Q, K and V are rounded ONCE to the operand format OP (pa16_pack2: lm_round16's
// bits) where they are staged -- K and V on their way from the prefetch registers into LDS, Q on its way into the B fragments -- so
// there is no packed copy of qkv and no workspace (a pre-pass that writes a packed qkv16 was not built: it needs [B * T, 3C] 16-bit
// scratch that the building block's signature does not have, and the kernel is 4 x the fp32 one without it).
//
//   S^T = K . Q^T   A = K tile (lane (key, hi) reads K[key][16 s + 8 hi + (0 .. 7)], one ds_read_b128 of the row-major image), B = Q
//                   (lane (query, hi) holds Q[query][16 s + 8 hi + (0 .. 7)] in HD / 16 fragments for the whole block).  The products
//                   are exact (16-bit x 16-bit), the sum is the MFMA's fp32 accumulation.  The finished dot is multiplied by
//                   fl(log2(e) / sqrt(hd)) (one constant, rounded once): the scale with the exponential's base change folded in.
//   C/D map         as the fp32 kernel's: register r of lane (query, hi) is key mfma32_row(r, hi) of the tile, so registers
//                   8 n .. 8 n + 7, rounded to OP, are as they stand the B fragment of
//   O^T += V^T . P^T  k-step n (n = 0, 1): element j of lane half hi stands for key 16 n + 4 hi + (j & 3) + 8 (j >> 2).  P never leaves
//                   its registers.  The A fragment of lane (dim, hi) is V of keys 16 n + 4 hi + {0 .. 3, 8 .. 11} at that dim: two
//                   ds_read_b64 of a TRANSPOSED image Vt[dim][key], which the staging threads write after a 4 x 4 transpose in
//                   registers (a thread owns 4 keys x 4 dims of V).
//   online softmax  over key tiles of KT = 32, ascending, anchored at key 0 of the stream; running max, sum and rescale in fp32; keys
//                   after the query's position are -inf before the max (only the diagonal tile has any).  The weight is
//                   v_exp_f32(s' - m') on the base-2 scores: documented error 1 ulp.  l sums the weights BEFORE their rounding
//                   to OP (fp32 values); P is rounded once (pa16_pack2) on its way into the MFMA; out = O / l, one division.
//
// LDS images (16-bit elements): Ks[32][HD + 8] (16 consecutive keys' b128 reads cover the 64 banks once), Vt[HD][36] (row stride 18
// dwords: the b64 reads of 32 dims cover the 64 banks once; the transposed b64 writes take the 4 passes their 512 bytes need).
//
// No atomics on the result, no split over keys across workgroups, no partials tensor.  What row (b, t) depends on, and the one
// limit (a non-finite V in a masked key of the diagonal tile), are the fp32 kernel's (the head of this file).
// Flags: an fp16 operand (an element of Q, K or V) that rounds to +-inf ORs LM_FLAG_AOP16_RANGE into *flag; an fp16 OUTPUT of +-inf
// LM_FLAG_PF16_RANGE, as the fp32 kernel.  bf16 sets neither.
// PA16_LDT, the pa16_* vector types, pa16_mfma and pa16_pack2: csrc/attn16_tiled.h, shared with the DiT's 16-bit attention body.

template <int HD, typename OP, typename OT>
__global__ __launch_bounds__(256, 2) void lm_attn_prefill16_kernel(const float *__restrict__ qkv, int T, int n_head, OT *__restrict__ out,
                                                                int *__restrict__ flag) {
    constexpr int KT = TA_KT, LDT = PA16_LDT;
    constexpr int LDK = HD + 8;   // row stride of the K image in 16-bit elements
    constexpr int NS = HD / 16;   // k-steps of S: B fragments of Q per lane
    constexpr int NDB = HD / 32;  // 32-dim blocks of O
    constexpr int C4 = HD / 4;    // f32x4 per K / V row
    constexpr int NLD = KT * C4 / 256;  // f32x4 of K per thread and tile
    constexpr int NVU = 8 * C4;         // threads that stage V: 4 keys x 4 dims each
    static_assert(KT * C4 % 256 == 0 && NVU <= 256, "a tile is a whole number of f32x4 per thread");
    __shared__ __attribute__((aligned(16))) unsigned short Ks[KT * LDK];
    __shared__ __attribute__((aligned(16))) unsigned short Vt[HD * LDT];

    const int b = blockIdx.x / n_head, h = blockIdx.x - b * n_head;
    const int qb = (int)gridDim.y - 1 - (int)blockIdx.y;  // long blocks first
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r32 = lane & 31, hi = lane >> 5;
    const int C = n_head * HD;
    const float *base = qkv + (int64_t)b * T * 3 * C + h * HD;  // row t of this stream and head: base + t * 3C (q), + C (k), + 2C (v)
    const int q0 = qb * TA_BQ + wave * 32;                    // first query of the wave
    const int tq = q0 + r32;                                    // this lane's query position
    const int last = min(qb * TA_BQ + TA_BQ - 1, T - 1);
    const int nkt = last / KT + 1;                              // key tiles of the workgroup
    const int diag = q0 / KT;                                   // the wave's diagonal tile
    const bool wave_active = q0 < T;
    bool op_inf = false;  // an fp16 operand rounded to +-inf

    pa16_u32x4 qf[NS];
    {
        const float *qrow = base + (int64_t)min(tq, T - 1) * 3 * C + 8 * hi;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const f32x4 a = *reinterpret_cast<const f32x4 *>(qrow + 16 * s), c = *reinterpret_cast<const f32x4 *>(qrow + 16 * s + 4);
            qf[s] = pa16_u32x4{pa16_pack2<OP>(a[0], a[1], op_inf), pa16_pack2<OP>(a[2], a[3], op_inf),
                               pa16_pack2<OP>(c[0], c[1], op_inf), pa16_pack2<OP>(c[2], c[3], op_inf)};
        }
    }
    // staging: K as the fp32 kernel (thread: f32x4 number tid + 256 j of the tile); V in units of 4 keys x 4 dims (thread tid < NVU:
    // keys 4 vg .. 4 vg + 3, dims 4 vc .. 4 vc + 3), so that a thread writes four 8-byte runs of the transposed image
    const int vg = tid & 7, vc = tid >> 3;
    const bool stages_v = tid < NVU;
    f32x4 rk[NLD], rv[4];
    auto gload = [&](int kt) {
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int id = tid + 256 * j, key = id / C4, c4 = id - key * C4;
            rk[j] = *reinterpret_cast<const f32x4 *>(base + (int64_t)min(kt * KT + key, T - 1) * 3 * C + C + c4 * 4);
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
            const int id = tid + 256 * j, key = id / C4, c4 = id - key * C4;
            const f32x4 k = rk[j];
            *reinterpret_cast<u32x2 *>(Ks + key * LDK + c4 * 4) = u32x2{pa16_pack2<OP>(k[0], k[1], op_inf), pa16_pack2<OP>(k[2], k[3], op_inf)};
        }
        if (stages_v) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                *reinterpret_cast<u32x2 *>(Vt + (vc * 4 + e) * LDT + 4 * vg) =
                    u32x2{pa16_pack2<OP>(rv[0][e], rv[1][e], op_inf), pa16_pack2<OP>(rv[2][e], rv[3][e], op_inf)};
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
        if (!wave_active || kt > diag) continue;  // wave-uniform: above the diagonal (the barriers above are still taken)
        // ---- S^T = K . Q^T for 32 keys x 32 queries
        f32x16 st;
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] = 0.0f;
        const unsigned short *kp = Ks + r32 * LDK + 8 * hi;
#pragma unroll
        for (int s = 0; s < NS; ++s) st = pa16_mfma<OP>(*reinterpret_cast<const pa16_u32x4 *>(kp + 16 * s), qf[s], st);
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] *= scale2;
        if (kt == diag) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (kt * KT + mfma32_row(r, hi) > tq) st[r] = -INFINITY;
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
    if constexpr (__is_same(OP, lm_fp16))
        if (op_inf && flag) atomicOr(flag, LM_FLAG_AOP16_RANGE);

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

// The host side of both kernels.  who: the exported entry the messages name; op_fmt 0: fp32 operands (omnitok_lm_attn_prefill16 refuses
// it before it comes here), else the operand format, and the output format's argument is called out_fmt
int lm_attn_prefill_any(const char *who, const float *qkv, int B, int T, int n_head, int head_dim, int op_fmt, float *out32, void *out16,
                        int out_fmt, int *flag, hipStream_t stream) {
    OT_CHECK_ARG(qkv, "%s: null pointer", who);
    OT_CHECK_ARG(op_fmt == 0 || op_fmt == OMNITOK_LM_W_BF16 || op_fmt == OMNITOK_LM_W_FP16,
                 "%s: op_fmt %d (OMNITOK_LM_W_BF16 | OMNITOK_LM_W_FP16)", who, op_fmt);
    OT_CHECK_ARG((out32 != nullptr) != (out16 != nullptr), "%s: exactly one of out32 / out16", who);
    OT_CHECK_ARG(!out16 || out_fmt == OMNITOK_LM_W_BF16 || out_fmt == OMNITOK_LM_W_FP16,
                 "%s: %s %d (OMNITOK_LM_W_BF16 | OMNITOK_LM_W_FP16)", who, op_fmt ? "out_fmt" : "fmt", out_fmt);
    OT_CHECK_ARG(aligned16(qkv) && aligned16(out32) && aligned16(out16), "%s: unaligned pointer (16 bytes)", who);
    OT_CHECK_ARG((reinterpret_cast<uintptr_t>(flag) & 3) == 0, "%s: unaligned flag", who);
    OT_CHECK_ARG(head_dim == 64 || head_dim == 96 || head_dim == 128, "%s: head_dim %d (64 | 96 | 128)", who, head_dim);
    OT_CHECK_ARG(B >= 1 && T >= 1 && (int64_t)B * T <= 65535 && n_head >= 1 && n_head <= 1024,
                 "%s: B %d, T %d (>= 1, B * T <= 65535), n_head %d (1 .. 1024)", who, B, T, n_head);
    const dim3 grid((unsigned)(B * n_head), (unsigned)((T + TA_BQ - 1) / TA_BQ));
    // the one dispatch over (head_dim, operands, output type); op float: the fp32 kernel, whose fp32 output never reads the flag
    auto launch = [&](auto hd, auto op, auto *out) {
        constexpr int HD = decltype(hd)::value;
        typedef decltype(op) OP;
        typedef std::remove_pointer_t<decltype(out)> OT;
        if constexpr (__is_same(OP, float))
            hipLaunchKernelGGL((lm_attn_prefill_kernel<HD, OT>), grid, dim3(256), 0, stream, qkv, T, n_head, out, __is_same(OT, float) ? nullptr : flag);
        else
            hipLaunchKernelGGL((lm_attn_prefill16_kernel<HD, OP, OT>), grid, dim3(256), 0, stream, qkv, T, n_head, out, flag);
    };
    auto with_out = [&](auto hd, auto op) {
        if (out32) launch(hd, op, out32);
        else if (out_fmt == OMNITOK_LM_W_BF16) launch(hd, op, static_cast<lm_bf16 *>(out16));
        else launch(hd, op, static_cast<lm_fp16 *>(out16));
    };
    auto with_op = [&](auto hd) {
        if (op_fmt == 0) with_out(hd, float{});
        else if (op_fmt == OMNITOK_LM_W_BF16) with_out(hd, lm_bf16{});
        else with_out(hd, lm_fp16{});
    };
    switch (head_dim) {
        case 64: with_op(std::integral_constant<int, 64>{}); break;
        case 96: with_op(std::integral_constant<int, 96>{}); break;
        default: with_op(std::integral_constant<int, 128>{}); break;
    }
    OT_LAUNCH_CHECK(who);
    return OMNITOK_OK;
}

}  // namespace omnitok

extern "C" int omnitok_lm_attn_prefill(const float *qkv, int B, int T, int n_head, int head_dim, float *out32, void *out16, int fmt,
                                       int *flag, omnitok_stream_t stream) {
    return omnitok::lm_attn_prefill_any("lm_attn_prefill", qkv, B, T, n_head, head_dim, 0, out32, out16, fmt, flag, static_cast<hipStream_t>(stream));
}

extern "C" int omnitok_lm_attn_prefill16(const float *qkv, int B, int T, int n_head, int head_dim, int op_fmt, float *out32, void *out16,
                                         int out_fmt, int *flag, omnitok_stream_t stream) {
    // op_fmt 0 is lm_attn_prefill_any's fp32 kernel: this entry refuses it where it checks op_fmt, after the null pointer
    OT_CHECK_ARG(!qkv || op_fmt != 0, "lm_attn_prefill16: op_fmt %d (OMNITOK_LM_W_BF16 | OMNITOK_LM_W_FP16)", op_fmt);
    return omnitok::lm_attn_prefill_any("lm_attn_prefill16", qkv, B, T, n_head, head_dim, op_fmt, out32, out16, out_fmt, flag,
                                        static_cast<hipStream_t>(stream));
}
