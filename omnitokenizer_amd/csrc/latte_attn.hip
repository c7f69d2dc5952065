// Latte denoiser: attention over the frames of every token position (omnitok_latte_attn_temporal; index: latte_common.h).
//
// The odd blocks of Latte attend over the F frames of one (sample b, position n): the reference gets those sequences by
// rearrange('(b f) t d -> (b t) f d') and undoes it after the block (latte.py:360, 373).  Here the activations stay in (b f) n order
// and one WAVE owns one (b, n, head): it reads the F rows (b F + f) N + n of qkv where they lie, N rows apart -- each row slice of a
// head is hd * 4 = 256 / 288 contiguous bytes, whole cache-line segments -- and writes the F output rows at the same places.  qkv
// is read once, out written once, no transposed copy exists.  A workgroup is 4 such waves (consecutive heads / positions); the
// waves share nothing but the barriers, so which workgroup a sequence lands in changes nothing.
//
// Steps of a wave (the LDS image is per wave: Qs, Ks, Vs [F][hd + 4], Ss [F][F | 1], Ms [32]):
//   stage   lane -> (f, 4 dims): three f32x4 loads (q, k, v) and three LDS stores, F hd / 4 of them over the 64 lanes.  Exactly
//           hd / 4 quads per row: at hd 72 no lane reads the neighbouring head's columns or past the row end.
//   logits  lane -> pair (i, j), p = lane + 64 r < F^2, i = p / F, j = p % F.  The dot product is FOUR fmaf chains from 0, chain e over the
//           dims d = e (mod 4) ascending (hd / 4 links), then s = ((c0 + c1) + (c2 + c3)) * scale, scale = fl(hd^-0.5) rounded once
//           from fp64 by the host: hd / 4 + 2 roundings on a product's path, then the scale's.
//   max     lane i < F: m_i = max_j s_ij (the softmax is anchored at the row maximum: a row of large logits survives).
//   exp     lane -> pair: p_ij = expf(s_ij - m_i), fp32.
//   P.V     lane -> (row group g, 4 dims): for its rows i = g, g + G, .. (G = 64 / (hd / 4) groups: 4 at hd 64, 3 at hd 72 with 10 idle
//           lanes) ONE fmaf chain from 0 over j ascending per output element, l_i = p_i0 + p_i1 + .. in ascending j (every lane of the
//           row adds the same F terms in the same order), out = acc / l_i: one IEEE division per element.
// So: F roundings on a product's path in P.V, F - 1 in l.  Nothing is summed across lanes; no order depends on B, N, heads, the
// wave's slot or the grid.
//
// LDS: rows of hd + 4 floats (stride 4 mod 8 dwords: the b128 reads of 16 consecutive rows cover the 64 banks once), score rows of
// F | 1 floats (odd: the max step's lane-per-row reads do not collide).  4 waves x (3 F (hd + 4) + F (F | 1) + 32) floats: 18.8 KB
// at F 5 / hd 72 (8 workgroups per CU), 62 KB at F 16 (2), 131 KB at F 32 (1).
//
// Why no MFMA: the two products of a sequence are F x F x hd, F <= 32 and 5 in the flagship model -- a 32 x 32 tile would be 2 % live
// at F = 5 -- and the kernel moves 4 hd F 4 bytes for F^2 hd 4 flops, 1.25 F flop per byte: the VALU covers that many times over at
// the HBM rate.  Time goes to the strided reads and the dependent LDS steps, not to arithmetic.
#include "latte_common.h"

#include <cmath>

namespace omnitok {

constexpr int LT_WAVES = 4;

static inline int lt_wave_floats(int F, int hd) { return (3 * F * (hd + 4) + F * (F | 1) + LATTE_F_MAX + 3) / 4 * 4; }

template <int HD>
__global__ __launch_bounds__(64 * LT_WAVES) void latte_attn_temporal_kernel(const float *__restrict__ qkv, int64_t n_seq, int F, int N,
                                                                             int heads, int wave_floats, float scale,
                                                                             float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float lt_lds[];
    constexpr int LD = HD + 4, NQ = HD / 4, G = 64 / NQ;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t seq = (int64_t)blockIdx.x * LT_WAVES + wave;
    const bool live = seq < n_seq;  // wave-uniform; a dead wave only keeps the barriers
    const int SF = F | 1, C = heads * HD, FF = F * F;
    float *Qs = lt_lds + (size_t)wave * wave_floats, *Ks = Qs + F * LD, *Vs = Ks + F * LD, *Ss = Vs + F * LD, *Ms = Ss + F * SF;
    int64_t row0 = 0;
    int h = 0;
    if (live) {
        h = (int)(seq % heads);
        const int64_t bn = seq / heads, b = bn / N;
        row0 = b * F * N + (bn - b * N);  // frame f of the sequence is row row0 + f N
    }
    if (live) {
        for (int idx = lane; idx < F * NQ; idx += 64) {
            const int f = idx / NQ, c = idx - f * NQ;
            const float *src = qkv + (row0 + (int64_t)f * N) * (3 * (int64_t)C) + h * HD + 4 * c;
            const f32x4 q = *reinterpret_cast<const f32x4 *>(src), k = *reinterpret_cast<const f32x4 *>(src + C),
                        v = *reinterpret_cast<const f32x4 *>(src + 2 * C);
            *reinterpret_cast<f32x4 *>(Qs + f * LD + 4 * c) = q;
            *reinterpret_cast<f32x4 *>(Ks + f * LD + 4 * c) = k;
            *reinterpret_cast<f32x4 *>(Vs + f * LD + 4 * c) = v;
        }
    }
    __syncthreads();
    if (live) {
        for (int p = lane; p < FF; p += 64) {
            const int i = p / F, j = p - i * F;
            const float *qr = Qs + i * LD, *kr = Ks + j * LD;
            float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, c3 = 0.0f;
#pragma unroll
            for (int u = 0; u < NQ; ++u) {
                const f32x4 qf = *reinterpret_cast<const f32x4 *>(qr + 4 * u), kf = *reinterpret_cast<const f32x4 *>(kr + 4 * u);
                c0 = fmaf(qf[0], kf[0], c0);
                c1 = fmaf(qf[1], kf[1], c1);
                c2 = fmaf(qf[2], kf[2], c2);
                c3 = fmaf(qf[3], kf[3], c3);
            }
            Ss[i * SF + j] = ((c0 + c1) + (c2 + c3)) * scale;
        }
    }
    __syncthreads();
    if (live && lane < F) {
        const float *sr = Ss + lane * SF;
        float m = sr[0];
        for (int j = 1; j < F; ++j) m = fmaxf(m, sr[j]);
        Ms[lane] = m;
    }
    __syncthreads();
    if (live) {
        for (int p = lane; p < FF; p += 64) {
            const int i = p / F, j = p - i * F;
            Ss[i * SF + j] = expf(Ss[i * SF + j] - Ms[i]);
        }
    }
    __syncthreads();
    if (live && lane < G * NQ) {
        const int g = lane / NQ, c = lane - g * NQ;
        for (int i = g; i < F; i += G) {
            const float *pr = Ss + i * SF;
            float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f, l = 0.0f;
            for (int j = 0; j < F; ++j) {
                const float p = pr[j];
                const f32x4 v = *reinterpret_cast<const f32x4 *>(Vs + j * LD + 4 * c);
                a0 = fmaf(p, v[0], a0);
                a1 = fmaf(p, v[1], a1);
                a2 = fmaf(p, v[2], a2);
                a3 = fmaf(p, v[3], a3);
                l += p;
            }
            f32x4 o;
            o[0] = a0 / l;
            o[1] = a1 / l;
            o[2] = a2 / l;
            o[3] = a3 / l;
            *reinterpret_cast<f32x4 *>(out + (row0 + (int64_t)i * N) * C + h * HD + 4 * c) = o;
        }
    }
}

}  // namespace omnitok

using namespace omnitok;

extern "C" int omnitok_latte_attn_temporal(const float *qkv, int B, int F, int N, int heads, int head_dim, float *out,
                                           omnitok_stream_t stream) {
    OT_CHECK_ARG(qkv && out, "latte_attn_temporal: null pointer");
    OT_CHECK_ARG(aligned16(qkv) && aligned16(out), "latte_attn_temporal: unaligned pointer (16 bytes)");
    OT_CHECK_ARG(head_dim == 64 || head_dim == 72, "latte_attn_temporal: head_dim %d (64 | 72)", head_dim);
    OT_CHECK_ARG(F >= 1 && F <= LATTE_F_MAX, "latte_attn_temporal: F %d frames (1 .. %d)", F, LATTE_F_MAX);
    OT_CHECK_ARG(B >= 1 && N >= 1 && heads >= 1 && heads <= 1024, "latte_attn_temporal: B %d, N %d, heads %d (1 .. 1024)", B, N, heads);
    const int64_t n_seq = (int64_t)B * N * heads;
    OT_CHECK_ARG((int64_t)B * N < (1ll << 31) / LATTE_F_MAX && n_seq / LT_WAVES < (1ll << 31) - 1,
                 "latte_attn_temporal: B %d * N %d positions, %lld sequences: too many", B, N, (long long)n_seq);
    const int wave_floats = lt_wave_floats(F, head_dim), lds = LT_WAVES * wave_floats * 4;
    const void *kernel = head_dim == 64 ? reinterpret_cast<const void *>(latte_attn_temporal_kernel<64>)
                                        : reinterpret_cast<const void *>(latte_attn_temporal_kernel<72>);
    if (int rc = set_max_dynamic_lds(kernel, lds)) return rc;
    const dim3 grid((unsigned)((n_seq + LT_WAVES - 1) / LT_WAVES));
    const float scale = (float)(1.0 / sqrt((double)head_dim));
    if (head_dim == 64)
        hipLaunchKernelGGL((latte_attn_temporal_kernel<64>), grid, dim3(64 * LT_WAVES), lds, static_cast<hipStream_t>(stream), qkv, n_seq, F,
                           N, heads, wave_floats, scale, out);
    else
        hipLaunchKernelGGL((latte_attn_temporal_kernel<72>), grid, dim3(64 * LT_WAVES), lds, static_cast<hipStream_t>(stream), qkv, n_seq, F,
                           N, heads, wave_floats, scale, out);
    OT_LAUNCH_CHECK("latte_attn_temporal");
    return OMNITOK_OK;
}
