// LM decode: flash-decode attention over the K/V cache, the merge of its chunk partials, the cache's scatter and read-back kernels,
// omnitok_lm_attn_decode / omnitok_lm_attn_decode_kv16 (index: lm_common.h)
#include "lm_common.h"

#include <cmath>

namespace omnitok {

int g_lm_attn_waves = 8;  // "lm_attn_waves": 8 = a wave owns 32 keys of the 256-key chunk (one batch of loads) | 4 = 64 keys, two batches

// F4 = head_dim / 32 float4 per lane: 8 lanes cover one K/V row of head_dim floats.  NWV waves per workgroup share the chunk's
// LM_CHUNK keys: with 8 waves a wave owns 32 keys = ONE batch of loads, and nothing in a load address depends on cache_len (rows are
// clamped to the slab, the new token's row comes from qkv and is selected afterwards): q, cache_len and every K / V row of the chunk
// are one memory round trip where the 4-wave form took three (q + length, then two batches of 32 keys) -- the kernel is a latency
// chain at decode sizes, not a stream (profiles/r05_lm_balance.txt).
//
// KT = element type of the cache (float | lm_bf16 | lm_fp16, omnitok_lm_set_cache_format).  A 16-bit cache keeps the lane mapping -- a
// lane owns the same 4 consecutive dims per i, 8-byte loads where fp32 takes 16 -- the chunking, the keys per wave and the fmaf order:
// rows are widened to fp32 in registers (exact), the token's own row stays the fp32 values of qkv (`fresh`), and its cache copy is
// rounded once at the append.  So the kernel computes what the float instantiation computes on a cache that holds the widened values
// (tests/test_gpu_lm_kv16.py).  An fp16 append that rounds to +-inf raises LM_FLAG_FP16_RANGE.  KT = float compiles to what it was.
//
// KT = lm_fp8 (omnitok_lm_set_cache_quant): the cache holds e4m3fn bytes and one power-of-two fp32 scale per row in ksc / vsc
// [max_batch][n_head][max_len] (unused by every other KT).  A lane's quad is one dword; the 8 lanes of a key slot load the row's scale
// from one address, clamped like the row itself.  kv = widen(q) * s per element (exact, fp32 subnormals included) in front of the
// unchanged chain, so this is the float instantiation's arithmetic on a cache that holds s * widen(q), bit for bit
// (tests/test_gpu_lm_kv8.py).  The append quantises the token's rows by lm_quantize_fp8_kernel's rule: wave 0 takes K's row, wave 1
// V's, one or two elements per lane, the amax by shuffles; a NaN or an infinity in a row raises LM_FLAG_KV8_NONFINITE.
template <typename KT, int F4, int NWV, int CHUNK>
__global__ __launch_bounds__(NWV * 64) void lm_attn_decode_kernel(const float *__restrict__ qkv, KT *kc, KT *vc,
                                                                  const int32_t *__restrict__ cache_len, int n_head,
                                                                  int max_len, int prefill_T,
                                                                  float *__restrict__ part, int nchunk,
                                                                  int *__restrict__ err_flag, float *ksc, float *vsc) {
    constexpr int HD = F4 * 32;
    constexpr bool Q8 = __is_same(KT, lm_fp8);
    constexpr int KPW = CHUNK / NWV;  // keys per wave
    static_assert(KPW % 32 == 0, "a wave takes its keys in batches of 32");
    // decode: one query row per stream (row == b), len = cache_len[b].  prefill (prefill_T > 0): row =
    // b * T + t is query position t of stream b; its keys 0..t-1 are already in the cache (scattered by
    // lm_kv_scatter_kernel), key t is the row's own K/V
    const int c = blockIdx.x, h = blockIdx.y, row = blockIdx.z;
    const int b = prefill_T > 0 ? row / prefill_T : row;
    const int C = n_head * HD;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int slot = lane >> 3, ds = lane & 7;  // key slot 0..7, dim slot 0..7
    const float *qn = qkv + (int64_t)row * 3 * C + h * HD;
    const float *kn = qn + C, *vn = qn + 2 * C;
    KT *krow = kc + ((int64_t)b * n_head + h) * (int64_t)max_len * HD;
    KT *vrow = vc + ((int64_t)b * n_head + h) * (int64_t)max_len * HD;
    float *ksrow = nullptr, *vsrow = nullptr;  // the rows' scales (Q8 only)
    if constexpr (Q8) {
        ksrow = ksc + ((int64_t)b * n_head + h) * (int64_t)max_len;
        vsrow = vsc + ((int64_t)b * n_head + h) * (int64_t)max_len;
    }
    typedef typename LmW<KT>::quad kquad;  // 4 consecutive cache elements as loaded
    const int kbase = c * CHUNK + wave * KPW;
    // everything this lane will read, requested at once
    f32x4 q[F4], knv[F4], vnv[F4];
#pragma unroll
    for (int i = 0; i < F4; ++i) {
        q[i] = *reinterpret_cast<const f32x4 *>(qn + (ds + 8 * i) * 4);
        knv[i] = *reinterpret_cast<const f32x4 *>(kn + (ds + 8 * i) * 4);
        vnv[i] = *reinterpret_cast<const f32x4 *>(vn + (ds + 8 * i) * 4);
    }
    kquad kk[4][F4], vv[4][F4];
    float ks[4] = {}, vs[4] = {};  // Q8: the scale of each key's K and V row (otherwise unused)
    auto request = [&](int it0) {  // rows past the slab are read from row 0 (a safe address); rows past the sequence hold whatever
#pragma unroll                     // the cache holds (never used: masked below)
        for (int j = 0; j < 4; ++j) {
            const int key = kbase + (it0 + j) * 8 + slot;
            const int64_t off = (int64_t)(key < max_len ? key : 0) * HD;
#pragma unroll
            for (int i = 0; i < F4; ++i) {
                kk[j][i] = *reinterpret_cast<const kquad *>(krow + off + (ds + 8 * i) * 4);
                vv[j][i] = *reinterpret_cast<const kquad *>(vrow + off + (ds + 8 * i) * 4);
            }
            if constexpr (Q8) {
                ks[j] = ksrow[key < max_len ? key : 0];
                vs[j] = vsrow[key < max_len ? key : 0];
            }
        }
    };
    request(0);
    int len = prefill_T > 0 ? row - b * prefill_T : cache_len[row];
    if (len >= max_len) {
        // a caller stepped past the cache it allocated: flag it (omnitok_lm_overflowed) and stay inside
        // this head's K/V slab instead of reading the neighbour's rows
        if (err_flag && threadIdx.x == 0) {
            if constexpr (LmKV<KT>::CAN_OVERFLOW || Q8) atomicOr(err_flag, LM_FLAG_PAST_CACHE);  // (the word has a second bit to keep)
            else *err_flag = LM_FLAG_PAST_CACHE;
        }
        len = max_len - 1;
    }
    const int total = len + 1;
    if (c * CHUNK >= total) return;   // chunk beyond the sequence (static launch grid)
    // append the new token's K/V (only the workgroup whose chunk holds index len)
    if (prefill_T == 0 && len >= c * CHUNK && len < (c + 1) * CHUNK && len < max_len) {
        if constexpr (Q8) {
            if (wave < 2) {  // wave 0: K's row | wave 1: V's row; elements lane and lane + 64
                const float *src = wave == 0 ? kn : vn;
                const bool two = lane + 64 < HD;
                const float x0 = src[lane], x1 = two ? src[lane + 64] : 0.0f;
                const unsigned a0 = __builtin_bit_cast(unsigned, x0) & 0x7FFFFFFFu, a1 = __builtin_bit_cast(unsigned, x1) & 0x7FFFFFFFu;
                unsigned amax = a0 > a1 ? a0 : a1;
#pragma unroll
                for (int sh = 32; sh >= 1; sh >>= 1) {
                    const unsigned o = (unsigned)__shfl_xor((int)amax, sh);
                    amax = o > amax ? o : amax;
                }
                const int e = lm_fp8_scale_exp(amax);
                const unsigned p = (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(__builtin_ldexpf(x0, -e), __builtin_ldexpf(x1, -e), 0, false);
                lm_fp8 *dst = (wave == 0 ? krow : vrow) + (int64_t)len * HD;
                dst[lane] = lm_fp8{(unsigned char)(p & 0xFFu)};
                if (two) dst[lane + 64] = lm_fp8{(unsigned char)((p >> 8) & 0xFFu)};
                if (lane == 0) {
                    (wave == 0 ? ksrow : vsrow)[len] = lm_fp8_scale(e);
                    if (amax >= 0x7F800000u && err_flag) atomicOr(err_flag, LM_FLAG_KV8_NONFINITE);
                }
            }
        } else {
            bool inf = false;
            for (int d = tid; d < HD; d += NWV * 64) {
                krow[(int64_t)len * HD + d] = LmKV<KT>::store(kn[d], inf);
                vrow[(int64_t)len * HD + d] = LmKV<KT>::store(vn[d], inf);
            }
            if constexpr (LmKV<KT>::CAN_OVERFLOW)
                if (inf && err_flag) atomicOr(err_flag, LM_FLAG_FP16_RANGE);
        }
    }
    const float scale = 1.0f / sqrtf((float)HD);
    float m = -INFINITY, l = 0.0f;
    f32x4 o[F4];
#pragma unroll
    for (int i = 0; i < F4; ++i) o[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    // 8 keys per iteration, four iterations (32 keys) per batch of loads
    for (int it0 = 0; it0 < KPW / 8; it0 += 4) {
        if (kbase + it0 * 8 >= total) break;  // wave-uniform: no keys left in this chunk
        if (it0 > 0) request(it0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int key = kbase + (it0 + j) * 8 + slot;
            const bool valid = key < total;
            // the new token's row comes from qkv (its cache copy is being written by this kernel)
            const bool fresh = key == len;
            float s = 0.0f;
#pragma unroll
            for (int i = 0; i < F4; ++i) {
                const f32x4 kv = fresh ? knv[i] : lm_kv_widen<KT>(kk[j][i], ks[j]);
                s = fmaf(q[i][0], kv[0], s);
                s = fmaf(q[i][1], kv[1], s);
                s = fmaf(q[i][2], kv[2], s);
                s = fmaf(q[i][3], kv[3], s);
            }
            s += __shfl_xor(s, 1);
            s += __shfl_xor(s, 2);
            s += __shfl_xor(s, 4);
            s = valid ? s * scale : -INFINITY;
            const float mn = fmaxf(m, s);
            if (valid && mn > -INFINITY) {   // a masked key changes nothing (and its V row may be uninitialised)
                const float corr = expf(m - mn), p = expf(s - mn);
                l = l * corr + p;
#pragma unroll
                for (int i = 0; i < F4; ++i) o[i] = o[i] * corr + (fresh ? vnv[i] : lm_kv_widen<KT>(vv[j][i], vs[j])) * p;
                m = mn;
            }
        }
    }
    // merge the 8 key slots of the wave (lanes with equal dim slot: xor 8, 16, 32)
    float ma = m;
    ma = fmaxf(ma, __shfl_xor(ma, 8));
    ma = fmaxf(ma, __shfl_xor(ma, 16));
    ma = fmaxf(ma, __shfl_xor(ma, 32));
    const float sc = ma > -INFINITY ? expf(m - ma) : 0.0f;
    l *= sc;
#pragma unroll
    for (int i = 0; i < F4; ++i) o[i] = o[i] * sc;
#pragma unroll
    for (int sh = 8; sh <= 32; sh <<= 1) {
        l += __shfl_xor(l, sh);
#pragma unroll
        for (int i = 0; i < F4; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) o[i][e] += __shfl_xor(o[i][e], sh);
    }
    // merge the waves through LDS
    __shared__ float s_m[NWV], s_l[NWV];
    __shared__ __attribute__((aligned(16))) float s_o[NWV][HD];
    if (lane < 8) {
#pragma unroll
        for (int i = 0; i < F4; ++i) *reinterpret_cast<f32x4 *>(&s_o[wave][(lane + 8 * i) * 4]) = o[i];
        if (lane == 0) {
            s_m[wave] = ma;
            s_l[wave] = l;
        }
    }
    __syncthreads();
    if (tid < HD) {
        float M = s_m[0];
#pragma unroll
        for (int wv = 1; wv < NWV; ++wv) M = fmaxf(M, s_m[wv]);
        float L = 0.0f, O = 0.0f;
#pragma unroll
        for (int wv = 0; wv < NWV; ++wv) {
            const float f = s_m[wv] > -INFINITY ? expf(s_m[wv] - M) : 0.0f;
            L += s_l[wv] * f;
            O += s_o[wv][tid] * f;
        }
        float *pp = part + (((int64_t)row * n_head + h) * nchunk + c) * (2 + HD);
        pp[2 + tid] = O;
        if (tid == 0) {
            pp[0] = M;
            pp[1] = L;
        }
    }
}

// OT = float: out [rows][n_head * HD] fp32 | lm_bf16 / lm_fp16: the same value rounded once (lm_round16) into a packed 16-bit row, the
// proj GEMM's operand of a PF_W16 prefill or an SF_W16 step; an fp16 result of +-inf raises flag_bit in *flag
template <typename OT>
__global__ void lm_attn_merge_kernel(const float *__restrict__ part, const int32_t *__restrict__ cache_len, int n_head,
                                     int HD, int nchunk, int prefill_T, OT *__restrict__ out, int chunk, int *__restrict__ flag,
                                     int flag_bit) {
    const int h = blockIdx.x, b = blockIdx.y, d = threadIdx.x;  // b: query row
    if (d >= HD) return;
    const int total = (prefill_T > 0 ? b % prefill_T : cache_len[b]) + 1;
    int used = (total + chunk - 1) / chunk;
    if (used > nchunk) used = nchunk;  // a stream stepped past max_len (flagged, clamped the same way by the attention kernel)
    const float *pp = part + ((int64_t)b * n_head + h) * nchunk * (2 + HD);
    float M = -INFINITY;
    for (int c = 0; c < used; ++c) M = fmaxf(M, pp[c * (2 + HD)]);
    float L = 0.0f, O = 0.0f;
    for (int c = 0; c < used; ++c) {
        const float f = expf(pp[c * (2 + HD)] - M);
        L += pp[c * (2 + HD) + 1] * f;
        O += pp[c * (2 + HD) + 2 + d] * f;
    }
    if constexpr (__is_same(OT, float)) {
        out[((int64_t)b * n_head + h) * HD + d] = O / L;
    } else {
        bool inf = false;
        out[((int64_t)b * n_head + h) * HD + d] = LmKV<OT>::store(O / L, inf);
        if (inf && flag) atomicOr(flag, flag_bit);
    }
}

// qkv[B*T, 3C] (query | key | value) -> K/V cache rows [b][h][t][hd], rounded to the cache's element type KT on the way (the prefill's
// one rounding of a row; an fp16 element that becomes +-inf raises LM_FLAG_FP16_RANGE in the engine's flag word)
template <typename KT>
__global__ __launch_bounds__(256) void lm_kv_scatter_kernel(const float *__restrict__ qkv, KT *__restrict__ kc,
                                                            KT *__restrict__ vc, int T, int n_head, int hd,
                                                            int max_len, int *__restrict__ err_flag) {
    const int64_t row = blockIdx.x;  // b * T + t
    const int b = (int)(row / T), t = (int)(row % T), C = n_head * hd;
    typedef typename LmW<KT>::quad kquad;
    bool inf = false;
    for (int i = threadIdx.x * 4; i < C; i += 256 * 4) {
        const int h = i / hd, d = i - h * hd;
        const int64_t dst = (((int64_t)b * n_head + h) * max_len + t) * hd + d;
        *reinterpret_cast<kquad *>(kc + dst) = LmKV<KT>::store4(*reinterpret_cast<const f32x4 *>(qkv + row * 3 * C + C + i), inf);
        *reinterpret_cast<kquad *>(vc + dst) = LmKV<KT>::store4(*reinterpret_cast<const f32x4 *>(qkv + row * 3 * C + 2 * C + i), inf);
    }
    if constexpr (LmKV<KT>::CAN_OVERFLOW)
        if (inf && err_flag) atomicOr(err_flag, LM_FLAG_FP16_RANGE);
}

// The scatter into an fp8 cache (OMNITOK_LM_KQ_FP8): a row's scale needs the amax of its head_dim elements, and the mapping above puts a
// head's hd / 4 threads across a wave boundary at head_dim 96.  Here an aligned group of 8 lanes owns one (row, head, K | V): a lane
// reads F4 = hd / 32 float4 (quads ds + 8 i, the attention kernel's dim slots) once into registers, the amax is three shuffles inside
// the group, and the lane writes F4 dwords of e4m3fn; lane 0 of the group writes the scale.  The rule is lm_quantize_fp8_kernel's
// (lm_fp8_scale_exp); a NaN or an infinity in a row raises LM_FLAG_KV8_NONFINITE.  groups = rows * n_head * 2.
template <int F4>
__global__ __launch_bounds__(256) void lm_kv_scatter8_kernel(const float *__restrict__ qkv, lm_fp8 *__restrict__ kc, lm_fp8 *__restrict__ vc,
                                                             float *__restrict__ ksc, float *__restrict__ vsc, int64_t groups, int T,
                                                             int n_head, int max_len, int *__restrict__ err_flag) {
    constexpr int HD = F4 * 32;
    const int64_t g = (int64_t)blockIdx.x * 32 + (threadIdx.x >> 3);
    if (g >= groups) return;  // (a whole group leaves together: the shuffles below stay inside a group)
    const int ds = threadIdx.x & 7;
    const int kv = (int)(g & 1), h = (int)((g >> 1) % n_head);
    const int64_t row = (g >> 1) / n_head;  // b * T + t
    const int b = (int)(row / T), t = (int)(row % T), C = n_head * HD;
    const float *src = qkv + row * 3 * C + (1 + kv) * C + h * HD;
    f32x4 v[F4];
    unsigned amax = 0u;
#pragma unroll
    for (int i = 0; i < F4; ++i) {
        v[i] = *reinterpret_cast<const f32x4 *>(src + (ds + 8 * i) * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float f = v[i][e];  // (a scalar copy: __builtin_bit_cast of a vector ELEMENT reads element 0 with this compiler)
            const unsigned a = __builtin_bit_cast(unsigned, f) & 0x7FFFFFFFu;
            amax = a > amax ? a : amax;
        }
    }
#pragma unroll
    for (int sh = 4; sh >= 1; sh >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)amax, sh);
        amax = o > amax ? o : amax;
    }
    const int e = lm_fp8_scale_exp(amax);
    const int64_t r = ((int64_t)b * n_head + h) * max_len + t;  // the row in its slab
    unsigned *dst = reinterpret_cast<unsigned *>((kv ? vc : kc) + r * HD);
#pragma unroll
    for (int i = 0; i < F4; ++i) {
        int p = __builtin_amdgcn_cvt_pk_fp8_f32(__builtin_ldexpf(v[i][0], -e), __builtin_ldexpf(v[i][1], -e), 0, false);
        p = __builtin_amdgcn_cvt_pk_fp8_f32(__builtin_ldexpf(v[i][2], -e), __builtin_ldexpf(v[i][3], -e), p, true);
        dst[ds + 8 * i] = (unsigned)p;
    }
    if (ds == 0) {
        (kv ? vsc : ksc)[r] = lm_fp8_scale(e);
        if (amax >= 0x7F800000u && err_flag) atomicOr(err_flag, LM_FLAG_KV8_NONFINITE);
    }
}

// omnitok_lm_cache_read: rows t0 .. t0 + n - 1 of one stream's K and V slabs [n_head][max_len][hd], gathered and widened to fp32
// [n_head][n][hd] (an fp8 cache: times the row's scale from ksc / vsc [n_head][max_len], unused otherwise).  One thread per 4
// consecutive dims.
template <typename KT>
__global__ __launch_bounds__(256) void lm_kv_read_kernel(const KT *__restrict__ kc, const KT *__restrict__ vc, int t0, int n,
                                                         int n_head, int hd, int max_len, float *__restrict__ k_out,
                                                         float *__restrict__ v_out, const float *__restrict__ ksc,
                                                         const float *__restrict__ vsc) {
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;  // element of the output
    if (i >= (int64_t)n_head * n * hd) return;
    const int d = (int)(i % hd), t = (int)(i / hd % n), h = (int)(i / hd / n);
    const int64_t src = ((int64_t)h * max_len + t0 + t) * hd + d;
    typedef typename LmW<KT>::quad kquad;
    float sk = 1.0f, sv = 1.0f;
    if constexpr (__is_same(KT, lm_fp8)) {
        sk = ksc[(int64_t)h * max_len + t0 + t];
        sv = vsc[(int64_t)h * max_len + t0 + t];
    }
    *reinterpret_cast<f32x4 *>(k_out + i) = lm_kv_widen<KT>(*reinterpret_cast<const kquad *>(kc + src), sk);
    *reinterpret_cast<f32x4 *>(v_out + i) = lm_kv_widen<KT>(*reinterpret_cast<const kquad *>(vc + src), sv);
}

int lm_attn_partials(const LmAttnArgs &a, hipStream_t stream) {
    OT_CHECK_ARG(a.qkv && a.kc && a.vc && (a.cache_len || a.prefill_T > 0) && a.part, "lm_attn_decode: null pointer");
    OT_CHECK_ARG(a.kq != OMNITOK_LM_KQ_FP8 || (a.ksc && a.vsc), "lm_attn_decode: null scale pointer");
    OT_CHECK_ARG(a.head_dim == 64 || a.head_dim == 96 || a.head_dim == 128, "lm_attn_decode: head_dim %d (64 | 96 | 128)",
                 a.head_dim);
    OT_CHECK_ARG(a.max_len > 0 && a.n_head > 0, "lm_attn_decode: bad sizes");
    const int chunk = a.chunk, nchunk = ((a.prefill_T > 0 ? a.prefill_T : a.max_len) + chunk - 1) / chunk;
    const int rows = a.prefill_T > 0 ? a.B * a.prefill_T : a.B;
    OT_CHECK_ARG(rows <= 65535, "lm_attn_decode: %d query rows (max 65535)", rows);
    const dim3 grid(nchunk, a.n_head, rows);
    const bool wide = g_lm_attn_waves == 8;
    lm_with_kt(a.kvfmt, a.kq, [&](auto kt) {
        typedef decltype(kt) KT;
        KT *k = static_cast<KT *>(a.kc), *v = static_cast<KT *>(a.vc);
        auto launch = [&](auto f4) {
            constexpr int F4 = decltype(f4)::value;
            const bool w8 = wide && chunk != LM_CHUNK_SHORT;
            const auto kernel = chunk == LM_CHUNK_SHORT ? lm_attn_decode_kernel<KT, F4, 4, LM_CHUNK_SHORT>
                                : wide ? lm_attn_decode_kernel<KT, F4, 8, LM_CHUNK> : lm_attn_decode_kernel<KT, F4, 4, LM_CHUNK>;
            hipLaunchKernelGGL(kernel, grid, dim3(w8 ? 512 : 256), 0, stream, a.qkv, k, v, a.cache_len, a.n_head, a.max_len, a.prefill_T,
                               a.part, nchunk, a.err_flag, a.ksc, a.vsc);
        };
        switch (a.head_dim) {
            case 64: launch(std::integral_constant<int, 2>{}); break;
            case 96: launch(std::integral_constant<int, 3>{}); break;
            default: launch(std::integral_constant<int, 4>{}); break;
        }
    });
    OT_LAUNCH_CHECK("lm_attn_decode");
    return OMNITOK_OK;
}

void lm_attn_merge(const float *part, const int32_t *cache_len, int n_head, int hd, int nchunk, int prefill_T, float *out32, void *out16,
                   int fmt, int64_t rows, int *flag, int chunk, hipStream_t stream, int flag_bit) {
    const dim3 grid(n_head, (unsigned)rows);
    auto launch = [&](auto *out, int *fl) {
        typedef std::remove_pointer_t<decltype(out)> OT;
        hipLaunchKernelGGL(lm_attn_merge_kernel<OT>, grid, dim3(128), 0, stream, part, cache_len, n_head, hd, nchunk, prefill_T, out, chunk, fl,
                           flag_bit);
    };
    if (out32) launch(out32, static_cast<int *>(nullptr));
    else if (fmt == OMNITOK_LM_W_BF16) launch(static_cast<lm_bf16 *>(out16), flag);
    else launch(static_cast<lm_fp16 *>(out16), flag);
}

int lm_kv_scatter(const float *qkv, void *kc, void *vc, int kvfmt, int kq, float *ksc, float *vsc, int64_t rows, int T, int n_head, int hd,
                  int max_len, int *err_flag, hipStream_t stream) {
    if (kq == OMNITOK_LM_KQ_FP8) {
        const int64_t groups = rows * n_head * 2;
        auto launch = [&](auto f4) {
            hipLaunchKernelGGL(lm_kv_scatter8_kernel<decltype(f4)::value>, dim3((unsigned)((groups + 31) / 32)), dim3(256), 0, stream, qkv,
                               static_cast<lm_fp8 *>(kc), static_cast<lm_fp8 *>(vc), ksc, vsc, groups, T, n_head, max_len, err_flag);
        };
        switch (hd) {
            case 64: launch(std::integral_constant<int, 2>{}); break;
            case 96: launch(std::integral_constant<int, 3>{}); break;
            default: launch(std::integral_constant<int, 4>{}); break;
        }
        OT_LAUNCH_CHECK("lm_kv_scatter8");
        return OMNITOK_OK;
    }
    lm_with_kfmt(kvfmt, [&](auto kt) {
        typedef decltype(kt) KT;
        hipLaunchKernelGGL(lm_kv_scatter_kernel<KT>, dim3((unsigned)rows), dim3(256), 0, stream, qkv, static_cast<KT *>(kc),
                           static_cast<KT *>(vc), T, n_head, hd, max_len, err_flag);
    });
    OT_LAUNCH_CHECK("lm_kv_scatter");
    return OMNITOK_OK;
}

int lm_kv_read(const void *kc, const void *vc, int kvfmt, int kq, const float *ksc, const float *vsc, int t0, int n, int n_head, int hd,
               int max_len, float *k_out, float *v_out, hipStream_t stream) {
    const int64_t quads = (int64_t)n_head * n * hd / 4;
    const dim3 grid((unsigned)((quads + 255) / 256));
    lm_with_kt(kvfmt, kq, [&](auto kt) {
        typedef decltype(kt) KT;
        hipLaunchKernelGGL(lm_kv_read_kernel<KT>, grid, dim3(256), 0, stream, static_cast<const KT *>(kc), static_cast<const KT *>(vc),
                           t0, n, n_head, hd, max_len, k_out, v_out, ksc, vsc);
    });
    OT_LAUNCH_CHECK("lm_kv_read");
    return OMNITOK_OK;
}

// partials + merge launch over caches of element format kvfmt: the exported building blocks
// (ksc / vsc: the row scales of e4m3fn caches -- OMNITOK_LM_KQ_FP8 -- or nullptr)
static int lm_attn_decode_any(const char *who, const float *qkv, void *kc, void *vc, int kvfmt, const int32_t *cache_len, int B,
                              int n_head, int head_dim, int max_len, float *scratch, float *out, hipStream_t stream,
                              float *ksc = nullptr, float *vsc = nullptr) {
    OT_CHECK_ARG(out, "%s: null pointer", who);
    LmAttnArgs a = {};
    a.qkv = qkv; a.kc = kc; a.vc = vc; a.kvfmt = kvfmt;
    a.kq = ksc ? OMNITOK_LM_KQ_FP8 : OMNITOK_LM_KQ_NONE; a.ksc = ksc; a.vsc = vsc;
    a.cache_len = cache_len; a.B = B; a.n_head = n_head; a.head_dim = head_dim; a.max_len = max_len;
    a.part = scratch; a.chunk = LM_CHUNK;
    if (int rc = lm_attn_partials(a, stream)) return rc;
    lm_attn_merge(scratch, cache_len, n_head, head_dim, (max_len + LM_CHUNK - 1) / LM_CHUNK, 0, out, nullptr, 0, B, nullptr, LM_CHUNK, stream);
    OT_LAUNCH_CHECK("lm_attn_merge");
    return OMNITOK_OK;
}

}  // namespace omnitok

using namespace omnitok;

extern "C" int omnitok_lm_attn_decode(const float *qkv, float *kc, float *vc, const int32_t *cache_len, int B,
                                      int n_head, int head_dim, int max_len, float *scratch, float *out,
                                      omnitok_stream_t stream_) {
    if (B == 0) return OMNITOK_OK;
    return lm_attn_decode_any("lm_attn_decode", qkv, kc, vc, OMNITOK_LM_KV_FP32, cache_len, B, n_head, head_dim, max_len, scratch, out,
                              static_cast<hipStream_t>(stream_));
}

extern "C" int omnitok_lm_attn_decode_kv16(const float *qkv, void *kc16, void *vc16, int fmt, const int32_t *cache_len, int B,
                                           int n_head, int head_dim, int max_len, float *scratch, float *out,
                                           omnitok_stream_t stream_) {
    OT_CHECK_ARG(fmt == OMNITOK_LM_KV_BF16 || fmt == OMNITOK_LM_KV_FP16,
                 "lm_attn_decode_kv16: fmt %d (OMNITOK_LM_KV_BF16 | OMNITOK_LM_KV_FP16)", fmt);
    if (B == 0) return OMNITOK_OK;
    OT_CHECK_ARG(qkv && kc16 && vc16, "lm_attn_decode_kv16: null pointer");
    OT_CHECK_ARG(aligned16(kc16) && aligned16(vc16), "lm_attn_decode_kv16: unaligned cache pointer (16 bytes)");
    return lm_attn_decode_any("lm_attn_decode_kv16", qkv, kc16, vc16, fmt, cache_len, B, n_head, head_dim, max_len, scratch, out,
                              static_cast<hipStream_t>(stream_));
}

extern "C" int omnitok_lm_attn_decode_kv8(const float *qkv, void *kc8, void *vc8, float *kscale, float *vscale,
                                          const int32_t *cache_len, int B, int n_head, int head_dim, int max_len, float *scratch,
                                          float *out, omnitok_stream_t stream_) {
    if (B == 0) return OMNITOK_OK;
    OT_CHECK_ARG(qkv && kc8 && vc8 && kscale && vscale, "lm_attn_decode_kv8: null pointer");
    OT_CHECK_ARG(aligned16(qkv) && aligned16(kc8) && aligned16(vc8), "lm_attn_decode_kv8: unaligned pointer (16 bytes)");
    return lm_attn_decode_any("lm_attn_decode_kv8", qkv, kc8, vc8, OMNITOK_LM_KV_FP32, cache_len, B, n_head, head_dim, max_len, scratch, out,
                              static_cast<hipStream_t>(stream_), kscale, vscale);
}
