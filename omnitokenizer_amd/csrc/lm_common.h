// LM consumer of the token path: KV-cached decode step of the reference's minGPT
// (OmniTokenizer/modules/gpt.py:74-275) for sample_with_past (gpt.py:327-359).
//
// One token per stream per step, so every matrix product is a GEMV over the weights: the step is
// HBM-bound (24 layers x 12 C^2 x 4 B = 2.7 GB of fp32 weights at C = 1536, half of that in a 16-bit
// weight format -- omnitok_lm_set_weight_format -- plus the K/V cache), not MFMA-bound.
// Shapes and launch grids do not depend on the position (chunks beyond the cache length exit at
// once), so a step can be captured once in a HIP graph and replayed for every token.
//
// Which unit holds what (every kernel template lives in the one .hip that launches it; this header defines no kernel):
//   lm_common.h       the constants, the weight / cache element types (LmW, lm_round16, LmKV), LmMerge, the host types LmMat and
//                     LmLinear, the format dispatches lm_with_wt / lm_with_kt, lm_grow, and the host functions that cross units
//   lm_gemv.hip       lm_gemv_kernel (the row GEMV), lm_gemv_any (the loop over groups of 8 / 4 / 2 / 1 streams), omnitok_lm_gemv[_w16|_fp8]
//   lm_gemv_ks.hip    lm_gemv_ks_kernel (the K-sliced GEMV of K in {1536, 2048, 6144, 8192}) behind lm_gemv_ks_try; LM_TRACE
//   lm_quant.hip      lm_quantize_fp8_kernel (row amax -> power-of-two scale -> packed e4m3fn image), omnitok_lm_quantize_fp8
//   lm_gemm_mfma.hip  lm_gemm4_kernel (4 .. 8 streams on the matrix cores, "lm_mfma" 1) behind lm_gemm4_try; lm_gemm_streams_kernel and
//                     lm_streams_reduce_kernel (17 .. 128 streams, omnitok_lm_set_max_streams), omnitok_lm_gemm_streams
//   lm_gemm_streams16.hip  lm_gemm_streams16_kernel and lm_streams16_reduce_kernel (17 .. 128 streams on the 16-bit MFMA over packed
//                     activations and weights, omnitok_lm_set_streams_format), omnitok_lm_gemm_streams16
//   lm_gemm16.hip     lm_gemm16_kernel (the 16-bit MFMA GEMM of a PF_W16 prefill, omnitok_lm_set_prefill_format), omnitok_lm_gemm16
//   lm_attn.hip       lm_attn_decode_kernel (flash-decode over the fp32 / bf16 / fp16 / fp8 K/V cache, chunk partials), lm_attn_merge_kernel
//                     (fp32 or, for a PF_W16 prefill, 16-bit output), lm_kv_scatter_kernel, lm_kv_scatter8_kernel (the fp8 cache's),
//                     lm_kv_read_kernel, omnitok_lm_attn_decode[_kv16|_kv8]
//   lm_attn_prefill.hip  the tiled causal attention of the prefill, K/V tiles shared by 128 query rows (omnitok_lm_set_prefill_attention):
//                     lm_attn_prefill_kernel on the fp32-input MFMA (the body it shares with the DiT: attn_f32_tiled.h) and lm_attn_prefill16_kernel on the bf16 / fp16 MFMA (Q / K / V / P
//                     rounded once to the operand format; omnitok_lm_set_prefill_attention_operands) behind one host side,
//                     lm_attn_prefill_any; omnitok_lm_attn_prefill, omnitok_lm_attn_prefill16
//   lm_engine.hip     struct omnitok_lm and its exported functions (create .. finalize, alloc_cache, step, prefill, prefill_loss) and the
//                     small kernels: embed, embed_seq, layernorm_rows (fp32 or 16-bit output, omnitok_lm_layernorm16), gelu, set_len,
//                     advance, concat3, round_w16
#pragma once
#include "common.h"
#include "../../include/omnitok_lm.h"

#include <type_traits>

namespace omnitok {

constexpr int LM_CHUNK = 256;   // keys per attention workgroup
constexpr int LM_CHUNK_SHORT = 128;  // ... of the decode step when the cache holds at most 32 such chunks: twice the workgroups (a
                                     // 256-key chunk is 196 KB through ONE CU: the kernel is bound by that CU's share of the bandwidth);
                                     // 64 measured better per token on average and worse at 512 keys, where the merge in the
                                     // projection's prologue outgrows its first round of loads
constexpr int LM_KP = 2048;        // K panel staged in LDS (BQ * LM_KP * 4 B <= 64 KiB; one 6144-float panel for the
                                   // FC2 input at B = 1 measured the same: 1.114 ms / token)
constexpr int LM_MAX_CHUNKS = 32;  // attention chunks per sequence: max_len <= 8192
constexpr int LM_MAX_HEADS = 32;   // (bounds the merge-weight table in LDS: B * heads * chunks floats)

// Weight element types of the decode GEMVs (omnitok_lm_set_weight_format).  Both kernels below take the element type WT as a template
// parameter; a lane's share of a 256-column chunk is always the same 4 consecutive weights -- 16 bytes of fp32, 8 bytes of a 16-bit
// format, 4 bytes of fp8 -- widened to fp32 in registers (exact) in front of the same fmaf chain.  WT = float compiles to the code it
// was before.
struct lm_bf16 { unsigned short bits; };
struct lm_fp16 { unsigned short bits; };
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
struct lm_fp8 { unsigned char bits; };  // OCP e4m3fn, the decode-quant image (omnitok_lm_set_decode_quant): 4 weights are one dword
template <typename WT> struct LmW;
template <> struct LmW<float> {
    typedef f32x4 quad;  // 4 consecutive weights as loaded
    static __device__ __forceinline__ f32x4 widen(const f32x4 &q) { return q; }
    static __device__ __forceinline__ quad load(__amdgpu_buffer_rsrc_t rs, int byte_off) {
        return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, byte_off, 0, 2));
    }
};
template <> struct LmW<lm_bf16> {
    typedef u32x2 quad;
    static __device__ __forceinline__ f32x4 widen(const u32x2 &q) {  // bf16 is the high half of the fp32 pattern: a shift or a mask per element
        return f32x4{__builtin_bit_cast(float, q[0] << 16), __builtin_bit_cast(float, q[0] & 0xffff0000u),
                     __builtin_bit_cast(float, q[1] << 16), __builtin_bit_cast(float, q[1] & 0xffff0000u)};
    }
    static __device__ __forceinline__ quad load(__amdgpu_buffer_rsrc_t rs, int byte_off) {
        return __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(rs, byte_off, 0, 2));
    }
};
template <> struct LmW<lm_fp16> {
    typedef u32x2 quad;
    // fp16 -> fp32 of each half, subnormals included (exact).  The compiler folds the conversion into the multiply-add
    // (v_fma_mix_f32 reads an fp16 half as a source operand): no VALU instruction of its own.  The quad is reinterpreted as a whole:
    // __builtin_bit_cast of ONE ELEMENT of an ext_vector (q[1]) reads element 0 with this compiler.
    static __device__ __forceinline__ f32x4 widen(const u32x2 &q) {
        const f16x4 h = __builtin_bit_cast(f16x4, q);
        return f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
    }
    static __device__ __forceinline__ quad load(__amdgpu_buffer_rsrc_t rs, int byte_off) {
        return __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(rs, byte_off, 0, 2));
    }
};

template <> struct LmW<lm_fp8> {
    typedef unsigned quad;
    // e4m3fn -> fp32 of each byte, subnormals and +-0 included (exact): v_cvt_pk_f32_fp8 on the low and the high half of the dword.  The
    // row's power-of-two scale is NOT applied here but once per output, in the kernels' epilogue (exact as well)
    static __device__ __forceinline__ f32x4 widen(const unsigned &q) {
        const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)q, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)q, true);
        return f32x4{lo[0], lo[1], hi[0], hi[1]};
    }
    static __device__ __forceinline__ quad load(__amdgpu_buffer_rsrc_t rs, int byte_off) {
        return (unsigned)__builtin_amdgcn_raw_buffer_load_b32(rs, byte_off, 0, 2);
    }
};

// fp32 -> 16-bit, round to nearest even: the bits of tensor.to(torch.bfloat16) / .to(torch.float16), fp16 subnormals kept, NaN -> quiet
// NaN.  One conversion for the weight images (lm_round_w16_kernel) and the K/V cache (the attention kernel's append, the prefill's
// scatter).  f is a scalar copy: __builtin_bit_cast of a vector ELEMENT reads element 0 with this compiler.
template <typename T> __device__ __forceinline__ unsigned short lm_round16(float f);
template <> __device__ __forceinline__ unsigned short lm_round16<lm_bf16>(float f) {
    const unsigned u = __builtin_bit_cast(unsigned, f);
    return f != f ? (unsigned short)0x7FC0 : (unsigned short)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
template <> __device__ __forceinline__ unsigned short lm_round16<lm_fp16>(float f) {
    return __builtin_bit_cast(unsigned short, (_Float16)f);  // v_cvt_f16_f32: round to nearest even, subnormal results kept
}
__device__ __forceinline__ bool lm_f16_is_inf(unsigned short h) { return (h & 0x7FFF) == 0x7C00; }

// Element types of the K/V cache (omnitok_lm_set_cache_format): float, or one of the 16-bit types above.  A row is rounded ONCE, where
// it is stored; it is read back through LmW<KT>::widen (exact).  Only an fp16 store can leave the range (CAN_OVERFLOW).
template <typename KT> struct LmKV {
    static constexpr bool CAN_OVERFLOW = __is_same(KT, lm_fp16);
    static __device__ __forceinline__ KT store(float f, bool &inf) {
        const unsigned short h = lm_round16<KT>(f);
        if constexpr (CAN_OVERFLOW) inf = inf || lm_f16_is_inf(h);
        return KT{h};
    }
    // 4 consecutive elements as one 8-byte value
    static __device__ __forceinline__ u32x2 store4(const f32x4 &v, bool &inf) {
        unsigned short h[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float f = v[e];
            h[e] = lm_round16<KT>(f);
            if constexpr (CAN_OVERFLOW) inf = inf || lm_f16_is_inf(h[e]);
        }
        return u32x2{(unsigned)h[0] | ((unsigned)h[1] << 16), (unsigned)h[2] | ((unsigned)h[3] << 16)};
    }
};
template <> struct LmKV<float> {
    static constexpr bool CAN_OVERFLOW = false;
    static __device__ __forceinline__ float store(float f, bool &) { return f; }
    static __device__ __forceinline__ f32x4 store4(const f32x4 &v, bool &) { return v; }
};
// The power-of-two row scale 2^e of the fp8 images (lm_quantize_fp8_kernel, the K/V cache under omnitok_lm_set_cache_quant) from the row's
// amax, given as the fp32 pattern without its sign: e is the smallest integer such that amax 2^-e <= 448.  amax = 1.f x 2^(E - 127)
// = m x 2^(E - 126) with m = 1.f / 2 in [0.5, 1), and m <= 0.875 <=> mantissa field <= 0x600000 (448 = 1.75 x 2^8); a subnormal amax
// (E = 0) lands below the clamp whatever its mantissa; e = 0 for a zero row; clamped so that the scale is a normal fp32
__device__ __forceinline__ int lm_fp8_scale_exp(unsigned amax) {
    int e = 0;
    if (amax != 0u) {
        const int E = (int)(amax >> 23), x = E - 126;
        e = (amax & 0x7FFFFFu) <= 0x600000u ? x - 9 : x - 8;
        e = e < -126 ? -126 : (e > 127 ? 127 : e);
    }
    return e;
}
__device__ __forceinline__ float lm_fp8_scale(int e) { return __builtin_bit_cast(float, (unsigned)(e + 127) << 23); }
// a cached quad as fp32: widened, and for the fp8 cache multiplied by its row's scale s (exact: a power of two times at most 4
// significant bits, fp32 subnormals kept); every other KT ignores s
template <typename KT> __device__ __forceinline__ f32x4 lm_kv_widen(const typename LmW<KT>::quad &q, float s) {
    if constexpr (__is_same(KT, lm_fp8)) return LmW<KT>::widen(q) * s;
    else return LmW<KT>::widen(q);
}
constexpr int LM_FLAG_PAST_CACHE = 1;  // bits of the engine's flag word (omnitok_lm_overflowed)
constexpr int LM_FLAG_FP16_RANGE = 2;
constexpr int LM_FLAG_PF16_RANGE = 4;  // an activation of an fp16 PF_W16 prefill rounded to +-inf
constexpr int LM_FLAG_AOP16_RANGE = 8;  // a Q / K / V element of a prefill attention with fp16 operands rounded to +-inf
constexpr int LM_FLAG_SF16_RANGE = 16;  // an activation of an fp16 SF_W16 many-stream step rounded to +-inf
constexpr int LM_FLAG_KV8_NONFINITE = 32;  // a K or V row stored into an fp8 cache (OMNITOK_LM_KQ_FP8) held a NaN or an infinity

struct LmMerge {
    const float *part;         // [B][n_head][nchunk][2 + hd]
    const int32_t *cache_len;  // [B]
    int n_head, hd, nchunk;
    int chunk;                 // keys per attention chunk (LM_CHUNK, or LM_CHUNK_SHORT for caches of up to 4096 tokens)
    float *merged = nullptr;   // [B][n_head * hd] scratch: where the multi-stream MFMA path materialises the merged attention output
};

// ---- host side: what crosses the units ----------------------------------------------------------------------------------------

// One weight matrix of the decode step.  w32: the fp32 matrix | w16 != nullptr: its packed image in format fmt (OMNITOK_LM_W_BF16 /
// _FP16), which every group of streams then takes: the 16-bit kernels measured faster than the fp32 ones over the rounded fp32 image
// at 1, 2, 4 and 8 streams, so no group is routed back.
// w8 != nullptr (omnitok_lm_set_decode_quant, OMNITOK_LM_DQ_FP8): the e4m3fn image of the matrix [N, K] and its per-row scales
// scale [N] (powers of two).  Only lm_gemv_any reads them -- the decode step of fewer than "lm_streams_min" streams -- and there they
// take precedence over w32 / w16; every other consumer of an LmMat keeps reading the weight format's images.
struct LmMat { const float *w32; const void *w16; int fmt; const void *w8 = nullptr; const float *scale = nullptr; };  // w16 == nullptr: fp32
// the one dispatch on the weight format: f(the matrix as const float * | const lm_bf16 * | const lm_fp16 *)
template <class F>
auto lm_with_wt(const LmMat &m, F &&f) {
    if (!m.w16) return f(m.w32);
    if (m.fmt == OMNITOK_LM_W_BF16) return f(static_cast<const lm_bf16 *>(m.w16));
    return f(static_cast<const lm_fp16 *>(m.w16));
}
// ... and with the fp8 image in front, for the two VALU GEMV kernels: f(const lm_fp8 *) when the matrix carries one
template <class F>
auto lm_with_wt_dq(const LmMat &m, F &&f) {
    if (m.w8) return f(static_cast<const lm_fp8 *>(m.w8));
    return lm_with_wt(m, f);
}
// the one dispatch on the cache format: f(a value of the format's element type)
template <class F>
auto lm_with_kfmt(int kvfmt, F &&f) {
    if (kvfmt == OMNITOK_LM_KV_FP32) return f(float{});
    if (kvfmt == OMNITOK_LM_KV_BF16) return f(lm_bf16{});
    return f(lm_fp16{});
}
// ... and on the cache's storage: lm_fp8 under OMNITOK_LM_KQ_FP8, whatever the format
template <class F>
auto lm_with_kt(int kvfmt, int kq, F &&f) {
    if (kq == OMNITOK_LM_KQ_FP8) return f(lm_fp8{});
    return lm_with_kfmt(kvfmt, f);
}

// One nn.Linear call of the decode step: y = act(LN(x) W^T + bias) (+ residual) for B rows.  bias, residual and the LayerNorm pair
// may be nullptr (ln_g and ln_b come together); act 1 = exact GELU; residual may be y.
struct LmLinear { const float *x; LmMat w; const float *bias, *residual, *ln_g, *ln_b; float *y; int B, N, K, act; };
// The instantiations both VALU GEMV kernels exist in, for a group of c.B = 8 | 4 | 2 | 1 streams: the attention merge as prologue
// (xm: no LayerNorm, no GELU), or LayerNorm or not x GELU or not.  f(BQ, ACT, LN, XM) as std::integral_constant values.
template <class F>
auto lm_with_gemv_cfg(const LmLinear &c, bool xm, F &&f) {
    auto shape = [&](auto bq) {
        const std::integral_constant<int, 0> a0; const std::integral_constant<int, 1> a1;
        const std::false_type no; const std::true_type yes;
        if (xm) return f(bq, a0, no, yes);
        if (c.ln_g) return c.act ? f(bq, a1, yes, no) : f(bq, a0, yes, no);
        return c.act ? f(bq, a1, no, no) : f(bq, a0, no, no);
    };
    switch (c.B) {
        case 8: return shape(std::integral_constant<int, 8>{});
        case 4: return shape(std::integral_constant<int, 4>{});
        case 2: return shape(std::integral_constant<int, 2>{});
        default: return shape(std::integral_constant<int, 1>{});
    }
}

// grow-only device workspace: *p holds *have bytes; a larger need frees it and allocates need_bytes
inline int lm_grow(void **p, int64_t *have, int64_t need_bytes) {
    if (*have >= need_bytes) return OMNITOK_OK;
    if (*p) OT_HIP(hipFree(*p));  // (synchronises: no earlier call still uses it)
    *p = nullptr;
    *have = 0;
    OT_HIP(hipMalloc(p, (size_t)need_bytes));
    *have = need_bytes;
    return OMNITOK_OK;
}

extern int g_lm_streams_min;  // lm_gemm_mfma.hip

// lm_gemv.hip.  y = act(LN(x) W^T + b) (+ residual) for B rows, in groups of up to 8 rows per pass over the weights.
// mg != nullptr: the activations are the merged attention partials (c.x unused).
int lm_gemv_any(const LmLinear &c, const LmMerge *mg, hipStream_t stream);
// the checks the three exported GEMVs share: sizes (1 <= B <= bmax), the LayerNorm pair, act, alignment of x and w (of y: y16)
int lm_linear_check(const char *who, int bmax, const LmLinear &c, bool y16);
// lm_gemv_ks.hip / lm_gemm_mfma.hip.  One group of c.B streams on lm_gemv_ks_kernel / lm_gemm4_kernel: false = not its shape, no launch
bool lm_gemv_ks_try(const LmLinear &c, const LmMerge &mg, bool xm, hipStream_t stream);  // xm: mg feeds the prologue (c.x unused)
bool lm_gemm4_try(const LmLinear &c, hipStream_t stream);
void lm_trace_reset();
// lm_gemm_mfma.hip.  y = act(LN(x) W^T + b) (+ residual) for 1 <= B <= 128 streams on lm_gemm_streams_kernel.  xn: scratch [B, K] for
// the normalised activations (needed when c.ln_g), part: scratch of lm_streams_part_floats(B, N, K) floats.
int lm_gemm_streams_any(const LmLinear &c, float *xn, float *part, hipStream_t stream);
int64_t lm_streams_part_floats(int B, int N, int K);
// lm_gemm_streams16.hip.  y = act(a16 [B, K] . w16 [N, K]^T + bias) (+ residual) for 1 <= B <= 128 streams on lm_gemm_streams16_kernel into
// y32 or (rounded to fmt, no residual) y16: the contract of omnitok_lm_gemm_streams16 without its argument checks.  part: scratch of
// lm_streams16_part_floats(B, N, K) floats; an fp16 +-inf raises LM_FLAG_SF16_RANGE in *flag
int lm_gemm_streams16(const void *a16, const void *w16, int fmt, const float *bias, const float *residual, float *y32, void *y16, int B,
                      int N, int K, int act, float *part, int *flag, hipStream_t stream);
int64_t lm_streams16_part_floats(int B, int N, int K);
// lm_attn.hip.  chunk partials only (the engine merges them inside the proj GEMV)
// prefill_T > 0: B * prefill_T query rows (row = b * T + t, keys 0..t), chunks sized for T keys
struct LmAttnArgs {
    const float *qkv;
    void *kc, *vc;             // K / V slabs of one layer, elements of kvfmt (e4m3fn bytes when kq is OMNITOK_LM_KQ_FP8)
    int kvfmt;
    int kq;                    // OMNITOK_LM_KQ_*
    float *ksc, *vsc;          // kq == OMNITOK_LM_KQ_FP8: the slabs' row scales [max_batch][n_head][max_len]; otherwise unused
    const int32_t *cache_len;  // [B] (unused when prefill_T > 0)
    int B, n_head, head_dim, max_len;
    float *part;               // [rows][n_head][nchunk][2 + head_dim]
    int prefill_T;
    int *err_flag;             // may be nullptr
    int chunk;                 // keys per chunk: LM_CHUNK | LM_CHUNK_SHORT
};
int lm_attn_partials(const LmAttnArgs &a, hipStream_t stream);
// the one launch of lm_attn_merge_kernel from the partials of `rows` query rows (the caller checks the launch) into out32 [rows][n_head * hd]
// or, rounded to fmt (OMNITOK_LM_W_BF16 | _FP16), out16: the proj GEMM's operand of a PF_W16 prefill; an fp16 +-inf raises
// flag_bit (LM_FLAG_PF16_RANGE | LM_FLAG_SF16_RANGE) in *flag.  Exactly one of out32 / out16.  The decode step passes cache_len and its chunk, the prefill prefill_T and LM_CHUNK
void lm_attn_merge(const float *part, const int32_t *cache_len, int n_head, int hd, int nchunk, int prefill_T, float *out32, void *out16,
                   int fmt, int64_t rows, int *flag, int chunk, hipStream_t stream, int flag_bit = LM_FLAG_PF16_RANGE);
// qkv [B * T, 3C] -> cache rows 0 .. T - 1 of every stream | rows t0 .. t0 + n - 1 of one stream's slabs -> fp32.  kq / ksc / vsc as
// in LmAttnArgs (lm_kv_read: the scales of that stream's rows)
int lm_kv_scatter(const float *qkv, void *kc, void *vc, int kvfmt, int kq, float *ksc, float *vsc, int64_t rows, int T, int n_head, int hd,
                  int max_len, int *err_flag, hipStream_t stream);
int lm_kv_read(const void *kc, const void *vc, int kvfmt, int kq, const float *ksc, const float *vsc, int t0, int n, int n_head, int hd,
               int max_len, float *k_out, float *v_out, hipStream_t stream);
// lm_attn_prefill.hip.  Causal attention of B streams x T rows straight from qkv [B * T, 3C] into out32 [B * T, C] or (rounded to out_fmt)
// out16, with fp32 operands (op_fmt 0) or Q, K, V and P rounded once to op_fmt (OMNITOK_LM_W_BF16 | _FP16) on the 16-bit MFMA: the contract
// of omnitok_lm_attn_prefill / omnitok_lm_attn_prefill16, their argument checks included (`who` names the entry in the messages); an fp16
// operand of +-inf raises LM_FLAG_AOP16_RANGE in *flag
int lm_attn_prefill_any(const char *who, const float *qkv, int B, int T, int n_head, int head_dim, int op_fmt, float *out32, void *out16,
                        int out_fmt, int *flag, hipStream_t stream);
// lm_engine.hip.  nn.LayerNorm(x) over `rows` rows of K floats into y32 or, each value rounded to fmt (OMNITOK_LM_W_BF16 | _FP16), y16; an
// fp16 +-inf raises flag_bit (LM_FLAG_PF16_RANGE | LM_FLAG_SF16_RANGE) in *flag.  Exactly one of y32 / y16
int lm_layernorm_rows(const float *x, const float *g, const float *beta, float *y32, void *y16, int fmt, int64_t rows, int K, int *flag,
                      hipStream_t stream, int flag_bit = LM_FLAG_PF16_RANGE);
// lm_gemm16.hip.  y = act(a16 [M, K] . w16 [N, K]^T + bias) (+ residual) on the 16-bit MFMA into y32 or (rounded to fmt) y16: the
// contract of omnitok_lm_gemm16, its argument checks included
int lm_gemm16(const void *a16, const void *w16, int fmt, const float *bias, const float *residual, float *y32, void *y16, int64_t M,
              int N, int K, int act, int *flag, hipStream_t stream);
// lm_quant.hip.  The fp8 image of w [N, K] (K % 4 == 0): scale[n] = 2^e with e the smallest integer such that amax_n 2^-e <= 448 (1 for
// a zero row), q8[n, k] = e4m3fn(w[n, k] 2^-e), one round to nearest even.  A row with a NaN or an infinity sets flags[n / seg_rows]
// (flags may be nullptr); what q8 and scale hold for such a row is not specified.  The contract of omnitok_lm_quantize_fp8 without
// its argument checks
int lm_quantize_fp8(const float *w, void *q8, float *scale, int N, int K, int seg_rows, int *flags, hipStream_t stream);

}  // namespace omnitok
