// LM decode: the engine -- struct omnitok_lm, its weights, cache and workspaces, the decode step, the batched prefill and its loss --
// and the small kernels only it launches (index: lm_common.h)
#include "lm_common.h"
#include "gemm_x_common.h"  // gelu_erf

#include <algorithm>
#include <map>
#include <string>
#include <vector>

namespace omnitok {

int g_lm_attn_short = 1;  // "lm_attn_short": 1 = 128-key attention chunks for caches of up to 4096 tokens (read at omnitok_lm_alloc_cache) | 0 = 256
int g_lm_loss_chunk_rows = 2048;  // "lm_loss_chunk_rows": rows per head-GEMM block of omnitok_lm_prefill_loss (a guess, not measured)

// x = token_embedding + position_embedding (reference gpt.py:209-226 / 238-258): the token embedding is
// tok_emb[idx] or an explicit vector (`embeddings=`, emb [B, C]); the position embedding is pos_emb[pos],
// plus the vtokens_pos term (extra [B, C], gathered from vtokens_pos_emb by the caller) when given -- summed
// in the reference's order: tok + (pos + extra).
__global__ __launch_bounds__(256) void lm_embed_kernel(const int64_t *__restrict__ idx, const int32_t *__restrict__ pos,
                                                       const float *__restrict__ tok, const float *__restrict__ pe,
                                                       const float *__restrict__ emb, const float *__restrict__ extra,
                                                       float *__restrict__ x, int C, int vocab, int block_size) {
    const int b = blockIdx.x;
    int64_t id = idx ? idx[b] : 0;
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    int p = pos[b];
    p = p < 0 ? 0 : (p >= block_size ? block_size - 1 : p);
    const float *src = emb ? emb + (int64_t)b * C : tok + id * C;
    for (int i = threadIdx.x * 4; i < C; i += 256 * 4) {
        const f32x4 a = *reinterpret_cast<const f32x4 *>(src + i);
        f32x4 c = *reinterpret_cast<const f32x4 *>(pe + (int64_t)p * C + i);
        if (extra) c = c + *reinterpret_cast<const f32x4 *>(extra + (int64_t)b * C + i);
        *reinterpret_cast<f32x4 *>(x + (int64_t)b * C + i) = a + c;
    }
}

// ---- batched prefill of a conditioning prefix (the same arithmetic as T decode steps, as GEMMs; with OMNITOK_LM_PF_W16 the GEMMs run
// on the 16-bit MFMA over activations rounded to the weight format instead: lm_gemm16.hip; with OMNITOK_LM_PA_TILED the attention runs
// tiled from qkv, lm_attn_prefill.hip: on the fp32-input MFMA, and "same arithmetic as T decode steps" holds to rounding, not to the
// bit, or with 16-bit operands on the bf16 / fp16 MFMA, and it no longer holds.  One layer loop for all of them: LmPrefill) ------
// positions t < Te take the explicit embeddings emb[b, t] (prepended, gpt.py:214-216), the rest tok_emb[idx[b, t - Te]]
__global__ __launch_bounds__(256) void lm_embed_seq_kernel(const int64_t *__restrict__ idx, const float *__restrict__ tok,
                                                           const float *__restrict__ pe, const float *__restrict__ emb,
                                                           int Te, const float *__restrict__ extra,
                                                           float *__restrict__ x, int T, int C, int vocab) {
    const int64_t row = blockIdx.x;  // b * T + t
    const int t = (int)(row % T);
    const int64_t b = row / T;
    const float *src;
    if (t < Te) {
        src = emb + (b * Te + t) * C;
    } else {
        int64_t id = idx[b * (T - Te) + (t - Te)];
        id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
        src = tok + id * C;
    }
    for (int i = threadIdx.x * 4; i < C; i += 256 * 4) {
        f32x4 c = *reinterpret_cast<const f32x4 *>(pe + (int64_t)t * C + i);
        if (extra) c = c + *reinterpret_cast<const f32x4 *>(extra + row * C + i);
        *reinterpret_cast<f32x4 *>(x + row * C + i) = *reinterpret_cast<const f32x4 *>(src + i) + c;
    }
}

// nn.LayerNorm over rows of any width (two-pass, eps 1e-5): one wave per row.  OT = float: y fp32 | lm_bf16 / lm_fp16: the same
// values rounded once (lm_round16) into packed 16-bit rows, the GEMM operand of a PF_W16 prefill or an SF_W16 step; an fp16 result of
// +-inf raises flag_bit in *flag
template <typename OT>
__global__ __launch_bounds__(256) void lm_layernorm_rows_kernel(const float *__restrict__ x, const float *__restrict__ g,
                                                                const float *__restrict__ beta, OT *__restrict__ y,
                                                                int64_t rows, int K, int *__restrict__ flag, int flag_bit) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float *xr = x + row * K;
    float s = 0.0f;
    for (int k = lane * 4; k < K; k += 256) {
        const f32x4 v = *reinterpret_cast<const f32x4 *>(xr + k);
        s += (v[0] + v[1]) + (v[2] + v[3]);
    }
    const float mean = wave_allsum(s) / (float)K;
    float q = 0.0f;
    for (int k = lane * 4; k < K; k += 256) {
        const f32x4 v = *reinterpret_cast<const f32x4 *>(xr + k);
        const float a0 = v[0] - mean, a1 = v[1] - mean, a2 = v[2] - mean, a3 = v[3] - mean;
        q += (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
    }
    const float rstd = 1.0f / sqrtf(wave_allsum(q) / (float)K + 1e-5f);
    for (int k = lane * 4; k < K; k += 256) {
        f32x4 v = *reinterpret_cast<const f32x4 *>(xr + k);
        const f32x4 g4 = *reinterpret_cast<const f32x4 *>(g + k), b4 = *reinterpret_cast<const f32x4 *>(beta + k);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (v[e] - mean) * rstd * g4[e] + b4[e];
        if constexpr (__is_same(OT, float)) {
            *reinterpret_cast<f32x4 *>(y + row * K + k) = v;
        } else {
            bool inf = false;
            *reinterpret_cast<u32x2 *>(y + row * K + k) = LmKV<OT>::store4(v, inf);
            if (inf && flag) atomicOr(flag, flag_bit);
        }
    }
}

__global__ __launch_bounds__(256) void lm_gelu_kernel(float *__restrict__ x, int64_t n4) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    f32x4 v = reinterpret_cast<f32x4 *>(x)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = gelu_erf(v[e]);
    reinterpret_cast<f32x4 *>(x)[i] = v;
}

__global__ void lm_set_len_kernel(int32_t *pos, int32_t *cache_len, int B, int T) {
    const int b = threadIdx.x;
    if (b < B) {
        pos[b] = T;
        cache_len[b] = T;
    }
}

__global__ void lm_advance_kernel(int32_t *pos, int32_t *cache_len, int B) {
    const int b = threadIdx.x;
    if (b < B) {
        pos[b] += 1;
        cache_len[b] += 1;
    }
}

// rows of a (key | query | value) trio concatenated as (query | key | value) [3C, C] / [3C]
__global__ void lm_concat3_kernel(const float *a, const float *b, const float *c, int64_t n, float *out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 3 * n) return;
    out[i] = i < n ? a[i] : (i < 2 * n ? b[i - n] : c[i - 2 * n]);
}

// omnitok_lm_set_weight_format: rounds a matrix to bf16 / fp16 (round to nearest even: the bits of tensor.to(torch.bfloat16) /
// .to(torch.float16), fp16 subnormals included), writes the packed image for the decode GEMVs and puts the rounded values back into
// the fp32 image in place (what the prefill GEMMs read).  An fp16 result of +-inf sets flags[element / seg]: one flag per source
// tensor of a concatenated matrix.  n % 4 == 0.
template <int FMT>
__global__ __launch_bounds__(256) void lm_round_w16_kernel(float *__restrict__ w, unsigned short *__restrict__ out, int64_t n4,
                                                           int64_t seg, int *__restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    f32x4 v = reinterpret_cast<const f32x4 *>(w)[i];
    unsigned short h[4];
    bool inf = false;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float f = v[e];  // (a scalar copy: __builtin_bit_cast of a vector ELEMENT reads element 0 with this compiler)
        if constexpr (FMT == OMNITOK_LM_W_BF16) {
            h[e] = lm_round16<lm_bf16>(f);
            v[e] = __builtin_bit_cast(float, (unsigned)h[e] << 16);
        } else {
            h[e] = lm_round16<lm_fp16>(f);
            v[e] = (float)__builtin_bit_cast(_Float16, h[e]);
            inf = inf || lm_f16_is_inf(h[e]);
        }
    }
    reinterpret_cast<f32x4 *>(w)[i] = v;
    reinterpret_cast<u32x2 *>(out)[i] = u32x2{(unsigned)h[0] | ((unsigned)h[1] << 16), (unsigned)h[2] | ((unsigned)h[3] << 16)};
    if (inf) flags[(i * 4) / seg] = 1;
}

int lm_layernorm_rows(const float *x, const float *g, const float *beta, float *y32, void *y16, int fmt, int64_t rows, int K, int *flag,
                      hipStream_t stream, int flag_bit) {
    auto launch = [&](auto *y, int *fl) {
        typedef std::remove_pointer_t<decltype(y)> OT;
        hipLaunchKernelGGL(lm_layernorm_rows_kernel<OT>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, x, g, beta, y, rows, K, fl,
                           flag_bit);
    };
    if (y32) launch(y32, static_cast<int *>(nullptr));
    else if (fmt == OMNITOK_LM_W_BF16) launch(static_cast<lm_bf16 *>(y16), flag);
    else launch(static_cast<lm_fp16 *>(y16), flag);
    OT_LAUNCH_CHECK(y32 ? "lm_layernorm_rows" : "lm_layernorm_rows16");
    return OMNITOK_OK;
}

}  // namespace omnitok

using namespace omnitok;

// ---------------------------------------------------------------------------------------------
// engine
// ---------------------------------------------------------------------------------------------
struct LmLayer {
    const float *ln1w, *ln1b, *ln2w, *ln2b;
    LmMat wqkv;   // (query | key | value) concatenated at finalize
    float *bqkv;
    LmMat wproj, w1, w2;  // (w16: the packed 16-bit image, weight_format != FP32)
    const float *bproj, *b1, *b2;
};

// bytes of one cache element: a byte under OMNITOK_LM_KQ_FP8 (the format then decides nothing about storage), else the format's
static int lm_kv_elem_bytes(int fmt, int kq) { return kq == OMNITOK_LM_KQ_FP8 ? 1 : fmt == OMNITOK_LM_KV_FP32 ? 4 : 2; }

struct omnitok_lm {
    omnitok_lm_config cfg;
    std::map<std::string, std::vector<int64_t>> spec;
    std::map<std::string, float *> w;
    std::vector<void *> owned;
    std::vector<LmLayer> layers;
    bool finalized = false;
    int weight_format = OMNITOK_LM_W_FP32;  // of the matrices a decode step streams (omnitok_lm_set_weight_format)
    int decode_quant = OMNITOK_LM_DQ_NONE;  // the fp8 image a decode step of up to 16 streams reads instead (omnitok_lm_set_decode_quant)
    int prefill_format = OMNITOK_LM_PF_FP32;  // how the batched prefill runs its GEMMs (omnitok_lm_set_prefill_format)
    int prefill_attention = OMNITOK_LM_PA_ROWS;  // how the batched prefill runs its attention (omnitok_lm_set_prefill_attention)
    int prefill_attention_operands = OMNITOK_LM_AOP_FP32;  // operand format of the tiled attention (omnitok_lm_set_prefill_attention_operands)
    int streams_format = OMNITOK_LM_SF_FP32;  // how a many-stream step runs its GEMMs (omnitok_lm_set_streams_format)
    LmMat head = {nullptr, nullptr, OMNITOK_LM_W_FP32};  // head.weight
    // cache + workspaces
    void *kv = nullptr;                       // [n_layer][2][max_batch][n_head][max_len][head_dim] elements of cache_format
    int cache_format = OMNITOK_LM_KV_FP32;    // element type of kv (omnitok_lm_set_cache_format; applies at omnitok_lm_alloc_cache)
    int cache_quant = OMNITOK_LM_KQ_NONE;     // OMNITOK_LM_KQ_FP8: kv holds e4m3fn bytes and kvs their row scales (omnitok_lm_set_cache_quant)
    float *kvs = nullptr;                     // [n_layer][2][max_batch][n_head][max_len] fp32 row scales (cache_quant only)
    int max_batch = 0, max_len = 0;
    int max_streams = 16;  // what omnitok_lm_alloc_cache accepts as max_batch (omnitok_lm_set_max_streams, up to 128)
    int chunk = LM_CHUNK;  // keys per attention chunk of the decode step (omnitok_lm_alloc_cache)
    int *err_flag = nullptr;  // LM_FLAG_PAST_CACHE: the attention kernel met a stream past max_len | LM_FLAG_FP16_RANGE: a K/V value
                              // stored into an fp16 cache rounded to +-inf (the append, the prefill's scatter) | LM_FLAG_KV8_NONFINITE: a
                              // K/V row stored into an fp8 cache held a NaN or an infinity (the same two places)
    float *x = nullptr, *qkv = nullptr, *att = nullptr, *hid = nullptr, *part = nullptr;
    float *gs = nullptr;  // K-split partials of lm_gemm_streams_kernel / lm_gemm_streams16_kernel (the many-stream step)
    unsigned short *x16 = nullptr, *h16 = nullptr;  // packed GEMM operands of an SF_W16 step: [max_batch, C] | [max_batch, 4 C] (one allocation)
    int64_t cache_bytes = 0;
    // grow-only prefill workspace (rows = B * T)
    float *pf = nullptr;
    int64_t pf_bytes = 0;
    // grow-only workspace of omnitok_lm_prefill_loss: a block of logits rows; nll [rows] | rank [rows] | reduction partials
    float *lg = nullptr;
    int64_t lg_bytes = 0;
    float *ce = nullptr;
    int64_t ce_rows = 0, ce_bytes = 0;
    int head_dim() const { return cfg.n_embd / cfg.n_head; }
    // the K slab of a layer and the V slab that follows it: [max_batch][n_head][max_len][head_dim] elements of cache_format each
    int64_t slab_bytes() const { return (int64_t)max_batch * cfg.n_head * max_len * head_dim() * lm_kv_elem_bytes(cache_format, cache_quant); }
    void *k_slab(int layer) const { return static_cast<char *>(kv) + 2 * layer * slab_bytes(); }
    void *v_slab(int layer) const { return static_cast<char *>(kv) + (2 * layer + 1) * slab_bytes(); }
    // ... and the scales of their rows: [max_batch][n_head][max_len] floats each (nullptr without a cache quant)
    int64_t slab_rows() const { return (int64_t)max_batch * cfg.n_head * max_len; }
    float *k_scales(int layer) const { return kvs ? kvs + 2 * layer * slab_rows() : nullptr; }
    float *v_scales(int layer) const { return kvs ? kvs + (2 * layer + 1) * slab_rows() : nullptr; }
};

static const float *LW(omnitok_lm *lm, const std::string &k) {
    auto it = lm->w.find(k);
    return it == lm->w.end() ? nullptr : it->second;
}

extern "C" int omnitok_lm_create(const omnitok_lm_config *cfg, omnitok_lm **out) {
    OT_CHECK_ARG(cfg && out, "lm_create: null pointer");
    const omnitok_lm_config &c = *cfg;
    OT_CHECK_ARG(c.n_layer > 0 && c.n_head > 0 && c.n_embd > 0 && c.vocab_size > 0 && c.block_size > 0,
                 "lm_create: bad config");
    const int hd = c.n_embd / c.n_head;
    if (c.n_embd % c.n_head || (hd != 64 && hd != 96 && hd != 128) || c.n_embd % 256) {
        set_error("lm_create: n_embd %d / n_head %d: head_dim must be 64, 96 or 128 and n_embd %% 256 == 0", c.n_embd,
                  c.n_head);
        return OMNITOK_ERR_UNSUPPORTED;
    }
    omnitok_lm *lm = new omnitok_lm();
    lm->cfg = c;
    const int64_t C = c.n_embd, V = c.vocab_size;
    lm->spec["pos_emb"] = {1, c.block_size, C};
    lm->spec["tok_emb.weight"] = {V, C};
    for (int i = 0; i < c.n_layer; ++i) {
        const std::string p = "blocks." + std::to_string(i);
        for (const char *n : {".ln1", ".ln2"}) {
            lm->spec[p + n + ".weight"] = {C};
            lm->spec[p + n + ".bias"] = {C};
        }
        for (const char *n : {".attn.key", ".attn.query", ".attn.value", ".attn.proj"}) {
            lm->spec[p + n + ".weight"] = {C, C};
            lm->spec[p + n + ".bias"] = {C};
        }
        lm->spec[p + ".mlp.0.weight"] = {4 * C, C};
        lm->spec[p + ".mlp.0.bias"] = {4 * C};
        lm->spec[p + ".mlp.2.weight"] = {C, 4 * C};
        lm->spec[p + ".mlp.2.bias"] = {C};
    }
    lm->spec["ln_f.weight"] = {C};
    lm->spec["ln_f.bias"] = {C};
    lm->spec["head.weight"] = {V, C};
    *out = lm;
    return OMNITOK_OK;
}

static void lm_free_cache(omnitok_lm *lm) {
    lm->pf_bytes = lm->lg_bytes = lm->ce_rows = lm->ce_bytes = 0;
    for (float **p : {&lm->x, &lm->qkv, &lm->att, &lm->hid, &lm->part, &lm->gs, &lm->pf, &lm->lg, &lm->ce})
        if (*p) {
            (void)hipFree(*p);
            *p = nullptr;
        }
    if (lm->x16) (void)hipFree(lm->x16);
    lm->x16 = lm->h16 = nullptr;
    if (lm->kv) (void)hipFree(lm->kv);
    lm->kv = nullptr;
    if (lm->kvs) (void)hipFree(lm->kvs);
    lm->kvs = nullptr;
    lm->cache_bytes = 0;
}

extern "C" void omnitok_lm_destroy(omnitok_lm *lm) {
    if (!lm) return;
    for (auto &kv : lm->w)
        if (kv.second) (void)hipFree(kv.second);
    for (void *p : lm->owned) (void)hipFree(p);
    lm_free_cache(lm);
    if (lm->err_flag) (void)hipFree(lm->err_flag);
    delete lm;
}

extern "C" int omnitok_lm_set_weight(omnitok_lm *lm, const char *name, const void *dev_ptr, const int64_t *shape,
                                     int ndim, omnitok_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    OT_CHECK_ARG(lm && name && dev_ptr && shape, "lm_set_weight: null pointer");
    auto it = lm->spec.find(name);
    if (it == lm->spec.end()) return 1;
    std::vector<int64_t> shp(shape, shape + ndim);
    if (shp != it->second) {
        std::string want, got;
        for (auto s : it->second) want += std::to_string(s) + ",";
        for (auto s : shp) got += std::to_string(s) + ",";
        set_error("lm_set_weight: size mismatch for %s: expected [%s] got [%s]", name, want.c_str(), got.c_str());
        return OMNITOK_ERR_INVALID;
    }
    int64_t n = 1;
    for (auto s : shp) n *= s;
    float *&p = lm->w[name];
    if (!p) OT_HIP(hipMalloc(reinterpret_cast<void **>(&p), (size_t)n * 4));
    OT_HIP(hipMemcpyAsync(p, dev_ptr, (size_t)n * 4, hipMemcpyDeviceToDevice, stream));
    lm->finalized = false;
    return OMNITOK_OK;
}

extern "C" int omnitok_lm_set_weight_format(omnitok_lm *lm, int fmt) {
    OT_CHECK_ARG(lm, "lm_set_weight_format: null engine");
    OT_CHECK_ARG(fmt == OMNITOK_LM_W_FP32 || fmt == OMNITOK_LM_W_BF16 || fmt == OMNITOK_LM_W_FP16,
                 "lm_set_weight_format: unknown format %d", fmt);
    lm->weight_format = fmt;
    lm->finalized = false;
    return OMNITOK_OK;
}

extern "C" int omnitok_lm_weight_format(omnitok_lm *lm) {
    OT_CHECK_ARG(lm, "lm_weight_format: null engine");
    return lm->weight_format;
}

extern "C" int omnitok_lm_set_decode_quant(omnitok_lm *lm, int q) {
    OT_CHECK_ARG(lm, "lm_set_decode_quant: null engine");
    OT_CHECK_ARG(q == OMNITOK_LM_DQ_NONE || q == OMNITOK_LM_DQ_FP8, "lm_set_decode_quant: unknown value %d", q);
    lm->decode_quant = q;
    lm->finalized = false;  // the images are made (or dropped) by the next finalize, from weights set again
    return OMNITOK_OK;
}

extern "C" int omnitok_lm_decode_quant(omnitok_lm *lm) {
    OT_CHECK_ARG(lm, "lm_decode_quant: null engine");
    return lm->decode_quant;
}

extern "C" int omnitok_lm_set_prefill_format(omnitok_lm *lm, int fmt) {
    OT_CHECK_ARG(lm, "lm_set_prefill_format: null engine");
    OT_CHECK_ARG(fmt == OMNITOK_LM_PF_FP32 || fmt == OMNITOK_LM_PF_W16, "lm_set_prefill_format: unknown format %d", fmt);
    lm->prefill_format = fmt;  // read at the next prefill: the weights, `finalized` and the cache are left alone
    return OMNITOK_OK;
}

extern "C" int omnitok_lm_prefill_format(omnitok_lm *lm) {
    OT_CHECK_ARG(lm, "lm_prefill_format: null engine");
    return lm->prefill_format;
}

extern "C" int omnitok_lm_set_prefill_attention(omnitok_lm *lm, int mode) {
    OT_CHECK_ARG(lm, "lm_set_prefill_attention: null engine");
    OT_CHECK_ARG(mode == OMNITOK_LM_PA_ROWS || mode == OMNITOK_LM_PA_TILED, "lm_set_prefill_attention: unknown mode %d", mode);
    lm->prefill_attention = mode;  // read at the next prefill: the weights, `finalized` and the cache are left alone
    return OMNITOK_OK;
}

extern "C" int omnitok_lm_prefill_attention(omnitok_lm *lm) {
    OT_CHECK_ARG(lm, "lm_prefill_attention: null engine");
    return lm->prefill_attention;
}

extern "C" int omnitok_lm_set_prefill_attention_operands(omnitok_lm *lm, int fmt) {
    OT_CHECK_ARG(lm, "lm_set_prefill_attention_operands: null engine");
    OT_CHECK_ARG(fmt == OMNITOK_LM_AOP_FP32 || fmt == OMNITOK_LM_AOP_BF16 || fmt == OMNITOK_LM_AOP_FP16,
                 "lm_set_prefill_attention_operands: unknown operands format %d", fmt);
    lm->prefill_attention_operands = fmt;  // read at the next prefill: the weights, `finalized` and the cache are left alone
    return OMNITOK_OK;
}

extern "C" int omnitok_lm_prefill_attention_operands(omnitok_lm *lm) {
    OT_CHECK_ARG(lm, "lm_prefill_attention_operands: null engine");
    return lm->prefill_attention_operands;
}

extern "C" int omnitok_lm_set_streams_format(omnitok_lm *lm, int fmt) {
    OT_CHECK_ARG(lm, "lm_set_streams_format: null engine");
    OT_CHECK_ARG(fmt == OMNITOK_LM_SF_FP32 || fmt == OMNITOK_LM_SF_W16, "lm_set_streams_format: unknown format %d", fmt);
    lm->streams_format = fmt;  // read at the next step: the weights, `finalized` and the cache are left alone
    return OMNITOK_OK;
}

extern "C" int omnitok_lm_streams_format(omnitok_lm *lm) {
    OT_CHECK_ARG(lm, "lm_streams_format: null engine");
    return lm->streams_format;
}

extern "C" int omnitok_lm_set_cache_format(omnitok_lm *lm, int fmt) {
    OT_CHECK_ARG(lm, "lm_set_cache_format: null engine");
    OT_CHECK_ARG(fmt == OMNITOK_LM_KV_FP32 || fmt == OMNITOK_LM_KV_BF16 || fmt == OMNITOK_LM_KV_FP16,
                 "lm_set_cache_format: unknown format %d", fmt);
    lm_free_cache(lm);  // the cache and the step workspaces: the next step / prefill asks for omnitok_lm_alloc_cache
    lm->max_batch = lm->max_len = 0;
    lm->cache_format = fmt;
    return OMNITOK_OK;
}

extern "C" int omnitok_lm_cache_format(omnitok_lm *lm) {
    OT_CHECK_ARG(lm, "lm_cache_format: null engine");
    return lm->cache_format;
}

extern "C" int omnitok_lm_set_cache_quant(omnitok_lm *lm, int q) {
    OT_CHECK_ARG(lm, "lm_set_cache_quant: null engine");
    OT_CHECK_ARG(q == OMNITOK_LM_KQ_NONE || q == OMNITOK_LM_KQ_FP8, "lm_set_cache_quant: unknown value %d", q);
    lm_free_cache(lm);  // the cache and the step workspaces: the next step / prefill asks for omnitok_lm_alloc_cache
    lm->max_batch = lm->max_len = 0;
    lm->cache_quant = q;
    return OMNITOK_OK;
}

extern "C" int omnitok_lm_cache_quant(omnitok_lm *lm) {
    OT_CHECK_ARG(lm, "lm_cache_quant: null engine");
    return lm->cache_quant;
}

extern "C" int omnitok_lm_set_max_streams(omnitok_lm *lm, int n) {
    OT_CHECK_ARG(lm, "lm_set_max_streams: null engine");
    OT_CHECK_ARG(n >= 1 && n <= 128, "lm_set_max_streams: %d streams (1 .. 128)", n);
    lm_free_cache(lm);  // the cache and the step workspaces: the next step / prefill asks for omnitok_lm_alloc_cache
    lm->max_batch = lm->max_len = 0;
    lm->max_streams = n;
    return OMNITOK_OK;
}

extern "C" int omnitok_lm_max_streams(omnitok_lm *lm) {
    OT_CHECK_ARG(lm, "lm_max_streams: null engine");
    return lm->max_streams;
}

extern "C" int64_t omnitok_lm_step_weight_bytes(omnitok_lm *lm) {
    if (!lm) return 0;
    const int64_t C = lm->cfg.n_embd, V = lm->cfg.vocab_size;
    if (lm->decode_quant == OMNITOK_LM_DQ_FP8)  // one byte per weight and one fp32 scale per output row
        return (12 * C * C * lm->cfg.n_layer + V * C) + (12 * C * lm->cfg.n_layer + V) * 4;
    return (12 * C * C * lm->cfg.n_layer + V * C) * (lm->weight_format == OMNITOK_LM_W_FP32 ? 4 : 2);
}

extern "C" int omnitok_lm_finalize(omnitok_lm *lm, omnitok_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    OT_CHECK_ARG(lm, "lm_finalize: null");
    for (auto &kv : lm->spec)
        if (!lm->w.count(kv.first)) {
            set_error("lm_finalize: missing weight %s", kv.first.c_str());
            return OMNITOK_ERR_STATE;
        }
    for (auto &kv : lm->w)
        if (!kv.second) {  // q/k/v were folded into wqkv by an earlier finalize and released
            set_error("lm_finalize: %s was released by a previous finalize; set all weights again", kv.first.c_str());
            return OMNITOK_ERR_STATE;
        }
    OT_HIP(hipStreamSynchronize(stream));
    for (void *p : lm->owned) (void)hipFree(p);
    lm->owned.clear();
    lm->layers.clear();
    const int64_t C = lm->cfg.n_embd;
    for (int i = 0; i < lm->cfg.n_layer; ++i) {
        const std::string p = "blocks." + std::to_string(i);
        LmLayer L;
        L.ln1w = LW(lm, p + ".ln1.weight");
        L.ln1b = LW(lm, p + ".ln1.bias");
        L.ln2w = LW(lm, p + ".ln2.weight");
        L.ln2b = LW(lm, p + ".ln2.bias");
        void *wq = nullptr, *bq = nullptr;
        OT_HIP(hipMalloc(&wq, (size_t)3 * C * C * 4));
        OT_HIP(hipMalloc(&bq, (size_t)3 * C * 4));
        lm->owned.push_back(wq);
        lm->owned.push_back(bq);
        L.wqkv = {static_cast<float *>(wq), nullptr, OMNITOK_LM_W_FP32};
        L.bqkv = static_cast<float *>(bq);
        hipLaunchKernelGGL(lm_concat3_kernel, dim3((unsigned)((3 * C * C + 255) / 256)), dim3(256), 0, stream,
                           LW(lm, p + ".attn.query.weight"), LW(lm, p + ".attn.key.weight"),
                           LW(lm, p + ".attn.value.weight"), C * C, static_cast<float *>(wq));
        hipLaunchKernelGGL(lm_concat3_kernel, dim3((unsigned)((3 * C + 255) / 256)), dim3(256), 0, stream,
                           LW(lm, p + ".attn.query.bias"), LW(lm, p + ".attn.key.bias"), LW(lm, p + ".attn.value.bias"),
                           C, L.bqkv);
        OT_LAUNCH_CHECK("lm_concat3");
        L.wproj = {LW(lm, p + ".attn.proj.weight"), nullptr, OMNITOK_LM_W_FP32};
        L.bproj = LW(lm, p + ".attn.proj.bias");
        L.w1 = {LW(lm, p + ".mlp.0.weight"), nullptr, OMNITOK_LM_W_FP32};
        L.b1 = LW(lm, p + ".mlp.0.bias");
        L.w2 = {LW(lm, p + ".mlp.2.weight"), nullptr, OMNITOK_LM_W_FP32};
        L.b2 = LW(lm, p + ".mlp.2.bias");
        lm->layers.push_back(L);
    }
    lm->head = {LW(lm, "head.weight"), nullptr, OMNITOK_LM_W_FP32};
    // one flag per source tensor of the five matrix families (6 per layer + the head) -> the tensor's name
    const int nflags = 6 * lm->cfg.n_layer + 1;
    auto first_flagged = [&](int *flags, std::string *name) -> int {
        std::vector<int> hf((size_t)nflags);
        OT_HIP(hipMemcpyAsync(hf.data(), flags, (size_t)nflags * sizeof(int), hipMemcpyDeviceToHost, stream));
        OT_HIP(hipStreamSynchronize(stream));
        for (int f = 0; f < nflags && name->empty(); ++f)
            if (hf[(size_t)f]) {
                static const char *const names[6] = {".attn.query.weight", ".attn.key.weight", ".attn.value.weight",
                                                     ".attn.proj.weight", ".mlp.0.weight", ".mlp.2.weight"};
                *name = f == nflags - 1 ? std::string("head.weight") : "blocks." + std::to_string(f / 6) + names[f % 6];
            }
        return OMNITOK_OK;
    };
    std::string nonfinite;  // the first tensor with a NaN or an infinity (only looked for by the fp8 quantiser)
    if (lm->decode_quant == OMNITOK_LM_DQ_FP8) {
        // the fp8 image and the row scales of the five matrix families, for the decode step of up to 16 streams -- made BEFORE the
        // 16-bit rounding below overwrites the fp32 images: always from the fp32 originals, whatever the weight format is
        const int64_t V = lm->cfg.vocab_size;
        int *flags = nullptr;
        OT_HIP(hipMalloc(reinterpret_cast<void **>(&flags), (size_t)nflags * sizeof(int)));
        lm->owned.push_back(flags);
        OT_HIP(hipMemsetAsync(flags, 0, (size_t)nflags * sizeof(int), stream));
        auto quant = [&](LmMat &m, int64_t N, int64_t K, int64_t seg_rows, int *fl) -> int {
            void *p8 = nullptr, *sc = nullptr;
            OT_HIP(hipMalloc(&p8, (size_t)(N * K)));
            lm->owned.push_back(p8);
            OT_HIP(hipMalloc(&sc, (size_t)N * 4));
            lm->owned.push_back(sc);
            if (int rc = lm_quantize_fp8(m.w32, p8, static_cast<float *>(sc), (int)N, (int)K, (int)seg_rows, fl, stream)) return rc;
            m.w8 = p8;
            m.scale = static_cast<const float *>(sc);
            return OMNITOK_OK;
        };
        for (int i = 0; i < lm->cfg.n_layer; ++i) {
            LmLayer &L = lm->layers[i];
            int *fl = flags + 6 * i;
            if (int rc = quant(L.wqkv, 3 * C, C, C, fl)) return rc;
            if (int rc = quant(L.wproj, C, C, C, fl + 3)) return rc;
            if (int rc = quant(L.w1, 4 * C, C, 4 * C, fl + 4)) return rc;
            if (int rc = quant(L.w2, C, 4 * C, C, fl + 5)) return rc;
        }
        if (int rc = quant(lm->head, V, C, V, flags + 6 * lm->cfg.n_layer)) return rc;
        if (int rc = first_flagged(flags, &nonfinite)) return rc;
    }
    std::string overflow;  // the first tensor with an element outside the fp16 range
    if (lm->weight_format != OMNITOK_LM_W_FP32) {
        // 16-bit format: round the five matrix families on the device -- packed image for the decode GEMVs, rounded values back into
        // the fp32 image for the prefill GEMMs.  One overflow flag per source tensor (6 per layer + the head).
        const int fmt = lm->weight_format;
        const int64_t V = lm->cfg.vocab_size;
        int *flags = nullptr;
        OT_HIP(hipMalloc(reinterpret_cast<void **>(&flags), (size_t)nflags * sizeof(int)));
        lm->owned.push_back(flags);
        OT_HIP(hipMemsetAsync(flags, 0, (size_t)nflags * sizeof(int), stream));
        auto round = [&](LmMat &m, int64_t n, int64_t seg, int *fl) -> int {
            void *p16 = nullptr;
            OT_HIP(hipMalloc(&p16, (size_t)n * 2));
            lm->owned.push_back(p16);
            const int64_t n4 = n / 4;
            const dim3 grid((unsigned)((n4 + 255) / 256));
            hipLaunchKernelGGL(fmt == OMNITOK_LM_W_BF16 ? lm_round_w16_kernel<OMNITOK_LM_W_BF16> : lm_round_w16_kernel<OMNITOK_LM_W_FP16>, grid,
                               dim3(256), 0, stream, const_cast<float *>(m.w32), static_cast<unsigned short *>(p16), n4, seg, fl);
            OT_LAUNCH_CHECK("lm_round_w16");
            m.w16 = p16;
            m.fmt = fmt;
            return OMNITOK_OK;
        };
        for (int i = 0; i < lm->cfg.n_layer; ++i) {
            LmLayer &L = lm->layers[i];
            int *fl = flags + 6 * i;
            if (int rc = round(L.wqkv, 3 * C * C, C * C, fl)) return rc;
            if (int rc = round(L.wproj, C * C, C * C, fl + 3)) return rc;
            if (int rc = round(L.w1, 4 * C * C, 4 * C * C, fl + 4)) return rc;
            if (int rc = round(L.w2, 4 * C * C, 4 * C * C, fl + 5)) return rc;
        }
        if (int rc = round(lm->head, V * C, V * C, flags + 6 * lm->cfg.n_layer)) return rc;
        if (int rc = first_flagged(flags, &overflow)) return rc;
    }
    // the separate q/k/v copies are no longer needed: free them (2.7 GB model -> no duplicate)
    OT_HIP(hipStreamSynchronize(stream));
    for (int i = 0; i < lm->cfg.n_layer; ++i)
        for (const char *n : {".attn.key", ".attn.query", ".attn.value"})
            for (const char *s : {".weight", ".bias"}) {
                const std::string k = "blocks." + std::to_string(i) + n + s;
                // keep the map entry (finalize checks presence) but release the memory
                if (lm->w[k]) {
                    (void)hipFree(lm->w[k]);
                    lm->w[k] = nullptr;
                }
            }
    if (!nonfinite.empty()) {
        // as below: the q/k/v sources are gone, so the next finalize wants all weights set again
        set_error("lm_finalize: %s has a NaN or an infinity: the fp8 decode image (omnitok_lm_set_decode_quant, OMNITOK_LM_DQ_FP8) "
                  "needs finite weights; set all weights again", nonfinite.c_str());
        return OMNITOK_ERR_INVALID;
    }
    if (!overflow.empty()) {
        // the fp32 images already hold the fp16-rounded values (some +-inf).  The q/k/v sources were released above like after any
        // finalize, so a finalize in another format without setting the weights again is refused ("released by a previous finalize")
        set_error("lm_finalize: %s has an element that rounds to +-inf in fp16 (|w| >= 65520); use OMNITOK_LM_W_BF16 or "
                  "OMNITOK_LM_W_FP32 for this model, then set all weights again", overflow.c_str());
        return OMNITOK_ERR_INVALID;
    }
    lm->finalized = true;
    return OMNITOK_OK;
}

extern "C" int omnitok_lm_alloc_cache(omnitok_lm *lm, int max_batch, int max_len) {
    OT_CHECK_ARG(lm && max_batch > 0 && max_batch <= lm->max_streams && max_len > 0, "lm_alloc_cache: bad sizes (max_batch <= %d)",
                 lm ? lm->max_streams : 16);
    OT_CHECK_ARG(max_len <= LM_CHUNK * LM_MAX_CHUNKS && lm->cfg.n_head <= LM_MAX_HEADS,
                 "lm_alloc_cache: max_len <= %d and n_head <= %d", LM_CHUNK * LM_MAX_CHUNKS, LM_MAX_HEADS);
    lm_free_cache(lm);
    lm->max_batch = lm->max_len = 0;
    const omnitok_lm_config &c = lm->cfg;
    const int64_t C = c.n_embd;
    const int hd = c.n_embd / c.n_head;
    const int64_t per_layer = (int64_t)max_batch * c.n_head * max_len * hd;  // elements per K (or V)
    lm->chunk = g_lm_attn_short && max_len <= LM_CHUNK_SHORT * LM_MAX_CHUNKS ? LM_CHUNK_SHORT : LM_CHUNK;
    const int nchunk = (max_len + lm->chunk - 1) / lm->chunk;
    const int64_t kv_bytes = per_layer * 2 * c.n_layer * lm_kv_elem_bytes(lm->cache_format, lm->cache_quant);
    const int64_t scale_bytes = lm->cache_quant == OMNITOK_LM_KQ_FP8 ? per_layer / hd * 2 * c.n_layer * 4 : 0;  // one fp32 per cached row
    // split partials of the many-stream GEMMs of a step: the largest of its five shapes
    int64_t gs = 0;
    const int shapes[5][2] = {{(int)(3 * C), (int)C}, {(int)C, (int)C}, {(int)(4 * C), (int)C}, {(int)C, (int)(4 * C)}, {c.vocab_size, (int)C}};
    for (const auto &nk : shapes)  // (both streams formats: the switch may change after the cache exists)
        gs = std::max({gs, lm_streams_part_floats(max_batch, nk[0], nk[1]), lm_streams16_part_floats(max_batch, nk[0], nk[1])});
    // a failed allocation (193 GB of fp32 cache for 128 streams of the reference's model do not fit one device) returns its
    // error and leaves the engine without a cache
    auto alloc = [lm](void **p, int64_t bytes) {
        const hipError_t e = hipMalloc(p, (size_t)bytes);
        if (e != hipSuccess) {
            *p = nullptr;
            (void)hipGetLastError();
            lm_free_cache(lm);
            set_error("lm_alloc_cache: hipMalloc of %lld bytes failed: %s", (long long)bytes, hipGetErrorString(e));
        }
        return e == hipSuccess;
    };
    if (!alloc(&lm->kv, kv_bytes) || (scale_bytes > 0 && !alloc(reinterpret_cast<void **>(&lm->kvs), scale_bytes)) || !alloc(reinterpret_cast<void **>(&lm->x), max_batch * C * 4) ||
        !alloc(reinterpret_cast<void **>(&lm->qkv), max_batch * 3 * C * 4) ||
        !alloc(reinterpret_cast<void **>(&lm->att), max_batch * C * 4) ||
        !alloc(reinterpret_cast<void **>(&lm->hid), max_batch * 4 * C * 4) ||
        !alloc(reinterpret_cast<void **>(&lm->part), (int64_t)max_batch * c.n_head * nchunk * (2 + hd) * 4) ||
        (gs > 0 && !alloc(reinterpret_cast<void **>(&lm->gs), gs * 4)) ||
        !alloc(reinterpret_cast<void **>(&lm->x16), max_batch * 5 * C * 2))
        return OMNITOK_ERR_HIP;
    lm->h16 = lm->x16 + max_batch * C;
    lm->max_batch = max_batch;
    lm->max_len = max_len;
    lm->cache_bytes = kv_bytes + scale_bytes;
    if (!lm->err_flag) {
        OT_HIP(hipMalloc(reinterpret_cast<void **>(&lm->err_flag), sizeof(int)));
        OT_HIP(hipMemset(lm->err_flag, 0, sizeof(int)));
    }
    return OMNITOK_OK;
}

extern "C" int omnitok_lm_overflowed(omnitok_lm *lm, omnitok_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    OT_CHECK_ARG(lm, "lm_overflowed: null engine");
    if (!lm->err_flag) return 0;
    int h = 0;
    OT_HIP(hipMemcpyAsync(&h, lm->err_flag, sizeof(int), hipMemcpyDeviceToHost, stream));
    OT_HIP(hipStreamSynchronize(stream));
    if (h)
        if (int rc = device_fill_u32(lm->err_flag, 0u, 1, stream)) return rc;
    return h & (LM_FLAG_PAST_CACHE | LM_FLAG_FP16_RANGE | LM_FLAG_PF16_RANGE | LM_FLAG_AOP16_RANGE | LM_FLAG_SF16_RANGE | LM_FLAG_KV8_NONFINITE);
}

extern "C" int omnitok_lm_cache_read(omnitok_lm *lm, int layer, int b, int t0, int n, float *k_out, float *v_out,
                                     omnitok_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    OT_CHECK_ARG(lm && k_out && v_out, "lm_cache_read: null pointer");
    OT_CHECK_ARG(layer >= 0 && layer < lm->cfg.n_layer && b >= 0 && t0 >= 0 && n >= 0,
                 "lm_cache_read: layer %d (of %d), stream %d, rows %d + %d", layer, lm->cfg.n_layer, b, t0, n);
    if (!lm->kv) {
        set_error("lm_cache_read: no cache (omnitok_lm_alloc_cache)");
        return OMNITOK_ERR_STATE;
    }
    OT_CHECK_ARG(b < lm->max_batch && (int64_t)t0 + n <= lm->max_len, "lm_cache_read: stream %d (of %d), rows %d + %d (of %d)", b,
                 lm->max_batch, t0, n, lm->max_len);
    if (n == 0) return OMNITOK_OK;
    const omnitok_lm_config &c = lm->cfg;
    const int hd = lm->head_dim();
    const int64_t roff = (int64_t)b * c.n_head * lm->max_len;  // the stream's rows in a slab
    const int64_t off = roff * hd * lm_kv_elem_bytes(lm->cache_format, lm->cache_quant);
    return lm_kv_read(static_cast<const char *>(lm->k_slab(layer)) + off, static_cast<const char *>(lm->v_slab(layer)) + off,
                      lm->cache_format, lm->cache_quant, lm->kvs ? lm->k_scales(layer) + roff : nullptr,
                      lm->kvs ? lm->v_scales(layer) + roff : nullptr, t0, n, c.n_head, hd, lm->max_len, k_out, v_out, stream);
}

extern "C" int64_t omnitok_lm_cache_bytes(omnitok_lm *lm) { return lm ? lm->cache_bytes : 0; }

extern "C" int omnitok_lm_step(omnitok_lm *lm, const int64_t *idx, int32_t *pos, int32_t *cache_len, int B,
                               float *logits_out, int advance, omnitok_stream_t stream_) {
    return omnitok_lm_step_ex(lm, idx, nullptr, nullptr, pos, cache_len, B, logits_out, advance, stream_);
}


// One linear call of a decode step.  Below "lm_streams_min" streams the VALU kernels take it in groups of 8 / 4 / 2 / 1 (a merge mg
// happens inside the projection's prologue: c.x == nullptr).  From there on the many-stream GEMM does (lm_gemm_streams_kernel): one pass
// over the matrix for the whole batch; LayerNorm is a pass of its own into `att`, and the chunk partials are merged into `att` as a
// tensor (free again by then), which then feeds the projection.
// With OMNITOK_LM_SF_W16 the many-stream GEMM is lm_gemm_streams16_kernel over the packed weight image, and its operand is rounded once
// to the weight format where it is produced, the rounding points of a PF_W16 prefill: LayerNorm rows and the merged partials by their
// kernels' 16-bit form into x16, FC1's GELU output in its GEMM's epilogue into h16 -- which the one linear without LayerNorm or merge,
// FC2, reads.  An fp16 +-inf raises LM_FLAG_SF16_RANGE.
static int lm_step_linear(omnitok_lm *lm, LmLinear c, const LmMerge *mg, hipStream_t stream) {
    if (c.B < g_lm_streams_min) return lm_gemv_any(c, mg, stream);
    if (lm->streams_format == OMNITOK_LM_SF_W16) {
        const int fmt = c.w.fmt;
        const void *a16 = lm->h16;
        if (mg) {
            lm_attn_merge(mg->part, mg->cache_len, mg->n_head, mg->hd, mg->nchunk, 0, nullptr, lm->x16, fmt, c.B, lm->err_flag, mg->chunk,
                          stream, LM_FLAG_SF16_RANGE);
            OT_LAUNCH_CHECK("lm_attn_merge16");
            a16 = lm->x16;
        } else if (c.ln_g) {
            if (int rc = lm_layernorm_rows(c.x, c.ln_g, c.ln_b, nullptr, lm->x16, fmt, c.B, c.K, lm->err_flag, stream, LM_FLAG_SF16_RANGE))
                return rc;
            a16 = lm->x16;
        }
        return lm_gemm_streams16(a16, c.w.w16, fmt, c.bias, c.residual, c.act ? nullptr : c.y, c.act ? lm->h16 : nullptr, c.B, c.N, c.K,
                                 c.act, lm->gs, lm->err_flag, stream);
    }
    if (mg) {
        lm_attn_merge(mg->part, mg->cache_len, mg->n_head, mg->hd, mg->nchunk, 0, lm->att, nullptr, 0, c.B, nullptr, mg->chunk, stream);
        OT_LAUNCH_CHECK("lm_attn_merge");
        c.x = lm->att;
    }
    return lm_gemm_streams_any(c, lm->att, lm->gs, stream);
}

extern "C" int omnitok_lm_step_ex(omnitok_lm *lm, const int64_t *idx, const float *emb, const float *pos_extra,
                                  int32_t *pos, int32_t *cache_len, int B, float *logits_out, int advance,
                                  omnitok_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    OT_CHECK_ARG(lm, "lm_step: null engine");
    if (B == 0) return OMNITOK_OK;
    OT_CHECK_ARG((idx || emb) && pos && cache_len, "lm_step: null pointer");
    if (!lm->finalized) {
        set_error("lm_step: engine not finalised (load the weights first)");
        return OMNITOK_ERR_STATE;
    }
    if (lm->streams_format == OMNITOK_LM_SF_W16 && (lm->weight_format == OMNITOK_LM_W_FP32 || !lm->head.w16)) {
        set_error("lm_step: streams format OMNITOK_LM_SF_W16 (omnitok_lm_set_streams_format) needs the packed 16-bit weight images: set "
                  "omnitok_lm_set_weight_format to OMNITOK_LM_W_BF16 or OMNITOK_LM_W_FP16 (it is OMNITOK_LM_W_FP32), or the streams format "
                  "back to OMNITOK_LM_SF_FP32");
        return OMNITOK_ERR_STATE;
    }
    if (!lm->kv || B > lm->max_batch) {
        set_error("lm_step: cache not allocated for batch %d (omnitok_lm_alloc_cache)", B);
        return OMNITOK_ERR_STATE;
    }
    const omnitok_lm_config &c = lm->cfg;
    const int C = c.n_embd, hd = lm->head_dim();
    hipLaunchKernelGGL(lm_embed_kernel, dim3(B), dim3(256), 0, stream, idx, pos, LW(lm, "tok_emb.weight"),
                       LW(lm, "pos_emb"), emb, pos_extra, lm->x, C, c.vocab_size, c.block_size);
    OT_LAUNCH_CHECK("lm_embed");
    const LmMerge mg{lm->part, cache_len, c.n_head, hd, (lm->max_len + lm->chunk - 1) / lm->chunk, lm->chunk, lm->qkv};   // (qkv is free once the partials exist)
    LmAttnArgs at = {};
    at.qkv = lm->qkv; at.kvfmt = lm->cache_format; at.kq = lm->cache_quant; at.cache_len = cache_len;
    at.B = B; at.n_head = c.n_head; at.head_dim = hd; at.max_len = lm->max_len;
    at.part = lm->part; at.err_flag = lm->err_flag; at.chunk = lm->chunk;
    for (int i = 0; i < c.n_layer; ++i) {
        const LmLayer &L = lm->layers[i];
        at.kc = lm->k_slab(i); at.vc = lm->v_slab(i);
        at.ksc = lm->k_scales(i); at.vsc = lm->v_scales(i);
        // x + proj(attn(ln1(x)))   (reference gpt.py:159-161)
        if (int rc = lm_step_linear(lm, {lm->x, L.wqkv, L.bqkv, nullptr, L.ln1w, L.ln1b, lm->qkv, B, 3 * C, C, 0}, nullptr, stream)) return rc;
        if (int rc = lm_attn_partials(at, stream)) return rc;
        if (int rc = lm_step_linear(lm, {nullptr, L.wproj, L.bproj, lm->x, nullptr, nullptr, lm->x, B, C, C, 0}, &mg, stream)) return rc;
        // x + mlp(ln2(x))          (reference gpt.py:162, 150-155)
        if (int rc = lm_step_linear(lm, {lm->x, L.w1, L.b1, nullptr, L.ln2w, L.ln2b, lm->hid, B, 4 * C, C, 1}, nullptr, stream)) return rc;
        if (int rc = lm_step_linear(lm, {lm->hid, L.w2, L.b2, lm->x, nullptr, nullptr, lm->x, B, C, 4 * C, 0}, nullptr, stream)) return rc;
    }
    if (logits_out)  // ln_f + head (no bias), reference gpt.py:263-264
        if (int rc = lm_step_linear(lm, {lm->x, lm->head, nullptr, nullptr, LW(lm, "ln_f.weight"), LW(lm, "ln_f.bias"), logits_out, B,
                                         c.vocab_size, C, 0}, nullptr, stream))
            return rc;
    if (advance) {
        // one thread per stream: up to 128 of them also on this path ("lm_streams_min" above B sends any batch here)
        hipLaunchKernelGGL(lm_advance_kernel, dim3(1), dim3(128), 0, stream, pos, cache_len, B);
        OT_LAUNCH_CHECK("lm_advance");
    }
    return OMNITOK_OK;
}

extern "C" int omnitok_lm_prefill(omnitok_lm *lm, const int64_t *idx, int32_t *pos, int32_t *cache_len, int B, int T,
                                  float *logits_out, omnitok_stream_t stream_) {
    return omnitok_lm_prefill_ex(lm, idx, T, /*emb*/ nullptr, /*T_emb*/ 0, /*pos_extra*/ nullptr, pos, cache_len, B, logits_out, stream_);
}

// One batched prefill: the engine's four switches (prefill_format, prefill_attention, prefill_attention_operands, weight_format)
// resolved once per call by lm_prefill_plan, and the stages of a block, each of which picks its fp32 or 16-bit form.
// w16 (OMNITOK_LM_PF_W16): the five GEMMs run on the 16-bit MFMA over the packed weight images.  Their A operands are the fp32 prefill's
// values rounded once to the weight format: LayerNorm rows and the attention output by their own kernels' 16-bit form, FC1's GELU output
// in its GEMM's epilogue (no [M, 4C] fp32 tensor, no GELU pass).  xn / att / hid then hold packed 16-bit rows in the first half of their
// regions; x, qkv, the cache scatter and the attention partials stay fp32.  The attention modes: LmPrefill::attention.
struct LmPrefill {
    omnitok_lm *lm;
    hipStream_t stream;
    int B, T, nchunk;
    int64_t M;                                // rows: B * T, or those of a row block (rows())
    float *x, *xn, *att, *qkv, *hid, *part;   // workspace: x | xn | att [M, C], qkv [M, 3C], hid [M, 4C], partials (rows mode)
    bool w16, tiled;
    int wfmt, aop;  // w16: the weight format | 0; operands of the tiled attention: 0 (fp32), or OMNITOK_LM_W_BF16 | _FP16

    float *o32(float *p) const { return w16 ? nullptr : p; }  // a stage's output: exactly one of the two
    void *o16(float *p) const { return w16 ? p : nullptr; }
    // rows r0 .. r0 + n - 1 of x and xn (for ln and linear)
    LmPrefill rows(int64_t r0, int64_t n) const {
        LmPrefill v = *this;
        v.x += r0 * lm->cfg.n_embd; v.xn += r0 * lm->cfg.n_embd; v.M = n;
        return v;
    }
    // xn = nn.LayerNorm(x)
    int ln(const float *gamma, const float *beta) const {
        return lm_layernorm_rows(x, gamma, beta, o32(xn), o16(xn), wfmt, M, lm->cfg.n_embd, lm->err_flag, stream);
    }
    // nn.Linear: y [M, N] = act(a [M, K] . m [N, K]^T + bias) (+ residual [M, N], may be y); act 1 = exact GELU.  fp32: the fp32-MFMA GEMM
    // over dense rows and a GELU pass | w16: lm_gemm16, whose GELU output is packed 16-bit rows (FC1 into hid)
    int linear(const float *a, const LmMat &m, const float *bias, const float *residual, float *y, int N, int K, int act) const {
        if (w16) return lm_gemm16(a, m.w16, m.fmt, bias, residual, act ? nullptr : y, act ? y : nullptr, M, N, K, act, lm->err_flag, stream);
        omnitok_row_gemm g = {};
        g.a = a; g.lda = K; g.w = m.w32; g.ldw = K;
        g.bias = bias; g.residual = residual; g.ldr = N; g.c = y; g.ldc = N;
        g.M = M; g.N = N; g.K = K;
        g.flags = (bias ? OMNITOK_GEMM_BIAS : 0) | (residual ? OMNITOK_GEMM_RESIDUAL : 0);
        if (int rc = omnitok_gemm(&g, stream)) return rc;
        if (act) {
            hipLaunchKernelGGL(lm_gelu_kernel, dim3((unsigned)((M * N / 4 + 255) / 256)), dim3(256), 0, stream, y, M * N / 4);
            OT_LAUNCH_CHECK("lm_gelu");
        }
        return OMNITOK_OK;
    }
    int scatter(int layer) const {
        return lm_kv_scatter(qkv, lm->k_slab(layer), lm->v_slab(layer), lm->cache_format, lm->cache_quant, lm->k_scales(layer),
                             lm->v_scales(layer), M, T, lm->cfg.n_head, lm->head_dim(), lm->max_len, lm->err_flag, stream);
    }
    // att = causal attention of qkv.  rows (OMNITOK_LM_PA_ROWS): the decode kernel per query row over the cache just scattered, chunk
    // partials, a merge | tiled: straight from qkv, K/V tiles shared by 128 query rows on the fp32-input MFMA: no partials, no dependence on
    // the cache format; "same arithmetic as T decode steps" then holds to rounding, not to the bit | tiled with aop (refused without the
    // tiled mode): Q / K / V / P rounded once to that format on the bf16 / fp16 MFMA.  The scatter stays in every mode: the decode steps
    // after the prefill read the cache.
    int attention(int layer) const {
        const int n_head = lm->cfg.n_head, hd = lm->head_dim();
        if (tiled)
            return lm_attn_prefill_any(aop ? "lm_attn_prefill16" : "lm_attn_prefill", qkv, B, T, n_head, hd, aop, o32(att), o16(att), wfmt,
                                       lm->err_flag, stream);
        LmAttnArgs a = {};
        a.qkv = qkv; a.kc = lm->k_slab(layer); a.vc = lm->v_slab(layer); a.kvfmt = lm->cache_format;
        a.kq = lm->cache_quant; a.ksc = lm->k_scales(layer); a.vsc = lm->v_scales(layer);
        a.B = B; a.n_head = n_head; a.head_dim = hd; a.max_len = lm->max_len;
        a.part = part; a.prefill_T = T; a.chunk = LM_CHUNK;
        if (int rc = lm_attn_partials(a, stream)) return rc;
        lm_attn_merge(part, nullptr, n_head, hd, nchunk, T, o32(att), o16(att), wfmt, M, lm->err_flag, LM_CHUNK, stream);
        OT_LAUNCH_CHECK(w16 ? "lm_attn_merge16" : "lm_attn_merge");
        return OMNITOK_OK;
    }
};

// Checks the arguments and the engine's state for a prefill of B streams x T rows, grows the workspace and fills p.  B * T > 0.
static int lm_prefill_plan(omnitok_lm *lm, const int64_t *idx, int T_tok, const float *emb, int T_emb, int32_t *pos, int32_t *cache_len,
                           int B, hipStream_t stream, LmPrefill &p) {
    const int T = T_tok + T_emb;
    OT_CHECK_ARG((idx || T_tok == 0) && (emb || T_emb == 0) && pos && cache_len, "lm_prefill: null pointer");
    if (!lm->finalized) {
        set_error("lm_prefill: engine not finalised (load the weights first)");
        return OMNITOK_ERR_STATE;
    }
    if (lm->prefill_format == OMNITOK_LM_PF_W16 && (lm->weight_format == OMNITOK_LM_W_FP32 || !lm->head.w16)) {
        set_error("lm_prefill: prefill format OMNITOK_LM_PF_W16 (omnitok_lm_set_prefill_format) needs the packed 16-bit weight images: "
                  "set omnitok_lm_set_weight_format to OMNITOK_LM_W_BF16 or OMNITOK_LM_W_FP16 (it is OMNITOK_LM_W_FP32), or the prefill "
                  "format back to OMNITOK_LM_PF_FP32");
        return OMNITOK_ERR_STATE;
    }
    if (lm->prefill_attention_operands != OMNITOK_LM_AOP_FP32 && lm->prefill_attention != OMNITOK_LM_PA_TILED) {
        set_error("lm_prefill: 16-bit attention operands (omnitok_lm_set_prefill_attention_operands) need the tiled attention: set "
                  "omnitok_lm_set_prefill_attention to OMNITOK_LM_PA_TILED (it is OMNITOK_LM_PA_ROWS), or the operands back to "
                  "OMNITOK_LM_AOP_FP32");
        return OMNITOK_ERR_STATE;
    }
    if (!lm->kv || B > lm->max_batch || T > lm->max_len) {
        set_error("lm_prefill: cache not allocated for %d streams x %d tokens (omnitok_lm_alloc_cache)", B, T);
        return OMNITOK_ERR_STATE;
    }
    const omnitok_lm_config &c = lm->cfg;
    OT_CHECK_ARG(T <= c.block_size, "lm_prefill: %d tokens exceed block_size %d", T, c.block_size);
    const int64_t C = c.n_embd, M = (int64_t)B * T;
    OT_CHECK_ARG(M <= 65535, "lm_prefill: B * T = %lld rows (max 65535)", (long long)M);
    p.lm = lm; p.stream = stream; p.B = B; p.T = T; p.M = M;
    p.nchunk = (T + LM_CHUNK - 1) / LM_CHUNK;
    p.w16 = lm->prefill_format == OMNITOK_LM_PF_W16;
    p.wfmt = p.w16 ? lm->weight_format : 0;
    p.tiled = lm->prefill_attention == OMNITOK_LM_PA_TILED;
    p.aop = lm->prefill_attention_operands == OMNITOK_LM_AOP_BF16   ? OMNITOK_LM_W_BF16
            : lm->prefill_attention_operands == OMNITOK_LM_AOP_FP16 ? OMNITOK_LM_W_FP16
                                                                    : 0;
    const int64_t need = M * C * 3 + M * 3 * C + M * 4 * C + (p.tiled ? 0 : M * c.n_head * p.nchunk * (2 + lm->head_dim()));
    if (int rc = lm_grow(reinterpret_cast<void **>(&lm->pf), &lm->pf_bytes, need * 4)) return rc;
    p.x = lm->pf; p.xn = p.x + M * C; p.att = p.xn + M * C;
    p.qkv = p.att + M * C; p.hid = p.qkv + M * 3 * C; p.part = p.hid + M * 4 * C;
    return OMNITOK_OK;
}

// Embedding and the n_layer blocks of a batched prefill, shared by omnitok_lm_prefill_ex and omnitok_lm_prefill_loss: fills the K/V
// cache; p.x [M, C] is the residual stream after the last block, p.xn scratch for its ln_f.  B * T > 0.
static int lm_prefill_layers(omnitok_lm *lm, const int64_t *idx, int T_tok, const float *emb, int T_emb,
                             const float *pos_extra, int32_t *pos, int32_t *cache_len, int B, hipStream_t stream, LmPrefill &p) {
    if (int rc = lm_prefill_plan(lm, idx, T_tok, emb, T_emb, pos, cache_len, B, stream, p)) return rc;
    const int C = lm->cfg.n_embd;
    hipLaunchKernelGGL(lm_embed_seq_kernel, dim3((unsigned)p.M), dim3(256), 0, stream, idx, LW(lm, "tok_emb.weight"),
                       LW(lm, "pos_emb"), emb, T_emb, pos_extra, p.x, p.T, C, lm->cfg.vocab_size);
    OT_LAUNCH_CHECK("lm_embed_seq");
    for (int i = 0; i < lm->cfg.n_layer; ++i) {
        const LmLayer &L = lm->layers[i];
        // x + proj(attn(ln1(x)))   (reference gpt.py:159-161)
        if (int rc = p.ln(L.ln1w, L.ln1b)) return rc;
        if (int rc = p.linear(p.xn, L.wqkv, L.bqkv, nullptr, p.qkv, 3 * C, C, 0)) return rc;
        if (int rc = p.scatter(i)) return rc;
        if (int rc = p.attention(i)) return rc;
        if (int rc = p.linear(p.att, L.wproj, L.bproj, p.x, p.x, C, C, 0)) return rc;
        // x + mlp(ln2(x))          (reference gpt.py:162, 150-155)
        if (int rc = p.ln(L.ln2w, L.ln2b)) return rc;
        if (int rc = p.linear(p.xn, L.w1, L.b1, nullptr, p.hid, 4 * C, C, 1)) return rc;
        if (int rc = p.linear(p.hid, L.w2, L.b2, p.x, p.x, C, 4 * C, 0)) return rc;
    }
    return OMNITOK_OK;
}

// logits [p.M, V] = head(ln_f(p.x)), through p.xn
static int lm_head_rows(const LmPrefill &p, float *logits) {
    if (int rc = p.ln(LW(p.lm, "ln_f.weight"), LW(p.lm, "ln_f.bias"))) return rc;
    return p.linear(p.xn, p.lm->head, nullptr, nullptr, logits, p.lm->cfg.vocab_size, p.lm->cfg.n_embd, 0);
}

extern "C" int omnitok_lm_prefill_ex(omnitok_lm *lm, const int64_t *idx, int T_tok, const float *emb, int T_emb,
                                     const float *pos_extra, int32_t *pos, int32_t *cache_len, int B,
                                     float *logits_out, omnitok_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    OT_CHECK_ARG(lm, "lm_prefill: null engine");
    OT_CHECK_ARG(T_tok >= 0 && T_emb >= 0, "lm_prefill: negative length");
    const int T = T_tok + T_emb;
    if (B == 0 || T == 0) return OMNITOK_OK;
    LmPrefill pf;
    if (int rc = lm_prefill_layers(lm, idx, T_tok, emb, T_emb, pos_extra, pos, cache_len, B, stream, pf)) return rc;
    if (logits_out)
        if (int rc = lm_head_rows(pf, logits_out)) return rc;
    hipLaunchKernelGGL(lm_set_len_kernel, dim3(1), dim3(128), 0, stream, pos, cache_len, B, T);
    OT_LAUNCH_CHECK("lm_set_len");
    return OMNITOK_OK;
}

extern "C" int omnitok_lm_prefill_loss(omnitok_lm *lm, const int64_t *idx, int T_tok, const float *emb, int T_emb,
                                       const float *pos_extra, const int64_t *targets, int32_t *pos, int32_t *cache_len,
                                       int B, float *nll, int32_t *rank, double *sums, omnitok_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    OT_CHECK_ARG(lm, "lm_prefill_loss: null engine");
    OT_CHECK_ARG(T_tok >= 0 && T_emb >= 0 && B >= 0, "lm_prefill_loss: negative length");
    OT_CHECK_ARG(targets && sums, "lm_prefill_loss: null pointer (targets / sums)");
    OT_CHECK_ARG((reinterpret_cast<uintptr_t>(targets) & 7) == 0 && (reinterpret_cast<uintptr_t>(sums) & 7) == 0,
                 "lm_prefill_loss: targets / sums are not 8-byte aligned");
    const int T = T_tok + T_emb;
    OT_CHECK_ARG(B > 0 && T > 0, "lm_prefill_loss: no rows (B %d, T %d)", B, T);
    const int64_t M = (int64_t)B * T, V = lm->cfg.vocab_size;
    OT_CHECK_ARG(M <= 65535, "lm_prefill_loss: B * T = %lld rows (max 65535)", (long long)M);
    OT_CHECK_ARG(g_lm_loss_chunk_rows >= 1, "lm_prefill_loss: option lm_loss_chunk_rows = %d", g_lm_loss_chunk_rows);
    const int64_t R = std::min<int64_t>(g_lm_loss_chunk_rows, M);
    LmPrefill pf;
    if (int rc = lm_prefill_layers(lm, idx, T_tok, emb, T_emb, pos_extra, pos, cache_len, B, stream, pf)) return rc;
    // workspaces (grow-only)
    if (int rc = lm_grow(reinterpret_cast<void **>(&lm->lg), &lm->lg_bytes, R * V * 4)) return rc;
    const int64_t red_bytes = omnitok_lm_token_ce_workspace(M);
    if (lm->ce_rows < M) {
        const int64_t rows8 = (M + 1) & ~(int64_t)1;  // keeps the partials 8-byte aligned
        lm->ce_rows = 0;
        if (int rc = lm_grow(reinterpret_cast<void **>(&lm->ce), &lm->ce_bytes, rows8 * 8 + red_bytes)) return rc;
        lm->ce_rows = rows8;
    }
    float *nll_w = nll ? nll : lm->ce;
    int32_t *rank_w = rank ? rank : reinterpret_cast<int32_t *>(lm->ce + lm->ce_rows);
    void *red = lm->ce + 2 * lm->ce_rows;
    // which blocks have a row that counts
    std::vector<int64_t> tg((size_t)M);
    OT_HIP(hipMemcpyAsync(tg.data(), targets, (size_t)M * 8, hipMemcpyDeviceToHost, stream));
    OT_HIP(hipStreamSynchronize(stream));
    for (int64_t r0 = 0; r0 < M; r0 += R) {
        const int64_t rows = std::min(R, M - r0);
        bool any = false;
        for (int64_t i = r0; i < r0 + rows && !any; ++i) any = tg[(size_t)i] >= 0;
        if (any)
            if (int rc = lm_head_rows(pf.rows(r0, rows), lm->lg)) return rc;
        // an all-ignored block: the kernel writes nll 0 / rank -1 from the targets alone and reads no logits
        if (int rc = lm_token_ce_rows(lm->lg, V, targets + r0, rows, (int)V, nll_w + r0, rank_w + r0, stream)) return rc;
    }
    if (int rc = lm_token_ce_reduce(nll_w, rank_w, M, (int)V, sums, red, red_bytes, stream)) return rc;
    hipLaunchKernelGGL(lm_set_len_kernel, dim3(1), dim3(128), 0, stream, pos, cache_len, B, T);
    OT_LAUNCH_CHECK("lm_set_len");
    return OMNITOK_OK;
}

extern "C" int omnitok_lm_layernorm16(const float *x, const float *gamma, const float *beta, void *y16, int fmt, int64_t rows, int K,
                                      int *flag, omnitok_stream_t stream) {
    OT_CHECK_ARG(fmt == OMNITOK_LM_W_BF16 || fmt == OMNITOK_LM_W_FP16, "lm_layernorm16: fmt %d (OMNITOK_LM_W_BF16 | OMNITOK_LM_W_FP16)", fmt);
    OT_CHECK_ARG(x && gamma && beta && y16, "lm_layernorm16: null pointer");
    OT_CHECK_ARG(aligned16(x) && aligned16(gamma) && aligned16(beta) && aligned16(y16), "lm_layernorm16: unaligned pointer (16 bytes)");
    OT_CHECK_ARG(rows >= 1 && rows <= 0x7fffffffLL && K >= 32 && K % 32 == 0, "lm_layernorm16: rows %lld (1 .. 2^31 - 1), K %d (K %% 32 == 0)",
                 (long long)rows, K);
    return lm_layernorm_rows(x, gamma, beta, nullptr, y16, fmt, rows, K, flag, static_cast<hipStream_t>(stream));
}

extern "C" int64_t omnitok_lm_loss_workspace_bytes(omnitok_lm *lm) {
    return lm ? lm->lg_bytes + lm->ce_bytes : 0;
}
