// DiT denoiser: struct omnitok_dit and its exported functions (index: dit_common.h).
//
// One forward of B samples (M = B N token rows, D = hidden):
//   patch_embed + pos_embed                                         -> X [M, D]
//   table[t] -> Linear -> SiLU -> Linear, + label row, SiLU          -> c [B, D]     (c is silu(t_emb + y_emb): every adaLN_modulation starts
//                                                                                     with the same SiLU, models.py:113-116, 133-136)
//   ONE GEMM over the concatenated adaLN_modulation.1 weights        -> mod [B, depth * 6 D + 2 D]
//   per block: ln_modulate -> qkv GEMM -> attention -> proj GEMM -> gate_residual -> ln_modulate -> fc1 GEMM -> GELU-tanh -> fc2 GEMM
//              -> gate_residual
//   ln_modulate -> final linear -> unpatchify                       -> out [B, Cout, H, W]
// Every GEMM is omnitok_gemm with OMNITOK_GEMM_BIAS.
#include "dit_common.h"

#include <cmath>
#include <map>
#include <string>
#include <vector>

using namespace omnitok;

namespace {

struct DitSlot {
    std::vector<int64_t> shape;
    float **dst;        // where the engine keeps the tensor ...
    int64_t offset;     // ... at this float offset (the adaLN tensors lie inside the concatenated modulation weight / bias)
    int64_t alloc;      // floats to allocate when *dst is null (the whole concatenated buffer for an adaLN tensor)
    bool set = false;
};

struct DitBlock {
    float *wqkv = nullptr, *bqkv = nullptr, *wproj = nullptr, *bproj = nullptr, *wfc1 = nullptr, *bfc1 = nullptr, *wfc2 = nullptr,
          *bfc2 = nullptr;
};

}  // namespace

struct omnitok_dit {
    omnitok_dit_config cfg;
    int N, gw, K, Cout, hd, y_rows;
    int64_t modN;
    std::map<std::string, DitSlot> slots;
    std::vector<std::string> order;  // the state_dict's order, for omnitok_dit_missing
    std::vector<DitBlock> blocks;
    float *w_patch = nullptr, *b_patch = nullptr, *pos = nullptr, *w_t0 = nullptr, *b_t0 = nullptr, *w_t2 = nullptr, *b_t2 = nullptr,
          *ytable = nullptr, *w_mod = nullptr, *b_mod = nullptr, *w_final = nullptr, *b_final = nullptr;
    float *t_table = nullptr;
    std::vector<float> freqs;  // omnitok_dit_set_frequencies; empty: the built-in chain
    bool table_built = false;
    int *flag = nullptr;
    void *work = nullptr;
    int64_t work_bytes = 0;
    bool finalized = false;
};

// floats of the final linear's output, rounded up to whole f32x4 (what follows it in the workspace stays 16-byte aligned)
static int64_t dit_lin_floats(const omnitok_dit *e, int64_t M) {
    return (M * (int64_t)e->cfg.patch_size * e->cfg.patch_size * e->Cout + 3) / 4 * 4;
}

static int64_t dit_work_floats(const omnitok_dit *e, int B) {
    const int64_t M = (int64_t)B * e->N, D = e->cfg.hidden;
    // X, Xn, Y, A | qkv | fc1 | final linear | temb, h1, h2, c | mod
    return 4 * M * D + 3 * M * D + M * e->cfg.mlp_hidden + dit_lin_floats(e, M) +
           (int64_t)B * (DIT_T_FREQ + 3 * D) + (int64_t)B * e->modN;
}

extern "C" int omnitok_dit_create(const omnitok_dit_config *cfg, omnitok_dit **out) {
    OT_CHECK_ARG(cfg && out, "dit_create: null pointer");
    const omnitok_dit_config &c = *cfg;
    OT_CHECK_ARG(c.input_size > 0 && c.patch_size > 0 && c.in_channels > 0 && c.hidden > 0 && c.depth > 0 && c.heads > 0 &&
                     c.mlp_hidden > 0 && c.num_classes > 0,
                 "dit_create: every size must be positive");
    OT_CHECK_ARG(c.class_dropout >= 0.0f && c.class_dropout <= 1.0f, "dit_create: class_dropout %g outside [0, 1]", (double)c.class_dropout);
    OT_CHECK_ARG(c.input_size % c.patch_size == 0, "dit_create: input_size %d is not a multiple of patch_size %d", c.input_size,
                 c.patch_size);
    OT_CHECK_ARG(c.hidden % c.heads == 0 && (c.hidden / c.heads == 64 || c.hidden / c.heads == 72),
                 "dit_create: hidden %d / heads %d: head_dim must be 64 or 72", c.hidden, c.heads);
    OT_CHECK_ARG(c.hidden % 32 == 0 && c.mlp_hidden % 32 == 0, "dit_create: hidden %d and mlp_hidden %d must be multiples of 32", c.hidden,
                 c.mlp_hidden);
    OT_CHECK_ARG((int64_t)c.patch_size * c.patch_size * c.in_channels <= 512, "dit_create: patch_size^2 * in_channels = %lld (<= 512)",
                 (long long)c.patch_size * c.patch_size * c.in_channels);
    OT_CHECK_ARG(c.heads <= 1024 && c.depth <= 4096 && c.input_size <= 4096, "dit_create: heads %d (<= 1024), depth %d (<= 4096), input_size %d (<= 4096)",
                 c.heads, c.depth, c.input_size);
    omnitok_dit *e = new omnitok_dit();
    e->cfg = c;
    e->gw = c.input_size / c.patch_size;
    e->N = e->gw * e->gw;
    e->K = c.patch_size * c.patch_size * c.in_channels;
    e->Cout = c.learn_sigma ? 2 * c.in_channels : c.in_channels;
    e->hd = c.hidden / c.heads;
    e->y_rows = c.num_classes + (c.class_dropout > 0.0f ? 1 : 0);
    const int64_t D = c.hidden, F = c.mlp_hidden, p = c.patch_size;
    e->modN = (int64_t)c.depth * 6 * D + 2 * D;
    e->blocks.resize(c.depth);
    auto add = [&](const std::string &name, std::vector<int64_t> shape, float **dst, int64_t offset = 0, int64_t alloc = 0) {
        int64_t n = 1;
        for (auto s : shape) n *= s;
        e->slots[name] = DitSlot{std::move(shape), dst, offset, alloc ? alloc : n};
        e->order.push_back(name);
    };
    add("pos_embed", {1, e->N, D}, &e->pos);
    add("x_embedder.proj.weight", {D, c.in_channels, p, p}, &e->w_patch);
    add("x_embedder.proj.bias", {D}, &e->b_patch);
    add("t_embedder.mlp.0.weight", {D, DIT_T_FREQ}, &e->w_t0);
    add("t_embedder.mlp.0.bias", {D}, &e->b_t0);
    add("t_embedder.mlp.2.weight", {D, D}, &e->w_t2);
    add("t_embedder.mlp.2.bias", {D}, &e->b_t2);
    add("y_embedder.embedding_table.weight", {e->y_rows, D}, &e->ytable);
    for (int i = 0; i < c.depth; ++i) {
        const std::string b = "blocks." + std::to_string(i);
        DitBlock &L = e->blocks[i];
        add(b + ".attn.qkv.weight", {3 * D, D}, &L.wqkv);
        add(b + ".attn.qkv.bias", {3 * D}, &L.bqkv);
        add(b + ".attn.proj.weight", {D, D}, &L.wproj);
        add(b + ".attn.proj.bias", {D}, &L.bproj);
        add(b + ".mlp.fc1.weight", {F, D}, &L.wfc1);
        add(b + ".mlp.fc1.bias", {F}, &L.bfc1);
        add(b + ".mlp.fc2.weight", {D, F}, &L.wfc2);
        add(b + ".mlp.fc2.bias", {D}, &L.bfc2);
        add(b + ".adaLN_modulation.1.weight", {6 * D, D}, &e->w_mod, (int64_t)i * 6 * D * D, e->modN * D);
        add(b + ".adaLN_modulation.1.bias", {6 * D}, &e->b_mod, (int64_t)i * 6 * D, e->modN);
    }
    add("final_layer.linear.weight", {p * p * e->Cout, D}, &e->w_final);
    add("final_layer.linear.bias", {p * p * e->Cout}, &e->b_final);
    add("final_layer.adaLN_modulation.1.weight", {2 * D, D}, &e->w_mod, (int64_t)c.depth * 6 * D * D, e->modN * D);
    add("final_layer.adaLN_modulation.1.bias", {2 * D}, &e->b_mod, (int64_t)c.depth * 6 * D, e->modN);
    *out = e;
    return OMNITOK_OK;
}

extern "C" void omnitok_dit_destroy(omnitok_dit *e) {
    if (!e) return;
    for (auto &kv : e->slots)
        if (*kv.second.dst) {
            (void)hipFree(*kv.second.dst);
            *kv.second.dst = nullptr;  // (the adaLN slots share two buffers)
        }
    if (e->t_table) (void)hipFree(e->t_table);
    if (e->flag) (void)hipFree(e->flag);
    if (e->work) (void)hipFree(e->work);
    delete e;
}

extern "C" int omnitok_dit_set_weight(omnitok_dit *e, const char *name, const void *dev_ptr, const int64_t *shape, int ndim,
                                      omnitok_stream_t stream) {
    OT_CHECK_ARG(e && name && dev_ptr && shape && ndim >= 0, "dit_set_weight: null pointer");
    auto it = e->slots.find(name);
    if (it == e->slots.end()) return 1;
    DitSlot &s = it->second;
    const std::vector<int64_t> shp(shape, shape + ndim);
    if (shp != s.shape) {
        std::string want, got;
        for (auto v : s.shape) want += std::to_string(v) + ",";
        for (auto v : shp) got += std::to_string(v) + ",";
        set_error("dit_set_weight: size mismatch for %s: expected [%s] got [%s]", name, want.c_str(), got.c_str());
        return OMNITOK_ERR_INVALID;
    }
    int64_t n = 1;
    for (auto v : shp) n *= v;
    if (!*s.dst) OT_HIP(hipMalloc(reinterpret_cast<void **>(s.dst), (size_t)s.alloc * 4));
    OT_HIP(hipMemcpyAsync(*s.dst + s.offset, dev_ptr, (size_t)n * 4, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
    s.set = true;
    return OMNITOK_OK;
}

extern "C" int omnitok_dit_missing(omnitok_dit *e, char *buf, int cap) {
    OT_CHECK_ARG(e && (buf || cap == 0) && cap >= 0, "dit_missing: null pointer");
    int count = 0;
    size_t used = 0;
    if (cap > 0) buf[0] = 0;
    for (const std::string &name : e->order) {
        if (e->slots[name].set) continue;
        ++count;
        if (used + name.size() + 2 <= (size_t)cap) {
            if (used) buf[used++] = '\n';
            used += name.copy(buf + used, name.size());
            buf[used] = 0;
        }
    }
    return count;
}

// models.py:52-56 for t = 0 .. 999.  freqs = exp(-log(10000) * arange(128, fp32) / 128) and args = float(t) * freqs are fp32 values there.
// freqs == nullptr: the argument of exp is rebuilt with the reference's two fp32 roundings and exp is rounded correctly; an fp32 exp
// of another library may differ from that in the last bit (torch's CPU exp does in 3 of the 128), which is 3e-5 in a feature of
// t = 999 -- hence the caller may pass the frequencies its own reference run would use (omnitok_dit_set_frequencies).
// cos / sin of an argument up to 999 are taken in fp64 and rounded once.
extern "C" int omnitok_dit_timestep_table(const float *freqs, float *table) {
    OT_CHECK_ARG(table, "dit_timestep_table: null pointer");
    constexpr int half = DIT_T_FREQ / 2;
    const float neg_log = (float)(-log(10000.0));
    for (int i = 0; i < half; ++i) {
        float freq;
        if (freqs) {
            freq = freqs[i];
        } else {
            const volatile float prod = neg_log * (float)i;
            const volatile float arg = prod / (float)half;
            freq = (float)exp((double)arg);
        }
        for (int t = 0; t < DIT_T_STEPS; ++t) {
            const volatile float a = (float)t * freq;
            table[t * DIT_T_FREQ + i] = (float)cos((double)a);
            table[t * DIT_T_FREQ + half + i] = (float)sin((double)a);
        }
    }
    return OMNITOK_OK;
}

extern "C" int omnitok_dit_set_frequencies(omnitok_dit *e, const float *freqs, int n) {
    OT_CHECK_ARG(e && freqs, "dit_set_frequencies: null pointer");
    OT_CHECK_ARG(n == DIT_T_FREQ / 2, "dit_set_frequencies: n %d (the model has %d frequencies)", n, DIT_T_FREQ / 2);
    for (int i = 0; i < n; ++i) OT_CHECK_ARG(std::isfinite(freqs[i]), "dit_set_frequencies: frequency %d is not finite", i);
    e->freqs.assign(freqs, freqs + n);
    e->table_built = false;
    e->finalized = false;
    return OMNITOK_OK;
}

extern "C" int omnitok_dit_finalize(omnitok_dit *e, omnitok_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    OT_CHECK_ARG(e, "dit_finalize: null engine");
    for (const std::string &name : e->order)
        if (!e->slots[name].set) {
            set_error("dit_finalize: missing weight %s", name.c_str());
            return OMNITOK_ERR_STATE;
        }
    if (!e->table_built) {
        std::vector<float> host((size_t)DIT_T_STEPS * DIT_T_FREQ);
        if (int rc = omnitok_dit_timestep_table(e->freqs.empty() ? nullptr : e->freqs.data(), host.data())) return rc;
        if (!e->t_table) OT_HIP(hipMalloc(reinterpret_cast<void **>(&e->t_table), host.size() * 4));
        OT_HIP(hipStreamSynchronize(stream));  // no earlier forward still reads the table
        OT_HIP(hipMemcpy(e->t_table, host.data(), host.size() * 4, hipMemcpyHostToDevice));
        e->table_built = true;
    }
    if (!e->flag) {
        OT_HIP(hipMalloc(reinterpret_cast<void **>(&e->flag), 4));
        if (int rc = device_fill_u32(e->flag, 0, 1, stream)) return rc;
    }
    e->finalized = true;
    return OMNITOK_OK;
}

extern "C" int64_t omnitok_dit_workspace_bytes(omnitok_dit *e, int B) {
    if (!e || B < 1 || (int64_t)B * e->N > (1ll << 24)) {
        set_error("dit_workspace_bytes: null engine or B %d (B * tokens <= 2^24)", B);
        return -1;
    }
    return dit_work_floats(e, B) * 4;
}

// grow-only device workspace
static int dit_grow(void **p, int64_t *have, int64_t need_bytes) {
    if (*have >= need_bytes) return OMNITOK_OK;
    if (*p) OT_HIP(hipFree(*p));  // (synchronises: no earlier call still uses it)
    *p = nullptr;
    *have = 0;
    OT_HIP(hipMalloc(p, (size_t)need_bytes));
    *have = need_bytes;
    return OMNITOK_OK;
}

static int dit_linear(const float *a, const float *w, const float *bias, float *c, int64_t M, int N, int K, hipStream_t stream) {
    omnitok_row_gemm g{};
    g.a = a; g.lda = K; g.w = w; g.ldw = K; g.bias = bias; g.c = c; g.ldc = N;
    g.M = M; g.N = N; g.K = K; g.flags = OMNITOK_GEMM_BIAS;
    return omnitok_gemm(&g, stream);
}

static int dit_forward_any(const char *who, omnitok_dit *e, const float *x, const int64_t *t, const int64_t *y, int B, bool cfg,
                           float cfg_scale, float *out, hipStream_t stream) {
    OT_CHECK_ARG(e && x && t && y && out, "%s: null pointer", who);
    OT_CHECK_ARG(aligned16(x) && aligned16(out), "%s: unaligned pointer (16 bytes)", who);
    OT_CHECK_ARG(B >= 1 && (int64_t)B * e->N <= (1ll << 24), "%s: B %d (>= 1, B * tokens <= 2^24)", who, B);
    OT_CHECK_ARG(!cfg || B % 2 == 0, "%s: B %d must be even (the conditional and the unconditional half)", who, B);
    OT_CHECK_ARG(!cfg || std::isfinite(cfg_scale), "%s: cfg_scale is not finite", who);
    if (!e->finalized) {
        set_error("%s: engine not finalized", who);
        return OMNITOK_ERR_STATE;
    }
    const omnitok_dit_config &c = e->cfg;
    const int D = c.hidden, F = c.mlp_hidden, N = e->N, PC = c.patch_size * c.patch_size * e->Cout;
    const int64_t M = (int64_t)B * N, modN = e->modN;
    if (int rc = dit_grow(&e->work, &e->work_bytes, dit_work_floats(e, B) * 4)) return rc;
    float *X = static_cast<float *>(e->work), *Xn = X + M * D, *Y = Xn + M * D, *A = Y + M * D, *QKV = A + M * D, *H1 = QKV + 3 * M * D,
          *LIN = H1 + M * F, *temb = LIN + dit_lin_floats(e, M), *h1 = temb + (int64_t)B * DIT_T_FREQ, *h2 = h1 + (int64_t)B * D, *cs = h2 + (int64_t)B * D,
          *mod = cs + (int64_t)B * D;
#define DIT_RUN(call) \
    if (int rc_ = (call)) return rc_
    DIT_RUN(omnitok_dit_patch_embed(x, cfg ? B / 2 : B, e->w_patch, e->b_patch, e->pos, B, c.in_channels, c.input_size, c.patch_size, D, X,
                                    stream));
    DIT_RUN(dit_cond_gather(e->t_table, t, B, temb, e->flag, stream));
    DIT_RUN(dit_linear(temb, e->w_t0, e->b_t0, h1, B, D, DIT_T_FREQ, stream));
    DIT_RUN(dit_silu(h1, (int64_t)B * D, stream));
    DIT_RUN(dit_linear(h1, e->w_t2, e->b_t2, h2, B, D, D, stream));
    DIT_RUN(dit_cond_combine(h2, e->ytable, e->y_rows, y, B, D, cs, e->flag, stream));
    OT_CHECK_ARG(modN < (1ll << 31), "%s: depth * 6 * hidden + 2 * hidden = %lld does not fit the GEMM's N", who, (long long)modN);
    DIT_RUN(dit_linear(cs, e->w_mod, e->b_mod, mod, B, (int)modN, D, stream));
    for (int i = 0; i < c.depth; ++i) {
        const DitBlock &L = e->blocks[i];
        const float *m = mod + (int64_t)i * 6 * D;  // shift_msa | scale_msa | gate_msa | shift_mlp | scale_mlp | gate_mlp
        DIT_RUN(omnitok_dit_ln_modulate(X, m, m + D, modN, M, N, D, Xn, stream));
        DIT_RUN(dit_linear(Xn, L.wqkv, L.bqkv, QKV, M, 3 * D, D, stream));
        DIT_RUN(omnitok_dit_attn(QKV, B, N, c.heads, e->hd, A, stream));
        DIT_RUN(dit_linear(A, L.wproj, L.bproj, Y, M, D, D, stream));
        DIT_RUN(omnitok_dit_gate_residual(X, Y, m + 2 * D, modN, M, N, D, stream));
        DIT_RUN(omnitok_dit_ln_modulate(X, m + 3 * D, m + 4 * D, modN, M, N, D, Xn, stream));
        DIT_RUN(dit_linear(Xn, L.wfc1, L.bfc1, H1, M, F, D, stream));
        DIT_RUN(omnitok_dit_gelu_tanh(H1, M * F, stream));
        DIT_RUN(dit_linear(H1, L.wfc2, L.bfc2, Y, M, D, F, stream));
        DIT_RUN(omnitok_dit_gate_residual(X, Y, m + 5 * D, modN, M, N, D, stream));
    }
    const float *mf = mod + (int64_t)c.depth * 6 * D;  // shift | scale
    DIT_RUN(omnitok_dit_ln_modulate(X, mf, mf + D, modN, M, N, D, Xn, stream));
    DIT_RUN(dit_linear(Xn, e->w_final, e->b_final, LIN, M, PC, D, stream));
    DIT_RUN(omnitok_dit_unpatchify(LIN, B, N, c.patch_size, e->Cout, out, stream));
    if (cfg) DIT_RUN(dit_cfg_blend(out, B, e->Cout, (int64_t)c.input_size * c.input_size, cfg_scale, stream));
#undef DIT_RUN
    return OMNITOK_OK;
}

extern "C" int omnitok_dit_forward(omnitok_dit *e, const float *x, const int64_t *t, const int64_t *y, int B, float *out,
                                   omnitok_stream_t stream) {
    return dit_forward_any("dit_forward", e, x, t, y, B, false, 1.0f, out, static_cast<hipStream_t>(stream));
}

extern "C" int omnitok_dit_forward_cfg(omnitok_dit *e, const float *x, const int64_t *t, const int64_t *y, int B, float cfg_scale,
                                       float *out, omnitok_stream_t stream) {
    return dit_forward_any("dit_forward_cfg", e, x, t, y, B, true, cfg_scale, out, static_cast<hipStream_t>(stream));
}

extern "C" int omnitok_dit_check(omnitok_dit *e, omnitok_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    OT_CHECK_ARG(e, "dit_check: null engine");
    if (!e->flag) return OMNITOK_OK;  // nothing ran yet
    int bits = 0;
    OT_HIP(hipMemcpyAsync(&bits, e->flag, 4, hipMemcpyDeviceToHost, stream));
    OT_HIP(hipStreamSynchronize(stream));
    if (!bits) return OMNITOK_OK;
    if (int rc = device_fill_u32(e->flag, 0, 1, stream)) return rc;
    set_error("dit_forward: %s%s%s", bits & DIT_FLAG_T_RANGE ? "a timestep outside [0, 1000)" : "",
              (bits & DIT_FLAG_T_RANGE) && (bits & DIT_FLAG_Y_RANGE) ? " and " : "",
              bits & DIT_FLAG_Y_RANGE ? "a label outside the embedding table" : "");
    return OMNITOK_ERR_INVALID;
}
