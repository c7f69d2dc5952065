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
// Every GEMM is omnitok_gemm with OMNITOK_GEMM_BIAS.  Under a 16-bit linear format (omnitok_dit_set_linear_format, DitLinear in
// dit_scaffold.h) the four GEMMs of a block are omnitok_dit_gemm16 calls with gate_residual and GELU in their epilogues (dit_block).
// Under a 16-bit attention format (omnitok_dit_set_attention_format) the attention is omnitok_dit_attn16 (dit_spatial_attn).
#include "dit_scaffold.h"

using namespace omnitok;

struct omnitok_dit {
    omnitok_dit_config cfg;
    int N, gw, K, Cout, hd, y_rows;
    int64_t modN;
    DitSlots w;
    std::vector<DitBlock> blocks;
    float *w_patch = nullptr, *b_patch = nullptr, *pos = nullptr, *w_t0 = nullptr, *b_t0 = nullptr, *w_t2 = nullptr, *b_t2 = nullptr,
          *ytable = nullptr, *w_mod = nullptr, *b_mod = nullptr, *w_final = nullptr, *b_final = nullptr;
    DitLinear lin;  // omnitok_dit_set_linear_format
    int attn_fmt = OMNITOK_DIT_ATTN_FP32;  // omnitok_dit_set_attention_format
    DitTables tb;  // omnitok_dit_set_frequencies; no frequencies: the built-in chain
    void *work = nullptr;
    int64_t work_bytes = 0;
    bool finalized = false;
};

static int64_t dit_patch_out(const omnitok_dit *e) { return (int64_t)e->cfg.patch_size * e->cfg.patch_size * e->Cout; }

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
    DitSlots &w = e->w;
    w.add("pos_embed", {1, e->N, D}, &e->pos);
    w.add("x_embedder.proj.weight", {D, c.in_channels, p, p}, &e->w_patch);
    w.add("x_embedder.proj.bias", {D}, &e->b_patch);
    w.add("t_embedder.mlp.0.weight", {D, DIT_T_FREQ}, &e->w_t0);
    w.add("t_embedder.mlp.0.bias", {D}, &e->b_t0);
    w.add("t_embedder.mlp.2.weight", {D, D}, &e->w_t2);
    w.add("t_embedder.mlp.2.bias", {D}, &e->b_t2);
    w.add("y_embedder.embedding_table.weight", {e->y_rows, D}, &e->ytable);
    w.add_blocks(e->blocks, D, F, p * p * e->Cout, &e->w_mod, &e->b_mod, e->modN, &e->w_final, &e->b_final);
    *out = e;
    return OMNITOK_OK;
}

extern "C" void omnitok_dit_destroy(omnitok_dit *e) {
    if (!e) return;
    e->w.free_all();
    e->tb.free_all();
    e->lin.free_all();
    if (e->work) (void)hipFree(e->work);
    delete e;
}

extern "C" int omnitok_dit_set_weight(omnitok_dit *e, const char *name, const void *dev_ptr, const int64_t *shape, int ndim,
                                      omnitok_stream_t stream) {
    OT_CHECK_ARG(e && name && dev_ptr && shape && ndim >= 0, "dit_set_weight: null pointer");
    return e->w.set_weight("dit", name, dev_ptr, shape, ndim, static_cast<hipStream_t>(stream));
}

extern "C" int omnitok_dit_missing(omnitok_dit *e, char *buf, int cap) {
    OT_CHECK_ARG(e && (buf || cap == 0) && cap >= 0, "dit_missing: null pointer");
    return e->w.missing(buf, cap);
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
    OT_CHECK_ARG(e, "dit_set_frequencies: null pointer");
    if (int rc = e->tb.set_frequencies("dit", freqs, n)) return rc;
    e->finalized = false;
    return OMNITOK_OK;
}

extern "C" int omnitok_dit_finalize(omnitok_dit *e, omnitok_stream_t stream) {
    OT_CHECK_ARG(e, "dit_finalize: null engine");
    if (int rc = e->w.require_all("dit")) return rc;
    if (int rc = e->tb.finalize(static_cast<hipStream_t>(stream))) return rc;
    if (int rc = e->lin.finalize("dit", e->w, e->blocks, e->cfg.hidden, e->cfg.mlp_hidden, static_cast<hipStream_t>(stream))) return rc;
    e->finalized = true;
    return OMNITOK_OK;
}

extern "C" int64_t omnitok_dit_workspace_bytes(omnitok_dit *e, int B) {
    if (!e || B < 1 || (int64_t)B * e->N > (1ll << 24)) {
        set_error("dit_workspace_bytes: null engine or B %d (B * tokens <= 2^24)", B);
        return -1;
    }
    return dit_work_floats((int64_t)B * e->N, B, e->cfg.hidden, e->cfg.mlp_hidden, dit_patch_out(e), e->modN,
                           e->lin.fmt != OMNITOK_DIT_LIN_FP32) * 4;
}

extern "C" int omnitok_dit_set_linear_format(omnitok_dit *e, int fmt) {
    OT_CHECK_ARG(e, "dit_set_linear_format: null engine");
    if (int rc = e->lin.set("dit", fmt, e->cfg.hidden, e->cfg.mlp_hidden)) return rc;
    e->finalized = false;
    return OMNITOK_OK;
}

extern "C" int omnitok_dit_linear_format(omnitok_dit *e) {
    OT_CHECK_ARG(e, "dit_linear_format: null engine");
    return e->lin.fmt;
}

extern "C" int omnitok_dit_set_attention_format(omnitok_dit *e, int fmt) {
    OT_CHECK_ARG(e, "dit_set_attention_format: null engine");
    return dit_set_attention_format("dit", &e->attn_fmt, fmt);
}

extern "C" int omnitok_dit_attention_format(omnitok_dit *e) {
    OT_CHECK_ARG(e, "dit_attention_format: null engine");
    return e->attn_fmt;
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
    const int D = c.hidden, F = c.mlp_hidden, N = e->N, PC = (int)dit_patch_out(e);
    const int64_t M = (int64_t)B * N, modN = e->modN;
    const int fmt = e->lin.fmt;
    const bool lin16 = fmt != OMNITOK_DIT_LIN_FP32;
    const int afmt = e->attn_fmt;
    if (int rc = dit_grow(&e->work, &e->work_bytes, dit_work_floats(M, B, D, F, PC, modN, lin16) * 4)) return rc;
    const DitWork w(e->work, M, B, D, F, PC, lin16);
#define DIT_RUN(call) \
    if (int rc_ = (call)) return rc_
    DIT_RUN(omnitok_dit_patch_embed(x, cfg ? B / 2 : B, e->w_patch, e->b_patch, e->pos, B, c.in_channels, c.input_size, c.patch_size, D, w.X,
                                    stream));
    DIT_RUN(dit_conditioning(who, e->tb, e->w_t0, e->b_t0, e->w_t2, e->b_t2, e->ytable, e->y_rows, e->w_mod, e->b_mod, modN, t, y, B, D, w,
                             stream));
    for (int i = 0; i < c.depth; ++i)
        DIT_RUN(dit_block(e->blocks[i], w, w.mod + (int64_t)i * 6 * D, modN, M, N, D, F,
                          [&](const float *qkv, float *a32, unsigned short *a16) {
                              return dit_spatial_attn(qkv, B, N, c.heads, e->hd, afmt, fmt, a32, a16, e->tb.flag, stream);
                          },
                          afmt != OMNITOK_DIT_ATTN_FP32, fmt, e->tb.flag, stream));
    const float *mf = w.mod + (int64_t)c.depth * 6 * D;  // shift | scale
    DIT_RUN(omnitok_dit_ln_modulate(w.X, mf, mf + D, modN, M, N, D, w.Xn, stream));
    DIT_RUN(dit_linear(w.Xn, e->w_final, e->b_final, w.LIN, M, PC, D, stream));
    DIT_RUN(omnitok_dit_unpatchify(w.LIN, B, N, c.patch_size, e->Cout, out, stream));
    if (cfg) DIT_RUN(dit_cfg_blend(out, B, e->Cout, 3, (int64_t)c.input_size * c.input_size, cfg_scale, stream));
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

extern "C" int omnitok_dit_check(omnitok_dit *e, omnitok_stream_t stream) {
    OT_CHECK_ARG(e, "dit_check: null engine");
    return e->tb.check("dit", static_cast<hipStream_t>(stream));
}
