// Latte denoiser: struct omnitok_latte and its exported functions (index: latte_common.h).
//
// One forward of B samples of F frames (M = B F N token rows in (b f) n order, D = hidden; latte.py:319-382):
//   patch_embed + pos_embed over the B F frames                        -> X [M, D]
//   table[t] -> Linear -> SiLU -> Linear, (+ label row, extras == 2), SiLU -> c [B, D]   (the reference repeats c per frame for the
//                                                                        spatial blocks and per position for the temporal ones: the
//                                                                        same row of c for every row of sample b, so n_tokens = F N)
//   ONE GEMM over the concatenated adaLN_modulation.1 weights          -> mod [B, depth * 6 D + 2 D]
//   per pair: the DiT block with omnitok_dit_attn (omnitok_dit_attn16 under a 16-bit attention format) over B F sequences of N tokens; after the FIRST pair's spatial block the temp_embed
//             add; the DiT block with omnitok_latte_attn_temporal over the B N positions' F frames.  Nothing is rearranged.
//   ln_modulate -> final linear -> unpatchify of B F images             -> out [B, F, Cout, H, W]
// forward_cfg (latte.py:384-403): patch_embed reads the first B / 2 samples twice; the blend guides channels [0, 4) of every frame.
#include "dit_scaffold.h"
#include "latte_common.h"

using namespace omnitok;

struct omnitok_latte {
    omnitok_latte_config cfg;
    int N, Cout, hd, y_rows;
    int64_t modN;
    DitSlots w;
    std::vector<DitBlock> blocks;
    float *w_patch = nullptr, *b_patch = nullptr, *pos = nullptr, *temp = nullptr, *w_t0 = nullptr, *b_t0 = nullptr, *w_t2 = nullptr,
          *b_t2 = nullptr, *ytable = nullptr, *w_mod = nullptr, *b_mod = nullptr, *w_final = nullptr, *b_final = nullptr;
    DitLinear lin;  // omnitok_latte_set_linear_format
    int attn_fmt = OMNITOK_DIT_ATTN_FP32;  // omnitok_latte_set_attention_format: the spatial blocks' attention
    DitTables tb;
    void *work = nullptr;
    int64_t work_bytes = 0;
    bool finalized = false;
};

static int64_t latte_patch_out(const omnitok_latte *e) { return (int64_t)e->cfg.patch_size * e->cfg.patch_size * e->Cout; }
static int64_t latte_rows(const omnitok_latte *e, int B) { return (int64_t)B * e->cfg.num_frames * e->N; }

extern "C" int omnitok_latte_create(const omnitok_latte_config *cfg, omnitok_latte **out) {
    OT_CHECK_ARG(cfg && out, "latte_create: null pointer");
    const omnitok_latte_config &c = *cfg;
    OT_CHECK_ARG(c.extras != 78, "latte_create: extras 78 (the text-embedding model, latte.py:243-247) is not built");
    OT_CHECK_ARG(c.extras == 1 || c.extras == 2, "latte_create: extras %d (1: unconditional, 2: class labels)", c.extras);
    OT_CHECK_ARG(c.input_size > 0 && c.patch_size > 0 && c.in_channels > 0 && c.hidden > 0 && c.depth > 0 && c.heads > 0 &&
                     c.mlp_hidden > 0 && (c.extras == 1 || c.num_classes > 0),
                 "latte_create: every size must be positive");
    OT_CHECK_ARG(c.depth % 2 == 0, "latte_create: depth %d must be even (the blocks run in spatial / temporal pairs)", c.depth);
    OT_CHECK_ARG(c.num_frames >= 1 && c.num_frames <= LATTE_F_MAX, "latte_create: num_frames %d (1 .. %d)", c.num_frames, LATTE_F_MAX);
    OT_CHECK_ARG(c.class_dropout >= 0.0f && c.class_dropout <= 1.0f, "latte_create: class_dropout %g outside [0, 1]",
                 (double)c.class_dropout);
    OT_CHECK_ARG(c.input_size % c.patch_size == 0, "latte_create: input_size %d is not a multiple of patch_size %d", c.input_size,
                 c.patch_size);
    OT_CHECK_ARG(c.hidden % c.heads == 0 && (c.hidden / c.heads == 64 || c.hidden / c.heads == 72),
                 "latte_create: hidden %d / heads %d: head_dim must be 64 or 72", c.hidden, c.heads);
    OT_CHECK_ARG(c.hidden % 32 == 0 && c.mlp_hidden % 32 == 0, "latte_create: hidden %d and mlp_hidden %d must be multiples of 32", c.hidden,
                 c.mlp_hidden);
    OT_CHECK_ARG((int64_t)c.patch_size * c.patch_size * c.in_channels <= 512, "latte_create: patch_size^2 * in_channels = %lld (<= 512)",
                 (long long)c.patch_size * c.patch_size * c.in_channels);
    OT_CHECK_ARG(c.heads <= 1024 && c.depth <= 4096 && c.input_size <= 4096,
                 "latte_create: heads %d (<= 1024), depth %d (<= 4096), input_size %d (<= 4096)", c.heads, c.depth, c.input_size);
    omnitok_latte *e = new omnitok_latte();
    e->cfg = c;
    const int gw = c.input_size / c.patch_size;
    e->N = gw * gw;
    e->Cout = c.learn_sigma ? 2 * c.in_channels : c.in_channels;
    e->hd = c.hidden / c.heads;
    e->y_rows = c.extras == 2 ? c.num_classes + (c.class_dropout > 0.0f ? 1 : 0) : 0;
    const int64_t D = c.hidden, F = c.mlp_hidden, p = c.patch_size;
    e->modN = (int64_t)c.depth * 6 * D + 2 * D;
    e->blocks.resize(c.depth);
    DitSlots &w = e->w;  // latte.py's state_dict order
    w.add("pos_embed", {1, e->N, D}, &e->pos);
    w.add("temp_embed", {1, c.num_frames, D}, &e->temp);
    w.add("x_embedder.proj.weight", {D, c.in_channels, p, p}, &e->w_patch);
    w.add("x_embedder.proj.bias", {D}, &e->b_patch);
    w.add("t_embedder.mlp.0.weight", {D, DIT_T_FREQ}, &e->w_t0);
    w.add("t_embedder.mlp.0.bias", {D}, &e->b_t0);
    w.add("t_embedder.mlp.2.weight", {D, D}, &e->w_t2);
    w.add("t_embedder.mlp.2.bias", {D}, &e->b_t2);
    if (c.extras == 2) w.add("y_embedder.embedding_table.weight", {e->y_rows, D}, &e->ytable);
    w.add_blocks(e->blocks, D, F, p * p * e->Cout, &e->w_mod, &e->b_mod, e->modN, &e->w_final, &e->b_final);
    *out = e;
    return OMNITOK_OK;
}

extern "C" void omnitok_latte_destroy(omnitok_latte *e) {
    if (!e) return;
    e->w.free_all();
    e->tb.free_all();
    e->lin.free_all();
    if (e->work) (void)hipFree(e->work);
    delete e;
}

extern "C" int omnitok_latte_set_weight(omnitok_latte *e, const char *name, const void *dev_ptr, const int64_t *shape, int ndim,
                                        omnitok_stream_t stream) {
    OT_CHECK_ARG(e && name && dev_ptr && shape && ndim >= 0, "latte_set_weight: null pointer");
    return e->w.set_weight("latte", name, dev_ptr, shape, ndim, static_cast<hipStream_t>(stream));
}

extern "C" int omnitok_latte_missing(omnitok_latte *e, char *buf, int cap) {
    OT_CHECK_ARG(e && (buf || cap == 0) && cap >= 0, "latte_missing: null pointer");
    return e->w.missing(buf, cap);
}

extern "C" int omnitok_latte_set_frequencies(omnitok_latte *e, const float *freqs, int n) {
    OT_CHECK_ARG(e, "latte_set_frequencies: null pointer");
    if (int rc = e->tb.set_frequencies("latte", freqs, n)) return rc;
    e->finalized = false;
    return OMNITOK_OK;
}

extern "C" int omnitok_latte_finalize(omnitok_latte *e, omnitok_stream_t stream) {
    OT_CHECK_ARG(e, "latte_finalize: null engine");
    if (int rc = e->w.require_all("latte")) return rc;
    if (int rc = e->tb.finalize(static_cast<hipStream_t>(stream))) return rc;
    if (int rc = e->lin.finalize("latte", e->w, e->blocks, e->cfg.hidden, e->cfg.mlp_hidden, static_cast<hipStream_t>(stream))) return rc;
    e->finalized = true;
    return OMNITOK_OK;
}

extern "C" int64_t omnitok_latte_workspace_bytes(omnitok_latte *e, int B) {
    if (!e || B < 1 || latte_rows(e, B) > (1ll << 24)) {
        set_error("latte_workspace_bytes: null engine or B %d (B * frames * tokens <= 2^24)", B);
        return -1;
    }
    return dit_work_floats(latte_rows(e, B), B, e->cfg.hidden, e->cfg.mlp_hidden, latte_patch_out(e), e->modN,
                           e->lin.fmt != OMNITOK_DIT_LIN_FP32) * 4;
}

extern "C" int omnitok_latte_set_linear_format(omnitok_latte *e, int fmt) {
    OT_CHECK_ARG(e, "latte_set_linear_format: null engine");
    if (int rc = e->lin.set("latte", fmt, e->cfg.hidden, e->cfg.mlp_hidden)) return rc;
    e->finalized = false;
    return OMNITOK_OK;
}

extern "C" int omnitok_latte_linear_format(omnitok_latte *e) {
    OT_CHECK_ARG(e, "latte_linear_format: null engine");
    return e->lin.fmt;
}

extern "C" int omnitok_latte_set_attention_format(omnitok_latte *e, int fmt) {
    OT_CHECK_ARG(e, "latte_set_attention_format: null engine");
    return dit_set_attention_format("latte", &e->attn_fmt, fmt);
}

extern "C" int omnitok_latte_attention_format(omnitok_latte *e) {
    OT_CHECK_ARG(e, "latte_attention_format: null engine");
    return e->attn_fmt;
}

static int latte_forward_any(const char *who, omnitok_latte *e, const float *x, const int64_t *t, const int64_t *y, int B, bool cfg,
                             float cfg_scale, float *out, hipStream_t stream) {
    OT_CHECK_ARG(e && x && t && out, "%s: null pointer", who);
    OT_CHECK_ARG(y || e->cfg.extras != 2, "%s: null labels (the model has extras == 2)", who);
    OT_CHECK_ARG(aligned16(x) && aligned16(out), "%s: unaligned pointer (16 bytes)", who);
    OT_CHECK_ARG(B >= 1 && latte_rows(e, B) <= (1ll << 24), "%s: B %d (>= 1, B * frames * tokens <= 2^24)", who, B);
    OT_CHECK_ARG(!cfg || B % 2 == 0, "%s: B %d must be even (the conditional and the unconditional half)", who, B);
    OT_CHECK_ARG(!cfg || std::isfinite(cfg_scale), "%s: cfg_scale is not finite", who);
    if (!e->finalized) {
        set_error("%s: engine not finalized", who);
        return OMNITOK_ERR_STATE;
    }
    const omnitok_latte_config &c = e->cfg;
    const int D = c.hidden, F = c.mlp_hidden, N = e->N, NF = c.num_frames, PC = (int)latte_patch_out(e), BF = B * NF;
    const int64_t M = latte_rows(e, B), modN = e->modN;
    const int fmt = e->lin.fmt;
    const bool lin16 = fmt != OMNITOK_DIT_LIN_FP32;
    const int afmt = e->attn_fmt;
    if (int rc = dit_grow(&e->work, &e->work_bytes, dit_work_floats(M, B, D, F, PC, modN, lin16) * 4)) return rc;
    const DitWork w(e->work, M, B, D, F, PC, lin16);
#define LATTE_RUN(call) \
    if (int rc_ = (call)) return rc_
    LATTE_RUN(omnitok_dit_patch_embed(x, cfg ? BF / 2 : BF, e->w_patch, e->b_patch, e->pos, BF, c.in_channels, c.input_size, c.patch_size, D,
                                      w.X, stream));
    LATTE_RUN(dit_conditioning(who, e->tb, e->w_t0, e->b_t0, e->w_t2, e->b_t2, e->ytable, e->y_rows, e->w_mod, e->b_mod, modN, t, y, B, D, w,
                               stream));
    for (int i = 0; i < c.depth; i += 2) {
        LATTE_RUN(dit_block(e->blocks[i], w, w.mod + (int64_t)i * 6 * D, modN, M, NF * N, D, F,
                            [&](const float *qkv, float *a32, unsigned short *a16) {
                                return dit_spatial_attn(qkv, BF, N, c.heads, e->hd, afmt, fmt, a32, a16, e->tb.flag, stream);
                            },
                            afmt != OMNITOK_DIT_ATTN_FP32, fmt, e->tb.flag, stream));
        if (i == 0) LATTE_RUN(omnitok_latte_add_temp_embed(w.X, e->temp, B, NF, N, D, stream));
        LATTE_RUN(dit_block(e->blocks[i + 1], w, w.mod + (int64_t)(i + 1) * 6 * D, modN, M, NF * N, D, F,
                            [&](const float *qkv, float *a32, unsigned short *) {  // fp32 only: the round pass runs behind it
                                return omnitok_latte_attn_temporal(qkv, B, NF, N, c.heads, e->hd, a32, stream);
                            },
                            false, fmt, e->tb.flag, stream));
    }
    const float *mf = w.mod + (int64_t)c.depth * 6 * D;  // shift | scale
    LATTE_RUN(omnitok_dit_ln_modulate(w.X, mf, mf + D, modN, M, NF * N, D, w.Xn, stream));
    LATTE_RUN(dit_linear(w.Xn, e->w_final, e->b_final, w.LIN, M, PC, D, stream));
    LATTE_RUN(omnitok_dit_unpatchify(w.LIN, BF, N, c.patch_size, e->Cout, out, stream));
    if (cfg) LATTE_RUN(dit_cfg_blend(out, BF, e->Cout, 4, (int64_t)c.input_size * c.input_size, cfg_scale, stream));
#undef LATTE_RUN
    return OMNITOK_OK;
}

extern "C" int omnitok_latte_forward(omnitok_latte *e, const float *x, const int64_t *t, const int64_t *y, int B, float *out,
                                     omnitok_stream_t stream) {
    return latte_forward_any("latte_forward", e, x, t, y, B, false, 1.0f, out, static_cast<hipStream_t>(stream));
}

extern "C" int omnitok_latte_forward_cfg(omnitok_latte *e, const float *x, const int64_t *t, const int64_t *y, int B, float cfg_scale,
                                         float *out, omnitok_stream_t stream) {
    return latte_forward_any("latte_forward_cfg", e, x, t, y, B, true, cfg_scale, out, static_cast<hipStream_t>(stream));
}

extern "C" int omnitok_latte_check(omnitok_latte *e, omnitok_stream_t stream) {
    OT_CHECK_ARG(e, "latte_check: null engine");
    return e->tb.check("latte", static_cast<hipStream_t>(stream));
}
