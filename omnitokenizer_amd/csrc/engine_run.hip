// Engine, one Transformer: the block walk (PEG, attention / window attention, pooling / Up blocks, FeedForward; residual
// order and grid tracking of reference attention.py:655-689) and the dispatch of its nn.Linear layers onto the GEMM kernels
// of the engine's mode (plane data flow gemm_pl.h | fp16 split gemm_h2.hip | bf16 split gemm_x3.hip | fp32 MFMA gemm.hip).
//
// run_transformer = per layer one stage by kind, then feed_forward; at the end norm_out.     stage -> flows -> kernels
//   pool_block 'a' 'm' 'l'    token_resample | eg_gemm (Linear 4D -> D)                     no residual, grid / 2
//   up_block 'n' 'r'          [eg_gemm (Linear D -> D)] -> token_resample                   no residual, grid * 2
//   temporal_block 't'        peg3d, then one of
//     temporal_single_token   T' = 1: plane: stats_pack -> gemm_pl on Wo . Wv | eg_gemm V -> [pack_rows] -> out-projection
//     temporal_fused5         T' = 5, causal, plane: stats_pack_temporal -> gemm_pl PL_TSCORE (q|k) -> gemm_pl PL_TPV (V)
//     produce_qkv             plane: stats_pack -> gemm_pl (packing epilogues q|k + V | fp32 q|k|v, per chunk with
//                             "temporal_chunk") | row_stats -> eg_gemm merged q|k|v [V planes] | layernorm -> eg_gemm q, kv
//     run_attention           spatial: [attn_pack] -> attn_spatial_h2 | qk_prep -> attn_spatial; temporal: attn_temporal
//     out-projection          plane: [pack_rows] -> gemm_out_pl (+ residual, LayerNorm planes of the FeedForward) | eg_gemm
//   window_block 'w'          plane: stats_pack_windows -> gemm_pl q|k + V -> attn_window_h2 | stats_pack -> gemm_pl -> attn_window (planes)
//                             | row_stats / layernorm -> eg_gemm -> attn_window; out-projection as above
//   feed_forward              plane: [layernorm -> pack_rows] -> gemm_pl GEGLU -> gemm_pl (+ residual) | row_stats / layernorm -> eg_gemm x 2
//   norm_out                  layernorm_planes (to_pixels) | layernorm_prevq (encoder end) | layernorm_transposed | layernorm
#include "engine.h"

namespace omnitok {

// arithmetic of each kernel is independent of the problem / tile size (batch-size independence).
int g_gemm_mode = 2;
// Spatial attention arithmetic.  "attn_mode"
//   1 (default): fp16-split operands on the fp16 MFMA (attn_h2.hip) wherever the per-clip ranges of the row
//      statistics pass exist (the split-operand GEMM path) and the q/k scales are usable;
//   0: the fp32-input MFMA kernel of attn_spatial.hip.
int g_attn_mode = 1;
// "attn_vpack" 1 (default): the merged q|k|v launch writes V straight into the attention kernel's fp16 planes
int g_attn_vpack = 1;
// "gemm_pl" 1 (default): to_out / proj, FF-in and FF-out run as plane x plane GEMMs (gemm_pl.h) whose activation operands
// are written as fp16 hi|lo planes by their producers (attention kernels, the LayerNorm epilogue of to_out, the GEGLU
// epilogue of FF-in): no row-statistics pass and no in-loop LayerNorm / split in front of the FeedForward.  0: the
// r02 data flow (fp32 activations everywhere, gemm_h2.hip splits its A operand in the K loop).
// "pl_min_tokens" (default 0 since r06: ONE data flow at every call size): calls with fewer tokens (B * T' * h * w) than this
// take the gemm_pl 0 data flow even when gemm_pl is 1.  Rounds 4-5 shipped 12288 here because the plane GEMM only had 256 x 256
// tiles (one 256^2 image 4.09 ms vs 2.00 ms, profiles/r04_small_batch_latency.txt) -- and a clip's low bits then depended on
// the size of the call it was in.  With the thin-tile family of gemm_pl.hip (128 x 128 / 128 x 64 / 32- and 64-row LayerNorm
// tiles, same bits as the big tiles) the plane flow is as fast or faster at every size (one image 2.40 vs 2.39 ms of kernel
// time, one clip 4.23 vs 4.44, two clips 5.86 vs 6.39: profiles/r06_small_calls.txt), so a clip is now encoded and decoded to
// the same bits alone and inside any batch.  The option stays as an A/B switch (also per engine:
// omnitok_engine_set_option "pl_min_tokens", -1 = this process default).
int g_gemm_pl = 1;
int g_pl_min_tokens = 0;
// "temporal_chunk" (clips per chunk, 0 = off): a temporal 't' block runs its q|k|v plane GEMM and the temporal attention
// kernel chunk by chunk -- GEMM(chunk) -> attention(chunk) back to back through ONE chunk-sized fp32 q|k|v buffer (31.5 MB
// per 17x256^2 clip), so that the attention kernel's reads hit the 256 MiB Infinity Cache instead of HBM
// (profiles/r05_temporal_chunk.txt).  Results are bit-identical to the unchunked launch: tiles never straddle a clip.
int g_temporal_chunk = 0;
// "prevq_fuse" 1 (default): omnitok_encode runs pre_vq inside the encoder's last LayerNorm pass (omnitok_layernorm_prevq,
// bit-identical) whenever nothing sits between the two (no deferred pools); 0: LayerNorm store, then omnitok_pre_vq.
int g_prevq_fuse = 1;
// "temporal_fused" 1 (default): temporal 't' blocks with T' == 5 (17-frame clips at temporal_patch_size 4), causal, on the plane
// data flow run WITHOUT the fp32 q|k|v round trip (2 GB per block at C3): omnitok_stats_pack_temporal permutes the rows so that
// a sequence's five steps sit in one lane pair, a q|k GEMM forms the softmax weights in its epilogue (PL_TSCORE: the k wave hands
// k_s to the q wave through LDS) and a V GEMM applies them in its own (PL_TPV), writing the out-projection's operand planes.
// C3: 0.616 + 0.339 ms per block against 0.658 + 0.263 for the q|k|v GEMM + attn_temporal pair, but 2 GB less HBM traffic per
// block on a power-capped step: -0.86 ms per step (profiles/r05_temporal_fused.txt).  0: q|k|v GEMM + attn_temporal kernel
// (what every other T', non-causal configurations and grids with S % 64 != 0 take anyway).
int g_temporal_fused = 1;
// "qkv_pl" 1 (default, with gemm_pl): the q|k|v projection as a plane GEMM too -- one pass writes the row statistics and
// the centred rows x - mean as planes (omnitok_stats_pack), the LayerNorm of the Q columns is folded into the weight and finished in the
// epilogue, which for spatial attention also does RoPE + l2norm + scales and writes Q and K straight into the attention
// kernel's packed planes (no fp32 Q / K, no attn_pack pass); V by a swapped-orientation launch.  0: gemm_h2 with the
// LayerNorm fused into its A loader (r02 form).
int g_qkv_pl = 1;
// "attn_window_mode" 1 (default, with gemm_pl / qkv_pl): window attention on the fp16 matrix cores from packed operands --
// the q|k|v plane GEMM runs on window-major rows (omnitok_stats_pack_windows) and its packing epilogues write what
// omnitok_attn_window_h2 reads; no fp32 q|k|v in memory.  0: fp32 q|k|v + the fp32-MFMA kernel of attn_spatial.hip.
int g_attn_window_mode = 1;

int gemm_mode_of(const omnitok_engine *e) { return e->opt_gemm_mode >= 0 ? e->opt_gemm_mode : g_gemm_mode; }
int attn_mode_of(const omnitok_engine *e) { return e->opt_attn_mode >= 0 ? e->opt_attn_mode : g_attn_mode; }
int attn_vpack_of(const omnitok_engine *e) { return e->opt_attn_vpack >= 0 ? e->opt_attn_vpack : g_attn_vpack; }
int gemm_pl_of(const omnitok_engine *e, int64_t tokens) {
    const int min_tokens = e->opt_pl_min_tokens >= 0 ? e->opt_pl_min_tokens : g_pl_min_tokens;
    return (e->opt_gemm_pl >= 0 ? e->opt_gemm_pl : g_gemm_pl) && tokens >= min_tokens;
}
static int temporal_chunk_of(const omnitok_engine *e) { return e->opt_temporal_chunk >= 0 ? e->opt_temporal_chunk : g_temporal_chunk; }

bool x3_ok(const omnitok_engine *e, int N, int K, int flags) {
    return gemm_mode_of(e) >= 1 && N % 32 == 0 && K % 32 == 0 && !(flags & OMNITOK_GEMM_LEAKY) &&
           (!(flags & OMNITOK_GEMM_GEGLU) || N % 64 == 0);
}

float *next_bounds(omnitok_engine *e) {  // [n_clips][2] slots of one row-statistics launch
    if (e->bound_next >= N_BOUND_LAUNCHES) return nullptr;
    return e->bounds + (int64_t)2 * e->bound_clips * (e->bound_next++);
}

int eg_gemm(omnitok_engine *e, const EgGemm &g, hipStream_t stream, bool *vpacked) {
    omnitok_row_gemm d = {};
    d.a = g.a; d.lda = g.lda; d.w = g.w; d.ldw = g.ldw;
    d.bias = g.bias; d.residual = g.residual; d.ldr = g.ldr; d.c = g.c; d.ldc = g.ldc;
    d.M = g.M; d.N = g.N; d.K = g.K; d.flags = g.flags;
    d.a_rows_per_group = g.rpg; d.a_group_stride = g.gstride; d.a_group_offset = g.goff;
    d.a_bound = g.ab.stat; d.a_bound_dev = g.ab.dev; d.a_bound_stride = 2; d.a_rows_per_clip = g.ab.rpc;
    d.ln_stats = g.ln_stats; d.ln_gamma = g.ln_g; d.ln_beta = g.ln_b; d.ln_cols = g.ln_cols; d.ln_bound = g.ln_bound;
    d.c2 = g.c2; d.ldc2 = g.ldc2; d.split_col = g.split_col;
    if (gemm_mode_of(e) == 2 && g.ab.stat > 0.0f && x3_ok(e, g.N, g.K, g.flags) && (!g.ln_stats || g.ln_bound > 0.0f) &&
        (!g.ab.dev || (g.ab.rpc > 0 && g.ab.rpc % 64 == 0 && g.rpg == 0))) {
        auto it = e->h2w.find(g.w);
        if (it != e->h2w.end() && g.ldw == g.K) {
            d.w = nullptr; d.ldw = 0; d.w_planes = it->second.pl; d.w_scale = it->second.sc;
            if (g.vpk && g.ab.dev && g.ab.rpc % 128 == 0) {  // V columns straight into the attention kernel's fp16 planes
                *vpacked = true;
                d.v_planes = g.vpk->planes; d.v_col0 = g.vpk->col0; d.n_tokens = g.vpk->n_tokens; d.heads = g.vpk->heads;
                d.v_bound = g.vpk->bound; d.v_bound_dev = g.vpk->bound_dev; d.v_bound_stride = 2;
            }
            return omnitok_gemm_h2(&d, stream);
        }
    }
    if (x3_ok(e, g.N, g.K, g.flags)) return omnitok_gemm_x3(&d, stream);
    if (g.ln_stats) {
        set_error("eg_gemm: fused LayerNorm needs the x3 / h2 kernel");
        return OMNITOK_ERR_STATE;
    }
    return omnitok_gemm(&d, stream);
}

// plane x plane GEMM of the engine: the weight is looked up by its fp32 pointer
static int eg_gemm_pl(omnitok_engine *e, omnitok_pl_gemm g, const float *w, hipStream_t stream) {
    auto it = e->plw.find(w);
    if (it == e->plw.end()) {
        set_error("eg_gemm_pl: weight was not packed for the plane GEMM");
        return OMNITOK_ERR_STATE;
    }
    g.w = it->second.pl;
    g.w_scale = it->second.sc;
    return omnitok_gemm_pl(&g, stream);
}

// (planes, scales) of the columns [col0, ...) of a packed plane weight [N, K] (col0 % 64 == 0)
static H2W pl_cols(const H2W &w, int col0, int K) {
    return H2W{static_cast<const char *>(w.pl) + pl_row_offset(col0, K), w.sc + col0};
}

namespace {

struct AttnPlanes {  // packed Q / K / V operands of the fp16 attention kernels
    unsigned char *qp, *kp, *vp;
};

// per 't' block: the ranges of its x and the operands its stages share
struct TBlock {
    float *bs;       // device-side ranges of this layer's x, or nullptr
    int64_t rpc;     // rows per clip
    ABound ab_x, ab_ao;
    float *Q, *KV;   // fp32 Q [L, D] and K|V [L, 2D]
    float qb, kb;    // ranges of the l2-normalised q / k
    bool attn_h2;    // fp16-split spatial attention
    AttnPlanes p;
};

// what "produce q|k|v" hands to "run attention" and to the out-projection
struct QkvState {
    bool vpacked = false;        // the q|k|v launch wrote the V planes itself (no fp32 V round trip)
    bool qk_packed = false;      // the q|k launch wrote the packed Q / K planes itself (no attn_pack pass)
    bool ao_planes = false;      // the attention kernel wrote its output as planes (AO) with row scales (ST)
    bool temporal_done = false;  // the chunked temporal stage ran GEMM and attention already
};

// One run_transformer call: what its stages share.  The stage functions are members so that their bodies read the state
// (e, stream, L, S, gemm_f, pl, ...) by the names the launches are written with.
struct Run {
    omnitok_engine *e;
    const TransformerW &tw;
    hipStream_t stream;
    const omnitok_config &c;
    const int D, heads, B, T;
    const bool spatial;
    int gh = 0, gw = 0, S = 0;
    int64_t L = 0;
    double gemm_f = 0.0;
    bool fused = false;            // split-operand GEMMs apply the LayerNorm while staging their A operand (no LN pass over HBM)
    bool pl = false;               // plane data flow (gemm_pl.h)
    bool ln_planes_ready = false;  // Y holds the planes of the FeedForward's LayerNorm(x) for the current x

    Run(omnitok_engine *e_, const TransformerW &tw_, hipStream_t stream_, int B_, int T_, bool spatial_)
        : e(e_), tw(tw_), stream(stream_), c(e_->cfg), D(e_->cfg.dim), heads(e_->cfg.heads), B(B_), T(T_), spatial(spatial_) {}

    void set_grid(int gh_, int gw_) {
        gh = gh_;
        gw = gw_;
        S = gh * gw;
        L = (int64_t)B * T * S;
        gemm_f = 2.0 * (double)L * D;
    }
    // Y, HD are free while a block's attention runs
    AttnPlanes attn_planes() const {
        unsigned char *kp = reinterpret_cast<unsigned char *>(e->HD.p);
        return AttnPlanes{reinterpret_cast<unsigned char *>(e->Y.p), kp, kp + (size_t)L * D * 4};
    }
    // the fields every q|k|v plane GEMM shares: centred rows of x as planes (X2) with their row scales (Z) and statistics (ST)
    omnitok_pl_gemm qkv_pl_base(const H2W &w) const {
        omnitok_pl_gemm g{};
        g.a = e->X2.p;
        g.a_scale = e->Z.p;  // [L] row scales of the raw planes (Z is free inside a Transformer)
        g.w = w.pl;
        g.w_scale = w.sc;
        g.fold_stats = e->ST.p;
        g.M = L;
        g.K = D;
        return g;
    }
    // the fields the attention calls of a 't' block share: fp32 q | k|v rows, the q/k scales, the ranges of q, k and (per clip)
    // of V = of the output, the output as fp32 rows (AO) and, with `planes`, as planes (AO) with row scales (ST)
    omnitok_attn_desc attn_base(const Layer &ly, const TBlock &t, float *Q, float *KV, bool planes) const {
        omnitok_attn_desc a{};
        a.q = Q; a.ldq = D; a.k = KV; a.v = KV + D; a.ldkv = 2 * D;
        a.q_scale = ly.t.q_scale; a.k_scale = ly.t.k_scale; a.scale = 8.0f; a.heads = heads;
        a.q_bound = t.qb; a.k_bound = t.kb; a.v_bound = t.ab_ao.stat; a.v_bound_dev = t.ab_ao.dev; a.v_bound_stride = 2;
        a.out = e->AO.p; a.ldo = D; a.out_planes = planes ? e->AO.p : nullptr; a.out_scale = planes ? e->ST.p : nullptr;
        return a;
    }

    void decide_flow();
    int pack_rows(const float *src, void *planes, float *scales);
    int gemm_out_pl(const Layer &ly, const void *a_planes, const float *a_scale, float a_const, const float *w, const float *bias);
    int pool_block(const Layer &ly);
    int up_block(const Layer &ly);
    int temporal_block(const Layer &ly);
    int temporal_single_token(const Layer &ly, const TBlock &t);
    int temporal_fused5(const Layer &ly, const TBlock &t);
    int produce_qkv(const Layer &ly, const TBlock &t, QkvState &st);
    int produce_qkv_chunked(const Layer &ly, const TBlock &t, const omnitok_pl_gemm &g, int chunk, QkvState &st);
    int run_attention(const Layer &ly, const TBlock &t, QkvState &st);
    int window_block(const Layer &ly);
    int feed_forward(const Layer &ly);
    int norm_out(bool transpose_out, bool out_planes, const PreVqFuse *pv);
};

void Run::decide_flow() {
    fused = x3_ok(e, 3 * D, D, 0) && D <= 512;
    // Plane data flow (gemm_pl.h): attention output -> planes (AO) -> to_out / proj with the residual add and the
    // FeedForward's LayerNorm in its epilogue (x in place, LN(x) planes -> Y) -> FF-in with the GEGLU hidden as planes
    // (HD) -> FF-out (+ residual).  Needs full-row tiles for the LayerNorm epilogue (dim 512 = the reference's only width).
    bool pl_ok = gemm_pl_of(e, L) && gemm_mode_of(e) == 2 && fused && D == 512 && x3_ok(e, 2 * e->inner_pad, D, OMNITOK_GEMM_GEGLU);
    // the plane producers scale by constants derived from the static operand bounds: a degenerate FeedForward LayerNorm
    // (gamma == beta == 0 gives bound 0) or a non-finite bound sends the whole Transformer down the gemm_h2 / x3 branch,
    // which handles missing ranges by itself
    for (const Layer &ly : tw.layers)
        if (!(ly.ff.ln_bound > 0.0f && ly.ff.ln_bound < 1e30f && ly.ff.h_bound > 0.0f && ly.ff.h_bound < 1e30f)) pl_ok = false;
    pl = pl_ok;
}

// producers that cannot write planes themselves: fp32 rows -> planes with one power-of-two scale per row
int Run::pack_rows(const float *src, void *planes, float *scales) {
    OT_RUN("pack_rows", 2.0 * L * D * 4.0, omnitok_pl_pack_rows(src, D, L, D, pad256(L), planes, scales, 0.0f, stream));
    return OMNITOK_OK;
}

// to_out / proj as a plane GEMM: x += a . w^T (+ bias), and the planes of LN_ff(x) -> Y
int Run::gemm_out_pl(const Layer &ly, const void *a_planes, const float *a_scale, float a_const, const float *w,
                     const float *bias) {
    omnitok_pl_gemm g{};
    g.a = a_planes;
    g.a_scale = a_scale;
    g.a_scale_const = a_const;
    g.bias = bias;
    g.residual = e->X.p;
    g.ldr = D;
    g.c = e->X.p;
    g.ldc = D;
    g.out_planes = e->Y.p;
    g.out_planes_k = D;
    g.out_bound = ly.ff.ln_bound;
    g.ln_gamma = ly.ff.lw;
    g.ln_beta = ly.ff.lb;
    g.ln_eps = 1e-5f;
    g.epilogue = 2;
    g.M = L;
    g.N = D;
    g.K = D;
    OT_RUN("gemm_out", gemm_f * D, eg_gemm_pl(e, g, w, stream));
    ln_planes_ready = true;
    return OMNITOK_OK;
}

// Pooling (reference attention.py:83-113), no residual (:674); then FF (+residual) on the quarter-size sequence
int Run::pool_block(const Layer &ly) {
    if (!spatial || gh % 2 || gw % 2) {
        set_error("pooling block '%c' on a %dx%d grid", ly.kind, gh, gw);
        return OMNITOK_ERR_INVALID;
    }
    if (ly.kind == 'l') {  // Linear(4D -> D) on four consecutive tokens: x.view(B, N/4, 4C)
        EgGemm g;
        g.a = e->X.p; g.lda = 4 * D;
        g.w = ly.pool_w; g.ldw = 4 * D;
        g.bias = ly.pool_b;
        g.c = e->X2.p; g.ldc = D;
        g.M = L / 4; g.N = D; g.K = 4 * D;
        g.flags = OMNITOK_GEMM_BIAS;
        OT_RUN("pool", 2.0 * (double)L * D * D, eg_gemm(e, g, stream));
    } else {
        OT_RUN("pool", 1.25 * L * D * 4.0,
               omnitok_token_resample(e->X.p, e->X2.p, ly.kind == 'a' ? 0 : 1, (int64_t)B * T, 1, gh, gw, D, stream));
    }
    std::swap(e->X, e->X2);
    set_grid(gh / 2, gw / 2);
    return OMNITOK_OK;
}

// Up (reference attention.py:116-150): nearest 2x2 up-sampling of the token grid, no residual (:674),
// 'r' adds Linear(D, D).  A row-wise Linear commutes with the row duplication bit for bit, so it
// runs on the L source rows (a quarter of the work) and the result is up-sampled.
int Run::up_block(const Layer &ly) {
    if (!spatial) {
        set_error("Up block '%c' in a temporal transformer", ly.kind);
        return OMNITOK_ERR_INVALID;
    }
    const float *src = e->X.p;
    if (ly.kind == 'r') {
        EgGemm g;
        g.a = e->X.p; g.lda = D;
        g.w = ly.pool_w; g.ldw = D;
        g.bias = ly.pool_b;
        g.c = e->Y.p; g.ldc = D;
        g.M = L; g.N = D; g.K = D;
        g.flags = OMNITOK_GEMM_BIAS;
        OT_RUN("pool", 2.0 * (double)L * D * D, eg_gemm(e, g, stream));
        src = e->Y.p;
    }
    OT_RUN("pool", 1.25 * 4.0 * L * D * 4.0, omnitok_token_resample(src, e->X2.p, 2, (int64_t)B * T, 1, gh, gw, D, stream));
    std::swap(e->X, e->X2);
    set_grid(gh * 2, gw * 2);
    return OMNITOK_OK;
}

// 't' block: PEG, then attention over the frame's tokens (spatial) or over time (temporal), then the out-projection
int Run::temporal_block(const Layer &ly) {
    OT_RUN("peg3d", 2.0 * L * D * 4.0,
           omnitok_peg3d(e->X.p, ly.t.peg_w27, ly.t.peg_b, e->X2.p, B, T, gh, gw, D, c.causal_peg, stream));
    std::swap(e->X, e->X2);
    TBlock t;
    // device-side ranges of this layer's x (filled by the row-statistics pass): bs[0] >= max |x|,
    // bs[1] >= max ||x_row||; |V_j| <= ||x|| ||Wv_j|| bounds the attention output (a convex
    // combination of V rows) -- what the fp16-split GEMMs need (gemm_h2.hip)
    t.bs = fused ? next_bounds(e) : nullptr;
    if (fused && !t.bs) {
        set_error("run_transformer: out of range slots");
        return OMNITOK_ERR_STATE;
    }
    t.rpc = L / B;  // both token orders keep a clip's rows contiguous (b is the outermost index)
    t.ab_x = t.bs ? ABound{1.01f, t.bs, t.rpc} : ABound();
    t.ab_ao = t.bs ? ABound{1.01f * ly.t.vnorm, t.bs + 1, t.rpc} : ABound();
    if (!spatial && T == 1) return temporal_single_token(ly, t);
    if (!spatial && T == 5 && pl && g_qkv_pl && g_temporal_fused && t.bs && c.causal_temporal && ly.t.wqk_t &&
        e->plw.count(ly.t.wqk_t) && ly.t.wqkv_fold && e->plw.count(ly.t.wqkv_fold) && S % 64 == 0 && heads * 64 == D &&
        ly.t.vnorm > 0.0f)
        return temporal_fused5(ly, t);
    t.Q = e->QKV.p;
    t.KV = e->QKV.p + L * D;
    // fp16-split spatial attention (attn_h2.hip): Q, K (RoPE + l2norm + scales applied) and V as hi|lo planes
    // in MFMA fragment order (Y, HD are free here); |V| <= ||x_row|| ||Wv_j|| per clip from the row statistics
    t.qb = 1.01f * 8.0f * ly.t.q_amax;
    t.kb = 1.01f * ly.t.k_amax;
    t.attn_h2 = spatial && attn_mode_of(e) == 1 && t.bs && S % 64 == 0 && t.qb > 0.0f && t.kb > 0.0f && ly.t.vnorm > 0.0f &&
                t.qb < 1e30f && t.kb < 1e30f;
    t.p = attn_planes();
    QkvState st;
    if (int rc = produce_qkv(ly, t, st)) return rc;
    if (int rc = run_attention(ly, t, st)) return rc;
    if (pl) {
        const void *ap = e->AO.p;
        if (!st.ao_planes) {  // fp32 attention output (fp32-MFMA attention kernel, long temporal sequences): pack it
            if (int rc = pack_rows(e->AO.p, e->QKV.p, e->ST.p)) return rc;
            ap = e->QKV.p;
        }
        return gemm_out_pl(ly, ap, e->ST.p, 1.0f, ly.t.wo, nullptr);
    }
    EgGemm g;
    g.a = e->AO.p; g.lda = D;
    g.w = ly.t.wo; g.ldw = D;
    g.residual = e->X.p; g.ldr = D;
    g.c = e->X.p; g.ldc = D;
    g.M = L; g.N = D; g.K = D;
    g.flags = OMNITOK_GEMM_RESIDUAL;
    g.ab = t.ab_ao;
    OT_RUN("gemm_out", gemm_f * D, eg_gemm(e, g, stream));
    return OMNITOK_OK;
}

// Images: a temporal sequence of one token.  softmax over a single key is exactly 1
// (causal or not, with or without ALiBi), so the attention output is V bit for bit:
// only the V half of to_kv is needed (rows [D, 2D) of the weight); LN, to_q, the K
// half and the attention kernel drop out.  Identical results to the general path.
int Run::temporal_single_token(const Layer &ly, const TBlock &t) {
    if (pl && ly.t.wvo && e->plw.count(ly.t.wvo)) {
        // plane data flow: x as planes (one power-of-two scale per row) -> ONE GEMM on Wo . Wv with the residual
        // add and the FeedForward's LayerNorm planes in its epilogue.  (x Wv^T) Wo^T = x (Wo Wv)^T in exact
        // arithmetic; the composed weight is rounded once from fp64, the two-step form rounds V to fp32 in
        // between -- both inside the path's fp32 noise (golden image fixtures, tests/test_gpu_e2e.py).
        OT_RUN("stats_pack", 2.0 * L * D * 4.0,
               omnitok_stats_pack(e->X.p, L, D, 1e-5f, 0, e->X2.p, pad256(L), e->Z.p, nullptr, nullptr, 0, stream));
        return gemm_out_pl(ly, e->X2.p, e->Z.p, 1.0f, ly.t.wvo, nullptr);
    }
    if (t.bs && gemm_mode_of(e) == 2)  // only the ranges are needed here
        OT_RUN("row_stats", L * D * 4.0, omnitok_row_stats(e->X.p, L, D, 1e-5f, e->ST.p, t.bs, t.rpc, stream));
    EgGemm v;
    v.a = e->X.p; v.lda = D;
    v.w = ly.t.wkv + (int64_t)D * D; v.ldw = D;
    v.c = e->AO.p; v.ldc = D;
    v.M = L; v.N = D; v.K = D;
    v.ab = t.ab_x;
    OT_RUN("gemm_qkv", gemm_f * D, eg_gemm(e, v, stream));
    if (pl) {
        if (int rc = pack_rows(e->AO.p, e->QKV.p, e->ST.p)) return rc;
        return gemm_out_pl(ly, e->QKV.p, e->ST.p, 1.0f, ly.t.wo, nullptr);
    }
    EgGemm g;
    g.a = e->AO.p; g.lda = D;
    g.w = ly.t.wo; g.ldw = D;
    g.residual = e->X.p; g.ldr = D;
    g.c = e->X.p; g.ldc = D;
    g.M = L; g.N = D; g.K = D;
    g.flags = OMNITOK_GEMM_RESIDUAL;
    g.ab = t.ab_ao;
    OT_RUN("gemm_out", gemm_f * D, eg_gemm(e, g, stream));
    return OMNITOK_OK;
}

// fused temporal stage (gemm_pl.h PL_TSCORE / PL_TPV; reference attention.py:402-486 with is_spatial = False)
int Run::temporal_fused5(const Layer &ly, const TBlock &t) {
    const int64_t nseq = (int64_t)B * S;
    float *P = e->QKV.p, *out_scale = e->QKV.p + nseq * heads * 40;
    OT_RUN("stats_pack", 2.0 * L * D * 4.0,
           omnitok_stats_pack_temporal(e->X.p, nseq, D, 1e-5f, e->X2.p, e->Z.p, e->ST.p, t.bs, S, stream));
    const float *alibi = c.legacy_attention ? e->alibi : nullptr;
    omnitok_pl_gemm g = qkv_pl_base(H2W{});
    g.tp = P;
    g.t_nseq = (int)nseq;
    g.t_heads = heads;
    g.t_alibi = alibi;
    omnitok_pl_gemm q = g;
    const H2W &wqk = e->plw[ly.t.wqk_t];
    q.w = wqk.pl;
    q.w_scale = wqk.sc;
    q.fold_b = ly.t.qk_t_fb;
    q.fold_u = ly.t.qk_t_fu;
    q.N = 2 * D;
    q.epilogue = 6;
    q.q_scale = ly.t.q_scale;
    q.k_scale = ly.t.k_scale;
    q.q_mul = 8.0f;
    OT_RUN("gemm_qkv", gemm_f * 2 * D, omnitok_gemm_pl(&q, stream));
    const H2W wv = pl_cols(e->plw[ly.t.wqkv_fold], 2 * D, D);
    omnitok_pl_gemm v = g;
    v.w = wv.pl;
    v.w_scale = wv.sc;
    v.fold_u = ly.t.fold_u + 2 * D;
    v.N = D;
    v.epilogue = 7;
    v.out_planes = e->AO.p;
    v.out_planes_k = D;
    v.t_out_scale = out_scale;
    v.v_bound = t.ab_ao.stat;
    v.v_bound_dev = t.ab_ao.dev;
    v.v_bound_stride = 2;
    v.t_seqs_per_clip = S;
    OT_RUN("gemm_qkv", gemm_f * D, omnitok_gemm_pl(&v, stream));
    return gemm_out_pl(ly, e->AO.p, out_scale, 1.0f, ly.t.wo, nullptr);
}

// Q from LN(x), K/V from the raw x (reference attention.py:404-412)
int Run::produce_qkv(const Layer &ly, const TBlock &t, QkvState &st) {
    const VPack vpk{t.p.vp, 2 * D, S, heads, t.ab_ao.stat, t.ab_ao.dev};
    const bool qkv_pl = pl && g_qkv_pl && ly.t.wqkv_fold && e->plw.count(ly.t.wqkv_fold) && t.bs;
    if (qkv_pl) {
        OT_RUN("stats_pack", 2.0 * L * D * 4.0,
               omnitok_stats_pack(e->X.p, L, D, 1e-5f, 1, e->X2.p, pad256(L), e->Z.p, e->ST.p, t.bs, t.rpc, stream));
        const H2W &wf = e->plw[ly.t.wqkv_fold];
        omnitok_pl_gemm g = qkv_pl_base(wf);
        g.fold_b = ly.t.fold_b;
        g.fold_u = ly.t.fold_u;
        g.fold_cols = D;
        if (t.attn_h2 && t.rpc % 256 == 0) {
            // spatial attention on packed operands: Q | K through the packing epilogue, V through the swapped launch
            const float *cosp = nullptr, *sinp = nullptr;
            if (c.spatial_rope)
                if (int rc = get_rope(e, S, &cosp, &sinp, stream)) return rc;
            omnitok_pl_gemm q = g;
            q.N = 2 * D;
            q.epilogue = 4;
            q.qp = t.p.qp;
            q.kp = t.p.kp;
            q.qk_k0 = D;
            q.n_tokens = S;
            q.heads = heads;
            q.rope_cos = cosp;
            q.rope_sin = sinp;
            q.q_scale = ly.t.q_scale;
            q.k_scale = ly.t.k_scale;
            q.q_mul = 8.0f;
            q.q_bound = t.qb;
            q.k_bound = t.kb;
            OT_RUN("gemm_qkv", gemm_f * 2 * D, omnitok_gemm_pl(&q, stream));
            const H2W wv = pl_cols(wf, 2 * D, D);
            omnitok_pl_gemm v = g;
            v.fold_cols = 0;                 // every V column: xc . Wv^T + mean u
            v.fold_b = nullptr;
            v.fold_u = ly.t.fold_u + 2 * D;
            v.w = wv.pl;
            v.w_scale = wv.sc;
            v.N = D;
            v.epilogue = 3;
            v.vp = t.p.vp;
            v.n_tokens = S;
            v.heads = heads;
            v.v_bound = t.ab_ao.stat;
            v.v_bound_dev = t.ab_ao.dev;
            v.v_bound_stride = 2;
            v.rows_per_clip = t.rpc;
            OT_RUN("gemm_qkv", gemm_f * D, omnitok_gemm_pl(&v, stream));
            st.vpacked = true;
            st.qk_packed = true;
            return OMNITOK_OK;
        }
        g.N = 3 * D;
        g.epilogue = 0;
        g.c = t.Q;
        g.ldc = D;
        g.c2 = t.KV;
        g.ldc2 = 2 * D;
        g.c_split_n = D;
        const int chunk = (!spatial && T > 1) ? temporal_chunk_of(e) : 0;
        if (chunk > 0 && chunk < B && T <= 17 && S % 16 == 0 && t.rpc % 256 == 0) return produce_qkv_chunked(ly, t, g, chunk, st);
        OT_RUN("gemm_qkv", gemm_f * 3 * D, omnitok_gemm_pl(&g, stream));
        return OMNITOK_OK;
    }
    if (fused && D % 256 == 0) {
        // one launch on the merged weight: the LayerNorm is applied while the A tile is staged,
        // for the Q columns only; QKV rows are [q | k | v]
        OT_RUN("row_stats", L * D * 4.0, omnitok_row_stats(e->X.p, L, D, 1e-5f, e->ST.p, t.bs, t.rpc, stream));
        // ... and the two column ranges land in two dense tensors (Q [L, D], K|V [L, 2D]): the attention
        // kernels read rows of D / 2D floats (with a [L, 3D] row pitch spatial attention ran 15 % slower)
        EgGemm g;
        g.a = e->X.p; g.lda = D;
        g.w = ly.t.wqkv; g.ldw = D;
        g.c = t.Q; g.ldc = D;
        g.M = L; g.N = 3 * D; g.K = D;
        g.ab = t.ab_x;
        g.ln_stats = e->ST.p; g.ln_g = ly.t.ng; g.ln_b = ly.t.nb;
        g.ln_cols = D; g.ln_bound = ly.t.ln_bound;
        g.c2 = t.KV; g.ldc2 = 2 * D; g.split_col = D;
        g.vpk = t.attn_h2 && attn_vpack_of(e) ? &vpk : nullptr;
        OT_RUN("gemm_qkv", gemm_f * 3 * D, eg_gemm(e, g, stream, &st.vpacked));
        return OMNITOK_OK;
    }
    EgGemm q, kv;
    q.lda = D;
    q.w = ly.t.wq; q.ldw = D;
    q.c = t.Q; q.ldc = D;
    q.M = L; q.N = D; q.K = D;
    kv.a = e->X.p; kv.lda = D;
    kv.w = ly.t.wkv; kv.ldw = D;
    kv.c = t.KV; kv.ldc = 2 * D;
    kv.M = L; kv.N = 2 * D; kv.K = D;
    if (fused) {
        OT_RUN("row_stats", L * D * 4.0, omnitok_row_stats(e->X.p, L, D, 1e-5f, e->ST.p, t.bs, t.rpc, stream));
        q.a = e->X.p;
        q.ab = t.ab_x;
        q.ln_stats = e->ST.p; q.ln_g = ly.t.ng; q.ln_b = ly.t.nb;
        q.ln_cols = D; q.ln_bound = ly.t.ln_bound;
        kv.ab = t.ab_x;
    } else {
        OT_RUN("layernorm", 2.0 * L * D * 4.0, omnitok_layernorm(e->X.p, ly.t.ng, ly.t.nb, e->Y.p, L, D, 1e-5f, 0, 0, 0, stream));
        q.a = e->Y.p;
    }
    OT_RUN("gemm_qkv", gemm_f * D, eg_gemm(e, q, stream));
    OT_RUN("gemm_qkv", gemm_f * 2 * D, eg_gemm(e, kv, stream));
    return OMNITOK_OK;
}

// "temporal_chunk": GEMM(chunk) -> attention(chunk) through one chunk-sized q|k|v buffer that stays
// in the Infinity Cache between the two kernels.  A clip is a whole number of 256-row tiles and of
// 64-row plane blocks, so every launch computes exactly what the full launch computes for its rows.
int Run::produce_qkv_chunked(const Layer &ly, const TBlock &t, const omnitok_pl_gemm &g, int chunk, QkvState &st) {
    const float *alibi = (c.legacy_attention && c.causal_temporal) ? e->alibi : nullptr;
    float *Qc = e->QKV.p, *KVc = e->QKV.p + (int64_t)chunk * t.rpc * D;
    for (int c0 = 0; c0 < B; c0 += chunk) {
        const int nb = std::min(chunk, B - c0);
        const int64_t r0 = (int64_t)c0 * t.rpc, Lc = (int64_t)nb * t.rpc;
        const int64_t pl_off = pl_row_offset(r0, D);
        omnitok_pl_gemm gc = g;
        gc.a = static_cast<const char *>(g.a) + pl_off;
        gc.a_scale = e->Z.p + r0;
        gc.fold_stats = e->ST.p + 2 * r0;
        gc.c = Qc;
        gc.c2 = KVc;
        gc.M = Lc;
        OT_RUN("gemm_qkv", 2.0 * (double)Lc * D * 3 * D, omnitok_gemm_pl(&gc, stream));
        // out_scale rows [r0, r0 + Lc) of ST: behind every (mean, rstd) pair a later chunk still reads
        omnitok_attn_desc a = attn_base(ly, t, Qc, KVc, true);
        a.out = nullptr; a.out_planes = reinterpret_cast<char *>(e->AO.p) + pl_off; a.out_scale = e->ST.p + r0;
        a.v_bound_dev = t.ab_ao.dev + 2 * c0; a.seqs = (int64_t)nb * S; a.seqs_per_clip = S; a.n_tokens = T;
        a.causal = c.causal_temporal; a.alibi_slopes = alibi;
        OT_RUN("attn_temporal", 4.0 * Lc * D * 4.0, omnitok_attn_temporal(&a, stream));
    }
    st.temporal_done = true;
    st.ao_planes = true;
    return OMNITOK_OK;
}

int Run::run_attention(const Layer &ly, const TBlock &t, QkvState &st) {
    if (spatial) {
        const float *cosp = nullptr, *sinp = nullptr;
        if (c.spatial_rope)
            if (int rc = get_rope(e, S, &cosp, &sinp, stream)) return rc;
        const float *bias = nullptr;
        if (!ly.t.bias_prefix.empty())
            if (int rc = get_bias_table(e, ly.t.bias_prefix, gh, gw, &bias, stream)) return rc;
        // Two launches, one descriptor each.  prep (RoPE + l2norm + scales of q and k; with attn_h2 also the packing) has the
        // rows, scales and ranges of attn_base and no output; a (the attention kernel) adds the bias and keeps the output
        omnitok_attn_desc prep = attn_base(ly, t, t.Q, t.KV, false), a = attn_base(ly, t, t.Q, t.KV, pl && t.attn_h2);
        prep.seqs = a.seqs = (int64_t)B * T; prep.seqs_per_clip = a.seqs_per_clip = T; prep.n_tokens = a.n_tokens = S;
        prep.rope_cos = cosp; prep.rope_sin = sinp; prep.out = nullptr;
        a.bias_table = bias; a.gh = gh; a.gw = gw;
        if (t.attn_h2) {
            a.qp = prep.qp = t.p.qp; a.kp = prep.kp = t.p.kp; a.vp = t.p.vp;
            if (st.vpacked) prep.v = nullptr;  // the q|k|v launch wrote the V planes: pack q and k only
            else prep.vp = t.p.vp;
            if (!st.qk_packed) OT_RUN("qk_prep", (st.vpacked ? 4.0 : 6.0) * L * D * 4.0, omnitok_attn_pack(&prep, stream));
            a.q = a.k = nullptr; a.v = nullptr;  // attn_spatial_h2 reads the planes only (and refuses the fp32 rows)
            OT_RUN("attn_spatial", 4.0 * (double)B * T * heads * (double)S * S * 64.0, omnitok_attn_spatial_h2(&a, stream));
            st.ao_planes = pl;
        } else {
            OT_RUN("qk_prep", 4.0 * L * D * 4.0, omnitok_qk_prep(&prep, stream));
            OT_RUN("attn_spatial", 4.0 * (double)B * T * heads * (double)S * S * 64.0, omnitok_attn_spatial(&a, stream));
        }
    } else if (!st.temporal_done) {
        const float *alibi = (c.legacy_attention && c.causal_temporal) ? e->alibi : nullptr;
        const bool tp = pl && t.bs && T <= 17 && S % 16 == 0;
        omnitok_attn_desc a = attn_base(ly, t, t.Q, t.KV, tp);
        a.seqs = (int64_t)B * S; a.seqs_per_clip = S; a.n_tokens = T;
        a.causal = c.causal_temporal; a.alibi_slopes = alibi;
        OT_RUN("attn_temporal", 4.0 * L * D * 4.0, omnitok_attn_temporal(&a, stream));
        st.ao_planes = tp;
    }
    return OMNITOK_OK;
}

// 'w' block: 8 x 8 window attention (reference attention.py:254-293), q, k, v all from LN(x)
int Run::window_block(const Layer &ly) {
    const auto okb = [](float v) { return v > 0.0f && v < 1e30f; };
    omnitok_attn_desc a{};  // what the three forms of the attention call share
    a.bias_dense = ly.w.bias_dense; a.seqs = (int64_t)B * T; a.gh = gh; a.gw = gw; a.heads = heads;
    if (pl && g_qkv_pl && g_attn_window_mode == 1 && ly.w.wqkv_fold && e->plw.count(ly.w.wqkv_fold) && c.window_size == 8 &&
        gh % 8 == 0 && gw % 8 == 0 && c.dim_head == 64 && okb(ly.w.q_bound) && okb(ly.w.k_bound) && okb(ly.w.ao_bound)) {
        // Window attention on packed operands (reference attention.py:254-293): the centred rows go out in
        // window-major order, so that every 64 consecutive GEMM rows are one window and the packing epilogues (n_tokens
        // = 64; no RoPE, no l2norm, q * head scale) write the attention kernel's Q / K / V blocks directly; the
        // attention kernel maps its output rows back to token order (window_reverse) as planes for the proj GEMM.
        OT_RUN("stats_pack", 2.0 * L * D * 4.0,
               omnitok_stats_pack_windows(e->X.p, L, D, 1e-5f, 1, e->X2.p, pad256(L), e->Z.p, e->ST.p, gh, gw, 8, stream));
        const H2W &wf = e->plw[ly.w.wqkv_fold];
        const AttnPlanes p = attn_planes();
        omnitok_pl_gemm g = qkv_pl_base(wf);
        g.fold_b = ly.w.fold_b;
        omnitok_pl_gemm q = g;
        q.N = 2 * D;
        q.fold_cols = 2 * D;
        q.epilogue = 4;
        q.qp = p.qp;
        q.kp = p.kp;
        q.qk_k0 = D;
        q.n_tokens = 64;
        q.heads = heads;
        q.q_mul = 1.0f / sqrtf((float)c.dim_head);
        q.q_bound = ly.w.q_bound;
        q.k_bound = ly.w.k_bound;
        OT_RUN("gemm_qkv", gemm_f * 2 * D, omnitok_gemm_pl(&q, stream));
        const H2W wv = pl_cols(wf, 2 * D, D);
        omnitok_pl_gemm v = g;
        v.w = wv.pl;
        v.w_scale = wv.sc;
        v.fold_b = ly.w.fold_b + 2 * D;
        v.fold_cols = D;
        v.N = D;
        v.epilogue = 3;
        v.vp = p.vp;
        v.n_tokens = 64;
        v.heads = heads;
        v.v_bound = ly.w.ao_bound;
        OT_RUN("gemm_qkv", gemm_f * D, omnitok_gemm_pl(&v, stream));
        a.qp = p.qp; a.kp = p.kp; a.vp = p.vp; a.out_planes = e->AO.p;
        a.q_bound = ly.w.q_bound; a.k_bound = ly.w.k_bound; a.v_bound = ly.w.ao_bound;
        OT_RUN("attn_window", 4.0 * (double)L * 64.0 * D, omnitok_attn_window_h2(&a, stream));
        return gemm_out_pl(ly, e->AO.p, nullptr, omnitok_pl_unscale(ly.w.ao_bound), ly.w.wproj, ly.w.bproj);
    }
    if (pl && g_qkv_pl && ly.w.wqkv_fold && e->plw.count(ly.w.wqkv_fold)) {
        // q, k, v all from LN(x) (reference attention.py:262-272): the gain folded into every weight row
        OT_RUN("stats_pack", 2.0 * L * D * 4.0,
               omnitok_stats_pack(e->X.p, L, D, 1e-5f, 1, e->X2.p, pad256(L), e->Z.p, e->ST.p, nullptr, 0, stream));
        omnitok_pl_gemm g = qkv_pl_base(e->plw[ly.w.wqkv_fold]);
        g.fold_b = ly.w.fold_b;
        g.fold_cols = 3 * D;
        g.c = e->QKV.p;
        g.ldc = 3 * D;
        g.N = 3 * D;
        OT_RUN("gemm_qkv", gemm_f * 3 * D, omnitok_gemm_pl(&g, stream));
    } else {
        EgGemm g;
        g.lda = D;
        g.w = ly.w.wqkv; g.ldw = D;
        g.c = e->QKV.p; g.ldc = 3 * D;
        g.M = L; g.N = 3 * D; g.K = D;
        if (fused) {
            OT_RUN("row_stats", L * D * 4.0, omnitok_row_stats(e->X.p, L, D, 1e-5f, e->ST.p, nullptr, 0, stream));
            g.a = e->X.p;
            g.ab = ABound{1.0f, nullptr, 0};
            g.ln_stats = e->ST.p; g.ln_g = ly.w.ng; g.ln_b = ly.w.nb;
            g.ln_cols = 3 * D; g.ln_bound = ly.w.ln_bound;
        } else {
            OT_RUN("layernorm", 2.0 * L * D * 4.0,
                   omnitok_layernorm(e->X.p, ly.w.ng, ly.w.nb, e->Y.p, L, D, 1e-5f, 0, 0, 0, stream));
            g.a = e->Y.p;
        }
        OT_RUN("gemm_qkv", gemm_f * 3 * D, eg_gemm(e, g, stream));
    }
    a.q = e->QKV.p; a.ldq = 3 * D;  // fp32 q|k|v: the fused rows go in q
    if (pl && ly.w.ao_bound > 0.0f) {
        a.out_planes = e->AO.p; a.out_bound = ly.w.ao_bound;
        OT_RUN("attn_window", 4.0 * (double)L * 64.0 * D, omnitok_attn_window(&a, stream));
        return gemm_out_pl(ly, e->AO.p, nullptr, omnitok_pl_unscale(ly.w.ao_bound), ly.w.wproj, ly.w.bproj);
    }
    a.out = e->AO.p; a.ldo = D;
    OT_RUN("attn_window", 4.0 * (double)L * 64.0 * D, omnitok_attn_window(&a, stream));
    EgGemm g;
    g.a = e->AO.p; g.lda = D;
    g.w = ly.w.wproj; g.ldw = D;
    g.bias = ly.w.bproj;
    g.residual = e->X.p; g.ldr = D;
    g.c = e->X.p; g.ldc = D;
    g.M = L; g.N = D; g.K = D;
    g.flags = OMNITOK_GEMM_BIAS | OMNITOK_GEMM_RESIDUAL;
    g.ab = fused ? ABound{ly.w.ao_bound, nullptr, 0} : ABound();
    OT_RUN("gemm_out", gemm_f * D, eg_gemm(e, g, stream));
    return OMNITOK_OK;
}

// FeedForward (reference attention.py:153-168)
int Run::feed_forward(const Layer &ly) {
    if (pl) {
        if (!ln_planes_ready) {  // after pooling / Up blocks: LayerNorm pass, then planes
            OT_RUN("layernorm", 2.0 * L * D * 4.0,
                   omnitok_layernorm(e->X.p, ly.ff.lw, ly.ff.lb, e->AO.p, L, D, 1e-5f, 0, 0, 0, stream));
            OT_RUN("pack_rows", 2.0 * L * D * 4.0,
                   omnitok_pl_pack_rows(e->AO.p, D, L, D, pad256(L), e->Y.p, nullptr, ly.ff.ln_bound, stream));
        }
        omnitok_pl_gemm g{};
        g.a = e->Y.p;
        g.a_scale_const = omnitok_pl_unscale(ly.ff.ln_bound);
        g.out_planes = e->HD.p;
        g.out_planes_k = e->inner_pad;
        g.out_bound = ly.ff.h_bound;
        g.epilogue = 1;
        g.M = L;
        g.N = 2 * e->inner_pad;
        g.K = D;
        OT_RUN("gemm_ff_in", gemm_f * 2 * c.ff_inner, eg_gemm_pl(e, g, ly.ff.w1p, stream));
        omnitok_pl_gemm h{};
        h.a = e->HD.p;
        h.a_scale_const = omnitok_pl_unscale(ly.ff.h_bound);
        h.residual = e->X.p;
        h.ldr = D;
        h.c = e->X.p;
        h.ldc = D;
        h.epilogue = 0;
        h.M = L;
        h.N = D;
        h.K = e->inner_pad;
        h.k_valid = c.ff_inner;  // the hidden's pad columns are exactly 0 (GEGLU epilogue) and so are the weight's
        OT_RUN("gemm_ff_out", gemm_f * c.ff_inner, eg_gemm_pl(e, h, ly.ff.w2p, stream));
        return OMNITOK_OK;
    }
    EgGemm g, h;
    g.lda = D;
    g.w = ly.ff.w1p; g.ldw = D;
    g.c = e->HD.p; g.ldc = e->inner_pad;
    g.M = L; g.N = 2 * e->inner_pad; g.K = D;
    g.flags = OMNITOK_GEMM_GEGLU;
    h.a = e->HD.p; h.lda = e->inner_pad;
    h.w = ly.ff.w2p; h.ldw = e->inner_pad;
    h.residual = e->X.p; h.ldr = D;
    h.c = e->X.p; h.ldc = D;
    h.M = L; h.N = D; h.K = e->inner_pad;
    h.flags = OMNITOK_GEMM_RESIDUAL;
    if (fused && x3_ok(e, 2 * e->inner_pad, D, OMNITOK_GEMM_GEGLU)) {
        OT_RUN("row_stats", L * D * 4.0, omnitok_row_stats(e->X.p, L, D, 1e-5f, e->ST.p, nullptr, 0, stream));
        g.a = e->X.p;
        g.ab = ABound{1.0f, nullptr, 0};
        g.ln_stats = e->ST.p; g.ln_g = ly.ff.lw; g.ln_b = ly.ff.lb;
        g.ln_cols = 2 * e->inner_pad; g.ln_bound = ly.ff.ln_bound;
        h.ab = ABound{ly.ff.h_bound, nullptr, 0};
    } else {
        OT_RUN("layernorm", 2.0 * L * D * 4.0, omnitok_layernorm(e->X.p, ly.ff.lw, ly.ff.lb, e->Y.p, L, D, 1e-5f, 0, 0, 0, stream));
        g.a = e->Y.p;
    }
    OT_RUN("gemm_ff_in", gemm_f * 2 * c.ff_inner, eg_gemm(e, g, stream));
    OT_RUN("gemm_ff_out", gemm_f * c.ff_inner, eg_gemm(e, h, stream));
    return OMNITOK_OK;
}

// the Transformer's final LayerNorm, with what follows it on the path fused into its store
int Run::norm_out(bool transpose_out, bool out_planes, const PreVqFuse *pv) {
    if (out_planes) {  // the consumer is a plane GEMM (to_pixels): LayerNorm + operand split in one pass, rows stay in place
        OT_RUN("layernorm", 2.0 * L * D * 4.0,
               omnitok_layernorm_planes(e->X.p, L, D, 1e-5f, tw.og, tw.ob, tw.out_bound, e->Y.p, pad256(L), stream));
        return OMNITOK_OK;
    }
    if (pv) {  // encoder end: LayerNorm -> pre_vq -> l2norm in one pass, z rows in the order the LayerNorm would have stored
        OT_RUN("pre_vq", 1.0 * L * D * 4.0,
               omnitok_layernorm_prevq(e->X.p, tw.og, tw.ob, pv->w, pv->b, pv->z, B, spatial ? T : S, spatial ? S : T, D, 1e-5f,
                                       transpose_out && T > 1, pv->l2, stream));
        return OMNITOK_OK;
    }
    if (transpose_out && T > 1)  // rows (b, t, s) -> (b, s, t) after a spatial stage, (b, s, t) -> (b, t, s) after a temporal one
        OT_RUN("layernorm", 2.0 * L * D * 4.0,
               omnitok_layernorm_transposed(e->X.p, tw.og, tw.ob, e->X2.p, B, spatial ? T : S, spatial ? S : T, D, 1e-5f, stream));
    else
        OT_RUN("layernorm", 2.0 * L * D * 4.0, omnitok_layernorm(e->X.p, tw.og, tw.ob, e->X2.p, L, D, 1e-5f, 0, 0, 0, stream));
    std::swap(e->X, e->X2);
    return OMNITOK_OK;
}

}  // namespace

// One Transformer (reference attention.py:655-689). X holds the tokens on entry and on exit.
// Pooling blocks shrink the token grid (attention.py:683-684): *ghp / *gwp are updated.
// transpose_out: the final LayerNorm stores its rows in the OTHER stage's token order ('(b t)(h w)' <-> '(b h w) t'),
// i.e. the rearrange that follows every Transformer on the path is fused into the norm_out store.
int run_transformer(omnitok_engine *e, const TransformerW &tw, int B, int T, int *ghp, int *gwp, bool spatial,
                    hipStream_t stream, bool transpose_out, bool out_planes, const PreVqFuse *pv) {
    Run r(e, tw, stream, B, T, spatial);
    r.set_grid(*ghp, *gwp);
    r.decide_flow();
    for (const Layer &ly : tw.layers) {
        r.ln_planes_ready = false;
        int rc;
        switch (ly.kind) {
            case 'a': case 'm': case 'l': rc = r.pool_block(ly); break;
            case 'n': case 'r': rc = r.up_block(ly); break;
            case 't': rc = r.temporal_block(ly); break;
            default: rc = r.window_block(ly); break;
        }
        if (rc) return rc;
        if (int rc2 = r.feed_forward(ly)) return rc2;
    }
    if (int rc = r.norm_out(transpose_out, out_planes, pv)) return rc;
    *ghp = r.gh;
    *gwp = r.gw;
    return OMNITOK_OK;
}

}  // namespace omnitok
