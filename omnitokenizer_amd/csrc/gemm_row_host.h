// Host side shared by the entry points that take an omnitok_row_gemm (gemm.hip, gemm_x3.hip, gemm_h2.hip): the checks of the
// descriptor, the GemmParams fill, and for the two split-operand kernels the launch, the head of the tile choice and the flag
// dispatch.  `name` is the kernel's prefix in every message ("gemm", "gemm_x3", "gemm_h2").  No device code here.
#pragma once
#include "gemm_common.h"

namespace omnitok {

// a field that selects something the called kernel does not implement
#define OT_ROW_GEMM_REFUSE(name, d, field) \
    OT_CHECK_ARG(!(d)->field, "%s: " #field " is set, but this kernel does not implement it", name)

// What is checked before the M == 0 early return.  have_w: the kernel's weight operand is there.
inline int row_gemm_check_shape(const char *name, const omnitok_row_gemm &d, bool have_w) {
    OT_CHECK_ARG(d.a && have_w && d.c, "%s: null pointer", name);
    OT_CHECK_ARG(d.split_col == 0 || (d.c2 && d.split_col % 256 == 0 && d.split_col < d.N &&
                                      !(d.flags & (OMNITOK_GEMM_GEGLU | OMNITOK_GEMM_RESIDUAL))),
                 "%s: split output needs c2, split_col %% 256 == 0 and no GEGLU / residual epilogue", name);
    OT_CHECK_ARG(d.M >= 0 && d.N > 0 && d.K > 0, "%s: bad sizes M=%lld N=%d K=%d", name, (long long)d.M, d.N, d.K);
    return OMNITOK_OK;
}

// fp32 weight rows (gemm, x3): K and N granularity, alignment of both operands
inline int row_gemm_check_w_rows(const char *name, const omnitok_row_gemm &d, int n_multiple) {
    OT_CHECK_ARG(d.K % 32 == 0, "%s: K=%d must be a multiple of 32 (pad the weight)", name, d.K);
    OT_CHECK_ARG(d.N % n_multiple == 0, "%s: N=%d must be a multiple of %d", name, d.N, n_multiple);
    OT_CHECK_ARG(d.lda % 4 == 0 && d.ldw % 4 == 0 && aligned16(d.a) && aligned16(d.w),
                 "%s: operands must be 16-byte aligned with ld %% 4 == 0", name);
    return OMNITOK_OK;
}

// operands of the epilogue flags and of the fused LayerNorm (split kernels; h2 also needs the bound of |LN(a)|)
inline int row_gemm_check_options(const char *name, const omnitok_row_gemm &d, bool need_bound) {
    OT_CHECK_ARG(!(d.flags & OMNITOK_GEMM_BIAS) || d.bias, "%s: BIAS flag without bias", name);
    OT_CHECK_ARG(!(d.flags & OMNITOK_GEMM_RESIDUAL) || d.residual, "%s: RESIDUAL flag without residual", name);
    OT_CHECK_ARG(!d.ln_stats || (d.ln_gamma && d.K <= 512 && d.ln_cols > 0 && (!need_bound || d.ln_bound > 0.0f) &&
                                 (d.ln_cols >= d.N || d.ln_cols % 256 == 0)),
                 "%s: fused LayerNorm needs gamma,%s K <= 512 and ln_cols a multiple of 256 (or >= N)", name,
                 need_bound ? " a bound," : "");
    return OMNITOK_OK;
}

// gn: tile columns per column group of the tile order.  The tile counts are the launcher's.
inline GemmParams row_gemm_params(const omnitok_row_gemm &d, int gn) {
    GemmParams p{};
    p.a = d.a; p.w = d.w; p.bias = d.bias; p.residual = d.residual; p.c = d.c;
    p.lda = d.lda; p.ldw = d.ldw; p.ldr = d.ldr; p.ldc = d.ldc;
    p.M = d.M; p.N = d.N; p.K = d.K;
    p.a_rpg = d.a_rows_per_group; p.a_stride = d.a_group_stride; p.a_off = d.a_group_offset;
    p.gn = gn;
    return p;
}

// X3Params / H2Params: the GemmParams and what the two kernels name alike (fused LayerNorm, split output)
template <typename SplitParams>
void row_gemm_fill_split(SplitParams &sp, const omnitok_row_gemm &d, int gn) {
    sp.g = row_gemm_params(d, gn);
    sp.ln_stats = d.ln_stats; sp.ln_gamma = d.ln_gamma; sp.ln_beta = d.ln_beta; sp.ln_cols = d.ln_stats ? d.ln_cols : 0;
    sp.c2 = d.c2; sp.ldc2 = d.ldc2; sp.split_col = d.split_col;
}

// Tile id of a split kernel by how many tiles the problem offers per CU: 1 256x256, 3 128x128, 4 the small tile (every
// tile shape performs the same per-element arithmetic, so the choice never changes a result)
inline int split_auto_tile(const GemmParams &p, int n_cu) {
    auto tiles = [&](int tm, int tn) { return ((p.M + tm - 1) / tm) * (int64_t)((p.N + tn - 1) / tn); };
    if (tiles(256, 256) >= 2 * n_cu) return 1;
    return tiles(128, 128) >= n_cu ? 3 : 4;
}

// Persistent launch of KERNEL = gemm_{x3,h2}_kernel<FLAGS, C, LN>: at most 160 KiB of LDS per CU and two waves per SIMD
// (register budget of the kernels) decide the workgroups per CU
template <auto KERNEL, typename C, bool LN, typename SplitParams>
int launch_split_cfg(const char *name, SplitParams sp, int n_cu, hipStream_t stream) {
    GemmParams &p = sp.g;
    const int lds = 2 * C::STAGE + (LN ? C::LN_TAB : 0);
    if (int rc = set_max_dynamic_lds(reinterpret_cast<const void *>(KERNEL), lds)) return rc;
    const int64_t nbm = (p.M + C::TM - 1) / C::TM;
    const int nbn = (p.N + C::TN - 1) / C::TN;
    const int64_t nt = nbm * nbn;
    OT_CHECK_ARG(nt < (1ll << 31), "%s: grid too large", name);
    p.nbm = (int)nbm;
    p.nbn = nbn;
    p.ntiles = (int)nt;
    int wg_per_cu = (160 * 1024) / lds;
    const int by_waves = 8 / (C::NT / 64);
    if (wg_per_cu > by_waves) wg_per_cu = by_waves;
    if (wg_per_cu < 1) wg_per_cu = 1;
    const int64_t cap = (int64_t)n_cu * wg_per_cu;
    const int grid = (int)(nt < cap ? nt : cap);
    hipLaunchKernelGGL(KERNEL, dim3(grid), dim3(C::NT), lds, stream, sp);
    OT_LAUNCH_CHECK(name);
    return OMNITOK_OK;
}

// Epilogue flags of a split kernel -> LAUNCH<FLAGS, LN>(params, stream); returns from the calling function
#define OT_SPLIT_CASE(F, LAUNCH, params, ln, stream) \
    case F:                                          \
        return (ln) ? LAUNCH<F, true>(params, stream) : LAUNCH<F, false>(params, stream);
#define OT_SPLIT_DISPATCH(name, LAUNCH, params, d, ln, stream)                                               \
    switch ((d)->flags) {                                                                                    \
        OT_SPLIT_CASE(0, LAUNCH, params, ln, stream)                                                         \
        OT_SPLIT_CASE(OMNITOK_GEMM_BIAS, LAUNCH, params, ln, stream)                                         \
        OT_SPLIT_CASE(OMNITOK_GEMM_RESIDUAL, LAUNCH, params, ln, stream)                                     \
        OT_SPLIT_CASE(OMNITOK_GEMM_BIAS | OMNITOK_GEMM_RESIDUAL, LAUNCH, params, ln, stream)                 \
        case OMNITOK_GEMM_GEGLU:                                                                             \
            OT_CHECK_ARG((d)->N % 64 == 0, "%s: GEGLU packed width %d must be a multiple of 64", name, (d)->N); \
            return (ln) ? LAUNCH<OMNITOK_GEMM_GEGLU, true>(params, stream)                                   \
                        : LAUNCH<OMNITOK_GEMM_GEGLU, false>(params, stream);                                 \
        default:                                                                                             \
            set_error("%s: unsupported epilogue flags %d", name, (d)->flags);                                \
            return OMNITOK_ERR_INVALID;                                                                      \
    }

}  // namespace omnitok
