// Error reporting shared by all C-ABI entry points.
#include "common.h"
#include "../../include/omnitok_debug.h"
#include <limits.h>
#include <string.h>

namespace omnitok {
static thread_local char g_err[1024] = "";

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
}  // namespace omnitok

#include <map>
#include <mutex>
#include <utility>

namespace omnitok {
static std::mutex g_attr_mu;
static std::map<std::pair<const void *, int>, int> g_attr_bytes;
static std::map<int, int> g_dev_cus;

int set_max_dynamic_lds(const void *kernel, int bytes) {
    int dev = 0;
    OT_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_attr_mu);
    int &have = g_attr_bytes[std::make_pair(kernel, dev)];
    if (bytes > have) {
        OT_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
        have = bytes;
    }
    return OMNITOK_OK;
}

int current_device_cus(int *n_cu) {
    int dev = 0;
    OT_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_attr_mu);
    auto it = g_dev_cus.find(dev);
    if (it == g_dev_cus.end()) {
        int n = 0;
        OT_HIP(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
        it = g_dev_cus.emplace(dev, n).first;
    }
    *n_cu = it->second;
    return OMNITOK_OK;
}
}  // namespace omnitok

// Process options, one row each: X(name, readable through omnitok_get_option, smallest value accepted).  The variable is
// omnitok::g_<name>, defined next to the code that reads it.  omnitok_set_option and omnitok_get_option both walk this table.
#define OT_OPTIONS(X)                   \
    X(gemm_variant, false, INT_MIN)     \
    X(gemm_lds_pad_kb, false, INT_MIN)  \
    X(gemm_gn, false, INT_MIN)          \
    X(gemm_small, false, INT_MIN)       \
    X(vq_split, false, INT_MIN)         \
    X(vq_screen, false, INT_MIN)        \
    X(vq_screen_split, false, INT_MIN)  \
    X(x3_tile, false, INT_MIN)          \
    X(h2_tile, false, INT_MIN)          \
    X(peg_variant, false, INT_MIN)      \
    X(gemm_mode, true, INT_MIN)         \
    X(attn_mode, true, INT_MIN)         \
    X(attn_h2_variant, false, INT_MIN)  \
    X(attn_vpack, false, INT_MIN)       \
    X(attn_window_mode, false, INT_MIN) \
    X(gemm_pl, true, INT_MIN)           \
    X(qkv_pl, false, INT_MIN)           \
    X(pl_min_tokens, true, INT_MIN)     \
    X(pl_cfg, true, INT_MIN)            \
    X(pl_tail, true, INT_MIN)           \
    X(pl_stagger, false, INT_MIN)       \
    X(sp_small_blocks, true, INT_MIN)   \
    X(temporal_chunk, true, INT_MIN)    \
    X(temporal_fused, false, INT_MIN)   \
    X(temporal_kernel, false, INT_MIN)  \
    X(prevq_fuse, true, INT_MIN)        \
    X(lm_wide_u, true, INT_MIN)         \
    X(lm_balance, true, INT_MIN)        \
    X(lm_ksliced, true, INT_MIN)        \
    X(lm_mfma, true, INT_MIN)           \
    X(lm_mfma_mult, true, INT_MIN)      \
    X(lm_ks_deep, true, INT_MIN)        \
    X(lm_attn_short, true, INT_MIN)     \
    X(lm_attn_waves, true, INT_MIN)     \
    X(lm_streams_min, true, 1)          \
    X(lm_loss_chunk_rows, true, 1)

namespace omnitok {
extern long long *g_gemm_trace;
void lm_trace_reset();
#define OT_OPTION_DECL(name, readable, min) extern int g_##name;
OT_OPTIONS(OT_OPTION_DECL)
#undef OT_OPTION_DECL

struct Option {
    const char *name;
    int *value;
    bool readable;
    int min;
};
#define OT_OPTION_ROW(name, readable, min) {#name, &g_##name, readable, min},
static const Option g_options[] = {OT_OPTIONS(OT_OPTION_ROW)};
#undef OT_OPTION_ROW

static const Option *find_option(const char *name) {
    for (const Option &o : g_options)
        if (!strcmp(name, o.name)) return &o;
    return nullptr;
}
}  // namespace omnitok

extern "C" int omnitok_set_option(const char *name, int value) {
    if (!name) return OMNITOK_ERR_INVALID;
    const omnitok::Option *o = omnitok::find_option(name);
    if (!o) {
        omnitok::set_error("set_option: unknown option %s", name);
        return OMNITOK_ERR_INVALID;
    }
    OT_CHECK_ARG(value >= o->min, "set_option: %s %d, expected at least %d", name, value, o->min);
    *o->value = value;
    return OMNITOK_OK;
}

// current process default of a data-flow option (what an engine follows unless omnitok_engine_set_option pinned its own)
extern "C" int omnitok_get_option(const char *name, int *value) {
    if (!name || !value) return OMNITOK_ERR_INVALID;
    const omnitok::Option *o = omnitok::find_option(name);
    if (!o || !o->readable) {
        omnitok::set_error("get_option: %s is not a readable option", name);
        return OMNITOK_ERR_INVALID;
    }
    *value = *o->value;
    return OMNITOK_OK;
}

extern "C" int omnitok_debug_set_gemm_trace(long long *dev_ptr) {
    omnitok::g_gemm_trace = dev_ptr;
    omnitok::lm_trace_reset();
    return OMNITOK_OK;
}

extern "C" const char *omnitok_last_error(void) { return omnitok::g_err; }
extern "C" const char *omnitok_version(void) { return "omnitok 0.1 gfx950 fp32-mfma"; }
