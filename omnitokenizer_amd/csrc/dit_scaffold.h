// Host-side scaffold the DiT engine (dit_engine.hip) and the Latte engine (latte_engine.hip) share: the table of named weight
// slots behind set_weight / missing / finalize, the device timestep table, the grow-only workspace and the one GEMM call.
// `who` is the prefix of the caller's error messages ("dit" / "latte").
#pragma once
#include "dit_common.h"

#include <cmath>
#include <map>
#include <string>
#include <vector>

namespace omnitok {

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

struct DitSlots {
    std::map<std::string, DitSlot> slots;
    std::vector<std::string> order;  // the state_dict's order, for missing()

    void add(const std::string &name, std::vector<int64_t> shape, float **dst, int64_t offset = 0, int64_t alloc = 0) {
        int64_t n = 1;
        for (auto s : shape) n *= s;
        slots[name] = DitSlot{std::move(shape), dst, offset, alloc ? alloc : n};
        order.push_back(name);
    }

    // the transformer blocks and the final layer, the part of the key list DiT and Latte have in common
    void add_blocks(std::vector<DitBlock> &blocks, int64_t D, int64_t F, int64_t final_out, float **w_mod, float **b_mod, int64_t modN,
                    float **w_final, float **b_final) {
        const int depth = (int)blocks.size();
        for (int i = 0; i < depth; ++i) {
            const std::string b = "blocks." + std::to_string(i);
            DitBlock &L = blocks[i];
            add(b + ".attn.qkv.weight", {3 * D, D}, &L.wqkv);
            add(b + ".attn.qkv.bias", {3 * D}, &L.bqkv);
            add(b + ".attn.proj.weight", {D, D}, &L.wproj);
            add(b + ".attn.proj.bias", {D}, &L.bproj);
            add(b + ".mlp.fc1.weight", {F, D}, &L.wfc1);
            add(b + ".mlp.fc1.bias", {F}, &L.bfc1);
            add(b + ".mlp.fc2.weight", {D, F}, &L.wfc2);
            add(b + ".mlp.fc2.bias", {D}, &L.bfc2);
            add(b + ".adaLN_modulation.1.weight", {6 * D, D}, w_mod, (int64_t)i * 6 * D * D, modN * D);
            add(b + ".adaLN_modulation.1.bias", {6 * D}, b_mod, (int64_t)i * 6 * D, modN);
        }
        add("final_layer.linear.weight", {final_out, D}, w_final);
        add("final_layer.linear.bias", {final_out}, b_final);
        add("final_layer.adaLN_modulation.1.weight", {2 * D, D}, w_mod, (int64_t)depth * 6 * D * D, modN * D);
        add("final_layer.adaLN_modulation.1.bias", {2 * D}, b_mod, (int64_t)depth * 6 * D, modN);
    }

    void free_all() {
        for (auto &kv : slots)
            if (*kv.second.dst) {
                (void)hipFree(*kv.second.dst);
                *kv.second.dst = nullptr;  // (the adaLN slots share two buffers)
            }
    }

    int set_weight(const char *who, const char *name, const void *dev_ptr, const int64_t *shape, int ndim, hipStream_t stream) {
        auto it = slots.find(name);
        if (it == slots.end()) return 1;
        DitSlot &s = it->second;
        const std::vector<int64_t> shp(shape, shape + ndim);
        if (shp != s.shape) {
            std::string want, got;
            for (auto v : s.shape) want += std::to_string(v) + ",";
            for (auto v : shp) got += std::to_string(v) + ",";
            set_error("%s_set_weight: size mismatch for %s: expected [%s] got [%s]", who, name, want.c_str(), got.c_str());
            return OMNITOK_ERR_INVALID;
        }
        int64_t n = 1;
        for (auto v : shp) n *= v;
        if (!*s.dst) OT_HIP(hipMalloc(reinterpret_cast<void **>(s.dst), (size_t)s.alloc * 4));
        OT_HIP(hipMemcpyAsync(*s.dst + s.offset, dev_ptr, (size_t)n * 4, hipMemcpyDeviceToDevice, stream));
        s.set = true;
        return OMNITOK_OK;
    }

    int missing(char *buf, int cap) {
        int count = 0;
        size_t used = 0;
        if (cap > 0) buf[0] = 0;
        for (const std::string &name : order) {
            if (slots[name].set) continue;
            ++count;
            if (used + name.size() + 2 <= (size_t)cap) {
                if (used) buf[used++] = '\n';
                used += name.copy(buf + used, name.size());
                buf[used] = 0;
            }
        }
        return count;
    }

    // OMNITOK_ERR_STATE naming the first weight not set yet
    int require_all(const char *who) {
        for (const std::string &name : order)
            if (!slots[name].set) {
                set_error("%s_finalize: missing weight %s", who, name.c_str());
                return OMNITOK_ERR_STATE;
            }
        return OMNITOK_OK;
    }
};

// The range word and the timestep table an engine gathers from (omnitok_dit_timestep_table with the caller's frequencies, or the
// built-in chain when `freqs` is empty), uploaded once per set of frequencies.
struct DitTables {
    float *t_table = nullptr;
    std::vector<float> freqs;
    bool table_built = false;
    int *flag = nullptr;

    int set_frequencies(const char *who, const float *f, int n) {
        OT_CHECK_ARG(f, "%s_set_frequencies: null pointer", who);
        OT_CHECK_ARG(n == DIT_T_FREQ / 2, "%s_set_frequencies: n %d (the model has %d frequencies)", who, n, DIT_T_FREQ / 2);
        for (int i = 0; i < n; ++i) OT_CHECK_ARG(std::isfinite(f[i]), "%s_set_frequencies: frequency %d is not finite", who, i);
        freqs.assign(f, f + n);
        table_built = false;
        return OMNITOK_OK;
    }

    int finalize(hipStream_t stream) {
        if (!table_built) {
            std::vector<float> host((size_t)DIT_T_STEPS * DIT_T_FREQ);
            if (int rc = omnitok_dit_timestep_table(freqs.empty() ? nullptr : freqs.data(), host.data())) return rc;
            if (!t_table) OT_HIP(hipMalloc(reinterpret_cast<void **>(&t_table), host.size() * 4));
            OT_HIP(hipStreamSynchronize(stream));  // no earlier forward still reads the table
            OT_HIP(hipMemcpy(t_table, host.data(), host.size() * 4, hipMemcpyHostToDevice));
            table_built = true;
        }
        if (!flag) {
            OT_HIP(hipMalloc(reinterpret_cast<void **>(&flag), 4));
            if (int rc = device_fill_u32(flag, 0, 1, stream)) return rc;
        }
        return OMNITOK_OK;
    }

    // synchronises the stream; OMNITOK_ERR_INVALID with the reason if a forward since the last check clamped a t or a y
    int check(const char *who, hipStream_t stream) {
        if (!flag) return OMNITOK_OK;  // nothing ran yet
        int bits = 0;
        OT_HIP(hipMemcpyAsync(&bits, flag, 4, hipMemcpyDeviceToHost, stream));
        OT_HIP(hipStreamSynchronize(stream));
        if (!bits) return OMNITOK_OK;
        if (int rc = device_fill_u32(flag, 0, 1, stream)) return rc;
        set_error("%s_forward: %s%s%s", who, bits & DIT_FLAG_T_RANGE ? "a timestep outside [0, 1000)" : "",
                  (bits & DIT_FLAG_T_RANGE) && (bits & DIT_FLAG_Y_RANGE) ? " and " : "",
                  bits & DIT_FLAG_Y_RANGE ? "a label outside the embedding table" : "");
        return OMNITOK_ERR_INVALID;
    }

    void free_all() {
        if (t_table) (void)hipFree(t_table);
        if (flag) (void)hipFree(flag);
    }
};

// grow-only device workspace
inline int dit_grow(void **p, int64_t *have, int64_t need_bytes) {
    if (*have >= need_bytes) return OMNITOK_OK;
    if (*p) OT_HIP(hipFree(*p));  // (synchronises: no earlier call still uses it)
    *p = nullptr;
    *have = 0;
    OT_HIP(hipMalloc(p, (size_t)need_bytes));
    *have = need_bytes;
    return OMNITOK_OK;
}

inline int dit_linear(const float *a, const float *w, const float *bias, float *c, int64_t M, int N, int K, hipStream_t stream) {
    omnitok_row_gemm g{};
    g.a = a; g.lda = K; g.w = w; g.ldw = K; g.bias = bias; g.c = c; g.ldc = N;
    g.M = M; g.N = N; g.K = K; g.flags = OMNITOK_GEMM_BIAS;
    return omnitok_gemm(&g, stream);
}

// floats of one forward's workspace over M token rows of B samples (D hidden, F mlp hidden, lin_floats the final linear's output
// rounded up to whole f32x4):  X, Xn, Y, A | qkv | fc1 | final linear | temb, h1, h2, c | mod
inline int64_t dit_lin_floats(int64_t M, int64_t patch_out) { return (M * patch_out + 3) / 4 * 4; }
inline int64_t dit_work_floats(int64_t M, int64_t B, int64_t D, int64_t F, int64_t patch_out, int64_t modN) {
    return 4 * M * D + 3 * M * D + M * F + dit_lin_floats(M, patch_out) + B * (DIT_T_FREQ + 3 * D) + B * modN;
}

// the pointers of that workspace
struct DitWork {
    float *X, *Xn, *Y, *A, *QKV, *H1, *LIN, *temb, *h1, *h2, *cs, *mod;
    DitWork(void *base, int64_t M, int64_t B, int64_t D, int64_t F, int64_t patch_out) {
        X = static_cast<float *>(base);
        Xn = X + M * D;
        Y = Xn + M * D;
        A = Y + M * D;
        QKV = A + M * D;
        H1 = QKV + 3 * M * D;
        LIN = H1 + M * F;
        temb = LIN + dit_lin_floats(M, patch_out);
        h1 = temb + B * DIT_T_FREQ;
        h2 = h1 + B * D;
        cs = h2 + B * D;
        mod = cs + B * D;
    }
};

// One transformer block in place on X [M, D] (M rows, n_tokens of them per sample), m = the block's 6 D modulation columns of `mod`
// (shift_msa | scale_msa | gate_msa | shift_mlp | scale_mlp | gate_mlp, rows modN apart); attn(QKV, A) is the caller's attention.
template <typename Attn>
inline int dit_block(const DitBlock &L, const DitWork &w, const float *m, int64_t modN, int64_t M, int n_tokens, int D, int F, Attn attn,
                     hipStream_t stream) {
#define DIT_RUN(call) \
    if (int rc_ = (call)) return rc_
    DIT_RUN(omnitok_dit_ln_modulate(w.X, m, m + D, modN, M, n_tokens, D, w.Xn, stream));
    DIT_RUN(dit_linear(w.Xn, L.wqkv, L.bqkv, w.QKV, M, 3 * D, D, stream));
    DIT_RUN(attn(w.QKV, w.A));
    DIT_RUN(dit_linear(w.A, L.wproj, L.bproj, w.Y, M, D, D, stream));
    DIT_RUN(omnitok_dit_gate_residual(w.X, w.Y, m + 2 * D, modN, M, n_tokens, D, stream));
    DIT_RUN(omnitok_dit_ln_modulate(w.X, m + 3 * D, m + 4 * D, modN, M, n_tokens, D, w.Xn, stream));
    DIT_RUN(dit_linear(w.Xn, L.wfc1, L.bfc1, w.H1, M, F, D, stream));
    DIT_RUN(omnitok_dit_gelu_tanh(w.H1, M * F, stream));
    DIT_RUN(dit_linear(w.H1, L.wfc2, L.bfc2, w.Y, M, D, F, stream));
    DIT_RUN(omnitok_dit_gate_residual(w.X, w.Y, m + 5 * D, modN, M, n_tokens, D, stream));
#undef DIT_RUN
    return OMNITOK_OK;
}

// The conditioning of B samples: table[t] -> Linear -> SiLU -> Linear, (+ label row if ytable), SiLU -> cs [B, D], then ONE GEMM
// over the concatenated adaLN_modulation.1 weights -> mod [B, modN].
inline int dit_conditioning(const char *who, const DitTables &tb, const float *w_t0, const float *b_t0, const float *w_t2, const float *b_t2,
                            const float *ytable, int y_rows, const float *w_mod, const float *b_mod, int64_t modN, const int64_t *t,
                            const int64_t *y, int B, int D, const DitWork &w, hipStream_t stream) {
#define DIT_RUN(call) \
    if (int rc_ = (call)) return rc_
    DIT_RUN(dit_cond_gather(tb.t_table, t, B, w.temb, tb.flag, stream));
    DIT_RUN(dit_linear(w.temb, w_t0, b_t0, w.h1, B, D, DIT_T_FREQ, stream));
    DIT_RUN(dit_silu(w.h1, (int64_t)B * D, stream));
    DIT_RUN(dit_linear(w.h1, w_t2, b_t2, w.h2, B, D, D, stream));
    DIT_RUN(dit_cond_combine(w.h2, ytable, y_rows, y, B, D, w.cs, tb.flag, stream));
    OT_CHECK_ARG(modN < (1ll << 31), "%s: depth * 6 * hidden + 2 * hidden = %lld does not fit the GEMM's N", who, (long long)modN);
    DIT_RUN(dit_linear(w.cs, w_mod, b_mod, w.mod, B, (int)modN, D, stream));
#undef DIT_RUN
    return OMNITOK_OK;
}

}  // namespace omnitok
