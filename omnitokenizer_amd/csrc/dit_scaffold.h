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
    unsigned short *w16qkv = nullptr, *w16proj = nullptr, *w16fc1 = nullptr, *w16fc2 = nullptr;  // inside DitLinear::image
};

struct DitSlots {
    std::map<std::string, DitSlot> slots;
    std::vector<std::string> order;  // the state_dict's order, for missing()
    bool changed = true;             // a weight was set since DitLinear built its image

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
        changed = true;
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
        static const struct { int bit; const char *what; } clauses[] = {
            {DIT_FLAG_T_RANGE, "a timestep outside [0, 1000)"},
            {DIT_FLAG_Y_RANGE, "a label outside the embedding table"},
            {DIT_FLAG_F16_RANGE, "an activation outside the fp16 range (linear format fp16: use bf16 or fp32)"},
            {DIT_FLAG_ATTN16_RANGE, "a q, k or v outside the fp16 range (attention format fp16: use bf16 or fp32)"}};
        std::string msg;
        for (const auto &c : clauses)
            if (bits & c.bit) msg += (msg.empty() ? "" : " and ") + std::string(c.what);
        set_error("%s_forward: %s", who, msg.c_str());
        return OMNITOK_ERR_INVALID;
    }

    void free_all() {
        if (t_table) (void)hipFree(t_table);
        if (flag) (void)hipFree(flag);
    }
};

// The linear format of an engine (omnitok_dit_set_linear_format) and, under a 16-bit one, the packed image of the four matrices of
// every block: attn.qkv | attn.proj | mlp.fc1 | mlp.fc2, block after block, rounded on the device by omnitok_dit_round16.  The fp32
// originals stay where DitSlots put them.
struct DitLinear {
    int fmt = OMNITOK_DIT_LIN_FP32;
    int built = OMNITOK_DIT_LIN_FP32;  // the format `image` holds; -1: none that can be used
    unsigned short *image = nullptr;
    int *wflags = nullptr;  // one range word per matrix

    int set(const char *who, int f, int D, int F) {
        OT_CHECK_ARG(f == OMNITOK_DIT_LIN_FP32 || f == OMNITOK_DIT_LIN_BF16 || f == OMNITOK_DIT_LIN_FP16,
                     "%s_set_linear_format: format %d (OMNITOK_DIT_LIN_FP32 | _BF16 | _FP16)", who, f);
        OT_CHECK_ARG(f == OMNITOK_DIT_LIN_FP32 || (D % 32 == 0 && F % 32 == 0),
                     "%s_set_linear_format: the 16-bit GEMM needs K %% 32 == 0, hidden is %d and mlp_hidden %d", who, D, F);
        fmt = f;
        return OMNITOK_OK;
    }

    int finalize(const char *who, DitSlots &slots, std::vector<DitBlock> &blocks, int64_t D, int64_t F, hipStream_t stream) {
        if (fmt == OMNITOK_DIT_LIN_FP32) {
            free_all();  // (hipFree synchronises: no earlier forward still reads the image)
            for (DitBlock &L : blocks) L.w16qkv = L.w16proj = L.w16fc1 = L.w16fc2 = nullptr;
            built = fmt;
            return OMNITOK_OK;
        }
        if (image && built == fmt && !slots.changed) return OMNITOK_OK;
        built = -1;
        const int64_t per = 4 * D * D + 2 * F * D;
        const int n = 4 * (int)blocks.size();
        if (!image) OT_HIP(hipMalloc(reinterpret_cast<void **>(&image), (size_t)per * blocks.size() * 2));
        if (!wflags) OT_HIP(hipMalloc(reinterpret_cast<void **>(&wflags), (size_t)n * 4));
        if (int rc = device_fill_u32(wflags, 0, n, stream)) return rc;
        for (size_t i = 0; i < blocks.size(); ++i) {
            DitBlock &L = blocks[i];
            L.w16qkv = image + (int64_t)i * per;
            L.w16proj = L.w16qkv + 3 * D * D;
            L.w16fc1 = L.w16proj + D * D;
            L.w16fc2 = L.w16fc1 + F * D;
            const float *src[4] = {L.wqkv, L.wproj, L.wfc1, L.wfc2};
            unsigned short *dst[4] = {L.w16qkv, L.w16proj, L.w16fc1, L.w16fc2};
            const int64_t count[4] = {3 * D * D, D * D, F * D, D * F};
            for (int k = 0; k < 4; ++k)
                if (int rc = omnitok_dit_round16(src[k], fmt, dst[k], count[k], wflags + 4 * i + k, stream)) return rc;
        }
        if (fmt == OMNITOK_DIT_LIN_FP16) {
            std::vector<int> host(n);
            OT_HIP(hipMemcpyAsync(host.data(), wflags, (size_t)n * 4, hipMemcpyDeviceToHost, stream));
            OT_HIP(hipStreamSynchronize(stream));
            static const char *const names[4] = {"attn.qkv.weight", "attn.proj.weight", "mlp.fc1.weight", "mlp.fc2.weight"};
            for (int k = 0; k < n; ++k)
                OT_CHECK_ARG(!host[k], "%s_finalize: blocks.%d.%s has an element outside the fp16 range (linear format fp16: use bf16 or fp32)",
                             who, k / 4, names[k % 4]);
        }
        built = fmt;
        slots.changed = false;
        return OMNITOK_OK;
    }

    void free_all() {
        if (image) (void)hipFree(image);
        if (wflags) (void)hipFree(wflags);
        image = nullptr;
        wflags = nullptr;
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
// rounded up to whole f32x4):  X, Xn, Y, A | qkv | fc1 | final linear | temb, h1, h2, c | mod.  Under a 16-bit linear format
// (lin16) there is no Y -- its M D floats hold the packed Xn16 | A16 -- and fc1's output is the packed H16, half the bytes.
inline int64_t dit_lin_floats(int64_t M, int64_t patch_out) { return (M * patch_out + 3) / 4 * 4; }
inline int64_t dit_work_floats(int64_t M, int64_t B, int64_t D, int64_t F, int64_t patch_out, int64_t modN, bool lin16) {
    return 4 * M * D + 3 * M * D + M * F / (lin16 ? 2 : 1) + dit_lin_floats(M, patch_out) + B * (DIT_T_FREQ + 3 * D) + B * modN;
}

// the pointers of that workspace
struct DitWork {
    float *X, *Xn, *Y, *A, *QKV, *H1, *LIN, *temb, *h1, *h2, *cs, *mod;
    unsigned short *Xn16 = nullptr, *A16 = nullptr, *H16 = nullptr;
    DitWork(void *base, int64_t M, int64_t B, int64_t D, int64_t F, int64_t patch_out, bool lin16) {
        X = static_cast<float *>(base);
        Xn = X + M * D;
        Y = Xn + M * D;
        A = Y + M * D;
        QKV = A + M * D;
        H1 = QKV + 3 * M * D;
        LIN = H1 + M * F / (lin16 ? 2 : 1);
        if (lin16) {
            Xn16 = reinterpret_cast<unsigned short *>(Y);
            A16 = Xn16 + M * D;
            H16 = reinterpret_cast<unsigned short *>(H1);
            Y = H1 = nullptr;
        }
        temb = LIN + dit_lin_floats(M, patch_out);
        h1 = temb + B * DIT_T_FREQ;
        h2 = h1 + B * D;
        cs = h2 + B * D;
        mod = cs + B * D;
    }
};

// The attention format of an engine (omnitok_dit_set_attention_format): the operands of the SPATIAL attention.  No weight image
// depends on it, so setting it does not touch `finalized`.
inline int dit_set_attention_format(const char *who, int *afmt, int f) {
    OT_CHECK_ARG(f == OMNITOK_DIT_ATTN_FP32 || f == OMNITOK_DIT_ATTN_BF16 || f == OMNITOK_DIT_ATTN_FP16,
                 "%s_set_attention_format: format %d (OMNITOK_DIT_ATTN_FP32 | _BF16 | _FP16)", who, f);
    *afmt = f;
    return OMNITOK_OK;
}

// The spatial attention of both engines over B sequences of N tokens, the callback dit_block takes: attention format fp32 is
// omnitok_dit_attn (a16 is never asked for: attn_packs is false); a 16-bit one omnitok_dit_attn16 into a32, or into a16 packed in
// the linear format lin_fmt.
inline int dit_spatial_attn(const float *qkv, int B, int N, int heads, int hd, int afmt, int lin_fmt, float *a32, unsigned short *a16,
                            int *flag, hipStream_t stream) {
    if (afmt == OMNITOK_DIT_ATTN_FP32) return omnitok_dit_attn(qkv, B, N, heads, hd, a32, stream);
    return omnitok_dit_attn16(qkv, B, N, heads, hd, afmt, a32, a16, lin_fmt, flag, stream);
}

// One transformer block in place on X [M, D] (M rows, n_tokens of them per sample), m = the block's 6 D modulation columns of `mod`
// (shift_msa | scale_msa | gate_msa | shift_mlp | scale_mlp | gate_mlp, rows modN apart); attn(QKV, a32, a16) is the caller's attention
// into exactly one of a32 (fp32) / a16 (packed in fmt).
// fmt: the engine's linear format; under a 16-bit one the four linears are omnitok_dit_gemm16 calls on the packed images L.w16*, each
// A operand rounded once where it is produced, gate_residual and GELU inside the epilogues; `flag` is the engine's range word.
// attn_packs (read under a 16-bit fmt only): the attention writes the packed A16 itself (dit_spatial_attn under a 16-bit attention
// format); else it writes fp32 and omnitok_dit_round16 runs behind it.
template <typename Attn>
inline int dit_block(const DitBlock &L, const DitWork &w, const float *m, int64_t modN, int64_t M, int n_tokens, int D, int F, Attn attn,
                     bool attn_packs, int fmt, int *flag, hipStream_t stream) {
#define DIT_RUN(call) \
    if (int rc_ = (call)) return rc_
    if (fmt != OMNITOK_DIT_LIN_FP32) {
        DIT_RUN(omnitok_dit_ln_modulate16(w.X, m, m + D, modN, M, n_tokens, D, fmt, w.Xn16, flag, stream));
        DIT_RUN(omnitok_dit_gemm16(w.Xn16, L.w16qkv, fmt, L.bqkv, OMNITOK_DIT_EPI_BIAS, w.QKV, nullptr, nullptr, 0, 0, nullptr, M, 3 * D, D,
                                   flag, stream));
        if (attn_packs) {
            DIT_RUN(attn(w.QKV, nullptr, w.A16));
        } else {
            DIT_RUN(attn(w.QKV, w.A, nullptr));
            DIT_RUN(omnitok_dit_round16(w.A, fmt, w.A16, M * D, flag, stream));
        }
        DIT_RUN(omnitok_dit_gemm16(w.A16, L.w16proj, fmt, L.bproj, OMNITOK_DIT_EPI_GATE_RESIDUAL, nullptr, nullptr, m + 2 * D, modN,
                                   n_tokens, w.X, M, D, D, flag, stream));
        DIT_RUN(omnitok_dit_ln_modulate16(w.X, m + 3 * D, m + 4 * D, modN, M, n_tokens, D, fmt, w.Xn16, flag, stream));
        DIT_RUN(omnitok_dit_gemm16(w.Xn16, L.w16fc1, fmt, L.bfc1, OMNITOK_DIT_EPI_GELU16, nullptr, w.H16, nullptr, 0, 0, nullptr, M, F, D,
                                   flag, stream));
        DIT_RUN(omnitok_dit_gemm16(w.H16, L.w16fc2, fmt, L.bfc2, OMNITOK_DIT_EPI_GATE_RESIDUAL, nullptr, nullptr, m + 5 * D, modN, n_tokens,
                                   w.X, M, D, F, flag, stream));
        return OMNITOK_OK;
    }
    DIT_RUN(omnitok_dit_ln_modulate(w.X, m, m + D, modN, M, n_tokens, D, w.Xn, stream));
    DIT_RUN(dit_linear(w.Xn, L.wqkv, L.bqkv, w.QKV, M, 3 * D, D, stream));
    DIT_RUN(attn(w.QKV, w.A, nullptr));
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
