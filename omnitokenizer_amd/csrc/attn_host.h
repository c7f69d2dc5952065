// Host side shared by the entry points that take an omnitok_attn_desc (attn_spatial.hip, attn_h2.hip, attn_temporal.hip): the
// checks that more than one kernel makes; `name` is the entry point's prefix in every message ("qk_prep", "attn_spatial_h2").
// Rules of one kernel (token multiples, the 8 x 8 window, what a plane output needs) stay in its file.  No device code here.
#pragma once
#include "common.h"

namespace omnitok {

enum AttnFields : unsigned {  // field groups of the descriptor: what an entry point refuses, requires or wants aligned
    AF_Q = 1, AF_K = 2, AF_V = 4,                  // q + ldq, k + ldkv, v
    AF_QKP = 8, AF_VP = 16,                        // qp + kp, vp
    AF_ROPE = 32, AF_SCALES = 64,                  // rope_cos + rope_sin, q_scale + k_scale
    AF_V_BOUND_DEV = 128, AF_BIAS_TABLE = 256, AF_BIAS_DENSE = 512,
    AF_TEMPORAL = 1024,                            // alibi_slopes, causal
    AF_OUT = 2048, AF_OUT_PLANES = 4096,           // out + ldo (as a requirement: out or out_planes), out_planes
    AF_ROWS = AF_Q | AF_K | AF_V, AF_PLANES = AF_QKP | AF_VP,
};

// NULL descriptor; a field of the groups `refused` that selects something the called kernel does not implement
inline int attn_check_desc(const char *name, const omnitok_attn_desc *d, unsigned refused) {
    OT_CHECK_ARG(d, "%s: null descriptor", name);
    const struct { unsigned group; bool set; const char *field; } fields[] = {
        {AF_Q, d->q != nullptr, "q"}, {AF_K, d->k != nullptr, "k"}, {AF_V, d->v != nullptr, "v"},
        {AF_QKP, d->qp != nullptr, "qp"}, {AF_QKP, d->kp != nullptr, "kp"}, {AF_VP, d->vp != nullptr, "vp"},
        {AF_ROPE, d->rope_cos != nullptr, "rope_cos"}, {AF_ROPE, d->rope_sin != nullptr, "rope_sin"},
        {AF_V_BOUND_DEV, d->v_bound_dev != nullptr, "v_bound_dev"}, {AF_BIAS_TABLE, d->bias_table != nullptr, "bias_table"},
        {AF_BIAS_DENSE, d->bias_dense != nullptr, "bias_dense"}, {AF_TEMPORAL, d->alibi_slopes != nullptr, "alibi_slopes"},
        {AF_TEMPORAL, d->causal != 0, "causal"}, {AF_OUT, d->out != nullptr, "out"},
        {AF_OUT_PLANES, d->out_planes != nullptr, "out_planes"}};
    for (const auto &f : fields)
        OT_CHECK_ARG(!((refused & f.group) && f.set), "%s: %s is set, but this kernel does not implement it", name, f.field);
    return OMNITOK_OK;
}

// The operands of the groups `need` are there; they and those of `optional` (absent = fine) are 16-byte aligned with
// ld % 4 == 0 (the ld of an fp32 output that the plane output replaces is not looked at); AF_ROPE: cos and sin come as a pair
inline int attn_check_operands(const char *name, const omnitok_attn_desc &d, unsigned need, unsigned optional = 0) {
    const auto ok = [](unsigned groups, unsigned group, bool fine) { return !(groups & group) || fine; };
    OT_CHECK_ARG(ok(need, AF_Q, d.q) && ok(need, AF_K, d.k) && ok(need, AF_V, d.v) && ok(need, AF_QKP, d.qp && d.kp) &&
                     ok(need, AF_VP, d.vp) && ok(need, AF_SCALES, d.q_scale && d.k_scale) && ok(need, AF_BIAS_DENSE, d.bias_dense) &&
                     ok(need, AF_OUT, d.out || d.out_planes),
                 "%s: null pointer", name);
    OT_CHECK_ARG(ok(optional, AF_ROPE, (d.rope_cos == nullptr) == (d.rope_sin == nullptr)),
                 "%s: cos/sin must both be given or both null", name);
    const unsigned al = need | optional;
    OT_CHECK_ARG(ok(al, AF_Q, d.ldq % 4 == 0 && aligned16(d.q)) && ok(al, AF_K, d.ldkv % 4 == 0 && aligned16(d.k)) &&
                     ok(al, AF_V, aligned16(d.v)) && ok(al, AF_QKP, aligned16(d.qp) && aligned16(d.kp)) && ok(al, AF_VP, aligned16(d.vp)) &&
                     ok(al, AF_OUT, (d.out_planes || d.ldo % 4 == 0) && aligned16(d.out)),
                 "%s: unaligned", name);
    return OMNITOK_OK;
}

// ranges behind the operand scales; per-clip ranges need the clip length (`clip_rule`: its wording there, nullptr = dev refused)
inline int attn_check_ranges(const char *name, const omnitok_attn_desc &d, bool need_v, const char *clip_rule) {
    OT_CHECK_ARG(d.q_bound > 0.0f && d.k_bound > 0.0f && (!need_v || d.v_bound > 0.0f), "%s: operand bounds must be positive", name);
    OT_CHECK_ARG(!clip_rule || !d.v_bound_dev || d.seqs_per_clip > 0, "%s: %s", name, clip_rule);
    return OMNITOK_OK;
}
// sequences that share one v_bound_dev slot (without per-clip ranges: all of them)
inline int64_t attn_clip_seqs(const omnitok_attn_desc &d) { return d.v_bound_dev ? d.seqs_per_clip : (d.seqs > 0 ? d.seqs : 1); }

}  // namespace omnitok
