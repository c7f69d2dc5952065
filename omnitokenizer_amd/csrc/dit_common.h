// DiT denoiser (include/omnitok_dit.h): the class-conditional diffusion transformer of the reference's image-generation
// pipeline (Diffusion/DiT/models.py:145-266) and the per-step update of its ancestral sampler
// (Diffusion/DiT/diffusion/gaussian_diffusion.py:254-417).
//
// Which unit holds what:
//   dit_common.h   the constants the units share and the flag bits of the engine's range word
//   dit_ops.hip    the small kernels: patch_embed (+ pos_embed), the conditioning's gather / SiLU passes, ln_modulate, gelu_tanh,
//                  gate_residual, unpatchify, the classifier-free-guidance blend and p_sample, with their exported entry points
//   dit_attn.hip   dit_attn_kernel: non-causal attention on v_mfma_f32_32x32x2_f32, head_dim 64 and 72 (omnitok_dit_attn);
//                  dit_attn16_kernel: the same with bf16 / fp16 operands on v_mfma_f32_32x32x16_{bf16,f16}, fp32 or packed 16-bit output
//                  (omnitok_dit_attn16; the engines' attention format, omnitok_dit_set_attention_format)
//   attn_f32_tiled.h  (not the DiT's alone) the body of dit_attn_kernel, shared with the LM's tiled causal prefill attention
//   attn16_tiled.h    the body of dit_attn16_kernel, and the pa16_* helpers it shares with the LM's 16-bit prefill attention
//   dit_gemm16.hip dit_gemm16_kernel: the block linears of a 16-bit linear format (omnitok_dit_set_linear_format) on
//                  v_mfma_f32_32x32x16_{bf16,f16}, the K loop of csrc/gemm16_tile.h with the DiT's three epilogues (omnitok_dit_gemm16)
//   dit_engine.hip struct omnitok_dit and its exported functions (create .. finalize, forward, forward_cfg)
//   dit_scaffold.h the engine's host-side scaffold (weight slots, timestep table, workspace, one block, the conditioning), shared
//                  with the Latte video denoiser (latte_engine.hip, index: latte_common.h)
// The linears (qkv, proj, fc1, fc2, the conditioning MLP, the modulation GEMM and the final linear) are omnitok_gemm calls; under a
// 16-bit linear format the four of a block are omnitok_dit_gemm16 calls on operands rounded once where they are produced
// (omnitok_dit_ln_modulate16, omnitok_dit_round16 behind the attention, the fc1 epilogue).  Under a 16-bit attention format the
// spatial attention is omnitok_dit_attn16; with both it writes the packed operand of attn.proj itself and the round16 pass is not run.
#pragma once
#include "common.h"
#include "lm_common.h"  // lm_bf16, lm_fp16, lm_round16: the 16-bit element types and their one conversion
#include "../../include/omnitok_dit.h"

namespace omnitok {

constexpr int DIT_T_STEPS = 1000;  // timesteps of the table: t in [0, 1000)
constexpr int DIT_T_FREQ = 256;    // frequency_embedding_size of TimestepEmbedder (models.py:31)
constexpr int DIT_FLAG_T_RANGE = 1;  // bits of the engine's range word (omnitok_dit_check)
constexpr int DIT_FLAG_Y_RANGE = 2;
constexpr int DIT_FLAG_F16_RANGE = 4;  // an activation of an fp16 linear format rounded from a finite value to +-inf
constexpr int DIT_FLAG_ATTN16_RANGE = 8;  // a q, k or v of an fp16 attention format rounded from a finite value to +-inf

#ifdef __HIPCC__
// nn.GELU(approximate="tanh"): 0.5 x (1 + tanh(sqrt(2 / pi) (x + 0.044715 x^3))) -- dit_gelu_tanh_kernel and the fc1 epilogue of
// dit_gemm16_kernel
__device__ __forceinline__ float dit_gelu_tanh_f(float v) {
    const float inner = 0.7978845608028654f * (v + 0.044715f * v * v * v);
    return 0.5f * v * (1.0f + tanhf(inner));
}

// One value / four consecutive values rounded to OT = lm_bf16 | lm_fp16 (lm_round16: the bits of tensor.to(dtype)); `inf` records a
// FINITE value that became +-inf, which only fp16 can do.
template <typename OT> __device__ __forceinline__ unsigned short dit_round16(float f, bool &inf) {
    const unsigned short h = lm_round16<OT>(f);
    if constexpr (__is_same(OT, lm_fp16)) inf = inf || (lm_f16_is_inf(h) && fabsf(f) <= 3.402823466e38f);
    return h;
}
template <typename OT> __device__ __forceinline__ u32x2 dit_round16x4(const f32x4 &v, bool &inf) {
    unsigned short h[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float f = v[e];
        h[e] = dit_round16<OT>(f, inf);
    }
    return u32x2{(unsigned)h[0] | ((unsigned)h[1] << 16), (unsigned)h[2] | ((unsigned)h[3] << 16)};
}
#endif

// dit_ops.hip: the conditioning's element-wise steps (rows of D floats, one per sample)
//   temb[b, :] = table[clamp(t[b])][:]                       (DIT_T_FREQ floats; raises DIT_FLAG_T_RANGE)
//   x = silu(x)                                              in place
//   c[b, :] = silu(temb2[b, :] + ytable[clamp(y[b])][:])     (raises DIT_FLAG_Y_RANGE); ytable == nullptr (a model without labels,
//                                                            Latte's extras == 1): c[b, :] = silu(temb2[b, :]), y is not read
int dit_cond_gather(const float *table, const int64_t *t, int B, float *temb, int *flag, hipStream_t stream);
int dit_silu(float *x, int64_t n, hipStream_t stream);
int dit_cond_combine(const float *temb2, const float *ytable, int y_rows, const int64_t *y, int B, int D, float *c, int *flag,
                     hipStream_t stream);
// out [B, Cout, HW]: channels [0, min(channels, Cout)) of both halves <- uncond + s * (cond - uncond), in place (the DiT guides 3
// channels, Latte 4 of every frame: the literals of models.py:262 and latte.py:399)
int dit_cfg_blend(float *out, int B, int Cout, int channels, int64_t HW, float s, hipStream_t stream);

}  // namespace omnitok
