/* omnitok_dit.h -- C ABI of the DiT denoiser, the second downstream consumer of the tokenizer's latents.
 *
 * The reference's image-generation pipeline samples a class-conditional DiT on the `--use_vae` tokenizer's latents
 * (Diffusion/DiT/models.py:145-266, sample.py, sample_ddp.py) with the ancestral sampler of
 * Diffusion/DiT/diffusion/gaussian_diffusion.py:376-417.  This library runs the model's forward pass and the per-step update
 * of the sampler on the device; omnitokenizer_amd/dit.py and omnitokenizer_amd/diffusion.py are the ctypes bindings that
 * mirror the reference's `DiT` class and `create_diffusion`.
 *
 * Same conventions as omnitok_lm.h: device pointers, fp32 (timesteps and labels int64), row-major, every launch on the given
 * stream, 0 = OK, argument errors are returned before any HIP call, omnitok_last_error holds the message.
 *
 * Arithmetic is fp32 throughout (the default; omnitok_dit_set_linear_format below opts the block linears into 16-bit operands,
 * omnitok_dit_set_attention_format the attention):
 * the linears run on the fp32-in row GEMM of omnitok.h (fp32 accumulate on v_mfma_f32_32x32x2_f32), the
 * attention on the same instruction, everything else on the VALU.  Results do not depend on the batch: sample i of a call
 * with B samples has the bits of a call with that sample alone.
 */
#ifndef OMNITOK_DIT_H
#define OMNITOK_DIT_H

#include "omnitok.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct omnitok_dit omnitok_dit;

typedef struct omnitok_dit_config {
    int input_size;      /* latent height = width (32 at 256 x 256 pixels)                                      */
    int patch_size;      /* p; input_size % p == 0; tokens N = (input_size / p)^2                               */
    int in_channels;     /* C; p * p * C <= 512                                                                 */
    int hidden;          /* D = heads * head_dim, head_dim 64 or 72; D % 32 == 0                                */
    int depth;           /* blocks                                                                              */
    int heads;
    int mlp_hidden;      /* int(D * mlp_ratio); % 32 == 0                                                       */
    int num_classes;     /* label table rows, + 1 (the null row of classifier-free guidance) if class_dropout > 0 */
    float class_dropout;
    int learn_sigma;     /* output channels 2 C (eps | variance interpolation) instead of C                      */
} omnitok_dit_config;

/* A configuration outside the list above: OMNITOK_ERR_INVALID, the reason in the error message. */
int omnitok_dit_create(const omnitok_dit_config *cfg, omnitok_dit **out);
void omnitok_dit_destroy(omnitok_dit *e);
/* Reference state_dict keys of models.py DiT: x_embedder.proj.weight [D,C,p,p], x_embedder.proj.bias [D],
 * t_embedder.mlp.{0,2}.{weight,bias}, y_embedder.embedding_table.weight [rows,D], pos_embed [1,N,D],
 * blocks.{i}.attn.{qkv,proj}.{weight,bias}, blocks.{i}.mlp.{fc1,fc2}.{weight,bias}, blocks.{i}.adaLN_modulation.1.{weight,bias},
 * final_layer.adaLN_modulation.1.{weight,bias}, final_layer.linear.{weight,bias}.  The tensor is copied.  Unknown keys return
 * 1 = ignored; a known key with another shape OMNITOK_ERR_INVALID. */
int omnitok_dit_set_weight(omnitok_dit *e, const char *name, const void *dev_ptr, const int64_t *shape, int ndim,
                           omnitok_stream_t stream);
/* Names not set yet, separated by '\n', as many as fit into buf (cap bytes, always terminated); returns their count
 * (right after create: every key of the list above). */
int omnitok_dit_missing(omnitok_dit *e, char *buf, int cap);
/* All weights set -> ready; OMNITOK_ERR_STATE names the first missing one.  Builds the timestep table (below). */
int omnitok_dit_finalize(omnitok_dit *e, omnitok_stream_t stream);
/* The sinusoidal timestep features of models.py:52-56 for t = 0 .. 999 as the engine gathers them: host memory,
 * table[1000][256], cos first, then sin.  The products t * freq are the reference's fp32 values; cos and sin of them are
 * computed in fp64 on the host and rounded once to fp32 (a device sinf of an argument up to 999 is not accurate enough).
 * freqs: host float[128], or NULL = exp of the reference's fp32 argument -log(10000) * i / 128, correctly rounded.  Needs no GPU. */
int omnitok_dit_timestep_table(const float *freqs, float *table);
/* The reference evaluates its frequencies with the fp32 exp of whatever runs it, and such exps differ in the last bit
 * (torch's CPU exp from the correctly rounded one in 3 of the 128: 3e-5 in a feature of t = 999).  A caller that compares
 * against a particular run passes that run's frequencies (host float[n], n == 128) before finalize; the binding passes torch's. */
int omnitok_dit_set_frequencies(omnitok_dit *e, const float *freqs, int n);
/* Device workspace one forward of B samples needs; the engine owns and grows it.  Needs no GPU; -1: bad arguments. */
int64_t omnitok_dit_workspace_bytes(omnitok_dit *e, int B);

/* models.py:233-248: x [B,C,H,W], t [B] int64 in [0, 1000), y [B] int64 in [0, table rows) -> out [B,Cout,H,W].  Fractional
 * timesteps are not supported.  t and y live on the device: a value outside its range is clamped into it (no read outside
 * the tables) and raises a bit that omnitok_dit_check reports. */
int omnitok_dit_forward(omnitok_dit *e, const float *x, const int64_t *t, const int64_t *y, int B, float *out,
                        omnitok_stream_t stream);
/* models.py:250-266, B even: the first B / 2 samples of x run twice, with y[0 .. B/2) and y[B/2 .. B); guidance
 * uncond + cfg_scale * (cond - uncond) is applied to channels [0, 3) only (the reference's quirk) and written to both halves;
 * every other channel passes through. */
int omnitok_dit_forward_cfg(omnitok_dit *e, const float *x, const int64_t *t, const int64_t *y, int B, float cfg_scale,
                            float *out, omnitok_stream_t stream);
/* Synchronises the stream and reads the range bits of the forwards since the last check: OMNITOK_ERR_INVALID with the reason
 * (t outside [0, 1000) / y outside [0, table rows) / under an fp16 linear or attention format a value outside the fp16 range), else 0.
 * Clears the bits. */
int omnitok_dit_check(omnitok_dit *e, omnitok_stream_t stream);

/* ---- opt-in 16-bit block linears ------------------------------------------------------------------------------------ */
#define OMNITOK_DIT_LIN_FP32 0 /* the default: everything above as written */
#define OMNITOK_DIT_LIN_BF16 1
#define OMNITOK_DIT_LIN_FP16 2
/* The format of the four linears of every block (attn.qkv, attn.proj, mlp.fc1, mlp.fc2).  Under a 16-bit format they run on
 * v_mfma_f32_32x32x16_{bf16,f16} (omnitok_dit_gemm16): both operands rounded ONCE to the format, to nearest even (the bits of
 * tensor.to(torch.bfloat16 / torch.float16)) -- the weights at the next finalize into a packed image beside the fp32 originals
 * (weight memory 1.5 x; switching back needs a finalize only), the activations where they are produced (the modulated LayerNorm rows,
 * the attention output, the GELU output) -- products exact, accumulators fp32.  Everything else stays fp32: the patch embedding, the
 * conditioning, the adaLN GEMM, the final layer, every bias, the residual stream, LayerNorm statistics and modulation, attention
 * (its own switch: omnitok_dit_set_attention_format), guidance, unpatchify, p_sample.  Batch invariance holds as before.
 * -1 before any HIP call for a null engine, an unknown format or sizes the 16-bit GEMM cannot take (hidden and mlp_hidden must be
 * multiples of 32); a refused value changes nothing.  Setting a format clears `finalized`.  fp16: a weight that rounds to +-inf makes
 * finalize fail with OMNITOK_ERR_INVALID naming the tensor (set another format and finalize again); an activation that does raises a
 * bit that omnitok_dit_check reports ("fp16"). */
int omnitok_dit_set_linear_format(omnitok_dit *e, int fmt);
int omnitok_dit_linear_format(omnitok_dit *e); /* -1: null engine */

/* ---- opt-in 16-bit attention operands -------------------------------------------------------------------------------- */
/* The OMNITOK_DIT_LIN_* values under a second name: one set of format codes, so that omnitok_dit_attn16 can write the packed
 * operand of attn.proj in the linear format without a translation. */
#define OMNITOK_DIT_ATTN_FP32 OMNITOK_DIT_LIN_FP32 /* the default: omnitok_dit_attn */
#define OMNITOK_DIT_ATTN_BF16 OMNITOK_DIT_LIN_BF16
#define OMNITOK_DIT_ATTN_FP16 OMNITOK_DIT_LIN_FP16
/* The format of the operands of every block's attention.  Under a 16-bit format it runs on omnitok_dit_attn16 (below: the arithmetic
 * contract and the fp16 range rules).  Independent of the linear format: all nine combinations are legal.  Where both are 16-bit the
 * attention writes the packed operand of attn.proj itself, in the linear format, and the omnitok_dit_round16 pass behind it is not
 * launched; its bits are those of that pass over the fp32 result.  With OMNITOK_DIT_ATTN_FP32 every launch is as before.
 * -1 before any HIP call for a null engine or an unknown format; a refused value changes nothing.  No weight image depends on the
 * format, so setting it does NOT clear `finalized`: it takes effect at the next forward.  fp16: a q, k or v that rounds from a finite
 * value to +-inf raises a bit that omnitok_dit_check reports ("attention format fp16"). */
int omnitok_dit_set_attention_format(omnitok_dit *e, int fmt);
int omnitok_dit_attention_format(omnitok_dit *e); /* -1: null engine */

/* ---- the operators of the forward, each usable without an engine ---------------------------------------------------- */

/* PatchEmbed (a stride-p conv = a [p*p*C -> D] linear per token) + pos_embed: x [x_batch,C,H,W], w [D,C,p,p], bias [D],
 * pos [N,D] -> out [B*N, D], N = (H/p)^2, H == W.  Sample b reads x[b % x_batch] (x_batch = B: every sample its own). */
int omnitok_dit_patch_embed(const float *x, int x_batch, const float *w, const float *bias, const float *pos, int B, int C,
                            int H, int p, int D, float *out, omnitok_stream_t stream);
/* out[r,:] = LayerNorm(x[r,:], eps 1e-6, no affine) * (1 + scale[b,:]) + shift[b,:], b = r / n_tokens; shift / scale rows
 * are ld_mod floats apart.  Two-pass statistics in fp32.  D % 4 == 0. */
int omnitok_dit_ln_modulate(const float *x, const float *shift, const float *scale, int64_t ld_mod, int64_t rows, int n_tokens,
                            int D, float *out, omnitok_stream_t stream);
/* Non-causal attention over [B, heads, N, hd] read straight from the qkv rows [B*N, 3*heads*hd] (timm's
 * reshape(B, N, 3, heads, hd)), scale hd^-0.5, hd 64 or 72 -> out [B*N, heads*hd]. */
int omnitok_dit_attn(const float *qkv, int B, int N, int heads, int head_dim, float *out, omnitok_stream_t stream);
/* omnitok_dit_attn with Q . K^T and P . V on v_mfma_f32_32x32x16_{bf16,f16}: op_fmt OMNITOK_DIT_LIN_BF16 | _FP16; the result goes to
 * exactly one of out32 [B*N, heads*hd] (fp32) and out16 (the same, rounded once more to out_fmt, a 16-bit format, and packed).
 *   - Q, K, V are each rounded ONCE to op_fmt, to nearest even (the bits of tensor.to(dtype)), where the kernel stages them: there
 *     is no packed copy of qkv and no workspace.
 *   - Products are exact.  A score is accumulated in fp32 and the finished dot multiplied by fl(log2(e) / sqrt(hd)), one constant
 *     rounded once from fp64: hd^-0.5 with the exponential's base change folded in.  At hd 72 the last half k-step multiplies zeros,
 *     never what lies behind column 71.
 *   - Online softmax over key tiles of 32, ascending; max, sum and rescale in fp32; the weights are v_exp_f32 of the base-2 score
 *     differences; l sums the weights BEFORE their rounding; P is rounded once to op_fmt on its way into P . V; O is accumulated in
 *     fp32; out = O / l, one division.
 *   - No atomics on the result, no split over keys, no partials.
 *   - Row (b, t) depends on rows b*N .. b*N + N - 1 of qkv only: not on B or on another sample.
 * flag (an int on the device, may be NULL): op_fmt fp16, a FINITE element of Q, K or V that rounds to +-inf ORs 8 into it; out_fmt
 * fp16, an output that rounds from a finite value to +-inf ORs 4, so out16 is bit for bit omnitok_dit_round16 of the out32 result, the
 * flag included.  bf16 sets neither.
 * -1 before any HIP call: null or non-16-byte-aligned pointers, both or neither output, op_fmt / out_fmt (with out16) not a 16-bit
 * format, head_dim not 64 | 72, sizes outside omnitok_dit_attn's. */
int omnitok_dit_attn16(const float *qkv, int B, int N, int heads, int head_dim, int op_fmt, float *out32, void *out16, int out_fmt,
                       int *flag, omnitok_stream_t stream);
/* x[r,:] += gate[b,:] * y[r,:], b = r / n_tokens; gate rows are ld_gate floats apart.  D % 4 == 0. */
int omnitok_dit_gate_residual(float *x, const float *y, const float *gate, int64_t ld_gate, int64_t rows, int n_tokens, int D,
                              omnitok_stream_t stream);
/* nn.GELU(approximate="tanh") in place over n floats. */
int omnitok_dit_gelu_tanh(float *x, int64_t n, omnitok_stream_t stream);
/* omnitok_dit_ln_modulate with its result rounded once to fmt (OMNITOK_DIT_LIN_BF16 | _FP16) into the packed out16 [rows, D].
 * fp16: a finite value that rounds to +-inf ORs 4 into *flag (an int on the device; may be NULL for bf16). */
int omnitok_dit_ln_modulate16(const float *x, const float *shift, const float *scale, int64_t ld_mod, int64_t rows, int n_tokens,
                              int D, int fmt, void *out16, int *flag, omnitok_stream_t stream);
/* dst16[i] = src[i] rounded to fmt, n % 4 == 0: the pass behind the attention, and the weight images.  flag as above. */
int omnitok_dit_round16(const float *src, int fmt, void *dst16, int64_t n, int *flag, omnitok_stream_t stream);
/* The GEMM of a 16-bit linear format: a16 [M, K] . w16 [N, K]^T, both packed in fmt and row-major, fp32 accumulators, K % 32 == 0,
 * M <= 2^24, and then one of three epilogues in fp32 on the accumulators (bias [N] is required): */
#define OMNITOK_DIT_EPI_BIAS 0          /* y32 [M, N] = acc + bias                                                              */
#define OMNITOK_DIT_EPI_GELU16 1        /* y16 [M, N] = gelu_tanh(acc + bias) (omnitok_dit_gelu_tanh's arithmetic) rounded to fmt;  */
                                        /* flag as above                                                                         */
#define OMNITOK_DIT_EPI_GATE_RESIDUAL 2 /* x [M, N] += gate[m / n_tokens, :] * (acc + bias): omnitok_dit_gate_residual's arithmetic; */
                                        /* gate rows ld_gate floats apart, ceil(M / n_tokens) of them                            */
/* Exactly the outputs of the epilogue are non-NULL (y32 | y16 | gate and x).  Row m of the result depends on row m of a16, on
 * x[m, :] and on its sample's gate row only; the order of a dot product's partial sums is fixed by K.  -1 before any HIP call for
 * null or non-16-byte-aligned pointers, sizes outside the contract, an unknown fmt or epilogue, or outputs that do not match it. */
int omnitok_dit_gemm16(const void *a16, const void *w16, int fmt, const float *bias, int epilogue, float *y32, void *y16,
                       const float *gate, int64_t ld_gate, int n_tokens, float *x, int64_t M, int N, int K, int *flag,
                       omnitok_stream_t stream);
/* models.py:218-231: lin [B*N, p*p*Cout] -> out [B,Cout,H,H] (nhwpqc -> nchpwq), H = sqrt(N) * p. */
int omnitok_dit_unpatchify(const float *lin, int B, int N, int p, int Cout, float *out, omnitok_stream_t stream);
/* One ancestral step, gaussian_diffusion.py:254-417 with epsilon prediction: model_out [B, 2C | C, HW], x, noise [B,C,HW],
 * t [B] int64 (clamped to [0, n_steps)), coef [n_steps][8] on the device:
 *   0 sqrt_recip_alphas_cumprod  1 sqrt_recipm1_alphas_cumprod  2 posterior_mean_coef1  3 posterior_mean_coef2
 *   4 posterior_log_variance_clipped (min_log)  5 log(betas) (max_log)  6 the fixed log variance  7 (t != 0)
 * learned_range != 0: log variance = frac * max_log + (1 - frac) * min_log, frac = (model_out[:, C + c] + 1) / 2; else coef 6.
 * pred_xstart = coef0 * x - coef1 * eps, clamped to [-1, 1] if clip; x_prev = coef2 * pred_xstart + coef3 * x +
 * coef7 * exp(0.5 * logvar) * noise.  pred_xstart may be NULL; x_prev may alias x. */
int omnitok_dit_p_sample(const float *model_out, const float *x, const float *noise, const float *coef, int n_steps,
                         const int64_t *t, int B, int C, int64_t HW, int learned_range, int clip, float *x_prev,
                         float *pred_xstart, omnitok_stream_t stream);
/* One DDIM step (gaussian_diffusion.py:513-560) or, with reverse != 0, one step of the reverse ODE (:562-598), epsilon prediction:
 * model_out, x, t as above, noise [B,C,HW] or NULL, coef [n_steps][8] on the device, the rows of
 * DDIMDiffusion.ddim_coefficient_table(eta) -- the reference's fp32 scalar chain, done on the host:
 *   0 sqrt_recip_alphas_cumprod  1 sqrt_recipm1_alphas_cumprod  2 sqrt(abar_prev)  3 sqrt(1 - abar_prev - sigma^2)
 *   4 sigma * (t != 0)  5 sqrt(abar_next)  6 sqrt(1 - abar_next)  7 unused (0)
 * Per element, each operation rounded to fp32 (the multiply-adds fused), eps = model_out[:, c]:
 *   pred_xstart = coef0 * x - coef1 * eps, clamped to [-1, 1] if clip;  e = (coef0 * x - pred_xstart) / coef1 (the reference
 *   re-derives eps from pred_xstart: under clip it is not the model's);
 *   forward: x_out = pred_xstart * coef2 + coef3 * e (+ coef4 * noise if noise != NULL);  reverse: x_out = pred_xstart * coef5 + coef6 * e.
 * DDIM ignores the variance: channels [C, 2C) of a learned_range output are never read.  noise is never read under reverse; pass
 * NULL for eta == 0 (coef4 == 0), and no draw is needed.  pred_xstart may be NULL.  Four elements per thread where C * HW % 4 == 0
 * and every pointer is 16-byte aligned, one otherwise: the bits are the same.
 * -1 before any HIP call, the message naming the argument: model_out, x, coef, t or x_out null; n_steps, B, C or HW below 1; more
 * elements than a 32-bit grid of 256-thread workgroups covers. */
int omnitok_dit_ddim_step(const float *model_out, const float *x, const float *noise, const float *coef, int n_steps,
                          const int64_t *t, int B, int C, int64_t HW, int learned_range, int clip, int reverse, float *x_out,
                          float *pred_xstart, omnitok_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* OMNITOK_DIT_H */
