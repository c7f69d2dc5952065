/* omnitok_latte.h -- C ABI of the Latte video denoiser, the video half of the reference's generation pipeline.
 *
 * The reference samples a Latte transformer on the `--use_vae` tokenizer's video latents (Diffusion/Latte/models/latte.py:209-403,
 * sample/sample_ddp.py:148-211) with the ancestral sampler of Diffusion/Latte/diffusion/gaussian_diffusion.py.  Latte is the DiT
 * of omnitok_dit.h with blocks that alternate: an even block attends over the N tokens of each frame (omnitok_dit_attn), an odd
 * block over the F frames of each token position (omnitok_latte_attn_temporal, below).  The reference rearranges the activations
 * '(b f) t d -> (b t) f d' and back around every odd block; this engine never does: rows stay in (b f) n order and the temporal
 * attention reads the F rows of a position where they lie, N rows apart.  omnitokenizer_amd/latte.py is the ctypes binding that
 * mirrors the reference's `Latte` class; the sampler is omnitokenizer_amd/diffusion.py (omnitok_dit_p_sample on the B F frames).
 *
 * Conventions of omnitok_dit.h: device pointers, fp32 (timesteps and labels int64), row-major, every launch on the given stream,
 * 0 = OK, argument errors are returned before any HIP call, omnitok_last_error holds the message.  Results do not depend on the
 * batch: sample i of a call with B samples has the bits of a call with that sample alone.
 *
 * Built: extras 1 (unconditional) and 2 (class labels).  Not built: extras 78 (the text embedding of latte_t2v.py's relatives),
 * latte_img.py, latte_t2v.py, fp16.  The samplers (ancestral and DDIM) are omnitok_dit.h's: omnitok_dit_p_sample and omnitok_dit_ddim_step
 * over the B F frames.
 */
#ifndef OMNITOK_LATTE_H
#define OMNITOK_LATTE_H

#include "omnitok_dit.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct omnitok_latte omnitok_latte;

typedef struct omnitok_latte_config {
    int input_size;      /* as omnitok_dit_config ...                                                             */
    int patch_size;
    int in_channels;
    int hidden;
    int depth;           /* ... and even: the forward takes the blocks in (spatial, temporal) pairs               */
    int heads;
    int mlp_hidden;
    int num_classes;     /* read when extras == 2                                                                 */
    float class_dropout;
    int learn_sigma;
    int num_frames;      /* latent frames F, 1 .. 32 (5 for the OmniTokenizer VAE at 17 frames, 16 for sd1.4)     */
    int extras;          /* 1: c = silu(t_emb); 2: c = silu(t_emb + y_emb); 78 (text): not built                  */
} omnitok_latte_config;

/* A configuration outside the list above: OMNITOK_ERR_INVALID, the reason in the error message. */
int omnitok_latte_create(const omnitok_latte_config *cfg, omnitok_latte **out);
void omnitok_latte_destroy(omnitok_latte *e);
/* Reference state_dict keys of latte.py Latte: the keys of omnitok_dit_set_weight plus temp_embed [1,F,D];
 * y_embedder.embedding_table.weight exists only with extras == 2.  Same return values. */
int omnitok_latte_set_weight(omnitok_latte *e, const char *name, const void *dev_ptr, const int64_t *shape, int ndim,
                             omnitok_stream_t stream);
int omnitok_latte_missing(omnitok_latte *e, char *buf, int cap);
int omnitok_latte_finalize(omnitok_latte *e, omnitok_stream_t stream);
/* The DiT engine's set_frequencies under this engine's name (the timestep table is the one of omnitok_dit.h). */
int omnitok_latte_set_frequencies(omnitok_latte *e, const float *freqs, int n);
/* Device workspace one forward of B samples (B F frames) needs; needs no GPU; -1: bad arguments. */
int64_t omnitok_latte_workspace_bytes(omnitok_latte *e, int B);

/* latte.py:319-382: x [B,F,C,H,W], t [B] int64 in [0, 1000), y [B] int64 in [0, table rows) (extras == 2; ignored and may be
 * NULL with extras == 1) -> out [B,F,Cout,H,W].  Out-of-range t / y are clamped and flagged as in omnitok_dit_forward. */
int omnitok_latte_forward(omnitok_latte *e, const float *x, const int64_t *t, const int64_t *y, int B, float *out,
                          omnitok_stream_t stream);
/* latte.py:384-403, B even: the first B / 2 samples of x run twice, with y[0 .. B/2) and y[B/2 .. B); guidance
 * uncond + cfg_scale * (cond - uncond) is applied to channels [0, 4) of every frame (the reference's literal 4: half of the eps
 * channels of an 8-channel latent) and written to both halves; every other channel passes through. */
int omnitok_latte_forward_cfg(omnitok_latte *e, const float *x, const int64_t *t, const int64_t *y, int B, float cfg_scale,
                              float *out, omnitok_stream_t stream);
int omnitok_latte_check(omnitok_latte *e, omnitok_stream_t stream);
/* The opt-in 16-bit block linears of omnitok_dit.h under this engine's name: declared in omnitok_latte_linear.h, included below.
 * The opt-in 16-bit operands of the spatial attention likewise: omnitok_latte_attention.h. */

/* ---- the operators Latte adds to those of omnitok_dit.h, each usable without an engine -------------------------------- */

/* Non-causal attention over the FRAMES of every token position: qkv [B*F*N, 3*heads*hd] with rows in (b f) n order (timm's
 * reshape(.., 3, heads, hd) columns); for every (b, n, head) the sequence is the F rows (b*F + f)*N + n, f = 0 .. F-1;
 * scale = fl(hd^-0.5); out [B*F*N, heads*hd] at the same rows.  hd 64 or 72, F 1 .. 32, 16-byte aligned pointers. */
int omnitok_latte_attn_temporal(const float *qkv, int B, int F, int N, int heads, int head_dim, float *out,
                                omnitok_stream_t stream);
/* x[(b*F + f)*N + n, :] += temp_embed[f, :] (latte.py:360-363, one rounding per element).  D % 4 == 0. */
int omnitok_latte_add_temp_embed(float *x, const float *temp_embed, int B, int F, int N, int D, omnitok_stream_t stream);
/* out [images, Cout, HW], images even: channels [0, min(channels, Cout)) of image i and image i + images/2 both become
 * uncond + scale * (cond - uncond) (cond = image i, three fp32 roundings as torch's); in place. */
int omnitok_latte_cfg_blend(float *out, int images, int Cout, int channels, int64_t HW, float scale, omnitok_stream_t stream);

#ifdef __cplusplus
}
#endif

#include "omnitok_latte_linear.h"
#include "omnitok_latte_attention.h"

#endif /* OMNITOK_LATTE_H */
