/* omnitok_lm.h -- C ABI of the autoregressive LM consumer of the token path.
 *
 * The reference samples video/image tokens with a minGPT (OmniTokenizer/modules/gpt.py:170-275)
 * through `sample_with_past` (gpt.py:327-359): one token per step, the K/V of every layer kept and
 * re-concatenated on every step (torch.cat(past, dim=-2), gpt.py:244).  This library keeps a
 * preallocated K/V cache in HBM and runs one decode step as a fixed sequence of kernels whose
 * shapes do not depend on the position, so the caller can capture the step in a HIP graph.
 * omnitokenizer_amd/gpt.py is the ctypes binding that mirrors the reference's `GPT` class
 * (forward / forward_with_past) and its sampling loops.
 *
 * Same conventions as omnitok.h: device pointers, fp32 (ids int64, positions int32), row-major,
 * every launch on the given stream, 0 = OK, omnitok_last_error() for the message.
 */
#ifndef OMNITOK_LM_H
#define OMNITOK_LM_H

#include "omnitok.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct omnitok_lm omnitok_lm;

typedef struct omnitok_lm_config {
    int vocab_size; /* gpt_vocab_size = first_stage + cond_stage (+1), lm_transformer.py:60-62 */
    int block_size; /* positions, 5120 + conditioning */
    int n_layer;    /* 24 */
    int n_head;     /* 16 */
    int n_embd;     /* 1536; head_dim = n_embd / n_head must be 64, 96 or 128 */
} omnitok_lm_config;

int omnitok_lm_create(const omnitok_lm_config *cfg, omnitok_lm **out);
void omnitok_lm_destroy(omnitok_lm *lm);
/* reference state_dict keys of modules/gpt.py GPT: pos_emb [1,block,C], tok_emb.weight [V,C],
 * blocks.{i}.ln1|ln2.{weight,bias}, blocks.{i}.attn.{key,query,value,proj}.{weight,bias},
 * blocks.{i}.mlp.{0,2}.{weight,bias}, ln_f.{weight,bias}, head.weight [V,C].  Unknown keys
 * (blocks.{i}.attn.mask) return 1 = ignored. */
int omnitok_lm_set_weight(omnitok_lm *lm, const char *name, const void *dev_ptr,
                          const int64_t *shape, int ndim, omnitok_stream_t stream);
int omnitok_lm_finalize(omnitok_lm *lm, omnitok_stream_t stream);
/* Format of the weight matrices a decode step streams -- per engine, default OMNITOK_LM_W_FP32 (nothing below applies then).  The
 * reference trains this model under Lightning's precision="bf16" / 16 (transformer_train.py:63-66): every nn.Linear sees 16-bit
 * weights there.  A 16-bit engine rounds ONLY the matrices; activations, accumulation, LayerNorm and attention stay fp32 (the K/V
 * cache has a format switch of its own, omnitok_lm_set_cache_format below), and the decode step -- bound by the bytes of exactly these matrices -- streams half of them.
 *   Which tensors: wqkv (query | key | value, concatenated at finalize), attn.proj.weight, mlp.0.weight, mlp.2.weight of every
 *     block and head.weight.  Biases, LayerNorm parameters, tok_emb, pos_emb and the K/V cache stay fp32 (gathers, or a few KB
 *     per step).
 *   Rounding: on the device, inside omnitok_lm_finalize, round to nearest even -- the bits of tensor.to(torch.bfloat16) /
 *     .to(torch.float16), fp16 subnormals included.
 *   Two images of each matrix: the packed 16-bit one, which the decode GEMVs read and widen to fp32 in registers (exact), and the
 *     fp32 one OVERWRITTEN IN PLACE with the rounded values, which omnitok_lm_prefill* and omnitok_lm_prefill_loss keep using
 *     unchanged -- prefill and stepping compute on the same weight values ("same arithmetic as T decode steps" below holds).
 *     Weight memory is 1.5 x the fp32 engine's.
 *   fp16 range: if an element of one of these matrices rounds to +-inf in fp16, omnitok_lm_finalize fails with
 *     OMNITOK_ERR_INVALID and names the tensor in omnitok_last_error(); the engine stays unfinalized and, its images being
 *     half-rounded by then, accepts a finalize only after ALL weights were set again.  bf16 has fp32's range.
 *   omnitok_lm_set_weight_format clears `finalized` (-1: null engine / unknown format).  As after any finalize the q/k/v
 *     sources are gone: set ALL weights again, then finalize. */
#define OMNITOK_LM_W_FP32 0
#define OMNITOK_LM_W_BF16 1
#define OMNITOK_LM_W_FP16 2
int omnitok_lm_set_weight_format(omnitok_lm *lm, int fmt);
int omnitok_lm_weight_format(omnitok_lm *lm); /* -1: null engine */
/* bytes of matrices one decode step WITH logits streams in the engine's format:
 * (12 * n_embd^2 * n_layer + vocab_size * n_embd) * sizeof(element).  Needs no GPU; 0 for a null engine. */
int64_t omnitok_lm_step_weight_bytes(omnitok_lm *lm);

/* Weight-only fp8 for the decode step -- per engine, default OMNITOK_LM_DQ_NONE (nothing below applies then: a default engine issues
 * exactly the launches and computes exactly the bits it did before the switch existed).  It is NOT a weight format: the weight
 * format keeps deciding what every other path reads.  With OMNITOK_LM_DQ_FP8 omnitok_lm_finalize additionally makes, for each of
 * the five matrix families a step streams (wqkv, attn.proj, mlp.0, mlp.2 of every block and head.weight), an OCP e4m3fn image of one
 * byte per weight and one fp32 scale per output row, and a decode step of fewer than "lm_streams_min" (default 17) streams reads
 * those instead of the fp32 / 16-bit image: a quarter / half of the bytes.
 *   Scale: s[n] = 2^e with e the smallest integer such that amax_n * 2^-e <= 448 (e4m3fn's largest value).  Exactly, with
 *     amax_n = m * 2^x, m in [0.5, 1) (frexp): e = x - 9 if m <= 0.875, else x - 8; an all-zero row has s[n] = 1; e is clamped to
 *     [-126, 127] so that s is a normal fp32.
 *   Weight: q[n, k] = e4m3fn(w[n, k] * 2^-e) -- the scaling is exact, the conversion ONE round to nearest even with subnormal results
 *     kept: the bits of torch's CPU tensor.to(torch.float8_e4m3fn).  No value exceeds 448 after the scaling, so nothing saturates.
 *     Always quantised from the fp32 values that were set, also when the weight format rounds the other images to 16 bits.
 *   A step then computes y = act(s[n] * sum_k x[k] * q[n, k] + bias) (+ residual): s * q is exact in fp32 and so is the scaling of
 *     the sum, i.e. an fp32 dot product of the fp32 activations with the exact fp32 values s * q in some order -- the fp32 step's
 *     arithmetic on other weight values, as with the 16-bit formats.  Activations, accumulation, LayerNorm, attention and the K/V
 *     cache are untouched.  e4m3 has 3 mantissa bits: relative weight error up to 2^-4 above the subnormal range of a row.
 *   Scope: ONLY that decode step.  The batched prefill, omnitok_lm_prefill_loss and a step of "lm_streams_min" or more streams keep
 *     running on the weight format's images, bit for bit as without the switch; option "lm_mfma" 1 does not take fp8 matrices.  So
 *     "same arithmetic as T decode steps" does NOT hold under OMNITOK_LM_DQ_FP8: prefill and stepping compute on different weight
 *     values (as they compute on different activations under OMNITOK_LM_PF_W16).
 *   Non-finite weights: a NaN or an infinity in one of these matrices makes omnitok_lm_finalize fail with OMNITOK_ERR_INVALID and
 *     the tensor's name in omnitok_last_error(); set all weights again.
 *   Memory: the images add a quarter of the fp32 weights' bytes.  omnitok_lm_step_weight_bytes under OMNITOK_LM_DQ_FP8 is
 *     (12 * n_embd^2 * n_layer + vocab_size * n_embd) * 1 + (12 * n_embd * n_layer + vocab_size) * 4: the scales are counted.
 * omnitok_lm_set_decode_quant: -1 for a null engine or an unknown value (a refused value changes nothing).  Like
 * omnitok_lm_set_weight_format it clears `finalized`: set ALL weights again, then finalize.  Independent of the weight, cache,
 * prefill and streams formats and of max_streams. */
#define OMNITOK_LM_DQ_NONE 0
#define OMNITOK_LM_DQ_FP8 1
int omnitok_lm_set_decode_quant(omnitok_lm *lm, int q);
int omnitok_lm_decode_quant(omnitok_lm *lm); /* -1: null engine */

/* Format of the K/V cache -- per engine, default OMNITOK_LM_KV_FP32 (nothing below applies then), independent of the weight format
 * (all 3 x 3 combinations work).  At long contexts the cache is the other half of a decode step's traffic (24 layers x 2 x 4608 rows
 * x 1536 x 4 B = 1.36 GB per stream and step at the reference's context), and under the reference's precision="bf16" its own
 * `present` K/V tensors are 16-bit.  A 16-bit cache stores half the bytes:
 *   Rounding at the store: a token's K and V rows are rounded ONCE, where they are stored -- the decode step's append and the
 *     prefill's scatter -- to nearest even: the bits of tensor.to(torch.bfloat16) / .to(torch.float16), fp16 subnormals kept,
 *     NaN -> quiet NaN (the conversions of the weight images).
 *   The own row stays fp32: in the step (or prefill row) that produces a token, the token's own K/V row enters the attention as the
 *     fp32 values of qkv; every earlier row is read from the cache and widened to fp32 in registers, which is exact.
 *   Everything else stays fp32: q, the scores, the softmax, the accumulators, the chunk partials, their merge and all activations.
 *   Consequence: attention over a 16-bit cache is the fp32 kernel's arithmetic on a cache that holds the widened values, bit for bit.
 *     Prefill and stepping stay the same arithmetic in the sense they are today: their fp32 K/V differ in the last bits (other
 *     summation orders), so a few cached elements may round to neighbouring 16-bit values.
 *   fp16 range: a stored element that rounds to +-inf raises bit 2 of the engine's flag word (omnitok_lm_overflowed); the cache then
 *     holds the infinity.  bf16 has fp32's range.
 * omnitok_lm_set_cache_format: -1 for a null engine or an unknown format (a refused format changes nothing).  It frees an allocated
 * cache and its step workspaces -- the next step or prefill returns OMNITOK_ERR_STATE until omnitok_lm_alloc_cache runs again -- and
 * touches neither `finalized` nor any weight. */
#define OMNITOK_LM_KV_FP32 0
#define OMNITOK_LM_KV_BF16 1
#define OMNITOK_LM_KV_FP16 2
int omnitok_lm_set_cache_format(omnitok_lm *lm, int fmt);
int omnitok_lm_cache_format(omnitok_lm *lm); /* -1: null engine */

/* fp8 K/V cache -- per engine, default OMNITOK_LM_KQ_NONE (nothing below applies then: a default engine issues exactly the launches
 * and bits it did), independent of the weight format, the decode quant, the streams / prefill formats and max_streams.  It is not a
 * fourth cache format but a quantisation with side data, as omnitok_lm_set_decode_quant is beside the weight format: the cache FORMAT
 * keeps its value and its getter and decides nothing about storage while the quant is on.  With OMNITOK_LM_KQ_FP8:
 *   Storage: for every (layer, K | V, stream, head, position) head_dim bytes of OCP e4m3fn, laid out
 *     [n_layer][2][max_batch][n_head][max_len][head_dim] as before, and one fp32 scale per such row,
 *     [n_layer][2][max_batch][n_head][max_len].  omnitok_lm_cache_bytes counts both: elements x 1 + rows x 4 -- a quarter of the fp32
 *     cache plus 4 / head_dim of it.
 *   Scale rule: omnitok_lm_set_decode_quant's, applied to one head's row of one token: s = 2^e with e the smallest integer such that
 *     amax 2^-e <= 448 -- with amax = m 2^x, m in [0.5, 1) (frexp): e = x - 9 if m <= 0.875 else x - 8 -- s = 1 for an all-zero row,
 *     e clamped to [-126, 127]; q = e4m3fn(v 2^-e), one round to nearest even, subnormal results kept.  The cache HOLDS THE VALUES
 *     s * widen(q), which are exact in fp32, fp32 subnormals included.
 *   Quantised once, where a row is stored: the decode step's append and the prefill's scatter -- where the 16-bit formats round.  The
 *     step (or prefill row) that produces a token uses that token's own fp32 row of qkv.  The OMNITOK_LM_PA_ROWS prefill reads
 *     earlier rows from the cache, so it sees them quantised; the OMNITOK_LM_PA_TILED prefill reads qkv and is unaffected.
 *   Arithmetic: every cached element enters as widen(q) * s in front of the unchanged fp32 chain, so attention over an fp8 cache is
 *     the fp32 kernel's arithmetic on a cache that holds s * widen(q), bit for bit: lane mapping, fmaf chains, softmax, chunking and
 *     merge are those of the fp32 cache.  omnitok_lm_cache_read returns s * widen(q).
 *   Non-finite rows: a K or V row that holds a NaN or an infinity when it is stored raises bit 32 of the engine's flag word
 *     (omnitok_lm_overflowed); what the cache holds for that row is unspecified.
 * omnitok_lm_set_cache_quant: -1 for a null engine or an unknown value (a refused value changes nothing).  Like
 * omnitok_lm_set_cache_format it frees an allocated cache and its step workspaces -- the next step or prefill returns
 * OMNITOK_ERR_STATE until omnitok_lm_alloc_cache runs again -- and touches neither `finalized` nor any weight. */
#define OMNITOK_LM_KQ_NONE 0
#define OMNITOK_LM_KQ_FP8 1
int omnitok_lm_set_cache_quant(omnitok_lm *lm, int q);
int omnitok_lm_cache_quant(omnitok_lm *lm); /* -1: null engine */

/* Streams per engine -- default 16 (nothing below applies then).  omnitok_lm_alloc_cache accepts max_batch <= max_streams; with more
 * than 16 streams one step serves all of them in ONE pass over every weight matrix (the <= 16-stream kernels read each matrix once
 * per group of 8 streams), so tokens per second over all streams keep growing with the batch.  Classifier-free guidance doubles the
 * batch: 2 B rows.
 *   Routing: a step of B >= option "lm_streams_min" (default 17) streams runs the many-stream kernels (omnitok_lm_gemm_streams below,
 *     the chunk partials of the attention merged into a tensor, LayerNorm as a pass of its own); a step of fewer streams runs exactly
 *     the kernels it ran before, whatever max_streams is.  Both paths serve every B <= max_batch: with "lm_streams_min" above B a step of up
 *     to 128 streams runs the <= 16-stream kernels in groups of 8 / 4 / 2 / 1 streams (one pass over the weights per group).  Prefill, omnitok_lm_prefill_loss, omnitok_lm_cache_read and
 *     omnitok_lm_overflowed work for every B <= max_batch.
 *   Arithmetic: unchanged -- fp32 activations, fp32 products with the weight's exact fp32 value, fp32 accumulation in a fixed order
 *     (no atomics: two calls give equal bits).  A stream's logits do not depend on how many streams share the step, on its slot, or
 *     on what the others hold.  The order of a dot product's partial sums differs from the <= 16-stream kernels': the two paths agree
 *     to rounding, not to the bit.
 *   Memory: the cache grows with max_batch.  At the reference's model (24 layers x 1536, 5121 positions) 128 streams are 193 GB in
 *     fp32 and 97 GB in a 16-bit cache format (16 streams: 24 GB / 12 GB).  An allocation the device cannot satisfy makes
 *     omnitok_lm_alloc_cache return OMNITOK_ERR_HIP with hipMalloc's message; the engine is then left without a cache.
 * omnitok_lm_set_max_streams: -1 for a null engine or an n outside [1, 128] (a refused n changes nothing).  Like
 * omnitok_lm_set_cache_format it frees an allocated cache and its step workspaces -- the next step or prefill returns
 * OMNITOK_ERR_STATE until omnitok_lm_alloc_cache runs again -- and touches neither `finalized` nor any weight. */
int omnitok_lm_set_max_streams(omnitok_lm *lm, int n);
int omnitok_lm_max_streams(omnitok_lm *lm); /* -1: null engine */

/* How a many-stream decode step runs its GEMMs -- per engine, default OMNITOK_LM_SF_FP32 (nothing below applies then: a default engine
 * issues exactly the launches it issued before the switch existed).  The many-stream step (B >= option "lm_streams_min" streams, above)
 * multiplies fp32 activations on the fp32-input MFMA even when the engine holds packed 16-bit weight images, widening every weight in
 * registers; at 64 and 128 streams it is bound by that instruction, which runs at 1/16 of the matrix cores' 16-bit rate.
 * OMNITOK_LM_SF_W16 runs the step's four linears per block and the head on the bf16 / fp16 MFMA instead (omnitok_lm_gemm_streams16 below)
 * over the packed images:
 *   Needs a 16-bit weight format: with OMNITOK_LM_W_FP32 in force omnitok_lm_step / _step_ex return OMNITOK_ERR_STATE and name both
 *     switches in omnitok_last_error(), whatever B is -- there is no fallback.
 *   Only the many-stream step: a step of fewer than "lm_streams_min" streams (default 17) runs the <= 16-stream kernels exactly as before,
 *     and the switch has no effect on it ("lm_streams_min" 1 sends every B to the 16-bit kernel, as it sends it to the fp32-MFMA one
 *     today).  The prefill has its own switch (omnitok_lm_set_prefill_format) and is unaffected.
 *   What is rounded: the A operand of each GEMM, ONCE, to the engine's weight format (lm_round16, round to nearest even) -- the rounding
 *     points of an OMNITOK_LM_PF_W16 prefill: the LayerNorm rows (ln1, ln2, ln_f), the merged attention output and FC1's GELU output (in
 *     its GEMM's fp32 epilogue).  Products are exact in fp32, accumulation is fp32 in an order fixed by (N, K) alone, no atomics: a
 *     stream's logits do not depend on B, on its slot or on what the other streams hold, and two calls give equal bits.
 *   Everything else stays fp32: the embeddings, the residual stream, the LayerNorm statistics, qkv and what goes into the K/V cache (in
 *     the cache's own format), the flash-decode attention and its partials, biases and the logits.
 *   The step is then no longer the fp32 step's arithmetic: its logits differ from the OMNITOK_LM_SF_FP32 step's by the activation rounding
 *     (tests/test_gpu_lm_streams16.py holds them to the bar of tests/lm_prefill16_ref.py, the restatement of these rounding points).
 *   fp16 range: an activation that rounds to +-inf raises bit 16 of the engine's flag word (omnitok_lm_overflowed).  bf16 has fp32's
 *     range and never does.
 * omnitok_lm_set_streams_format: -1 for a null engine or an unknown format (a refused format changes nothing); it touches neither
 * `finalized`, the weights nor the cache, is independent of the cache format, the three prefill switches and max_streams, and applies
 * from the next step on (a captured graph keeps the launches it was captured with). */
#define OMNITOK_LM_SF_FP32 0
#define OMNITOK_LM_SF_W16 1
int omnitok_lm_set_streams_format(omnitok_lm *lm, int fmt);
int omnitok_lm_streams_format(omnitok_lm *lm); /* -1: null engine */

/* How the batched prefill runs its GEMMs -- per engine, default OMNITOK_LM_PF_FP32 (nothing below applies then).  The prefill
 * (omnitok_lm_prefill, _prefill_ex, _prefill_loss) is bound by its five nn.Linear GEMMs per block and the head GEMM, which run on the
 * fp32-input MFMA (omnitok_gemm) at 1/16 of the matrix cores' 16-bit rate; under the reference's precision="bf16" its nn.Linears see
 * 16-bit activations AND 16-bit weights.  OMNITOK_LM_PF_W16 runs these six GEMMs on the bf16 / fp16 MFMA (omnitok_lm_gemm16 below)
 * over the packed weight images a 16-bit engine already holds:
 *   Needs a 16-bit weight format: with OMNITOK_LM_W_FP32 in force the three prefill entry points return OMNITOK_ERR_STATE and name
 *     both switches in omnitok_last_error() -- there is no fallback to the fp32 GEMM.
 *   What is rounded: the A operand of each GEMM, ONCE, to the engine's weight format (round to nearest even, lm_round16: the bits
 *     of tensor.to(torch.bfloat16) / .to(torch.float16)) -- the LayerNorm rows (ln1, ln2, ln_f), the merged attention output and
 *     FC1's GELU output.  Each is the rounding of the fp32 value the fp32 prefill computes at that point (the same LayerNorm and
 *     merge kernels with a 16-bit store; the GELU in the GEMM's fp32 epilogue).  Products are exact in fp32, accumulation is fp32 in
 *     an order fixed by K alone (no split-K, no atomics): a row's results do not depend on B, T or the other rows, two calls give
 *     equal bits, and omnitok_lm_prefill_loss gives equal bits for every "lm_loss_chunk_rows".
 *   Everything else stays fp32: the embedding and the residual stream, qkv and the K/V scatter into the cache (in the cache's own
 *     format), the attention partials and their merge, the LayerNorm statistics, bias / GELU / residual epilogues, the logits and
 *     the token cross-entropy.  The decode step is unaffected.
 *   "Same arithmetic as T decode steps" NO LONGER HOLDS: a step multiplies fp32 activations, a PF_W16 prefill rounded ones.  The
 *     prefill's logits differ from the fp32 prefill's of the same 16-bit engine by the activation rounding: measured on the golden
 *     models (3 streams x 40 tokens, logits of magnitude 3 .. 6) max |difference| 1.2e-2 .. 2.9e-2 in bf16 and 1.4e-3 .. 3.9e-3 in
 *     fp16 (tests/test_gpu_lm_prefill16.py prints them); the K/V rows a PF_W16 prefill leaves in the cache differ in the same way.
 *   fp16 range: an activation that rounds to +-inf raises bit 4 of the engine's flag word (omnitok_lm_overflowed).  bf16 has
 *     fp32's range.
 * omnitok_lm_set_prefill_format: -1 for a null engine or an unknown format (a refused format changes nothing); it touches neither
 * `finalized`, the weights nor the cache, and applies from the next prefill on. */
#define OMNITOK_LM_PF_FP32 0
#define OMNITOK_LM_PF_W16 1
int omnitok_lm_set_prefill_format(omnitok_lm *lm, int fmt);
int omnitok_lm_prefill_format(omnitok_lm *lm); /* -1: null engine */

/* How the batched prefill runs its causal attention -- per engine, default OMNITOK_LM_PA_ROWS (nothing below applies then).  The
 * rows mode is the decode step's attention kernel launched once per query row, head and 256-key chunk over the cache the prefill
 * has just filled, plus a merge of [B * T, n_head, chunks, 2 + head_dim] partials: every row re-reads its whole K/V prefix and its
 * dot products are fmaf chains on the VALU.  OMNITOK_LM_PA_TILED runs omnitok_lm_attn_prefill (below) instead: K/V tiles shared by
 * 128 query rows, both products on the fp32-input MFMA, no partials (that term leaves the prefill workspace).
 *   The arithmetic contract is kept: fp32 products, fp32 accumulation, expf in fp32, no value rounded that the rows mode does not
 *     round.  The ORDER of the sums differs (one dot-product chain per score instead of eight partial chains; online softmax over
 *     32-key tiles instead of 256-key chunks and a merge), so "same arithmetic as T decode steps" holds TO ROUNDING, NOT TO THE BIT,
 *     under the tiled mode: its results differ from the rows mode's by fp32 rounding (tests/test_gpu_lm_prefill_attn.py holds both
 *     to a derived bar against fp64).
 *   Operands: K and V are read from qkv, not from the cache (a prefill fills empty streams: every key of a row is in qkv), so the
 *     tiled attention does not depend on the cache format.  Under a 16-bit cache the rows mode reads the PAST rows rounded to the
 *     cache format and the row's own K/V in fp32; the tiled mode reads every row in fp32.  The K/V scatter is unchanged: the cache
 *     holds what the decode steps after the prefill read, rounded as before.
 *   Independent of the weight, cache and prefill formats and of max_streams: every combination works.  With OMNITOK_LM_PF_W16 the
 *     attention output is rounded once to the weight format (an fp16 +-inf raises bit 4 of the flag word), as the merge's was.
 *   The decode step is unaffected.
 * omnitok_lm_set_prefill_attention: -1 for a null engine or an unknown mode (a refused mode changes nothing); it touches neither
 * `finalized`, the weights nor the cache, and applies from the next prefill on. */
#define OMNITOK_LM_PA_ROWS 0
#define OMNITOK_LM_PA_TILED 1
int omnitok_lm_set_prefill_attention(omnitok_lm *lm, int mode);
int omnitok_lm_prefill_attention(omnitok_lm *lm); /* -1: null engine */

/* Operand format of the tiled prefill attention -- per engine, default OMNITOK_LM_AOP_FP32 (nothing below applies then: the bits of
 * omnitok_lm_set_prefill_attention above).  With OMNITOK_LM_AOP_BF16 / _FP16 and OMNITOK_LM_PA_TILED the prefill runs
 * omnitok_lm_attn_prefill16 (below) instead of omnitok_lm_attn_prefill: the same tiling with both products on the bf16 / fp16 MFMA
 * (16 x the rate of the fp32-input one).  This is the arithmetic of attention under autocast: 16-bit operands, fp32 accumulation.
 *   Rounded, each ONCE to lm_round16's bits (those of tensor.to(torch.bfloat16 / float16); a NaN stays a NaN, its payload is not
 *     specified): every element of Q, K and V, where the kernel stages it (no packed copy of qkv, no workspace), and every softmax
 *     weight P on its way into the P . V product.
 *   fp32: the accumulation of both products, the scale, the running max, the running sum l (of the weights BEFORE their rounding),
 *     the rescale, O and the division out = O / l.
 *   "Same arithmetic as T decode steps" does NOT hold in this mode, neither to the bit nor to fp32 rounding: the results differ from
 *     the fp32 modes' by the operand rounding (2^-9 relative per bf16 operand, 2^-12 per fp16 operand).  tests/lm_prefill_attn16_ref.py
 *     derives the bar against fp64 attention over the rounded operands.
 *   Deterministic: a row depends only on its position and its own stream's rows up to the end of its diagonal 32-key tile, and two
 *     calls give equal values (the statement of omnitok_lm_attn_prefill, its one limit included).  Key tiles of KT = 32; the
 *     exponential is v_exp_f32 on base-2 scores (log2(e) folded into the scale), documented error 1 ulp.
 *   fp16 range: a Q, K or V element that rounds to +-inf raises bit 8 of the engine's flag word (omnitok_lm_overflowed).  bf16 has
 *     fp32's range and never does.
 *   Independent of the weight, cache and prefill formats and of max_streams: an fp32-weight engine may use it.  With OMNITOK_LM_PF_W16
 *     the attention output is rounded once to the WEIGHT format, as before.  The K/V scatter (the cache holds the unrounded rows in
 *     the cache format) and the decode step are unchanged.
 *   With OMNITOK_LM_PA_ROWS and operands other than OMNITOK_LM_AOP_FP32, omnitok_lm_prefill, _prefill_ex and _prefill_loss return
 *     OMNITOK_ERR_STATE with both switches named in the message: there is no fallback.
 * omnitok_lm_set_prefill_attention_operands: -1 for a null engine or an unknown value (a refused value changes nothing); it touches
 * neither `finalized`, the weights nor the cache, and applies from the next prefill on. */
#define OMNITOK_LM_AOP_FP32 0
#define OMNITOK_LM_AOP_BF16 1
#define OMNITOK_LM_AOP_FP16 2
int omnitok_lm_set_prefill_attention_operands(omnitok_lm *lm, int fmt);
int omnitok_lm_prefill_attention_operands(omnitok_lm *lm); /* -1: null engine */

/* K/V cache [n_layer][2][max_batch][n_head][max_len][head_dim] in the engine's cache format (or e4m3fn bytes and their row scales,
 * omnitok_lm_set_cache_quant) + step workspaces;
 * max_batch <= omnitok_lm_max_streams (16 unless raised), otherwise -1 with the limit in force in the message. */
int omnitok_lm_alloc_cache(omnitok_lm *lm, int max_batch, int max_len);
int64_t omnitok_lm_cache_bytes(omnitok_lm *lm); /* the bytes allocated: half for a 16-bit cache, elements + 4 per row for an fp8 cache; 0 without a cache */
/* Rows t0 .. t0 + n - 1 of stream b of one layer, widened to fp32: k_out / v_out [n_head, n, head_dim] on the device (the
 * counterpart of the reference's `present`).  Every format; fp32 is a plain copy; an fp8 cache (omnitok_lm_set_cache_quant) returns s * widen(q).  Rows beyond cache_len[b] hold whatever the cache
 * holds.  -1: null pointers, layer outside [0, n_layer), b outside [0, max_batch), t0 < 0, n < 0 or t0 + n > max_len;
 * OMNITOK_ERR_STATE: no cache. */
int omnitok_lm_cache_read(omnitok_lm *lm, int layer, int b, int t0, int n, float *k_out, float *v_out,
                          omnitok_stream_t stream);

/* One decode step for B independent streams (GPT.forward_with_past with one new token per row,
 * gpt.py:236-275): token idx[b] enters at position embedding pos[b]; its K/V are appended to row
 * b of the cache at index cache_len[b]; it attends to cache entries [0, cache_len[b]] (all of the
 * past plus itself, gpt.py:125).  logits_out[B, vocab] (may be NULL: prefill steps whose logits
 * are not needed skip ln_f + head).  If advance != 0, cache_len[b] and pos[b] are incremented on
 * the device at the end of the step, so that the same captured graph can be replayed.
 * idx int64[B], pos / cache_len int32[B], all on the device. */
int omnitok_lm_step(omnitok_lm *lm, const int64_t *idx, int32_t *pos, int32_t *cache_len, int B,
                    float *logits_out, int advance, omnitok_stream_t stream);

/* The same step with the reference's optional inputs (gpt.py:236-258): emb [B, C] != NULL replaces the token
 * embedding (an explicit `embeddings=` vector; idx may then be NULL), pos_extra [B, C] != NULL is added to the
 * position embedding (the vtokens_pos term: rows of vtokens_pos_emb gathered by the caller from cbox). */
int omnitok_lm_step_ex(omnitok_lm *lm, const int64_t *idx, const float *emb, const float *pos_extra,
                       int32_t *pos, int32_t *cache_len, int B, float *logits_out, int advance,
                       omnitok_stream_t stream);

/* A mask of what happened since the last call, 0 if nothing; clears the flags.  Synchronises the stream (call it once after a
 * sampling loop).
 *   1: a decode step found cache_len[b] >= max_len (a stream stepped past the cache that omnitok_lm_alloc_cache sized; the step
 *      then stays inside the stream's own K/V slab and its logits are invalid);
 *   2: a K/V value stored into an OMNITOK_LM_KV_FP16 cache (a step's append or a prefill) left the fp16 range and was stored as
 *      +-inf: the logits from there on are invalid.  An fp32 or bf16 cache never returns 2.
 *   4: an activation of an OMNITOK_LM_PF_W16 prefill on an fp16 engine (a LayerNorm row, a merged attention row or FC1's GELU
 *      output) left the fp16 range and entered its GEMM as +-inf: that prefill's logits and cache rows are invalid.  Never set by
 *      the default prefill format or a bf16 engine.
 *   8: a Q, K or V element of a prefill attention with OMNITOK_LM_AOP_FP16 operands left the fp16 range and entered its MFMA as
 *      +-inf: that prefill's logits are invalid (the cache rows are stored unrounded and are not).  Never set by fp32 or bf16
 *      operands.
 *  16: an activation of an OMNITOK_LM_SF_W16 many-stream step on an fp16 engine (a LayerNorm row, a merged attention row or FC1's GELU
 *      output) left the fp16 range and entered its GEMM as +-inf: the logits from there on are invalid (a non-finite K/V row may sit
 *      in the cache).  Never set by the default streams format or a bf16 engine.
 *  32: a K or V row stored into an OMNITOK_LM_KQ_FP8 cache (a step's append or a prefill) held a NaN or an infinity: the row's cache
 *      contents are unspecified and the logits from there on are invalid.  Never set without the cache quant. */
int omnitok_lm_overflowed(omnitok_lm *lm, omnitok_stream_t stream);

/* Batched prefill of a conditioning prefix into EMPTY streams (GPT.forward / the first
 * forward_with_past call of the reference, gpt.py:207-275, positions 0..T-1): idx[B, T] int64.
 * Same arithmetic as T decode steps, executed as [B*T]-row fp32-MFMA GEMMs (omnitok_gemm) + causal
 * flash attention over the cache (with OMNITOK_LM_PF_W16 the GEMMs run on the 16-bit MFMA over
 * rounded activations instead, and "same arithmetic" no longer holds: omnitok_lm_set_prefill_format
 * above; with OMNITOK_LM_PA_TILED the attention runs tiled on the fp32-input MFMA straight from qkv, and
 * "same arithmetic" holds to rounding, not to the bit: omnitok_lm_set_prefill_attention above).  Fills the K/V cache, sets pos[b] = cache_len[b] = T on the
 * device.  logits_out (optional) [B, T, vocab]: teacher-forced logits of every position.
 * B * T <= 65535; may hipMalloc its (grow-only) workspace. */
int omnitok_lm_prefill(omnitok_lm *lm, const int64_t *idx, int32_t *pos, int32_t *cache_len, int B,
                       int T, float *logits_out, omnitok_stream_t stream);

/* ... with explicit embeddings prepended (GPT.forward(idx, embeddings=...), gpt.py:214-216): the sequence is
 * emb[B, T_emb, C] followed by tok_emb[idx[B, T_tok]], T = T_emb + T_tok positions; pos_extra [B, T, C] (optional)
 * is the vtokens_pos term added to the position embeddings (gpt.py:222-226).  logits_out [B, T, vocab]. */
int omnitok_lm_prefill_ex(omnitok_lm *lm, const int64_t *idx, int T_tok, const float *emb, int T_emb,
                          const float *pos_extra, int32_t *pos, int32_t *cache_len, int B,
                          float *logits_out, omnitok_stream_t stream);

/* Token cross-entropy and top-1 / top-5 hits of the reference's validation step (lm_transformer.py:308-321: F.cross_entropy and
 * utils.accuracy(topk=(1, 5))) in ONE read of the logits (csrc/lm_loss.hip).  logits [N, V] fp32 with row stride ld >= V (rows
 * need not be 16-byte aligned), targets int64 [N].  Per row i with t = targets[i]:
 *   t < 0    ignored: nll[i] = 0, rank[i] = -1, counted in no sum;
 *   t >= V   invalid: nll[i] = NaN, rank[i] = V, counted (the loss becomes NaN; nothing is read out of bounds);
 *   else     nll[i] = (m + log s) - l_t with m = max_j l_j, s = sum_j exp(l_j - m) in fp32;
 *            rank[i] = #{j : l_j > l_t} + #{j < t : l_j == l_t}: how many entries come before the target in a descending
 *            order with the lowest index first among equals (omnitok_lm_select's argmax convention).
 * sums[4] double = { sum of nll over the counted rows, counted rows, rows with rank == 0, rows with 0 <= rank < 5 }, added in
 * fp64 in a fixed order through `work` (no atomics: two calls give equal bits).  1 <= N <= 2^31, V >= 1; the grids are sized
 * from the CU count.  work: omnitok_lm_token_ce_workspace(N) bytes (-1 for an N outside the range), 8-byte aligned. */
int64_t omnitok_lm_token_ce_workspace(int64_t N);
int omnitok_lm_token_ce(const float *logits, int64_t ld, const int64_t *targets, int64_t N, int V, float *nll, int32_t *rank,
                        double *sums, void *work, int64_t work_bytes, omnitok_stream_t stream);

/* omnitok_lm_prefill_ex without the [B, T, vocab] logits tensor: the same layers, then ln_f, the head GEMM and the token
 * cross-entropy above over blocks of R rows into a grow-only R x vocab workspace; R = option "lm_loss_chunk_rows" (default 2048:
 * an UNMEASURED guess that keeps a block's logits inside the Infinity Cache).  With R >= B * T the head is the one GEMM call of
 * omnitok_lm_prefill_ex and every output equals omnitok_lm_token_ce on its logits bit for bit.  targets [B, T] int64 (< 0 =
 * ignored position); nll / rank [B, T] are optional (NULL: kept in the engine's workspace); sums [4] double as above, reduced once
 * over all B * T rows.  A block whose rows are all ignored skips its GEMM: the targets are copied to the host first, so the call
 * synchronises the stream once (and cannot be captured in a graph).  Fills the K/V cache like the prefill. */
int omnitok_lm_prefill_loss(omnitok_lm *lm, const int64_t *idx, int T_tok, const float *emb, int T_emb,
                            const float *pos_extra, const int64_t *targets, int32_t *pos, int32_t *cache_len, int B,
                            float *nll, int32_t *rank, double *sums, omnitok_stream_t stream);
/* bytes of the engine's loss workspace (the R x vocab logits block, per-row nll / rank, the reduction's partials) */
int64_t omnitok_lm_loss_workspace_bytes(omnitok_lm *lm);

/* Token selection of the sampling loops (gpt.py:347-357; CFG blend :428-431) for B streams, one workgroup each:
 *   v = logits / temperature,  or with logits_uncond:  v = cfg_c1 * (logits / T) - cfg_c2 * (logits_uncond / T)
 *   (cfg_c1 = 1 + t, cfg_c2 = t as fp32, the reference's roundings);
 *   top_k < 0: no filtering (the reference's top_k=None);  top_k >= 0: keep v >= k-th largest (0: all), then the
 *   nucleus top_p (1.0: off) as top_k_top_p_filtering (gpt.py:19-51);
 *   sample == 0: out[b] = argmax (lowest index on ties);  else one draw from softmax of the survivors by inverse
 *   CDF with the caller's uniform u[b] in [0, 1).
 * blend_out (optional) [B, V] receives v.  err_flag (optional) is set when more than 16384 values survive top_k
 * while a nucleus cut is requested (the LDS sort buffer; the argmax is returned then). */
int omnitok_lm_select(const float *logits, const float *logits_uncond, int B, int V, float temperature,
                      float cfg_c1, float cfg_c2, int top_k, float top_p, int sample, const float *u,
                      int64_t *out, float *blend_out, int *err_flag, omnitok_stream_t stream);

/* building blocks, exported for the parity tests */
/* y[b, n] = act(sum_k x[b, k] * w[n, k] + bias[n]) (+ residual[b, n]);  act: 0 none, 1 exact-erf
 * GELU (nn.GELU(), gpt.py:152).  B <= 16, K % 256 == 0.  If ln_gamma != NULL, x is layer-normalised
 * first (eps 1e-5, ln_gamma / ln_beta [K]): the LayerNorm of gpt.py:159/162/263 fused in.
 * residual may alias y. HBM-bound: streams w once for up to 8 rows of x. */
int omnitok_lm_gemv(const float *x, const float *w, const float *bias, const float *residual,
                    const float *ln_gamma, const float *ln_beta, float *y, int B, int N, int K,
                    int act, omnitok_stream_t stream);
/* omnitok_lm_gemv over a packed 16-bit weight matrix w16 [N, K] (fmt = OMNITOK_LM_W_BF16 | OMNITOK_LM_W_FP16, 16-byte aligned;
 * anything else returns -1): each weight is widened to fp32 in registers, then the same fmaf chains into fp32 accumulators.
 * Same contract otherwise. */
int omnitok_lm_gemv_w16(const float *x, const void *w16, int fmt, const float *bias, const float *residual,
                        const float *ln_gamma, const float *ln_beta, float *y, int B, int N, int K, int act,
                        omnitok_stream_t stream);
/* omnitok_lm_gemv over an fp8 weight matrix q8 [N, K] (e4m3fn bytes, 16-byte aligned) with one fp32 scale per output row, scale [N]
 * (powers of two, as omnitok_lm_quantize_fp8 writes them): y[b, n] = act(scale[n] * sum_k x[b, k] * float(q8[n, k]) + bias[n])
 * (+ residual[b, n]).  Each byte is widened to fp32 in registers (exact, subnormals and +-0 included), then the same fmaf chains into
 * fp32 accumulators; the scale multiplies the finished sum once, in front of the bias (exact for a power of two).  Same contract and
 * argument checks otherwise (null pointers -- scale included --, unaligned x / q8, K % 256, B <= 16: -1 before any HIP call). */
int omnitok_lm_gemv_fp8(const float *x, const void *q8, const float *scale, const float *bias, const float *residual,
                        const float *ln_gamma, const float *ln_beta, float *y, int B, int N, int K, int act,
                        omnitok_stream_t stream);
/* The quantiser of omnitok_lm_set_decode_quant alone: w [N, K] fp32 -> q8 [N, K] e4m3fn bytes and scale [N] by the rule stated
 * there.  K % 4 == 0; w and q8 16-byte aligned; -1 for null pointers (flag may be NULL), sizes outside these or unaligned pointers,
 * before any HIP call.  *flag (an int on the device) is SET to 1 if w holds a NaN or an infinity and left alone otherwise; what q8
 * and scale hold for the rows of such an element is not specified. */
int omnitok_lm_quantize_fp8(const float *w, void *q8, float *scale, int N, int K, int *flag, omnitok_stream_t stream);
/* The many-stream form: y[B, N] = act(LN(x)[B, K] . w[N, K]^T + bias) (+ residual) for 1 <= B <= 128 in one pass over w, which is
 * fp32, bf16 or fp16 (fmt = OMNITOK_LM_W_FP32 | _BF16 | _FP16; 16-byte aligned like x and y).  N >= 1, K % 256 == 0; -1 for null
 * pointers, unaligned pointers, sizes outside these or an unknown fmt, before any HIP call.  Every product is an fp32 product of an
 * fp32 activation and the weight's exact fp32 value (16-bit weights are widened in registers) accumulated in fp32 on the f32-input
 * MFMA, the partial sums of a dot product joined in an order fixed by (N, K): row b of y depends on row b of x only, and its bits do
 * not change with B, with the row's slot or with the other rows' contents (NaN / Inf included); two calls give equal bits.  LayerNorm
 * (eps 1e-5) is a pass of its own in front; bias, exact-erf GELU and residual as omnitok_lm_gemv; residual may alias y.
 * B < option "lm_streams_min" (default 17) is served by the kernels of omnitok_lm_gemv / _w16 in groups of up to 8 rows instead.
 * Uses a process-wide grow-only scratch (may hipMalloc): calls on different streams must not overlap. */
int omnitok_lm_gemm_streams(const float *x, const void *w, int fmt, const float *bias, const float *residual,
                            const float *ln_gamma, const float *ln_beta, float *y, int B, int N, int K, int act,
                            omnitok_stream_t stream);
/* The GEMM of an OMNITOK_LM_SF_W16 many-stream step: y[B, N] = act(a16[B, K] . w16[N, K]^T + bias) (+ residual) for 1 <= B <= 128 in
 * one pass over w16, with a16 and w16 packed bf16 or fp16 (fmt = OMNITOK_LM_W_BF16 | OMNITOK_LM_W_FP16), row-major, on
 * v_mfma_f32_32x32x16_{bf16,f16}: exact products, fp32 accumulators.  N >= 1, K % 64 == 0.  Always this kernel: no routing to the
 * <= 16-stream kernels, no dependence on "lm_streams_min".  The partial sums of a dot product are joined in an order fixed by (N, K):
 * row b of y depends on row b of a16 only -- its bits do not change with B, with the row's slot or with the other rows' contents (NaN /
 * Inf included) -- and two calls give equal bits.  Epilogue in fp32: + bias [N] (optional), exact-erf GELU if act == 1, then
 *   y32 != NULL: + residual [B, N] (optional, may alias y32), stored as fp32; or
 *   y16 != NULL: rounded to fmt (round to nearest even) into a packed [B, N]; no residual in this form.  An fp16 element that rounds to
 *     +-inf ORs 16 into *flag (flag may be NULL; bf16 never sets it).
 * Exactly one of y32 / y16.  -1 before any HIP call for null or non-16-byte-aligned pointers, sizes outside the above, an unknown fmt or
 * act, both or neither output, or a residual with y16.  Uses a process-wide grow-only scratch (may hipMalloc): calls on different
 * streams must not overlap. */
int omnitok_lm_gemm_streams16(const void *a16, const void *w16, int fmt, const float *bias, const float *residual,
                              float *y32, void *y16, int B, int N, int K, int act, int *flag, omnitok_stream_t stream);
/* The GEMM of an OMNITOK_LM_PF_W16 prefill: y[M, N] = act(a16[M, K] . w16[N, K]^T + bias) (+ residual) with a16 and w16 packed bf16 or
 * fp16 (fmt = OMNITOK_LM_W_BF16 | OMNITOK_LM_W_FP16), row-major, 16-byte aligned, on v_mfma_f32_32x32x16_{bf16,f16}: exact products,
 * fp32 accumulators.  1 <= M <= 65535, N >= 1, K % 32 == 0.  The partial sums of a dot product are joined in k order, an order fixed
 * by K alone: row m of y depends on row m of a16 only -- not on M, the row's position or the other rows' contents (NaN / Inf included)
 * -- and two calls give equal bits.  Epilogue in fp32: + bias [N] (optional), exact-erf GELU if act == 1, then
 *   y32 != NULL: + residual [M, N] (optional, may alias y32), stored as fp32; or
 *   y16 != NULL: rounded to fmt (round to nearest even, the bits of torch's .to()) into a packed [M, N] -- the next GEMM's operand; no
 *     residual in this form.  An fp16 element that rounds to +-inf ORs 4 into *flag (flag may be NULL; bf16 never sets it).
 * Exactly one of y32 / y16.  -1 before any HIP call for null or unaligned pointers, sizes outside the above, an unknown fmt or act,
 * both or neither output, or a residual with y16. */
int omnitok_lm_gemm16(const void *a16, const void *w16, int fmt, const float *bias, const float *residual,
                      float *y32, void *y16, int64_t M, int N, int K, int act, int *flag, omnitok_stream_t stream);
/* nn.LayerNorm (eps 1e-5, two-pass statistics in fp32: the arithmetic of the fp32 prefill's LayerNorm) of x [rows, K] fp32 with each
 * result rounded once to fmt into y16 [rows, K] packed: the producer of omnitok_lm_gemm16's A operand.  All four pointers 16-byte
 * aligned, rows >= 1, K % 32 == 0; an fp16 element that rounds to +-inf ORs 4 into *flag (may be NULL).  -1 before any HIP call for
 * null or unaligned pointers, sizes outside these or an unknown fmt. */
int omnitok_lm_layernorm16(const float *x, const float *gamma, const float *beta, void *y16, int fmt,
                           int64_t rows, int K, int *flag, omnitok_stream_t stream);
/* Decode attention for one layer: qkv[B, 3*C] = (query | key | value) of the new token; K/V cache of
 * this layer kc / vc [max_batch][n_head][max_len][head_dim]; out[B, C].  scratch: float
 * [B * n_head * ceil(max_len/256) * (2 + head_dim)]. */
int omnitok_lm_attn_decode(const float *qkv, float *kc, float *vc, const int32_t *cache_len, int B,
                           int n_head, int head_dim, int max_len, float *scratch, float *out,
                           omnitok_stream_t stream);
/* omnitok_lm_attn_decode over packed 16-bit caches kc16 / vc16 [max_batch][n_head][max_len][head_dim] (fmt = OMNITOK_LM_KV_BF16 |
 * OMNITOK_LM_KV_FP16; anything else returns -1; 16-byte aligned, otherwise -1 "unaligned"): cached rows are widened to fp32 in
 * registers, the new token's row is appended rounded to fmt.  Same contract otherwise; out equals omnitok_lm_attn_decode's on
 * fp32 caches that hold the widened values, bit for bit. */
int omnitok_lm_attn_decode_kv16(const float *qkv, void *kc16, void *vc16, int fmt, const int32_t *cache_len, int B,
                                int n_head, int head_dim, int max_len, float *scratch, float *out,
                                omnitok_stream_t stream);
/* omnitok_lm_attn_decode over fp8 caches (OMNITOK_LM_KQ_FP8): kc8 / vc8 [max_batch][n_head][max_len][head_dim] e4m3fn bytes and
 * kscale / vscale [max_batch][n_head][max_len] fp32 row scales.  Cached rows enter as widen(q) * s, the new token's rows are appended
 * quantised by omnitok_lm_set_cache_quant's rule (bytes and scale).  -1 before any HIP call: null pointers (the scales included),
 * head_dim not 64 | 96 | 128, qkv / kc8 / vc8 not 16-byte aligned ("unaligned"), bad sizes.  Same contract otherwise; out equals
 * omnitok_lm_attn_decode's on fp32 caches that hold s * widen(q), bit for bit.  (There is no flag word here: a non-finite row is
 * reported by the engine only.) */
int omnitok_lm_attn_decode_kv8(const float *qkv, void *kc8, void *vc8, float *kscale, float *vscale,
                               const int32_t *cache_len, int B, int n_head, int head_dim, int max_len,
                               float *scratch, float *out, omnitok_stream_t stream);
/* Causal attention of a batched prefill (the OMNITOK_LM_PA_TILED mode).  qkv [B*T, 3C] fp32 (query | key | value), C = n_head * head_dim,
 * head_dim 64, 96 or 128.  Row b*T + t attends to rows b*T .. b*T + t of its own stream.
 * Exactly one of out32 [B*T, C] fp32 / out16 [B*T, C] packed (fmt = OMNITOK_LM_W_BF16 | _FP16, the value rounded
 * once by lm_round16; an fp16 result of +-inf ORs 4 into *flag, which may be NULL).
 * Arithmetic: score = (q . k) * (1.0f / sqrtf(head_dim)), the dot product ONE fmaf chain from 0 on v_mfma_f32_32x32x2_f32 (dims in the
 * fixed order 0 4 1 5 2 6 3 7 | 8 12 ...), the scale applied to the finished dot; keys after the query's position are -inf before the
 * softmax; online softmax over 32-key tiles anchored at key 0 of the stream, ascending, expf in fp32; P . V on the same MFMA with
 * fp32 P (per tile the keys are added in the fixed order 0 4 1 5 2 6 3 7 | 8 12 ...); out = O / l, one division per element.  No
 * atomics, no split over keys across workgroups, no partials: needs no scratch.
 * Determinism: row (b, t) depends only on t and on the qkv rows of its own stream up to the end of its diagonal 32-key tile (rows
 * 0 .. min(32 (t / 32) + 31, T - 1)) -- not on B, T, the stream's slot or other streams' contents (NaN / Inf included) -- and two
 * calls give equal values (a masked key adds 0 * v, which may turn a -0 sum into +0: equal as numbers, torch.equal).
 * One limit, stated and not fixed: a masked key's V row enters the MFMA with weight 0, so a NON-FINITE V in a later row of the same
 * diagonal tile of the same stream turns the earlier rows of that tile into NaN, where the rows kernel skips it.
 * -1 before any HIP call for null or non-16-byte-aligned pointers, B < 1, T < 1, B * T > 65535, n_head outside 1 .. 1024, an
 * unsupported head_dim, both or neither output, or an unknown fmt with out16. */
int omnitok_lm_attn_prefill(const float *qkv, int B, int T, int n_head, int head_dim, float *out32, void *out16, int fmt,
                            int *flag, omnitok_stream_t stream);
/* The same attention with 16-bit operands (omnitok_lm_set_prefill_attention_operands): qkv, B, T, n_head, head_dim, out32 / out16 /
 * out_fmt and the argument checks as omnitok_lm_attn_prefill; op_fmt = OMNITOK_LM_W_BF16 | _FP16 is the operand format (any other value:
 * -1, "op_fmt" in the message).
 * Arithmetic: every element of Q, K and V rounded ONCE to op_fmt (lm_round16's bits) where it is staged; score = (q . k) * (1 / sqrt(head_dim))
 * with exact 16-bit products accumulated in fp32 on v_mfma_f32_32x32x16_bf16 / _f16, the scale applied to the finished dot (as ONE
 * fp32 constant log2(e) / sqrt(head_dim): the scores are kept in base 2); keys after the query's position are -inf before the
 * softmax; online softmax over key tiles of KT = 32 anchored at key 0 of the stream, ascending, with fp32 running max, sum and
 * rescale; the weight is v_exp_f32 of an fp32 difference (documented error 1 ulp); l sums the weights BEFORE their rounding; P is
 * rounded ONCE to op_fmt on its way into the P . V MFMA (fp32 accumulation); out = O / l, one division per element, fp32 or rounded
 * once to out_fmt.  No atomics on the result, no split over keys across workgroups, no partials: needs no scratch.
 * Determinism and the one limit (a non-finite V in a masked key of the diagonal tile): as omnitok_lm_attn_prefill.
 * *flag (may be NULL): an fp16 OPERAND that rounds to +-inf ORs 8, an fp16 OUTPUT of +-inf ORs 4; bf16 sets neither. */
int omnitok_lm_attn_prefill16(const float *qkv, int B, int T, int n_head, int head_dim, int op_fmt, float *out32, void *out16,
                              int out_fmt, int *flag, omnitok_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* OMNITOK_LM_H */
