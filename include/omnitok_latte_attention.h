/* omnitok_latte_attention.h -- the attention format of the Latte engine; part of omnitok_latte.h, which includes it.
 *
 * The DiT engine's switch (OMNITOK_DIT_ATTN_FP32 | _BF16 | _FP16, omnitok_dit.h: independent of the linear format, -1 before any HIP
 * call for a null engine or an unknown format, a refused value changes nothing, `finalized` untouched, the fp16 range rule) under
 * this engine's name.  It covers the attention of the SPATIAL blocks, which under a 16-bit format is omnitok_dit_attn16 over the B F
 * frames; with a 16-bit linear format as well it writes the packed operand of attn.proj itself.  The temporal attention stays fp32
 * under every format, with the round pass of a 16-bit linear format behind it.
 */
#ifndef OMNITOK_LATTE_ATTENTION_H
#define OMNITOK_LATTE_ATTENTION_H

#include "omnitok_latte.h"

#ifdef __cplusplus
extern "C" {
#endif

int omnitok_latte_set_attention_format(omnitok_latte *e, int fmt);
int omnitok_latte_attention_format(omnitok_latte *e); /* -1: null engine */

#ifdef __cplusplus
}
#endif

#endif /* OMNITOK_LATTE_ATTENTION_H */
