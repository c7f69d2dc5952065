/* omnitok_latte_linear.h -- the linear format of the Latte engine; part of omnitok_latte.h, which includes it.
 *
 * The DiT engine's switch (OMNITOK_DIT_LIN_FP32 | _BF16 | _FP16, omnitok_dit.h: what is rounded and where, what stays fp32, the
 * return values, the fp16 range rules) under this engine's name.  It covers the four linears of BOTH kinds of block; under the
 * default attention format the spatial and the temporal attention stay fp32 and their output is rounded once in front of attn.proj.
 * (omnitok_latte_attention.h: the attention format, under which the spatial attention writes that operand itself.)
 */
#ifndef OMNITOK_LATTE_LINEAR_H
#define OMNITOK_LATTE_LINEAR_H

#include "omnitok_latte.h"

#ifdef __cplusplus
extern "C" {
#endif

int omnitok_latte_set_linear_format(omnitok_latte *e, int fmt);
int omnitok_latte_linear_format(omnitok_latte *e); /* -1: null engine */

#ifdef __cplusplus
}
#endif

#endif /* OMNITOK_LATTE_LINEAR_H */
