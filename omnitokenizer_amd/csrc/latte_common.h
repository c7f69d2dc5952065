// Latte video denoiser (include/omnitok_latte.h): the class-conditional / unconditional video diffusion transformer of the
// reference's video-generation pipeline (Diffusion/Latte/models/latte.py:209-403).  Latte is the DiT with alternating blocks: the
// even ones attend over the tokens of a frame, the odd ones over the frames of a token position.
//
// Which unit holds what:
//   latte_common.h    this index
//   latte_attn.hip    latte_attn_temporal_kernel: attention over the F <= 32 frames of every (sample, position, head), read from
//                     and written to rows N apart -- nothing is rearranged (omnitok_latte_attn_temporal)
//   latte_ops.hip     the temp_embed add and the exported form of the guidance blend with a channel count
//   latte_engine.hip  struct omnitok_latte and its exported functions (create .. finalize, forward, forward_cfg, the linear format
//                     and the attention format: the latter covers the spatial blocks only, the temporal attention stays fp32)
// Everything else is the DiT's (index: dit_common.h): its operators serve both kinds of block with n_tokens = F N rows per sample,
// its spatial attention runs over B F "samples" of N tokens, and dit_scaffold.h is the host-side scaffold of both engines.
#pragma once
#include "dit_common.h"
#include "../../include/omnitok_latte.h"

namespace omnitok {

constexpr int LATTE_F_MAX = 32;  // frames of one temporal sequence (latte_attn.hip's LDS image and its row-max lanes)

}  // namespace omnitok
