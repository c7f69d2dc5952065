"""ctypes binding of include/omnitok.h (libomnitok.so).

The HIP library is the product: if it is missing or fails to load this module raises -- there is
no CPU or PyTorch fallback anywhere in the package.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, Structure, c_char, c_char_p, c_float, c_int, c_int64, c_void_p

HERE = os.path.dirname(os.path.abspath(__file__))
# OMNITOK_LIB: another build of the same library (an experiment build compiled with extra flags, tools/ab_bench.sh)
LIB_PATH = os.environ.get("OMNITOK_LIB") or os.path.join(HERE, "lib", "libomnitok.so")


class OmnitokConfig(Structure):
    _fields_ = [
        ("resolution", c_int), ("image_channels", c_int), ("patch_size", c_int),
        ("temporal_patch_size", c_int), ("dim", c_int), ("heads", c_int), ("dim_head", c_int),
        ("ff_inner", c_int), ("window_size", c_int), ("n_codes", c_int), ("codebook_dim", c_int),
        ("l2_code", c_int), ("spatial_rope", c_int), ("legacy_attention", c_int),
        ("causal_temporal", c_int), ("causal_peg", c_int), ("temporal_depth", c_int),
        ("enc_block", c_char * 16), ("dec_block", c_char * 16), ("use_vae", c_int),
        ("patch_embed_cnn", c_int), ("defer_temporal_pool", c_int), ("defer_spatial_pool", c_int),
        ("gen_upscale", c_int), ("external_codebook", c_int),
    ]


class OmnitokLmConfig(Structure):
    _fields_ = [("vocab_size", c_int), ("block_size", c_int), ("n_layer", c_int), ("n_head", c_int),
                ("n_embd", c_int)]


class OmnitokDitConfig(Structure):
    """omnitok_dit_config (include/omnitok_dit.h)."""
    _fields_ = [("input_size", c_int), ("patch_size", c_int), ("in_channels", c_int), ("hidden", c_int), ("depth", c_int),
                ("heads", c_int), ("mlp_hidden", c_int), ("num_classes", c_int), ("class_dropout", c_float),
                ("learn_sigma", c_int)]


class OmnitokLatteConfig(Structure):
    """omnitok_latte_config (include/omnitok_latte.h): the DiT's fields, then num_frames and extras."""
    _fields_ = OmnitokDitConfig._fields_ + [("num_frames", c_int), ("extras", c_int)]


class OmnitokPlGemm(Structure):
    """omnitok_pl_gemm (include/omnitok.h): arguments of the plane x plane GEMM."""
    _fields_ = [
        ("a", c_void_p), ("a_scale", c_void_p), ("a_scale_const", c_float),
        ("a2", c_void_p), ("a2_scale", c_void_p), ("a2_scale_const", c_float), ("a_split_n", c_int),
        ("w", c_void_p), ("w_scale", c_void_p), ("bias", c_void_p), ("residual", c_void_p), ("ldr", c_int64),
        ("c", c_void_p), ("ldc", c_int64), ("c2", c_void_p), ("ldc2", c_int64), ("c_split_n", c_int),
        ("out_planes", c_void_p), ("out_planes_k", c_int), ("out_bound", c_float),
        ("ln_gamma", c_void_p), ("ln_beta", c_void_p), ("ln_eps", c_float), ("epilogue", c_int),
        ("fold_stats", c_void_p), ("fold_b", c_void_p), ("fold_u", c_void_p), ("fold_cols", c_int),
        ("qp", c_void_p), ("kp", c_void_p), ("vp", c_void_p), ("qk_k0", c_int), ("n_tokens", c_int), ("heads", c_int),
        ("rope_cos", c_void_p), ("rope_sin", c_void_p), ("q_scale", c_void_p), ("k_scale", c_void_p),
        ("q_mul", c_float), ("q_bound", c_float), ("k_bound", c_float), ("v_bound", c_float),
        ("v_bound_dev", c_void_p), ("v_bound_stride", c_int), ("rows_per_clip", c_int64),
        ("M", c_int64), ("N", c_int), ("K", c_int), ("cfg", c_int), ("debug_cycles", c_void_p),
        ("a_rpg", c_int64), ("a_gstride", c_int64), ("a_goff", c_int64),
        ("up_C", c_int), ("up_F", c_int), ("up_H", c_int), ("up_W", c_int), ("up_f0", c_int), ("up_t", c_int),
        ("up_pt", c_int), ("up_p", c_int), ("k_valid", c_int),
        ("tp", c_void_p), ("t_nseq", c_int), ("t_heads", c_int), ("t_seqs_per_clip", c_int), ("t_alibi", c_void_p),
        ("t_out_scale", c_void_p),
    ]


class OmnitokRowGemm(Structure):
    """omnitok_row_gemm (include/omnitok.h): arguments of omnitok_gemm / omnitok_gemm_x3 / omnitok_gemm_h2."""
    _fields_ = [
        ("a", c_void_p), ("lda", c_int64), ("w", c_void_p), ("ldw", c_int64), ("w_planes", c_void_p), ("w_scale", c_void_p),
        ("bias", c_void_p), ("residual", c_void_p), ("ldr", c_int64), ("c", c_void_p), ("ldc", c_int64),
        ("M", c_int64), ("N", c_int), ("K", c_int), ("flags", c_int),
        ("a_rows_per_group", c_int64), ("a_group_stride", c_int64), ("a_group_offset", c_int64),
        ("a_bound", c_float), ("a_bound_dev", c_void_p), ("a_bound_stride", c_int), ("a_rows_per_clip", c_int64),
        ("ln_stats", c_void_p), ("ln_gamma", c_void_p), ("ln_beta", c_void_p), ("ln_cols", c_int), ("ln_bound", c_float),
        ("c2", c_void_p), ("ldc2", c_int64), ("split_col", c_int),
        ("v_planes", c_void_p), ("v_col0", c_int), ("n_tokens", c_int), ("heads", c_int), ("v_bound", c_float),
        ("v_bound_dev", c_void_p), ("v_bound_stride", c_int),
    ]


class OmnitokAttnDesc(Structure):
    """omnitok_attn_desc (include/omnitok.h): arguments of omnitok_qk_prep and the omnitok_attn_* entry points."""
    _fields_ = [
        ("q", c_void_p), ("ldq", c_int64), ("k", c_void_p), ("v", c_void_p), ("ldkv", c_int64),
        ("qp", c_void_p), ("kp", c_void_p), ("vp", c_void_p),
        ("rope_cos", c_void_p), ("rope_sin", c_void_p), ("q_scale", c_void_p), ("k_scale", c_void_p), ("scale", c_float),
        ("q_bound", c_float), ("k_bound", c_float), ("v_bound", c_float), ("v_bound_dev", c_void_p),
        ("v_bound_stride", c_int), ("seqs_per_clip", c_int64),
        ("bias_table", c_void_p), ("bias_dense", c_void_p), ("alibi_slopes", c_void_p), ("causal", c_int),
        ("out", c_void_p), ("ldo", c_int64), ("out_planes", c_void_p), ("out_scale", c_void_p), ("out_bound", c_float),
        ("seqs", c_int64), ("n_tokens", c_int), ("heads", c_int), ("gh", c_int), ("gw", c_int),
    ]


class OmnitokFramesDesc(Structure):
    """omnitok_frames_desc (include/omnitok.h): one uint8 clip of omnitok_frames_to_pixels."""
    _fields_ = [("frames", c_void_p), ("frame_stride", c_int64), ("row_stride", c_int64),
                ("F", c_int), ("H", c_int), ("W", c_int), ("frame_start", c_int), ("frame_step", c_int),
                ("crop_top", c_int), ("crop_left", c_int), ("resize_h", c_int), ("resize_w", c_int)]


class OmnitokMetricsOperand(Structure):
    """omnitok_metrics_operand (include/omnitok.h): one video of omnitok_frame_metrics."""
    _fields_ = [("data", c_void_p), ("stride", c_int64 * 5), ("dtype", c_int), ("clamp", c_int), ("shift", c_float)]


class OmnitokConv3d(Structure):
    """omnitok_conv3d (include/omnitok.h): one Unit3D of the I3D net."""
    _fields_ = [("x", c_void_p), ("x_cs", c_int64), ("x_off", c_int), ("B", c_int), ("T", c_int), ("H", c_int),
                ("W", c_int), ("Cin", c_int), ("w", c_void_p), ("bias", c_void_p), ("Cout", c_int), ("kt", c_int),
                ("kh", c_int), ("kw", c_int), ("st", c_int), ("sh", c_int), ("sw", c_int), ("relu", c_int),
                ("y", c_void_p), ("y_cs", c_int64), ("y_off", c_int), ("y2", c_void_p), ("y2_cs", c_int64),
                ("y2_off", c_int), ("split", c_int)]


class OmnitokConv2d(Structure):
    """omnitok_conv2d_desc (include/omnitok.h): one BasicConv2d of the Inception V3 net."""
    _fields_ = [("x", c_void_p), ("x_cs", c_int64), ("x_off", c_int), ("N", c_int), ("H", c_int), ("W", c_int),
                ("Cin", c_int), ("w", c_void_p), ("bias", c_void_p), ("Cout", c_int), ("kh", c_int), ("kw", c_int),
                ("sh", c_int), ("sw", c_int), ("ph", c_int), ("pw", c_int), ("relu", c_int), ("y", c_void_p),
                ("y_cs", c_int64), ("y_off", c_int), ("y2", c_void_p), ("y2_cs", c_int64), ("y2_off", c_int),
                ("split", c_int)]


class OmnitokError(RuntimeError):
    pass


P = c_void_p
I64 = c_int64

# name -> argtypes (restype is int unless listed in _RESTYPES); mirrors include/omnitok.h
_PROTOS = {
    "omnitok_layernorm": [P, P, P, P, I64, c_int, c_float, I64, I64, I64, P],
    "omnitok_gemm": [POINTER(OmnitokRowGemm), P],
    "omnitok_gemm_x3": [POINTER(OmnitokRowGemm), P],
    "omnitok_h2_pack_weight": [P, I64, c_int, c_int, P, P, P],
    "omnitok_gemm_h2": [POINTER(OmnitokRowGemm), P],
    "omnitok_row_stats": [P, I64, c_int, c_float, P, P, I64, P],
    "omnitok_weight_range": [P, I64, c_int, c_int, P, P],
    "omnitok_pack_geglu_weight": [P, c_int, c_int, c_int, P, P],
    "omnitok_patchify_ln": [P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, P, c_float, P, I64, P],
    "omnitok_unpatchify": [P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, P],
    "omnitok_peg3d": [P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, P],
    "omnitok_pack_peg_weight": [P, c_int, P, P],
    "omnitok_transpose_tokens": [P, P, I64, I64, I64, c_int, P],
    "omnitok_rope_table": [c_int, c_int, c_float, P, P],
    **{name: [POINTER(OmnitokAttnDesc), P] for name in (
        "omnitok_qk_prep", "omnitok_attn_spatial", "omnitok_attn_pack", "omnitok_attn_spatial_h2", "omnitok_attn_window",
        "omnitok_attn_window_h2", "omnitok_attn_temporal")},
    "omnitok_pre_vq": [P, P, P, P, I64, c_int, c_int, c_int, P],
    "omnitok_vq_prepare": [P, c_int, c_int, P, P, P],
    "omnitok_vq_argmin": [P, P, P, I64, c_int, P, P],
    "omnitok_vq_screen_prepare": [P, P, c_int, c_int, P, P],
    "omnitok_vq_argmin_screened": [P, P, P, P, I64, c_int, P, P],
    "omnitok_vq_argmax_cos": [P, P, I64, c_int, P, P],
    "omnitok_vq_argmin_cdist": [P, P, P, I64, c_int, P, P],
    "omnitok_dequant_post_vq": [P, P, c_int, c_int, P, P, P, I64, c_int, P, P],
    "omnitok_dequant_table": [P, c_int, c_int, P, P, P, c_int, P, P],
    "omnitok_gather_rows": [P, P, c_int, P, I64, c_int, P, P],
    "omnitok_gather_rows_transposed": [P, P, c_int, P, I64, c_int, c_int, c_int, P, P],
    "omnitok_layernorm_transposed": [P, P, P, P, I64, c_int, c_int, c_int, c_float, P],
    "omnitok_layernorm_prevq": [P, P, P, P, P, P, I64, c_int, c_int, c_int, c_float, c_int, c_int, P],
    "omnitok_token_resample": [P, P, c_int, I64, c_int, c_int, c_int, c_int, P],
    "omnitok_vae_sample": [P, P, P, P, P, P, I64, I64, c_int, c_int, P],
    "omnitok_post_vq": [P, c_int, I64, I64, c_int, P, P, P, c_int, P],
    "omnitok_vq_embed_st": [P, P, P, c_int, I64, I64, P, P],
    "omnitok_vq_stats": [P, I64, c_int, P, P, P, c_int, c_float, P, P],
    "omnitok_engine_create": [POINTER(OmnitokConfig), POINTER(P)],
    "omnitok_engine_destroy": [P],
    "omnitok_engine_set_weight": [P, c_char_p, P, POINTER(I64), c_int, c_int, P],
    "omnitok_engine_finalize": [P, P],
    "omnitok_engine_missing": [P, c_char_p, c_int],
    "omnitok_encode": [P, P, c_int, c_int, c_int, c_int, P, P, P, P],
    "omnitok_decode": [P, P, c_int, c_int, c_int, c_int, P, P],
    "omnitok_encode_vae": [P, P, c_int, c_int, c_int, c_int, P, P, P, P],
    "omnitok_decode_vae": [P, P, c_int, c_int, c_int, c_int, c_int, P, P],
    "omnitok_engine_encode_shape": [P, c_int, c_int, c_int, POINTER(c_int), POINTER(c_int), POINTER(c_int)],
    "omnitok_engine_decode_shape": [P, c_int, c_int, c_int, POINTER(c_int), POINTER(c_int), POINTER(c_int)],
    "omnitok_engine_check_ids": [P, P],
    "omnitok_engine_workspace_bytes": [P],
    "omnitok_engine_workspace_need_encode": [P, c_int, c_int, c_int, c_int],
    "omnitok_engine_workspace_need_decode": [P, c_int, c_int, c_int, c_int],
    "omnitok_engine_set_workspace": [P, P, I64],
    "omnitok_engine_set_timing": [P, c_int],
    "omnitok_engine_set_option": [P, c_char_p, c_int],
    "omnitok_engine_timing_report": [P, c_char_p, c_int],
    "omnitok_frames_to_pixels": [POINTER(OmnitokFramesDesc), c_int, c_int, c_int, c_int, c_int, c_int, P, P, P],
    "omnitok_pixels_to_frames": [P, c_int, c_int, c_int, c_int, c_int, c_int, P, P],
    "omnitok_frames_resize_pil_workspace": [POINTER(OmnitokFramesDesc), c_int, c_int, c_int],
    "omnitok_frames_resize_pil": [POINTER(OmnitokFramesDesc), c_int, c_int, c_int, c_int, c_int, c_int, P, I64, P, P],
    "omnitok_pil_resize_coeffs": [c_int, c_int, c_int, POINTER(c_int), P, P],
    "omnitok_frame_metrics_workspace": [c_int, c_int, c_int, c_int],
    "omnitok_frame_metrics": [POINTER(OmnitokMetricsOperand), POINTER(OmnitokMetricsOperand), c_int, c_int, c_int, c_int,
                              c_int, P, P, P, ctypes.c_size_t, P],
    "omnitok_same_pad": [c_int, c_int, c_int, POINTER(c_int), POINTER(c_int)],
    "omnitok_i3d_preprocess": [P, c_int, c_int, c_int, c_int, c_int, c_int, P, P],
    "omnitok_conv3d_packed_ldw": [c_int, c_int, c_int, c_int],
    "omnitok_conv3d_same": [POINTER(OmnitokConv3d), P],
    "omnitok_maxpool3d_same": [P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, P],
    "omnitok_i3d_head": [P, c_int, c_int, c_int, c_int, c_int, P, P, c_int, P, P],
    "omnitok_fid_preprocess": [P, c_int, c_int64, c_int, c_int, c_int, c_int, c_int, c_int, P, P],
    "omnitok_conv2d_out": [c_int, c_int, c_int, c_int],
    "omnitok_conv2d": [POINTER(OmnitokConv2d), P],
    "omnitok_maxpool2d": [P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, c_int64, c_int, P],
    "omnitok_avgpool2d": [P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, c_int64, c_int, P],
    "omnitok_spatial_mean": [P, c_int, c_int, c_int, c_int, P, P],
    "omnitok_lpips_preprocess": [POINTER(OmnitokMetricsOperand), c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, P, P,
                                 P],
    "omnitok_lpips_workspace": [c_int, c_int, c_int],
    "omnitok_lpips_layer": [P, c_int, c_int, c_int, c_int, P, c_int, P, ctypes.c_size_t, P, P],
    "omnitok_lpips_finalize": [P, c_int, P, P],
    "omnitok_losses_workspace": [c_int],
    "omnitok_recon_losses": [P, P, c_int, I64, c_int, P, P, P, ctypes.c_size_t, P],
    "omnitok_commitment_sum": [P, P, P, I64, c_int, c_int, P, P, ctypes.c_size_t, P],
    "omnitok_kl_sum": [P, c_int, I64, P, P, P, ctypes.c_size_t, P],
    # include/omnitok_lm.h
    "omnitok_lm_create": [POINTER(OmnitokLmConfig), POINTER(P)],
    "omnitok_lm_destroy": [P],
    "omnitok_lm_set_weight": [P, c_char_p, P, POINTER(I64), c_int, P],
    "omnitok_lm_finalize": [P, P],
    "omnitok_lm_set_weight_format": [P, c_int],
    "omnitok_lm_weight_format": [P],
    "omnitok_lm_step_weight_bytes": [P],
    "omnitok_lm_set_decode_quant": [P, c_int],
    "omnitok_lm_decode_quant": [P],
    "omnitok_lm_set_cache_format": [P, c_int],
    "omnitok_lm_cache_format": [P],
    "omnitok_lm_set_cache_quant": [P, c_int],
    "omnitok_lm_cache_quant": [P],
    "omnitok_lm_set_streams_format": [P, c_int],
    "omnitok_lm_streams_format": [P],
    "omnitok_lm_set_prefill_format": [P, c_int],
    "omnitok_lm_prefill_format": [P],
    "omnitok_lm_set_prefill_attention": [P, c_int],
    "omnitok_lm_prefill_attention": [P],
    "omnitok_lm_set_prefill_attention_operands": [P, c_int],
    "omnitok_lm_prefill_attention_operands": [P],
    "omnitok_lm_set_max_streams": [P, c_int],
    "omnitok_lm_max_streams": [P],
    "omnitok_lm_cache_read": [P, c_int, c_int, c_int, c_int, P, P, P],
    "omnitok_lm_alloc_cache": [P, c_int, c_int],
    "omnitok_lm_cache_bytes": [P],
    "omnitok_lm_overflowed": [P, P],
    "omnitok_lm_step": [P, P, P, P, c_int, P, c_int, P],
    "omnitok_lm_prefill": [P, P, P, P, c_int, c_int, P, P],
    "omnitok_lm_step_ex": [P, P, P, P, P, P, c_int, P, c_int, P],
    "omnitok_lm_prefill_ex": [P, P, c_int, P, c_int, P, P, P, c_int, P, P],
    "omnitok_lm_token_ce_workspace": [I64],
    "omnitok_lm_token_ce": [P, I64, P, I64, c_int, P, P, P, P, I64, P],
    "omnitok_lm_prefill_loss": [P, P, c_int, P, c_int, P, P, P, P, c_int, P, P, P, P],
    "omnitok_lm_loss_workspace_bytes": [P],
    "omnitok_lm_select": [P, P, c_int, c_int, c_float, c_float, c_float, c_int, c_float, c_int, P, P, P, P, P],
    "omnitok_lm_gemv": [P, P, P, P, P, P, P, c_int, c_int, c_int, c_int, P],
    "omnitok_lm_gemv_w16": [P, P, c_int, P, P, P, P, P, c_int, c_int, c_int, c_int, P],
    "omnitok_lm_gemv_fp8": [P, P, P, P, P, P, P, P, c_int, c_int, c_int, c_int, P],
    "omnitok_lm_quantize_fp8": [P, P, P, c_int, c_int, P, P],
    "omnitok_lm_gemm_streams": [P, P, c_int, P, P, P, P, P, c_int, c_int, c_int, c_int, P],
    "omnitok_lm_gemm_streams16": [P, P, c_int, P, P, P, P, c_int, c_int, c_int, c_int, P, P],
    "omnitok_lm_gemm16": [P, P, c_int, P, P, P, P, I64, c_int, c_int, c_int, P, P],
    "omnitok_lm_layernorm16": [P, P, P, P, c_int, I64, c_int, P, P],
    "omnitok_lm_attn_decode": [P, P, P, P, c_int, c_int, c_int, c_int, P, P, P],
    "omnitok_lm_attn_decode_kv16": [P, P, P, c_int, P, c_int, c_int, c_int, c_int, P, P, P],
    "omnitok_lm_attn_decode_kv8": [P, P, P, P, P, P, c_int, c_int, c_int, c_int, P, P, P],
    "omnitok_lm_attn_prefill": [P, c_int, c_int, c_int, c_int, P, P, c_int, P, P],
    "omnitok_lm_attn_prefill16": [P, c_int, c_int, c_int, c_int, c_int, P, P, c_int, P, P],
    "omnitok_pl_planes_bytes": [I64, c_int, c_int],
    "omnitok_pl_unscale": [c_float],
    "omnitok_pl_pack_weight": [P, I64, c_int, c_int, c_int, P, P, P],
    "omnitok_pl_pack_rows": [P, I64, I64, c_int, I64, P, P, c_float, P],
    "omnitok_gemm_pl": [POINTER(OmnitokPlGemm), P],
    "omnitok_stats_pack": [P, I64, c_int, c_float, c_int, P, I64, P, P, P, I64, P],
    "omnitok_layernorm_planes": [P, I64, c_int, c_float, P, P, c_float, P, I64, P],
    "omnitok_stats_pack_windows": [P, I64, c_int, c_float, c_int, P, I64, P, P, c_int, c_int, c_int, P],
    "omnitok_stats_pack_temporal": [P, I64, c_int, c_float, P, P, P, P, I64, P],
    # include/omnitok_comm.h
    "omnitok_comm_available": [c_char_p, c_int],
    "omnitok_comm_unique_id": [P],
    "omnitok_comm_create": [P, c_int, c_int, POINTER(P)],
    "omnitok_comm_destroy": [P],
    "omnitok_comm_world": [P],
    "omnitok_comm_rank": [P],
    "omnitok_comm_allgather_i32": [P, P, P, I64, P],
    "omnitok_comm_allgather_ids": [P, P, P, I64, P],
    "omnitok_set_option": [c_char_p, c_int],
    "omnitok_get_option": [c_char_p, POINTER(c_int)],
    "omnitok_debug_set_gemm_trace": [P],
    "omnitok_debug_mfma_peak": [P, P, c_int, c_int, c_int, P, P],
    "omnitok_debug_fp64_peak": [P, P, c_int, c_int, P],
    "omnitok_last_error": [],
    "omnitok_version": [],
}
_RESTYPES = {"omnitok_last_error": c_char_p, "omnitok_version": c_char_p,
             "omnitok_engine_destroy": None, "omnitok_engine_workspace_bytes": c_int64,
             "omnitok_engine_workspace_need_encode": c_int64, "omnitok_engine_workspace_need_decode": c_int64,
             "omnitok_lm_destroy": None, "omnitok_comm_destroy": None, "omnitok_lm_cache_bytes": c_int64,
             "omnitok_pl_planes_bytes": c_int64, "omnitok_pl_unscale": c_float,
             "omnitok_frame_metrics_workspace": c_int64, "omnitok_frames_resize_pil_workspace": c_int64,
             "omnitok_same_pad": None,
             "omnitok_conv3d_packed_ldw": c_int64, "omnitok_lpips_workspace": c_int64,
             "omnitok_losses_workspace": c_int64, "omnitok_lm_token_ce_workspace": c_int64,
             "omnitok_lm_loss_workspace_bytes": c_int64, "omnitok_lm_step_weight_bytes": c_int64}

EXPORTED_SYMBOLS = tuple(_PROTOS)

# include/omnitok_dit.h, bound by load() like the table above
_DIT_PROTOS = {
    "omnitok_dit_create": [POINTER(OmnitokDitConfig), POINTER(P)],
    "omnitok_dit_destroy": [P],
    "omnitok_dit_set_weight": [P, c_char_p, P, POINTER(I64), c_int, P],
    "omnitok_dit_missing": [P, c_char_p, c_int],
    "omnitok_dit_finalize": [P, P],
    "omnitok_dit_timestep_table": [P, P],
    "omnitok_dit_set_frequencies": [P, P, c_int],
    "omnitok_dit_workspace_bytes": [P, c_int],
    "omnitok_dit_forward": [P, P, P, P, c_int, P, P],
    "omnitok_dit_forward_cfg": [P, P, P, P, c_int, c_float, P, P],
    "omnitok_dit_check": [P, P],
    "omnitok_dit_set_linear_format": [P, c_int],
    "omnitok_dit_linear_format": [P],
    "omnitok_dit_set_attention_format": [P, c_int],
    "omnitok_dit_attention_format": [P],
    "omnitok_dit_patch_embed": [P, c_int, P, P, P, c_int, c_int, c_int, c_int, c_int, P, P],
    "omnitok_dit_ln_modulate": [P, P, P, I64, I64, c_int, c_int, P, P],
    "omnitok_dit_attn": [P, c_int, c_int, c_int, c_int, P, P],
    "omnitok_dit_attn16": [P, c_int, c_int, c_int, c_int, c_int, P, P, c_int, P, P],
    "omnitok_dit_gate_residual": [P, P, P, I64, I64, c_int, c_int, P],
    "omnitok_dit_gelu_tanh": [P, I64, P],
    "omnitok_dit_ln_modulate16": [P, P, P, I64, I64, c_int, c_int, c_int, P, P, P],
    "omnitok_dit_round16": [P, c_int, P, I64, P, P],
    "omnitok_dit_gemm16": [P, P, c_int, P, c_int, P, P, P, I64, c_int, P, I64, c_int, c_int, P, P],
    "omnitok_dit_unpatchify": [P, c_int, c_int, c_int, c_int, P, P],
    "omnitok_dit_p_sample": [P, P, P, P, c_int, P, c_int, c_int, I64, c_int, c_int, P, P, P],
    "omnitok_dit_ddim_step": [P, P, P, P, c_int, P, c_int, c_int, I64, c_int, c_int, c_int, P, P, P],
}
_RESTYPES.update({"omnitok_dit_destroy": None, "omnitok_dit_workspace_bytes": c_int64})
DIT_EXPORTED_SYMBOLS = tuple(_DIT_PROTOS)

# include/omnitok_latte.h
_LATTE_PROTOS = {
    "omnitok_latte_create": [POINTER(OmnitokLatteConfig), POINTER(P)],
    "omnitok_latte_destroy": [P],
    "omnitok_latte_set_weight": [P, c_char_p, P, POINTER(I64), c_int, P],
    "omnitok_latte_missing": [P, c_char_p, c_int],
    "omnitok_latte_finalize": [P, P],
    "omnitok_latte_set_frequencies": [P, P, c_int],
    "omnitok_latte_workspace_bytes": [P, c_int],
    "omnitok_latte_forward": [P, P, P, P, c_int, P, P],
    "omnitok_latte_forward_cfg": [P, P, P, P, c_int, c_float, P, P],
    "omnitok_latte_check": [P, P],
    "omnitok_latte_attn_temporal": [P, c_int, c_int, c_int, c_int, c_int, P, P],
    "omnitok_latte_add_temp_embed": [P, P, c_int, c_int, c_int, c_int, P],
    "omnitok_latte_cfg_blend": [P, c_int, c_int, c_int, I64, c_float, P],
}
_RESTYPES.update({"omnitok_latte_destroy": None, "omnitok_latte_workspace_bytes": c_int64})
LATTE_EXPORTED_SYMBOLS = tuple(_LATTE_PROTOS)

# include/omnitok_latte_linear.h (the part of omnitok_latte.h that holds the engine's linear format)
_LATTE_LINEAR_PROTOS = {
    "omnitok_latte_set_linear_format": [P, c_int],
    "omnitok_latte_linear_format": [P],
}
LATTE_LINEAR_EXPORTED_SYMBOLS = tuple(_LATTE_LINEAR_PROTOS)

# include/omnitok_latte_attention.h (the part of omnitok_latte.h that holds the engine's attention format)
_LATTE_ATTENTION_PROTOS = {
    "omnitok_latte_set_attention_format": [P, c_int],
    "omnitok_latte_attention_format": [P],
}
LATTE_ATTENTION_EXPORTED_SYMBOLS = tuple(_LATTE_ATTENTION_PROTOS)

_lib = None


def load():
    """Loads libomnitok.so (building nothing: run `python omnitokenizer_amd/build.py` or
    __graft_entry__.build() first)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OmnitokError(
            f"{LIB_PATH} not found: the HIP library is required (no CPU fallback). "
            "Build it with `python omnitokenizer_amd/build.py`.")
    # PyTorch-ROCm ships its own HIP runtime; it must be the one in the process before libomnitok.so is mapped,
    # otherwise the library binds a second runtime (/opt/rocm) that sees no device once torch has initialised its
    # own ("no ROCm-capable device is detected" at the first hipMalloc).  Importing torch first pins the order no
    # matter what the caller imported before.
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    for name, argtypes in {**_PROTOS, **_DIT_PROTOS, **_LATTE_PROTOS, **_LATTE_LINEAR_PROTOS, **_LATTE_ATTENTION_PROTOS}.items():
        fn = getattr(lib, name)  # AttributeError here = header/library mismatch: fail loudly
        fn.argtypes = argtypes
        fn.restype = _RESTYPES.get(name, c_int)
    _lib = lib
    # tuning knobs for A/B runs: OMNITOK_OPTS="gemm_variant=1,gemm_lds_pad_kb=40"
    for kv in filter(None, os.environ.get("OMNITOK_OPTS", "").split(",")):
        k, v = kv.split("=")
        if lib.omnitok_set_option(k.strip().encode(), int(v)) != 0:
            raise OmnitokError(lib.omnitok_last_error().decode())
    return lib


def get_option(name: str) -> int:
    v = c_int()
    check(load().omnitok_get_option(name.encode(), ctypes.byref(v)), "get_option")
    return v.value


def set_option(name: str, value: int):
    check(load().omnitok_set_option(name.encode(), int(value)), "set_option")


def check(rc: int, what: str = ""):
    """Raises on a negative status: ValueError for invalid arguments (the reference's asserts),
    RuntimeError otherwise."""
    if rc >= 0:
        return rc
    msg = load().omnitok_last_error().decode(errors="replace")
    if rc == -1:
        raise ValueError(msg)
    if rc == -4:
        raise NotImplementedError(msg)
    raise OmnitokError(f"{what}: {msg} (status {rc})")


def ptr(t):
    """the address of tensor t as a ctypes pointer argument; None (a null pointer) for None"""
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    """the current torch stream as the omnitok_stream_t argument of the entry points"""
    import torch
    return torch.cuda.current_stream().cuda_stream
