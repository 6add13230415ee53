"""ctypes binding of libsd_engine.so (the C-ABI in include/sd_engine.h).

There is deliberately no fallback: if the shared library is missing or a call fails the shim
raises -- the product path never routes through the CPU oracle.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsd_engine.so")

SD_MAX_BLOCKS = 4
SD_STEP_MAX_SLOTS = 4
SD_STEP_MAX_WRITES = 2
SD_DTYPE_F16 = 0
SD_DTYPE_F32 = 1


class SdUNetConfig(C.Structure):
    _fields_ = [
        ("in_channels", C.c_int32),
        ("out_channels", C.c_int32),
        ("num_blocks", C.c_int32),
        ("block_out_channels", C.c_int32 * SD_MAX_BLOCKS),
        ("down_block_has_attn", C.c_int32 * SD_MAX_BLOCKS),
        ("up_block_has_attn", C.c_int32 * SD_MAX_BLOCKS),
        ("num_heads", C.c_int32 * SD_MAX_BLOCKS),
        ("transformer_layers", C.c_int32 * SD_MAX_BLOCKS),
        ("layers_per_block", C.c_int32),
        ("cross_attention_dim", C.c_int32),
        ("use_linear_projection", C.c_int32),
        ("norm_num_groups", C.c_int32),
        ("norm_eps", C.c_float),
        ("flip_sin_to_cos", C.c_int32),
        ("freq_shift", C.c_float),
        ("addition_time_embed_dim", C.c_int32),
        ("projection_class_embeddings_input_dim", C.c_int32),
        ("num_time_ids", C.c_int32),
        ("time_cond_proj_dim", C.c_int32),
    ]


class SdVAEConfig(C.Structure):
    _fields_ = [
        ("in_channels", C.c_int32),
        ("out_channels", C.c_int32),
        ("latent_channels", C.c_int32),
        ("num_blocks", C.c_int32),
        ("block_out_channels", C.c_int32 * SD_MAX_BLOCKS),
        ("layers_per_block", C.c_int32),
        ("norm_num_groups", C.c_int32),
    ]


SD_VAE_TILE_MAX_AXIS = 64
SD_VAE_TILE_MAX_CLASSES = 9
SD_VAE_TILE_MAX_BATCH = 32


class SdVAETiles(C.Structure):
    """sd_vae_tiles (include/sd_engine.h): the plan of one tiled decode / encode."""
    _fields_ = [
        ("ny", C.c_int32), ("nx", C.c_int32),
        ("tile_in", C.c_int32), ("stride_in", C.c_int32),
        ("tile_out", C.c_int32), ("blend", C.c_int32), ("limit", C.c_int32),
        ("scale", C.c_int32),
        ("in_h", C.c_int32), ("in_w", C.c_int32), ("out_h", C.c_int32), ("out_w", C.c_int32),
        ("size_y", C.c_int32 * SD_VAE_TILE_MAX_AXIS), ("size_x", C.c_int32 * SD_VAE_TILE_MAX_AXIS),
        ("n_classes", C.c_int32),
        ("class_h", C.c_int32 * SD_VAE_TILE_MAX_CLASSES), ("class_w", C.c_int32 * SD_VAE_TILE_MAX_CLASSES),
        ("class_count", C.c_int32 * SD_VAE_TILE_MAX_CLASSES),
        ("class_iy0", C.c_int32 * SD_VAE_TILE_MAX_CLASSES), ("class_ny", C.c_int32 * SD_VAE_TILE_MAX_CLASSES),
        ("class_ix0", C.c_int32 * SD_VAE_TILE_MAX_CLASSES), ("class_nx", C.c_int32 * SD_VAE_TILE_MAX_CLASSES),
    ]


class SdClipConfig(C.Structure):
    _fields_ = [
        ("vocab_size", C.c_int32),
        ("hidden_size", C.c_int32),
        ("intermediate_size", C.c_int32),
        ("num_layers", C.c_int32),
        ("num_heads", C.c_int32),
        ("max_positions", C.c_int32),
        ("hidden_act", C.c_int32),
        ("projection_dim", C.c_int32),
        ("layer_norm_eps", C.c_float),
    ]


class SdClipVisionConfig(C.Structure):
    _fields_ = [
        ("hidden_size", C.c_int32),
        ("intermediate_size", C.c_int32),
        ("num_layers", C.c_int32),
        ("num_heads", C.c_int32),
        ("image_size", C.c_int32),
        ("patch_size", C.c_int32),
        ("hidden_act", C.c_int32),
        ("projection_dim", C.c_int32),
        ("layer_norm_eps", C.c_float),
    ]


class SdIPProjectionConfig(C.Structure):
    _fields_ = [
        ("kind", C.c_int32),
        ("image_embed_dim", C.c_int32),
        ("num_tokens", C.c_int32),
        ("dim", C.c_int32),
        ("heads", C.c_int32),
        ("depth", C.c_int32),
        ("ff_mult", C.c_int32),
    ]


SD_IP_PROJ_LINEAR = 0
SD_IP_PROJ_RESAMPLER = 1


class SdMotionConfig(C.Structure):
    """sd_motion_config (include/sd_engine.h): an AnimateDiff motion adapter for a UNet topology."""
    _fields_ = [
        ("num_blocks", C.c_int32),
        ("block_out_channels", C.c_int32 * SD_MAX_BLOCKS),
        ("num_heads", C.c_int32 * SD_MAX_BLOCKS),
        ("layers_per_block", C.c_int32),
        ("max_seq_length", C.c_int32),
        ("use_mid_block", C.c_int32),
    ]


class SdProfEntry(C.Structure):
    _fields_ = [("kernel", C.c_char * 64), ("flops", C.c_double), ("bytes", C.c_double),
                ("ms", C.c_double), ("launches", C.c_int64)]


class SdTapInfo(C.Structure):
    _fields_ = [("name", C.c_char_p), ("kind", C.c_int32), ("dtype", C.c_int32), ("N", C.c_int32), ("H", C.c_int32),
                ("W", C.c_int32), ("C", C.c_int32), ("c0", C.c_int32), ("ld", C.c_int64), ("bytes", C.c_int64),
                ("scale", C.c_float)]


SD_TAP_IN, SD_TAP_OUT, SD_TAP_PRE = 0, 1, 2


class SdCnProblem(C.Structure):
    _fields_ = [("x", C.c_void_p), ("ldx", C.c_int64), ("w", C.c_void_p), ("bias", C.c_void_p),
                ("y", C.c_void_p), ("ldy", C.c_int64), ("M", C.c_int), ("C", C.c_int)]


SD_MAX_CONTROLNETS = 4


class SdCnMultiProblem(C.Structure):
    """One residual site of sd_op_controlnet_residuals_multi: up to four sources, weights and biases onto one y."""
    _fields_ = [("x", C.c_void_p * SD_MAX_CONTROLNETS), ("ldx", C.c_int64 * SD_MAX_CONTROLNETS),
                ("w", C.c_void_p * SD_MAX_CONTROLNETS), ("bias", C.c_void_p * SD_MAX_CONTROLNETS),
                ("y", C.c_void_p), ("ldy", C.c_int64), ("M", C.c_int), ("C", C.c_int)]


class SdStepPlan(C.Structure):
    """One scheduler step for sd_sched_affine_step: rows of float64 coefficients over (x, m, z, h_0 .. h_3)."""
    _fields_ = [("n_slots", C.c_int32), ("n_writes", C.c_int32), ("write_slot", C.c_int32 * SD_STEP_MAX_WRITES),
                ("out", C.c_double * (3 + SD_STEP_MAX_SLOTS)),
                ("write", C.c_double * (3 + SD_STEP_MAX_SLOTS) * SD_STEP_MAX_WRITES)]


def step_plan(plan) -> SdStepPlan:
    """schedulers.AffinePlan -> the struct sd_sched_affine_step takes."""
    if len(plan.writes) > SD_STEP_MAX_WRITES or plan.n_slots > SD_STEP_MAX_SLOTS:
        raise ValueError(f"an affine step has at most {SD_STEP_MAX_WRITES} writes and {SD_STEP_MAX_SLOTS} slots")
    p = SdStepPlan(n_slots=plan.n_slots, n_writes=len(plan.writes))
    p.out[:] = plan.out
    for j, (slot, row) in enumerate(plan.writes):
        p.write_slot[j] = slot
        p.write[j][:] = row
    return p


# name -> (restype, argtypes); every symbol include/sd_engine.h declares
_P = C.c_void_p
_I = C.c_int
_I64 = C.c_int64
_F = C.c_float
SIGNATURES = {
    "sd_last_error": (C.c_char_p, []),
    "sd_engine_version": (_I, []),
    "sd_engine_arch": (C.c_char_p, []),
    "sd_unet_create": (_I, [C.POINTER(SdUNetConfig), C.POINTER(_P)]),
    "sd_unet_destroy": (_I, [_P]),
    "sd_unet_num_weights": (_I, [_P]),
    "sd_unet_weight_info": (_I, [_P, _I, C.POINTER(C.c_char_p), C.POINTER(_I64), C.POINTER(_I)]),
    "sd_unet_set_weight": (_I, [_P, C.c_char_p, _P, C.POINTER(_I64), _I, _I]),
    "sd_unet_finalize": (_I, [_P]),
    "sd_unet_forward": (_I, [_P, _P, _P, _P, _I, _P, _P, _P, _I, _I, _I, _P]),
    "sd_unet_use_graph": (_I, [_P, _I]),
    "sd_unet_graph_stats": (_I, [_P, C.POINTER(_I64), C.POINTER(_I64)]),
    "sd_unet_text_kv_cache": (_I, [_P, _I]),
    "sd_unet_memory": (_I, [_P, C.POINTER(_I64), C.POINTER(_I64)]),
    "sd_unet_forward_ex": (_I, [_P, _P, _P, _P, _I, _P, _P, _P, _I, _P, _I, _I, _I, _P]),
    "sd_unet_forward_tc": (_I, [_P, _P, _P, _P, _I, _P, _P, _P, _I, _P, _I, _P, _I, _I, _I, _P]),
    "sd_unet_forward_cfg": (_I, [_P, _P, _P, _P, _I, _P, _P, _P, _I, _F, _I, _P, _I, _I, _I, _P]),
    "sd_unet_cfg_share": (_I, [C.POINTER(SdUNetConfig)]),
    "sd_unet_set_ip_adapter": (_I, [_P, _P]),
    "sd_unet_set_ip_adapter_scale": (_I, [_P, _F]),
    "sd_unet_set_freeu": (_I, [_P, _I, _F, _F, _F, _F]),
    "sd_unet_set_tome": (_I, [_P, C.c_double, _I, _I, _I, _I, C.c_uint32]),
    "sd_unet_tome_step": (_I, [_P, C.c_uint32]),
    "sd_unet_tome_sites": (_I, [_P]),
    "sd_unet_tome_read": (_I, [_P, _I, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _I64]),
    "sd_unet_set_hypertile": (_I, [_P, _I, _I, _I, C.c_uint32]),
    "sd_unet_hypertile_step": (_I, [_P, C.c_uint32]),
    "sd_unet_hypertile_sites": (_I, [_P]),
    "sd_unet_hypertile_read": (_I, [_P, _I, C.POINTER(C.c_int32)]),
    "sd_unet_set_pag_layers": (_I, [_P, _P, _I]),
    "sd_unet_forward_pag": (_I, [_P, _P, _P, _P, _I, _P, _P, _F, _I, _I, _P, _I, _I, _I, _P]),
    "sd_unet_forward_concat": (_I, [_P, _P, _I, _F, _P, _I, _I, _I, _P, _P, _I, _P, _P, _P, _I, _I, _I, _P]),
    "sd_unet_set_regions": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "sd_unet_set_deep_cache": (_I, [_P, _I]),
    "sd_unet_deep_cache_mode": (_I, [_P, _I]),
    "sd_ip_adapter_create": (_I, [_P, _I, _I, C.POINTER(_P)]),
    "sd_ip_adapter_create_ex": (_I, [_P, C.POINTER(SdIPProjectionConfig), C.POINTER(_P)]),
    "sd_ip_adapter_set_feature_tokens": (_I, [_P, _I]),
    "sd_ip_adapter_project": (_I, [_P, _P, _I, _P, _P]),
    "sd_ip_adapter_destroy": (_I, [_P]),
    "sd_ip_adapter_num_weights": (_I, [_P]),
    "sd_ip_adapter_weight_info": (_I, [_P, _I, C.POINTER(C.c_char_p), C.POINTER(_I64), C.POINTER(_I)]),
    "sd_ip_adapter_set_weight": (_I, [_P, C.c_char_p, _P, C.POINTER(_I64), _I, _I]),
    "sd_ip_adapter_finalize": (_I, [_P]),
    "sd_unet_set_controlnet": (_I, [_P, _P]),
    "sd_unet_forward_cn": (_I, [_P, _P, _P, _P, _I, _P, _P, _P, _I, _P, _I, _F, _P, _I, _I, _I, _P]),
    "sd_unet_set_controlnets": (_I, [_P, C.POINTER(_P), _I]),
    "sd_unet_forward_mcn": (_I, [_P, _P, _P, _P, _I, _P, _P, _P, _I, C.POINTER(_P), C.POINTER(_I), C.POINTER(_F), _I, _P, _I,
                                _I, _I, _P]),
    "sd_unet_cn_fold_count": (_I64, [_P]),
    "sd_cn_kcat_force": (_I, [_I]),
    "sd_controlnet_create": (_I, [_P, C.POINTER(SdUNetConfig), _I, C.POINTER(_P)]),
    "sd_controlnet_destroy": (_I, [_P]),
    "sd_controlnet_num_weights": (_I, [_P]),
    "sd_controlnet_weight_info": (_I, [_P, _I, C.POINTER(C.c_char_p), C.POINTER(_I64), C.POINTER(_I)]),
    "sd_controlnet_set_weight": (_I, [_P, C.c_char_p, _P, C.POINTER(_I64), _I, _I]),
    "sd_controlnet_finalize": (_I, [_P]),
    "sd_vae_create": (_I, [C.POINTER(SdVAEConfig), C.POINTER(_P)]),
    "sd_vae_destroy": (_I, [_P]),
    "sd_vae_num_weights": (_I, [_P]),
    "sd_vae_weight_info": (_I, [_P, _I, C.POINTER(C.c_char_p), C.POINTER(_I64), C.POINTER(_I)]),
    "sd_vae_set_weight": (_I, [_P, C.c_char_p, _P, C.POINTER(_I64), _I, _I]),
    "sd_vae_finalize": (_I, [_P]),
    "sd_vae_decode": (_I, [_P, _P, _P, _I, _I, _I, _P]),
    "sd_vae_encode": (_I, [_P, _P, _P, _I, _I, _I, _P]),
    "sd_vae_encode_range_shift": (_I, [_P, _I]),
    "sd_vae_memory": (_I, [_P, C.POINTER(_I64), C.POINTER(_I64)]),
    "sd_unet_tap": (_I, [_P, _I]),
    "sd_unet_tap_count": (_I, [_P]),
    "sd_unet_tap_info": (_I, [_P, _I, C.POINTER(SdTapInfo)]),
    "sd_unet_tap_read": (_I, [_P, _I, _P, _I64]),
    "sd_vae_tap": (_I, [_P, _I]),
    "sd_vae_tap_count": (_I, [_P]),
    "sd_vae_tap_info": (_I, [_P, _I, C.POINTER(SdTapInfo)]),
    "sd_vae_tap_read": (_I, [_P, _I, _P, _I64]),
    "sd_unet_poison_workspace": (_I, [_P, _I, C.POINTER(_I64)]),
    "sd_vae_poison_workspace": (_I, [_P, _I, C.POINTER(_I64)]),
    "sd_clip_poison_workspace": (_I, [_P, _I, C.POINTER(_I64)]),
    "sd_clip_vision_poison_workspace": (_I, [_P, _I, C.POINTER(_I64)]),
    "sd_ip_adapter_poison_workspace": (_I, [_P, _I, C.POINTER(_I64)]),
    "sd_ip_adapter_memory": (_I, [_P, C.POINTER(_I64), C.POINTER(_I64)]),
    "sd_clip_create": (_I, [C.POINTER(SdClipConfig), C.POINTER(_P)]),
    "sd_clip_destroy": (_I, [_P]),
    "sd_clip_num_weights": (_I, [_P]),
    "sd_clip_weight_info": (_I, [_P, _I, C.POINTER(C.c_char_p), C.POINTER(_I64), C.POINTER(_I)]),
    "sd_clip_set_weight": (_I, [_P, C.c_char_p, _P, C.POINTER(_I64), _I, _I]),
    "sd_clip_finalize": (_I, [_P]),
    "sd_clip_forward": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _P]),
    "sd_clip_final_layer_norm": (_I, [_P, _P, _P, _I64, _P]),
    "sd_clip_memory": (_I, [_P, C.POINTER(_I64), C.POINTER(_I64)]),
    "sd_clip_vision_create": (_I, [C.POINTER(SdClipVisionConfig), C.POINTER(_P)]),
    "sd_clip_vision_destroy": (_I, [_P]),
    "sd_clip_vision_num_weights": (_I, [_P]),
    "sd_clip_vision_weight_info": (_I, [_P, _I, C.POINTER(C.c_char_p), C.POINTER(_I64), C.POINTER(_I)]),
    "sd_clip_vision_set_weight": (_I, [_P, C.c_char_p, _P, C.POINTER(_I64), _I, _I]),
    "sd_clip_vision_finalize": (_I, [_P]),
    "sd_clip_vision_forward": (_I, [_P, _P, _P, _P, _P, _P, _I, _P]),
    "sd_clip_vision_memory": (_I, [_P, C.POINTER(_I64), C.POINTER(_I64)]),
    "sd_op_vit_patch_embed": (_I, [_P, _P, _P, _P, _P, _I64, _I, _I, _I, _I, _P]),
    "sd_op_attention_ex": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "sd_cfg_duplicate": (_I, [_P, _P, _I64, _I, _F, _P]),
    "sd_inpaint_blend": (_I, [_P, _P, _P, _P, _F, _F, _I, _I, _I, _I, _P]),
    "sd_images_to_uint8": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "sd_view_plan": (_I, [_I, _I, _I, _I, C.POINTER(_I), _I]),
    "sd_views_gather": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, C.POINTER(_I), _I, C.POINTER(_I), _I, _I, _P]),
    "sd_views_merge": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, C.POINTER(_I), _I, C.POINTER(_I), _I, _I, _I, _P]),
    "sd_vae_tile_plan": (_I, [_I, _I, _I, _I, _I, C.c_double, C.POINTER(SdVAETiles)]),
    "sd_vae_tile_stack": (_I, [C.POINTER(SdVAETiles), _I, _I, C.POINTER(_I64), C.POINTER(_I64)]),
    "sd_vae_decode_tiled": (_I, [_P, _P, _P, _I, _I, _I, _I, C.c_double, _I, _P]),
    "sd_vae_encode_tiled": (_I, [_P, _P, _P, _I, _I, _I, _I, C.c_double, _I, _P]),
    "sd_vae_memory_tiled": (_I, [_P, C.POINTER(_I64), C.POINTER(_I64), C.POINTER(_I64)]),
    "sd_op_vae_tiles_gather": (_I, [_P, _I64, _P, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I), _I, _I, _I, _I, _I, _I, _I, _I,
                                    C.POINTER(_F), _P]),
    "sd_op_vae_tiles_merge": (_I, [_P, _I64, _P, _I64, C.POINTER(SdVAETiles), _I, _I, _I, C.POINTER(_F), _P]),
    "sd_cfg_linear_step": (_I, [_P, _P, _P, _I64, _F, _F, _F, _F, _F, _F, _P]),
    "sd_pag_linear_step": (_I, [_P, _I, _P, _P, _I64, _F, _F, _F, _F, _F, _F, _F, _P]),
    "sd_pag_combine": (_I, [_P, _I, _P, _I64, _F, _F, _P]),
    "sd_ip2p_linear_step": (_I, [_P, _P, _P, _I64, _F, _F, _F, _F, _F, _F, _F, _P]),
    "sd_ip2p_combine": (_I, [_P, _P, _I64, _F, _F, _P]),
    "sd_cfg_rescale_linear_step": (_I, [_P, _P, _P, _I, _I64, _F, _F, _F, _F, _F, _F, _F, _P, _P]),
    "sd_lcm_step": (_I, [_P, _I, _P, _P, _P, _I64, _F, _F, _F, _F, _F, _P]),
    "sd_sched_affine_step": (_I, [_P, _I, _P, _P, _P, _I64, _I64, _F, C.POINTER(SdStepPlan), _P]),
    "sd_igemm_force": (_I, [_I, _I]),
    "sd_igemm_plan": (_I, [C.POINTER(_I), C.POINTER(_I), C.POINTER(_I64), C.c_char_p]),
    "sd_halo80_force": (_I, [_I]),
    "sd_halo80_plan": (_I, [C.POINTER(_I), C.POINTER(_I), _I, C.POINTER(_I64), C.c_char_p]),
    "sd_conv_plan": (_I, [C.POINTER(_I), C.POINTER(_I), _I, _I, C.POINTER(_I64), C.c_char_p]),
    "sd_probe_mfma": (_I, [_I, C.POINTER(_F), _P]),
    "sd_probe_lds_dma": (_I, [_I64, _I, _I, _I, C.POINTER(_F), _P]),
    "sd_probe_copy": (_I, [_I64, _I, C.POINTER(_F), _P]),
    "sd_prof_enable": (_I, [_I]),
    "sd_prof_collect": (_I, [C.POINTER(SdProfEntry), _I, C.POINTER(_I)]),
    "sd_op_conv2d": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "sd_op_conv2d_ex": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I64, _I64, _I64, _I, _I, _F, _F, _I,
                             C.POINTER(_I), _P]),
    "sd_op_conv2d_gnstats": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _I64, C.POINTER(_I), C.POINTER(_I), _P]),
    "sd_upconv_fold_supported": (_I, [_I, _I, _I, _I, _I]),
    "sd_op_fold_upconv": (_I, [_P, _P, _I, _I, _P]),
    "sd_op_upconv2x_ex": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I64, _I64, _I64, _F, _F, _I, _P,
                               C.POINTER(_I), _P]),
    "sd_op_conv3x3_small_cout": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "sd_op_conv2d_groupnorm": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _F, _I,
                                    C.POINTER(_I), _P]),
    "sd_op_groupnorm_conv2d": (_I, [_P, _P, _P, _I, _F, _I, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, C.POINTER(_F),
                                    C.POINTER(_I), _P]),
    "sd_op_unet_conv_in2": (_I, [_P, _I, _I, _F, _P, _I, _I, _I, _P, _P, _P, _I64, _P, _I, _I, _I, _I, _I, _I, C.POINTER(_F), _P]),
    "sd_op_unet_conv_in": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, C.POINTER(_F), _P]),
    "sd_op_unet_conv_out": (_I, [_P, _P, _P, _I, _F, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, C.POINTER(_F), _P]),
    "sd_op_ffn_geglu": (_I, [_P, _P, _P, _F, _P, _P, _P, _P, _P, _I, _I, _I, C.POINTER(_F), C.POINTER(_I), _P]),
    "sd_op_linear_rowstats": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I), _P]),
    "sd_op_ln_linear": (_I, [_P, _P, _I, _I, _P, _P, _F, _P, _P, _P, _I, _I, _I, _I, _I, _F, C.POINTER(_I), _P]),
    "sd_op_ln_ffn_geglu": (_I, [_P, _P, _I, _I, _P, _P, _F, _P, _P, _P, _P, _P, _I, _I, C.POINTER(_I), _P]),
    "sd_op_fold_linear": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "sd_op_ffn_geglu_proj_out": (_I, [_P, _P, _P, _P, _F, _P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(_I), _I, _I, _I,
                                      C.POINTER(_I), _P]),
    "sd_bench_conv2d": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, C.POINTER(_F), _P]),
    "sd_op_groupnorm": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _F, _I, _P]),
    "sd_op_unet_conv_out_ex": (_I, [_P, _I64, _P, _P, _I, _F, _I, _P, _P, _P, _I, _I, _I, _I, _I, _P, _I, _I64, _I, C.POINTER(_F), _P]),
    "sd_norm_plan": (_I, [_I, _I64, _I, _I, _I, _I, C.POINTER(_I64)]),
    "sd_norm_plan_batch": (_I, [_I, C.POINTER(_I64), C.POINTER(_I64)]),
    "sd_op_groupnorm_ex": (_I, [_P, _I64, _P, _P, _P, _I64, _I, _I64, _I, _I, _F, _I, _P, _I, _I64, C.POINTER(_I64), _P]),
    "sd_op_gn_stats": (_I, [_P, _I64, _I, _I64, _I, _I, C.POINTER(_F), C.POINTER(_I), C.POINTER(_I64), C.POINTER(_I), _P]),
    "sd_op_groupnorm_concat": (_I, [_P, _I, _I, _P, _P, _P, _I, _I, _I, _F, _I, _P]),
    "sd_bench_groupnorm": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _F, _I, _I, C.POINTER(_F), _P]),
    "sd_op_timestep_sinusoid": (_I, [_P, _P, _I, _I, _I, _F, _P]),
    "sd_op_text_time_input": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _F, _P]),
    "sd_op_timestep_cond_embedding": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _F, _P]),
    "sd_small_linear_plan": (_I, [_I, _I, _I]),
    "sd_op_small_linear": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "sd_op_freeu": (_I, [_P, _I, _I, _I, _I, _I, _F, _F, _P]),
    "sd_tome_plan": (_I, [_I, _I, _I, _I, C.c_double, _I, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_int32),
                          C.POINTER(C.c_int32)]),
    "sd_tome_plan_bytes": (_I64, [_I, _I]),
    "sd_op_tome_match": (_I, [_P, _I64, _I, _I, _I, _I, _I, _I, C.c_double, _I, C.c_uint32, C.c_uint32, C.c_uint32, _P, _P, _P,
                              _P, _P]),
    "sd_op_tome_plan_from_map": (_I, [C.POINTER(C.c_int32), _I, _I, _I, _P, _P]),
    "sd_op_tome_merge": (_I, [_P, _I64, _I, _P, _I, _I, _P, _I64, _P]),
    "sd_op_tome_unmerge": (_I, [_P, _I64, _I, _P, _I, _I, _P, _I64, _P]),
    "sd_hypertile_plan": (_I, [_I, _I, _I, _I, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_int32)]),
    "sd_op_hypertile_gather": (_I, [_P, _I64, _I, _I, _I, _I, _I, _I, _P, _I64, _P]),
    "sd_op_hypertile_scatter": (_I, [_P, _I64, _I, _I, _I, _I, _I, _I, _P, _I64, _P]),
    "sd_motion_create": (_I, [_P, C.POINTER(SdMotionConfig), C.POINTER(C.c_void_p)]),
    "sd_motion_destroy": (_I, [_P]),
    "sd_motion_num_weights": (_I, [_P]),
    "sd_motion_weight_info": (_I, [_P, _I, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.POINTER(_I)]),
    "sd_motion_set_weight": (_I, [_P, C.c_char_p, _P, C.POINTER(C.c_int64), _I, _I]),
    "sd_motion_finalize": (_I, [_P]),
    "sd_unet_set_motion": (_I, [_P, _P]),
    "sd_unet_forward_motion": (_I, [_P, _P, _P, _P, _I, _I, _P, _I, _I, _I, _P]),
    "sd_unet_forward_cfg_ex": (_I, [_P, _P, _P, _P, _I, _P, _P, _P, _I, _F, _I, _I, _P, _I, _I, _I, _P]),
    "sd_temporal_attention_plan": (_I, [_I, _I, _I, _I, _I, C.POINTER(_I64)]),
    "sd_op_temporal_attention": (_I, [_P, _P, _P, _P, _P, _I64, _I64, _I64, _I64, _I64, _I, _I, _I, _I, _I, _I, _P]),
    "sd_op_motion_pos_bias": (_I, [_P, _I, _I, _I, _F, _I, _P, _I64, _P]),
    "sd_op_layernorm": (_I, [_P, _P, _P, _P, _I, _I, _F, _P]),
    "sd_op_layernorm_ex": (_I, [_P, _I64, _P, _P, _P, _I64, _I64, _I, _F, _P]),
    "sd_op_row_stats": (_I, [_P, _I64, _P, _I64, _I, _P]),
    "sd_op_attention": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "sd_attention_plan": (_I, [_I, _I, _I, _I, _I, _I, _I, C.POINTER(_I)]),
    "sd_op_ip_cross_attention": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _F, _I, _I,
                                      C.POINTER(_F), _P]),
    "sd_ip_attention_plan": (_I, [_I, _I, _I, _I, _I, _I, _F, C.POINTER(_I)]),
    "sd_op_region_cross_attention": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "sd_region_plan": (_I, [_I, _I, _I, C.POINTER(_I)]),
    "sd_op_region_pyramid": (_I, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "sd_op_resampler_attention": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I,
                                       C.POINTER(_F), _P]),
    "sd_op_controlnet_residuals": (_I, [C.POINTER(SdCnProblem), _I, _F, _I, _I, C.POINTER(_F), _P]),
    "sd_op_cn_fold_scales": (_I, [C.POINTER(_P), C.POINTER(_P), C.POINTER(_F), _I, _I, _P, _P, _I, C.POINTER(_F), _P]),
    "sd_op_controlnet_residuals_multi": (_I, [C.POINTER(SdCnMultiProblem), _I, C.POINTER(_F), _I, _I, _I, C.POINTER(_F), _P]),
    "sd_op_controlnet_cond_embed": (_I, [_P, _P, _I, _I, _I, _P, _I, C.POINTER(_F), _P]),
    "sd_op_cn_cond_conv": (_I, [_P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P]),
}

_lib = None


class EngineError(RuntimeError):
    pass


def load():
    """Load libsd_engine.so; raises if it has not been built (no CPU fallback exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EngineError(
            f"{LIB_PATH} not found: build it with `python -m stablediffusion_amd.build` "
            "(hipcc --offload-arch=gfx950). The HIP engine is mandatory; there is no CPU fallback.")
    # The engine works on torch's device pointers, so it must share torch's HIP runtime.  torch ships its own
    # libamdhip64 under the system library's soname: with torch loaded first the engine binds to that copy; loaded
    # before torch, the process would end up with two HIP / HSA runtimes and the engine's would see no device.
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = load().sd_last_error()
        raise EngineError(f"{what}: error {rc}: {msg.decode() if msg else '?'}")


def require_gpu():
    import torch
    if not torch.cuda.is_available():
        raise EngineError("no HIP device visible: the gfx950 engine cannot run (and nothing else will run in its place)")
