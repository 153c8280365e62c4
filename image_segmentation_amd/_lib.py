"""ctypes binding of libsegk.so (the C ABI declared in include/segk.h).

The product path has NO CPU or eager-PyTorch fallback: if the HIP library is missing this module raises
at first use, and every op raises RuntimeError(segk_last_error()) on a non-zero return code.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libsegk.so")

F32, BF16 = 0, 1
ABI_VERSION = 340        # SEGK_ABI_VERSION of the include/segk.h this table was written against
MAX_CLASSES = 8
MAX_VIEWS = 16           # SEGK_MAX_VIEWS
MAX_TEMPS = 32           # SEGK_MAX_TEMPS
MSE_PART_FLOATS = 1024   # SEGK_MSE_PART_FLOATS
OPTIM_CHUNK = 4096       # SEGK_OPTIM_CHUNK
OPTIM_MAX_GROUPS = 1024  # SEGK_OPTIM_MAX_GROUPS
MORPH_MAX_RADIUS = 32    # SEGK_MORPH_MAX_RADIUS
MORPH_TILE_H, MORPH_TILE_W = 64, 128       # SEGK_MORPH_TILE_H, SEGK_MORPH_TILE_W
MORPH_WILD, MORPH_FAR = 0xFFFF, 0xFFFF     # SEGK_MORPH_WILD, SEGK_MORPH_FAR
MORPH_METRICS = {"square": 0, "diamond": 1, "disk": 2}     # SEGK_MORPH_SQUARE / _DIAMOND / _DISK
MIX_NONE, MIX_BOX, MIX_CLASS, MIX_OBJECT = 0, 1, 2, 3      # SEGK_MIX_NONE / _BOX / _CLASS / _OBJECT
MIX_TILE_H, MIX_TILE_W = 16, 64            # SEGK_MIX_TILE_H, SEGK_MIX_TILE_W
MIX_MAX_OBJECTS, MIX_MAX_COMPONENTS = 32, 65536            # SEGK_MIX_MAX_OBJECTS, SEGK_MIX_MAX_COMPONENTS
MIX_STAGE_BYTES, MIX_STAGE_SELECT = 0, 1   # SEGK_MIX_STAGE_BYTES, SEGK_MIX_STAGE_SELECT
BOUNDARY_TILE_H, BOUNDARY_TILE_W = 64, 128 # SEGK_BOUNDARY_TILE_H, SEGK_BOUNDARY_TILE_W
BOUNDARY_MAX_WIDTH, BOUNDARY_BINS = 32, 34 # SEGK_BOUNDARY_MAX_WIDTH, SEGK_BOUNDARY_BINS
BOUNDARY_HIST_WORDS, BOUNDARY_STAT_WORDS = 544, 656        # SEGK_BOUNDARY_HIST_WORDS, SEGK_BOUNDARY_STAT_WORDS
# word offsets in the statistics: SEGK_BOUNDARY_BAND_G / _BAND_P / _BAND_I / _CONF / _HD_SUM / _HD_IMAGES / _HD_CAPPED / _HIST
BOUNDARY_OFFSETS = {"band_g": 0, "band_p": 8, "band_i": 16, "conf": 24, "hd_sum": 88, "hd_images": 96, "hd_capped": 104, "hist": 112}
SLIC_TILE, SLIC_MAX_CELLS = 64, 18          # SEGK_SLIC_TILE, SEGK_SLIC_MAX_CELLS
SLIC_TILE_ROWS = (64, 16, 4)               # the tile_rows segk_slic_assign and segk_snap_vote take
SLIC_MIN_STEP, SLIC_MAX_STEP = 4, 64       # SEGK_SLIC_MIN_STEP, SEGK_SLIC_MAX_STEP
SLIC_MAX_COMPACTNESS, SLIC_MAX_ITERATIONS, SLIC_MAX_SIDE = 255, 20, 1 << 27    # SEGK_SLIC_MAX_COMPACTNESS / _ITERATIONS / _SIDE
SLIC_SPACES = {"rgb": 0, "ycc": 1}         # SEGK_SLIC_RGB / _YCC
SLIC_CENTRE_WORDS, SLIC_SUM_WORDS, SNAP_NONE = 5, 8, 255   # SEGK_SLIC_CENTRE_WORDS, SEGK_SLIC_SUM_WORDS, SEGK_SNAP_NONE
# flags of segk_optim_grad_norm (CLIP, SKIP_NONFINITE) and of segk_optim_adamw (NORMED, SKIP_NONFINITE, EMA_WARMUP, SWAP)
OPTIM_CLIP, OPTIM_SKIP_NONFINITE, OPTIM_NORMED, OPTIM_EMA_WARMUP, OPTIM_SWAP = 1, 2, 1, 4, 8

_vp, _fp, _i, _l, _f, _d = C.c_void_p, C.c_void_p, C.c_int, C.c_long, C.c_float, C.c_double

# name -> (restype, argtypes); mirrors include/segk.h one to one (checked by tests/test_abi.py)
SIGNATURES = {
    "segk_version": (_i, []),
    "segk_entry_count": (_i, []),
    "segk_clock_probe": (_i, [_vp, _i, _i, _i, _vp]),
    "segk_debug_poison_tickets": (_i, [C.c_uint64, _vp]),
    "segk_build_id": (C.c_char_p, []),
    "segk_last_error": (C.c_char_p, []),
    "segk_nchw_to_nhwc": (_i, [_fp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "segk_nhwc_to_nchw": (_i, [_vp, _fp, _i, _i, _i, _i, _i, _i, _vp]),
    "segk_pack_conv_weight": (_i, [_fp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "segk_pack_conv3x3_both": (_i, [_fp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "segk_pack_multi": (_i, [_vp, _i, _i, _i, _vp]),
    "segk_pack_convt_chunk": (_i, []),
    "segk_pack_convt_weight": (_i, [_fp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "segk_conv_tiles": (_i, [_i, _i, _i, _i, _i, _i]),
    "segk_bn_stats_floats": (_i, [_i, _i]),
    "segk_conv3x3": (_i, [_vp, _vp, _vp, _fp, _fp, _fp, _vp, _vp, _fp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "segk_conv_writes_act_q": (_i, [_i, _i, _i]),
    "segk_conv3x3_act": (_i, [_vp, _vp, _fp, _fp, _vp, _vp, _fp, _i, _i, _i, _i, _i, _i, _vp]),
    "segk_stem3x3_rows": (_i, [_i, _i, _i, _i, _i, _i]),
    "segk_stem3x3": (_i, [_fp, _fp, _vp, _vp, _fp, _i, _i, _i, _i, _i, _i, _vp]),
    "segk_stem3x3_wgrad_slabs": (_i, [_i, _i, _i, _i, _i, _i]),
    "segk_stem3x3_wgrad": (_i, [_fp, _vp, _fp, _i, _i, _i, _i, _i, _i, _vp]),
    "segk_stem3x3_wgrad_bn": (_i, [_fp, _vp, _vp, _fp, _fp, _fp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _i, _vp]),
    "segk_conv1x1": (_i, [_vp, _vp, _fp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "segk_convt2x2_fwd": (_i, [_vp, _vp, _fp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "segk_convt2x2_dgrad": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "segk_wgrad_tiles": (_i, [_i, _i, _i, _i, _i]),
    "segk_wgrad_split": (_i, [_i, _i, _i, _i, _i, _i]),
    "segk_wgrad": (_i, [_vp, _vp, _vp, _fp, _fp, _fp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "segk_wgrad_reduce": (_i, [_fp, _i, _fp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "segk_wgrad_reduce_multi": (_i, [_vp, _i, _vp]),
    "segk_bn_finalize": (_i, [_fp, _i, _i, _i, _d, _fp, _fp, _fp, _fp, _fp, _f, _f, _i, _fp, _fp, _fp, _fp, _vp]),
    "segk_bn_relu_apply": (_i, [_vp, _vp, _fp, _fp, _l, _i, _i, _vp]),
    "segk_bn_relu_apply_pool": (_i, [_vp, _vp, _vp, _fp, _fp, _i, _i, _i, _i, _i, _vp]),
    "segk_bn_bwd_blocks": (_i, [_l, _i, _i]),
    "segk_bn_relu_bwd": (_i, [_vp, _vp, _vp, _fp, _fp, _fp, _fp, _l, _i, _i, _fp, _fp, _fp, _fp, _i, _vp]),
    "segk_channel_sum": (_i, [_vp, _l, _i, _i, _fp, _fp, _i, _vp]),
    "segk_maxpool2x2_fwd": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "segk_maxpool2x2_bwd": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "segk_maxpool_bwd_stat_blocks": (_i, [_i, _i, _i, _i, _i]),
    "segk_maxpool2x2_bwd_bnstat": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _fp, _fp, _fp, _fp, _fp, _vp, _i, _vp]),
    "segk_bn_relu_bwd_from_part": (_i, [_vp, _vp, _vp, _fp, _fp, _fp, _fp, _l, _i, _i, _fp, _i, _fp, _fp, _fp, _i, _vp]),
    "segk_bn_relu_bwd_stats": (_i, [_vp, _vp, _fp, _fp, _fp, _fp, _l, _i, _i, _fp, _fp, _fp, _fp, _i, _vp]),
    "segk_bilinear_fwd": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "segk_bilinear_bwd": (_i, [_vp, _vp, _fp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "segk_linear": (_i, [_vp, _vp, _fp, _vp, _l, _i, _i, _i, _i, _vp]),
    "segk_vit_patchify": (_i, [_fp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "segk_vit_embed_ln": (_i, [_vp, _fp, _fp, _fp, _fp, _f, _fp, _i, _i, _i, _i, _i, _vp]),
    "segk_add_layernorm": (_i, [_fp, _vp, _fp, _fp, _f, _vp, _l, _i, _i, _i, _vp]),
    "segk_linear_splitk": (_i, [_vp, _vp, _fp, _vp, _l, _i, _i, _i, _i, _vp]),
    "segk_add_layernorm_parts": (_i, [_fp, _vp, _i, _l, _fp, _fp, _f, _vp, _l, _i, _i, _i, _vp]),
    "segk_attention": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _f, _i, _vp]),
    "segk_vit_tokens_to_grid": (_i, [_fp, _vp, _i, _i, _i, _i, _i, _vp]),
    "segk_resize_pad": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "segk_crop_resize": (_i, [_fp, _fp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "segk_resize_pad_u8": (_i, [_vp, _fp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "segk_predict_mask": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "segk_resize_pad_flip": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "segk_resize_pad_u8_flip": (_i, [_vp, _fp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "segk_predict_merge": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _fp, _vp]),
    "segk_tile_gather_u8": (_i, [_vp, _fp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "segk_tile_gather": (_i, [_fp, _fp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "segk_predict_tiles": (_i, [_fp, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _fp, _vp]),
    "segk_calib_hist": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "segk_calib_temps": (_i, [_fp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _i, _fp, _i, _vp, _vp, _vp, _vp, _vp]),
    "segk_cc_label": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "segk_cc_clean": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "segk_mask_finish": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "segk_vec_runs": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "segk_vec_rings": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "segk_raster_labels": (_i, [_vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _l, _i, _vp]),
    "segk_pq_pairs": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "segk_pq_match": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp]),
    "segk_morph": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "segk_byte_lut": (_i, [_vp, _vp, _vp, _l, _vp]),
    "segk_fill_holes": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "segk_mix_select": (_i, [_vp, _i, _i, _vp, _i, _i, _i, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _i, _i, _vp]),
    "segk_mix_apply": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _i, _vp, _i, _i, _i, _l, _vp]),
    "segk_boundary_stats": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "segk_boundary_finish": (_i, [_vp, _vp, _i, _i, _vp]),
    "segk_slic_start": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "segk_slic_assign": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "segk_slic_update": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "segk_snap_vote": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "segk_snap_paint": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _l, _l, _l, _l, _i, _i, _i, _i, _vp]),
    "segk_head_fwd": (_i, [_vp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "segk_head_fwd_bn": (_i, [_vp, _fp, _fp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "segk_head_bwd_bn": (_i, [_fp, _vp, _fp, _vp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _i, _fp, _fp, _fp, _fp, _fp, _i, _vp]),
    "segk_head_bwd_bn_stats": (_i, [_fp, _vp, _fp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _i, _fp, _fp, _fp, _fp, _fp, _i, _vp]),
    "segk_head_bn_bwd_apply": (_i, [_fp, _vp, _fp, _vp, _fp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _i, _fp, _i, _fp, _fp, _fp, _i, _vp]),
    "segk_head_part_floats": (_i, [_l, _i]),
    "segk_head_bwd": (_i, [_fp, _vp, _fp, _vp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "segk_head_bwd_blocks": (_i, [_l]),
    "segk_head_bwd_bnstat": (_i, [_fp, _vp, _fp, _vp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _i, _fp, _fp, _fp, _fp, _fp, _i, _vp]),
    "segk_loss_part_floats": (_i, [_l]),
    "segk_loss_state_floats": (_i, []),
    "segk_loss_fwd": (_i, [_fp, _vp, _fp, _i, _i, _l, _i, _f, _f, _f, _fp, _fp, _fp, _vp]),
    "segk_loss_bwd": (_i, [_fp, _vp, _fp, _fp, _fp, _i, _i, _l, _i, _f, _f, _fp, _vp]),
    "segk_distill_fwd": (_i, [_fp, _vp, _i, _vp, _i, _i, _i, _i, _i, _f, _f, _f, _fp, _fp, _fp, _vp]),
    "segk_distill_bwd": (_i, [_fp, _vp, _i, _vp, _fp, _fp, _i, _i, _i, _i, _i, _f, _f, _f, _fp, _vp]),
    "segk_hard_loss_fwd": (_i, [_fp, _vp, _fp, _i, _i, _l, _i, _f, _f, _i, _f, _i, _i, _vp, _vp, _fp, _fp, _fp, _vp]),
    "segk_hard_loss_bwd": (_i, [_fp, _vp, _fp, _vp, _fp, _fp, _i, _i, _l, _i, _f, _f, _i, _fp, _vp]),
    "segk_lovasz_fwd": (_i, [_fp, _vp, _fp, _i, _i, _l, _i, _i, _i, _vp, _l, _fp, _vp, _fp, _vp]),
    "segk_lovasz_bwd": (_i, [_fp, _vp, _fp, _vp, _fp, _i, _i, _l, _i, _i, _fp, _vp]),
    "segk_prompt_mix_fwd": (_i, [_fp, _fp, _fp, _i, _l, _vp]),
    "segk_prompt_mix_bwd": (_i, [_fp, _fp, _fp, _fp, _i, _l, _vp]),
    "segk_prob_loss_fwd": (_i, [_fp, _vp, _fp, _i, _i, _l, _i, _f, _f, _f, _i, _f, _fp, _fp, _fp, _vp]),
    "segk_prob_loss_bwd": (_i, [_fp, _vp, _fp, _fp, _fp, _i, _i, _l, _i, _f, _f, _i, _f, _fp, _vp]),
    "segk_confusion": (_i, [_fp, _vp, _i, _i, _l, _vp, _vp]),
    "segk_recon_head_fwd": (_i, [_vp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "segk_recon_sigmoid_bwd": (_i, [_fp, _fp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "segk_mse_fwd": (_i, [_fp, _fp, _fp, _i, _fp, _l, _i, _vp]),
    "segk_mse_bwd": (_i, [_fp, _fp, _fp, _fp, _fp, _l, _i, _vp]),
    "segk_prompt_scores": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _i, _i, _i, _i, _vp]),
    "segk_prompt_make": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _fp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "segk_prompt_heatmap": (_i, [_vp, _i, _vp, _i, _fp, _i, _i, _vp]),
    "segk_aug_prefilter": (_i, [_vp, _i, _i, _vp]),
    "segk_aug_resample": (_i, [_vp, _i, _i, _vp, _vp, _i, _vp, _i, _vp, _i, _vp, _fp, _vp, _vp, _vp]),
    "segk_aug_merge": (_i, [_vp, _vp, _i, _i, _vp, _fp, _vp, _vp, _vp]),
    "segk_label_hist": (_i, [_vp, _l, _i, _i, _i, _l, _vp, _vp]),
    "segk_rgb_label_to_classes": (_i, [_vp, _vp, _l, _vp]),
    "segk_perturb_point": (_i, [_vp, _i, _i, _i, _vp, _vp]),
    "segk_perturb_blur": (_i, [_vp, _i, _i, _i, _vp]),
    "segk_optim_grad_norm": (_i, [_vp, _i, _i, _vp, _i, _vp, _vp, _d, _i, _i, _vp]),
    "segk_optim_adamw": (_i, [_vp, _i, _i, _vp, _i, _vp, _i, _i, _vp]),
}



class ReduceJob(C.Structure):
    """segk_reduce_job of include/segk.h (one reduction of segk_wgrad_reduce_multi)."""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("kind", C.c_int), ("S", C.c_int), ("N", C.c_int), ("CA", C.c_int),
                ("CB", C.c_int), ("Np", C.c_int), ("CAp", C.c_int), ("CBp", C.c_int), ("taps", C.c_int), ("pad_", C.c_int)]


class PackEntry(C.Structure):
    """SegkPackEntry of csrc/segk_internal.h (one tensor of segk_pack_multi's device table, 64 bytes)."""
    _fields_ = [("w", C.c_void_p), ("dst_fwd", C.c_void_p), ("dst_dgrad", C.c_void_p), ("Cout", C.c_int), ("CA", C.c_int),
                ("CB", C.c_int), ("Coutp", C.c_int), ("CAp", C.c_int), ("CBp", C.c_int), ("block0", C.c_int), ("kind", C.c_int),
                ("pad_", C.c_int * 2)]


class OptimRec(C.Structure):
    """segk_optim_rec of include/segk.h (one tensor of the optimizer table, 64 bytes)."""
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("shadow", C.c_void_p),
                ("numel", C.c_int64), ("block0", C.c_int32), ("group", C.c_int32), ("pad_", C.c_int32 * 2)]


class OptimGroup(C.Structure):
    """segk_optim_group of include/segk.h (the per-step scalars of one param group, 64 bytes)."""
    _fields_ = [("lr", C.c_float), ("decay", C.c_float), ("omb1", C.c_float), ("b2", C.c_float), ("omb2", C.c_float),
                ("eps", C.c_float), ("omd", C.c_float), ("ema_decay", C.c_float), ("beta1", C.c_double), ("beta2", C.c_double),
                ("pad_", C.c_int32 * 4)]


_lib = None


def load():
    """Load libsegk.so (building nothing: run `python -m image_segmentation_amd.build` or
    __graft_entry__.build() first).  Raises if the library is absent -- there is no fallback path."""
    global _lib, LIB_PATH
    if _lib is None:
        if os.environ.get("SEGK_LIB"):       # diagnostic builds only (tools/stamp_build.sh, same-box A/B of two builds)
            LIB_PATH = os.path.abspath(os.environ["SEGK_LIB"])
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: the HIP extension is required (no CPU/eager fallback exists). "
                "Build it with `python -m image_segmentation_amd.build`.")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            try:
                fn = getattr(lib, name)
            except AttributeError:
                raise RuntimeError(f"{LIB_PATH} does not export {name}: it was built from another include/segk.h than "
                                   "this binding (rebuild with `python -m image_segmentation_amd.build`)") from None
            fn.restype = res
            fn.argtypes = args
        # A library built against another header is refused (SEGK_LIB / --lib diagnostic builds included): the host sizes
        # buffers with this table's queries, so a kernel set with other geometry rules must never run behind it
        ver, nent = lib.segk_version(), lib.segk_entry_count()
        if ver != ABI_VERSION or nent != len(SIGNATURES):
            raise RuntimeError(f"{LIB_PATH}: ABI version {ver} with {nent} entries, this binding expects version "
                               f"{ABI_VERSION} with {len(SIGNATURES)} entries -- refusing to drive a library built from "
                               "another include/segk.h")
        _lib = lib
    return _lib


def call(name, *args):
    """Invoke an int-returning entry point; raise with the library's message on failure."""
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise RuntimeError(f"{name} failed ({rc}): {lib.segk_last_error().decode()}")


def build_id():
    """Source hash compiled into the loaded library (see build.source_hash)."""
    return load().segk_build_id().decode()


def query(name, *args):
    """Invoke a pure size/geometry query (returns its int result)."""
    return getattr(load(), name)(*args)
