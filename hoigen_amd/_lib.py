"""ctypes binding of ``libhoigen_amd.so`` (the C ABI declared in ``include/hoigen_amd.h``).

This is the only place the native library is touched.  There is **no CPU fallback**: if the library
is missing, or no HIP device is present when a compute entry point is called, a ``RuntimeError`` is
raised.  The structures below mirror the header field by field.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import threading
from typing import Dict, Optional

HERE = os.path.dirname(os.path.abspath(__file__))
# HG_LIB_PATH: load another build of the same ABI (A/B timing of kernel variants inside one GPU session)
LIB_PATH = os.environ.get("HG_LIB_PATH") or os.path.join(HERE, "csrc", "libhoigen_amd.so")
HG_MAX_SLOTS = 16
HG_F32, HG_F16 = 0, 1


class hg_tensor(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("dtype", C.c_int32)]


_BLOCK_FIELDS = ["in_proj_weight", "in_proj_bias", "out_proj_weight", "out_proj_bias", "ln_1_weight",
                 "ln_1_bias", "c_fc_weight", "c_fc_bias", "c_proj_weight", "c_proj_bias", "ln_2_weight",
                 "ln_2_bias"]


class hg_block_weights(C.Structure):
    _fields_ = [(n, hg_tensor) for n in _BLOCK_FIELDS]


_DEC_FIELDS = ["attn_in_proj_weight", "attn_in_proj_bias", "attn_out_proj_weight", "attn_out_proj_bias",
               "linear1_weight", "linear1_bias", "linear2_weight", "linear2_bias", "norm2_weight",
               "norm2_bias", "norm3_weight", "norm3_bias"]


class hg_decoder_layer_weights(C.Structure):
    _fields_ = [(n, hg_tensor) for n in _DEC_FIELDS]


class hg_adapter_weights(C.Structure):
    _fields_ = [("present", C.c_int32), ("bottleneck", C.c_int32), ("scale", hg_tensor),
                ("down_proj_weight", hg_tensor), ("down_proj_bias", hg_tensor),
                ("up_proj_weight", hg_tensor), ("up_proj_bias", hg_tensor),
                ("prior_layer", hg_decoder_layer_weights), ("self_layer", hg_decoder_layer_weights),
                ("n_extra_prior_layers", C.c_int32), ("extra_prior_layers", C.POINTER(hg_decoder_layer_weights))]


class hg_vit_weights(C.Structure):
    _fields_ = [("width", C.c_int32), ("layers", C.c_int32), ("heads", C.c_int32), ("patch_size", C.c_int32),
                ("input_resolution", C.c_int32), ("output_dim", C.c_int32),
                ("conv1_weight", hg_tensor), ("class_embedding", hg_tensor), ("positional_embedding", hg_tensor),
                ("ln_pre_weight", hg_tensor), ("ln_pre_bias", hg_tensor), ("ln_post_weight", hg_tensor),
                ("ln_post_bias", hg_tensor), ("proj", hg_tensor),
                ("blocks", C.POINTER(hg_block_weights)), ("adapters", C.POINTER(hg_adapter_weights))]


class hg_text_weights(C.Structure):
    _fields_ = [("width", C.c_int32), ("layers", C.c_int32), ("heads", C.c_int32),
                ("context_length", C.c_int32), ("vocab_size", C.c_int32), ("output_dim", C.c_int32),
                ("token_embedding", hg_tensor), ("positional_embedding", hg_tensor),
                ("ln_final_weight", hg_tensor), ("ln_final_bias", hg_tensor), ("text_projection", hg_tensor),
                ("blocks", C.POINTER(hg_block_weights))]


class hg_vae_weights(C.Structure):
    _fields_ = [("dim", C.c_int32), ("enc_hidden", C.c_int32), ("gen_hidden", C.c_int32),
                ("enc_w0", hg_tensor), ("enc_b0", hg_tensor), ("enc_mean_w", hg_tensor), ("enc_mean_b", hg_tensor),
                ("enc_logvar_w", hg_tensor), ("enc_logvar_b", hg_tensor), ("gen_w0", hg_tensor),
                ("gen_b0", hg_tensor), ("gen_w2", hg_tensor), ("gen_b2", hg_tensor)]


class hg_mlp_weights(C.Structure):
    _fields_ = [("in_dim", C.c_int32), ("hidden_dim", C.c_int32), ("out_dim", C.c_int32),
                ("w0", hg_tensor), ("b0", hg_tensor), ("w2", hg_tensor), ("b2", hg_tensor),
                ("w4", hg_tensor), ("b4", hg_tensor)]


class hg_cache_weights(C.Structure):
    _fields_ = [("weight", hg_tensor), ("bias", hg_tensor), ("labels", hg_tensor), ("sample_lens", hg_tensor),
                ("S", C.c_int32), ("K", C.c_int32), ("C", C.c_int32), ("post_div", C.c_float)]


HG_HOI_MAX_BRANCH = 6
HG_HOI_SRC = {"human": 0, "object": 1, "union": 2, "human_object": 3, "global": 4, "image": 5}
HG_HOI_MAX_K_IMG = 4096


class hg_hoi_branch(C.Structure):
    _fields_ = [("source", C.c_int32), ("slot", C.c_int32), ("scale", C.c_float)]


class hg_hoi_head_args(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("feat_local", "feat_global", "boxes", "scores", "labels")] + \
               [("box_off", C.POINTER(C.c_int32)), ("n_human", C.POINTER(C.c_int32))] + \
               [(n, C.c_int32) for n in ("B", "C", "H", "W", "P")] + [("spatial_scale", C.c_float), ("n_branch", C.c_int32),
                ("branch", hg_hoi_branch * HG_HOI_MAX_BRANCH), ("obj2target", C.c_void_p), ("n_obj_classes", C.c_int32),
                ("num_classes", C.c_int32), ("score_pow", C.c_float)] + \
               [(n, C.c_void_p) for n in ("pair_h", "pair_o", "objects", "union_boxes", "pooled_single", "pooled_union", "feats",
                                          "branch_logits", "logits", "prior", "scores_out")]


class hg_hoi_image_args(C.Structure):
    _fields_ = [("feat_image", C.c_void_p), ("K_img", C.c_int32), ("image_logits", C.c_void_p)]


HG_MAX_PRIOR_SLOTS = 4


class hg_prior_weights(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("E", "hidden", "out", "n_obj_classes")] + \
               [(n, hg_tensor) for n in ("w0", "b0", "w1", "b1", "w2", "b2", "object_embedding")]


class hg_region_priors_args(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("scores", "labels", "boxes")] + \
               [("q_off", C.POINTER(C.c_int32)), ("image_sizes", C.POINTER(C.c_float)), ("B", C.c_int32),
                ("box_score_thresh", C.c_float), ("nms_thresh", C.c_float)] + \
               [(n, C.c_int32) for n in ("human_idx", "min_instances", "max_instances", "prior_slot")] + \
               [(n, C.c_void_p) for n in ("counts", "keep", "out_boxes", "out_scores", "out_labels", "survivors", "priors", "mask",
                                          "table_out")]


class hg_hoi_detections_args(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("prior", "scores", "pair_h", "pair_o", "objects", "boxes")] + \
               [("pair_off", C.POINTER(C.c_int32)), ("box_off", C.POINTER(C.c_int32)), ("B", C.c_int32), ("num_classes", C.c_int32),
                ("conversion", C.c_void_p), ("n_obj_classes", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("gt_boxes_h", "gt_boxes_o", "gt_hoi")] + \
               [("gt_off", C.POINTER(C.c_int32)), ("gt_sizes", C.POINTER(C.c_int32)), ("gt_format", C.c_int32), ("min_iou", C.c_float),
                ("cap", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("det_off", "det_pair", "det_verb", "det_h", "det_o", "det_object", "det_score", "det_interaction",
                                          "det_label", "det_gt", "det_max_iou", "gt_boxes_out", "status")]


HG_PRE_MAX_IMAGES, HG_PRE_MAX_N, HG_PRE_MAX_NPX, HG_PRE_MAX_TAPS = 64, 4096, 518, 65      # limits of one hg_preprocess_batch call


class hg_preprocess_batch_args(C.Structure):
    _fields_ = [("images", C.POINTER(C.c_void_p)), ("heights", C.POINTER(C.c_int32)), ("widths", C.POINTER(C.c_int32)), ("B", C.c_int32),
                ("boxes", C.c_void_p), ("crop_image", C.c_void_p), ("n", C.c_int32), ("n_px", C.c_int32), ("flags", C.c_int32),
                ("background", C.c_uint32), ("out", C.c_void_p), ("out_u8", C.c_void_p), ("status", C.c_void_p)]


# limits of one hg_detector_views call, and the tiling of its kernel (hoigen_amd/csrc/hg_detector_views_geom.h): output rows of a band at
# most, output columns of a strip, strips of a workgroup, rows of the window in LDS
HG_DV_MAX_IMAGES, HG_DV_MAX_SIDE, HG_DV_MAX_TAPS, HG_DV_MAX_CLIP_PX = 64, 2048, 65, 518
HG_DV_BAND, HG_DV_STRIP, HG_DV_STRIPS, HG_DV_WIN_ROWS = 32, 64, 4, 72


class hg_detector_views_args(C.Structure):
    _fields_ = [("images", C.POINTER(C.c_void_p)), ("heights", C.POINTER(C.c_int32)), ("widths", C.POINTER(C.c_int32))] + \
               [(n, C.c_int32) for n in ("B", "size", "max_size", "clip_px", "hmax", "wmax")] + \
               [(n, C.c_void_p) for n in ("resized_u8", "detr", "mask", "clip")]


_DETR_LAYER_FIELDS = ["in_proj_weight", "in_proj_bias", "out_proj_weight", "out_proj_bias", "linear1_weight", "linear1_bias",
                      "linear2_weight", "linear2_bias", "norm1_weight", "norm1_bias", "norm2_weight", "norm2_bias"]
HG_DETR_ATTN_MAX_L = 1792      # tokens per image of one hg_detr_encoder call at most (hoigen_amd/csrc/hg_kernels.h)


class hg_detr_layer_weights(C.Structure):
    _fields_ = [(n, hg_tensor) for n in _DETR_LAYER_FIELDS]


class hg_detr_encoder_weights(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("d_model", "heads", "d_ff", "n_layers", "normalize_before", "activation")] + \
               [("layers", C.POINTER(hg_detr_layer_weights))]


class hg_detr_encoder_args(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("src", "pos", "mask", "out", "trace")] + [("B", C.c_int32), ("S", C.c_int32),
                ("src_stride", C.c_int64 * 3), ("pos_stride", C.c_int64 * 3), ("out_stride", C.c_int64 * 3)]


_DETR_DEC_LAYER_FIELDS = _DETR_LAYER_FIELDS + ["cross_in_proj_weight", "cross_in_proj_bias", "cross_out_proj_weight", "cross_out_proj_bias",
                                               "norm3_weight", "norm3_bias"]


class hg_detr_dec_layer_weights(C.Structure):
    _fields_ = [(n, hg_tensor) for n in _DETR_DEC_LAYER_FIELDS]


class hg_detr_decoder_weights(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("d_model", "heads", "d_ff", "n_layers", "normalize_before", "activation")] + \
               [("norm_weight", hg_tensor), ("norm_bias", hg_tensor), ("layers", C.POINTER(hg_detr_dec_layer_weights))]


class hg_detr_decoder_args(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("tgt", "query_pos", "memory", "pos", "memory_mask", "out", "trace")] + \
               [(n, C.c_int32) for n in ("B", "S", "Q", "return_intermediate")] + \
               [(n, C.c_int64 * 3) for n in ("tgt_stride", "query_pos_stride", "memory_stride", "pos_stride")] + [("out_stride", C.c_int64 * 4)]


# limits of one hg_detr_heads call (hoigen_amd/csrc/hg_kernels.h): logits, levels, images, queries
HG_DETR_HEADS_MAX_C, HG_DETR_HEADS_MAX_L, HG_DETR_HEADS_MAX_B, HG_DETR_HEADS_MAX_Q = 256, 12, 64, 1792


class hg_detr_heads_weights(C.Structure):
    _fields_ = [(n, hg_tensor) for n in ("class_weight", "class_bias", "l0_w", "l0_b", "l1_w", "l1_b", "l2_w", "l2_b")] + \
               [("d_model", C.c_int32), ("n_logits", C.c_int32), ("class_rows", C.POINTER(C.c_int32)), ("n_class_rows", C.c_int32)]


class hg_detr_heads_args(C.Structure):
    _fields_ = [("hs", C.c_void_p), ("hs_stride", C.c_int64 * 3), ("L", C.c_int32), ("B", C.c_int32), ("Q", C.c_int32),
                ("target_sizes", C.POINTER(C.c_float))] + \
               [(n, C.c_void_p) for n in ("pred_logits", "pred_boxes", "scores", "labels", "boxes")]


# limits of one hg_detr_neck call (hoigen_amd/csrc/hg_kernels.h): input channels, images, image-mask side
HG_DETR_NECK_MAX_CIN, HG_DETR_NECK_MAX_B, HG_DETR_NECK_MAX_IMG = 4096, 64, 8192


class hg_detr_neck_weights(C.Structure):
    _fields_ = [("weight", hg_tensor), ("bias", hg_tensor), ("cin", C.c_int32), ("d_model", C.c_int32), ("num_pos_feats", C.c_int32),
                ("temperature", C.c_float), ("normalize", C.c_int32), ("scale", C.c_float)]


class hg_detr_neck_args(C.Structure):
    _fields_ = [("x", C.c_void_p), ("x_stride", C.c_int64 * 3), ("image_mask", C.c_void_p), ("Hi", C.c_int32), ("Wi", C.c_int32),
                ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("src", C.c_void_p), ("src_stride", C.c_int64 * 2),
                ("pos", C.c_void_p), ("pos_stride", C.c_int64 * 2), ("mask", C.c_void_p)]


# limits of hg_load_resnet_stages / hg_resnet_stages (hoigen_amd/csrc/hg_kernels.h): channels, input channels of a 3 x 3, side, images, blocks
HG_RESNET_MAX_C, HG_RESNET_MAX_C3, HG_RESNET_MAX_SIDE, HG_RESNET_MAX_B, HG_RESNET_MAX_BLOCKS = 2048, 512, 1024, 64, 64


class hg_resnet_conv(C.Structure):
    _fields_ = [("weight", C.c_void_p)] + [(n, C.c_int32) for n in ("cout", "cin", "kh", "kw", "stride_h", "stride_w", "pad_h", "pad_w",
                                                                   "dil_h", "dil_w", "groups", "has_bias")]


class hg_resnet_norm(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("weight", "bias", "running_mean", "running_var")] + [("eps", C.c_double)]


class hg_resnet_block(C.Structure):
    _fields_ = [(n, hg_resnet_conv) for n in ("conv1", "conv2", "conv3", "down_conv")] + \
               [(n, hg_resnet_norm) for n in ("bn1", "bn2", "bn3", "down_bn")] + [("has_downsample", C.c_int32), ("ends_level", C.c_int32)]


class hg_resnet_weights(C.Structure):
    _fields_ = [("blocks", C.POINTER(hg_resnet_block)), ("n_blocks", C.c_int32)]


class hg_resnet_args(C.Structure):
    _fields_ = [("x", C.c_void_p), ("x_stride", C.c_int64 * 3), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("first_block", C.c_int32), ("last_block", C.c_int32), ("out", C.c_void_p), ("out_stride", C.c_int64 * 2),
                ("trace", C.POINTER(C.c_void_p))]


class hg_test_resnet_conv_args(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("x", "w", "scale", "bias", "identity", "out32", "out16")] + \
               [(n, C.c_int32) for n in ("B", "H", "W", "cin", "cout", "k", "stride", "epi", "tile")]


class hg_resnet_stem_weights(C.Structure):
    _fields_ = [("conv1", hg_resnet_conv), ("bn1", hg_resnet_norm)] + \
               [(n, C.c_int32) for n in ("pool_kernel", "pool_stride", "pool_padding", "pool_dilation", "pool_ceil_mode")]


class hg_resnet_stem_args(C.Structure):
    _fields_ = [("x", C.c_void_p), ("x_stride", C.c_int64 * 3), ("B", C.c_int32), ("Hi", C.c_int32), ("Wi", C.c_int32),
                ("out", C.c_void_p), ("out_stride", C.c_int64 * 2)]


class hg_resnet_body_args(C.Structure):
    _fields_ = [("x", C.c_void_p), ("x_stride", C.c_int64 * 3), ("B", C.c_int32), ("Hi", C.c_int32), ("Wi", C.c_int32),
                ("last_block", C.c_int32), ("out", C.c_void_p), ("out_stride", C.c_int64 * 2), ("trace", C.POINTER(C.c_void_p))]


class hg_resnet_features_args(C.Structure):
    _fields_ = [("x", C.c_void_p), ("x_stride", C.c_int64 * 3), ("B", C.c_int32), ("Hi", C.c_int32), ("Wi", C.c_int32),
                ("pooled", C.c_void_p), ("features", C.c_void_p), ("map_out", C.c_void_p), ("map_stride", C.c_int64 * 2)]


class hg_test_resnet_stem_args(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("x", "w", "scale", "bias", "out32", "out16")] + [(n, C.c_int32) for n in ("B", "Hi", "Wi")]


class hg_prof_rec(C.Structure):
    _fields_ = [("kind", C.c_int32), ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("ms", C.c_float)]


class hg_test_gemm_ex_args(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("a", "w", "bias", "out", "out_hi", "pos", "scale", "mu", "cs", "gamma", "out2", "out3", "mr_out", "mu_out")] + \
               [(n, C.c_int32) for n in ("M", "N", "K", "lda", "ldc", "epi", "kernel", "G", "L", "n_split", "ld2", "ld3", "chain", "stop")]


class hg_test_qkv_attn_ex_args(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("a", "w", "bias", "cs", "mr", "out", "qkv_out")] + \
               [(n, C.c_int32) for n in ("n_seq", "L", "heads", "fused", "lda", "ldo", "pad_fill")]


class hg_test_elem_args(C.Structure):
    _fields_ = [("p", C.c_void_p * 9), ("n", C.c_uint64), ("i", C.c_int32 * 6)]


class hg_test_detr_rows_args(C.Structure):
    _fields_ = [("p", C.c_void_p * 12), ("s", C.c_int64 * 4), ("i", C.c_int32 * 4)]


# the text tower's backward (hoigen_amd/csrc/hg_kernels.h): tokens per prompt at most; prompts per chunk of grad_ctx's first stage
HG_TEXT_GRAD_MAX_L, HG_PROMPTS_BWD_CHUNK = 80, 64

HG_PROF_OFF, HG_PROF_ALL, HG_PROF_ATTENTION, HG_PROF_QKV_ATTN = -1, -2, 100, 101
HG_PROF_DETR_FFN, HG_PROF_DETR_ROWS, HG_PROF_DETR_NECK = 104, 105, 106
HG_PROF_RESNET_CONV = 107
HG_PROF_RESNET_STEM = 108
HG_PROF_RESNET_POOL = 109
HG_PROF_TEXT_ATTN_BWD, HG_PROF_TEXT_GRAD_ROWS = 110, 111      # hg_text_backward_embeds: the attention backward; its row and elementwise launches
# threads of hg_resnet_pool.hip's workgroup: a thread's channels lie this far apart (hoigen_amd/csrc/hg_kernels.h)
HG_RESNET_POOL_THREADS = 256
# pooled pixels of a work item of hg_resnet_stem.hip (hoigen_amd/csrc/hg_kernels.h), and the largest image side of hg_resnet_stem
HG_RESNET_STEM_TILE, HG_RESNET_STEM_MAX_SIDE = (4, 8), 4 * HG_RESNET_MAX_SIDE

_P = C.c_void_p
_I = C.c_int
# name -> (restype, argtypes); must list every symbol of include/hoigen_amd.h (tests check this)
SIGNATURES = {
    "hg_create": (_P, [_I]),
    "hg_destroy": (None, [_P]),
    "hg_last_error": (C.c_char_p, [_P]),
    "hg_version": (C.c_char_p, []),
    "hg_load_vit": (_I, [_P, C.POINTER(hg_vit_weights)]),
    "hg_load_text": (_I, [_P, C.POINTER(hg_text_weights)]),
    "hg_load_vae": (_I, [_P, _I, C.POINTER(hg_vae_weights)]),
    "hg_load_mlp": (_I, [_P, _I, C.POINTER(hg_mlp_weights)]),
    "hg_update_adapters": (_I, [_P, C.POINTER(hg_adapter_weights), _I]),
    "hg_encode_image": (_I, [_P, _P, _I, _P, _P]),
    "hg_encode_image_prior": (_I, [_P, _P, _P, _P, _I, _I, _P, _P, _P]),
    "hg_encode_image_trace": (_I, [_P, _P, _I, _P, _P, _P]),
    "hg_encode_text_ids": (_I, [_P, _P, _I, _I, _P, _I, _P]),
    "hg_encode_text_embeds": (_I, [_P, _P, _P, _I, _I, _P, _I, _P]),
    "hg_encode_text_embeds_save": (_I, [_P, _P, _P, _I, _I, _P, _I, _P, _P]),
    "hg_text_backward_embeds": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _P]),
    "hg_token_embedding": (_I, [_P, _P, _I, _P, _P]),
    "hg_vae_forward": (_I, [_P, _I, _P, _P, _I, _P, _P, _P, _P, _P]),
    "hg_generator": (_I, [_P, _I, _P, _I, _P, _P]),
    "hg_mlp_net": (_I, [_P, _I, _P, _I, _P, _P]),
    "hg_assemble_prompts": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P]),
    "hg_assemble_prompts_backward": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "hg_l2_normalize": (_I, [_P, _P, _I, _I, _P, _P]),
    "hg_vae_loss": (_I, [_P, _P, _P, _P, _P, _I, _I, _P, _P]),
    "hg_roi_align": (_I, [_P, _P, _I, _I, _I, _P, _I, C.c_float, _I, _P, _P, _P]),
    "hg_load_cache": (_I, [_P, _I, _P]),
    "hg_cache_logits": (_I, [_P, _I, _P, _I, _P, _P]),
    "hg_hoi_head": (_I, [_P, C.POINTER(hg_hoi_head_args), _P]),
    "hg_hoi_head_image": (_I, [_P, C.POINTER(hg_hoi_head_args), C.POINTER(hg_hoi_image_args), _P]),
    "hg_load_priors": (_I, [_P, _I, C.POINTER(hg_prior_weights)]),
    "hg_region_priors": (_I, [_P, C.POINTER(hg_region_priors_args), _P]),
    "hg_hoi_detections": (_I, [_P, C.POINTER(hg_hoi_detections_args), _P]),
    "hg_preprocess_crops": (_I, [_P, _P, _I, _I, _P, _I, _I, _I, C.c_uint32, _P, _P, _P]),
    "hg_preprocess_batch": (_I, [_P, C.POINTER(hg_preprocess_batch_args), _P]),
    "hg_detector_view_shapes": (_I, [C.POINTER(C.c_int32), C.POINTER(C.c_int32), _I, _I, _I, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                     C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "hg_detector_views": (_I, [_P, C.POINTER(hg_detector_views_args), _P]),
    "hg_load_detr_encoder": (_I, [_P, C.POINTER(hg_detr_encoder_weights)]),
    "hg_detr_encoder": (_I, [_P, C.POINTER(hg_detr_encoder_args), _P]),
    "hg_load_detr_decoder": (_I, [_P, C.POINTER(hg_detr_decoder_weights)]),
    "hg_detr_decoder": (_I, [_P, C.POINTER(hg_detr_decoder_args), _P]),
    "hg_load_detr_heads": (_I, [_P, C.POINTER(hg_detr_heads_weights)]),
    "hg_detr_heads": (_I, [_P, C.POINTER(hg_detr_heads_args), _P]),
    "hg_load_detr_neck": (_I, [_P, C.POINTER(hg_detr_neck_weights)]),
    "hg_detr_neck": (_I, [_P, C.POINTER(hg_detr_neck_args), _P]),
    "hg_load_resnet_stages": (_I, [_P, C.POINTER(hg_resnet_weights)]),
    "hg_resnet_out_shape": (_I, [C.POINTER(hg_resnet_weights), _I, _I, _I, _I, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "hg_resnet_stages": (_I, [_P, C.POINTER(hg_resnet_args), _P]),
    "hg_load_resnet_stem": (_I, [_P, C.POINTER(hg_resnet_stem_weights)]),
    "hg_resnet_stem_out_shape": (_I, [_I, _I, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "hg_resnet_stem": (_I, [_P, C.POINTER(hg_resnet_stem_args), _P]),
    "hg_resnet_body": (_I, [_P, C.POINTER(hg_resnet_body_args), _P]),
    "hg_resnet_features": (_I, [_P, C.POINTER(hg_resnet_features_args), _P]),
    "hg_workspace_bytes": (_I, [_P, C.POINTER(C.c_uint64)]),
    "hg_set_option": (_I, [_P, C.c_char_p, _I]),
    "hg_get_option": (_I, [_P, C.c_char_p, C.POINTER(C.c_int32)]),
    "hg_test_gemm": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "hg_test_gemm_ex": (_I, [_P, C.POINTER(hg_test_gemm_ex_args), _P]),
    "hg_test_gemm_ln": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P]),
    "hg_test_attention": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P, _P]),
    "hg_test_detr_attention": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P]),
    "hg_test_detr_ffn": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P]),
    "hg_test_qkv_attn": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P]),
    "hg_test_qkv_attn_ex": (_I, [_P, C.POINTER(hg_test_qkv_attn_ex_args), _P]),
    "hg_test_gemm_hilo": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "hg_test_image_stream": (_I, [_P, _P, _I, _P, _P, _P]),
    "hg_test_text_stream": (_I, [_P, _P, _I, _I, _I, _P, _P, _P]),
    "hg_test_adapter": (_I, [_P, _I, _I, _P, _P, _I, _I, _I, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P]),
    "hg_test_elem": (_I, [_P, _I, C.POINTER(hg_test_elem_args), _P]),
    "hg_test_text_grad": (_I, [_P, _I, C.POINTER(hg_test_elem_args), _P]),
    "hg_test_detr_rows": (_I, [_P, _I, C.POINTER(hg_test_detr_rows_args), _P]),
    "hg_test_resnet_conv": (_I, [_P, C.POINTER(hg_test_resnet_conv_args), _P]),
    "hg_test_resnet_stem": (_I, [_P, C.POINTER(hg_test_resnet_stem_args), _P]),
    "hg_test_resnet_pool": (_I, [_P, _P, _I, _I, _I, _P, _P, _P]),
    "hg_profile_begin": (_I, [_P, _I, _I]),
    "hg_profile_end": (_I, [_P, _P, _I, C.POINTER(C.c_int32)]),
}

_lib = None
_lock = threading.RLock()   # re-entrant: ctx() calls lib() under the lock
_ctxs: Dict[int, int] = {}


def build(force: bool = False) -> str:
    """Compile the HIP sources for gfx950 with hipcc (cross-compiles without a GPU)."""
    script = os.path.join(HERE, "csrc", "build.sh")
    if force:
        for f in os.listdir(os.path.join(HERE, "csrc")):
            if f.endswith(".o"):
                os.remove(os.path.join(HERE, "csrc", f))
    subprocess.run(["bash", script], check=True)
    return LIB_PATH


def lib():
    """The loaded shared library (raises RuntimeError if it has not been built)."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise RuntimeError(
                        f"hoigen_amd: native library {LIB_PATH} is missing. Build it with "
                        "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc). "
                        "There is no CPU fallback.")
                try:
                    l = C.CDLL(LIB_PATH)
                except OSError as e:  # pragma: no cover
                    raise RuntimeError(f"hoigen_amd: cannot load {LIB_PATH}: {e}") from e
                for name, (res, args) in SIGNATURES.items():
                    fn = getattr(l, name)
                    fn.restype = res
                    fn.argtypes = args
                _lib = l
    return _lib


def ctx(device: int) -> int:
    """The per-device context handle (created on first use)."""
    h = _ctxs.get(device)
    if h is None:
        with _lock:
            h = _ctxs.get(device)
            if h is None:
                h = lib().hg_create(device)
                if not h:
                    raise RuntimeError(
                        f"hoigen_amd: hg_create({device}) failed - no HIP device. The hot path runs only on "
                        "an AMD GPU (gfx950); there is no CPU fallback.")
                _ctxs[device] = h
    return h


def check(device: int, rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().hg_last_error(ctx(device))
        raise RuntimeError(f"hoigen_amd: {what} failed ({rc}): {msg.decode() if msg else '?'}")


def profile(handle: int, kind: int, max_launches: int, fn):
    """Run ``fn()`` with hipEvent pairs around the launches of ``kind`` (HG_PROF_ALL: every GEMM / attention /
    fused-VAE launch) of the context ``handle``; returns ``(fn's result, [(kind, M, N, K, ms), ...])``."""
    l = lib()
    rc = l.hg_profile_begin(handle, kind, max_launches)
    if rc:
        raise RuntimeError(f"hoigen_amd: hg_profile_begin failed ({rc})")
    try:
        out = fn()
    finally:
        recs = (hg_prof_rec * max(1, max_launches))()
        n = C.c_int32()
        rc = l.hg_profile_end(handle, recs, max_launches, C.byref(n))
    if rc:
        raise RuntimeError(f"hoigen_amd: hg_profile_end failed ({rc})")
    return out, [(r.kind, r.M, r.N, r.K, float(r.ms)) for r in recs[: n.value]]


def tensor(t: Optional["object"]) -> hg_tensor:
    """hg_tensor view of a contiguous CUDA(HIP) torch tensor (fp32 or fp16)."""
    import torch

    if t is None:
        return hg_tensor(None, 0)
    if not t.is_cuda:
        raise RuntimeError("hoigen_amd: weights must live on a HIP device (call .cuda() on the module)")
    if t.dtype == torch.float32:
        dt = HG_F32
    elif t.dtype == torch.float16:
        dt = HG_F16
    else:
        raise RuntimeError(f"hoigen_amd: unsupported weight dtype {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError("hoigen_amd: weight tensors must be contiguous")
    return hg_tensor(t.data_ptr(), dt)
