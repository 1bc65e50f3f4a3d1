"""ctypes binding of libbevf_hip.so (include/bevf.h).  Fails loudly if the library is missing.

This is the one module that knows the C ABI: every launch in the package goes through a wrapper
here.  A wrapper takes torch CUDA tensors, checks buffer sizes, device / dtype / contiguity on
the host, passes raw `data_ptr()`s and launches on torch's current HIP stream, so the launches are
ordered with (and graph-capturable alongside) everything else torch does on that stream.
There is no CPU fallback: a CPU tensor raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libbevf_hip.so")


class BevfError(RuntimeError):
    pass


class ConvDesc(C.Structure):
    _fields_ = [("x", C.c_void_p), ("w", C.c_void_p), ("scale", C.c_void_p), ("shift", C.c_void_p),
                ("res", C.c_void_p), ("y", C.c_void_p), ("colmax", C.c_void_p)] + \
               [(n, C.c_int32) for n in ("N", "H", "W", "Cin", "x_cs", "Ho", "Wo", "Cout", "y_cs", "res_cs",
                                         "KH", "KW", "stride", "pad", "relu", "rows_per_group", "tile")] + \
               [(n, C.c_void_p) for n in ("stats", "stats_pivot", "bnb_x", "bnb_y", "bnb_mean", "bnb_invstd", "bnb_gamma",
                                          "bnb_beta")]


class RadarDesc(C.Structure):
    _fields_ = [("x", C.c_void_p), ("w", C.c_void_p * 4), ("scale", C.c_void_p * 4), ("shift", C.c_void_p * 4),
                ("out", C.c_void_p), ("R", C.c_int32), ("B", C.c_int32), ("P", C.c_int32), ("Cin", C.c_int32),
                ("c", C.c_int32 * 4)]


class HeadDesc(C.Structure):
    _fields_ = [("hid", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("out", C.c_void_p * 5),
                ("B", C.c_int32), ("P", C.c_int32), ("hc", C.c_int32), ("c", C.c_int32 * 5),
                ("n_sigmoid", C.c_int32)]


class DecodeDesc(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("heat", "offset", "size", "rot", "vel", "boxes", "scores", "labels",
                                          "velocities", "count", "work", "pool_ind")] + \
               [(n, C.c_int32) for n in ("B", "C", "H", "W", "K", "true_labels", "raw_scores")] + \
               [(n, C.c_float) for n in ("thresh", "voxel", "x_min", "y_min")]


class TargetsDesc(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("boxes", "labels", "has_vel", "heatmap", "offset", "size", "rot", "vel",
                                          "mask", "ind", "reg_mask", "target_offset", "target_size", "target_rot",
                                          "target_vel", "owner_scratch")] + \
               [(n, C.c_int32) for n in ("B", "nmax", "H", "W", "C", "max_objects", "min_radius")] + \
               [("pc_range", C.c_float * 6), ("gaussian_overlap", C.c_float)]


class WgradDesc(C.Structure):
    _fields_ = [("x", C.c_void_p), ("dy", C.c_void_p), ("dw", C.c_void_p), ("pixtab", C.c_void_p)] + \
               [(n, C.c_int32) for n in ("N", "H", "W", "Cin", "x_cs", "Cout", "dy_cs", "KH", "KW", "stride", "pad")]


class HeadBwdDesc(C.Structure):
    _fields_ = [("hid", C.c_void_p), ("w", C.c_void_p), ("out0", C.c_void_p), ("dout", C.c_void_p * 5),
                ("dhid", C.c_void_p), ("dw", C.c_void_p), ("db", C.c_void_p), ("B", C.c_int32), ("P", C.c_int32),
                ("hc", C.c_int32), ("c", C.c_int32 * 5), ("n_sigmoid", C.c_int32)]


class VoxelizeDesc(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("points", "voxel_features", "voxel_coords", "num_points", "num_voxels", "work")] + \
               [(n, C.c_int32) for n in ("B", "N", "C", "max_points", "max_voxels")] + \
               [("pc_range", C.c_float * 6), ("voxel_size", C.c_float * 3)]


class PillarGeom(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("voxel_features", "voxel_coords", "num_points", "num_voxels")] + \
               [(n, C.c_int32) for n in ("B", "Nv", "P", "C", "H", "W")] + [(n, C.c_float) for n in ("x0", "y0", "vx", "vy")]


class LossDesc(C.Structure):
    _fields_ = [("pred_heatmap", C.c_void_p), ("tgt_heatmap", C.c_void_p), ("pred_reg", C.c_void_p * 4),
                ("tgt_reg", C.c_void_p * 4), ("ind", C.c_void_p), ("reg_mask", C.c_void_p), ("work", C.c_void_p),
                ("out", C.c_void_p)] + [(n, C.c_int32) for n in ("B", "C", "H", "W", "K")] + \
               [("weights", C.c_float * 5)]


class DeconvDesc(C.Structure):
    """bevf_deconv_desc."""
    _fields_ = [(n, C.c_void_p) for n in ("x", "w", "scale", "shift", "y")] + \
               [(n, C.c_int32) for n in ("N", "H", "W", "Cin", "x_cs", "Cout", "y_cs", "s", "relu")]


_lib: Optional[C.CDLL] = None

# name -> (restype, argtypes); tests/test_abi_and_host.py holds these, and the Structures above, equal to include/bevf.h
SIGNATURES = {
    "bevf_version": (C.c_int, []),
    "bevf_last_error": (C.c_char_p, []),
    "bevf_conv2d_nhwc_f32": (C.c_int, [C.POINTER(ConvDesc), C.c_void_p]),
    "bevf_conv2d_nhwc_f32_if": (C.c_int, [C.POINTER(ConvDesc), C.c_void_p, C.c_void_p, C.c_void_p]),
    "bevf_conv2d_bound_f32x2": (C.c_int, [C.POINTER(ConvDesc), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "bevf_prune_compact_f32": (C.c_int, [C.c_void_p] * 6 + [C.c_int] * 4 + [C.c_void_p]),
    "bevf_stem_pool_f32": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 3 + [C.c_void_p]),
    "bevf_stem_conv7x7_f32": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 4 + [C.c_void_p]),
    "bevf_maxpool3x3s2_nhwc_f32": (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 4 + [C.c_void_p]),
    "bevf_pointwise_smallk_f32": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 4 + [C.c_void_p]),
    "bevf_pointnet_front_f32": (C.c_int, [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 11),
    "bevf_pointnet_front_pack_f32": (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 2 + [C.c_void_p]),
    "bevf_group_max_f32": (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 3 + [C.c_void_p]),
    "bevf_vfe_smallk_max_f32": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 4 + [C.c_void_p]),
    "bevf_radar_mlp_max_f32": (C.c_int, [C.POINTER(RadarDesc), C.c_void_p]),
    "bevf_linear_f32": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 6 + [C.c_void_p]),
    "bevf_cam_mean_f32": (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 4 + [C.c_void_p]),
    "bevf_bilinear_nhwc_f32": (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 8 + [C.c_void_p]),
    "bevf_broadcast_nhwc_f32": (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 4 + [C.c_void_p]),
    "bevf_expand_border_classes_f32": (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 5 + [C.c_void_p]),
    "bevf_head_tail_f32": (C.c_int, [C.POINTER(HeadDesc), C.c_void_p]),
    "bevf_nchw_to_nhwc_f32": (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 4 + [C.c_void_p]),
    "bevf_nhwc_to_nchw_f32": (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 4 + [C.c_void_p]),
    "bevf_fill_f32": (C.c_int, [C.c_void_p, C.c_float, C.c_size_t, C.c_void_p]),
    "bevf_wino_filter_floats": (C.c_size_t, [C.c_int] * 2),
    "bevf_wino_filter_transform_f32": (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 2 + [C.c_void_p]),
    "bevf_conv3x3_wino_f32": (C.c_int, [C.POINTER(ConvDesc), C.c_void_p]),
    "bevf_wino_stat_rows": (C.c_int, [C.c_int] * 3),
    "bevf_bn_backward_from_partials_f32": (C.c_int, [C.c_void_p] * 6 + [C.c_int] + [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_void_p]),
    "bevf_bn_stats_from_partials_f32": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int] * 2 + [C.c_float, C.c_void_p]),
    "bevf_centernet_decode_work_bytes": (C.c_size_t, [C.c_int] * 5),
    "bevf_centernet_decode_f32": (C.c_int, [C.POINTER(DecodeDesc), C.c_void_p]),
    "bevf_centernet_decode_rectify_f32": (C.c_int, [C.POINTER(DecodeDesc), C.c_void_p, C.c_void_p, C.c_void_p]),
    "bevf_centernet_targets_f32": (C.c_int, [C.POINTER(TargetsDesc), C.c_void_p]),
    "bevf_nms_keep_f32": (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 3 + [C.c_void_p]),
    "bevf_boxes_iou_f32": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 4 + [C.c_void_p]),
    "bevf_nms_boxes_work_bytes": (C.c_size_t, [C.c_int] * 2),
    "bevf_nms_boxes_f32": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 3 + [C.c_float] + [C.c_int] * 2 + [C.c_void_p] * 8),
    "bevf_centernet_loss_work_floats": (C.c_size_t, []),
    "bevf_centernet_loss_f32": (C.c_int, [C.POINTER(LossDesc), C.c_void_p]),
    # ---- IoU-aware head: IoU targets, IoU / DIoU loss ----
    "bevf_iou_targets_f32": (C.c_int, [C.c_void_p] * 9 + [C.c_int] * 4 + [C.c_float] * 4 + [C.c_void_p]),
    "bevf_iou_aware_loss_work_floats": (C.c_size_t, [C.c_int]),
    "bevf_iou_aware_loss_f32": (C.c_int, [C.c_void_p] * 11 + [C.c_int] * 4 + [C.c_float] * 6 + [C.c_void_p]),
    "bevf_iou_aware_loss_bwd_f32": (C.c_int, [C.c_void_p] * 12 + [C.c_int] * 4 + [C.c_float] * 6 + [C.c_void_p]),
    "bevf_voxelize_work_bytes": (C.c_size_t, [C.c_int] * 2),
    "bevf_voxelize_f32": (C.c_int, [C.POINTER(VoxelizeDesc), C.c_void_p]),
    "bevf_scatter_voxels_f32": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 6 + [C.c_void_p]),
    "bevf_pillar_work_bytes": (C.c_size_t, [C.c_int]),
    "bevf_pillar_pfn_f32": (C.c_int, [C.POINTER(PillarGeom)] + [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 2),
    "bevf_pillar_moments_f32": (C.c_int, [C.POINTER(PillarGeom)] + [C.c_void_p] * 4 + [C.c_int, C.c_float, C.c_float] +
                                [C.c_void_p] * 10),
    "bevf_pillar_pfn_backward_f32": (C.c_int, [C.POINTER(PillarGeom)] + [C.c_void_p] * 10 + [C.c_int] * 2 + [C.c_void_p] * 6),
    # ---- sparse-voxel LiDAR encoder ----
    "bevf_sparse_fill_index": (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 5 + [C.c_void_p] * 3),
    "bevf_sparse_down_work_bytes": (C.c_size_t, [C.c_int] * 4),
    "bevf_sparse_down": (C.c_int, [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p] * 5),
    "bevf_sparse_table": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 10 + [C.c_void_p] * 2),
    "bevf_sparse_vfe_mean_f32": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 5 + [C.c_void_p] * 2),
    "bevf_sparse_conv_f32": (C.c_int, [C.c_void_p] * 6 + [C.c_int] * 6 + [C.c_void_p] * 2),
    "bevf_sparse_conv_row_tile": (C.c_int, []),
    "bevf_sparse_wgrad_work_floats": (C.c_size_t, [C.c_int] * 2),
    "bevf_sparse_conv_wgrad_f32": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 6 + [C.c_void_p] * 3),
    "bevf_sparse_canvas_f32": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 6 + [C.c_void_p, C.c_int, C.c_void_p]),
    "bevf_sparse_canvas_bwd_f32": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 6 + [C.c_void_p] * 2),
    "bevf_sparse_bn_work_bytes": (C.c_size_t, [C.c_int]),
    "bevf_sparse_bn_stats_f32": (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 3 + [C.c_float] * 2 + [C.c_void_p] * 8),
    "bevf_sparse_bn_apply_f32": (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 3 + [C.c_void_p] * 6),
    "bevf_sparse_bn_backward_f32": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 6),
    # ---- input pipeline ----
    "bevf_resize_normalize_u8": (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 5 + [C.c_void_p] * 2 + [C.c_int] + [C.c_void_p] * 2 +
                                 [C.c_int] + [C.POINTER(C.c_float)] * 2 + [C.c_void_p]),
    "bevf_lidar_filter_pad_f32": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 3 + [C.POINTER(C.c_float), C.c_void_p]),
    # ---- training augmentation ----
    "bevf_resample_tables_box_f64": (C.c_int, [C.c_void_p] + [C.c_int] * 7 + [C.c_void_p] * 5),
    "bevf_resize_crop_u8": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 5 + [C.c_void_p] * 2 + [C.c_int] + [C.c_void_p] * 2 + [C.c_int] +
                            [C.c_void_p]),
    "bevf_jitter_flip_normalize_u8": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 3 + [C.POINTER(C.c_float)] * 2 + [C.c_void_p]),
    "bevf_points_affine_work_floats": (C.c_size_t, [C.c_int] * 3),
    "bevf_points_affine_filter_pad_f32": (C.c_int, [C.c_void_p] * 6 + [C.c_int] * 6 + [C.POINTER(C.c_float), C.c_void_p]),
    "bevf_points_affine_f32": (C.c_int, [C.c_void_p] * 3 + [C.c_float] + [C.c_int] * 5 + [C.c_void_p]),
    "bevf_boxes_affine_f32": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 3 + [C.c_void_p]),
    # ---- points in boxes, GT-paste ----
    "bevf_points_in_boxes_f32": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 5 + [C.c_void_p]),
    "bevf_paste_accept_f32": (C.c_int, [C.c_void_p] * 12 + [C.c_int] * 6 + [C.c_void_p]),
    "bevf_paste_points_work_ints": (C.c_size_t, [C.c_int] * 2),
    "bevf_paste_points_f32": (C.c_int, [C.c_void_p] * 11 + [C.c_int] * 7 + [C.c_void_p]),
    # ---- bf16 storage path ----
    "bevf_split_weights_f32x3": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "bevf_conv2d_nhwc_f32x3": (C.c_int, [C.POINTER(ConvDesc), C.c_void_p]),
    "bevf_conv2d_nhwc_bf16": (C.c_int, [C.POINTER(ConvDesc), C.c_void_p]),
    "bevf_conv3x3_pack_elems": (C.c_size_t, [C.c_int] * 2),
    "bevf_conv3x3_bf16_ct": (C.c_int, [C.c_int]),
    "bevf_conv3x3_pack_bf16": (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 2 + [C.c_void_p]),
    "bevf_conv3x3_bf16": (C.c_int, [C.POINTER(ConvDesc), C.c_void_p]),
    "bevf_debug_conv3x3_stamps": (C.c_int, [C.c_void_p]),
    "bevf_debug_wino_stamps": (C.c_int, [C.c_void_p]),
    "bevf_debug_wino_workgroups": (C.c_int, [C.c_int]),
    "bevf_stem_pack_bf16": (C.c_int, [C.c_void_p] * 3),
    "bevf_stem_conv7x7_bf16mma": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 4 + [C.c_void_p]),
    "bevf_stem_pool_bf16mma": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 3 + [C.c_void_p]),
    "bevf_stem_conv7x7_bf16out": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 4 + [C.c_void_p]),
    "bevf_maxpool3x3s2_nhwc_bf16": (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 4 + [C.c_void_p]),
    "bevf_pointwise_smallk_bf16out": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 4 + [C.c_void_p]),
    "bevf_linear_bf16w": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 7 + [C.c_void_p]),
    "bevf_cam_mean_bf16": (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 4 + [C.c_void_p]),
    "bevf_bilinear_nhwc_bf16": (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 8 + [C.c_void_p]),
    "bevf_broadcast_nhwc_bf16": (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 4 + [C.c_void_p]),
    "bevf_expand_border_classes_bf16": (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 5 + [C.c_void_p]),
    "bevf_head_tail_bf16": (C.c_int, [C.POINTER(HeadDesc), C.c_void_p]),
    # ---- training step ----
    "bevf_conv_pixtab_bytes": (C.c_size_t, [C.c_int] * 7),
    "bevf_conv_pixtab": (C.c_int, [C.c_void_p] + [C.c_int] * 8 + [C.c_void_p]),
    "bevf_conv2d_wgrad_f32": (C.c_int, [C.POINTER(WgradDesc), C.c_void_p]),
    "bevf_wino_wgrad_workspace_floats": (C.c_size_t, [C.c_int] * 5),
    "bevf_wino_wgrad_table_bytes": (C.c_size_t, [C.c_int] * 3),
    "bevf_wino_wgrad_table": (C.c_int, [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p]),
    "bevf_conv3x3_wgrad_wino_f32": (C.c_int, [C.POINTER(WgradDesc), C.c_void_p, C.c_int, C.c_void_p]),
    "bevf_zero_stuff_nhwc_f32": (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 7 + [C.c_void_p]),
    "bevf_stem_wgrad_f32": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_void_p]),
    "bevf_interleave2x2_nhwc_f32": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 4 + [C.c_void_p]),
    "bevf_bn_work_floats": (C.c_size_t, [C.c_int]),
    "bevf_bn_update_running_f32": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 2 + [C.c_float, C.c_void_p]),
    "bevf_bn_stats_f32": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 3 + [C.c_float, C.c_void_p]),
    "bevf_bn_apply_f32": (C.c_int, [C.c_void_p] * 7 + [C.c_int] * 4 + [C.c_void_p]),
    "bevf_bn_relu_group_max_idx_f32": (C.c_int, [C.c_void_p] * 8 + [C.c_int] * 3 + [C.c_void_p]),
    "bevf_gmax_bn_backward_f32": (C.c_int, [C.c_void_p] * 11 + [C.c_int] * 4 + [C.c_void_p]),
    "bevf_gmax_bn_sums_f32": (C.c_int, [C.c_void_p] * 9 + [C.c_int] * 4 + [C.c_void_p]),
    "bevf_bn_backward_f32": (C.c_int, [C.c_void_p] * 11 + [C.c_int] * 4 + [C.c_void_p]),
    "bevf_pool_bn_backward_f32": (C.c_int, [C.c_void_p] * 11 + [C.c_int] * 4 + [C.c_void_p]),
    "bevf_bn_relu_maxpool3x3s2_idx_f32": (C.c_int, [C.c_void_p] * 7 + [C.c_int] * 4 + [C.c_void_p]),
    "bevf_add_inplace_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "bevf_relu_mask_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "bevf_maxpool3x3s2_idx_f32": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_void_p]),
    "bevf_maxpool3x3s2_bwd_f32": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_void_p]),
    "bevf_bilinear_bwd_nhwc_f32": (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 8 + [C.c_void_p]),
    "bevf_cam_mean_bwd_f32": (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 4 + [C.c_void_p]),
    "bevf_group_max_idx_work_bytes": (C.c_size_t, [C.c_int] * 3),
    "bevf_group_max_idx_f32": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 3 + [C.c_void_p]),
    "bevf_group_max_bwd_f32": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_void_p]),
    "bevf_sparse_rows_wgrad_f32": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 4 + [C.c_void_p]),
    "bevf_sparse_rows_scatter_add_f32": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 4 + [C.c_void_p]),
    "bevf_linear_bwd_work_floats": (C.c_size_t, [C.c_int] * 3),
    "bevf_linear_bwd_f32": (C.c_int, [C.c_void_p] * 7 + [C.c_int] * 5 + [C.c_void_p]),
    "bevf_head_tail_bwd_f32": (C.c_int, [C.POINTER(HeadBwdDesc), C.c_void_p]),
    "bevf_centernet_loss_bwd_f32": (C.c_int, [C.POINTER(LossDesc), C.c_void_p * 5, C.c_void_p, C.c_void_p]),
    "bevf_stem_im2col_f32": (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 3 + [C.c_void_p]),
    "bevf_smallk_wgrad_f32": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_void_p]),
    "bevf_grad_norm_f32": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]),
    "bevf_adamw_step_f32": (C.c_int, [C.c_void_p] * 5 + [C.c_size_t] + [C.c_double] * 5 + [C.c_int, C.c_void_p]),
    "bevf_csr_gather_f32": (C.c_int, [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t]
                            + [C.c_int] * 3 + [C.c_void_p]),
    "bevf_csr_gather_bf16": (C.c_int, [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t]
                             + [C.c_int] * 3 + [C.c_void_p]),
    "bevf_camera_table_build_f64": (C.c_int, [C.c_void_p, C.c_int, C.c_int] + [C.c_float] * 4 + [C.c_int] * 2 + [C.c_float] * 2
                                    + [C.c_int, C.c_double] + [C.c_int] * 4 + [C.c_void_p] * 3 + [C.c_size_t, C.c_void_p, C.c_void_p]),
    "bevf_camera_table_transpose": (C.c_int, [C.c_void_p] * 3 + [C.c_size_t] + [C.c_int] * 3 + [C.c_void_p] * 5),
    "bevf_csr_gather_frames_f32": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p,
                                             C.c_size_t, C.c_int, C.c_void_p, C.c_size_t] + [C.c_int] * 3 + [C.c_void_p]),
    "bevf_csr_gather_frames_bf16": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p,
                                              C.c_size_t, C.c_int, C.c_void_p, C.c_size_t] + [C.c_int] * 3 + [C.c_void_p]),
    "bevf_softmax_rows_f32": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_size_t, C.c_int, C.c_void_p]),
    "bevf_softmax_rows_bwd_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_int,
                                            C.c_void_p]),
    "bevf_csr_lift_f32": (C.c_int, [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t,
                                    C.c_void_p, C.c_size_t] + [C.c_int] * 3 + [C.c_void_p]),
    "bevf_csr_lift_bwd_f32": (C.c_int, [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t,
                                        C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t]
                              + [C.c_int] * 2 + [C.c_void_p]),
    "bevf_frustum_table_sort_wave_rows": (C.c_int, []),
    "bevf_frustum_table_work_elems": (C.c_size_t, [C.c_int] * 7),
    "bevf_frustum_table_build_f64": (C.c_int, [C.c_void_p, C.c_int, C.c_int] + [C.c_float] * 4 + [C.c_int] * 2 + [C.c_float] * 2
                                     + [C.c_int, C.c_double, C.c_double] + [C.c_int] * 4 + [C.c_void_p] * 5),
    "bevf_frustum_pool_f32": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                        C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t] + [C.c_int] * 3 + [C.c_void_p]),
    "bevf_frustum_pool_bwd_f32": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p,
                                            C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p,
                                            C.c_size_t] + [C.c_int] * 2 + [C.c_void_p]),
    "bevf_depth_ce_work_doubles": (C.c_size_t, []),
    "bevf_depth_targets_f64": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t] + [C.c_int] * 5
                               + [C.c_double] * 2 + [C.c_int] * 2 + [C.c_void_p] * 2),
    "bevf_depth_ce_f32": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bevf_depth_ce_bwd_f32": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_size_t, C.c_int, C.c_void_p]),
    # ---- temporal fusion: ego-motion BEV warp ----
    "bevf_bev_warp_f32": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 6 + [C.c_float] * 4 + [C.c_void_p]),
    "bevf_bev_warp_bf16": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 6 + [C.c_float] * 4 + [C.c_void_p]),
    "bevf_bev_warp_bwd_f32": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 5 + [C.c_float] * 4 + [C.c_void_p]),
    # ---- BEV map-segmentation head: grid resample, focal loss, IoU counts ----
    "bevf_bev_grid_resample_f32": (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 8 + [C.c_double] * 8 + [C.c_void_p]),
    "bevf_bev_grid_resample_bf16": (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 8 + [C.c_double] * 8 + [C.c_void_p]),
    "bevf_bev_grid_resample_bwd_f32": (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 7 + [C.c_double] * 8 + [C.c_void_p]),
    "bevf_seg_focal_work_doubles": (C.c_size_t, [C.c_int]),
    "bevf_seg_focal_loss_f32": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 3 + [C.c_float] * 2 + [C.c_void_p] * 3),
    "bevf_seg_focal_loss_bwd_f32": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_float] * 2 + [C.c_void_p]),
    "bevf_seg_iou_counts": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 2 + [C.c_int, C.c_void_p] + [C.c_int] * 3 + [C.c_void_p]),
    # ---- segmentation targets rasterised from map polygons and polylines ----
    "bevf_map_raster_work_bytes": (C.c_size_t, [C.c_int] * 2),
    "bevf_map_raster_u8": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_int]
                           + [C.c_void_p] * 2 + [C.c_int] * 3 + [C.c_double] * 4 + [C.c_void_p] * 3),
    # ---- multi-sweep LiDAR accumulation ----
    "bevf_sweeps_merge_work_bytes": (C.c_size_t, [C.c_int] * 3),
    "bevf_sweeps_merge_f32": (C.c_int, [C.c_void_p] * 8 + [C.c_int] * 5 + [C.c_float, C.POINTER(C.c_float), C.c_void_p]),
    "bevf_sweep_pose_chain_f64": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 2 + [C.c_void_p]),
    # ---- multi-object tracking ----
    "bevf_track_step_f32": (C.c_int, [C.c_void_p] * 21 + [C.c_int] * 5 + [C.c_float, C.c_int, C.c_void_p]),
    # ---- BEV backbone / FPN neck: transposed convolution with kernel = stride (DeconvDesc goes in as an opaque pointer) ----
    "bevf_deconv_pack_elems": (C.c_size_t, [C.c_int] * 4),
    "bevf_deconv_pack_f32": (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 3 + [C.c_void_p]),
    "bevf_deconv_pack_bf16": (C.c_int, [C.c_void_p] * 2 + [C.c_int] * 3 + [C.c_void_p]),
    "bevf_deconv_nhwc_f32": (C.c_int, [C.c_void_p, C.c_void_p]),
    "bevf_deconv_nhwc_bf16": (C.c_int, [C.c_void_p, C.c_void_p]),
    # ---- CenterPoint second stage: RoI BEV-point gather, targets, loss, refine ----
    "bevf_roi_bev_points_table_words": (C.c_size_t, [C.c_int] * 2),
    "bevf_roi_bev_points_f32": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 6 + [C.c_double] * 4 + [C.c_void_p]),
    "bevf_roi_bev_points_bf16": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 6 + [C.c_double] * 4 + [C.c_void_p]),
    "bevf_roi_bev_points_bwd_f32": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 5 + [C.c_void_p]),
    "bevf_roi_targets_f32": (C.c_int, [C.c_void_p] * 10 + [C.c_int] * 5 + [C.c_float, C.c_void_p]),
    "bevf_roi_loss_f32": (C.c_int, [C.c_void_p] * 6 + [C.c_int] * 2 + [C.c_float] * 2 + [C.c_void_p]),
    "bevf_roi_loss_bwd_f32": (C.c_int, [C.c_void_p] * 6 + [C.c_int] * 2 + [C.c_float] * 2 + [C.c_void_p]),
    "bevf_roi_refine_f32": (C.c_int, [C.c_void_p] * 11 + [C.c_int] * 2 + [C.c_float, C.c_void_p]),
}


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise BevfError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                            f"or `make -C {os.path.dirname(LIB_PATH)}` -- there is no CPU fallback")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)
            fn.restype, fn.argtypes = res, args
        _lib = l
    return _lib


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _call(name: str, *args) -> None:
    """Launch entry point `name` on torch's current stream; a nonzero status raises with the library's message."""
    rc = getattr(lib(), name)(*args, _stream())
    if rc != 0:
        raise BevfError(f"{name} failed ({rc}): {lib().bevf_last_error().decode()}")


def _p(t: Optional[torch.Tensor], dtype=torch.float32) -> Optional[int]:
    if t is None:
        return None
    if not t.is_cuda:
        raise BevfError("HIP path needs CUDA/HIP tensors; got a CPU tensor (no CPU fallback in this package)")
    if t.dtype != dtype:
        raise BevfError(f"expected {dtype}, got {t.dtype}")
    return t.data_ptr()


BF16 = torch.bfloat16


def _sfx(t: torch.Tensor) -> str:
    """Entry-point suffix for a storage dtype."""
    if t.dtype == torch.float32:
        return "f32"
    if t.dtype == BF16:
        return "bf16"
    raise BevfError(f"unsupported storage dtype {t.dtype} (fp32 or bf16)")


def _pc(t: Optional[torch.Tensor], dtype=torch.float32) -> Optional[int]:
    if t is not None and not t.is_contiguous():
        raise BevfError("tensor must be contiguous")
    return _p(t, dtype)


# ---- wrappers -------------------------------------------------------------------------------------

def conv2d_nhwc(x: torch.Tensor, w: torch.Tensor, scale, shift, y: Optional[torch.Tensor], *, N: int, H: int,
                W: int, Cin: int, x_cs: int, Cout: int, y_cs: int, KH: int, KW: int, stride: int, pad: int,
                relu: bool, res: Optional[torch.Tensor] = None, res_cs: int = 0,
                colmax: Optional[torch.Tensor] = None, rows_per_group: int = 0, tile: int = 0,
                run_if: Optional[torch.Tensor] = None, group_rows: Optional[torch.Tensor] = None) -> None:
    """run_if: optional int32 device word; the launch does nothing when it reads 0 (decided on the stream, no host read).
    group_rows: optional int32 [groups] with colmax: tiles whose rows all lie at or past group_rows[g] of their group are skipped."""
    Ho = (H + 2 * pad - KH) // stride + 1
    Wo = (W + 2 * pad - KW) // stride + 1
    M = N * Ho * Wo
    if x.numel() < (N * H * W - 1) * x_cs + Cin:
        raise BevfError("conv: input buffer smaller than N*H*W*x_cs")
    split = x.dtype == torch.float32 and w.dtype == torch.bfloat16      # f32x3: planes from split_weights_f32x3
    if w.numel() != Cout * KH * KW * Cin * (3 if split else 1):
        raise BevfError(f"conv: packed weight has {w.numel()} elements, expected {Cout * KH * KW * Cin * (3 if split else 1)}")
    if y is not None and y.numel() < (M - 1) * y_cs + Cout:
        raise BevfError("conv: output buffer too small")
    if res is not None and res.numel() < (M - 1) * res_cs + Cout:
        raise BevfError("conv: residual buffer too small")
    for v in (scale, shift):
        if v is not None and v.numel() != Cout:
            raise BevfError("conv: scale/shift length != Cout")
    if colmax is not None and colmax.numel() < -(-M // rows_per_group) * Cout:
        raise BevfError("conv: colmax buffer too small")
    dt = x.dtype
    d = ConvDesc(_p(x, dt), _pc(w, w.dtype), _pc(scale), _pc(shift), _p(res, dt), _p(y, dt), _pc(colmax, torch.int32),
                 N, H, W, Cin, x_cs, Ho, Wo, Cout, y_cs, res_cs, KH, KW, stride, pad, int(relu), rows_per_group, tile)
    if group_rows is not None and (colmax is None or group_rows.numel() < -(-M // rows_per_group)):
        raise BevfError("conv: group_rows needs colmax and one entry per group")
    if run_if is not None or group_rows is not None:
        if split or x.dtype != torch.float32:
            raise BevfError("conv: run_if / group_rows exist for the exact fp32 kernel only")
        _call("bevf_conv2d_nhwc_f32_if", C.byref(d), _p(run_if, torch.int32), _pc(group_rows, torch.int32))
        return
    fn = "bevf_conv2d_nhwc_f32x3" if split else "bevf_conv2d_nhwc_" + _sfx(x)
    _call(fn, C.byref(d))


def conv2d_bound(x: torch.Tensor, planes: torch.Tensor, scale, shift, bound_g: torch.Tensor, thr: torch.Tensor,
                 flag: Optional[torch.Tensor], *, M: int, Cin: int, Cout: int, rows_per_group: int, seed_stride: int = 0,
                 tile: int = 0) -> None:
    """Bound pass of the pruned column max over the pointwise layer x [M][Cin] -> Cout channels (bevf_conv2d_bound_f32x2):
    raises thr [groups][Cout] (int32 bit patterns, zeroed by the caller); seed_stride = 0 also sets flag [M], seed_stride = k > 0
    runs every k-th row tile and takes flag = None.  planes = split_weights_f32x3 of the layer's filter."""
    if x.numel() < M * Cin:
        raise BevfError("conv_bound: input buffer smaller than M*Cin")
    if planes.dtype != torch.bfloat16 or planes.numel() != 3 * Cout * Cin:
        raise BevfError(f"conv_bound: planes have {planes.numel()} elements, expected {3 * Cout * Cin} bf16")
    for v in (scale, shift, bound_g):
        if v is None or v.numel() != Cout:
            raise BevfError("conv_bound: scale / shift / bound_g length != Cout")
    if thr.numel() < -(-M // rows_per_group) * Cout:
        raise BevfError("conv_bound: threshold buffer too small")
    if (flag is None) != (seed_stride > 0):
        raise BevfError("conv_bound: a seed launch takes no flags, a main launch needs them")
    if flag is not None and flag.numel() < M:
        raise BevfError("conv_bound: flag buffer smaller than M")
    d = ConvDesc(_p(x), _pc(planes, torch.bfloat16), _pc(scale), _pc(shift), None, None, _pc(thr, torch.int32),
                 M, 1, 1, Cin, Cin, 1, 1, Cout, Cout, 0, 1, 1, 1, 0, 1, rows_per_group, tile)
    _call("bevf_conv2d_bound_f32x2", C.byref(d), _pc(bound_g), _pc(flag, torch.int32), seed_stride)


def prune_compact(x: torch.Tensor, flag: torch.Tensor, rp: torch.Tensor, cand: torch.Tensor, rows: torch.Tensor,
                  overflow: torch.Tensor, B: int, N: int, Cc: int, cap: int) -> None:
    """flag [B][N] -> cand [B][cap][Cc]: each frame's flagged rows of x [B][N][Cc], then the frame's row 0 up to the next multiple
    of 128 slots; rows [B] = min(flagged rows, cap) (conv2d_nhwc's group_rows); overflow (int32 word, zeroed by the caller) is set
    when a frame has more than cap flagged rows.  rp: work, B*(N+1) int32."""
    if x.numel() < B * N * Cc or flag.numel() < B * N:
        raise BevfError("prune_compact: x / flag smaller than B*N rows")
    if rp.numel() < B * (N + 1) or cand.numel() < B * cap * Cc or rows.numel() < B or overflow.numel() < 1:
        raise BevfError("prune_compact: rp / cand / rows / overflow buffer too small")
    _call("bevf_prune_compact_f32", _pc(x), _pc(flag, torch.int32), _pc(rp, torch.int32), _pc(cand), _pc(rows, torch.int32),
          _pc(overflow, torch.int32), B, N, Cc, cap)


def wino_filter_transform(w_ohwi: torch.Tensor, Cout: int, Cin: int) -> torch.Tensor:
    """fp32 OHWI 3x3 filter -> the transformed-filter image of bevf_conv3x3_wino_f32."""
    w_ohwi = w_ohwi.contiguous()
    if w_ohwi.numel() != Cout * 9 * Cin:
        raise BevfError(f"wino_filter_transform: filter has {w_ohwi.numel()} elements, expected {Cout * 9 * Cin}")
    u = torch.empty(lib().bevf_wino_filter_floats(Cout, Cin), dtype=torch.float32, device=w_ohwi.device)
    _call("bevf_wino_filter_transform_f32", _pc(w_ohwi), _p(u), Cout, Cin)
    return u


def wino_stat_rows(N: int, H: int, W: int) -> int:
    """Rows of conv3x3_wino's BatchNorm partial-sum buffer."""
    return int(lib().bevf_wino_stat_rows(N, H, W))


def conv3x3_wino(x: torch.Tensor, u: torch.Tensor, scale, shift, y: torch.Tensor, *, N: int, H: int, W: int, Cin: int,
                 x_cs: int, Cout: int, y_cs: int, relu: bool, res: Optional[torch.Tensor] = None, res_cs: int = 0,
                 stats: Optional[torch.Tensor] = None, stats_pivot: Optional[torch.Tensor] = None, bnb: Optional[dict] = None,
                 tile: int = 0) -> None:
    """3x3 / stride 1 / pad 1 convolution as fused fp32 Winograd F(2x2,3x3); `u` from wino_filter_transform.
    tile: 0 = the tiling that covers the batch with the fewest blocks, 1 = 16x16-pixel blocks per image, 2 = 32x8-pixel blocks per image,
    3 / 4 = the same two block shapes over the images' rows stacked into one map (bit-identical results, fewer dead rows).
    `stats` [bevf_wino_stat_rows(N,H,W)][Cout][2]: also leave the BatchNorm partial sums of the output (training)."""
    if stats is not None and stats.numel() < wino_stat_rows(N, H, W) * Cout * 2:
        raise BevfError("conv_wino: stats buffer too small")
    if stats_pivot is not None and stats_pivot.numel() < Cout:
        raise BevfError("conv_wino: stats_pivot shorter than Cout")
    M = N * H * W
    if x.numel() < (M - 1) * x_cs + Cin:
        raise BevfError("conv_wino: input buffer smaller than N*H*W*x_cs")
    if u.numel() != lib().bevf_wino_filter_floats(Cout, Cin):
        raise BevfError("conv_wino: transformed filter has the wrong size")
    if y.numel() < (M - 1) * y_cs + Cout:
        raise BevfError("conv_wino: output buffer too small")
    if res is not None and res.numel() < (M - 1) * res_cs + Cout:
        raise BevfError("conv_wino: residual buffer too small")
    for v in (scale, shift):
        if v is not None and v.numel() != Cout:
            raise BevfError("conv_wino: scale/shift length != Cout")
    d = ConvDesc(_p(x), _pc(u), _pc(scale), _pc(shift), _p(res), _p(y), None, N, H, W, Cin, x_cs, H, W, Cout, y_cs, res_cs,
                 3, 3, 1, 1, int(relu), 0, int(tile), _p(stats), _pc(stats_pivot))
    if bnb is not None:       # this conv's output is dY of a train-mode BatchNorm(+ReLU) layer: mask + backward sums in the epilogue
        for k in ("x", "mean", "invstd"):
            if bnb.get(k) is None:
                raise BevfError(f"conv_wino: bnb needs '{k}'")
        if bnb["x"].numel() < M * Cout or (bnb.get("y") is not None and bnb["y"].numel() < M * Cout):
            raise BevfError("conv_wino: bnb x / y smaller than the output")
        d.bnb_x, d.bnb_y = _p(bnb["x"]), _p(bnb.get("y"))
        d.bnb_mean, d.bnb_invstd = _p(bnb["mean"]), _p(bnb["invstd"])
        d.bnb_gamma, d.bnb_beta = _p(bnb.get("gamma")), _p(bnb.get("beta"))
    _call("bevf_conv3x3_wino_f32", C.byref(d))


def conv3x3_pack_bf16(w_ohwi: torch.Tensor, Cout: int, Cin: int) -> torch.Tensor:
    """bf16 OHWI 3x3 filter -> the MFMA-fragment-ordered filter image of bevf_conv3x3_bf16."""
    w_ohwi = w_ohwi.contiguous()
    if w_ohwi.dtype != torch.bfloat16 or w_ohwi.numel() != Cout * 9 * Cin:
        raise BevfError(f"conv3x3_pack: need a bf16 filter of {Cout * 9 * Cin} elements, got {w_ohwi.dtype} x {w_ohwi.numel()}")
    out = torch.empty(lib().bevf_conv3x3_pack_elems(Cout, Cin), dtype=torch.bfloat16, device=w_ohwi.device)
    _call("bevf_conv3x3_pack_bf16", _pc(w_ohwi, torch.bfloat16), _p(out, torch.bfloat16), Cout, Cin)
    return out


def conv3x3_bf16(x: torch.Tensor, wp: torch.Tensor, scale, shift, y: torch.Tensor, *, N: int, H: int, W: int, Cin: int,
                 x_cs: int, Cout: int, y_cs: int, relu: bool, res: Optional[torch.Tensor] = None, res_cs: int = 0,
                 tile: int = 0) -> None:
    """3x3 / stride 1 / pad 1 convolution of bf16 activations (fp32 accumulate, folded BN, residual, ReLU); `wp` from
    conv3x3_pack_bf16.  tile (64-channel tiles only): 0 auto, 1 = two patch buffers / two workgroups per CU, 2 = one / four,
    3 = one buffer and 32-row blocks."""
    M = N * H * W
    dt = torch.bfloat16
    if x.numel() < (M - 1) * x_cs + Cin:
        raise BevfError("conv3x3_bf16: input buffer smaller than N*H*W*x_cs")
    if wp.dtype != dt or wp.numel() != lib().bevf_conv3x3_pack_elems(Cout, Cin):
        raise BevfError("conv3x3_bf16: packed filter has the wrong size / dtype")
    if y.numel() < (M - 1) * y_cs + Cout:
        raise BevfError("conv3x3_bf16: output buffer too small")
    if res is not None and res.numel() < (M - 1) * res_cs + Cout:
        raise BevfError("conv3x3_bf16: residual buffer too small")
    for v in (scale, shift):
        if v is not None and v.numel() != Cout:
            raise BevfError("conv3x3_bf16: scale/shift length != Cout")
    d = ConvDesc(_p(x, dt), _pc(wp, dt), _pc(scale), _pc(shift), _p(res, dt), _p(y, dt), None, N, H, W, Cin, x_cs, H, W, Cout,
                 y_cs, res_cs, 3, 3, 1, 1, int(relu), 0, int(tile))
    _call("bevf_conv3x3_bf16", C.byref(d))


def split_weights_f32x3(w: torch.Tensor) -> torch.Tensor:
    """fp32 packed filter -> [3][n] bf16 planes (hi, mid, lo) for the f32x3 convolution."""
    w = w.contiguous()
    out = torch.empty(3 * w.numel(), dtype=torch.bfloat16, device=w.device)
    _call("bevf_split_weights_f32x3", _pc(w), _p(out, torch.bfloat16), w.numel())
    return out


def stem_pack_bf16(w_oihw: torch.Tensor) -> torch.Tensor:
    out = torch.empty(64 * 176, dtype=torch.bfloat16, device=w_oihw.device)
    _call("bevf_stem_pack_bf16", _pc(w_oihw.float().contiguous()), _p(out, torch.bfloat16))
    return out


def stem_conv7x7_bf16mma(x: torch.Tensor, w_packed: torch.Tensor, scale, shift, y: torch.Tensor, N: int, H: int, W: int,
                         relu: bool = True):
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if x.numel() != N * 3 * H * W or w_packed.numel() != 64 * 176 or y.numel() < N * Ho * Wo * 64:
        raise BevfError("stem bf16: buffer sizes do not match N,H,W")
    _call("bevf_stem_conv7x7_bf16mma", _pc(x), _pc(w_packed, torch.bfloat16), _pc(scale), _pc(shift), _p(y, torch.bfloat16),
          N, H, W, int(relu))


def stem_conv7x7(x: torch.Tensor, w_packed: torch.Tensor, scale, shift, y: torch.Tensor, N: int, H: int, W: int,
                 relu: bool = True):
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if x.numel() != N * 3 * H * W or w_packed.numel() != 148 * 64 or y.numel() < N * Ho * Wo * 64:
        raise BevfError("stem: buffer sizes do not match N,H,W")
    fn = "bevf_stem_conv7x7_f32" if y.dtype == torch.float32 else "bevf_stem_conv7x7_bf16out"
    _call(fn, _pc(x), _pc(w_packed), _pc(scale), _pc(shift), _p(y, y.dtype), N, H, W, int(relu))


def stem_pool(x: torch.Tensor, w_packed: torch.Tensor, scale, shift, y: torch.Tensor, N: int, H: int, W: int):
    """stem 7x7/s2 + BN + ReLU + 3x3/s2 max-pool in one kernel: (N,3,H,W) fp32 -> pooled NHWC [N][Hp][Wp][64]."""
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    Hp, Wp = (Ho - 1) // 2 + 1, (Wo - 1) // 2 + 1
    if x.numel() != N * 3 * H * W or w_packed.numel() != 148 * 64 or y.numel() < N * Hp * Wp * 64:
        raise BevfError("stem_pool: buffer sizes do not match N,H,W")
    _call("bevf_stem_pool_f32", _pc(x), _pc(w_packed), _pc(scale), _pc(shift), _p(y), N, H, W)


def stem_pool_bf16mma(x: torch.Tensor, w_packed: torch.Tensor, scale, shift, y: torch.Tensor, N: int, H: int, W: int):
    """bf16 stem + BN + ReLU + 3x3/s2 max-pool in one kernel: (N,3,H,W) fp32 -> pooled bf16 NHWC [N][Hp][Wp][64]."""
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    Hp, Wp = (Ho - 1) // 2 + 1, (Wo - 1) // 2 + 1
    if x.numel() != N * 3 * H * W or w_packed.numel() != 64 * 176 or y.numel() < N * Hp * Wp * 64:
        raise BevfError("stem_pool bf16: buffer sizes do not match N,H,W")
    _call("bevf_stem_pool_bf16mma", _pc(x), _pc(w_packed, torch.bfloat16), _pc(scale), _pc(shift), _p(y, torch.bfloat16),
          N, H, W)


def maxpool3x3s2(x: torch.Tensor, y: torch.Tensor, N: int, H: int, W: int, Cc: int):
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if x.numel() < N * H * W * Cc or y.numel() < N * Ho * Wo * Cc:
        raise BevfError("maxpool: buffer too small")
    fn = "bevf_maxpool3x3s2_nhwc_" + _sfx(x)
    _call(fn, _p(x, x.dtype), _p(y, x.dtype), N, H, W, Cc)


def pointwise_smallk(x, w, scale, shift, y, M: int, K: int, Cout: int, relu: bool):
    if x.numel() < M * K or w.numel() != Cout * K or y.numel() < M * Cout:
        raise BevfError("pointwise: buffer sizes do not match M,K,Cout")
    fn = "bevf_pointwise_smallk_f32" if y.dtype == torch.float32 else "bevf_pointwise_smallk_bf16out"
    _call(fn, _pc(x), _pc(w), _pc(scale), _pc(shift), _p(y, y.dtype), M, K, Cout, int(relu))


def pointnet_front_pack(w: torch.Tensor) -> torch.Tensor:
    """(Cout, Cin) fp32 pointwise filter -> MFMA fragment order for pointnet_front."""
    cout, cin = w.shape
    w = w.detach().float().contiguous()
    wf = torch.empty(cout * cin, device=w.device)
    _call("bevf_pointnet_front_pack_f32", _p(w), _p(wf), cout, cin)
    return wf


def pointnet_front(x, w1, s1, b1, w2f, s2, b2, w3f, s3, b3, y, M: int, K: int):
    if x.numel() < M * K or w1.numel() != 64 * K or w2f.numel() != 128 * 64 or w3f.numel() != 256 * 128 or y.numel() < M * 256 \
            or min(s1.numel(), b1.numel()) < 64 or min(s2.numel(), b2.numel()) < 128 or min(s3.numel(), b3.numel()) < 256:
        raise BevfError("pointnet_front: buffer sizes do not match M, K and the 64/128/256 widths")
    _call("bevf_pointnet_front_f32", _pc(x), M, K, _pc(w1), _pc(s1), _pc(b1), _pc(w2f), _pc(s2), _pc(b2), _pc(w3f), _pc(s3),
          _pc(b3), _p(y))


def vfe_smallk_max(x, w, scale, shift, y, G: int, P: int, K: int, Cout: int) -> None:
    """VFELayer for K <= 16 in one pass: pointwise linear + folded BN + ReLU + max over the P rows of each group."""
    if x.numel() < G * P * K or w.numel() != Cout * K or y.numel() < G * Cout:
        raise BevfError("vfe_smallk_max: buffer sizes do not match G, P, K, Cout")
    _call("bevf_vfe_smallk_max_f32", _pc(x), _pc(w), _pc(scale), _pc(shift), _p(y), G, P, K, Cout)


def group_max(x, y, G: int, P: int, Cc: int):
    if x.numel() < G * P * Cc or y.numel() < G * Cc:
        raise BevfError("group_max: buffer too small")
    _call("bevf_group_max_f32", _p(x), _p(y), G, P, Cc)


def radar_mlp_max(x, ws: Sequence[torch.Tensor], scales, shifts, out, R: int, B: int, P: int, Cin: int,
                  widths: Sequence[int]):
    if x.numel() != R * B * P * Cin or out.numel() < B * R * widths[3]:
        raise BevfError("radar: buffer sizes do not match R,B,P,Cin")
    cin = Cin
    for i in range(4):
        if ws[i].numel() != cin * widths[i] or scales[i].numel() != widths[i] or shifts[i].numel() != widths[i]:
            raise BevfError(f"radar: layer {i} parameter sizes wrong")
        cin = widths[i]
    d = RadarDesc()
    d.x, d.out, d.R, d.B, d.P, d.Cin = _pc(x), _p(out), R, B, P, Cin
    for i in range(4):
        d.w[i], d.scale[i], d.shift[i], d.c[i] = _pc(ws[i]), _pc(scales[i]), _pc(shifts[i]), widths[i]
    _call("bevf_radar_mlp_max_f32", C.byref(d))


def linear(x, w, bias, y, B: int, K: int, O: int, relu: bool, perm_inner: int = 0, perm_outer: int = 0):
    if x.numel() < B * K or w.numel() != O * K or y.numel() < B * O or (bias is not None and bias.numel() != O):
        raise BevfError("linear: buffer sizes do not match B,K,O")
    if w.dtype == torch.float32:
        _call("bevf_linear_f32", _p(x), _pc(w), _pc(bias), _p(y), B, K, O, int(relu), perm_inner, perm_outer)
    else:
        _call("bevf_linear_bf16w", _p(x), _pc(w, BF16), _pc(bias), _p(y, y.dtype), int(y.dtype == BF16), B, K, O,
              int(relu), perm_inner, perm_outer)


def cam_mean(x, y, B: int, ncam: int, P: int, Cc: int):
    if x.numel() < B * ncam * P * Cc or y.numel() < B * P * Cc:
        raise BevfError("cam_mean: buffer too small")
    fn = "bevf_cam_mean_" + _sfx(x)
    _call(fn, _p(x, x.dtype), _p(y, x.dtype), B, ncam, P, Cc)


def bilinear_nhwc(x, y, B: int, Hi: int, Wi: int, Cc: int, x_cs: int, Ho: int, Wo: int, y_cs: int):
    if x.numel() < (B * Hi * Wi - 1) * x_cs + Cc or y.numel() < (B * Ho * Wo - 1) * y_cs + Cc:
        raise BevfError("bilinear: buffer too small")
    fn = "bevf_bilinear_nhwc_" + _sfx(x)
    _call(fn, _p(x, x.dtype), _p(y, x.dtype), B, Hi, Wi, Cc, x_cs, Ho, Wo, y_cs)


def broadcast_nhwc(v, y, B: int, P: int, Cc: int, y_cs: int):
    if v.numel() < B * Cc or y.numel() < (B * P - 1) * y_cs + Cc:
        raise BevfError("broadcast: buffer too small")
    fn = "bevf_broadcast_nhwc_" + _sfx(y)
    _call(fn, _p(v), _p(y, y.dtype), B, P, Cc, y_cs)


def expand_border_classes(small, y, B: int, Sh: int, Sw: int, Cc: int, y_cs: int):
    if small.numel() < B * 25 * Cc or y.numel() < (B * Sh * Sw - 1) * y_cs + Cc:
        raise BevfError("expand: buffer too small")
    fn = "bevf_expand_border_classes_" + _sfx(small)
    _call(fn, _p(small, small.dtype), _p(y, small.dtype), B, Sh, Sw, Cc, y_cs)


def head_tail(hid, w, bias, outs: Sequence[torch.Tensor], B: int, P: int, hc: int, cs: Sequence[int], n_sigmoid: int):
    if hid.numel() < B * P * 5 * hc or w.numel() != sum(cs) * hc or bias.numel() != sum(cs):
        raise BevfError("head_tail: buffer sizes wrong")
    d = HeadDesc()
    d.hid, d.w, d.bias, d.B, d.P, d.hc, d.n_sigmoid = _p(hid, hid.dtype), _pc(w), _pc(bias), B, P, hc, n_sigmoid
    for k in range(5):
        if cs[k] == 0:                                               # empty branch: no buffer, a null pointer
            d.out[k], d.c[k] = None, 0
            continue
        if outs[k] is None or outs[k].numel() != B * cs[k] * P:
            raise BevfError("head_tail: output size wrong")
        d.out[k], d.c[k] = _pc(outs[k]), cs[k]
    fn = "bevf_head_tail_" + _sfx(hid)
    _call(fn, C.byref(d))


def nchw_to_nhwc(x, y, N: int, Cc: int, P: int, y_cs: int):
    if x.numel() < N * Cc * P or y.numel() < (N * P - 1) * y_cs + Cc:
        raise BevfError("nchw_to_nhwc: buffer too small")
    _call("bevf_nchw_to_nhwc_f32", _pc(x), _p(y), N, Cc, P, y_cs)


def nhwc_to_nchw(x, y, N: int, Cc: int, P: int, x_cs: int):
    if x.numel() < (N * P - 1) * x_cs + Cc or y.numel() < N * Cc * P:
        raise BevfError("nhwc_to_nchw: buffer too small")
    _call("bevf_nhwc_to_nchw_f32", _p(x), _pc(y), N, Cc, P, x_cs)


def fill(y: torch.Tensor, v: float):
    _call("bevf_fill_f32", _p(y), float(v), y.numel())


def centernet_decode(pred: dict, K: int, thresh: float, voxel: float, x_min: float, y_min: float,
                     true_labels: bool = False, raw_scores: bool = False, pool_ind: Optional[torch.Tensor] = None,
                     iou: Optional[torch.Tensor] = None, alpha: Optional[torch.Tensor] = None):
    """iou (B,1,H,W) and alpha [C] fp32 on the device: the score-rectifying entry point (bevf_centernet_decode_rectify_f32)."""
    heat = pred["heatmap"]
    B, Cn, H, W = heat.shape
    dev = heat.device
    if (iou is None) != (alpha is None):
        raise BevfError("decode: iou and alpha belong together")
    if iou is not None:
        if raw_scores:
            raise BevfError("decode: raw_scores cannot be combined with score rectification")
        if tuple(iou.shape) != (B, 1, H, W) or alpha.numel() != Cn:
            raise BevfError(f"decode: iou has shape {tuple(iou.shape)} and alpha {alpha.numel()} entries, expected {(B, 1, H, W)} and {Cn}")
    for k, c in (("offset", 2), ("size", 3), ("rot", 2), ("vel", 2)):
        if tuple(pred[k].shape) != (B, c, H, W):
            raise BevfError(f"decode: {k} has shape {tuple(pred[k].shape)}, expected {(B, c, H, W)}")
    boxes = torch.empty(B, K, 7, device=dev)
    scores = torch.empty(B, K, device=dev)
    labels = torch.empty(B, K, dtype=torch.int64, device=dev)
    vels = torch.empty(B, K, 2, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    work = torch.empty(lib().bevf_centernet_decode_work_bytes(B, Cn, H, W, K), dtype=torch.uint8, device=dev)
    d = DecodeDesc(_pc(heat), _pc(pred["offset"]), _pc(pred["size"]), _pc(pred["rot"]), _pc(pred["vel"]),
                   _p(boxes), _p(scores), _p(labels, torch.int64), _p(vels), _p(count, torch.int32),
                   _p(work, torch.uint8), _p(pool_ind, torch.int64), B, Cn, H, W, K, int(true_labels),
                   int(raw_scores), thresh, voxel, x_min, y_min)
    if iou is None:
        _call("bevf_centernet_decode_f32", C.byref(d))
    else:
        _call("bevf_centernet_decode_rectify_f32", C.byref(d), _pc(iou), _pc(alpha))
    return boxes, scores, labels, vels, count


def nms_keep(heat: torch.Tensor, out: torch.Tensor, planes: int, H: int, W: int):
    if heat.numel() != planes * H * W or out.numel() != planes * H * W:
        raise BevfError("nms_keep: buffer sizes do not match planes,H,W")
    _call("bevf_nms_keep_f32", _pc(heat), _pc(out), planes, H, W)


IOU_MODES = {"bev": 0, "3d": 1}
NMS_MODES = {"rotate": 0, "circle": 1}


def _box_sets(what: str, *sets) -> None:
    for t in sets:
        if t.dim() != 3 or t.shape[2] != 7 or t.shape[0] != sets[0].shape[0] or t.shape[0] == 0 or t.shape[1] == 0:
            raise BevfError(f"{what}: boxes must be non-empty (B,N,7) sets with one B, got {tuple(t.shape)}")


def boxes_iou(a: torch.Tensor, b: torch.Tensor, mode: str, count_a: Optional[torch.Tensor] = None,
              count_b: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Pairwise IoU (bevf_boxes_iou_f32) of a (B,N,7) with b (B,M,7) -> (B,N,M); mode 'bev' | '3d'; count_* (B,) int32 or None."""
    if mode not in IOU_MODES:
        raise BevfError(f"boxes_iou: mode must be one of {sorted(IOU_MODES)}, got {mode!r}")
    _box_sets("boxes_iou", a, b)
    B, N, M = a.shape[0], a.shape[1], b.shape[1]
    _need("boxes_iou", count_a=(count_a, B), count_b=(count_b, B))
    out = torch.empty(B, N, M, dtype=torch.float32, device=a.device)
    _call("bevf_boxes_iou_f32", _pc(a), _pc(count_a, torch.int32), _pc(b), _pc(count_b, torch.int32), _p(out), B, N, M,
          IOU_MODES[mode])
    return out


def nms_boxes_work_bytes(B: int, N: int) -> int:
    return int(lib().bevf_nms_boxes_work_bytes(B, N))


def nms_boxes(boxes: torch.Tensor, count: Optional[torch.Tensor], mode: str, thresh: float, post_max: int,
              scores: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None,
              velocities: Optional[torch.Tensor] = None, class_aware: bool = False, gather: bool = False):
    """Greedy NMS (bevf_nms_boxes_f32) over (B,N,7) boxes in descending score order; mode 'rotate' (thresh = IoU threshold) |
    'circle' (thresh = radius).  Returns (keep_idx (B,N) int32 padded with -1, keep_count (B,) int32) and, with gather=True, also
    the kept boxes / scores / labels / velocities (those given) compacted in the same order, zero padded."""
    if mode not in NMS_MODES:
        raise BevfError(f"nms_boxes: mode must be one of {sorted(NMS_MODES)}, got {mode!r}")
    _box_sets("nms_boxes", boxes)
    B, N = boxes.shape[0], boxes.shape[1]
    if N > 4096:
        raise BevfError(f"nms_boxes: N={N} exceeds the kernel's 4096 boxes per frame")
    if class_aware and labels is None:
        raise BevfError("nms_boxes: class_aware needs labels")
    if int(post_max) <= 0 or not float(thresh) >= 0.0:
        raise BevfError("nms_boxes: post_max must be positive and the threshold / radius >= 0")
    _need("nms_boxes", count=(count, B), scores=(scores, B * N), labels=(labels, B * N), velocities=(velocities, B * N * 2))
    dev = boxes.device
    keep_idx = torch.empty(B, N, dtype=torch.int32, device=dev)
    keep_count = torch.empty(B, dtype=torch.int32, device=dev)
    work = torch.empty(-(-nms_boxes_work_bytes(B, N) // 8), dtype=torch.int64, device=dev)
    o_boxes = torch.empty(B, N, 7, device=dev) if gather else None
    o_scores = torch.empty(B, N, device=dev) if gather and scores is not None else None
    o_labels = torch.empty(B, N, dtype=torch.int64, device=dev) if gather and labels is not None else None
    o_vels = torch.empty(B, N, 2, device=dev) if gather and velocities is not None else None
    _call("bevf_nms_boxes_f32", _pc(boxes), _pc(scores), _pc(labels, torch.int64), _pc(velocities), _pc(count, torch.int32),
          B, N, NMS_MODES[mode], float(thresh), int(class_aware), int(post_max), _p(work, torch.int64),
          _p(keep_idx, torch.int32), _p(keep_count, torch.int32), _p(o_boxes), _p(o_scores), _p(o_labels, torch.int64),
          _p(o_vels))
    if gather:
        return keep_idx, keep_count, o_boxes, o_scores, o_labels, o_vels
    return keep_idx, keep_count


def centernet_targets(boxes, labels, has_vel, out: dict, B: int, nmax: int, H: int, W: int, Cn: int,
                      max_objects: int, pc_range, overlap: float, min_radius: int):
    dev = boxes.device
    if tuple(boxes.shape) != (B, nmax, 9) or tuple(labels.shape) != (B, nmax) or has_vel.numel() != B:
        raise BevfError("targets: boxes must be (B,nmax,9), labels (B,nmax), has_vel (B,)")
    want = dict(heatmap=(B, Cn, H, W), offset=(B, 2, H, W), size=(B, 3, H, W), rot=(B, 2, H, W), vel=(B, 2, H, W),
                mask=(B, max_objects), ind=(B, max_objects), reg_mask=(B, max_objects),
                target_offset=(B, max_objects, 2), target_size=(B, max_objects, 3), target_rot=(B, max_objects, 2),
                target_vel=(B, max_objects, 2))
    for k, shp in want.items():
        if tuple(out[k].shape) != shp:
            raise BevfError(f"targets: output {k} has shape {tuple(out[k].shape)}, expected {shp}")
    owner = torch.zeros(B, H * W, dtype=torch.int32, device=dev)
    d = TargetsDesc()
    d.boxes, d.labels, d.has_vel = _pc(boxes), _pc(labels, torch.int32), _pc(has_vel, torch.int32)
    for k in ("heatmap", "offset", "size", "rot", "vel", "target_offset", "target_size", "target_rot", "target_vel"):
        setattr(d, k, _pc(out[k]))
    d.mask, d.reg_mask, d.ind = _pc(out["mask"], torch.uint8), _pc(out["reg_mask"], torch.uint8), _pc(out["ind"], torch.int64)
    d.owner_scratch = _pc(owner, torch.int32)
    d.B, d.nmax, d.H, d.W, d.C, d.max_objects, d.min_radius = B, nmax, H, W, Cn, max_objects, min_radius
    for i in range(6):
        d.pc_range[i] = float(pc_range[i])
    d.gaussian_overlap = overlap
    _call("bevf_centernet_targets_f32", C.byref(d))


def _loss_desc(pred: dict, tgt: dict, weights, keep: list) -> LossDesc:
    """Descriptor of CenterNetLoss's inputs (work / out left unset); the fp32 copies it makes are appended to `keep`."""
    heat = pred["heatmap"]
    B, Cn, H, W = heat.shape
    K = tgt["ind"].shape[1]
    if tuple(tgt["heatmap"].shape) != (B, Cn, H, W):
        raise BevfError("loss: target heatmap shape differs from the prediction")
    d = LossDesc()

    def f32(t):
        t = t.float().contiguous()
        keep.append(t)
        return _pc(t)
    d.pred_heatmap, d.tgt_heatmap = f32(heat), f32(tgt["heatmap"])
    for q, (name, c) in enumerate((("offset", 2), ("size", 3), ("rot", 2), ("vel", 2))):
        if tuple(pred[name].shape) != (B, c, H, W) or tuple(tgt["target_" + name].shape) != (B, K, c):
            raise BevfError(f"loss: {name} shapes wrong")
        d.pred_reg[q], d.tgt_reg[q] = f32(pred[name]), f32(tgt["target_" + name])
    ind = tgt["ind"].to(torch.int64).contiguous()
    rm = tgt["reg_mask"].to(torch.uint8).contiguous()
    if int(ind.numel()) != B * K or rm.numel() != B * K:
        raise BevfError("loss: ind / reg_mask must be (B,K)")
    keep += [ind, rm]
    d.ind, d.reg_mask = _pc(ind, torch.int64), _pc(rm, torch.uint8)
    d.B, d.C, d.H, d.W, d.K = B, Cn, H, W, K
    for i in range(5):
        d.weights[i] = float(weights[i])
    return d


def centernet_loss(pred: dict, tgt: dict, weights) -> torch.Tensor:
    keep = []
    d = _loss_desc(pred, tgt, weights, keep)
    dev = pred["heatmap"].device
    work = torch.empty(lib().bevf_centernet_loss_work_floats(), device=dev)
    out = torch.empty(6, device=dev)
    d.work, d.out = _pc(work), _pc(out)
    _call("bevf_centernet_loss_f32", C.byref(d))
    return out


def _iou_aware_args(what: str, pred: dict, tgt: dict, pc_range, need_iou: bool, keep: list):
    """Checked arguments shared by the three IoU-aware entry points: (pointers..., B, K, H, W, x_min, y_min, x_max, y_max); the fp32
    copies made are appended to `keep`."""
    off = pred["offset"]
    if off.dim() != 4 or off.shape[1] != 2:
        raise BevfError(f"{what}: offset must be (B,2,H,W), got {tuple(off.shape)}")
    B, _, H, W = off.shape
    K = tgt["ind"].shape[-1]
    want = [("size", pred, (B, 3, H, W)), ("rot", pred, (B, 2, H, W)), ("target_offset", tgt, (B, K, 2)), ("target_size", tgt, (B, K, 3)),
            ("target_rot", tgt, (B, K, 2)), ("ind", tgt, (B, K)), ("reg_mask", tgt, (B, K))]
    if need_iou:
        want.insert(0, ("iou", pred, (B, 1, H, W)))
    for name, src, shp in want:
        if tuple(src[name].shape) != shp:
            raise BevfError(f"{what}: {name} has shape {tuple(src[name].shape)}, expected {shp}")
    if len(pc_range) != 6:
        raise BevfError(f"{what}: pc_range must be [xmin, ymin, zmin, xmax, ymax, zmax], got {list(pc_range)}")

    def f32(t):
        t = t.detach().float().contiguous()
        keep.append(t)
        return _pc(t)
    ind = tgt["ind"].to(torch.int64).contiguous()
    rm = tgt["reg_mask"].to(torch.uint8).contiguous()
    keep += [ind, rm]
    ptrs = ([f32(pred["iou"])] if need_iou else []) + [f32(pred[n]) for n in ("offset", "size", "rot")] + \
        [f32(tgt[n]) for n in ("target_offset", "target_size", "target_rot")] + [_pc(ind, torch.int64), _pc(rm, torch.uint8)]
    geom = (B, K, H, W, float(pc_range[0]), float(pc_range[1]), float(pc_range[3]), float(pc_range[4]))
    return ptrs, geom


def iou_targets(pred: dict, tgt: dict, pc_range) -> torch.Tensor:
    """(B, K) fp32: 2 * IoU_bev(predicted box, GT box) - 1 where reg_mask is set, 0 elsewhere (bevf_iou_targets_f32)."""
    keep = []
    ptrs, geom = _iou_aware_args("iou_targets", pred, tgt, pc_range, False, keep)
    out = torch.zeros(geom[0], geom[1], device=pred["offset"].device)
    if out.numel():
        _call("bevf_iou_targets_f32", *ptrs, _p(out), *geom)
    return out


def iou_aware_loss(pred: dict, tgt: dict, pc_range, w_iou: float, w_diou: float) -> torch.Tensor:
    """(3,) device tensor: total, iou_loss, diou_loss (bevf_iou_aware_loss_f32); zeros for an empty batch."""
    keep = []
    ptrs, geom = _iou_aware_args("iou_aware_loss", pred, tgt, pc_range, True, keep)
    dev = pred["offset"].device
    out = torch.zeros(3, device=dev)
    if geom[0] * geom[1]:
        work = torch.empty(max(int(lib().bevf_iou_aware_loss_work_floats(geom[0])), 1), device=dev)
        _call("bevf_iou_aware_loss_f32", *ptrs, _p(work), _p(out), *geom, float(w_iou), float(w_diou))
    return out


def iou_aware_loss_bwd(pred: dict, tgt: dict, pc_range, w_iou: float, w_diou: float, d_iou, d_offset, d_size) -> None:
    """d total / d (iou, offset, size) into the zero-filled fp32 maps d_iou, d_offset, d_size (bevf_iou_aware_loss_bwd_f32)."""
    keep = []
    ptrs, geom = _iou_aware_args("iou_aware_loss_bwd", pred, tgt, pc_range, True, keep)
    _need("iou_aware_loss_bwd", d_iou=(d_iou, pred["iou"].numel()), d_offset=(d_offset, pred["offset"].numel()),
          d_size=(d_size, pred["size"].numel()))
    if geom[0] * geom[1]:
        _call("bevf_iou_aware_loss_bwd_f32", *ptrs, _p(d_iou), _p(d_offset), _p(d_size), *geom, float(w_iou), float(w_diou))


def centernet_decode_raw(pred: dict, K: int):
    """Top-K bookkeeping only (no keep mask): voxel 1, origin 0, zero offsets -> boxes[...,0:2] are the integer
    (x, y) cells; also returns each winner's position in the (C,K) pool."""
    heat = pred["heatmap"]
    pool_ind = torch.empty(heat.shape[0], K, dtype=torch.int64, device=heat.device)
    boxes, scores, labels, _, _ = centernet_decode(pred, K, -1.0, 1.0, 0.0, 0.0, False, True, pool_ind)
    return boxes, scores, labels, pool_ind


def scatter_voxels(features: torch.Tensor, coords: torch.Tensor, grid, num_voxels: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(B,Nv,C) features + (B,Nv,3) int64 (z,y,x) -> dense (B,C,D,H,W); last row wins on duplicates (ref encoders.py:407-410)."""
    if features.dim() != 3 or coords.shape != (features.shape[0], features.shape[1], 3):
        raise BevfError("scatter_voxels: features must be (B,Nv,C) and coords (B,Nv,3)")
    B, Nv, Cc = features.shape
    D, H, W = (int(g) for g in grid)
    out = torch.empty(B, Cc, D, H, W, device=features.device)
    owner = torch.empty(B * D * H * W, dtype=torch.int32, device=features.device)
    _call("bevf_scatter_voxels_f32", _pc(features), _pc(coords, torch.int64), _pc(num_voxels, torch.int32),
          _p(owner, torch.int32), _p(out), B, Nv, Cc, D, H, W)
    return out


def voxelize_work_bytes(B: int, N: int) -> int:
    return int(lib().bevf_voxelize_work_bytes(B, N))


def voxelize(points: torch.Tensor, pc_range, voxel_size, max_points: int, max_voxels: int, out=None):
    """out = (feats, coords, npts, nvox, work): caller-owned buffers of at least the sizes allocated below (the engines'
    grow-only workspaces).  They are NOT zero-filled here: the kernel writes only the kept voxels' rows / entries, so
    readers of `out` must stop at num_points / num_voxels (the pillar kernels do).  Without `out` the outputs are fresh
    zero-padded tensors, as before."""
    if points.dim() != 3 or points.shape[2] < 3:
        raise BevfError("voxelize: points must be (B, N, C>=3)")
    B, N, Cc = points.shape
    dev = points.device
    if out is None:
        feats = torch.zeros(B, max_voxels, max_points, Cc, device=dev)
        coords = torch.zeros(B, max_voxels, 3, dtype=torch.int64, device=dev)
        npts = torch.zeros(B, max_voxels, dtype=torch.int32, device=dev)
        nvox = torch.zeros(B, dtype=torch.int32, device=dev)
        work = torch.empty(lib().bevf_voxelize_work_bytes(B, N), dtype=torch.uint8, device=dev)
    else:
        feats, coords, npts, nvox, work = out
        if (feats.numel() < B * max_voxels * max_points * Cc or coords.numel() < B * max_voxels * 3 or npts.numel() < B * max_voxels
                or nvox.numel() < B or work.numel() < lib().bevf_voxelize_work_bytes(B, N)):
            raise BevfError("voxelize: out= buffers too small for B, N, C, max_points, max_voxels")
    d = VoxelizeDesc(_pc(points), _p(feats), _p(coords, torch.int64), _p(npts, torch.int32), _p(nvox, torch.int32),
                     _p(work, torch.uint8), B, N, Cc, max_points, max_voxels)
    for i in range(6):
        d.pc_range[i] = float(pc_range[i])
    for i in range(3):
        d.voxel_size[i] = float(voxel_size[i])
    _call("bevf_voxelize_f32", C.byref(d))
    return feats, coords, npts, nvox


def pillar_geom(feats, coords, npts, nvox, B: int, Nv: int, P: int, Cc: int, H: int, W: int, x0: float, y0: float,
                vx: float, vy: float) -> PillarGeom:
    """Descriptor of voxelize's outputs on a one-pillar-per-cell grid (flat buffers of at least these sizes)."""
    if feats.numel() < B * Nv * P * Cc or coords.numel() < B * Nv * 3 or npts.numel() < B * Nv or nvox.numel() < B:
        raise BevfError("pillars: voxel buffers smaller than B, Nv, P, C")
    return PillarGeom(_p(feats), _p(coords, torch.int64), _p(npts, torch.int32), _p(nvox, torch.int32), B, Nv, P, Cc, H, W,
                      float(x0), float(y0), float(vx), float(vy))


def pillar_work_bytes(Cout: int) -> int:
    return int(lib().bevf_pillar_work_bytes(Cout))


def pillar_pfn(g: PillarGeom, w, scale, shift, Cout: int, canvas, argmax=None) -> None:
    """Decorate + Linear + scale/shift + ReLU + max over each pillar's rows -> NHWC canvas [B][H][W][Cout] (fp32 or bf16)."""
    K = g.C + 5
    if w.numel() != Cout * K or scale.numel() < Cout or shift.numel() < Cout or canvas.numel() < g.B * g.H * g.W * Cout:
        raise BevfError("pillar_pfn: buffer sizes do not match C, Cout and the canvas")
    if argmax is not None and argmax.numel() < g.B * g.Nv * Cout:
        raise BevfError("pillar_pfn: argmax buffer smaller than B * Nv * Cout")
    bf = canvas.dtype == BF16
    _call("bevf_pillar_pfn_f32", C.byref(g), _pc(w), _pc(scale), _pc(shift), Cout, _p(canvas, canvas.dtype if bf else torch.float32),
          int(bf), _p(argmax, torch.uint8))


def pillar_moments(g: PillarGeom, w, bias, gamma, beta, Cout: int, eps: float, momentum: float, running_mean, running_var, nbt,
                   moments, mean, invstd, scale, shift, work) -> None:
    K = g.C + 5
    if (w.numel() != Cout * K or moments.numel() < 272 or min(mean.numel(), invstd.numel(), scale.numel(), shift.numel()) < Cout
            or work.numel() < pillar_work_bytes(Cout)):
        raise BevfError("pillar_moments: buffer sizes do not match C and Cout")
    _call("bevf_pillar_moments_f32", C.byref(g), _pc(w), _pc(bias), _pc(gamma), _pc(beta), Cout, float(eps), float(momentum),
          _p(running_mean), _p(running_var), _p(nbt, torch.int64), _p(moments, torch.float64),
          _p(mean), _p(invstd), _p(scale), _p(shift), _p(work, torch.uint8))


def pillar_backward(g: PillarGeom, dcanvas, argmax, w, bias, scale, shift, mean, invstd, gamma, moments, Cout: int, frozen: bool,
                    dw, db, dgamma, dbeta, work) -> None:
    K = g.C + 5
    if (dcanvas.numel() < g.B * g.H * g.W * Cout or argmax.numel() < g.B * g.Nv * Cout or w.numel() != Cout * K
            or dw.numel() < Cout * K or min(db.numel(), dgamma.numel(), dbeta.numel()) < Cout or work.numel() < pillar_work_bytes(Cout)):
        raise BevfError("pillar_backward: buffer sizes do not match C, Cout and the canvas")
    _call("bevf_pillar_pfn_backward_f32", C.byref(g), _pc(dcanvas), _pc(argmax, torch.uint8), _pc(w), _pc(bias), _pc(scale),
          _pc(shift), _pc(mean), _pc(invstd), _pc(gamma), _pc(moments, torch.float64), Cout,
          int(frozen), _p(dw), _p(db), _p(dgamma), _p(dbeta), _p(work, torch.uint8))


# ---- sparse-voxel LiDAR encoder (csrc/sparse_index.hip, sparse_conv.hip, sparse_rows.hip) ---------------------------------
# A level is `cap` row slots per frame, active while slot < count[b]; count stays on the device.

I32 = torch.int32


def _sp_need(what: str, **bufs) -> None:
    for name, (t, n) in bufs.items():
        if t is not None and t.numel() < n:
            raise BevfError(f"{what}: {name} holds {t.numel()} elements, needs {n}")


def sparse_fill_index(coords, count, B: int, cap: int, D: int, H: int, W: int, index, cell) -> None:
    if B * D * H * W >= 1 << 31:
        raise BevfError(f"sparse encoder: B * cells = {B * D * H * W} does not fit int32 (an index volume per level; no hash table)")
    _sp_need("sparse_fill_index", coords=(coords, B * cap * 3), count=(count, B), index=(index, B * D * H * W), cell=(cell, B * cap))
    _call("bevf_sparse_fill_index", _pc(coords, torch.int64), _pc(count, I32), B, cap, D, H, W, _pc(index, I32), _pc(cell, I32))


def sparse_down_work_bytes(B: int, D: int, H: int, W: int) -> int:
    return int(lib().bevf_sparse_down_work_bytes(B, D, H, W))


def sparse_down(index_in, B: int, D: int, H: int, W: int, cap_out: int, index_out, cell_out, count_out, work) -> None:
    co = (D // 2) * (H // 2) * (W // 2)
    _sp_need("sparse_down", index_in=(index_in, B * D * H * W), index_out=(index_out, B * co), cell_out=(cell_out, B * cap_out),
             count_out=(count_out, B), work=(work, sparse_down_work_bytes(B, D, H, W)))
    _call("bevf_sparse_down", _pc(index_in, I32), B, D, H, W, cap_out, _pc(index_out, I32), _pc(cell_out, I32), _pc(count_out, I32),
          _pc(work, torch.uint8))


def sparse_table(index, cell, count, B: int, cap: int, in_dims, row_dims, stride: int, transposed: bool, table) -> None:
    (Di, Hi, Wi), (Dr, Hr, Wr) = in_dims, row_dims
    _sp_need("sparse_table", index=(index, B * Di * Hi * Wi), cell=(cell, B * cap), count=(count, B), table=(table, B * cap * 27))
    _call("bevf_sparse_table", _pc(index, I32), _pc(cell, I32), _pc(count, I32), B, cap, Di, Hi, Wi, Dr, Hr, Wr, stride, int(transposed),
          _pc(table, I32))


def sparse_vfe_mean(feats, npts, nvox, B: int, Nv: int, P: int, Cc: int, Cpad: int, rows) -> None:
    _sp_need("sparse_vfe_mean", feats=(feats, B * Nv * P * Cc), npts=(npts, B * Nv), nvox=(nvox, B), rows=(rows, B * Nv * Cpad))
    _call("bevf_sparse_vfe_mean_f32", _pc(feats), _pc(npts, I32), _pc(nvox, I32), B, Nv, P, Cc, Cpad, _pc(rows))


def sparse_conv_row_tile() -> int:
    return int(lib().bevf_sparse_conv_row_tile())


def sparse_conv(x, table, count, w, scale, shift, B: int, cap: int, rows_in: int, Cin: int, Cout: int, relu: bool, y) -> None:
    """y [B * cap][Cout] = gather-GEMM of x [rows_in][Cin] through table [B * cap][27] with w [27][Cin][Cout] (+ scale / shift / ReLU)."""
    _sp_need("sparse_conv", x=(x, rows_in * Cin), table=(table, B * cap * 27), count=(count, B), w=(w, 27 * Cin * Cout),
             scale=(scale, Cout), shift=(shift, Cout), y=(y, B * cap * Cout))
    _call("bevf_sparse_conv_f32", _pc(x), _pc(table, I32), _pc(count, I32), _pc(w), _pc(scale), _pc(shift), B, cap, rows_in, Cin, Cout,
          int(relu), _pc(y))


def sparse_wgrad_work_floats(Cin: int, Cout: int) -> int:
    return int(lib().bevf_sparse_wgrad_work_floats(Cin, Cout))


def sparse_conv_wgrad(x, dy, table, count, B: int, cap: int, rows_in: int, Cin: int, Cout: int, cin_real: int, dw, work) -> None:
    _sp_need("sparse_conv_wgrad", x=(x, rows_in * Cin), dy=(dy, B * cap * Cout), table=(table, B * cap * 27), count=(count, B),
             dw=(dw, Cout * cin_real * 27), work=(work, sparse_wgrad_work_floats(Cin, Cout)))
    _call("bevf_sparse_conv_wgrad_f32", _pc(x), _pc(dy), _pc(table, I32), _pc(count, I32), B, cap, rows_in, Cin, Cout, cin_real, _pc(dw),
          _pc(work))


def sparse_canvas(rows, cell, count, B: int, cap: int, D: int, H: int, W: int, Cc: int, canvas) -> None:
    """canvas [B][H][W][D * C] (fp32 or bf16) from the level's rows; inactive cells exactly 0."""
    _sp_need("sparse_canvas", rows=(rows, B * cap * Cc), cell=(cell, B * cap), count=(count, B), canvas=(canvas, B * D * H * W * Cc))
    bf = canvas.dtype == BF16
    _call("bevf_sparse_canvas_f32", _pc(rows), _pc(cell, I32), _pc(count, I32), B, cap, D, H, W, Cc,
          _pc(canvas, canvas.dtype if bf else torch.float32), int(bf))


def sparse_canvas_bwd(dcanvas, cell, count, B: int, cap: int, D: int, H: int, W: int, Cc: int, drows) -> None:
    _sp_need("sparse_canvas_bwd", dcanvas=(dcanvas, B * D * H * W * Cc), cell=(cell, B * cap), count=(count, B), drows=(drows, B * cap * Cc))
    _call("bevf_sparse_canvas_bwd_f32", _pc(dcanvas), _pc(cell, I32), _pc(count, I32), B, cap, D, H, W, Cc, _pc(drows))


def sparse_bn_work_bytes(Cc: int) -> int:
    return int(lib().bevf_sparse_bn_work_bytes(Cc))


def sparse_bn_stats(y, count, B: int, cap: int, Cc: int, eps: float, momentum: float, running_mean, running_var, nbt, mean, invstd,
                    nrows, work) -> None:
    _sp_need("sparse_bn_stats", y=(y, B * cap * Cc), count=(count, B), running_mean=(running_mean, Cc), running_var=(running_var, Cc),
             nbt=(nbt, 1), mean=(mean, Cc), invstd=(invstd, Cc), nrows=(nrows, 1), work=(work, sparse_bn_work_bytes(Cc)))
    _call("bevf_sparse_bn_stats_f32", _pc(y), _pc(count, I32), B, cap, Cc, float(eps), float(momentum), _pc(running_mean),
          _pc(running_var), _pc(nbt, torch.int64), _pc(mean), _pc(invstd), _pc(nrows, I32), _pc(work, torch.uint8))


def sparse_bn_apply(y, count, B: int, cap: int, Cc: int, mean, invstd, gamma, beta, a) -> None:
    _sp_need("sparse_bn_apply", y=(y, B * cap * Cc), count=(count, B), mean=(mean, Cc), invstd=(invstd, Cc), gamma=(gamma, Cc),
             beta=(beta, Cc), a=(a, B * cap * Cc))
    _call("bevf_sparse_bn_apply_f32", _pc(y), _pc(count, I32), B, cap, Cc, _pc(mean), _pc(invstd), _pc(gamma), _pc(beta), _pc(a))


def sparse_bn_backward(y, da, count, B: int, cap: int, Cc: int, mean, invstd, gamma, beta, frozen: bool, dy, dgamma, dbeta, sums,
                       work) -> None:
    _sp_need("sparse_bn_backward", y=(y, B * cap * Cc), da=(da, B * cap * Cc), count=(count, B), mean=(mean, Cc), invstd=(invstd, Cc),
             gamma=(gamma, Cc), beta=(beta, Cc), dy=(dy, B * cap * Cc), dgamma=(dgamma, Cc), dbeta=(dbeta, Cc), sums=(sums, 2 * Cc),
             work=(work, sparse_bn_work_bytes(Cc)))
    _call("bevf_sparse_bn_backward_f32", _pc(y), _pc(da), _pc(count, I32), B, cap, Cc, _pc(mean), _pc(invstd), _pc(gamma), _pc(beta),
          int(frozen), _pc(dy), _pc(dgamma), _pc(dbeta), _pc(sums), _pc(work, torch.uint8))


# ---- training step --------------------------------------------------------------------------------------------------------

def _need(what: str, **bufs) -> None:
    """Each keyword = (tensor or None, the number of elements the kernel reads or writes through it)."""
    for name, (t, n) in bufs.items():
        if t is not None and t.numel() < n:
            raise BevfError(f"{what}: {name} holds {t.numel()} elements, needs {n}")


def _strided(M: int, C: int, cs: int) -> int:
    """Elements covered by M rows of C channels at channel stride cs."""
    return (M - 1) * cs + C


def conv_pixtab_bytes(N: int, H: int, W: int, KH: int, KW: int, stride: int, pad: int) -> int:
    return int(lib().bevf_conv_pixtab_bytes(N, H, W, KH, KW, stride, pad))


def conv_pixtab(tab, N: int, H: int, W: int, KH: int, KW: int, stride: int, pad: int, x_cs: int) -> None:
    """Tap table of conv2d_wgrad for this shape and x_cs, into int32 `tab`."""
    _need("conv_pixtab", tab=(tab, -(-conv_pixtab_bytes(N, H, W, KH, KW, stride, pad) // 4)))
    _call("bevf_conv_pixtab", _pc(tab, torch.int32), N, H, W, KH, KW, stride, pad, x_cs)


def wino_wgrad_workspace_floats(N: int, H: int, W: int, Cin: int, Cout: int) -> int:
    """0 = shape not supported by conv3x3_wgrad_wino."""
    return int(lib().bevf_wino_wgrad_workspace_floats(N, H, W, Cin, Cout))


def wino_wgrad_table_bytes(N: int, H: int, W: int) -> int:
    return int(lib().bevf_wino_wgrad_table_bytes(N, H, W))


def wino_wgrad_table(tab, N: int, H: int, W: int, x_cs: int, dy_cs: int) -> None:
    _need("wino_wgrad_table", tab=(tab, -(-wino_wgrad_table_bytes(N, H, W) // 4)))
    _call("bevf_wino_wgrad_table", _pc(tab, torch.int32), N, H, W, x_cs, dy_cs)


def conv2d_wgrad(x, dy, dw, pixtab, *, N: int, H: int, W: int, Cin: int, x_cs: int, Cout: int, dy_cs: int, KH: int, KW: int,
                 stride: int, pad: int) -> None:
    """dw [Cout][KH][KW][Cin] += the weight gradient (fp32 atomics; dw zero-filled by the caller); pixtab from conv_pixtab."""
    Ho, Wo = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
    _need("conv2d_wgrad", x=(x, _strided(N * H * W, Cin, x_cs)), dy=(dy, _strided(N * Ho * Wo, Cout, dy_cs)), dw=(dw, Cout * KH * KW * Cin),
          pixtab=(pixtab, -(-conv_pixtab_bytes(N, H, W, KH, KW, stride, pad) // 4)))
    d = WgradDesc(_pc(x), _pc(dy), _pc(dw), _pc(pixtab, torch.int32), N, H, W, Cin, x_cs, Cout, dy_cs, KH, KW, stride, pad)
    _call("bevf_conv2d_wgrad_f32", C.byref(d))


def conv3x3_wgrad_wino(x, dy, dw, table, work, *, N: int, H: int, W: int, Cin: int, x_cs: int, Cout: int, dy_cs: int,
                       accumulate: bool) -> None:
    """3x3 / stride 1 / pad 1 weight gradient in the Winograd domain (deterministic); table from wino_wgrad_table, work of
    wino_wgrad_workspace_floats floats.  accumulate: dw += instead of dw =."""
    M = N * H * W
    _need("conv3x3_wgrad_wino", x=(x, _strided(M, Cin, x_cs)), dy=(dy, _strided(M, Cout, dy_cs)), dw=(dw, Cout * 9 * Cin),
          table=(table, -(-wino_wgrad_table_bytes(N, H, W) // 4)), work=(work, wino_wgrad_workspace_floats(N, H, W, Cin, Cout)))
    d = WgradDesc(_pc(x), _pc(dy), _pc(dw), _pc(table, torch.int32), N, H, W, Cin, x_cs, Cout, dy_cs, 3, 3, 1, 1)
    _call("bevf_conv3x3_wgrad_wino_f32", C.byref(d), _pc(work), int(accumulate))


def zero_stuff_nhwc(dy, out, N: int, Ho: int, Wo: int, Cc: int, H: int, W: int, s: int) -> None:
    """out [N][H][W][C] = dy [N][Ho][Wo][C] spread to every s-th row and column, zeros in between."""
    _need("zero_stuff_nhwc", dy=(dy, N * Ho * Wo * Cc), out=(out, N * H * W * Cc))
    _call("bevf_zero_stuff_nhwc_f32", _pc(dy), _pc(out), N, Ho, Wo, Cc, H, W, s)


def interleave2x2_nhwc(cls: Sequence[Optional[torch.Tensor]], hq: Sequence[int], wq: Sequence[int], dx, N: int, H: int, W: int,
                       Cc: int) -> None:
    """dx [N][H][W][C] from the four input-parity classes cls[q] [N][hq[q]][wq[q]][C] (None = zeros)."""
    for q in range(4):
        _need("interleave2x2_nhwc", **{f"cls[{q}]": (cls[q], N * hq[q] * wq[q] * Cc)})
    _need("interleave2x2_nhwc", dx=(dx, N * H * W * Cc))
    ptrs = (C.c_void_p * 4)(*[_pc(c) for c in cls])
    _call("bevf_interleave2x2_nhwc_f32", ptrs, (C.c_int32 * 4)(*hq), (C.c_int32 * 4)(*wq), _pc(dx), N, H, W, Cc)


def stem_wgrad(x, dy, dw, N: int, H: int, W: int) -> None:
    """dw [64][160] += the 7x7 / stride-2 stem's weight gradient; x planar [N][3][H][W], dy [N][Ho][Wo][64]."""
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    _need("stem_wgrad", x=(x, N * 3 * H * W), dy=(dy, N * Ho * Wo * 64), dw=(dw, 64 * 160))
    _call("bevf_stem_wgrad_f32", _pc(x), _pc(dy), _pc(dw), N, H, W)


def smallk_wgrad(dy, x, dw, M: int, K: int, Cout: int) -> None:
    _need("smallk_wgrad", dy=(dy, M * Cout), x=(x, M * K), dw=(dw, Cout * K))
    _call("bevf_smallk_wgrad_f32", _pc(dy), _pc(x), _pc(dw), M, K, Cout)


def bn_work_floats(Cc: int) -> int:
    return int(lib().bevf_bn_work_floats(Cc))


def bn_stats(x, work, mean, var, invstd, M: int, Cc: int, cs: int, eps: float) -> None:
    _need("bn_stats", x=(x, _strided(M, Cc, cs)), work=(work, bn_work_floats(Cc)), mean=(mean, Cc), var=(var, Cc), invstd=(invstd, Cc))
    _call("bevf_bn_stats_f32", _pc(x), _pc(work), _pc(mean), _pc(var), _pc(invstd), M, Cc, cs, float(eps))


def bn_stats_from_partials(part, G: int, pivot, mean, var, invstd, M: int, Cc: int, eps: float) -> None:
    _need("bn_stats_from_partials", part=(part, G * Cc * 2), pivot=(pivot, Cc), mean=(mean, Cc), var=(var, Cc), invstd=(invstd, Cc))
    _call("bevf_bn_stats_from_partials_f32", _pc(part), G, _pc(pivot), _pc(mean), _pc(var), _pc(invstd), M, Cc, float(eps))


def bn_apply(x, mean, invstd, gamma, beta, res, y, M: int, Cc: int, cs: int, relu: bool) -> None:
    n = _strided(M, Cc, cs)
    _need("bn_apply", x=(x, n), mean=(mean, Cc), invstd=(invstd, Cc), gamma=(gamma, Cc), beta=(beta, Cc), res=(res, n), y=(y, n))
    _call("bevf_bn_apply_f32", _pc(x), _pc(mean), _pc(invstd), _pc(gamma), _pc(beta), _pc(res), _pc(y), M, Cc, cs, int(relu))


def bn_update_running(mean, var, running_mean, running_var, num_batches_tracked, Cc: int, M: int, momentum: float) -> None:
    """torch's train-mode running-buffer update.  The buffers are written through raw pointers: the caller bumps their versions."""
    _need("bn_update_running", mean=(mean, Cc), var=(var, Cc), running_mean=(running_mean, Cc), running_var=(running_var, Cc),
          num_batches_tracked=(num_batches_tracked, 1))
    _call("bevf_bn_update_running_f32", _pc(mean), _pc(var), _pc(running_mean), _pc(running_var),
          _pc(num_batches_tracked, torch.int64), Cc, M, float(momentum))


def bn_backward(dy, y, x, mean, invstd, gamma, beta, work, dgamma, dbeta, dx, M: int, Cc: int, cs: int, *, relu: bool = False,
                has_res: bool = False, frozen: bool = False) -> None:
    """BatchNorm(+ReLU) backward.  relu and has_res: dy is masked with the forward output y in place; relu alone: the mask is
    recomputed from x (y unused, dy untouched).  frozen: the statistics were the running buffers.  dx None: only the sums
    (no relu, x / mean / invstd may be None: column sums of dy into dbeta)."""
    mode = ((1 if has_res else 2) if relu else 0) | (4 if frozen else 0)
    y = y if mode & 3 == 1 else None
    n = _strided(M, Cc, cs)
    _need("bn_backward", dy=(dy, n), y=(y, n), x=(x, n), mean=(mean, Cc), invstd=(invstd, Cc), gamma=(gamma, Cc), beta=(beta, Cc),
          work=(work, bn_work_floats(Cc)), dgamma=(dgamma, Cc), dbeta=(dbeta, Cc), dx=(dx, n))
    _call("bevf_bn_backward_f32", _pc(dy), _pc(y), _pc(x), _pc(mean), _pc(invstd), _pc(gamma), _pc(beta), _pc(work), _pc(dgamma),
          _pc(dbeta), _pc(dx), M, Cc, cs, mode)


def bn_backward_from_partials(dy, x, mean, invstd, gamma, part, G: int, dgamma, dbeta, dx, M: int, Cc: int, cs: int) -> None:
    n = _strided(M, Cc, cs)
    _need("bn_backward_from_partials", dy=(dy, n), x=(x, n), mean=(mean, Cc), invstd=(invstd, Cc), gamma=(gamma, Cc),
          part=(part, G * Cc * 2), dgamma=(dgamma, Cc), dbeta=(dbeta, Cc), dx=(dx, n))
    _call("bevf_bn_backward_from_partials_f32", _pc(dy), _pc(x), _pc(mean), _pc(invstd), _pc(gamma), _pc(part), G, _pc(dgamma),
          _pc(dbeta), _pc(dx), M, Cc, cs)


def pool_bn_backward(dpool, idx, x, mean, invstd, gamma, beta, work, dgamma, dbeta, dx, N: int, H: int, W: int, Cc: int) -> None:
    """BatchNorm + ReLU backward whose dY is the 3x3 / stride-2 max-pool's backward of dpool (idx from maxpool3x3s2_idx)."""
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    n, npool = N * H * W * Cc, N * Ho * Wo * Cc
    _need("pool_bn_backward", dpool=(dpool, npool), idx=(idx, npool), x=(x, n), mean=(mean, Cc), invstd=(invstd, Cc), gamma=(gamma, Cc),
          beta=(beta, Cc), work=(work, bn_work_floats(Cc)), dgamma=(dgamma, Cc), dbeta=(dbeta, Cc), dx=(dx, n))
    _call("bevf_pool_bn_backward_f32", _pc(dpool), _pc(idx, torch.uint8), _pc(x), _pc(mean), _pc(invstd), _pc(gamma), _pc(beta),
          _pc(work), _pc(dgamma), _pc(dbeta), _pc(dx), N, H, W, Cc)


def bn_relu_maxpool3x3s2_idx(x, mean, invstd, gamma, beta, y, idx, N: int, H: int, W: int, Cc: int) -> None:
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    npool = N * Ho * Wo * Cc
    _need("bn_relu_maxpool3x3s2_idx", x=(x, N * H * W * Cc), mean=(mean, Cc), invstd=(invstd, Cc), gamma=(gamma, Cc), beta=(beta, Cc),
          y=(y, npool), idx=(idx, npool))
    _call("bevf_bn_relu_maxpool3x3s2_idx_f32", _pc(x), _pc(mean), _pc(invstd), _pc(gamma), _pc(beta), _pc(y), _pc(idx, torch.uint8),
          N, H, W, Cc)


def group_max_idx_work_bytes(G: int, P: int, Cc: int) -> int:
    return int(lib().bevf_group_max_idx_work_bytes(G, P, Cc))


def bn_relu_group_max_idx(x, mean, invstd, gamma, beta, y, idx, work, G: int, P: int, Cc: int) -> None:
    _need("bn_relu_group_max_idx", x=(x, G * P * Cc), mean=(mean, Cc), invstd=(invstd, Cc), gamma=(gamma, Cc), beta=(beta, Cc),
          y=(y, G * Cc), idx=(idx, G * Cc), work=(work, group_max_idx_work_bytes(G, P, Cc)))
    _call("bevf_bn_relu_group_max_idx_f32", _pc(x), _pc(mean), _pc(invstd), _pc(gamma), _pc(beta), _pc(y), _pc(idx, torch.int32),
          _pc(work, torch.uint8), G, P, Cc)


def gmax_bn_backward(dg, gmax, idx, x, mean, invstd, gamma, dgm, dgamma, dbeta, dx, B: int, P: int, Cc: int, cs: int) -> None:
    n = _strided(B * P, Cc, cs)
    _need("gmax_bn_backward", dg=(dg, B * Cc), gmax=(gmax, B * Cc), idx=(idx, B * Cc), x=(x, n), mean=(mean, Cc), invstd=(invstd, Cc),
          gamma=(gamma, Cc), dgm=(dgm, B * Cc), dgamma=(dgamma, Cc), dbeta=(dbeta, Cc), dx=(dx, n))
    _call("bevf_gmax_bn_backward_f32", _pc(dg), _pc(gmax), _pc(idx, torch.int32), _pc(x), _pc(mean), _pc(invstd), _pc(gamma), _pc(dgm),
          _pc(dgamma), _pc(dbeta), _pc(dx), B, P, Cc, cs)


def gmax_bn_sums(dg, gmax, idx, x, mean, invstd, dgm, dgamma, dbeta, B: int, P: int, Cc: int, cs: int) -> None:
    _need("gmax_bn_sums", dg=(dg, B * Cc), gmax=(gmax, B * Cc), idx=(idx, B * Cc), x=(x, _strided(B * P, Cc, cs)), mean=(mean, Cc),
          invstd=(invstd, Cc), dgm=(dgm, B * Cc), dgamma=(dgamma, Cc), dbeta=(dbeta, Cc))
    _call("bevf_gmax_bn_sums_f32", _pc(dg), _pc(gmax), _pc(idx, torch.int32), _pc(x), _pc(mean), _pc(invstd), _pc(dgm), _pc(dgamma),
          _pc(dbeta), B, P, Cc, cs)


def maxpool3x3s2_idx(x, y, idx, N: int, H: int, W: int, Cc: int) -> None:
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    _need("maxpool3x3s2_idx", x=(x, N * H * W * Cc), y=(y, N * Ho * Wo * Cc), idx=(idx, N * Ho * Wo * Cc))
    _call("bevf_maxpool3x3s2_idx_f32", _pc(x), _pc(y), _pc(idx, torch.uint8), N, H, W, Cc)


def maxpool3x3s2_bwd(dy, idx, dx, N: int, H: int, W: int, Cc: int) -> None:
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    _need("maxpool3x3s2_bwd", dy=(dy, N * Ho * Wo * Cc), idx=(idx, N * Ho * Wo * Cc), dx=(dx, N * H * W * Cc))
    _call("bevf_maxpool3x3s2_bwd_f32", _pc(dy), _pc(idx, torch.uint8), _pc(dx), N, H, W, Cc)


def group_max_idx(x, y, idx, work, G: int, P: int, Cc: int) -> None:
    """y / idx [G][C] = max and first argmax row over the P rows of each group of x [G][P][C]."""
    _need("group_max_idx", x=(x, G * P * Cc), y=(y, G * Cc), idx=(idx, G * Cc), work=(work, group_max_idx_work_bytes(G, P, Cc)))
    _call("bevf_group_max_idx_f32", _pc(x), _pc(y), _pc(idx, torch.int32), _pc(work, torch.uint8), G, P, Cc)


def group_max_bwd(dy, idx, dx, G: int, P: int, Cc: int) -> None:
    """dx [G][P][C] (zero-filled by the caller) gets dy [G][C] at the argmax rows."""
    _need("group_max_bwd", dy=(dy, G * Cc), idx=(idx, G * Cc), dx=(dx, G * P * Cc))
    _call("bevf_group_max_bwd_f32", _pc(dy), _pc(idx, torch.int32), _pc(dx), G, P, Cc)


def sparse_rows_wgrad(S, idx, A, out, G: int, P: int, Cc: int, K: int) -> None:
    _need("sparse_rows_wgrad", S=(S, G * Cc), idx=(idx, G * Cc), A=(A, G * P * K), out=(out, Cc * K))
    _call("bevf_sparse_rows_wgrad_f32", _pc(S), _pc(idx, torch.int32), _pc(A), _pc(out), G, P, Cc, K)


def sparse_rows_scatter_add(S, idx, Wt, dA, G: int, P: int, Cc: int, K: int) -> None:
    _need("sparse_rows_scatter_add", S=(S, G * Cc), idx=(idx, G * Cc), W=(Wt, Cc * K), dA=(dA, G * P * K))
    _call("bevf_sparse_rows_scatter_add_f32", _pc(S), _pc(idx, torch.int32), _pc(Wt), _pc(dA), G, P, Cc, K)


def bilinear_bwd_nhwc(dy, dx, B: int, Hi: int, Wi: int, Cc: int, x_cs: int, Ho: int, Wo: int, y_cs: int) -> None:
    """Backward of bilinear_nhwc; dx zero-filled by the caller."""
    _need("bilinear_bwd_nhwc", dy=(dy, _strided(B * Ho * Wo, Cc, y_cs)), dx=(dx, _strided(B * Hi * Wi, Cc, x_cs)))
    _call("bevf_bilinear_bwd_nhwc_f32", _pc(dy), _pc(dx), B, Hi, Wi, Cc, x_cs, Ho, Wo, y_cs)


def cam_mean_bwd(dy, dx, B: int, ncam: int, P: int, Cc: int) -> None:
    _need("cam_mean_bwd", dy=(dy, B * P * Cc), dx=(dx, B * ncam * P * Cc))
    _call("bevf_cam_mean_bwd_f32", _pc(dy), _pc(dx), B, ncam, P, Cc)


def _n4(n: int) -> int:
    return (n + 3) // 4 * 4


def relu_mask(dy, y, n: int) -> None:
    """dy *= (y > 0) over the first n elements; the kernel works in fours, so both buffers must hold n rounded up to 4."""
    n4 = _n4(n)
    _need("relu_mask", dy=(dy, n4), y=(y, n4))
    _call("bevf_relu_mask_f32", _pc(dy), _pc(y), n4)


def add_inplace(y, x, n: int) -> None:
    """y += x over the first n elements; both buffers must hold n rounded up to 4."""
    n4 = _n4(n)
    _need("add_inplace", y=(y, n4), x=(x, n4))
    _call("bevf_add_inplace_f32", _pc(y), _pc(x), n4)


def linear_bwd_work_floats(B: int, K: int, O: int) -> int:
    return int(lib().bevf_linear_bwd_work_floats(B, K, O))


def linear_bwd(dy, x, w, dx, dw, db, work, B: int, K: int, O: int, perm_inner: int = 0, perm_outer: int = 0) -> None:
    """Backward of linear (dy in the forward's stored order); dx None: weight and bias gradients only."""
    _need("linear_bwd", dy=(dy, B * O), x=(x, B * K), w=(w, O * K), dx=(dx, B * K), dw=(dw, O * K), db=(db, O),
          work=(work, linear_bwd_work_floats(B, K, O)))
    _call("bevf_linear_bwd_f32", _pc(dy), _pc(x), _pc(w), _pc(dx), _pc(dw), _pc(db), _pc(work), B, K, O, perm_inner, perm_outer)


def head_tail_bwd(hid, w, out0, douts: Sequence[torch.Tensor], dhid, dw, db, B: int, P: int, hc: int, cs: Sequence[int],
                  n_sigmoid: int) -> None:
    """Backward of head_tail: douts[k] (B, cs[k], H, W) -> dhid [B*P][5*hc], dw / db (zero-filled by the caller)."""
    ctot = sum(cs)
    _need("head_tail_bwd", hid=(hid, B * P * 5 * hc), w=(w, ctot * hc), out0=(out0, B * cs[0] * P), dhid=(dhid, B * P * 5 * hc),
          dw=(dw, ctot * hc), db=(db, ctot))
    for k in range(5):
        _need("head_tail_bwd", **{f"douts[{k}]": (douts[k], B * cs[k] * P)})
    d = HeadBwdDesc()
    d.hid, d.w, d.out0 = _pc(hid), _pc(w), _pc(out0)
    for k in range(5):
        d.dout[k], d.c[k] = _pc(douts[k]), cs[k]
    d.dhid, d.dw, d.db, d.B, d.P, d.hc, d.n_sigmoid = _pc(dhid), _pc(dw), _pc(db), B, P, hc, n_sigmoid
    _call("bevf_head_tail_bwd_f32", C.byref(d))


def centernet_loss_bwd(pred: dict, tgt: dict, weights, dpred: Sequence[torch.Tensor], scratch) -> None:
    """d total_loss / d predictions into dpred (heatmap, offset, size, rot, vel; zero-filled by the caller); scratch: 2 floats."""
    names = ("heatmap", "offset", "size", "rot", "vel")
    for k, name in enumerate(names):
        _need("centernet_loss_bwd", **{f"dpred[{k}]": (dpred[k], pred[name].numel())})
    _need("centernet_loss_bwd", scratch=(scratch, 2))
    keep = []
    d = _loss_desc(pred, tgt, weights, keep)
    arr = (C.c_void_p * 5)(*[_pc(t) for t in dpred])
    _call("bevf_centernet_loss_bwd_f32", C.byref(d), arr, _pc(scratch))


def grad_norm(g, work, max_norm: float, out) -> None:
    """out = {L2 norm of g, min(1, max_norm / (norm + 1e-6))}; work: 512 doubles."""
    _need("grad_norm", work=(work, 512), out=(out, 2))
    _call("bevf_grad_norm_f32", _pc(g), g.numel(), _pc(work, torch.float64), float(max_norm), _pc(out))


def adamw_step(p, g, m, v, clip, lr: float, beta1: float, beta2: float, eps: float, weight_decay: float, step: int) -> None:
    """One AdamW step over the g.numel() leading elements of p / m / v; clip (optional): grad_norm's out, scales g by clip[1]."""
    n = g.numel()
    _need("adamw_step", p=(p, n), m=(m, n), v=(v, n), clip=(clip, 2))
    _call("bevf_adamw_step_f32", _pc(p), _pc(g), _pc(m), _pc(v), _pc(clip), n, float(lr), float(beta1), float(beta2), float(eps),
          float(weight_decay), int(step))


# ---- input pipeline -------------------------------------------------------------------------------------------------------

def resize_normalize_u8(x, out, n: int, H: int, W: int, Ho: int, Wo: int, bounds_h, coef_h, ksize_h: int, bounds_v, coef_v,
                        ksize_v: int, mean: Sequence[float], std: Sequence[float]) -> None:
    """uint8 [n][H][W][3] -> fp32 planar [n][3][Ho][Wo] (Pillow-identical resize, then (x/255 - mean) / std); bounds / coef:
    int32 per-axis tables of preprocess.resample_tables."""
    _need("resize_normalize_u8", x=(x, n * H * W * 3), out=(out, n * 3 * Ho * Wo), bounds_h=(bounds_h, Wo * 2),
          coef_h=(coef_h, Wo * ksize_h), bounds_v=(bounds_v, Ho * 2), coef_v=(coef_v, Ho * ksize_v))
    _call("bevf_resize_normalize_u8", _pc(x, torch.uint8), _pc(out), n, H, W, Ho, Wo, _pc(bounds_h, torch.int32),
          _pc(coef_h, torch.int32), ksize_h, _pc(bounds_v, torch.int32), _pc(coef_v, torch.int32), ksize_v,
          (C.c_float * 3)(*mean), (C.c_float * 3)(*std))


def lidar_filter_pad(points, out, count, work, choice, N: int, Cc: int, max_points: int, pc_range: Sequence[float]) -> None:
    """One sweep [N][C] -> the in-range points, in order, zero-padded (or picked by `choice`, max_points int64) to out
    [max_points][C]; count: 1 int32; work: N*C + ceil(N / 1024) floats.  `choice` is used only when count >= max_points
    (with fewer survivors it is ignored: survivors in order, then zero rows); an entry that is negative or >= count reads no
    survivor and gives a zero row."""
    _need("lidar_filter_pad", points=(points, N * Cc), out=(out, max_points * Cc), count=(count, 1),
          work=(work, N * Cc + -(-N // 1024)), choice=(choice, max_points))
    _call("bevf_lidar_filter_pad_f32", _pc(points), _pc(out), _pc(count, torch.int32), _pc(work), _pc(choice, torch.int64), N, Cc,
          max_points, (C.c_float * 6)(*pc_range))


# ---- training augmentation (csrc/augment.hip) ---------------------------------------------------------------------

def resample_tables_box(windows, n: int, H: int, W: int, Ho: int, Wo: int, ksize_h: int, ksize_v: int, bounds_h, coef_h, bounds_v,
                        coef_v) -> None:
    """Pillow's coefficient tables for the integer windows [n][4] = (x0, x1, y0, y1), on the device (bevf_resample_tables_box_f64):
    bounds_h [n][Wo][2], coef_h [n][Wo][ksize_h], bounds_v [n][Ho][2], coef_v [n][Ho][ksize_v], all int32."""
    _need("resample_tables_box", windows=(windows, n * 4), bounds_h=(bounds_h, n * Wo * 2), coef_h=(coef_h, n * Wo * ksize_h),
          bounds_v=(bounds_v, n * Ho * 2), coef_v=(coef_v, n * Ho * ksize_v))
    i32 = torch.int32
    _call("bevf_resample_tables_box_f64", _pc(windows, i32), n, H, W, Ho, Wo, ksize_h, ksize_v, _pc(bounds_h, i32), _pc(coef_h, i32),
          _pc(bounds_v, i32), _pc(coef_v, i32))


def resize_crop_u8(x, out, gray_sum, n: int, H: int, W: int, Ho: int, Wo: int, bounds_h, coef_h, ksize_h: int, bounds_v, coef_v,
                   ksize_v: int) -> None:
    """uint8 [n][H][W][3] -> uint8 [n][Ho][Wo][3] through the per-image tables of resample_tables_box (Pillow-identical), and
    gray_sum [n] int64 = the sum of Pillow's gray value over each output image."""
    _need("resize_crop_u8", x=(x, n * H * W * 3), out=(out, n * Ho * Wo * 3), gray_sum=(gray_sum, n), bounds_h=(bounds_h, n * Wo * 2),
          coef_h=(coef_h, n * Wo * ksize_h), bounds_v=(bounds_v, n * Ho * 2), coef_v=(coef_v, n * Ho * ksize_v))
    i32 = torch.int32
    _call("bevf_resize_crop_u8", _pc(x, torch.uint8), _pc(out, torch.uint8), _pc(gray_sum, torch.int64), n, H, W, Ho, Wo,
          _pc(bounds_h, i32), _pc(coef_h, i32), ksize_h, _pc(bounds_v, i32), _pc(coef_v, i32), ksize_v)


def jitter_flip_normalize_u8(x, out, gray_sum, jitter, flip, n: int, Ho: int, Wo: int, mean: Sequence[float],
                             std: Sequence[float]) -> None:
    """uint8 [n][Ho][Wo][3] -> planar fp32 [n][3][Ho][Wo]: per-image jitter [n][4] = (contrast, brightness, saturation, hue shift),
    flip [n] int32, then (x - mean) / std (bevf_jitter_flip_normalize_u8)."""
    _need("jitter_flip_normalize_u8", x=(x, n * Ho * Wo * 3), out=(out, n * 3 * Ho * Wo), gray_sum=(gray_sum, n), jitter=(jitter, n * 4),
          flip=(flip, n))
    _call("bevf_jitter_flip_normalize_u8", _pc(x, torch.uint8), _pc(out), _pc(gray_sum, torch.int64), _pc(jitter), _pc(flip, torch.int32),
          n, Ho, Wo, (C.c_float * 3)(*mean), (C.c_float * 3)(*std))


def points_affine_work_floats(B: int, N: int, Cc: int) -> int:
    return int(lib().bevf_points_affine_work_floats(B, N, Cc))


def _vel_ch(vel_ch) -> Sequence[int]:
    return (-1, -1) if vel_ch is None else (int(vel_ch[0]), int(vel_ch[1]))


def points_affine_filter_pad(points, n_in, mat, out, count, work, B: int, N: int, Cc: int, max_points: int, vel_ch,
                             pc_range: Sequence[float]) -> None:
    """points [B][N][C] (n_in [B] int32 valid rows, or None) through mat [B][12], range filter, compaction, zero padding: out
    [B][max_points][C], count [B] int32 (bevf_points_affine_filter_pad_f32); vel_ch: None or the two velocity channels."""
    _need("points_affine_filter_pad", points=(points, B * N * Cc), n_in=(n_in, B), mat=(mat, B * 12), out=(out, B * max_points * Cc),
          count=(count, B), work=(work, points_affine_work_floats(B, N, Cc)))
    _call("bevf_points_affine_filter_pad_f32", _pc(points), _pc(n_in, torch.int32), _pc(mat), _pc(out), _pc(count, torch.int32),
          _pc(work), B, N, Cc, max_points, *_vel_ch(vel_ch), (C.c_float * 6)(*pc_range))


def points_affine(points, mat, noise, noise_std: float, B: int, N: int, Cc: int, vel_ch) -> None:
    """points [B][N][C] through mat [B][12] in place; noise [B][N][3] (or None) times noise_std onto channels 0-2."""
    _need("points_affine", points=(points, B * N * Cc), mat=(mat, B * 12), noise=(noise, B * N * 3))
    _call("bevf_points_affine_f32", _pc(points), _pc(mat), _pc(noise), float(noise_std), B, N, Cc, *_vel_ch(vel_ch))


def boxes_affine(boxes, labels, velocities, mat, scale, B: int, M: int, ncol: int) -> None:
    """boxes [B][M][ncol] / velocities [B][M][2] (or None) through mat [B][12] in place; labels [B][M] int64 < 0 mark padding rows,
    scale [B] the transform's isotropic scale (bevf_boxes_affine_f32)."""
    _need("boxes_affine", boxes=(boxes, B * M * ncol), labels=(labels, B * M), velocities=(velocities, B * M * 2), mat=(mat, B * 12),
          scale=(scale, B))
    _call("bevf_boxes_affine_f32", _pc(boxes), _pc(labels, torch.int64), _pc(velocities), _pc(mat), _pc(scale), B, M, ncol)


# ---- points in boxes, GT-paste (csrc/gt_paste.hip) ----------------------------------------------------------------

def _ncol(what: str, ncol: int) -> None:
    if ncol not in (7, 9):
        raise BevfError(f"{what}: boxes have 7 or 9 columns, got {ncol}")


def points_in_boxes(points, n_in, boxes, box_mask, idx, B: int, N: int, Cc: int, M: int, ncol: int) -> None:
    """idx [B][N] int32 = the lowest box of boxes [B][M][ncol] that contains point i of points [B][N][C], or -1; n_in [B] int32 valid
    rows (or None), box_mask [B][M] int32 (or None): rows < 0 are ignored (bevf_points_in_boxes_f32)."""
    _ncol("points_in_boxes", ncol)
    _need("points_in_boxes", points=(points, B * N * Cc), n_in=(n_in, B), boxes=(boxes, B * M * ncol), box_mask=(box_mask, B * M),
          idx=(idx, B * N))
    i32 = torch.int32
    _call("bevf_points_in_boxes_f32", _pc(points), _pc(n_in, i32), _pc(boxes), _pc(box_mask, i32), _pc(idx, i32), B, N, Cc, M, ncol)


def paste_accept(gt_boxes, gt_labels, gt_velocities, bank_boxes, bank_labels, obj_ptr, cand, accepted, prefix, out_boxes, out_labels,
                 out_velocities, B: int, M: int, ncol: int, K: int, bank_ncol: int, Kc: int) -> None:
    """The greedy accept step and the new GT rows (bevf_paste_accept_f32): cand / accepted [B][Kc] int32, prefix [B][Kc + 1] int32,
    out_* with M + Kc rows per frame; labels int64."""
    _ncol("paste_accept", ncol)
    _ncol("paste_accept", bank_ncol)
    if not 0 < Kc <= 64 or K <= 0:
        raise BevfError(f"paste_accept: needs 0 < Kc <= 64 candidates per frame and a bank that holds objects, got Kc = {Kc}, K = {K}")
    if (gt_velocities is None) != (out_velocities is None):
        raise BevfError("paste_accept: velocities go in and come out together")
    R = M + Kc
    _need("paste_accept", gt_boxes=(gt_boxes, B * M * ncol), gt_labels=(gt_labels, B * M), gt_velocities=(gt_velocities, B * M * 2),
          bank_boxes=(bank_boxes, K * bank_ncol), bank_labels=(bank_labels, K), obj_ptr=(obj_ptr, K + 1), cand=(cand, B * Kc),
          accepted=(accepted, B * Kc), prefix=(prefix, B * (Kc + 1)), out_boxes=(out_boxes, B * R * ncol), out_labels=(out_labels, B * R),
          out_velocities=(out_velocities, B * R * 2))
    i32, i64 = torch.int32, torch.int64
    _call("bevf_paste_accept_f32", _pc(gt_boxes), _pc(gt_labels, i64), _pc(gt_velocities), _pc(bank_boxes), _pc(bank_labels, i64),
          _pc(obj_ptr, i32), _pc(cand, i32), _pc(accepted, i32), _pc(prefix, i32), _pc(out_boxes), _pc(out_labels, i64),
          _pc(out_velocities), B, M, ncol, K, bank_ncol, Kc)


def paste_points_work_ints(B: int, N: int) -> int:
    return int(lib().bevf_paste_points_work_ints(B, N))


def paste_points(points, n_in, bank_points, obj_ptr, bank_boxes, cand, accepted, prefix, out, count, work, B: int, N: int, Cc: int,
                 K: int, bank_ncol: int, Kc: int, capacity: int) -> None:
    """The remove and append steps (bevf_paste_points_f32): out [B][capacity][C], count [B] int32; bank_points [P][C] with P =
    the bank's point total (the caller holds obj_ptr[K] <= P)."""
    _ncol("paste_points", bank_ncol)
    if not 0 < Kc <= 64 or K <= 0 or capacity <= 0:
        raise BevfError(f"paste_points: needs 0 < Kc <= 64, K > 0 and capacity > 0, got Kc = {Kc}, K = {K}, capacity = {capacity}")
    _need("paste_points", points=(points, B * N * Cc), n_in=(n_in, B), bank_points=(bank_points, Cc), obj_ptr=(obj_ptr, K + 1),
          bank_boxes=(bank_boxes, K * bank_ncol), cand=(cand, B * Kc), accepted=(accepted, B * Kc), prefix=(prefix, B * (Kc + 1)),
          out=(out, B * capacity * Cc), count=(count, B), work=(work, paste_points_work_ints(B, N)))
    i32 = torch.int32
    _call("bevf_paste_points_f32", _pc(points), _pc(n_in, i32), _pc(bank_points), _pc(obj_ptr, i32), _pc(bank_boxes), _pc(cand, i32),
          _pc(accepted, i32), _pc(prefix, i32), _pc(out), _pc(count, i32), _pc(work, i32), B, N, Cc, K, bank_ncol, Kc, capacity)


def csr_gather(row_ptr, col, w, nrows: int, ncols: int, x, x_bs: int, x_cs: int, y, y_bs: int, y_cs: int, B: int, C: int) -> None:
    """y[b][r][0:C] = sum_e w[e] * x[b][col[e]][0:C] over CSR row r (bevf_csr_gather): the camera -> BEV projection and, on the
    transposed table, its backward.  x / y in the same storage dtype (fp32 or bf16), batch strides x_bs / y_bs and row strides
    x_cs / y_cs in elements; ncols = the table's column count (every col < ncols, checked when the table is built)."""
    if row_ptr.numel() != nrows + 1:
        raise BevfError(f"csr_gather: row_ptr holds {row_ptr.numel()} elements, needs nrows + 1 = {nrows + 1}")
    nnz = col.numel()
    if w.numel() != nnz:
        raise BevfError(f"csr_gather: {nnz} columns but {w.numel()} weights")
    _need("csr_gather", x=(x, (B - 1) * x_bs + _strided(ncols, C, x_cs)), y=(y, (B - 1) * y_bs + _strided(nrows, C, y_cs)))
    if y.dtype != x.dtype:
        raise BevfError(f"csr_gather: x is {x.dtype}, y is {y.dtype}")
    if x.is_cuda and y.is_cuda and x.untyped_storage().data_ptr() == y.untyped_storage().data_ptr():
        raise BevfError("csr_gather: x and y share storage")
    _call("bevf_csr_gather_" + _sfx(x), _pc(row_ptr, torch.int32), _pc(col, torch.int32) if nnz else None,
          _pc(w) if nnz else None, nrows, _p(x, x.dtype), x_bs, x_cs, _p(y, y.dtype), y_bs, y_cs, B, C)


def camera_table_capacity(P: int, num_heights: int, ncam: int) -> int:
    """Entries per frame that a device-built projection table can need at worst: every (cell, height, camera) sample valid with
    four distinct taps."""
    return P * num_heights * ncam * 4


def camera_table_work_elems(B: int, cap: int, nrows: int) -> int:
    """int32 elements of the work buffer of camera_table_build (nrows = P) / camera_table_transpose (nrows = ncols)."""
    return 2 * B * cap + B * nrows


def camera_table_build(calib, B: int, ncam: int, grid: Sequence[float], bev_h: int, bev_w: int, z_range: Sequence[float],
                       num_heights: int, min_depth: float, image_size: Sequence[int], Hc: int, Wc: int, row_ptr, col, w, cap: int,
                       work) -> None:
    """The projection tables of B frames from calib [B][ncam][4][4] fp64 (camera_rig.calib_matrices) on the device
    (bevf_camera_table_build_f64): row_ptr [B][P + 1], col / w [B][cap].  grid = (x0, y0, vx, vy) of encoders.pillar_grid, z_range =
    (z0, z1), image_size = (H, W)."""
    P = bev_h * bev_w
    if cap < camera_table_capacity(P, num_heights, ncam):
        raise BevfError(f"camera_table_build: capacity {cap} below the worst case {camera_table_capacity(P, num_heights, ncam)}")
    _need("camera_table_build", calib=(calib, B * ncam * 16), row_ptr=(row_ptr, B * (P + 1)), col=(col, B * cap), w=(w, B * cap),
          work=(work, camera_table_work_elems(B, cap, P)))
    _call("bevf_camera_table_build_f64", _pc(calib, torch.float64), B, ncam, *(float(v) for v in grid), bev_h, bev_w,
          float(z_range[0]), float(z_range[1]), num_heights, float(min_depth), int(image_size[0]), int(image_size[1]), Hc, Wc,
          _pc(row_ptr, torch.int32), _pc(col, torch.int32), _pc(w), cap, _pc(work, torch.int32))


def camera_table_transpose(row_ptr, col, w, cap: int, B: int, P: int, ncols: int, t_row_ptr, t_col, t_w, work) -> None:
    """The per-frame tables of camera_table_build as CSR by pixel (bevf_camera_table_transpose): t_row_ptr [B][ncols + 1], t_col /
    t_w [B][cap], rows in ascending cell order, deterministic."""
    _need("camera_table_transpose", row_ptr=(row_ptr, B * (P + 1)), col=(col, B * cap), w=(w, B * cap),
          t_row_ptr=(t_row_ptr, B * (ncols + 1)), t_col=(t_col, B * cap), t_w=(t_w, B * cap),
          work=(work, camera_table_work_elems(B, cap, ncols)))
    _call("bevf_camera_table_transpose", _pc(row_ptr, torch.int32), _pc(col, torch.int32), _pc(w), cap, B, P, ncols,
          _pc(t_row_ptr, torch.int32), _pc(t_col, torch.int32), _pc(t_w), _pc(work, torch.int32))


def csr_gather_frames(row_ptr, col, w, cap: int, nrows: int, ncols: int, x, x_bs: int, x_cs: int, y, y_bs: int, y_cs: int, B: int,
                      C: int) -> None:
    """csr_gather with one table per frame (bevf_csr_gather_frames): frame b reads row_ptr[b] ([B][nrows + 1], offsets within the
    frame) and col / w [b * cap ...]; every col < ncols and row_ptr[b][nrows] <= cap by construction of the table."""
    if cap <= 0:
        raise BevfError("csr_gather_frames: capacity must be positive")
    _need("csr_gather_frames", row_ptr=(row_ptr, B * (nrows + 1)), col=(col, B * cap), w=(w, B * cap),
          x=(x, (B - 1) * x_bs + _strided(ncols, C, x_cs)), y=(y, (B - 1) * y_bs + _strided(nrows, C, y_cs)))
    if y.dtype != x.dtype:
        raise BevfError(f"csr_gather_frames: x is {x.dtype}, y is {y.dtype}")
    if x.is_cuda and y.is_cuda and x.untyped_storage().data_ptr() == y.untyped_storage().data_ptr():
        raise BevfError("csr_gather_frames: x and y share storage")
    _call("bevf_csr_gather_frames_" + _sfx(x), _pc(row_ptr, torch.int32), nrows + 1, _pc(col, torch.int32), _pc(w), cap, nrows,
          _p(x, x.dtype), x_bs, x_cs, _p(y, y.dtype), y_bs, y_cs, B, C)


def _depth_bins(what: str, D: int) -> None:
    if not 1 <= D <= 64:
        raise BevfError(f"{what}: {D} depth bins, the kernels hold one bin per lane (1 <= D <= 64)")


def softmax_rows(x, x_rs: int, y, y_rs: int, nrows: int, D: int) -> None:
    """y[r][0:D] (row stride y_rs) = softmax(x[r][0:D]) (row stride x_rs), fp32 (bevf_softmax_rows_f32): the depth distribution."""
    _depth_bins("softmax_rows", D)
    _need("softmax_rows", x=(x, _strided(nrows, D, x_rs)), y=(y, _strided(nrows, D, y_rs)))
    _call("bevf_softmax_rows_f32", _p(x), x_rs, _p(y), y_rs, nrows, D)


def softmax_rows_bwd(pd, dpd, p_rs: int, dx, x_rs: int, x_cols: int, nrows: int, D: int) -> None:
    """dx[r][d] = pd (dpd - sum_d pd dpd) for d < D, 0 for D <= d < x_cols (bevf_softmax_rows_bwd_f32)."""
    _depth_bins("softmax_rows_bwd", D)
    if not D <= x_cols <= 64:
        raise BevfError(f"softmax_rows_bwd: {x_cols} output columns for {D} bins (D <= x_cols <= 64)")
    _need("softmax_rows_bwd", pd=(pd, _strided(nrows, D, p_rs)), dpd=(dpd, _strided(nrows, D, p_rs)),
          dx=(dx, _strided(nrows, x_cols, x_rs)))
    _call("bevf_softmax_rows_bwd_f32", _p(pd), _p(dpd), p_rs, _p(dx), x_rs, x_cols, nrows, D)


def csr_lift(row_ptr, col2, w, nrows: int, ncols: int, D: int, x, x_bs: int, x_cs: int, pd, pd_bs: int, y, y_bs: int, y_cs: int,
             B: int, C: int) -> None:
    """y[b][r][0:C] = sum_e w[e] * pd[b][col2[e]] * x[b][col2[e] // D][0:C] over CSR row r (bevf_csr_lift_f32): the learned-depth
    camera -> BEV lift.  col2 = pixel * D + bin < ncols * D (checked when the table is built); pd [b] at pd_bs holds [ncols][D]."""
    _depth_bins("csr_lift", D)
    if row_ptr.numel() != nrows + 1:
        raise BevfError(f"csr_lift: row_ptr holds {row_ptr.numel()} elements, needs nrows + 1 = {nrows + 1}")
    nnz = col2.numel()
    if w.numel() != nnz:
        raise BevfError(f"csr_lift: {nnz} columns but {w.numel()} weights")
    if ncols * D >= 2 ** 31:
        raise BevfError("csr_lift: pixel * D + bin does not fit int32")
    _need("csr_lift", x=(x, (B - 1) * x_bs + _strided(ncols, C, x_cs)), pd=(pd, (B - 1) * pd_bs + ncols * D),
          y=(y, (B - 1) * y_bs + _strided(nrows, C, y_cs)))
    if x.is_cuda and y.is_cuda and x.untyped_storage().data_ptr() == y.untyped_storage().data_ptr():
        raise BevfError("csr_lift: x and y share storage")
    _call("bevf_csr_lift_f32", _pc(row_ptr, torch.int32), _pc(col2, torch.int32) if nnz else None, _pc(w) if nnz else None, nrows, D,
          _p(x), x_bs, x_cs, _p(pd), pd_bs, _p(y), y_bs, y_cs, B, C)


def csr_lift_bwd(t_row_ptr, t_cell, t_bin, t_w, npix: int, P: int, D: int, x, x_bs: int, x_cs: int, pd, pd_bs: int, dy, dy_bs: int,
                 dy_cs: int, dx, dx_bs: int, dx_cs: int, dpd, dpd_bs: int, B: int, C: int) -> None:
    """The lift's backward on the transposed table (bevf_csr_lift_bwd_f32): dx [b][pix][0:C] and dpd [b][pix][0:D], every element
    written once.  t_cell < P and t_bin < D by construction of the table."""
    _depth_bins("csr_lift_bwd", D)
    if t_row_ptr.numel() != npix + 1:
        raise BevfError(f"csr_lift_bwd: t_row_ptr holds {t_row_ptr.numel()} elements, needs npix + 1 = {npix + 1}")
    nnz = t_cell.numel()
    if t_bin.numel() != nnz or t_w.numel() != nnz:
        raise BevfError(f"csr_lift_bwd: {nnz} cells but {t_bin.numel()} bins and {t_w.numel()} weights")
    _need("csr_lift_bwd", x=(x, (B - 1) * x_bs + _strided(npix, C, x_cs)), pd=(pd, (B - 1) * pd_bs + npix * D),
          dy=(dy, (B - 1) * dy_bs + _strided(P, C, dy_cs)), dx=(dx, (B - 1) * dx_bs + _strided(npix, C, dx_cs)),
          dpd=(dpd, (B - 1) * dpd_bs + npix * D))
    for name, t in (("x", x), ("dy", dy)):
        if t.is_cuda and dx.is_cuda and t.untyped_storage().data_ptr() == dx.untyped_storage().data_ptr():
            raise BevfError(f"csr_lift_bwd: {name} and dx share storage")
    _call("bevf_csr_lift_bwd_f32", _pc(t_row_ptr, torch.int32), _pc(t_cell, torch.int32) if nnz else None,
          _pc(t_bin, torch.int32) if nnz else None, _pc(t_w) if nnz else None, npix, D, _p(x), x_bs, x_cs, _p(pd), pd_bs, _p(dy),
          dy_bs, dy_cs, _p(dx), dx_bs, dx_cs, _p(dpd), dpd_bs, B, C)


def frustum_table_sort_wave_rows() -> int:
    """Longest row that frustum_table_build sorts with one wave; longer rows are sorted by a whole workgroup (the sort's only
    row-length threshold)."""
    return int(lib().bevf_frustum_table_sort_wave_rows())


def frustum_table_work_elems(B: int, ncam: int, bev_h: int, bev_w: int, D: int, Hc: int, Wc: int) -> int:
    """int32 elements of frustum_table_build's work buffer."""
    return int(lib().bevf_frustum_table_work_elems(B, ncam, bev_h, bev_w, D, Hc, Wc))


def frustum_table_build(calib, B: int, ncam: int, grid: Sequence[float], bev_h: int, bev_w: int, z_range: Sequence[float], D: int,
                        depth_min: float, depth_max: float, image_size: Sequence[int], Hc: int, Wc: int, cell_of, row_ptr, col2,
                        work) -> None:
    """The frustum tables of B frames from calib [B][ncam][4][4] fp64 on the device (bevf_frustum_table_build_f64): cell_of
    [B][ncols * D], row_ptr [B][P + 1], col2 [B][ncols * D] with every row ascending.  grid = (x0, y0, vx, vy) of
    encoders.pillar_grid, z_range = (z0, z1), image_size = (H, W)."""
    _depth_bins("frustum_table_build", D)
    P, cap = bev_h * bev_w, ncam * Hc * Wc * D
    _need("frustum_table_build", calib=(calib, B * ncam * 16), cell_of=(cell_of, B * cap), row_ptr=(row_ptr, B * (P + 1)),
          col2=(col2, B * cap), work=(work, frustum_table_work_elems(B, ncam, bev_h, bev_w, D, Hc, Wc)))
    _call("bevf_frustum_table_build_f64", _pc(calib, torch.float64), B, ncam, *(float(v) for v in grid), bev_h, bev_w,
          float(z_range[0]), float(z_range[1]), D, float(depth_min), float(depth_max), int(image_size[0]), int(image_size[1]), Hc, Wc,
          _pc(cell_of, torch.int32), _pc(row_ptr, torch.int32), _pc(col2, torch.int32), _pc(work, torch.int32))


def frustum_pool(row_ptr, col2, tables: int, cap: int, nrows: int, ncols: int, D: int, x, x_bs: int, x_cs: int, pd, pd_bs: int, y,
                 y_bs: int, y_cs: int, B: int, C: int) -> None:
    """y[b][r][0:C] = sum_e pd[b][col2[e]] * x[b][col2[e] // D][0:C] over row r of frame b's table (bevf_frustum_pool_f32).  tables
    = B: row_ptr [B][nrows + 1], col2 [B][cap]; tables = 1: one table shared by all frames (stride 0)."""
    _depth_bins("frustum_pool", D)
    if tables not in (1, B) or cap <= 0:
        raise BevfError(f"frustum_pool: {tables} tables for {B} frames (1 or B), capacity {cap}")
    _need("frustum_pool", row_ptr=(row_ptr, tables * (nrows + 1)), col2=(col2, tables * cap),
          x=(x, (B - 1) * x_bs + _strided(ncols, C, x_cs)), pd=(pd, (B - 1) * pd_bs + ncols * D),
          y=(y, (B - 1) * y_bs + _strided(nrows, C, y_cs)))
    if x.untyped_storage().data_ptr() == y.untyped_storage().data_ptr():
        raise BevfError("frustum_pool: x and y share storage")
    shared = tables == 1 and B > 1
    _call("bevf_frustum_pool_f32", _pc(row_ptr, torch.int32), 0 if shared else nrows + 1, _pc(col2, torch.int32), 0 if shared else cap,
          nrows, D, _p(x), x_bs, x_cs, _p(pd), pd_bs, _p(y), y_bs, y_cs, B, C)


def frustum_pool_bwd(cell_of, tables: int, npix: int, P: int, D: int, x, x_bs: int, x_cs: int, pd, pd_bs: int, dy, dy_bs: int,
                     dy_cs: int, dx, dx_bs: int, dx_cs: int, dpd, dpd_bs: int, B: int, C: int) -> None:
    """The pool's dense backward (bevf_frustum_pool_bwd_f32): dx [b][pix][0:C] and dpd [b][pix][0:D], every element written once;
    cell_of [tables][npix * D] with tables = B, or 1 for a table shared by all frames.  cell_of < P by construction."""
    _depth_bins("frustum_pool_bwd", D)
    if tables not in (1, B):
        raise BevfError(f"frustum_pool_bwd: {tables} tables for {B} frames (1 or B)")
    _need("frustum_pool_bwd", cell_of=(cell_of, tables * npix * D), x=(x, (B - 1) * x_bs + _strided(npix, C, x_cs)),
          pd=(pd, (B - 1) * pd_bs + npix * D), dy=(dy, (B - 1) * dy_bs + _strided(P, C, dy_cs)),
          dx=(dx, (B - 1) * dx_bs + _strided(npix, C, dx_cs)), dpd=(dpd, (B - 1) * dpd_bs + npix * D))
    for name, t in (("x", x), ("dy", dy)):
        if t.untyped_storage().data_ptr() == dx.untyped_storage().data_ptr():
            raise BevfError(f"frustum_pool_bwd: {name} and dx share storage")
    _call("bevf_frustum_pool_bwd_f32", _pc(cell_of, torch.int32), 0 if tables == 1 and B > 1 else npix * D, npix, D, _p(x), x_bs, x_cs,
          _p(pd), pd_bs, _p(dy), dy_bs, dy_cs, _p(dx), dx_bs, dx_cs, _p(dpd), dpd_bs, B, C)


def depth_ce_work_doubles() -> int:
    """fp64 elements of depth_ce's partials buffer."""
    return int(lib().bevf_depth_ce_work_doubles())


def depth_targets(points, N: int, counts, calib, shared: bool, B: int, ncam: int, Hc: int, Wc: int, D: int, depth_min: float,
                  depth_max: float, image_size: Sequence[int], target) -> None:
    """target [B][ncam][Hc][Wc] int32 = the nearest depth bin a LiDAR return puts on each feature pixel, -1 where there is none
    (bevf_depth_targets_f64).  points [B][N][>= 3] fp32 with strides (rows may be wider than 3 and frames padded); counts [B] int32
    valid rows per frame or None; calib fp64 [B][ncam][4][4], or [1][ncam][4][4] with shared = True (one calibration for every
    frame); image_size = (H, W)."""
    _depth_bins("depth_targets", D)
    if N:
        if points.dim() != 3 or points.shape[0] != B or points.shape[1] != N or points.shape[2] < 3 or points.stride(2) != 1:
            raise BevfError(f"depth_targets: points must be (B, N, >= 3) with unit column stride, got {tuple(points.shape)} "
                            f"strides {tuple(points.stride())} for B = {B}, N = {N}")
        p_bs, p_rs = (points.stride(0) if B > 1 else (N - 1) * points.stride(1) + 3), points.stride(1)
        if p_rs < 3 or p_bs < (N - 1) * p_rs + 3:
            raise BevfError(f"depth_targets: overlapping point rows (strides {tuple(points.stride())})")
    else:
        p_bs = p_rs = 0
    _need("depth_targets", counts=(counts, B), calib=(calib, (1 if shared else B) * ncam * 16), target=(target, B * ncam * Hc * Wc))
    _call("bevf_depth_targets_f64", _p(points) if N else None, p_bs, p_rs, N, _pc(counts, torch.int32), _pc(calib, torch.float64),
          0 if shared else ncam * 16, B, ncam, Hc, Wc, D, float(depth_min), float(depth_max), int(image_size[0]), int(image_size[1]),
          _pc(target, torch.int32))


def depth_ce(logits, l_rs: int, target, nrows: int, D: int, partials, out) -> None:
    """out = (mean over the rows with target >= 0 of logsumexp(logits[r][0:D]) - logits[r][target[r]], their count) -- (0, 0) when
    there is none (bevf_depth_ce_f32).  logits fp32 rows at stride l_rs, target [nrows] int32, partials fp64
    [depth_ce_work_doubles()], out fp32 [2]."""
    _depth_bins("depth_ce", D)
    if nrows > 1 << 24:
        raise BevfError(f"depth_ce: {nrows} rows, at most 2^24 (the count is returned as a float)")
    _need("depth_ce", logits=(logits, _strided(nrows, D, l_rs)), target=(target, nrows), partials=(partials, depth_ce_work_doubles()),
          out=(out, 2))
    _call("bevf_depth_ce_f32", _p(logits), l_rs, _pc(target, torch.int32), nrows, D, _pc(partials, torch.float64), _pc(out))


def depth_ce_bwd(pd, p_rs: int, target, g, out, dlogit, x_rs: int, nrows: int, D: int) -> None:
    """dlogit[r][d] += g[0] / max(out[1], 1) * (pd[r][d] - [d == target[r]]) for d < D on the rows with target >= 0
    (bevf_depth_ce_bwd_f32); g: one fp32 on the device, out: depth_ce's."""
    _depth_bins("depth_ce_bwd", D)
    _need("depth_ce_bwd", pd=(pd, _strided(nrows, D, p_rs)), target=(target, nrows), g=(g, 1), out=(out, 2),
          dlogit=(dlogit, _strided(nrows, D, x_rs)))
    _call("bevf_depth_ce_bwd_f32", _p(pd), p_rs, _pc(target, torch.int32), _pc(g), _pc(out), _p(dlogit), x_rs, nrows, D)


# ---- temporal fusion: ego-motion BEV warp (csrc/bev_warp.hip) ----

def _warp_args(what: str, ego, B: int, C: int, *strides: int) -> None:
    if C % 4 or any(cs % 4 or cs < C for cs in strides):
        raise BevfError(f"{what}: C = {C} and the channel strides {strides} must be multiples of 4, strides >= C")
    _need(what, ego=(ego, B * 16))


def bev_warp(x, y, ego, B: int, H: int, W: int, Cc: int, x_cs: int, y_cs: int, grid) -> None:
    """y [B][H][W] rows of Cc channels at stride y_cs = x (stride x_cs), the previous frame's map, sampled bilinearly where each
    current cell was in the previous frame (bevf_bev_warp): ego fp64 [B][4][4] on the device maps current -> previous in metres,
    grid = (x0, y0, vx, vy) of encoders.pillar_grid.  Zeros outside the map; every row of y is written.  fp32 or bf16 storage."""
    _warp_args("bev_warp", ego, B, Cc, x_cs, y_cs)
    if x.dtype != y.dtype:
        raise BevfError(f"bev_warp: x is {x.dtype}, y is {y.dtype}")
    _need("bev_warp", x=(x, _strided(B * H * W, Cc, x_cs)), y=(y, _strided(B * H * W, Cc, y_cs)))
    if x.untyped_storage().data_ptr() == y.untyped_storage().data_ptr():
        raise BevfError("bev_warp: x and y share storage")
    _call("bevf_bev_warp_" + _sfx(x), _p(x, x.dtype), _p(y, x.dtype), _pc(ego, torch.float64), B, H, W, Cc, x_cs, y_cs,
          *(float(v) for v in grid))


def warp_singular_values(ego_host, grid):
    """The singular values [B][2] of the index-space 2 x 2 part of each current -> previous map (numpy fp64 on the host)."""
    import numpy as np
    M = np.asarray(ego_host, dtype=np.float64).reshape(-1, 4, 4)
    _, _, vx, vy = (float(v) for v in grid)
    A = M[:, :2, :2] * np.array([[1.0, vy / vx], [vx / vy, 1.0]])
    if not np.isfinite(M[:, :2, [0, 1, 3]]).all():
        return np.full((M.shape[0], 2), np.nan)
    return np.linalg.svd(A, compute_uv=False)


def bev_warp_bwd(dy, dx, ego, B: int, H: int, W: int, Cc: int, dy_cs: int, grid, ego_host=None) -> None:
    """dx [B][H][W][Cc] = the transpose of bev_warp applied to dy (stride dy_cs): a deterministic pull, every element written
    (bevf_bev_warp_bwd_f32, fp32).  ego_host: the same matrices on the host (read back from `ego` when None, which waits for the
    device); a map whose index-space singular values leave [1/4, 4], or with a non-finite entry, is refused -- the kernel's
    candidate box would be unbounded."""
    _warp_args("bev_warp_bwd", ego, B, Cc, dy_cs)
    _need("bev_warp_bwd", dy=(dy, _strided(B * H * W, Cc, dy_cs)), dx=(dx, B * H * W * Cc))
    sv = warp_singular_values(ego.detach().cpu().numpy() if ego_host is None else ego_host, grid)
    if not (sv >= 0.25).all() or not (sv <= 4.0).all():
        raise BevfError(f"bev_warp_bwd: the ego-motion map must be finite with index-space singular values within [1/4, 4], got "
                        f"{sv.tolist()}")
    _call("bevf_bev_warp_bwd_f32", _p(dy), _p(dx), _pc(ego, torch.float64), B, H, W, Cc, dy_cs, *(float(v) for v in grid))


# ---- BEV map-segmentation head: grid resample, focal loss, IoU counts (csrc/bev_seg.hip) ----

def _grids(what: str, in_grid, out_grid):
    g = tuple(float(v) for v in in_grid) + tuple(float(v) for v in out_grid)
    if len(g) != 8 or any(g[k] == 0.0 for k in (2, 3, 6, 7)):
        raise BevfError(f"{what}: grids are (x0, y0, vx, vy) with non-zero cell sizes, got {tuple(in_grid)} and {tuple(out_grid)}")
    return g


def bev_grid_resample(x, y, B: int, Hi: int, Wi: int, Ho: int, Wo: int, Cc: int, x_cs: int, y_cs: int, in_grid, out_grid) -> None:
    """y [B][Ho][Wo] rows of Cc channels at stride y_cs, on out_grid = (ox0, oy0, ovx, ovy), = x [B][Hi][Wi] (stride x_cs) on
    in_grid = (x0, y0, vx, vy) sampled bilinearly at the output cell centres (bevf_bev_grid_resample): zeros outside the input,
    every output row written.  fp32 or bf16 storage; the geometry is fp64."""
    g = _grids("bev_grid_resample", in_grid, out_grid)
    if x.dtype != y.dtype:
        raise BevfError(f"bev_grid_resample: x is {x.dtype}, y is {y.dtype}")
    if x_cs < Cc or y_cs < Cc:
        raise BevfError(f"bev_grid_resample: channel strides {x_cs}, {y_cs} below C = {Cc}")
    _need("bev_grid_resample", x=(x, _strided(B * Hi * Wi, Cc, x_cs)), y=(y, _strided(B * Ho * Wo, Cc, y_cs)))
    if x.untyped_storage().data_ptr() == y.untyped_storage().data_ptr():
        raise BevfError("bev_grid_resample: x and y share storage")
    _call("bevf_bev_grid_resample_" + _sfx(x), _p(x, x.dtype), _p(y, x.dtype), B, Hi, Wi, Ho, Wo, Cc, x_cs, y_cs, *g)


def bev_grid_resample_bwd(dy, dx, B: int, Hi: int, Wi: int, Ho: int, Wo: int, Cc: int, dy_cs: int, in_grid, out_grid) -> None:
    """dx [B][Hi][Wi][Cc] = the transpose of bev_grid_resample applied to dy [B][Ho][Wo] (stride dy_cs): a deterministic pull, every
    element written (bevf_bev_grid_resample_bwd_f32, fp32)."""
    g = _grids("bev_grid_resample_bwd", in_grid, out_grid)
    if dy_cs < Cc:
        raise BevfError(f"bev_grid_resample_bwd: channel stride {dy_cs} below C = {Cc}")
    _need("bev_grid_resample_bwd", dy=(dy, _strided(B * Ho * Wo, Cc, dy_cs)), dx=(dx, B * Hi * Wi * Cc))
    _call("bevf_bev_grid_resample_bwd_f32", _p(dy), _pc(dx), B, Hi, Wi, Ho, Wo, Cc, dy_cs, *g)


def seg_focal_work_doubles(K: int) -> int:
    """fp64 elements of seg_focal_loss's partials buffer for K classes."""
    return int(lib().bevf_seg_focal_work_doubles(K))


def _seg_shape(what: str, B: int, P: int, K: int, cs: int) -> None:
    if not (B > 0 and P > 0 and 0 < K <= 64 and cs >= K):
        raise BevfError(f"{what}: bad shape B = {B}, P = {P}, K = {K}, row stride {cs} (1 <= K <= 64 <= stride)")


def seg_focal_loss(logits, cs: int, targets, B: int, P: int, K: int, alpha: float, gamma: float, partials, out) -> None:
    """out[k] = the mean over the B * P pixels of the sigmoid focal loss of class k, out[K] = their sum (bevf_seg_focal_loss_f32).
    logits fp32 rows of K classes at stride cs, targets uint8 [B][K][P], partials fp64 [seg_focal_work_doubles(K)], out fp32 [K + 1];
    alpha < 0: no alpha weighting."""
    _seg_shape("seg_focal_loss", B, P, K, cs)
    _need("seg_focal_loss", logits=(logits, _strided(B * P, K, cs)), targets=(targets, B * K * P),
          partials=(partials, seg_focal_work_doubles(K)), out=(out, K + 1))
    _call("bevf_seg_focal_loss_f32", _p(logits), cs, _pc(targets, torch.uint8), B, P, K, float(alpha), float(gamma),
          _pc(partials, torch.float64), _pc(out))


def seg_focal_loss_bwd(logits, cs: int, targets, g, dlogit, B: int, P: int, K: int, alpha: float, gamma: float) -> None:
    """dlogit rows (stride cs, all cs columns written, zeros from K on) = g[0] * d out[K] / d logits (bevf_seg_focal_loss_bwd_f32);
    g: one fp32 on the device."""
    _seg_shape("seg_focal_loss_bwd", B, P, K, cs)
    _need("seg_focal_loss_bwd", logits=(logits, _strided(B * P, K, cs)), targets=(targets, B * K * P), g=(g, 1),
          dlogit=(dlogit, B * P * cs))
    _call("bevf_seg_focal_loss_bwd_f32", _p(logits), cs, _pc(targets, torch.uint8), _pc(g), _p(dlogit), B, P, K, float(alpha),
          float(gamma))


def seg_iou_counts(logits, cs: int, targets, thr, counts, B: int, P: int, K: int) -> None:
    """counts int64 [T][K][3] = (TP, FP, FN) of logits[r][k] >= thr[t] against targets uint8 [B][K][P] (bevf_seg_iou_counts);
    thr: T <= 32 fp32 logit thresholds on the device."""
    _seg_shape("seg_iou_counts", B, P, K, cs)
    T = thr.numel()
    if not 0 < T <= 32:
        raise BevfError(f"seg_iou_counts: {T} thresholds (1 .. 32)")
    _need("seg_iou_counts", logits=(logits, _strided(B * P, K, cs)), targets=(targets, B * K * P), counts=(counts, T * K * 3))
    _call("bevf_seg_iou_counts", _p(logits), cs, _pc(targets, torch.uint8), _pc(thr), T, _pc(counts, torch.int64), B, P, K)


# ---- segmentation targets rasterised from map polygons and polylines (csrc/map_raster.hip) ----

def map_raster_work_bytes(S: int, V: int) -> int:
    """Bytes of map_raster's workspace for S shapes with V vertices in all."""
    return int(lib().bevf_map_raster_work_bytes(S, V))


def map_raster(vertices, ring_offsets, shape_offsets, shape_class, shape_kind, shape_width, frame_offsets, mat, scale, work, out,
               B: int, K: int, Ho: int, Wo: int, grid) -> None:
    """out uint8 [B][K][Ho][Wo] = the class masks of the packed shapes (bevf_map_raster_u8; the rules: include/bevf.h) on
    grid = (x0, y0, vx, vy) of seg_head.range_grid.  vertices fp32 [V][2], ring_offsets int32 [R + 1], shape_offsets int32 [S + 1],
    shape_class / shape_kind int32 [S], shape_width fp32 [S], frame_offsets int32 [B + 1]; mat fp32 [B][12] or None (identity), scale
    fp32 [B] or None (1); work: uint8 [map_raster_work_bytes(S, V)].  Every byte of out is written."""
    I32, U8 = torch.int32, torch.uint8
    S, V, R = shape_class.numel(), vertices.numel() // 2, ring_offsets.numel() - 1
    if not (B > 0 and Ho > 0 and Wo > 0 and 1 <= K <= 64):
        raise BevfError(f"map_raster: bad shape B = {B}, K = {K}, Ho = {Ho}, Wo = {Wo} (1 <= K <= 64)")
    g = tuple(float(v) for v in grid)
    if len(g) != 4:
        raise BevfError(f"map_raster: the grid is (x0, y0, vx, vy), got {tuple(grid)}")
    _need("map_raster", vertices=(vertices, 2 * V), ring_offsets=(ring_offsets, 1), shape_offsets=(shape_offsets, S + 1),
          shape_class=(shape_class, S), shape_kind=(shape_kind, S), shape_width=(shape_width, S), frame_offsets=(frame_offsets, B + 1), mat=(mat, B * 12),
          scale=(scale, B), work=(work, map_raster_work_bytes(S, V)), out=(out, B * K * Ho * Wo))
    _call("bevf_map_raster_u8", _pc(vertices), V, _pc(ring_offsets, I32), R, _pc(shape_offsets, I32), _pc(shape_class, I32),
          _pc(shape_kind, I32), _pc(shape_width), S, _pc(frame_offsets, I32), B, _pc(mat), _pc(scale), K, Ho, Wo, *g,
          _pc(work, U8), _pc(out, U8))


# ---- multi-sweep LiDAR accumulation (csrc/sweeps.hip) ----

def sweeps_merge_work_bytes(B: int, S: int, N: int) -> int:
    """Bytes of sweeps_merge's workspace (two int32 per tile of 1024 rows)."""
    return int(lib().bevf_sweeps_merge_work_bytes(B, S, N))


def sweeps_merge(points, counts, sweep_to_key, time_lag, out, count, sweep_count, work, B: int, S: int, N: int, Cc: int, max_points: int,
                 close_radius: float, pc_range: Sequence[float]) -> None:
    """points [B][S][N][C] (counts [B][S] int32 valid rows) through sweep_to_key fp64 [B][S][4][4], close-point and range filter, merged
    in sweep order with time_lag [B][S] as channel C: out [B][max_points][C + 1], count [B] and sweep_count [B][S] int32
    (bevf_sweeps_merge_f32; the rules: include/bevf.h).  work: int32 [ceil(sweeps_merge_work_bytes(B, S, N) / 4)]."""
    if not (B > 0 and S > 0 and N >= 0 and 3 <= Cc <= 8 and max_points > 0):
        raise BevfError(f"sweeps_merge: bad shape B = {B}, S = {S}, N = {N}, C = {Cc}, max_points = {max_points} (3 <= C <= 8)")
    if len(pc_range) != 6:
        raise BevfError(f"sweeps_merge: pc_range is (x0, y0, z0, x1, y1, z1), got {tuple(pc_range)}")
    i32 = torch.int32
    _need("sweeps_merge", points=(points, B * S * N * Cc), counts=(counts, B * S), sweep_to_key=(sweep_to_key, B * S * 16),
          time_lag=(time_lag, B * S), out=(out, B * max_points * (Cc + 1)), count=(count, B), sweep_count=(sweep_count, B * S),
          work=(work, -(-sweeps_merge_work_bytes(B, S, N) // 4)))
    _call("bevf_sweeps_merge_f32", _pc(points), _pc(counts, i32), _pc(sweep_to_key, torch.float64), _pc(time_lag), _pc(out),
          _pc(count, i32), _pc(sweep_count, i32), _pc(work, i32), B, S, N, Cc, max_points, float(close_radius), (C.c_float * 6)(*pc_range))


def sweep_pose_chain(key_lidar2ego, key_ego2global, sweep_lidar2ego, sweep_ego2global, sweep_to_key, B: int, S: int) -> None:
    """sweep_to_key [B][S][4][4] = inv(L_k) . inv(E_k) . E_s . L_s from key_lidar2ego / key_ego2global [B][4][4] and sweep_lidar2ego /
    sweep_ego2global [B][S][4][4], all fp64 on the device (bevf_sweep_pose_chain_f64)."""
    if not (B > 0 and S > 0):
        raise BevfError(f"sweep_pose_chain: bad shape B = {B}, S = {S}")
    f64 = torch.float64
    _need("sweep_pose_chain", key_lidar2ego=(key_lidar2ego, B * 16), key_ego2global=(key_ego2global, B * 16),
          sweep_lidar2ego=(sweep_lidar2ego, B * S * 16), sweep_ego2global=(sweep_ego2global, B * S * 16),
          sweep_to_key=(sweep_to_key, B * S * 16))
    _call("bevf_sweep_pose_chain_f64", _pc(key_lidar2ego, f64), _pc(key_ego2global, f64), _pc(sweep_lidar2ego, f64),
          _pc(sweep_ego2global, f64), _pc(sweep_to_key, f64), B, S)


# ---- multi-object tracking (csrc/track.hip) ----

TRACK_MAX_N, TRACK_MAX_T = 4096, 1024
TRACK_STATE = (("track_box", torch.float32, (7,)), ("track_vel", torch.float32, (2,)), ("track_score", torch.float32, ()),
               ("track_label", torch.int64, ()), ("track_id", torch.int64, ()), ("track_age", torch.int32, ()),
               ("track_hits", torch.int32, ()))
TRACK_OUT = (("det_track_id", torch.int64), ("det_hits", torch.int32), ("det_slot", torch.int32))


def _track_want(name: str, t, dtype, shape) -> None:
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != tuple(shape):
        got = f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise BevfError(f"track_step: {name} must be a {dtype} {tuple(shape)} tensor, got {got}")


def track_step(boxes, velocities, scores, labels, count, ego_motion, dt, max_dist, state: dict, out: dict, max_age: int,
               birth_score: float, class_aware: bool) -> None:
    """One tracker step (bevf_track_step_f32; the rules: include/bevf.h).  Detections (B,N,7) / (B,N,2) / (B,N) / int64 (B,N) / int32
    (B,); ego_motion float64 (B,4,4) current -> previous frame; dt (B,); max_dist (C,).  state: the TRACK_STATE tensors (B,T,...) plus
    track_count int32 (B,) and next_id int64 (B,), updated in place; out: det_track_id int64 (B,N), det_hits / det_slot int32 (B,N) and
    overflow int32 (B,), written.  Everything is checked before the launch; nothing is allocated or read back."""
    if not isinstance(boxes, torch.Tensor) or boxes.dim() != 3 or boxes.shape[2] != 7 or boxes.shape[0] == 0:
        got = tuple(boxes.shape) if isinstance(boxes, torch.Tensor) else type(boxes).__name__
        raise BevfError(f"track_step: boxes must be a (B,N,7) tensor with B > 0, got {got}")
    B, N = boxes.shape[0], boxes.shape[1]
    tb = state.get("track_box")
    if not isinstance(tb, torch.Tensor) or tb.dim() != 3 or tb.shape[1] == 0:
        raise BevfError("track_step: state['track_box'] must be a (B,T,7) tensor with T > 0")
    T = tb.shape[1]
    if N > TRACK_MAX_N:
        raise BevfError(f"track_step: N={N} exceeds the kernel's {TRACK_MAX_N} detections per stream")
    if T > TRACK_MAX_T:
        raise BevfError(f"track_step: T={T} exceeds the kernel's {TRACK_MAX_T} tracks per stream")
    f32, i32, i64 = torch.float32, torch.int32, torch.int64
    _track_want("boxes", boxes, f32, (B, N, 7))
    _track_want("velocities", velocities, f32, (B, N, 2))
    _track_want("scores", scores, f32, (B, N))
    _track_want("labels", labels, i64, (B, N))
    _track_want("count", count, i32, (B,))
    _track_want("ego_motion", ego_motion, torch.float64, (B, 4, 4))
    _track_want("dt", dt, f32, (B,))
    if not isinstance(max_dist, torch.Tensor) or max_dist.dtype != f32 or max_dist.dim() != 1 or max_dist.numel() == 0:
        raise BevfError("track_step: max_dist must be a non-empty float32 (C,) tensor of per-class limits in metres")
    for name, dtype, tail in TRACK_STATE:
        _track_want(f"state[{name!r}]", state.get(name), dtype, (B, T) + tail)
    _track_want("state['track_count']", state.get("track_count"), i32, (B,))
    _track_want("state['next_id']", state.get("next_id"), i64, (B,))
    for name, dtype in TRACK_OUT:
        _track_want(f"out[{name!r}]", out.get(name), dtype, (B, N))
    _track_want("out['overflow']", out.get("overflow"), i32, (B,))
    if int(max_age) < 0:
        raise BevfError(f"track_step: max_age must be >= 0, got {max_age}")
    _call("bevf_track_step_f32", _pc(boxes), _pc(velocities), _pc(scores), _pc(labels, i64), _pc(count, i32),
          _pc(ego_motion, torch.float64), _pc(dt), _pc(max_dist), *[_pc(state[name], dtype) for name, dtype, _ in TRACK_STATE],
          _pc(state["track_count"], i32), _pc(state["next_id"], i64), *[_pc(out[name], dtype) for name, dtype in TRACK_OUT],
          _pc(out["overflow"], i32), B, N, T, max_dist.numel(), int(max_age), float(birth_score), int(bool(class_aware)))


# ---- BEV backbone / FPN neck: transposed convolution with kernel = stride ------------------------------------------------------------

def deconv_check_dims(N: int, H: int, W: int, x_cs: int, y_cs: int, s: int, elem_bytes: int = 4) -> None:
    """The size rule of bevf_deconv_nhwc_* from the dimensions alone: the kernel addresses both maps with 32-bit offsets."""
    x_elems, y_elems = N * H * W * x_cs, N * s * H * s * W * y_cs
    if x_elems >= 1 << 31 or y_elems >= 1 << 31:
        raise BevfError(f"deconv: N*H*W*x_cs = {x_elems} and N*sH*sW*y_cs = {y_elems} must stay below 2^31 (32-bit offsets)")
    if max(x_elems, y_elems) * elem_bytes >= 1 << 31:
        raise BevfError(f"deconv: input / output maps of {x_elems * elem_bytes} / {y_elems * elem_bytes} bytes must stay below 2 GiB "
                        "(32-bit byte offsets)")


def deconv_pack_elems(Cin: int, Cout: int, s: int, dtype=torch.float32) -> int:
    return int(lib().bevf_deconv_pack_elems(Cin, Cout, s, int(dtype == BF16)))


def deconv_pack(w: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """nn.ConvTranspose2d's fp32 (Cin, Cout, s, s) weight -> the packed filter of deconv_nhwc in storage type `dtype`
    (once per weight version)."""
    if w.dim() != 4 or w.shape[2] != w.shape[3] or w.dtype != torch.float32:
        raise BevfError(f"deconv_pack: need an fp32 (Cin, Cout, s, s) weight, got {w.dtype} {tuple(w.shape)}")
    if dtype not in (torch.float32, BF16):
        raise BevfError(f"deconv_pack: unsupported storage dtype {dtype} (fp32 or bf16)")
    Cin, Cout, s = int(w.shape[0]), int(w.shape[1]), int(w.shape[2])
    w = w.contiguous()
    src = _pc(w)
    out = torch.empty(deconv_pack_elems(Cin, Cout, s, dtype), dtype=dtype, device=w.device)
    _call("bevf_deconv_pack_" + _sfx(out), src, _p(out, dtype), Cin, Cout, s)
    return out


def deconv_nhwc(x: torch.Tensor, wp: torch.Tensor, scale, shift, y: torch.Tensor, *, N: int, H: int, W: int, Cin: int, x_cs: int,
                Cout: int, y_cs: int, s: int, relu: bool) -> None:
    """y [N][sH][sW][y_cs] (Cout channels per pixel written; y may start inside a wider map) = the kernel = stride = s transposed
    convolution of x [N][H][W][x_cs] with the packed filter `wp` (deconv_pack), then scale / shift (fp32 [Cout] or None) and ReLU.
    x, wp and y share one storage dtype (fp32 or bf16)."""
    dt = x.dtype
    es = 2 if dt == BF16 else 4
    deconv_check_dims(N, H, W, x_cs, y_cs, s, es)
    _need("deconv", x=(x, _strided(N * H * W, Cin, x_cs)), wp=(wp, deconv_pack_elems(Cin, Cout, s, dt)),
          y=(y, _strided(N * H * W * s * s, Cout, y_cs)), scale=(scale, Cout), shift=(shift, Cout))
    d = DeconvDesc(_p(x, dt), _pc(wp, dt), _pc(scale), _pc(shift), _p(y, dt), N, H, W, Cin, x_cs, Cout, y_cs, s, int(relu))
    _call("bevf_deconv_nhwc_" + _sfx(x), C.addressof(d))


# ---- CenterPoint second stage: RoI BEV-point gather, targets, loss, refine (csrc/roi_points.hip, csrc/roi_head.hip) ------------------

ROI_MAX_K = 4096                                 # bevf_roi_refine_f32 stages a frame's scores in LDS (the tracker's limit on N)


def _roi_want(what: str, name: str, t, dtype, shape) -> None:
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != tuple(shape):
        got = f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise BevfError(f"{what}: {name} must be a {dtype} {tuple(shape)} tensor, got {got}")


def _roi_boxes(what: str, boxes, count):
    if not isinstance(boxes, torch.Tensor) or boxes.dim() != 3 or boxes.shape[2] != 7 or boxes.shape[0] == 0 or boxes.shape[1] == 0:
        got = tuple(boxes.shape) if isinstance(boxes, torch.Tensor) else type(boxes).__name__
        raise BevfError(f"{what}: boxes must be a (B,K,7) tensor with B, K > 0, got {got}")
    B, K = int(boxes.shape[0]), int(boxes.shape[1])
    _roi_want(what, "boxes", boxes, torch.float32, (B, K, 7))
    _roi_want(what, "count", count, I32, (B,))
    return B, K


def _roi_range(what: str, bev_range):
    r = tuple(float(v) for v in bev_range)
    if len(r) != 4 or r[2] == r[0] or r[3] == r[1]:
        raise BevfError(f"{what}: bev_range is (x_min, y_min, x_max, y_max) with a non-empty extent, got {tuple(bev_range)}")
    return r


def roi_bev_points_table_words(B: int, K: int) -> int:
    return int(lib().bevf_roi_bev_points_table_words(B, K))


def roi_bev_points(x, boxes, count, feat, table, H: int, W: int, Cc: int, x_cs: int, bev_range) -> None:
    """feat [B*K][5*Cc] (x's dtype) = the NHWC map x [B][H][W] (Cc channels at stride x_cs) sampled bilinearly at the centre and the
    four face centres of every RoI (bevf_roi_bev_points_*; the rules: include/bevf.h).  boxes (B,K,7) fp32, count int32 (B,);
    bev_range = (x_min, y_min, x_max, y_max) of the map.  table: None, or int32 [B*K*5*6] for roi_bev_points_bwd."""
    B, K = _roi_boxes("roi_bev_points", boxes, count)
    r = _roi_range("roi_bev_points", bev_range)
    if x.dtype != feat.dtype:
        raise BevfError(f"roi_bev_points: x is {x.dtype}, feat is {feat.dtype}")
    if x_cs < Cc or Cc <= 0 or H <= 0 or W <= 0:
        raise BevfError(f"roi_bev_points: bad map shape (H={H} W={W} C={Cc} stride={x_cs})")
    _need("roi_bev_points", x=(x, _strided(B * H * W, Cc, x_cs)), feat=(feat, B * K * 5 * Cc),
          table=(table, roi_bev_points_table_words(B, K)))
    if x.untyped_storage().data_ptr() == feat.untyped_storage().data_ptr():
        raise BevfError("roi_bev_points: x and feat share storage")
    _call("bevf_roi_bev_points_" + _sfx(x), _p(x, x.dtype), _pc(boxes), _pc(count, I32), _pc(feat, x.dtype), _pc(table, I32), B, K,
          H, W, Cc, x_cs, *r)


def roi_bev_points_bwd(dfeat, table, count, dx, B: int, K: int, H: int, W: int, Cc: int) -> None:
    """dx [B][H][W][Cc] = the transpose of roi_bev_points applied to dfeat [B*K][5*Cc], through the forward's sample table: a
    deterministic pull, every element written (bevf_roi_bev_points_bwd_f32, fp32)."""
    _roi_want("roi_bev_points_bwd", "count", count, I32, (B,))
    if min(B, K, H, W, Cc) <= 0:
        raise BevfError(f"roi_bev_points_bwd: bad shape (B={B} K={K} H={H} W={W} C={Cc})")
    _need("roi_bev_points_bwd", dfeat=(dfeat, B * K * 5 * Cc), table=(table, roi_bev_points_table_words(B, K)), dx=(dx, B * H * W * Cc))
    _call("bevf_roi_bev_points_bwd_f32", _pc(dfeat), _pc(table, I32), _pc(count, I32), _pc(dx), B, K, H, W, Cc)


def roi_targets(boxes, count, roi_labels, gt, gt_labels, use_bev: bool, match_labels: bool, reg_fg_thresh: float) -> dict:
    """The RoI targets (bevf_roi_targets_f32; the rules: include/bevf.h) of RoIs (B,K,7) / count int32 (B,) against the padded
    ground truth gt (B,M,7) fp32 / gt_labels int32 (B,M) (-1 = padding; M may be 0).  roi_labels int64 (B,K) with match_labels.
    Returns {'iou', 'cls_target' (B,K), 'gt_index' int32 (B,K), 'reg_mask' uint8 (B,K), 'reg_target' (B,K,7), 'count'}."""
    B, K = _roi_boxes("roi_targets", boxes, count)
    if not isinstance(gt, torch.Tensor) or gt.dim() != 3 or gt.shape[0] != B or gt.shape[2] != 7:
        got = tuple(gt.shape) if isinstance(gt, torch.Tensor) else type(gt).__name__
        raise BevfError(f"roi_targets: gt must be a ({B},M,7) tensor, got {got}")
    M = int(gt.shape[1])
    _roi_want("roi_targets", "gt", gt, torch.float32, (B, M, 7))
    _roi_want("roi_targets", "gt_labels", gt_labels, I32, (B, M))
    if match_labels:
        _roi_want("roi_targets", "roi_labels", roi_labels, torch.int64, (B, K))
    dev = boxes.device
    out = dict(iou=torch.empty(B, K, device=dev), gt_index=torch.empty(B, K, dtype=I32, device=dev),
               cls_target=torch.empty(B, K, device=dev), reg_mask=torch.empty(B, K, dtype=torch.uint8, device=dev),
               reg_target=torch.empty(B, K, 7, device=dev), count=count)
    _call("bevf_roi_targets_f32", _pc(boxes), _pc(count, I32), _pc(roi_labels, torch.int64) if match_labels else None,
          _pc(gt) if M else None, _pc(gt_labels, I32) if M else None, _pc(out["iou"]), _pc(out["gt_index"], I32),
          _pc(out["cls_target"]), _pc(out["reg_mask"], torch.uint8), _pc(out["reg_target"]), B, K, M, int(bool(use_bev)),
          int(bool(match_labels)), float(reg_fg_thresh))
    return out


def _roi_loss_args(what: str, pred, tgt: dict):
    if not isinstance(pred, torch.Tensor) or pred.dim() != 3 or pred.shape[2] != 8 or pred.shape[0] == 0 or pred.shape[1] == 0:
        got = tuple(pred.shape) if isinstance(pred, torch.Tensor) else type(pred).__name__
        raise BevfError(f"{what}: pred must be a (B,K,8) tensor (the logit, then seven residuals), got {got}")
    B, K = int(pred.shape[0]), int(pred.shape[1])
    _roi_want(what, "pred", pred, torch.float32, (B, K, 8))
    missing = [k for k in ("count", "cls_target", "reg_mask", "reg_target") if k not in tgt]
    if missing:
        raise BevfError(f"{what}: targets lack {missing} (build them with roi_refine.roi_targets)")
    _roi_want(what, "targets['count']", tgt["count"], I32, (B,))
    _roi_want(what, "targets['cls_target']", tgt["cls_target"], torch.float32, (B, K))
    _roi_want(what, "targets['reg_mask']", tgt["reg_mask"], torch.uint8, (B, K))
    _roi_want(what, "targets['reg_target']", tgt["reg_target"], torch.float32, (B, K, 7))
    return B, K, (_pc(pred), _pc(tgt["count"], I32), _pc(tgt["cls_target"]), _pc(tgt["reg_mask"], torch.uint8), _pc(tgt["reg_target"]))


def roi_loss(pred, tgt: dict, w_cls: float, w_reg: float) -> torch.Tensor:
    """(3,) device tensor: total, cls_loss, reg_loss (bevf_roi_loss_f32)."""
    B, K, ptrs = _roi_loss_args("roi_loss", pred, tgt)
    out = torch.empty(3, device=pred.device)
    _call("bevf_roi_loss_f32", *ptrs, _pc(out), B, K, float(w_cls), float(w_reg))
    return out


def roi_loss_bwd(pred, tgt: dict, w_cls: float, w_reg: float, dpred) -> None:
    """dpred (B,K,8) = d total / d pred, every element written (bevf_roi_loss_bwd_f32)."""
    B, K, ptrs = _roi_loss_args("roi_loss_bwd", pred, tgt)
    _roi_want("roi_loss_bwd", "dpred", dpred, torch.float32, (B, K, 8))
    _call("bevf_roi_loss_bwd_f32", *ptrs, _pc(dpred), B, K, float(w_cls), float(w_reg))


def roi_refine(boxes, scores, labels, velocities, count, pred, score_thresh: float) -> dict:
    """The refine step (bevf_roi_refine_f32; the rules: include/bevf.h) -> the padded records {'boxes', 'velocities', 'scores',
    'labels', 'count'}, compacted and in descending final score.  velocities may be None (then the result has none)."""
    B, K = _roi_boxes("roi_refine", boxes, count)
    if K > ROI_MAX_K:
        raise BevfError(f"roi_refine: K={K} exceeds the kernel's {ROI_MAX_K} RoIs per frame")
    _roi_want("roi_refine", "scores", scores, torch.float32, (B, K))
    _roi_want("roi_refine", "labels", labels, torch.int64, (B, K))
    _roi_want("roi_refine", "pred", pred, torch.float32, (B, K, 8))
    if velocities is not None:
        _roi_want("roi_refine", "velocities", velocities, torch.float32, (B, K, 2))
    dev = boxes.device
    out = dict(boxes=torch.empty(B, K, 7, device=dev), velocities=torch.empty(B, K, 2, device=dev) if velocities is not None else None,
               scores=torch.empty(B, K, device=dev), labels=torch.empty(B, K, dtype=torch.int64, device=dev),
               count=torch.empty(B, dtype=I32, device=dev))
    _call("bevf_roi_refine_f32", _pc(boxes), _pc(scores), _pc(labels, torch.int64), _pc(velocities), _pc(count, I32), _pc(pred),
          _pc(out["boxes"]), _pc(out["scores"]), _pc(out["labels"], torch.int64), _pc(out["velocities"]), _pc(out["count"], I32), B, K,
          float(score_thresh))
    return out
