"""ctypes binding of libdyolo.so (C-ABI declared in include/dyolo.h).

The library is built in-tree by ``__graft_entry__.build()`` / ``make -C drone-yolo_amd/csrc`` into
``drone-yolo_amd/lib/libdyolo.so``.  There is no fallback: if the library is missing, or a call
returns a non-zero status, this module raises — the product path never silently degrades to a
CPU or eager-PyTorch implementation.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libdyolo.so")

DY_BF16, DY_F16, DY_F32, DY_FP8, DY_F16X2 = 0, 1, 2, 3, 4
DY_ACT_NONE, DY_ACT_SILU, DY_ACT_SILU_L2E = 0, 1, 2
DY_MAX_LEVELS = 8
DY_WLAYOUT_ROWS, DY_WLAYOUT_HALO3X3, DY_WLAYOUT_FRAG1X1 = 0, 1, 2
DY_ROUTE_ROWS = 0  # dy_conv3x3_halo_route: the call needs the layer's DY_WLAYOUT_ROWS pack

_vp, _i32, _f32, _i64 = C.c_void_p, C.c_int32, C.c_float, C.c_int64


class PackJob(C.Structure):
    """dy_pack_job: one convolution of dy_pack_conv_weights_batched (the arguments of dy_pack_conv_weights)."""
    _fields_ = [("w", C.c_void_p), ("s_co", C.c_int64), ("s_ci", C.c_int64), ("s_r", C.c_int64), ("s_q", C.c_int64),
                ("cout", C.c_int32), ("cin", C.c_int32), ("ksize", C.c_int32), ("transpose_flip", C.c_int32), ("cin_logical", C.c_int32),
                ("w_layout", C.c_int32), ("dst", C.c_void_p), ("dst_elems", C.c_int64)]


class ConvDesc(C.Structure):
    """Mirror of ``dy_conv_desc`` (include/dyolo.h)."""

    _fields_ = [
        ("x", _vp), ("w", _vp), ("bias", _vp), ("residual", _vp), ("y", _vp),
        ("batch", _i32), ("h", _i32), ("w_in", _i32), ("cin", _i32), ("ld_x", _i32),
        ("ho", _i32), ("wo", _i32), ("cout", _i32), ("ld_y", _i32), ("ld_res", _i32),
        ("ksize", _i32), ("stride", _i32), ("pad", _i32),
        ("groups", _i32), ("act", _i32), ("dtype", _i32), ("out_f32", _i32),
        ("k_pad", _i32), ("cout_pad", _i32), ("up2x", _i32),
        ("x2", _vp), ("ld_x2", _i32), ("cin_split", _i32), ("w_layout", _i32),
        ("w_scale", _vp), ("act_scale", _f32), ("bn_stats", _vp), ("y_dtype1", _i32),
        ("bnb_z", _vp), ("bnb_ld_z", _i32), ("bnb_act", _i32), ("bnb_mean", _vp), ("bnb_rstd", _vp), ("bnb_gamma", _vp), ("bnb_beta", _vp),
    ]  # fmt: skip


class BranchDesc(C.Structure):
    """Mirror of ``dy_branch_desc``."""

    _fields_ = [
        ("x", _vp), ("w3", _vp), ("b3", _vp), ("w1", _vp), ("b1", _vp), ("out", _vp),
        ("batch", _i32), ("h", _i32), ("w", _i32), ("ld_x", _i32), ("c_in", _i32), ("c_mid", _i32), ("nc", _i32), ("reg_max", _i32),
        ("kind", _i32), ("dtype", _i32), ("anchors", _i32), ("anchor0", _i32),
        ("stride", _f32),
        ("nms_workspace", _vp), ("nms_workspace_bytes", _i64), ("conf_thres", _f32), ("classes_mask", _vp), ("act_l2e", _i32),
    ]  # fmt: skip


class DecodeDesc(C.Structure):
    """Mirror of ``dy_decode_desc``."""

    _fields_ = [
        ("level", _vp * DY_MAX_LEVELS),
        ("h", _i32 * DY_MAX_LEVELS), ("w", _i32 * DY_MAX_LEVELS), ("ld", _i32 * DY_MAX_LEVELS),
        ("stride", _f32 * DY_MAX_LEVELS),
        ("n_levels", _i32), ("batch", _i32), ("nc", _i32), ("reg_max", _i32),
        ("out", _vp),
        ("nms_workspace", _vp), ("nms_workspace_bytes", _i64), ("conf_thres", _f32), ("classes_mask", _vp),
    ]  # fmt: skip


class HeadDecodeDesc(C.Structure):
    """Mirror of ``dy_head_decode_desc``."""

    _fields_ = [
        ("x_box", _vp * DY_MAX_LEVELS), ("x_cls", _vp * DY_MAX_LEVELS),
        ("w_box", _vp * DY_MAX_LEVELS), ("w_cls", _vp * DY_MAX_LEVELS),
        ("b_box", _vp * DY_MAX_LEVELS), ("b_cls", _vp * DY_MAX_LEVELS),
        ("ld_box", _i32 * DY_MAX_LEVELS), ("ld_cls", _i32 * DY_MAX_LEVELS),
        ("h", _i32 * DY_MAX_LEVELS), ("w", _i32 * DY_MAX_LEVELS),
        ("stride", _f32 * DY_MAX_LEVELS),
        ("n_levels", _i32), ("batch", _i32), ("nc", _i32), ("reg_max", _i32),
        ("c_box", _i32), ("c_cls", _i32), ("dtype", _i32),
        ("out", _vp),
        ("nms_workspace", _vp), ("nms_workspace_bytes", _i64), ("conf_thres", _f32), ("classes_mask", _vp),
    ]  # fmt: skip


class NmsDesc(C.Structure):
    """Mirror of ``dy_nms_desc``."""

    _fields_ = [
        ("pred", _vp),
        ("batch", _i32), ("nc", _i32), ("n_extra", _i32), ("anchors", _i32),
        ("conf_thres", _f32), ("iou_thres", _f32),
        ("max_det", _i32), ("max_nms", _i32),
        ("max_wh", _f32), ("agnostic", _i32),
        ("classes_mask", _vp),
        ("out", _vp), ("out_count", _vp), ("out_index", _vp),
        ("workspace", _vp), ("workspace_bytes", _i64), ("prefiltered", _i32), ("multi_label", _i32),
    ]  # fmt: skip


class ObbDecodeDesc(C.Structure):
    """Mirror of ``dy_obb_decode_desc``."""

    _fields_ = [
        ("level", _vp * DY_MAX_LEVELS),
        ("h", _i32 * DY_MAX_LEVELS), ("w", _i32 * DY_MAX_LEVELS), ("ld", _i32 * DY_MAX_LEVELS),
        ("stride", _f32 * DY_MAX_LEVELS),
        ("n_levels", _i32), ("batch", _i32), ("nc", _i32), ("n_extra", _i32), ("anchors", _i32),
        ("pred", _vp), ("theta", _vp),
    ]  # fmt: skip


class ValMatchDesc(C.Structure):
    """Mirror of ``dy_val_match_desc``."""

    _fields_ = [
        ("rows", _vp), ("counts", _vp), ("tbox", _vp), ("tcls", _vp), ("timg", _vp), ("iouv", C.POINTER(_f32)),
        ("batch", _i32), ("max_det", _i32), ("n_labels", _i32), ("n_iouv", _i32),
        ("clip_w", _f32), ("clip_h", _f32), ("single_cls", _i32),
        ("tp", _vp), ("best_iou", _vp), ("best_label", _vp),
    ]  # fmt: skip


ValMatchRotatedDesc = ValMatchDesc  # dy_val_match_rotated_desc is a typedef of dy_val_match_desc (rows are 7 wide, tbox 8)


class TileMergeDesc(C.Structure):
    """Mirror of ``dy_tile_merge_desc``."""

    _fields_ = [
        ("rows", _vp), ("counts", _vp), ("offsets_yx", _vp),
        ("frames", _i32), ("tiles", _i32), ("max_det", _i32), ("nc", _i32), ("frame_h", _i32), ("frame_w", _i32),
        ("thr", _f32), ("metric", _i32), ("agnostic", _i32), ("merge_max_det", _i32),
        ("out", _vp), ("out_count", _vp), ("out_index", _vp), ("workspace", _vp), ("workspace_bytes", _i64),
    ]  # fmt: skip


class TileFuseDesc(C.Structure):
    """Mirror of ``dy_tile_fuse_desc``."""

    _fields_ = [
        ("rows", _vp), ("counts", _vp), ("offsets_yx", _vp),
        ("frames", _i32), ("tiles", _i32), ("max_det", _i32), ("nc", _i32), ("frame_h", _i32), ("frame_w", _i32),
        ("thr", _f32), ("metric", _i32), ("agnostic", _i32), ("merge_max_det", _i32), ("mode", _i32),
        ("out", _vp), ("out_count", _vp), ("out_index", _vp), ("out_members", _vp), ("workspace", _vp), ("workspace_bytes", _i64),
    ]  # fmt: skip


class TileMergeRotatedDesc(C.Structure):
    """Mirror of ``dy_tile_merge_rotated_desc`` (``dy_tile_merge_desc`` without the metric; rows are 7 wide)."""

    _fields_ = [
        ("rows", _vp), ("counts", _vp), ("offsets_yx", _vp),
        ("frames", _i32), ("tiles", _i32), ("max_det", _i32), ("nc", _i32), ("frame_h", _i32), ("frame_w", _i32),
        ("thr", _f32), ("agnostic", _i32), ("merge_max_det", _i32),
        ("out", _vp), ("out_count", _vp), ("out_index", _vp), ("workspace", _vp), ("workspace_bytes", _i64),
    ]  # fmt: skip


class TileMaskOwnerDesc(C.Structure):
    """Mirror of ``dy_tile_mask_owner_desc``."""

    _fields_ = [
        ("rows", _vp), ("counts", _vp), ("offsets_yx", _vp), ("kept_index", _vp), ("kept_count", _vp),
        ("frames", _i32), ("tiles", _i32), ("max_det", _i32), ("merge_max_det", _i32),
        ("thr", _f32), ("metric", _i32), ("agnostic", _i32), ("stitch", _i32),
        ("owner", _vp),
    ]  # fmt: skip


class TileProcessMaskDesc(C.Structure):
    """Mirror of ``dy_tile_process_mask_desc``."""

    _fields_ = [
        ("protos", _vp), ("side", _vp), ("counts", _vp), ("offsets_yx", _vp), ("owner", _vp), ("dest", _vp),
        ("frames", _i32), ("tiles", _i32), ("max_det", _i32), ("merge_max_det", _i32), ("nm", _i32), ("mh", _i32), ("mw", _i32), ("ld_p", _i32),
        ("tile_h", _i32), ("tile_w", _i32), ("frame_h", _i32), ("frame_w", _i32), ("stride", _i32), ("total", _i32),
        ("out", _vp),
    ]  # fmt: skip


class TrackDesc(C.Structure):
    """Mirror of ``dy_track_desc``."""

    _fields_ = [
        ("rows", _vp), ("counts", _vp), ("state", _vp), ("state_bytes", _i64), ("workspace", _vp), ("workspace_bytes", _i64),
        ("out", _vp), ("out_count", _vp),
        ("frames", _i32), ("streams", _i32), ("max_det", _i32), ("max_tracks", _i32),
        ("track_high_thresh", _f32), ("track_low_thresh", _f32), ("new_track_thresh", _f32), ("match_thresh", _f32),
        ("fuse_score", _i32), ("max_time_lost", _i32),
    ]  # fmt: skip


class LossDesc(C.Structure):
    """Mirror of ``dy_loss_desc``."""

    _fields_ = [
        ("level", _vp * DY_MAX_LEVELS),
        ("h", _i32 * DY_MAX_LEVELS), ("w", _i32 * DY_MAX_LEVELS), ("ld", _i32 * DY_MAX_LEVELS),
        ("stride", _f32 * DY_MAX_LEVELS),
        ("n_levels", _i32), ("batch", _i32), ("nc", _i32), ("reg_max", _i32),
        ("gt", _vp), ("gmax", _i32), ("topk", _i32),
        ("alpha", _f32), ("beta", _f32), ("box_gain", _f32), ("cls_gain", _f32), ("dfl_gain", _f32),
        ("out", _vp), ("out_owner", _vp), ("workspace", _vp), ("workspace_bytes", _i64),
        ("grad_level", _vp * DY_MAX_LEVELS), ("ld_grad", _i32 * DY_MAX_LEVELS),
    ]  # fmt: skip


class ObbLossDesc(C.Structure):
    """Mirror of ``dy_obb_loss_desc``."""

    _fields_ = [
        ("level", _vp * DY_MAX_LEVELS), ("angle", _vp * DY_MAX_LEVELS),
        ("h", _i32 * DY_MAX_LEVELS), ("w", _i32 * DY_MAX_LEVELS), ("ld", _i32 * DY_MAX_LEVELS), ("ld_angle", _i32 * DY_MAX_LEVELS),
        ("stride", _f32 * DY_MAX_LEVELS),
        ("n_levels", _i32), ("batch", _i32), ("nc", _i32), ("reg_max", _i32),
        ("gt", _vp), ("gmax", _i32), ("topk", _i32),
        ("alpha", _f32), ("beta", _f32), ("box_gain", _f32), ("cls_gain", _f32), ("dfl_gain", _f32),
        ("out", _vp), ("out_owner", _vp), ("workspace", _vp), ("workspace_bytes", _i64),
        ("grad_level", _vp * DY_MAX_LEVELS), ("grad_angle", _vp * DY_MAX_LEVELS),
        ("ld_grad", _i32 * DY_MAX_LEVELS), ("ld_grad_angle", _i32 * DY_MAX_LEVELS),
    ]  # fmt: skip


class SegLossDesc(C.Structure):
    """Mirror of ``dy_seg_loss_desc``."""

    _fields_ = [
        ("owner", _vp), ("gt", _vp), ("coef", _vp * DY_MAX_LEVELS),
        ("h", _i32 * DY_MAX_LEVELS), ("w", _i32 * DY_MAX_LEVELS), ("ld_coef", _i32 * DY_MAX_LEVELS),
        ("n_levels", _i32), ("batch", _i32), ("nm", _i32), ("gmax", _i32), ("topk", _i32),
        ("proto", _vp), ("proto_dtype", _i32), ("ld_proto", _i32), ("mh", _i32), ("mw", _i32),
        ("masks", _vp), ("mask_dtype", _i32), ("gh", _i32), ("gw", _i32),
        ("img_h", _f32), ("img_w", _f32), ("box_gain", _f32),
        ("out", _vp), ("workspace", _vp), ("workspace_bytes", _i64),
        ("grad_coef", _vp * DY_MAX_LEVELS), ("ld_grad_coef", _i32 * DY_MAX_LEVELS),
        ("grad_proto", _vp), ("ld_grad_proto", _i32),
    ]  # fmt: skip


class C2fTailDesc(C.Structure):
    """Mirror of ``dy_c2f_tail_desc``."""

    _fields_ = [
        ("t", _vp), ("buf", _vp), ("y", _vp), ("w3", _vp), ("b3", _vp), ("w1", _vp), ("b1", _vp),
        ("batch", _i32), ("h", _i32), ("w", _i32), ("hidden", _i32), ("cout", _i32), ("n_bottlenecks", _i32), ("shortcut", _i32),
        ("ld_t", _i32), ("ld_buf", _i32), ("ld_y", _i32), ("dtype", _i32), ("act_l2e", _i32),
    ]  # fmt: skip


class C2fFrontDesc(C.Structure):
    """Mirror of ``dy_c2f_front_desc``."""

    _fields_ = [
        ("x", _vp), ("other", _vp), ("y", _vp), ("w3", _vp), ("b3", _vp), ("w1", _vp), ("b1", _vp),
        ("batch", _i32), ("h", _i32), ("w", _i32), ("cin", _i32), ("cmid", _i32), ("c_other", _i32), ("cout", _i32),
        ("ld_x", _i32), ("ld_other", _i32), ("ld_y", _i32), ("act", _i32), ("dtype", _i32),
    ]  # fmt: skip


class C2fDesc(C.Structure):
    """Mirror of ``dy_c2f_desc``."""

    _fields_ = [
        ("x", _vp), ("x_lo", _vp), ("y", _vp), ("w_cv1", _vp), ("w_m_cv1", _vp), ("w_m_cv2", _vp), ("w_cv2", _vp), ("bias", _vp),
        ("batch", _i32), ("h", _i32), ("w", _i32), ("cin", _i32), ("cin_lo", _i32), ("hidden", _i32), ("cout", _i32),
        ("ld_x", _i32), ("ld_x_lo", _i32), ("ld_y", _i32), ("shortcut", _i32), ("dtype", _i32), ("act_l2e", _i32),
    ]  # fmt: skip


class Stem2Desc(C.Structure):
    """Mirror of ``dy_stem2_desc``."""

    _fields_ = [
        ("x", _vp), ("w0", _vp), ("b0", _vp), ("w1", _vp), ("b1", _vp), ("y", _vp),
        ("n", _i32), ("h", _i32), ("w", _i32), ("ld_y", _i32), ("act0", _i32), ("act1", _i32), ("dtype", _i32),
        ("w1_scale", _vp),
    ]  # fmt: skip


class BnDesc(C.Structure):
    """Mirror of ``dy_bn_desc``."""

    _fields_ = [
        ("z", _vp), ("y", _vp), ("addend", _vp), ("dy", _vp), ("dz", _vp),
        ("rows", _i64),
        ("c", _i32), ("ld_z", _i32), ("ld_y", _i32), ("ld_add", _i32), ("ld_dy", _i32), ("ld_dz", _i32), ("dtype", _i32), ("act", _i32),
        ("gamma", _vp), ("beta", _vp), ("mean", _vp), ("rstd", _vp), ("running_mean", _vp), ("running_var", _vp),
        ("eps", _f32), ("momentum", _f32),
        ("dgamma", _vp), ("dbeta", _vp), ("workspace", _vp), ("workspace_bytes", _i64), ("partial_slabs", _i32),
    ]  # fmt: skip


class MaskGatherDesc(C.Structure):
    """Mirror of ``dy_mask_gather_desc``."""

    _fields_ = [
        ("rows", _vp), ("counts", _vp), ("index", _vp),
        ("level", _vp * DY_MAX_LEVELS),
        ("h", _i32 * DY_MAX_LEVELS), ("w", _i32 * DY_MAX_LEVELS), ("ld", _i32 * DY_MAX_LEVELS),
        ("n_levels", _i32),
        ("pred", _vp), ("pred_ch", _i32), ("pred_c0", _i32), ("anchors", _i32),
        ("batch", _i32), ("max_det", _i32), ("nm", _i32),
        ("out", _vp),
    ]  # fmt: skip


class ProcessMaskDesc(C.Structure):
    """Mirror of ``dy_process_mask_desc``."""

    _fields_ = [
        ("protos", _vp), ("side", _vp), ("counts", _vp), ("offsets", _vp), ("window", _vp), ("crop_rows", _vp),
        ("batch", _i32), ("max_det", _i32), ("nm", _i32), ("mh", _i32), ("mw", _i32), ("ld_p", _i32), ("oh", _i32), ("ow", _i32),
        ("total", _i32), ("crop_at_output", _i32),
        ("ratio_x", _f32), ("ratio_y", _f32),
        ("out", _vp),
    ]  # fmt: skip


class KptDecodeDesc(C.Structure):
    """Mirror of ``dy_kpt_decode_desc``."""

    _fields_ = [
        ("level", _vp * DY_MAX_LEVELS),
        ("h", _i32 * DY_MAX_LEVELS), ("w", _i32 * DY_MAX_LEVELS), ("ld", _i32 * DY_MAX_LEVELS),
        ("stride", _f32 * DY_MAX_LEVELS),
        ("n_levels", _i32),
        ("batch", _i32), ("anchors", _i32), ("nkpt", _i32), ("ndim", _i32),
        ("pred_kpt", _vp), ("counts", _vp), ("index", _vp),
        ("max_det", _i32),
        ("out", _vp),
    ]  # fmt: skip


DY_MAP_U8, DY_MAP_I32 = 0, 1
VAL_MASK_MAX_LABELS = 1024  # labels per image dy_val_mask_match takes (csrc/val_mask.hip: one LDS bin each)


class ValMaskMatchDesc(C.Structure):
    """Mirror of ``dy_val_mask_match_desc``."""

    _fields_ = [
        ("protos", _vp), ("side", _vp), ("rows", _vp), ("counts", _vp), ("map", _vp), ("tcls", _vp), ("loff", _vp), ("iouv", C.POINTER(_f32)),
        ("batch", _i32), ("max_det", _i32), ("nm", _i32), ("mh", _i32), ("mw", _i32), ("ld_p", _i32), ("gh", _i32), ("gw", _i32),
        ("map_dtype", _i32), ("n_labels", _i32), ("l_cap", _i32), ("n_iouv", _i32),
        ("in_w", _i32), ("in_h", _i32), ("single_cls", _i32),
        ("tp_m", _vp), ("best_iou", _vp), ("best_label", _vp), ("area_gt", _vp), ("inter", _vp), ("area_pred", _vp),
    ]  # fmt: skip


OKS_MAX_KPT = 32  # DY_OKS_MAX_KPT: keypoints per label dy_val_oks_match takes (csrc/val_oks.hip: the LDS stage is sized for it)


class ValOksMatchDesc(C.Structure):
    """Mirror of ``dy_val_oks_match_desc``."""

    _fields_ = [
        ("rows", _vp), ("counts", _vp), ("kpts", _vp), ("index", _vp),
        ("stride_b", _i64), ("stride_ch", _i64), ("stride_d", _i64), ("anchors", _i32),
        ("tbox", _vp), ("tkpt", _vp), ("tcls", _vp), ("timg", _vp), ("sigma", C.POINTER(_f32)), ("iouv", C.POINTER(_f32)),
        ("batch", _i32), ("max_det", _i32), ("n_labels", _i32), ("n_iouv", _i32), ("nkpt", _i32), ("ndim", _i32),
        ("clip_w", _f32), ("clip_h", _f32), ("single_cls", _i32),
        ("tp", _vp), ("best_iou", _vp), ("best_label", _vp),
    ]  # fmt: skip


DY_AUG_FLIPLR, DY_AUG_FLIPUD, DY_AUG_HSV_OFF = 1, 2, 4


class AugSrc(C.Structure):
    """Mirror of ``dy_aug_src``: one pasted rectangle of an augmented image."""

    _fields_ = [("index", _i32), ("x1a", _i32), ("y1a", _i32), ("x2a", _i32), ("y2a", _i32), ("x1b", _i32), ("y1b", _i32), ("reserved", _i32)]


class AugRow(C.Structure):
    """Mirror of ``dy_aug_row``: the table row of one output image of ``dy_augment_u8_nchw``."""

    _fields_ = [("n_src", _i32), ("ch", _i32), ("cw", _i32), ("flags", _i32), ("src", AugSrc * 4), ("minv", _f32 * 9), ("hsv", _f32 * 3)]


# name -> (restype, argtypes); every symbol include/dyolo.h declares must appear here
# (tests/test_cabi.py checks both directions).
SIGNATURES = {
    "dy_version": (_i32, []),
    "dy_last_error_string": (C.c_char_p, []),
    "dy_last_kernel_name": (C.c_char_p, []),
    "dy_dtype_size": (_i32, [_i32]),
    "dy_pack_conv_weights_table_bytes": (C.c_int64, [_i32]),
    "dy_pack_conv_weights_table": (_i32, [C.POINTER(PackJob), _i32, _i32, _vp, C.c_int64, C.POINTER(C.c_int32)]),
    "dy_pack_conv_weights_batched": (_i32, [_vp, _i32, _i32, _i32, _vp]),
    "dy_conv_k_pad": (_i32, [_i32, _i32, _i32]),
    "dy_conv_cout_pad": (_i32, [_i32]),
    "dy_conv2d_nhwc": (_i32, [C.POINTER(ConvDesc), _vp]),
    "dy_conv_stats_written": (_i32, []),
    "dy_conv3x3_halo_route": (_i32, [_i32, _i32, _i32, _i32, _i64, _i64, _i32, C.c_uint64, _i32, _i32, _i32]),
    "dy_conv1x1_stream_supported": (_i32, [_i32, _i32, _i32, _i32]),
    "dy_c2f_fused_supported": (_i32, [_i32, _i32, _i32, _i32, _i32, _i32]),
    "dy_c2f_fused": (_i32, [C.POINTER(C2fDesc), _vp]),
    "dy_c2f_tail_fused_supported": (_i32, [_i32, _i32, _i32, _i32, _i32, _i32, _i32]),
    "dy_c2f_tail_fused": (_i32, [C.POINTER(C2fTailDesc), _vp]),
    "dy_c2f_front_fused_supported": (_i32, [_i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32]),
    "dy_c2f_front_fused": (_i32, [C.POINTER(C2fFrontDesc), _vp]),
    "dy_stem2_fused_supported": (_i32, [_i32, _i32, _i32, _i32, _i32, _i32]),
    "dy_stem2_fused": (_i32, [C.POINTER(Stem2Desc), _vp]),
    "dy_stem_conv3x3s2_nchw": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "dy_stem_conv3x3s2_nchw_u8": (_i32, [_vp, _f32, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "dy_nchw_f32_to_nhwc": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "dy_resize_bilinear_u8_nchw_f32": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "dy_scale_img_nchw_f32": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _vp]),
    "dy_nhwc_to_nchw_f32": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "dy_upsample2x_nhwc": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "dy_copy_nhwc": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "dy_sppf_maxpool3": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "dy_detect_decode": (_i32, [C.POINTER(DecodeDesc), _vp]),
    "dy_detect_head_decode_supported": (_i32, [_i32, _i32, _i32, _i32, _i32]),
    "dy_detect_head_decode": (_i32, [C.POINTER(HeadDecodeDesc), _vp]),
    "dy_nms_workspace_bytes": (_i64, [_i32, _i32]),
    "dy_nms": (_i32, [C.POINTER(NmsDesc), _vp]),
    "dy_nms_small_cap": (_i32, []),
    "dy_scale_boxes": (_i32, [_vp, _vp, _vp, _i32, _i32, _vp]),
    "dy_obb_decode": (_i32, [C.POINTER(ObbDecodeDesc), _vp]),
    "dy_nms_rotated_workspace_bytes": (_i64, [_i32, _i32]),
    "dy_nms_rotated": (_i32, [C.POINTER(NmsDesc), _vp, _vp]),
    "dy_nms_rotated_lds_cap": (_i32, []),
    "dy_nms_rotated_ml_workspace_bytes": (_i64, [_i32, _i32, _i32]),
    "dy_nms_rotated_ml": (_i32, [C.POINTER(NmsDesc), _vp, _vp]),
    "dy_scale_rboxes": (_i32, [_vp, _vp, _vp, _i32, _i32, _vp]),
    "dy_val_match": (_i32, [C.POINTER(ValMatchDesc), _vp]),
    "dy_val_match_rotated": (_i32, [C.POINTER(ValMatchRotatedDesc), _vp]),
    "dy_track_state_bytes": (_i64, [_i32, _i32]),
    "dy_track_workspace_bytes": (_i64, [_i32, _i32, _i32]),
    "dy_track_reset": (_i32, [_vp, _i32, _i32, _vp]),
    "dy_track_step": (_i32, [C.POINTER(TrackDesc), _vp]),
    "dy_track_state_bytes_rotated": (_i64, [_i32, _i32]),
    "dy_track_workspace_bytes_rotated": (_i64, [_i32, _i32, _i32]),
    "dy_track_reset_rotated": (_i32, [_vp, _i32, _i32, _vp]),
    "dy_track_step_rotated": (_i32, [C.POINTER(TrackDesc), _vp]),
    "dy_detection_loss_workspace_bytes": (_i64, [_i32, _i32, _i32, _i32]),
    "dy_conv2d_wgrad_nhwc": (_i32, [C.POINTER(ConvDesc), _vp, _i32, _vp, _vp]),
    "dy_conv2d_wgrad_nhwc_ws": (_i32, [C.POINTER(ConvDesc), _vp, _i32, _vp, _vp, C.c_int64, _vp]),
    "dy_conv2d_wgrad_workspace_bytes": (C.c_int64, [C.POINTER(ConvDesc), _i32]),
    "dy_quantize_fp8_nhwc": (_i32, [_vp, _vp, _i64, _i32, _i32, _i32, _i32, _f32, _vp]),
    "dy_pack_conv_weights": (_i32, [_vp, _i64, _i64, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _vp, _i64, _i32, _i32, _vp]),
    "dy_detect_branch_fused_supported": (_i32, [_i32, _i32, _i32, _i32, _i32, _i32, _i32]),
    "dy_detect_branch_fused": (_i32, [C.POINTER(BranchDesc), _vp]),
    "dy_nms_reset_counts": (_i32, [_vp, _i32, _vp]),
    "dy_conv2d_grouped_bwd_nhwc": (_i32, [C.POINTER(ConvDesc), _vp, _i32, _vp, _vp, _vp, _i32, _vp, _i32, _vp]),
    "dy_colsum": (_i32, [_vp, _vp, _i64, _i32, _i32, _i32, _vp]),
    "dy_nchw_u8_to_nhwc": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _i32, _vp]),
    "dy_letterbox_u8_to_nchw_f32": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _vp]),
    "dy_tiles_u8_to_nchw_f32": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _vp]),
    "dy_rows_to_pred": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp]),
    "dy_tiles_batch_u8_to_nchw_f32": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _vp]),
    "dy_tile_merge_workspace_bytes": (_i64, [_i32, _i32, _i32]),
    "dy_tile_merge": (_i32, [C.POINTER(TileMergeDesc), _vp]),
    "dy_tile_fuse_workspace_bytes": (_i64, [_i32, _i32, _i32, _i32]),
    "dy_tile_fuse": (_i32, [C.POINTER(TileFuseDesc), _vp]),
    "dy_tile_merge_rotated_workspace_bytes": (_i64, [_i32, _i32, _i32]),
    "dy_tile_merge_rotated": (_i32, [C.POINTER(TileMergeRotatedDesc), _vp]),
    "dy_tile_mask_owner": (_i32, [C.POINTER(TileMaskOwnerDesc), _vp]),
    "dy_tile_process_mask": (_i32, [C.POINTER(TileProcessMaskDesc), _vp]),
    "dy_upsample2x_bwd_nhwc": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "dy_maxpool_bwd_nhwc": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "dy_add_nhwc": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp]),
    "dy_add_dilated2_nhwc": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "dy_head_grad_split": (_i32, [_vp, _i32, _i64, _i32, _i32, _i32, _vp, _vp, _i32, _vp, _i32, _i32, _vp]),
    "dy_sumsq_f32": (_i32, [_vp, _i64, _vp, _vp]),
    "dy_sgd_step": (_i32, [_vp, _vp, _vp, _i64, _f32, _f32, _f32, _i32, _i32, _vp, _f32, _vp, _vp]),
    "dy_adamw_step": (_i32, [_vp, _vp, _vp, _vp, _i64, _f32, _f32, _f32, _f32, _f32, _i32, _vp, _f32, _vp, _vp]),
    "dy_amp_update": (_i32, [_vp, _vp, _f32, _f32, _i32, _vp]),
    "dy_ema_update": (_i32, [_vp, _vp, _i64, _f32, _vp]),
    "dy_grad_sink_flush": (_i32, [_vp, _i32, _vp, _vp, _vp]),
    "dy_bn_workspace_bytes": (_i64, [_i32]),
    "dy_bn_train_fwd": (_i32, [C.POINTER(BnDesc), _vp]),
    "dy_bn_train_bwd": (_i32, [C.POINTER(BnDesc), _vp]),
    "dy_silu_fwd": (_i32, [_vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp]),
    "dy_silu_bwd": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp]),
    "dy_detection_loss": (_i32, [C.POINTER(LossDesc), _vp]),
    "dy_obb_loss_workspace_bytes": (_i64, [_i32, _i32, _i32, _i32]),
    "dy_obb_loss": (_i32, [C.POINTER(ObbLossDesc), _vp]),
    "dy_obb_angle_grad_cast": (_i32, [_vp, _i32, _i64, _vp, _vp, _i32, _i32, _vp]),
    "dy_seg_loss_workspace_bytes": (_i64, [_i32, _i32, _i32, _i32]),
    "dy_seg_loss": (_i32, [C.POINTER(SegLossDesc), _vp]),
    "dy_space_to_depth2_nhwc": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "dy_grad_cast_scaled": (_i32, [_vp, _i32, _i64, _i32, _vp, _vp, _i32, _i32, _vp]),
    "dy_augment_u8_nchw": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp]),
    "dy_depth_to_space2_nhwc": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "dy_mask_gather": (_i32, [C.POINTER(MaskGatherDesc), _vp]),
    "dy_process_mask": (_i32, [C.POINTER(ProcessMaskDesc), _vp]),
    "dy_val_mask_match": (_i32, [C.POINTER(ValMaskMatchDesc), _vp]),
    "dy_kpt_decode": (_i32, [C.POINTER(KptDecodeDesc), _vp]),
    "dy_val_oks_match": (_i32, [C.POINTER(ValOksMatchDesc), _vp]),
    "dy_scale_coords": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "dy_crops_letterbox_u8_to_nchw_f32": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _vp]),
}

_lib = None


class DyoloError(RuntimeError):
    """A libdyolo call returned a non-zero ``dy_status``."""


def lib() -> C.CDLL:
    """Load (once) and return the library; raise loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} not found: the HIP extension has not been built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` or `make -C drone-yolo_amd/csrc`. "
                "There is no CPU / eager fallback for this path."
            )
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def check(rc: int, what: str = "libdyolo") -> None:
    if rc != 0:
        msg = lib().dy_last_error_string()
        raise DyoloError(f"{what} failed with status {rc}: {msg.decode() if msg else ''}")
