"""ctypes binding of libtdn.so (the C ABI declared in include/tdn.h).

The library is built in-tree by ``__graft_entry__.build()`` / ``make -C torch_detection_amd/csrc``.
There is no fallback: if the shared object is missing or a call fails, a RuntimeError is raised.
"""
import ctypes
import os
import threading

import torch  # noqa: F401  (loads the HIP runtime first so libtdn binds to the same libamdhip64)

_HERE = os.path.dirname(os.path.abspath(__file__))
# TDN_LIB: another build of the library in the package directory, for A/B runs of two builds (scripts/norm_bench.py);
# the package, the tests and bench.py use the product, libtdn.so
LIB_PATH = os.path.join(_HERE, os.path.basename(os.environ.get("TDN_LIB", "") or "libtdn.so"))

TDN_BF16 = 0
TDN_F16 = 1
TDN_F32 = 2
NMS_SEG_MAX = 4096
RPN_MAX_LEVELS = 8
RPN_MAX_NUM = 8192
ROI_MAX_LEVELS = 8
ROI_MAX_OUT = 16
ROI_MAX_SAMPLES = 512
TARGET_MAX_GT = 256
TARGET_MAX_BOXES = 1 << 20
TARGET_MAX_NUM = 8192
LOSS_MAX_LEVELS = 8
PRED_MAX_LEVELS = 8
PYR_MAX_LEVELS = 8
LOSS_MAX_CLASSES = 1024
LOSS_MAX_ROWS = 1 << 20
LOSS_MAX_AVG = 64
GHM_MAX_BINS = 64
GHM_TABLE_STRIDE = 136
GHM_SCOPE_LEVEL, GHM_SCOPE_BATCH = 0, 1
DET_MAX_CLASSES = 1024
DET_MAX_ROWS = 1 << 18
CASCADE_MAX_STAGES = 8
REFINE_CHUNK = 1024
DENSE_MAX_LEVELS = 8
FCOS_MAX_LEVELS = 8
MASK_MAX_SIZE = 56
MASK_IOU_MAX_CANVAS = 8192
MASK_IOU_MAX_COUT = 512
SGD_MAX_ITEMS = 1 << 20
SGD_MAX_GROUPS = 1024
SGD_PATH_LINEAR, SGD_PATH_TRANSPOSED, SGD_PATH_GENERAL = 0, 1, 2
SGD_NESTEROV, SGD_SKIP_NONFINITE, SGD_DYNAMIC_SCALE = 1, 2, 4
SGD_F_SCALE, SGD_F_NORM, SGD_F_COEF, SGD_F_SNAP_SCALE, SGD_F_COUNT = 0, 1, 2, 3, 4
SGD_I_TRACKER, SGD_I_TAKEN, SGD_I_SKIPPED, SGD_I_LAST_SKIPPED, SGD_I_BUF_INIT, SGD_I_SNAP_FIRST, SGD_I_COUNT = \
    0, 1, 2, 3, 4, 5, 8
ADD_NONE, ADD_SAME, ADD_UP2X, ADD_SUMPOOL2 = 0, 1, 2, 3

c_void_p = ctypes.c_void_p
c_int = ctypes.c_int
c_i64 = ctypes.c_int64
c_float = ctypes.c_float


class Epilogue(ctypes.Structure):
    """Mirror of ``tdn_epilogue`` (include/tdn.h)."""
    _fields_ = [
        ("scale", c_void_p),
        ("shift", c_void_p),
        ("addend", c_void_p),
        ("addend_mode", ctypes.c_int32),
        ("addend_h", ctypes.c_int32),
        ("addend_w", ctypes.c_int32),
        ("relu", ctypes.c_int32),
        ("mask_src", c_void_p),
        ("out_f32", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


_EP = ctypes.POINTER(Epilogue)


class WgradItem(ctypes.Structure):
    """Mirror of ``tdn_wgrad_item`` (include/tdn.h): one member of a grouped weight-gradient launch."""
    _fields_ = [
        ("x", c_void_p), ("g", c_void_p), ("w_fwd", c_void_p),
        ("scale", c_void_p), ("mean", c_void_p), ("invstd", c_void_p),
        ("dw", c_void_p), ("dgamma", c_void_p), ("dbeta", c_void_p),
        ("beta", c_float), ("kind", ctypes.c_int32),
        ("N", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32),
        ("Cin", ctypes.c_int32), ("Cout", ctypes.c_int32),
        ("k", ctypes.c_int32), ("stride", ctypes.c_int32), ("pad", ctypes.c_int32),
        ("groups", ctypes.c_int32), ("reserved", ctypes.c_int32),
    ]


_WI = ctypes.POINTER(WgradItem)


class PrepItem(ctypes.Structure):
    """Mirror of ``tdn_prep_item`` (include/tdn.h): one conv unit of a grouped fold + pack launch."""
    _fields_ = [
        ("w", c_void_p), ("w_fwd", c_void_p), ("w_dgrad", c_void_p),
        ("gamma", c_void_p), ("beta", c_void_p), ("mean", c_void_p), ("var", c_void_p), ("fold", c_void_p),
        ("s_o", c_i64), ("s_i", c_i64), ("s_h", c_i64), ("s_w", c_i64),
        ("Cout", ctypes.c_int32), ("Cin", ctypes.c_int32), ("kh", ctypes.c_int32), ("kw", ctypes.c_int32),
        ("eps", c_float), ("reserved", ctypes.c_int32),
    ]


_PI = ctypes.POINTER(PrepItem)


class AnchorLevel(ctypes.Structure):
    """Mirror of ``tdn_anchor_level`` (include/tdn.h)."""
    _fields_ = [("base_anchors", c_void_p), ("A", ctypes.c_int32), ("featH", ctypes.c_int32),
                ("featW", ctypes.c_int32), ("stride", ctypes.c_int32), ("valid_h", ctypes.c_int32),
                ("valid_w", ctypes.c_int32)]


_AL = ctypes.POINTER(AnchorLevel)


class RpnLevel(ctypes.Structure):
    """Mirror of ``tdn_rpn_level`` (include/tdn.h)."""
    _fields_ = [("logits", c_void_p), ("deltas", c_void_p), ("anchors", c_void_p),
                ("logit_strides", c_i64 * 4), ("delta_strides", c_i64 * 4),
                ("dtype", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32), ("A", ctypes.c_int32)]


class RpnConfig(ctypes.Structure):
    """Mirror of ``tdn_rpn_config`` (include/tdn.h)."""
    _fields_ = [("nms_pre", ctypes.c_int32), ("nms_post", ctypes.c_int32), ("max_num", ctypes.c_int32),
                ("nms_thr", c_float), ("min_bbox_size", c_float), ("means", c_float * 4), ("stds", c_float * 4),
                ("reserved", ctypes.c_int32)]


_RL = ctypes.POINTER(RpnLevel)
_RC = ctypes.POINTER(RpnConfig)


class TargetConfig(ctypes.Structure):
    """Mirror of ``tdn_target_config`` (include/tdn.h)."""
    _fields_ = [("pos_iou_thr", c_float), ("neg_iou_thr", c_float), ("min_pos_iou", c_float),
                ("gt_max_assign_all", ctypes.c_int32), ("num", ctypes.c_int32), ("num_pos_expected", ctypes.c_int32),
                ("allowed_border", ctypes.c_int32), ("add_gt_as_proposals", ctypes.c_int32),
                ("neg_pos_ub", ctypes.c_double), ("means", c_float * 4), ("stds", c_float * 4),
                ("seed", ctypes.c_uint32), ("reserved", ctypes.c_int32)]


_TC = ctypes.POINTER(TargetConfig)


class BalancedConfig(ctypes.Structure):
    """Mirror of ``tdn_balanced_config`` (include/tdn.h)."""
    _fields_ = [("floor_thr", c_float), ("floor_fraction", c_float), ("num_bins", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


_BC = ctypes.POINTER(BalancedConfig)


class LossLevel(ctypes.Structure):
    """Mirror of ``tdn_loss_level`` (include/tdn.h)."""
    _fields_ = [("cls", c_void_p), ("reg", c_void_p), ("dcls", c_void_p), ("dreg", c_void_p),
                ("H", ctypes.c_int32), ("W", ctypes.c_int32), ("cls_nhwc", ctypes.c_int32),
                ("reg_nhwc", ctypes.c_int32)]


class LossConfig(ctypes.Structure):
    """Mirror of ``tdn_loss_config`` (include/tdn.h)."""
    _fields_ = [("dtype", ctypes.c_int32), ("num_anchors", ctypes.c_int32), ("num_classes", ctypes.c_int32),
                ("focal", ctypes.c_int32), ("beta", c_float), ("gamma", c_float), ("alpha", c_float),
                ("reserved", ctypes.c_int32)]


class LossAvg(ctypes.Structure):
    """Mirror of ``tdn_loss_avg`` (include/tdn.h)."""
    _fields_ = [("a", c_void_p), ("b", c_void_p), ("na", ctypes.c_int32), ("nb", ctypes.c_int32),
                ("mode", ctypes.c_int32), ("value", c_float)]


_LL = ctypes.POINTER(LossLevel)
_LC = ctypes.POINTER(LossConfig)
_LA = ctypes.POINTER(LossAvg)


class RoiLevel(ctypes.Structure):
    """Mirror of ``tdn_roi_level`` (include/tdn.h)."""
    _fields_ = [("data", c_void_p), ("strides", c_i64 * 4), ("H", ctypes.c_int32), ("W", ctypes.c_int32),
                ("dtype", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class RoiConfig(ctypes.Structure):
    """Mirror of ``tdn_roi_config`` (include/tdn.h)."""
    _fields_ = [("out_size", ctypes.c_int32), ("sampling_ratio", ctypes.c_int32), ("finest_scale", c_float),
                ("reserved", ctypes.c_int32), ("scales", c_float * 8)]


class DeformDesc(ctypes.Structure):
    """Mirror of ``tdn_deform_desc`` (include/tdn.h)."""
    _fields_ = [("x", c_void_p), ("offset", c_void_p), ("mask", c_void_p), ("offset_pitch", c_i64),
                ("mask_pitch", c_i64), ("N", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32),
                ("C", ctypes.c_int32), ("stride", ctypes.c_int32), ("pad", ctypes.c_int32),
                ("deformable_groups", ctypes.c_int32), ("dtype", ctypes.c_int32), ("offset_dtype", ctypes.c_int32),
                ("mask_dtype", ctypes.c_int32), ("mask_is_logit", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class CarafeDesc(ctypes.Structure):
    """Mirror of ``tdn_carafe_desc`` (include/tdn.h)."""
    _fields_ = [("x", c_void_p), ("weights", c_void_p), ("addend", c_void_p), ("weight_pitch", c_i64),
                ("N", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32), ("C", ctypes.c_int32),
                ("kernel_size", ctypes.c_int32), ("group_size", ctypes.c_int32), ("scale_factor", ctypes.c_int32),
                ("out_h", ctypes.c_int32), ("out_w", ctypes.c_int32), ("dtype", ctypes.c_int32),
                ("weight_dtype", ctypes.c_int32), ("weights_are_logits", ctypes.c_int32)]


_CfD = ctypes.POINTER(CarafeDesc)
_DfD = ctypes.POINTER(DeformDesc)
_RoL = ctypes.POINTER(RoiLevel)
_RoC = ctypes.POINTER(RoiConfig)


class BottleneckArgs(ctypes.Structure):
    """Mirror of ``tdn_bottleneck_args`` (include/tdn.h)."""
    _fields_ = [("in_", c_void_p), ("w1", c_void_p), ("w2", c_void_p), ("w3", c_void_p),
                ("scale1", c_void_p), ("shift1", c_void_p), ("scale2", c_void_p), ("shift2", c_void_p),
                ("scale3", c_void_p), ("shift3", c_void_p),
                ("mask1", c_void_p), ("mask2", c_void_p), ("mask3", c_void_p),
                ("out1", c_void_p), ("out2", c_void_p), ("out3", c_void_p),
                ("N", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32), ("C", ctypes.c_int32),
                ("bits1", c_void_p), ("bits2", c_void_p), ("bits3", c_void_p)]


_BA = ctypes.POINTER(BottleneckArgs)


class BottleneckHeadArgs(ctypes.Structure):
    """Mirror of ``tdn_bottleneck_head_args`` (include/tdn.h)."""
    _fields_ = [("b", BottleneckArgs), ("addend", c_void_p), ("wd", c_void_p), ("scale_d", c_void_p),
                ("shift_d", c_void_p)]


_BHA = ctypes.POINTER(BottleneckHeadArgs)


class SgdItem(ctypes.Structure):
    """Mirror of ``tdn_sgd_item`` (include/tdn.h): one parameter of a fused SGD step."""
    _fields_ = [("p", c_void_p), ("g", c_void_p), ("buf", c_void_p),
                ("shape", c_i64 * 4), ("p_stride", c_i64 * 4), ("g_stride", c_i64 * 4),
                ("group", ctypes.c_int32), ("reserved", ctypes.c_int32)]


_SI = ctypes.POINTER(SgdItem)
_I64P = ctypes.POINTER(c_i64)


class PredLevel(ctypes.Structure):
    """Mirror of ``tdn_pred_level`` (include/tdn.h): one pyramid level of the dense head predictors."""
    _fields_ = [("h", c_void_p), ("cls", c_void_p), ("reg", c_void_p), ("dh", c_void_p), ("rows", c_i64)]


_PL = ctypes.POINTER(PredLevel)


class PyrLevel(ctypes.Structure):
    """Mirror of ``tdn_pyr_level`` (include/tdn.h): one pyramid level of the shared-weight 3x3 conv."""
    _fields_ = [("x", c_void_p), ("y", c_void_p), ("dx", c_void_p), ("mask_src", c_void_p), ("addend", c_void_p),
                ("H", ctypes.c_int32), ("W", ctypes.c_int32)]


_PyL = ctypes.POINTER(PyrLevel)


class PyrGnLevel(ctypes.Structure):
    """Mirror of ``tdn_pyr_gn_level`` (include/tdn.h): one pyramid level of the shared-affine GroupNorm."""
    _fields_ = [("z", c_void_p), ("y", c_void_p), ("g", c_void_p), ("dz", c_void_p),
                ("H", ctypes.c_int32), ("W", ctypes.c_int32)]


_PgL = ctypes.POINTER(PyrGnLevel)


class BfpLevel(ctypes.Structure):
    """Mirror of ``tdn_bfp_level`` (include/tdn.h): one pyramid level of the Balanced Feature Pyramid."""
    _fields_ = [("x", c_void_p), ("out", c_void_p), ("g", c_void_p), ("dx", c_void_p),
                ("H", ctypes.c_int32), ("W", ctypes.c_int32)]


_BfL = ctypes.POINTER(BfpLevel)
_I32P = ctypes.POINTER(ctypes.c_int32)


class DenseLevel(ctypes.Structure):
    """Mirror of ``tdn_dense_level`` (include/tdn.h): one pyramid level of a single-stage head's outputs."""
    _fields_ = [("cls", c_void_p), ("reg", c_void_p), ("anchors", c_void_p),
                ("cls_strides", c_i64 * 4), ("reg_strides", c_i64 * 4), ("H", ctypes.c_int32), ("W", ctypes.c_int32)]


class DenseConfig(ctypes.Structure):
    """Mirror of ``tdn_dense_config`` (include/tdn.h)."""
    _fields_ = [("wh_ratio_clip", ctypes.c_double), ("dtype", ctypes.c_int32), ("num_anchors", ctypes.c_int32),
                ("num_classes", ctypes.c_int32), ("nms_pre", ctypes.c_int32), ("max_num", ctypes.c_int32),
                ("score_thr", c_float), ("nms_thr", c_float), ("scale_factor", c_float),
                ("means", c_float * 4), ("stds", c_float * 4)]


_DL = ctypes.POINTER(DenseLevel)
_DC = ctypes.POINTER(DenseConfig)


class FcosLevel(ctypes.Structure):
    """Mirror of ``tdn_fcos_level`` (include/tdn.h): one pyramid level of an FCOS head."""
    _fields_ = [("cls", c_void_p), ("reg", c_void_p), ("ctr", c_void_p),
                ("dcls", c_void_p), ("dreg", c_void_p), ("dctr", c_void_p),
                ("H", ctypes.c_int32), ("W", ctypes.c_int32), ("stride", ctypes.c_int32),
                ("cls_nhwc", ctypes.c_int32), ("reg_nhwc", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("lo", c_float), ("hi", c_float)]


class FcosLossConfig(ctypes.Structure):
    """Mirror of ``tdn_fcos_loss_config`` (include/tdn.h)."""
    _fields_ = [("dtype", ctypes.c_int32), ("num_classes", ctypes.c_int32), ("giou", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("gamma", c_float), ("alpha", c_float), ("eps", c_float),
                ("reserved2", ctypes.c_int32)]


class FcosDetConfig(ctypes.Structure):
    """Mirror of ``tdn_fcos_det_config`` (include/tdn.h)."""
    _fields_ = [("dtype", ctypes.c_int32), ("num_classes", ctypes.c_int32), ("nms_pre", ctypes.c_int32),
                ("max_num", ctypes.c_int32), ("score_thr", c_float), ("nms_thr", c_float), ("scale_factor", c_float),
                ("reserved", ctypes.c_int32)]


_FL = ctypes.POINTER(FcosLevel)
_FLC = ctypes.POINTER(FcosLossConfig)
_FDC = ctypes.POINTER(FcosDetConfig)

SOFT_NAIVE, SOFT_LINEAR, SOFT_GAUSSIAN = 0, 1, 2
SOFT_SIGMA_MIN, SOFT_SIGMA_MAX = 1.0 / 64, 64.0


class SoftNmsConfig(ctypes.Structure):
    """Mirror of ``tdn_soft_nms_config`` (include/tdn.h)."""
    _fields_ = [("method", ctypes.c_int32), ("iou_thr", c_float), ("sigma", c_float), ("min_score", c_float)]


_SNC = ctypes.POINTER(SoftNmsConfig)


class GhmConfig(ctypes.Structure):
    """Mirror of ``tdn_ghm_config`` (include/tdn.h)."""
    _fields_ = [("dtype", ctypes.c_int32), ("num_anchors", ctypes.c_int32), ("num_classes", ctypes.c_int32),
                ("bins_cls", ctypes.c_int32), ("bins_reg", ctypes.c_int32), ("scope", ctypes.c_int32),
                ("momentum_cls", c_float), ("momentum_reg", c_float), ("mu", c_float), ("reserved", ctypes.c_int32)]


_GC = ctypes.POINTER(GhmConfig)

GA_MAX_APPROX = 16


class GaLevel(ctypes.Structure):
    """Mirror of ``tdn_ga_level`` (include/tdn.h): one pyramid level of a Guided Anchoring head."""
    _fields_ = [("loc", c_void_p), ("shape", c_void_p), ("dloc", c_void_p), ("dshape", c_void_p),
                ("H", ctypes.c_int32), ("W", ctypes.c_int32), ("stride", ctypes.c_int32),
                ("shape_nhwc", ctypes.c_int32)]


class GaLocConfig(ctypes.Structure):
    """Mirror of ``tdn_ga_loc_config`` (include/tdn.h)."""
    _fields_ = [("area_thr", c_float * LOSS_MAX_LEVELS), ("center_r", c_float), ("center_c", c_float),
                ("ignore_r", c_float), ("ignore_c", c_float)]


class GaLossConfig(ctypes.Structure):
    """Mirror of ``tdn_ga_loss_config`` (include/tdn.h)."""
    _fields_ = [("dtype", ctypes.c_int32), ("gamma", c_float), ("alpha", c_float), ("beta", c_float),
                ("eps", c_float), ("loc_avg_factor", c_float), ("means", c_float * 4), ("stds", c_float * 4)]


_GaL = ctypes.POINTER(GaLevel)
_GaLC = ctypes.POINTER(GaLocConfig)
_GaSC = ctypes.POINTER(GaLossConfig)

# name -> (restype, argtypes); must list every symbol of include/tdn.h (tests/test_abi.py checks this)
SIGNATURES = {
    "tdn_last_error": (ctypes.c_char_p, []),
    "tdn_version": (c_int, []),
    "tdn_bn_fold": (c_int, [c_void_p] * 4 + [c_float, c_int] + [c_void_p] * 3 + [c_void_p]),
    "tdn_pack_conv_weight": (c_int, [c_void_p, c_i64, c_i64, c_i64, c_i64, c_int, c_int, c_int, c_int,
                                     c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "tdn_pack_stem_weight": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p]),
    "tdn_prepare_group": (c_int, [_PI, c_int, c_int, c_void_p]),
    "tdn_conv2d_fwd": (c_int, [c_void_p] * 3 + [c_int] * 8 + [_EP, c_int, c_void_p]),
    "tdn_conv2d_dgrad": (c_int, [c_void_p] * 3 + [c_int] * 8 + [_EP, c_int, c_void_p]),
    "tdn_conv2d_wgrad_workspace": (c_i64, [c_int] * 8),
    "tdn_conv2d_wgrad": (c_int, [c_void_p] * 9 + [c_float] + [c_int] * 8 + [c_void_p, c_i64, c_int, c_void_p]),
    "tdn_wgrad_group_workspace": (c_i64, [_WI, c_int, c_int]),
    "tdn_wgrad_group": (c_int, [_WI, c_int, c_void_p, c_i64, c_int, c_void_p]),
    "tdn_wgrad_group_plan": (c_int, [_WI, c_int, c_int, ctypes.POINTER(ctypes.c_int32),
                                     ctypes.POINTER(ctypes.c_int32)]),
    "tdn_stage_image": (c_int, [c_void_p, c_i64, c_i64, c_i64, c_i64, c_int, c_int, c_int, c_void_p, c_int,
                                c_void_p]),
    "tdn_stem_conv_fwd": (c_int, [c_void_p] * 3 + [c_int] * 4 + [_EP, c_int, c_void_p]),
    "tdn_stem_pool_fwd": (c_int, [c_void_p] * 6 + [c_int] * 5 + [c_void_p]),
    "tdn_stem_conv_wgrad_workspace": (c_i64, [c_int] * 4),
    "tdn_stem_conv_wgrad": (c_int, [c_void_p] * 9 + [c_float] + [c_int] * 4 + [c_void_p, c_i64, c_int, c_void_p]),
    "tdn_maxpool3x3s2_fwd": (c_int, [c_void_p] * 3 + [c_int] * 5 + [c_void_p]),
    "tdn_maxpool3x3s2_bwd": (c_int, [c_void_p] * 4 + [c_int] * 5 + [c_void_p]),
    "tdn_maxpool3x3s2_relu_bwd": (c_int, [c_void_p] * 4 + [c_int] * 5 + [c_void_p]),
    "tdn_subsample2_fwd": (c_int, [c_void_p] * 2 + [c_int] * 5 + [c_void_p]),
    "tdn_subsample2_bwd": (c_int, [c_void_p] * 3 + [c_int] * 5 + [c_void_p]),
    "tdn_add_relu_mask": (c_int, [c_void_p] * 4 + [c_i64, c_int, c_void_p]),
    "tdn_clamp_max": (c_int, [c_void_p, c_float, c_i64, c_int, c_void_p]),
    "tdn_act_mask": (c_int, [c_void_p] * 3 + [c_float, c_i64, c_int, c_void_p]),
    "tdn_channel_affine_fwd": (c_int, [c_void_p] * 4 + [c_i64, c_int, c_int, c_int, c_void_p]),
    "tdn_channel_affine_bwd_workspace": (c_i64, [c_i64, c_int]),
    "tdn_channel_affine_bwd": (c_int, [c_void_p] * 8 + [c_float, c_i64, c_int, c_void_p, c_i64, c_int, c_void_p]),
    "tdn_nchw_f32_to_nhwc": (c_int, [c_void_p, c_i64, c_i64, c_i64, c_i64, c_int, c_int, c_int, c_int, c_void_p,
                                     c_int, c_void_p]),
    "tdn_nchw16_to_nhwc": (c_int, [c_void_p, c_i64, c_i64, c_i64, c_i64, c_int, c_int, c_int, c_int, c_void_p,
                                   c_void_p]),
    "tdn_nhwc_to_nchw_f32": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p]),
    "tdn_anchor_grid": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "tdn_anchor_pyramid": (c_int, [_AL, c_int, c_void_p, c_void_p, c_void_p]),
    "tdn_bbox_iou_pairwise": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    "tdn_nms_workspace": (c_i64, [c_int]),
    "tdn_nms": (c_int, [c_void_p, c_void_p, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_i64,
                        c_void_p]),
    "tdn_bbox_normalize": (c_int, [c_void_p, c_i64, ctypes.POINTER(c_float), ctypes.POINTER(c_float), c_void_p]),
    "tdn_bbox_denormalize": (c_int, [c_void_p, c_void_p, c_i64, c_int, ctypes.POINTER(c_float),
                                     ctypes.POINTER(c_float), c_void_p]),
    "tdn_bbox2delta": (c_int, [c_void_p, c_void_p, c_i64, ctypes.POINTER(c_float), ctypes.POINTER(c_float), c_void_p,
                               c_void_p]),
    "tdn_delta2bbox": (c_int, [c_void_p, c_void_p, c_i64, c_int, ctypes.POINTER(c_float), ctypes.POINTER(c_float),
                               ctypes.POINTER(ctypes.c_int32), ctypes.c_double, c_void_p, c_void_p]),
    "tdn_batched_nms_workspace": (c_i64, [c_int, c_int]),
    "tdn_batched_nms": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_float, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_i64, c_void_p]),
    "tdn_rpn_proposals_workspace": (c_i64, [_RL, c_int, c_int, _RC]),
    "tdn_rpn_proposals": (c_int, [_RL, c_int, c_int, c_void_p, _RC, c_void_p, c_void_p, c_void_p, c_void_p, c_i64,
                                  c_void_p]),
    "tdn_assign_max_iou_workspace_bytes": (c_i64, [c_int, c_int]),
    "tdn_assign_max_iou": (c_int, [c_void_p, c_i64, c_void_p, c_i64, c_void_p, c_void_p, c_int, c_int, c_int, _TC, c_void_p,
                                   c_void_p, c_void_p, c_i64, c_void_p]),
    "tdn_sample_assigned": (c_int, [c_void_p, c_int, c_int, _TC] + [c_void_p] * 6),
    "tdn_anchor_target_workspace_bytes": (c_i64, [c_int, c_int, c_int]),
    "tdn_anchor_target": (c_int, [c_void_p, c_i64, c_void_p, c_i64] + [c_void_p] * 3 + [c_int, c_int, c_int, _TC] + [c_void_p] * 9 +
                          [c_i64, c_void_p]),
    "tdn_sample_rois_workspace_bytes": (c_i64, [c_int, c_int, c_int, c_int]),
    "tdn_sample_rois": (c_int, [c_void_p] * 5 + [c_int, c_int, c_int, _TC] + [c_void_p] * 10 + [c_i64, c_void_p]),
    "tdn_sample_assigned_balanced": (c_int, [c_void_p, c_void_p, c_int, c_int, _TC, _BC] + [c_void_p] * 6),
    "tdn_sample_rois_balanced_workspace_bytes": (c_i64, [c_int, c_int, c_int, c_int]),
    "tdn_sample_rois_balanced": (c_int, [c_void_p] * 5 + [c_int, c_int, c_int, _TC, _BC] + [c_void_p] * 10 +
                                 [c_i64, c_void_p]),
    "tdn_loss_dense_workspace_bytes": (c_i64, [_LL, c_int, c_int, _LC]),
    "tdn_loss_dense_fwd": (c_int, [_LL, c_int, c_int, _LC] + [c_void_p] * 4 + [_LA, c_void_p, c_void_p, c_void_p, c_i64,
                                                                              c_void_p]),
    "tdn_loss_dense_bwd": (c_int, [_LL, c_int, c_int, _LC] + [c_void_p] * 7),
    "tdn_ghm_workspace_bytes": (c_i64, [_LL, c_int, c_int, _GC]),
    "tdn_ghm_fwd": (c_int, [_LL, c_int, c_int, _GC] + [c_void_p] * 9 + [c_i64, c_void_p]),
    "tdn_ghm_bwd": (c_int, [_LL, c_int, c_int, _GC] + [c_void_p] * 7),
    "tdn_loss_roi_workspace_bytes": (c_i64, [c_int]),
    "tdn_loss_roi_fwd": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int] + [c_void_p] * 4 +
                         [c_float, _LA, c_void_p, c_void_p, c_void_p, c_i64, c_void_p]),
    "tdn_loss_roi_bwd": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int] + [c_void_p] * 4 +
                         [c_float] + [c_void_p] * 5),
    "tdn_loss_roi_balanced_fwd": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int] + [c_void_p] * 4 +
                                  [c_float, c_float, c_float, _LA, c_void_p, c_void_p, c_void_p, c_i64, c_void_p]),
    "tdn_loss_roi_balanced_bwd": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int] + [c_void_p] * 4 +
                                  [c_float, c_float, c_float] + [c_void_p] * 5),
    "tdn_multiclass_nms_workspace_bytes": (c_i64, [c_int, c_int, c_int]),
    "tdn_multiclass_nms": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_float,
                                   c_int] + [c_void_p] * 5 + [c_i64, c_void_p]),
    "tdn_bbox_detections_workspace_bytes": (c_i64, [c_int, c_int, c_int]),
    "tdn_bbox_detections": (c_int, [c_void_p] * 3 + [c_int] * 5 + [c_void_p, c_void_p, c_float,
                                    ctypes.POINTER(c_float), ctypes.POINTER(c_float), ctypes.c_double, c_float, c_float,
                                    c_int] + [c_void_p] * 7 + [c_i64, c_void_p]),
    "tdn_cascade_detections": (c_int, [c_void_p, ctypes.POINTER(c_void_p), c_int, c_void_p] + [c_int] * 5 +
                               [c_void_p, c_void_p, c_float, ctypes.POINTER(c_float), ctypes.POINTER(c_float),
                                ctypes.c_double, c_float, c_float, c_int] + [c_void_p] * 7 + [c_i64, c_void_p]),
    "tdn_refine_bboxes": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int,
                                  c_void_p, c_void_p, c_int, ctypes.POINTER(c_float), ctypes.POINTER(c_float),
                                  ctypes.c_double, c_int] + [c_void_p] * 4 + [c_i64, c_void_p]),
    "tdn_dense_detections_plan": (c_int, [_DL, c_int, c_int, _DC, ctypes.POINTER(ctypes.c_int32)]),
    "tdn_dense_detections_workspace_bytes": (c_i64, [_DL, c_int, c_int, _DC]),
    "tdn_dense_detections": (c_int, [_DL, c_int, c_int, c_void_p, c_void_p, _DC] + [c_void_p] * 10 + [c_i64, c_void_p]),
    "tdn_anchor_target_all_workspace_bytes": (c_i64, [c_int, c_int, c_int]),
    "tdn_anchor_target_all": (c_int, [c_void_p, c_i64, c_void_p, c_i64] + [c_void_p] * 4 + [c_int, c_int, c_int, _TC] +
                              [c_void_p] * 8 + [c_i64, c_void_p]),
    "tdn_fcos_points": (c_int, [_FL, c_int, c_void_p, c_void_p]),
    "tdn_fcos_target_workspace_bytes": (c_i64, [_FL, c_int, c_int, c_int]),
    "tdn_fcos_target": (c_int, [_FL, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_float] + [c_void_p] * 5 +
                        [c_i64, c_void_p]),
    "tdn_fcos_loss_workspace_bytes": (c_i64, [_FL, c_int, c_int, _FLC]),
    "tdn_fcos_loss_fwd": (c_int, [_FL, c_int, c_int, _FLC] + [c_void_p] * 7 + [c_i64, c_void_p]),
    "tdn_fcos_loss_bwd": (c_int, [_FL, c_int, c_int, _FLC] + [c_void_p] * 8),
    "tdn_fcos_detections_plan": (c_int, [_FL, c_int, c_int, _FDC, ctypes.POINTER(ctypes.c_int32)]),
    "tdn_fcos_detections_workspace_bytes": (c_i64, [_FL, c_int, c_int, _FDC]),
    "tdn_fcos_detections": (c_int, [_FL, c_int, c_int, c_void_p, c_void_p, c_void_p, _FDC] + [c_void_p] * 10 +
                            [c_i64, c_void_p]),
    "tdn_multiclass_nms_soft_workspace_bytes": (c_i64, [c_int, c_int, c_int]),
    "tdn_multiclass_nms_soft": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, _SNC,
                                        c_int] + [c_void_p] * 5 + [c_i64, c_void_p]),
    "tdn_bbox_detections_soft_workspace_bytes": (c_i64, [c_int, c_int, c_int]),
    "tdn_bbox_detections_soft": (c_int, [c_void_p] * 3 + [c_int] * 5 + [c_void_p, c_void_p, c_float,
                                         ctypes.POINTER(c_float), ctypes.POINTER(c_float), ctypes.c_double, c_float,
                                         _SNC, c_int] + [c_void_p] * 7 + [c_i64, c_void_p]),
    "tdn_cascade_detections_soft_workspace_bytes": (c_i64, [c_int, c_int, c_int]),
    "tdn_cascade_detections_soft": (c_int, [c_void_p, ctypes.POINTER(c_void_p), c_int, c_void_p] + [c_int] * 5 +
                                    [c_void_p, c_void_p, c_float, ctypes.POINTER(c_float), ctypes.POINTER(c_float),
                                     ctypes.c_double, c_float, _SNC, c_int] + [c_void_p] * 7 + [c_i64, c_void_p]),
    "tdn_dense_detections_soft_workspace_bytes": (c_i64, [_DL, c_int, c_int, _DC]),
    "tdn_dense_detections_soft": (c_int, [_DL, c_int, c_int, c_void_p, c_void_p, _DC, _SNC] + [c_void_p] * 10 +
                                  [c_i64, c_void_p]),
    "tdn_fcos_detections_soft_workspace_bytes": (c_i64, [_FL, c_int, c_int, _FDC]),
    "tdn_fcos_detections_soft": (c_int, [_FL, c_int, c_int, c_void_p, c_void_p, c_void_p, _FDC, _SNC] +
                                 [c_void_p] * 10 + [c_i64, c_void_p]),
    "tdn_ga_loc_target": (c_int, [_GaL, c_int, c_int, c_void_p, c_void_p, c_int, _GaLC, c_void_p, c_void_p, c_void_p]),
    "tdn_ga_shape_target_workspace_bytes": (c_i64, [c_int] * 3),
    "tdn_ga_shape_target": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_i64, c_void_p, c_void_p, c_void_p, c_int,
                                    c_int, c_int, _TC, c_int] + [c_void_p] * 9 + [c_i64, c_void_p]),
    "tdn_guided_anchors": (c_int, [_GaL, c_int, c_int, c_int, c_void_p, ctypes.POINTER(c_float),
                                   ctypes.POINTER(c_float), c_int, c_float, c_void_p, c_void_p, c_void_p]),
    "tdn_ga_loss_workspace_bytes": (c_i64, [_GaL, c_int, c_int, _GaSC]),
    "tdn_ga_loss_fwd": (c_int, [_GaL, c_int, c_int, _GaSC] + [c_void_p] * 5 + [_LA, c_void_p, c_void_p, c_void_p, c_i64,
                                                                              c_void_p]),
    "tdn_ga_loss_bwd": (c_int, [_GaL, c_int, c_int, _GaSC] + [c_void_p] * 8),
    "tdn_ga_rpn_proposals_workspace_bytes": (c_i64, [_RL, c_int, c_int, _RC]),
    "tdn_ga_rpn_proposals": (c_int, [_RL, c_int, c_int, c_void_p, c_void_p, c_void_p, _RC] + [c_void_p] * 4 +
                             [c_i64, c_void_p]),
    "tdn_mask_target": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int,
                                c_void_p, c_void_p, c_void_p]),
    "tdn_mask_loss_workspace_bytes": (c_i64, [c_int]),
    "tdn_mask_loss_fwd": (c_int, [c_void_p] + [c_int] * 5 + [c_void_p] * 3 + [_LA, c_void_p, c_void_p, c_void_p, c_i64,
                                                                              c_void_p]),
    "tdn_mask_loss_bwd": (c_int, [c_void_p] + [c_int] * 5 + [c_void_p] * 7),
    "tdn_rois_from_detections": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_float, c_void_p, c_void_p]),
    "tdn_mask_paste": (c_int, [c_void_p] + [c_int] * 6 + [c_void_p] * 4 + [c_int, c_int, c_float, c_int, c_void_p,
                                                                          c_void_p]),
    "tdn_mask_iou_target": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int,
                                    c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_float, c_void_p,
                                    c_void_p]),
    "tdn_mask_iou_loss_workspace_bytes": (c_i64, [c_int]),
    "tdn_mask_iou_loss_fwd": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_float, c_void_p, c_void_p,
                                      c_void_p, c_i64, c_void_p]),
    "tdn_mask_iou_loss_bwd": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_float] + [c_void_p] * 4),
    "tdn_mask_scores": (c_int, [c_void_p, c_int, c_int, c_int, c_int] + [c_void_p] * 5),
    "tdn_mask_iou_stem_fwd": (c_int, [c_void_p] + [c_int] * 5 + [c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_int,
                                                                 c_void_p, c_void_p, c_void_p]),
    "tdn_mask_iou_stem_bwd_workspace_bytes": (c_i64, [c_int] * 3),
    "tdn_mask_iou_stem_bwd": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p] +
                              [c_int] * 5 + [c_void_p, c_int] + [c_void_p] * 4 + [c_i64, c_void_p]),
    "tdn_sgd_plan": (c_int, [_SI, c_int, c_int, _I64P, c_void_p, c_i64, ctypes.POINTER(ctypes.c_int32)]),
    "tdn_sgd_step": (c_int, [c_void_p, _I64P, c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_int, c_float, c_float,
                             c_float, c_int, c_void_p]),
    "tdn_pack_linear_weight": (c_int, [c_void_p, c_i64, c_i64, c_int, c_int, c_int, c_void_p, c_void_p, c_int,
                                       c_void_p]),
    "tdn_linear_workspace_bytes": (c_i64, [c_int] * 5),
    "tdn_linear_relu_bwd": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p]),
    "tdn_linear_plan": (c_int, [c_int] * 5 + [ctypes.POINTER(ctypes.c_int32)]),
    "tdn_linear_fwd": (c_int, [c_void_p, c_i64, c_void_p, c_void_p, c_void_p, c_i64] + [c_int] * 6 +
                       [c_void_p, c_i64, c_int, c_void_p]),
    "tdn_linear_dgrad": (c_int, [c_void_p, c_i64, c_void_p, c_void_p, c_i64, c_void_p, c_i64] + [c_int] * 4 +
                         [c_void_p, c_i64, c_int, c_void_p]),
    "tdn_linear_wgrad": (c_int, [c_void_p, c_i64, c_void_p, c_i64, c_void_p, c_void_p, c_float] + [c_int] * 5 +
                         [c_void_p, c_i64, c_int, c_void_p]),
    "tdn_pack_deconv2x2_weight": (c_int, [c_void_p] + [c_i64] * 4 + [c_int, c_int, c_void_p, c_void_p, c_int, c_void_p]),
    "tdn_deconv2x2_workspace_bytes": (c_i64, [c_int] * 7),
    "tdn_deconv2x2_plan": (c_int, [c_int] * 7 + [ctypes.POINTER(ctypes.c_int32)]),
    "tdn_deconv2x2_fwd": (c_int, [c_void_p] * 4 + [c_int] * 7 + [c_void_p]),
    "tdn_deconv2x2_dgrad": (c_int, [c_void_p] * 3 + [c_int] * 6 + [c_void_p]),
    "tdn_deconv2x2_wgrad": (c_int, [c_void_p] * 4 + [c_float] + [c_int] * 6 + [c_void_p, c_i64, c_int, c_void_p]),
    "tdn_pack_pred_weight": (c_int, [c_void_p, c_i64, c_i64, c_void_p, c_i64, c_i64, c_int, c_int, c_void_p, c_void_p,
                                     c_int, c_void_p]),
    "tdn_pred_workspace_bytes": (c_i64, [c_int, _I64P, c_int, c_int, c_int]),
    "tdn_pred_plan": (c_int, [c_int, _I64P, c_int, c_int, c_int, ctypes.POINTER(ctypes.c_int32)]),
    "tdn_pred_fwd": (c_int, [_PL, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "tdn_pred_dgrad": (c_int, [_PL, c_int, c_void_p, c_int, c_int, c_int, c_void_p]),
    "tdn_pred_wgrad": (c_int, [_PL, c_int] + [c_void_p] * 4 + [c_int, c_int, c_void_p, c_i64, c_int, c_void_p]),
    "tdn_pack_pyr_weight": (c_int, [c_void_p, c_i64, c_i64, c_i64, c_i64, c_int, c_int, c_void_p, c_void_p, c_int,
                                    c_void_p]),
    "tdn_pyr_workspace_bytes": (c_i64, [c_int, c_int, _I32P, c_int, c_int, c_int]),
    "tdn_pyr_plan": (c_int, [c_int, c_int, _I32P, c_int, c_int, c_int, _I32P]),
    "tdn_pyr_conv_fwd": (c_int, [_PyL, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "tdn_pyr_conv_dgrad": (c_int, [_PyL, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p]),
    "tdn_pyr_conv_wgrad": (c_int, [_PyL, c_int, c_int, c_void_p, c_i64, c_i64, c_i64, c_i64, c_void_p, c_int, c_int,
                                   c_void_p, c_i64, c_int, c_void_p]),
    "tdn_pyr_gn_workspace_bytes": (c_i64, [c_int, c_int, _I32P, c_int, c_int, c_int]),
    "tdn_pyr_gn_plan": (c_int, [c_int, c_int, _I32P, c_int, c_int, c_int, _I32P]),
    "tdn_pyr_gn_fwd": (c_int, [_PgL, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_float, c_int, c_void_p, c_void_p,
                               c_i64, c_int, c_void_p]),
    "tdn_pyr_gn_bwd": (c_int, [_PgL, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_float,
                               c_void_p, c_i64, c_int, c_void_p]),
    "tdn_bfp_gather_fwd": (c_int, [_BfL, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p]),
    "tdn_bfp_scatter_fwd": (c_int, [_BfL, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p]),
    "tdn_bfp_scatter_bwd": (c_int, [_BfL, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p]),
    "tdn_bfp_gather_bwd": (c_int, [_BfL, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p]),
    "tdn_roi_map_levels": (c_int, [c_void_p, c_i64, c_int, c_float, c_void_p, c_void_p]),
    "tdn_roi_align_fwd": (c_int, [_RoL, c_int, c_int, c_int, c_void_p, c_i64, _RoC, c_void_p, c_void_p]),
    "tdn_roi_align_bwd_workspace": (c_i64, [c_i64]),
    "tdn_roi_align_bwd": (c_int, [_RoL, c_int, c_int, c_int, c_void_p, c_i64, _RoC, c_void_p, c_void_p, c_i64,
                                  c_void_p]),
    "tdn_rois_from_proposals": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "tdn_deform_workspace_bytes": (c_i64, [c_int] * 6),
    "tdn_deform_sample": (c_int, [_DfD, c_void_p, c_void_p]),
    "tdn_pack_deform_weight": (c_int, [c_void_p, c_i64, c_i64, c_i64, c_i64, c_int, c_int, c_void_p, c_void_p, c_int,
                                       c_void_p]),
    "tdn_deform_coord_grad": (c_int, [_DfD, c_void_p, c_void_p, c_void_p, c_void_p]),
    "tdn_deform_input_grad": (c_int, [_DfD, c_void_p, c_void_p, c_void_p, c_i64, c_void_p]),
    "tdn_carafe_forward": (c_int, [_CfD, c_void_p, c_void_p]),
    "tdn_carafe_feature_grad": (c_int, [_CfD, c_void_p, c_void_p, c_void_p]),
    "tdn_carafe_mask_grad": (c_int, [_CfD, c_void_p, c_void_p, c_void_p]),
    "tdn_pack_gconv_weight": (c_int, [c_void_p, c_i64, c_i64, c_i64, c_i64, c_int, c_int, c_int, c_int, c_void_p,
                                      c_void_p, c_void_p, c_int, c_void_p]),
    "tdn_bottleneck_supported": (c_int, [c_int] * 5),
    "tdn_bottleneck_fwd": (c_int, [_BA, c_int, c_void_p]),
    "tdn_bottleneck_dgrad": (c_int, [_BA, c_int, c_void_p]),
    "tdn_bottleneck_head_supported": (c_int, [c_int] * 6),
    "tdn_bottleneck_head_fwd": (c_int, [_BHA, c_int, c_void_p]),
    "tdn_bottleneck_head_dgrad": (c_int, [_BHA, c_int, c_void_p]),
    "tdn_gconv2d_fwd": (c_int, [c_void_p] * 3 + [c_int] * 8 + [_EP, c_int, c_void_p]),
    "tdn_gconv2d_dgrad": (c_int, [c_void_p] * 3 + [c_int] * 8 + [_EP, c_int, c_void_p]),
    "tdn_gconv2d_wgrad_workspace": (c_i64, [c_int] * 8),
    "tdn_gconv2d_wgrad": (c_int, [c_void_p] * 9 + [c_float] + [c_int] * 8 + [c_void_p, c_i64, c_int, c_void_p]),
    "tdn_gn_workspace": (c_i64, [c_int] * 5),
    "tdn_gn_fwd": (c_int, [c_void_p] * 3 + [c_int] * 5 + [c_float, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p,
                           c_i64, c_int, c_void_p]),
    "tdn_gn_bwd": (c_int, [c_void_p] * 4 + [c_int] * 5 + [c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_i64,
                           c_int, c_void_p]),
    "tdn_bn_train_fwd": (c_int, [c_void_p] * 5 + [c_float] + [c_int] * 4 + [c_float, c_void_p, c_int, c_int, c_void_p,
                                 c_void_p, c_void_p, c_i64, c_int, c_void_p]),
    "tdn_bn_train_bwd": (c_int, [c_void_p] * 4 + [c_int] * 4 + [c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_i64,
                                 c_int, c_void_p]),
    "tdn_collate_images": (c_int, [ctypes.POINTER(c_void_p), ctypes.POINTER(ctypes.c_int32),
                                   ctypes.POINTER(ctypes.c_uint8), c_int, c_int, ctypes.POINTER(c_float),
                                   ctypes.POINTER(c_float), c_int, c_int, c_void_p, c_int, c_int, c_void_p]),
    "tdn_plan_begin": (c_int, []),
    "tdn_plan_end": (c_void_p, []),
    "tdn_plan_event_record": (c_int, [c_void_p]),
    "tdn_plan_stream_wait": (c_int, [c_void_p, c_int]),
    "tdn_plan_run": (c_int, [c_void_p]),
    "tdn_plan_stats": (c_int, [c_void_p, ctypes.POINTER(ctypes.c_int32)]),
    "tdn_plan_free": (c_int, [c_void_p]),
    "tdn_conv2d_plan": (c_int, [c_int] * 9 + [ctypes.POINTER(ctypes.c_int32)]),
}

_lib = None


def load():
    """Load libtdn.so (once) and attach prototypes. Raises RuntimeError if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "torch_detection_amd: native library %s is missing. Build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` or `make -C torch_detection_amd/csrc`. "
            "There is no CPU / eager fallback for this path." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing -> loud
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().tdn_last_error()
        raise RuntimeError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else "?"))


def ws_bytes(nbytes, what):
    """The answer of a ``*_workspace*()`` query of the detection heads: a negative one is a refusal (ValueError) whose
    reason the library left in ``tdn_last_error``."""
    if nbytes < 0:
        msg = load().tdn_last_error()
        raise ValueError("%s: %s" % (what, msg.decode() if msg else "?"))
    return nbytes


def size_word(out, i):
    """A 64-bit size of a plan record: its low 31 bits in word ``i``, the rest in word ``i + 1``."""
    return out[i] + (out[i + 1] << 31)


_GEMM128_PLAN = ("bm", "bn", "bk", "tiles_r", "tiles_c", "tiles", "slices", "chunks_per_slice", "chunks", "workgroups",
                 "launches")


def gemm128_plan(pl, query, args, what):
    """Fill ``pl`` from the 16-word record that ``tdn_linear_plan`` / ``tdn_deconv2x2_plan`` (``query``) write for
    ``args`` (csrc/gemm128_core.h, ``write_plan``) and return word 11, the file's own flags.  A refusal is a ValueError."""
    out = (ctypes.c_int32 * 16)()
    if query(*[int(a) for a in args], out) != 0:
        ws_bytes(-1, what)
    for name, v in zip(_GEMM128_PLAN, out):
        setattr(pl, name, v)
    pl.slab_bytes, pl.workspace_bytes = size_word(out, 12), size_word(out, 14)
    return out[11]


_tls = threading.local()


def stream_ptr():
    """Raw hipStream_t the kernels are enqueued on: PyTorch's current stream, or the stream set by
    ``use_stream`` for this thread (the weight-gradient side stream of functional.py)."""
    ov = getattr(_tls, "stream", None)
    if ov is not None:
        return ov
    return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())


def set_stream_override(raw_stream):
    """Route this thread's kernel launches to ``raw_stream`` (int) until reset with ``None``.  Cheaper than
    ``with torch.cuda.stream(...)`` (no allocator / current-stream switching); allocations stay on the current
    PyTorch stream, so callers must order memory reuse themselves (functional._side_refs)."""
    prev = getattr(_tls, "stream", None)
    _tls.stream = raw_stream
    return prev
