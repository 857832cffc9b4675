"""torch_detection_amd — MI355X-native ResNet/FPN + box-op hot path behind the Torch_Detection registry.

Drop-in surface (same names as the reference's ``models`` package): ``BACKBONES``, ``NECKS``, ``ResNet``,
``FPN``, ``PAFPN``, ``ConvModule``, the conv/norm builders and init helpers, plus the steps either side of it
(``ImageTransforms`` device-side batch staging, box ops, ``bbox_normalize`` / ``bbox_denormalize``,
``bbox2delta`` / ``delta2bbox``, ``batched_nms`` and ``rpn_proposals``, the training targets ``assign_max_iou`` /
``sample_assigned`` / ``anchor_target`` / ``sample_rois`` and the losses that consume them (``rpn_loss`` /
``anchor_head_loss`` / ``bbox_head_loss``), then ``rois_from_proposals``, ``roi_align``,
``map_roi_levels`` and ``SingleRoIExtractor``, the test-time detections ``bbox_head_detections`` /
``multiclass_nms``, and the mask branch ``pack_polygons`` / ``mask_target`` / ``mask_head_loss`` /
``rois_from_detections`` / ``mask_head_masks``, the fused optimizer step ``SGD``, and the
fully connected layers ``linear`` / ``BBoxHead`` between ``roi_align`` and the box losses, and the 2x2 stride-2 transposed
conv ``conv_transpose2x2`` / ``FCNMaskHead`` between ``roi_align`` and the mask loss, and ``RPNHead`` between ``FPN`` and
``rpn_loss`` / ``rpn_proposals``, and the single-stage path ``RetinaHead`` between ``FPN`` and ``anchor_target_all`` /
``anchor_head_loss`` / ``anchor_head_detections``, and ``FCOSHead`` with the operations around it: ``fcos_points`` /
``fcos_target`` / ``fcos_loss`` / ``fcos_detections``, and deformable convolution ``deform_conv2d`` with the modules
``DeformConv`` / ``ModulatedDeformConv`` / ``DeformConvPack`` / ``ModulatedDeformConvPack``, and Cascade R-CNN's
``refine_bboxes`` / ``cascade_detections`` / ``CascadeRoIHead``, and Libra R-CNN's ``BFP`` neck,
``sample_assigned_iou_balanced`` / ``sample_rois(neg_sampler='iou_balanced')`` and ``bbox_head_loss(reg_loss='balanced_l1')``,
and Mask Scoring R-CNN's ``MaskIoUHead`` with ``mask_iou_stem`` / ``mask_iou_target`` / ``mask_iou_loss`` / ``mask_scores``, and CARAFE upsampling: the ``carafe`` op, ``CARAFEPack`` and the ``FPN_CARAFE`` neck, and the gradient-harmonised losses ``ghm_head_loss`` / ``GHMC`` / ``GHMR`` that
``RetinaHead(loss_cls=..., loss_bbox=...)`` trains with, and the Guided Anchoring operations ``ga_loc_target`` /
``ga_shape_target`` / ``ga_loss`` / ``guided_anchors`` / ``ga_rpn_proposals``).  Everything computes through libtdn.so
(hand-written gfx950 HIP kernels, C ABI in include/tdn.h); there is no CPU or eager fallback.
"""
__version__ = "0.1.0"

from .registry import BACKBONES, HEADS, NECKS, Registry  # noqa: F401
from .layers import (ConvModule, Scale, conv1x1_group, conv3x3_group, conv7x7_group, get_group_gn,  # noqa: F401
                     norm_layer)
from .inits import (bias_init_with_prob, constant_init, kaiming_init, normal_init, uniform_init,  # noqa: F401
                    xavier_init)
from .checkpoint import load_checkpoint, load_state_dict, save_checkpoint  # noqa: F401
from .backbone import (BasicBlock, Bottleneck, ResNet, ResNeXt, ResNeXtBasicBlock,  # noqa: F401
                       ResNeXtBottleneck)
from .necks import BFP, FPN, FPN_CARAFE, PAFPN  # noqa: F401
from .staging import ImageTransforms, StagedImages  # noqa: F401
from .graph import GraphedStep, PreparedStep  # noqa: F401
from .functional import invalidate_packed  # noqa: F401
from .box import (AnchorGenerator, anchor_pyramid, batched_nms, bbox2delta, bbox_denormalize,  # noqa: F401
                  bbox_normalize, bbox_overlaps, delta2bbox, nms, nms_mask, rpn_proposals)
from .target import (anchor_target, assign_max_iou, sample_assigned, sample_assigned_iou_balanced,  # noqa: F401
                     sample_rois)
from .losses import (AnchorHeadLossFunction, BalancedBBoxHeadLossFunction, BBoxHeadLossFunction,  # noqa: F401
                     anchor_head_loss, bbox_head_loss, rpn_loss)
from .ghm import GHMC, GHMR, GHMHeadLossFunction, ghm_head_loss  # noqa: F401
from .detect import bbox_head_detections, multiclass_nms  # noqa: F401
from .dense_detect import (anchor_head_detections, anchor_head_detections_plan,  # noqa: F401
                           anchor_target_all)
from .fcos import (FcosLossFunction, fcos_detections, fcos_detections_plan, fcos_loss,  # noqa: F401
                   fcos_points, fcos_target)
from .guided import (GALossFunction, ga_loc_target, ga_loss, ga_rpn_proposals, ga_shape_target,  # noqa: F401
                     guided_anchors)
from .mask import (MaskHeadLossFunction, mask_head_loss, mask_head_masks, mask_target,  # noqa: F401
                   pack_polygons, rois_from_detections)
from .mask_iou import (MaskIoULossFunction, MaskIoUStemFunction, mask_iou_loss, mask_iou_stem,  # noqa: F401
                       mask_iou_target, mask_scores)
from .optim import SGD  # noqa: F401
from .linear import LinearFunction, linear  # noqa: F401
from .deconv import ConvTranspose2x2Function, conv_transpose2x2  # noqa: F401
from .deform import (DeformConv, DeformConvFunction, DeformConvPack, ModulatedDeformConv,  # noqa: F401
                     ModulatedDeformConvPack, deform_conv2d)
from .carafe import CarafeFunction, CARAFEPack, CARAFEPackFunction, carafe  # noqa: F401
from .heads import BBoxHead, FCNMaskHead, FCOSHead, MaskIoUHead, RetinaHead, RPNHead  # noqa: F401
from .roi import (RoIAlignFunction, SingleRoIExtractor, map_roi_levels, roi_align,  # noqa: F401
                  rois_from_proposals)
from .cascade import CascadeRoIHead, cascade_detections, refine_bboxes  # noqa: F401
