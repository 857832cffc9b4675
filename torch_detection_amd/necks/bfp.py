"""Balanced Feature Pyramid — the neck of Libra R-CNN (Pang et al., CVPR 2019), with mmdetection v1's constructor
(``mmdet/models/necks/bfp.py``), placed behind ``FPN`` in a neck list.

``forward`` runs as one autograd node (functional.BFPFunction): one launch gathers all levels at the size of level
``refine_level`` (``adaptive_max_pool2d`` for the finer levels, nearest resize for the others) and averages them, the
refine step runs on the existing conv path, and one launch scatters the result back to every level (nearest resize /
``adaptive_max_pool2d``) and adds the inputs; the backward is the two adjoint launches around the conv's own
(DESIGN.md §4r).  The level sizes need not be 2x apart.

``refine_type`` None and ``'conv'`` are built; ``'non_local'`` needs an attention kernel over the refine level's
positions, forward and backward, that this library does not have: it is refused at construction.
"""
import torch
import torch.nn as nn

from .. import functional as HF
from ..inits import constant_init, xavier_init
from ..layers import ConvModule
from ..registry import NECKS

MAX_LEVELS, MAX_CHANNELS = 8, 1024


def _norm_args(conv_cfg, norm_cfg):
    """mmdetection's ``conv_cfg`` / ``norm_cfg`` -> this project's ``ConvModule`` keywords; ValueError for the rest."""
    if conv_cfg is not None and not (isinstance(conv_cfg, dict) and conv_cfg.get('type', 'Conv') == 'Conv'
                                     and set(conv_cfg) <= {'type'}):
        raise ValueError("conv_cfg must be None or dict(type='Conv'), got %r" % (conv_cfg,))
    if norm_cfg is None:
        return dict(normalize=None, bias=True, use_gn=False)
    if not isinstance(norm_cfg, dict) or norm_cfg.get('type') not in ('BN', 'GN'):
        raise ValueError("norm_cfg must be None, dict(type='BN') or dict(type='GN', num_groups=32), got %r" % (norm_cfg,))
    extra = set(norm_cfg) - {'type', 'num_groups', 'requires_grad'}
    if extra or not norm_cfg.get('requires_grad', True):
        raise ValueError("norm_cfg: %s not supported" % (sorted(extra) or 'requires_grad=False'))
    use_gn = norm_cfg['type'] == 'GN'
    if use_gn and norm_cfg.get('num_groups', 32) != 32:
        raise ValueError("norm_cfg: GroupNorm is built with 32 groups, got num_groups=%r" % (norm_cfg['num_groups'],))
    if not use_gn and 'num_groups' in norm_cfg:
        raise ValueError("norm_cfg: num_groups given for BN")
    return dict(normalize=dict(norm_cfg), bias=False, use_gn=use_gn)      # bias='auto' of mmdetection's ConvModule


@NECKS.register_module
class BFP(nn.Module):

    def __init__(self, in_channels, num_levels, refine_level=2, refine_type=None, conv_cfg=None, norm_cfg=None):
        super(BFP, self).__init__()
        if refine_type == 'non_local':
            raise NotImplementedError("BFP(refine_type='non_local'): the attention kernel over the refine level's "
                                      "positions does not exist in this library; use refine_type=None or 'conv'")
        if refine_type not in (None, 'conv'):
            raise ValueError("refine_type must be None, 'conv' or 'non_local', got %r" % (refine_type,))
        if not isinstance(num_levels, int) or not 1 <= num_levels <= MAX_LEVELS:
            raise ValueError("num_levels must be an int in 1..%d, got %r" % (MAX_LEVELS, num_levels))
        if not isinstance(refine_level, int) or not 0 <= refine_level < num_levels:
            raise ValueError("refine_level must be an int in 0..%d, got %r" % (num_levels - 1, refine_level))
        mult = 64 if refine_type == 'conv' else 8
        if not isinstance(in_channels, int) or not mult <= in_channels <= MAX_CHANNELS or in_channels % mult:
            raise ValueError("in_channels must be a multiple of %d in %d..%d%s, got %r" % (
                mult, mult, MAX_CHANNELS, " with refine_type='conv'" if mult == 64 else "", in_channels))
        kw = _norm_args(conv_cfg, norm_cfg)
        self.in_channels = in_channels
        self.num_levels = num_levels
        self.refine_level = refine_level
        self.refine_type = refine_type
        self.conv_cfg = conv_cfg
        self.norm_cfg = norm_cfg
        if refine_type == 'conv':
            self.refine = ConvModule(in_channels, in_channels, 3, padding=1, activation='relu', **kw)

    def init_weights(self):
        """xavier-uniform convs (bias 0), norm weight 1, as FPN.init_weights."""
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                xavier_init(m, distribution='uniform')
            if isinstance(m, (nn.BatchNorm2d, nn.GroupNorm)):
                constant_init(m, 1)

    def hip_net(self, dtype=None):
        if dtype is None:
            dtype = getattr(self, 'compute_dtype', torch.bfloat16)
        unit = self.refine.hip_unit(dtype) if self.refine_type == 'conv' else None
        return HF.BFPNet(self.num_levels, self.refine_level, unit, dtype)

    def forward(self, inputs):
        assert len(inputs) == self.num_levels
        net = self.hip_net(HF.pick_dtype(self, inputs))
        return HF.BFPFunction.apply(net, *(tuple(inputs) + tuple(net.params())))
