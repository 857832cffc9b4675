"""FPN_CARAFE — the feature pyramid of CARAFE (Wang et al., ICCV 2019), mmdetection v1.1's ``necks/fpn_carafe.py`` with
``upsample_cfg=dict(type='carafe', ...)``: the top-down pathway upsamples with a ``CARAFEPack`` per level instead of a
nearest resize, and the extra levels (stride-2 3x3 convs) are part of that pathway.

``forward``: the laterals on the existing conv path (``ConvModule``); top-down, from the coarsest level,

    laterals[i - 1] = laterals[i - 1] + upsample_modules[i - 1](laterals[i])[:, :, :H(i - 1), :W(i - 1)]

as ONE reassembly launch per level (the crop and the add are the kernel's ``out_size`` / ``addend``); then the
3x3 output convs.  State-dict keys follow ``FPN``'s here (``lateral_convs.{i}.conv.*``, ``fpn_convs.{i}.conv.*``) plus
``upsample_modules.{i}.channel_compressor.*`` / ``.content_encoder.*``.

Built: ``norm_cfg=None``, ``activation=None``, the default ``order`` and ``upsample_cfg['type'] == 'carafe'`` with
``encoder_kernel=3``, ``encoder_dilation=1``; everything else raises ``NotImplementedError`` at construction.
"""
import torch.nn as nn

from ..carafe import CARAFEPack
from ..inits import xavier_init
from ..layers import ConvModule
from ..registry import NECKS

_DEFAULT_UPSAMPLE = dict(type='carafe', up_kernel=5, up_group=1, encoder_kernel=3, encoder_dilation=1)


@NECKS.register_module
class FPN_CARAFE(nn.Module):

    def __init__(self, in_channels, out_channels, num_outs, start_level=0, end_level=-1, norm_cfg=None, activation=None,
                 order=('conv', 'norm', 'act'),
                 upsample_cfg=dict(type='carafe', up_kernel=5, up_group=1, encoder_kernel=3, encoder_dilation=1)):
        super(FPN_CARAFE, self).__init__()
        if not isinstance(in_channels, (list, tuple)) or not in_channels:
            raise ValueError("in_channels must be a non-empty list, got %r" % (in_channels,))
        if norm_cfg is not None or activation is not None:
            raise NotImplementedError("FPN_CARAFE: norm_cfg / activation other than None are not built")
        if tuple(order) != ('conv', 'norm', 'act'):
            raise NotImplementedError("FPN_CARAFE: order must be ('conv', 'norm', 'act'), got %r" % (order,))
        if not isinstance(upsample_cfg, dict):
            raise ValueError("upsample_cfg must be a dict, got %r" % (upsample_cfg,))
        cfg = dict(upsample_cfg)
        if cfg.get('type') != 'carafe':
            raise NotImplementedError("FPN_CARAFE: upsample_cfg['type'] must be 'carafe', got %r" % (cfg.get('type'),))
        extra = set(cfg) - set(_DEFAULT_UPSAMPLE) - {'compressed_channels'}
        if extra:
            raise ValueError("upsample_cfg: unknown keys %s" % sorted(extra))
        cfg.pop('type')
        self.in_channels = list(in_channels)
        self.out_channels = out_channels
        self.num_ins = len(in_channels)
        self.num_outs = num_outs
        self.upsample_cfg = dict(cfg, type='carafe')
        if end_level == -1:
            self.backbone_end_level = self.num_ins
        else:
            if not start_level < end_level <= self.num_ins:
                raise ValueError("end_level must be -1 or in %d..%d, got %r" % (start_level + 1, self.num_ins, end_level))
            self.backbone_end_level = end_level
        if not 0 <= start_level < self.backbone_end_level:
            raise ValueError("start_level must be in 0..%d, got %r" % (self.backbone_end_level - 1, start_level))
        self.start_level, self.end_level = start_level, end_level
        levels = self.backbone_end_level - start_level
        extra_levels = num_outs - levels
        if extra_levels < 0:
            raise ValueError("num_outs = %r is below the %d backbone levels used" % (num_outs, levels))

        self.lateral_convs = nn.ModuleList()
        self.fpn_convs = nn.ModuleList()
        self.upsample_modules = nn.ModuleList()
        for i in range(start_level, self.backbone_end_level):
            self.lateral_convs.append(ConvModule(in_channels[i], out_channels, kernel_size=1))
            self.fpn_convs.append(ConvModule(out_channels, out_channels, kernel_size=3, padding=1))
        for j in range(extra_levels):
            cin = in_channels[self.backbone_end_level - 1] if j == 0 else out_channels
            self.lateral_convs.append(ConvModule(cin, out_channels, kernel_size=3, stride=2, padding=1))
            self.fpn_convs.append(ConvModule(out_channels, out_channels, kernel_size=3, padding=1))
        for _ in range(levels + extra_levels - 1):
            self.upsample_modules.append(CARAFEPack(out_channels, 2, **cfg))

    def init_weights(self):
        """xavier-uniform convs (bias 0); then every ``CARAFEPack``'s own initialisation (mmdetection's order)."""
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                xavier_init(m, distribution='uniform')
        for m in self.modules():
            if isinstance(m, CARAFEPack):
                m.init_weights()

    def forward(self, inputs):
        if len(inputs) != len(self.in_channels):
            raise ValueError("expected %d inputs, got %d" % (len(self.in_channels), len(inputs)))
        levels = self.backbone_end_level - self.start_level
        laterals = []
        for i, conv in enumerate(self.lateral_convs):
            if i < levels:
                src = inputs[self.start_level + i]
            elif i == levels:
                src = inputs[self.backbone_end_level - 1]
            else:
                src = laterals[-1]
            laterals.append(conv(src))
        for i in range(len(laterals) - 1, 0, -1):
            lo, hi = laterals[i - 1], laterals[i]
            if 2 * hi.shape[2] < lo.shape[2] or 2 * hi.shape[3] < lo.shape[3]:
                raise ValueError("level %d: the upsampled map %d x %d is smaller than the lateral %d x %d" % (
                    i, 2 * hi.shape[2], 2 * hi.shape[3], lo.shape[2], lo.shape[3]))
            laterals[i - 1] = self.upsample_modules[i - 1](hi, out_size=tuple(lo.shape[2:]), addend=lo)
        return tuple(conv(lat) for conv, lat in zip(self.fpn_convs, laterals))
