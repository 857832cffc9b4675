from .bfp import BFP
from .fpn import FPN
from .pafpn import PAFPN

__all__ = ['BFP', 'FPN', 'PAFPN']
