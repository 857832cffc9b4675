from .bfp import BFP
from .fpn import FPN
from .fpn_carafe import FPN_CARAFE
from .pafpn import PAFPN

__all__ = ['BFP', 'FPN', 'FPN_CARAFE', 'PAFPN']
