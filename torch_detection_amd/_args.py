"""Argument checks shared by the host wrappers of the detection heads (``ops.py`` from the box ops on,
``target_ops.py``, ``loss_ops.py``, ``detect_ops.py``, ``dense_detect_ops.py``, ``fcos_ops.py``, ``mask_ops.py``, ``cascade_ops.py``, ``mask_iou_ops.py``, ``carafe_ops.py``, ``ghm_ops.py``, ``guided_ops.py``).  Checks only: nothing here
allocates a tensor, calls the library or reads a tensor's contents, so a wrapper built from these stays capturable in a
graph.  Every refusal is a ValueError that names the argument and the requirement.
"""
import ctypes
import math

import torch

from . import _lib

# the element types the head kernels take (include/tdn.h); ops.dtype_code keeps the conv family's two
CODES = {torch.float32: _lib.TDN_F32, torch.bfloat16: _lib.TDN_BF16, torch.float16: _lib.TDN_F16}


def _names(dtypes):
    return " / ".join(str(d).replace("torch.", "") for d in dtypes)


def tensor(t, name, dtype, shape, contiguous=True):
    """``t`` is a tensor of ``dtype`` (one, or a tuple of allowed ones) and ``shape``; returns its shape.  An entry of
    ``shape`` is an int, a tuple of allowed ints, or None / a string for any size (the string is how the message shows
    it).  ``contiguous=False`` admits any strides.  The device is ``on_device``'s business."""
    if isinstance(t, torch.Tensor) and (t.dtype == dtype or (type(dtype) is tuple and t.dtype in dtype)) and \
            t.dim() == len(shape) and (not contiguous or t.is_contiguous()):
        got = t.shape
        for n, s in zip(got, shape):                # a plain loop: this runs for every operand of every call
            if n != s and (type(s) is int or (type(s) is tuple and n not in s)):
                break
        else:
            return got
    want = ", ".join("*" if s is None else " or ".join(map(str, s)) if isinstance(s, tuple) else str(s) for s in shape)
    raise ValueError("%s must be a %s%s (%s%s) tensor, got %s" % (
        name, "contiguous " if contiguous else "", _names(dtype if isinstance(dtype, tuple) else (dtype,)), want,
        "," if len(shape) == 1 else "",
        "%s %s" % (_names([t.dtype]), tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__))


def number(v, name, positive=False):
    """A finite Python number (no tensor, tuple or list) as a float; ``positive``: and > 0."""
    if torch.is_tensor(v) or isinstance(v, (tuple, list)):
        raise ValueError("%s must be a number" % name)
    v = float(v)
    if not math.isfinite(v) or (positive and v <= 0):
        raise ValueError("%s must be finite%s, got %r" % (name, " and > 0" if positive else "", v))
    return v


def integer(v, name, lo, hi=None):
    """``number`` as an int within lo..hi (no upper end: hi=None)."""
    v = int(number(v, name))
    if v < lo or (hi is not None and v > hi):
        raise ValueError("%s must be %s, got %d" % (name, ">= %d" % lo if hi is None else "in %d..%d" % (lo, hi), v))
    return v


def f4(vals, name):
    """Four finite floats (means / stds) as the ``float[4]`` the library takes."""
    try:
        vals = [float(v) for v in vals]
    except TypeError:
        vals = []
    if len(vals) != 4 or not all(math.isfinite(v) for v in vals):
        raise ValueError("%s must have 4 finite entries" % name)
    return (ctypes.c_float * 4)(*vals)


SOFT_METHODS = {"naive": _lib.SOFT_NAIVE, "linear": _lib.SOFT_LINEAR, "gaussian": _lib.SOFT_GAUSSIAN}
_NMS_KEYS = {"nms": ("type", "iou_thr"), "soft_nms": ("type", "iou_thr", "min_score", "method", "sigma")}


def nms_config(nms, nms_thr, default_thr=0.5):
    """The ``nms`` / ``nms_thr`` pair of the test-time detections -> ``(nms_thr, soft)``.  ``nms=None``:
    ``nms_thr`` as given and ``soft=None``, the greedy path; ``dict(type='nms', iou_thr=t)``: the same with ``t``;
    ``dict(type='soft_nms', iou_thr=0.5, min_score=0.001, method='linear', sigma=0.5)`` (mmdetection's defaults):
    ``soft`` is the ``tdn_soft_nms_config`` of the soft path.  Giving ``nms`` and a ``nms_thr`` other than the default
    is refused, as is every value the library would refuse."""
    if nms is None:
        return number(nms_thr, "nms_thr"), None
    if not isinstance(nms, dict):
        raise ValueError("nms must be None or a dict like dict(type='soft_nms', iou_thr=0.5), got %s" % type(nms).__name__)
    if number(nms_thr, "nms_thr") != default_thr:
        raise ValueError("give the threshold either as nms_thr or in nms['iou_thr'], not both (nms_thr=%r)" % (nms_thr,))
    kind = nms.get("type")
    if kind not in _NMS_KEYS:
        raise ValueError("nms: unknown type %r (one of 'nms', 'soft_nms')" % (kind,))
    extra = sorted(k for k in nms if k not in _NMS_KEYS[kind])
    if extra:
        raise ValueError("nms: unknown key %s for type %r (it takes %s)" % (", ".join(map(repr, extra)), kind,
                                                                            ", ".join(_NMS_KEYS[kind])))
    iou_thr = number(nms.get("iou_thr", 0.5), "nms['iou_thr']")
    if kind == "nms":
        return iou_thr, None
    method = nms.get("method", "linear")
    if not isinstance(method, str) or method not in SOFT_METHODS:
        raise ValueError("nms: method %r is not one of 'linear', 'gaussian', 'naive'" % (method,))
    soft = _lib.SoftNmsConfig()
    soft.method, soft.iou_thr = SOFT_METHODS[method], iou_thr
    soft.sigma = number(nms.get("sigma", 0.5), "nms['sigma']")
    soft.min_score = number(nms.get("min_score", 0.001), "nms['min_score']")
    for key in ("iou_thr", "min_score"):            # finite as the float32 the kernel reads, too
        if not math.isfinite(getattr(soft, key)):
            raise ValueError("nms[%r] must be finite, got %r" % (key, nms.get(key)))
    if not _lib.SOFT_SIGMA_MIN <= soft.sigma <= _lib.SOFT_SIGMA_MAX:
        raise ValueError("nms['sigma'] must lie in [1/64, 64], got %r" % (nms.get("sigma"),))
    if soft.min_score < 0:
        raise ValueError("nms['min_score'] must be >= 0, got %r" % (nms.get("min_score"),))
    return iou_thr, soft


def batch(B):
    """The batch limit of every head entry point (``tdn_check_batch``)."""
    if not 1 <= B <= 64:
        raise ValueError("batch size: the number of images must be in 1..64, got %d" % B)
    return B


def on_device(named):
    """Every (name, tensor) pair that is not None is on the current CUDA device.  A wrapper calls this last, so that
    what it refuses about shapes, dtypes and limits needs no GPU."""
    cur = None
    for name, t in named:
        if t is not None:
            if not t.is_cuda:
                raise ValueError("%s must be a CUDA tensor" % name)
            if cur is None:
                cur = torch.cuda.current_device()
            if t.device.index != cur:
                from .ops import _chk_dev          # raises; imported here because ops.py imports this module
                _chk_dev(t, name)
