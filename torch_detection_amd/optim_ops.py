"""Host wrappers of the fused SGD step (csrc/optim.hip), written in the vocabulary of ``_args.py``
(DESIGN.md §5e): every dtype, layout and limit is checked here, before any launch (ValueError that names the argument) —
dtypes and layouts first, so that those refusals need no GPU, the device last.  Everything the step touches on the
device — the state arrays, the momentum buffers, the descriptor table and the workspace — is allocated HERE, once, by
``sgd_state`` / ``sgd_momentum`` / ``sgd_upload``; ``sgd_step`` itself allocates nothing and never synchronises, so it
can be captured in a graph and recorded by a launch plan.

Like the other ``*_ops`` modules this lives beside ``ops.py`` rather than in it; ``tests/test_gpu_optim.py`` puts THIS
module under the guard of ``tests/guard_util.py``.
"""
import ctypes

import torch

from . import _lib
from ._args import integer, number, on_device, tensor
from .ops import _aligned_ws, _ptr, _workspace  # noqa: F401  (_workspace: swapped by the guard)


def _dense(t):
    """``t``'s dims of size > 1, sorted by stride, tile one block of ``t.numel()`` elements (no gaps, no overlap)."""
    want = 1
    for st, n in sorted((st, n) for st, n in zip(t.stride(), t.shape) if n > 1):
        if st != want:
            return False
        want *= n
    return True


def _operand(t, name, shape=None):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.is_sparse:
        raise ValueError("%s must be a dense float32 tensor, got %s" % (
            name, "%s %s" % (str(t.dtype).replace("torch.", ""), tuple(t.shape)) if torch.is_tensor(t)
            else type(t).__name__))
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError("%s must have the parameter's shape %s, got %s" % (name, tuple(shape), tuple(t.shape)))
    if t.numel() < 1 or t.numel() >= 1 << 31:
        raise ValueError("%s must hold 1..2^31-1 elements, got %d" % (name, t.numel()))
    if not _dense(t):
        raise ValueError("%s must be a dense, non-overlapping tensor (a permutation of a contiguous one), got shape %s "
                         "strides %s" % (name, tuple(t.shape), tuple(t.stride())))


def sgd_item(p, g, buf, group, name="p"):
    """One parameter of a step (``tdn_sgd_item``): ``p`` and its gradient ``g`` of the same shape, each dense in its own
    layout, ``buf`` the momentum buffer with ``p``'s strides or None.  The tensors are raw pointers from here on: the
    caller keeps them alive."""
    _operand(p, name)
    _operand(g, name + ".grad", p.shape)
    if buf is not None:
        _operand(buf, name + "'s momentum buffer", p.shape)
        if any(n > 1 and a != b for n, a, b in zip(p.shape, p.stride(), buf.stride())):
            raise ValueError("%s's momentum buffer must have the parameter's strides" % name)
    group = integer(group, "group", 0, _lib.SGD_MAX_GROUPS - 1)
    shape, ps, gs = tuple(p.shape), p.stride(), g.stride()
    if len(shape) > 4:
        if any(n > 1 and a != b for n, a, b in zip(shape, ps, gs)):
            raise ValueError("%s has %d dims: more than 4 are taken only when the gradient has the parameter's strides"
                             % (name, len(shape)))
        shape, ps, gs = (p.numel(),), (1,), (1,)             # one layout: the memory is one run of numel elements
    on_device([(name, p), (name + ".grad", g), (name + "'s momentum buffer", buf)])
    pad = 4 - len(shape)
    it = _lib.SgdItem()
    it.p, it.g, it.buf = p.data_ptr(), g.data_ptr(), buf.data_ptr() if buf is not None else None
    it.shape = (ctypes.c_int64 * 4)(*((1,) * pad + tuple(shape)))
    it.p_stride = (ctypes.c_int64 * 4)(*((0,) * pad + tuple(ps)))
    it.g_stride = (ctypes.c_int64 * 4)(*((0,) * pad + tuple(gs)))
    it.group = group
    return it


class SgdPlan(object):
    """What ``tdn_sgd_plan`` answered for one item list (host side)."""
    __slots__ = ("plan8", "table_host", "paths", "n", "n_groups", "table_bytes", "workspace_bytes", "norm_wgs",
                 "update_wgs", "norm_chunks", "update_chunks")


def sgd_plan(items, n_groups):
    """Host only: sizes, workgroup counts, the access path of every item and the descriptor table (a CPU uint8 tensor)
    for a list of ``sgd_item``s.  Refusals of the library (overlapping or non-dense tensors, limits) are ValueErrors."""
    n = len(items)
    if not 1 <= n <= _lib.SGD_MAX_ITEMS:
        raise ValueError("items: %d items (1..%d)" % (n, _lib.SGD_MAX_ITEMS))
    n_groups = integer(n_groups, "n_groups", 1, _lib.SGD_MAX_GROUPS)
    arr = (_lib.SgdItem * n)(*items)
    lib = _lib.load()
    pl = SgdPlan()
    pl.plan8 = (ctypes.c_int64 * 8)()
    paths = (ctypes.c_int32 * n)()
    if lib.tdn_sgd_plan(arr, n, n_groups, pl.plan8, None, 0, paths) != 0:
        _lib.ws_bytes(-1, "sgd_plan")
    pl.table_host = torch.zeros(pl.plan8[0] // 16 * 2, dtype=torch.int64).view(torch.uint8)   # 16-byte aligned
    if lib.tdn_sgd_plan(arr, n, n_groups, pl.plan8, ctypes.c_void_p(pl.table_host.data_ptr()),
                        pl.table_host.numel(), paths) != 0:
        _lib.ws_bytes(-1, "sgd_plan")
    pl.paths = list(paths)
    (pl.table_bytes, pl.workspace_bytes, pl.norm_wgs, pl.update_wgs, pl.norm_chunks, pl.update_chunks, pl.n,
     pl.n_groups) = list(pl.plan8)
    return pl


def sgd_state(device, scale=1.0):
    """-> (fstate float32 [SGD_F_COUNT], istate int32 [SGD_I_COUNT]) on ``device``: zeros, fstate[SGD_F_SCALE] = scale."""
    scale = number(scale, "scale", positive=True)
    fstate = torch.zeros(_lib.SGD_F_COUNT, dtype=torch.float32, device=device)
    istate = torch.zeros(_lib.SGD_I_COUNT, dtype=torch.int32, device=device)
    fstate[_lib.SGD_F_SCALE:_lib.SGD_F_SCALE + 1].fill_(scale)
    return fstate, istate


def sgd_momentum(numels, device):
    """-> (flat float32 zeros, offsets): one allocation for the momentum buffers of parameters of ``numels`` elements,
    every slot from a 64-element (256-byte) boundary."""
    offsets, off = [], 0
    for n in numels:
        offsets.append(off)
        off += (integer(n, "numels", 1) + 63) // 64 * 64
    return torch.zeros(max(off, 64), dtype=torch.float32, device=device), offsets


def sgd_upload(plan, device):
    """The device side of a plan: -> (table, table pointer, workspace, workspace pointer), both 256-byte aligned; the
    table is copied here, once."""
    if not isinstance(plan, SgdPlan):
        raise ValueError("plan must be what sgd_plan returned")
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError("device must be a CUDA device")
    table, tp = _aligned_ws(plan.table_bytes, device)
    off = tp.value - table.data_ptr()
    table[off:off + plan.table_bytes].copy_(plan.table_host[:plan.table_bytes])
    ws, wp = _aligned_ws(plan.workspace_bytes, device)
    return table, tp, ws, wp


def sgd_step(plan, table_ptr, hyper, fstate, istate, ws_ptr, nesterov=False, skip_nonfinite=True, dynamic=False,
             max_norm=0.0, growth=2.0, backoff=0.5, interval=2000):
    """The two launches of ``tdn_sgd_step`` on the current stream.  ``hyper`` float32 (n_groups, 3) = lr, weight decay,
    momentum; ``table_ptr`` / ``ws_ptr`` from ``sgd_upload`` of the same plan.  Returns nothing: the results are in
    ``fstate`` / ``istate`` (device)."""
    tensor(hyper, "hyper", torch.float32, (plan.n_groups, 3))
    tensor(fstate, "fstate", torch.float32, (_lib.SGD_F_COUNT,))
    tensor(istate, "istate", torch.int32, (_lib.SGD_I_COUNT,))
    on_device([("hyper", hyper), ("fstate", fstate), ("istate", istate)])
    flags = (_lib.SGD_NESTEROV if nesterov else 0) | (_lib.SGD_SKIP_NONFINITE if skip_nonfinite else 0) | \
        (_lib.SGD_DYNAMIC_SCALE if dynamic else 0)
    _lib.check(_lib.load().tdn_sgd_step(table_ptr, plan.plan8, _ptr(hyper), _ptr(fstate), _ptr(istate), ws_ptr,
                                        plan.workspace_bytes, flags, max_norm, growth, backoff, interval,
                                        _lib.stream_ptr()), "tdn_sgd_step")
