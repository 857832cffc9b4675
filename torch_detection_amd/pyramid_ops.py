"""Host wrappers of the shared-weight 3x3 conv over a pyramid (csrc/pyramid_conv.hip), written in the
vocabulary of ``_args.py``: every dtype, layout and limit is checked here, before any launch (ValueError
that names the argument) — dtypes, layouts and sizes first, so that those refusals need no GPU, the device last.

A pyramid is a list of 1..8 levels of one batch size.  The inputs ``xs[l]`` are logical (B, Cin, H_l, W_l) 16-bit tensors
in channels_last MEMORY (``t.permute(0, 2, 3, 1)`` is contiguous), Cin a multiple of 64 in 64..512; so are the outputs
``ys[l]`` (B, Cout, H_l, W_l) with ANY Cout in 1..1024 — exactly Cout channels per pixel, no padding —, their cotangents,
and the input gradients ``dxs[l]``.  A cotangent that is not channels_last memory of the compute dtype is brought there by
ONE copy (``dense_ops.cotangents``).  The packed weights are ``w_fwd`` (Cp, 3, 3, Cin) and ``w_dgrad`` (Cin, 3, 3, Cp) of
``pack_pyramid_weight``, Cp = Cout rounded up to 64 (the kernels' column tile), the pad rows / columns zero; ``w_dgrad``
holds the taps mirrored.  Parameters, biases and their gradients are float32.

Like the other ``*_ops`` modules this lives beside ``ops.py`` rather than in it; ``tests/test_gpu_pyramid_conv.py`` puts
THIS module under the guard of ``tests/guard_util.py``.
"""
import ctypes

import torch

from . import _lib
from ._args import integer, number, on_device, tensor
from .deconv_ops import _nhwc
from .dense_ops import _levels, _same_count, cotangents
from .ops import BF16, F16, _aligned_ws, _ptr, _workspace, dtype_code  # noqa: F401  (_workspace: swapped by the guard)

F32 = torch.float32
_16 = (BF16, F16)
FWD, DGRAD, WGRAD = 0, 1, 2
MAX_LEVELS, MAX_CIN, MAX_COUT, MAX_ROWS = _lib.PYR_MAX_LEVELS, 512, 1024, (1 << 31) - 1
COL_TILE = 64


def _pad(n, to=COL_TILE):
    return (n + to - 1) // to * to


def _cin(C, name="Cin"):
    C = integer(C, name, 64, MAX_CIN)
    if C % 64:
        raise ValueError("%s must be a multiple of 64 in 64..%d, got %d" % (name, MAX_CIN, C))
    return C


def _cout(C, name="Cout"):
    return integer(C, name, 1, MAX_COUT)


def _inputs(xs, name="xs"):
    """The Cin-channel maps: -> (list, dtype, B, Cin, [(H, W)]).  One dtype, one batch size, one channel count."""
    xs = _levels(xs, name)
    B, C, H, W = _nhwc(xs[0], "%s[0]" % name, _16, ("B", "Cin", "H", "W"))
    C = _cin(C)
    dtype = xs[0].dtype
    sizes = []
    for l, x in enumerate(xs):
        _, _, H, W = _nhwc(x, "%s[%d]" % (name, l), dtype, (B, C, "H", "W"))
        if H < 1 or W < 1:
            raise ValueError("%s[%d]: H and W must be positive, got %d x %d" % (name, l, H, W))
        integer(B * H * W, "%s[%d]: B*H*W" % (name, l), 0, MAX_ROWS)
        sizes.append((H, W))
    return xs, dtype, B, C, sizes


def _like(ts, name, dtype, B, C, sizes):
    """Optional per-level maps of the inputs' shape (mask sources, addends): a list with None entries, or None."""
    if ts is None:
        return [None] * len(sizes)
    ts = _same_count(ts, name, len(sizes))
    for l, (t, (H, W)) in enumerate(zip(ts, sizes)):
        if t is not None:
            _nhwc(t, "%s[%d]" % (name, l), dtype, (B, C, H, W))
    return ts


def _hw(sizes):
    return (ctypes.c_int32 * (2 * len(sizes)))(*[v for hw in sizes for v in hw])


def _table(sizes, x=None, y=None, dx=None, mask_src=None, addend=None):
    n = len(sizes)
    arr = (_lib.PyrLevel * n)()
    ptr = lambda ts, l: ts[l].data_ptr() if ts is not None and ts[l] is not None else None
    for l, (H, W) in enumerate(sizes):
        arr[l].x, arr[l].y, arr[l].dx = ptr(x, l), ptr(y, l), ptr(dx, l)
        arr[l].mask_src, arr[l].addend = ptr(mask_src, l), ptr(addend, l)
        arr[l].H, arr[l].W = H, W
    return arr


class PyramidPlan(object):
    """What ``tdn_pyr_plan`` answered (host side)."""
    __slots__ = ("pixels_per_workgroup", "workgroups", "slices", "pixels_per_slice", "launches", "cols_per_workgroup",
                 "Cp", "Kp", "lds_bytes", "col_tiles", "pixel_tiles", "slab_bytes", "workspace_bytes")


def _geometry(B, sizes, min_side=1, max_B=None):
    """(B, [(H, W)]) checked: 1..MAX_LEVELS levels, sides >= ``min_side`` (0: a level may be empty), B in 0..``max_B``.
    Where B is capped (the GroupNorm entry points, which keep H*W in an int of its own) H*W is refused before B*H*W."""
    B = integer(B, "B", 0, max_B)
    if not isinstance(sizes, (list, tuple)) or not 1 <= len(sizes) <= MAX_LEVELS:
        raise ValueError("sizes must be a list of 1..%d (H, W) pairs, got %s" % (
            MAX_LEVELS, len(sizes) if isinstance(sizes, (list, tuple)) else type(sizes).__name__))
    out = []
    for l, hw in enumerate(sizes):
        H, W = integer(hw[0], "sizes[%d][0]" % l, min_side), integer(hw[1], "sizes[%d][1]" % l, min_side)
        if max_B is not None:
            integer(H * W, "sizes[%d]: H*W" % l, 0, MAX_ROWS)
        integer(B * H * W, "sizes[%d]: B*H*W" % l, 0, MAX_ROWS)
        out.append((H, W))
    return B, out


def pyramid_conv_plan(kind, B, sizes, Cin, Cout):
    """Host only: the decomposition of one product (kind FWD / DGRAD / WGRAD) over levels of ``sizes[l]`` = (H_l, W_l)
    and batch size B.  ``col_tiles``: column tiles of a forward / dgrad grid, or the (Cout tile, tap, Cin tile) units of
    one wgrad slice.  Refusals are ValueErrors."""
    if kind not in (FWD, DGRAD, WGRAD):
        raise ValueError("kind must be FWD (0), DGRAD (1) or WGRAD (2), got %r" % (kind,))
    B, sizes = _geometry(B, sizes)
    Cin, Cout = _cin(Cin), _cout(Cout)
    out = (ctypes.c_int32 * 16)()
    if _lib.load().tdn_pyr_plan(int(kind), B, _hw(sizes), len(sizes), Cin, Cout, out) != 0:
        _lib.ws_bytes(-1, "pyramid_conv_plan")
    pl = PyramidPlan()
    (pl.pixels_per_workgroup, pl.workgroups, pl.slices, pl.pixels_per_slice, pl.launches, pl.cols_per_workgroup, pl.Cp,
     pl.Kp, pl.lds_bytes, pl.col_tiles, pl.pixel_tiles) = list(out)[:11]
    pl.slab_bytes, pl.workspace_bytes = _lib.size_word(out, 12), _lib.size_word(out, 14)
    return pl


def pack_pyramid_weight(w, want_dgrad=True, dtype=BF16, out=None):
    """float32 ``w`` (Cout, Cin, 3, 3) of any strides -> (w_fwd (Cp, 3, 3, Cin), w_dgrad (Cin, 3, 3, Cp) or None) in
    ``dtype``, by one launch: ``w_fwd[o, kh, kw, c] = w[o, c, kh, kw]`` and ``w_dgrad[c, th, tw, o] = w[o, c, 2 - th,
    2 - tw]``, each rounded once, zero for ``o >= Cout``.  ``out``: the pair of an earlier call, overwritten in place."""
    if not isinstance(w, torch.Tensor) or w.dim() != 4:
        tensor(w, "w", F32, ("Cout", "Cin", 3, 3), contiguous=False)
    Cout, Cin = _cout(w.shape[0]), _cin(w.shape[1])
    tensor(w, "w", F32, (Cout, Cin, 3, 3), contiguous=False)
    code = dtype_code(dtype)
    Cp = _pad(Cout)
    if out is not None:
        w_fwd, w_dgrad = out
        tensor(w_fwd, "out[0]", dtype, (Cp, 3, 3, Cin))
        if want_dgrad:
            tensor(w_dgrad, "out[1]", dtype, (Cin, 3, 3, Cp))
    on_device([("w", w)] + ([("out[0]", out[0]), ("out[1]", out[1] if want_dgrad else None)] if out else []))
    if out is None:
        w_fwd = torch.empty((Cp, 3, 3, Cin), dtype=dtype, device=w.device)
        w_dgrad = torch.empty((Cin, 3, 3, Cp), dtype=dtype, device=w.device) if want_dgrad else None
    if not want_dgrad:
        w_dgrad = None
    s = w.stride()
    _lib.check(_lib.load().tdn_pack_pyr_weight(_ptr(w), s[0], s[1], s[2], s[3], Cout, Cin, _ptr(w_fwd), _ptr(w_dgrad),
                                               code, _lib.stream_ptr()), "tdn_pack_pyr_weight")
    return w_fwd, w_dgrad


def pyramid_conv_fwd(xs, w_fwd, bias, Cout, relu=False):
    """-> ys: list of (B, Cout, H_l, W_l) tensors in ``xs``'s dtype, channels_last memory, exactly Cout channels per
    pixel: ``y_l = [relu](conv3x3(x_l, w) + bias)`` for all levels in one launch.  ``bias`` (Cout,) float32 or None."""
    xs, dtype, B, Cin, sizes = _inputs(xs)
    Cout = _cout(Cout)
    if bias is not None:
        tensor(bias, "bias", F32, (Cout,))
    tensor(w_fwd, "w_fwd", dtype, (_pad(Cout), 3, 3, Cin))
    on_device([("xs[%d]" % l, x) for l, x in enumerate(xs)] + [("w_fwd", w_fwd), ("bias", bias)])
    ys = [torch.empty((B, H, W, Cout), dtype=dtype, device=xs[0].device) for H, W in sizes]
    arr = _table(sizes, x=xs, y=ys)
    _lib.check(_lib.load().tdn_pyr_conv_fwd(arr, len(xs), B, _ptr(w_fwd), _ptr(bias), Cin, Cout, 1 if relu else 0,
                                            dtype_code(dtype), _lib.stream_ptr()), "tdn_pyr_conv_fwd")
    return [t.permute(0, 3, 1, 2) for t in ys]


def _grads(gs, like, name_like):
    """The cotangents ``gs`` against the Cin-channel maps ``like`` (the inputs, or any maps of their shape)."""
    like, dtype, B, Cin, sizes = _inputs(like, name_like)
    gs = _same_count(gs, "gs", len(like))
    Cout = _cout(gs[0].shape[1] if torch.is_tensor(gs[0]) and gs[0].dim() == 4 else 0)
    gs = cotangents(gs, "gs", dtype, B, Cout, sizes)
    return like, dtype, B, Cin, sizes, Cout, gs


def pyramid_conv_dgrad(gs, w_dgrad, mask_src=None, addend=None):
    """-> dxs: list of (B, Cin, H_l, W_l) tensors, channels_last memory: ``conv3x3^T(g_l, w) [+ addend_l]`` summed in
    fp32 and rounded once, exactly 0 where ``mask_src[l] <= 0``, all levels in one launch.  ``mask_src``: None or the
    list of the ReLU outputs that fed the forward conv; ``addend``: None or a list of maps of the result's shape (entries
    of either list may be None).  The compute dtype and Cin are ``w_dgrad``'s, the map sizes the cotangents', which are
    read where they lie."""
    w = tensor(w_dgrad, "w_dgrad", _16, ("Cin", 3, 3, "Cp"))
    dtype, Cin = w_dgrad.dtype, _cin(w[0])
    gs = _levels(gs, "gs")
    Cout = _cout(gs[0].shape[1] if torch.is_tensor(gs[0]) and gs[0].dim() == 4 else 0)
    if w[3] != _pad(Cout):
        raise ValueError("w_dgrad must be a (%d, 3, 3, %d) tensor for %d-channel cotangents, got %s" % (
            Cin, _pad(Cout), Cout, tuple(w_dgrad.shape)))
    B = gs[0].shape[0]
    sizes = []
    for l, g in enumerate(gs):
        if not torch.is_tensor(g) or g.dim() != 4:
            raise ValueError("gs[%d] must be a 4-D tensor" % l)
        sizes.append((g.shape[2], g.shape[3]))
    B, sizes = _geometry(B, sizes)
    gs = cotangents(gs, "gs", dtype, B, Cout, sizes)
    masks = _like(mask_src, "mask_src", dtype, B, Cin, sizes)
    adds = _like(addend, "addend", dtype, B, Cin, sizes)
    on_device([("gs[%d]" % l, g) for l, g in enumerate(gs)] + [("mask_src[%d]" % l, m) for l, m in enumerate(masks)] +
              [("addend[%d]" % l, a) for l, a in enumerate(adds)] + [("w_dgrad", w_dgrad)])
    dxs = [torch.empty((B, H, W, Cin), dtype=dtype, device=gs[0].device) for H, W in sizes]
    arr = _table(sizes, y=gs, dx=dxs, mask_src=masks, addend=adds)
    _lib.check(_lib.load().tdn_pyr_conv_dgrad(arr, len(gs), B, _ptr(w_dgrad), Cin, Cout, dtype_code(dtype),
                                              _lib.stream_ptr()), "tdn_pyr_conv_dgrad")
    return [t.permute(0, 3, 1, 2) for t in dxs]


def pyramid_conv_wgrad(xs, gs, channels_last=True):
    """-> (dw (Cout, Cin, 3, 3), dbias (Cout,)), float32: the sums over the pixels of all levels of ``g^T x`` per tap and
    of ``g``, cut into slices that depend on the shapes alone and added in slice order (two launches; the same bits on
    every run).  ``channels_last``: dw in channels_last memory (the layout the modules keep these parameters in), else
    contiguous.  An empty batch gives zeros."""
    xs, dtype, B, Cin, sizes, Cout, gs = _grads(gs, xs, "xs")
    on_device([("xs[%d]" % l, x) for l, x in enumerate(xs)] + [("gs[%d]" % l, g) for l, g in enumerate(gs)])
    dev = xs[0].device
    if channels_last:
        dw = torch.empty((Cout, 3, 3, Cin), dtype=F32, device=dev).permute(0, 3, 1, 2)
    else:
        dw = torch.empty((Cout, Cin, 3, 3), dtype=F32, device=dev)
    db = torch.empty((Cout,), dtype=F32, device=dev)
    nbytes = _lib.ws_bytes(_lib.load().tdn_pyr_workspace_bytes(WGRAD, B, _hw(sizes), len(sizes), Cin, Cout),
                           "pyramid workspace")
    ws, wp = _aligned_ws(nbytes, dev) if nbytes else (None, None)
    arr = _table(sizes, x=xs, y=gs)
    s = dw.stride()
    _lib.check(_lib.load().tdn_pyr_conv_wgrad(arr, len(xs), B, _ptr(dw), s[0], s[1], s[2], s[3], _ptr(db), Cin, Cout, wp,
                                              nbytes, dtype_code(dtype), _lib.stream_ptr()), "tdn_pyr_conv_wgrad")
    return dw, db


# ---- GroupNorm (+ ReLU) with shared affine parameters over a pyramid (csrc/pyramid_gn.hip) --------------
GN_FWD, GN_BWD = 0, 1
GN_CHANNELS = (64, 128, 256, 512)
GN_MAX_CPG = 256
GN_MAX_B = 65535 // MAX_LEVELS


def _gn_channels(C, G):
    C = integer(C, "C", 1)
    if C not in GN_CHANNELS:
        raise ValueError("C must be one of %s, got %d" % (", ".join(map(str, GN_CHANNELS)), C))
    G = integer(G, "groups", 1)
    if C % G or C // G > GN_MAX_CPG:
        raise ValueError("groups must divide C = %d into at most %d channels per group, got %d" % (C, GN_MAX_CPG, G))
    return C, G


def _gn_maps(zs, name="zs"):
    """The raw conv outputs: -> (list, dtype, B, C, [(H, W)]).  One dtype, one batch size, one channel count."""
    zs = _levels(zs, name)
    B, C, H, W = _nhwc(zs[0], "%s[0]" % name, _16, ("B", "C", "H", "W"))
    dtype = zs[0].dtype
    sizes = []
    for l, z in enumerate(zs):
        _, _, H, W = _nhwc(z, "%s[%d]" % (name, l), dtype, (B, C, "H", "W"))
        sizes.append((H, W))
    B, sizes = _geometry(B, sizes, 0, GN_MAX_B)
    return zs, dtype, B, C, sizes


def _gn_same(ts, name, dtype, B, C, sizes):
    ts = _same_count(ts, name, len(sizes))
    for l, (t, (H, W)) in enumerate(zip(ts, sizes)):
        _nhwc(t, "%s[%d]" % (name, l), dtype, (B, C, H, W))
    return ts


def _gn_table(sizes, z, y=None, g=None, dz=None):
    arr = (_lib.PyrGnLevel * len(sizes))()
    ptr = lambda ts, l: ts[l].data_ptr() if ts is not None and ts[l].numel() else None
    for l, (H, W) in enumerate(sizes):
        arr[l].z, arr[l].y, arr[l].g, arr[l].dz = ptr(z, l), ptr(y, l), ptr(g, l), ptr(dz, l)
        arr[l].H, arr[l].W = H, W
    return arr


class PyramidGnPlan(object):
    """What ``tdn_pyr_gn_plan`` answered (host side).  ``chunks[l]``: pixel chunks per image of level l (0: the level is
    skipped), ``chunk_pixels[l]``: pixels per chunk, ``workgroups``: of the three launches."""
    __slots__ = ("chunks", "chunk_pixels", "workgroups", "launches", "lanes_per_workgroup", "channels_per_block",
                 "workspace_bytes")


def pyramid_gn_plan(kind, B, sizes, C, groups):
    """Host only: how one GroupNorm product (kind GN_FWD / GN_BWD) over levels of ``sizes[l]`` = (H_l, W_l) and batch
    size B is cut.  Refusals are ValueErrors."""
    if kind not in (GN_FWD, GN_BWD):
        raise ValueError("kind must be GN_FWD (0) or GN_BWD (1), got %r" % (kind,))
    B, sizes = _geometry(B, sizes, 0, GN_MAX_B)
    C, G = _gn_channels(C, groups)
    out = (ctypes.c_int32 * 32)()
    if _lib.load().tdn_pyr_gn_plan(int(kind), B, _hw(sizes), len(sizes), C, G, out) != 0:
        _lib.ws_bytes(-1, "pyramid_gn_plan")
    pl = PyramidGnPlan()
    n = len(sizes)
    pl.chunks, pl.chunk_pixels = list(out)[:n], list(out)[MAX_LEVELS:MAX_LEVELS + n]
    pl.workgroups, pl.launches = tuple(out[16:19]), out[19]
    pl.lanes_per_workgroup, pl.channels_per_block = out[20], out[21]
    pl.workspace_bytes = _lib.size_word(out, 22)
    return pl


def _gn_ws(kind, B, sizes, C, G, dev):
    nbytes = _lib.ws_bytes(_lib.load().tdn_pyr_gn_workspace_bytes(kind, B, _hw(sizes), len(sizes), C, G),
                           "pyramid GroupNorm workspace")
    return (_aligned_ws(nbytes, dev) if nbytes else (None, None)) + (nbytes,)


def pyramid_gn_fwd(zs, gamma, beta, groups, eps=1e-5, relu=True):
    """-> (ys, stats): ``y_l = [relu](GroupNorm(z_l) * gamma + beta)`` for all levels in three launches, the statistics per
    (level, image, group); ``ys[l]`` like ``zs[l]`` (logical (B, C, H_l, W_l), channels_last memory), ``stats``
    (L, B, C, 2) float32 = (mean, rstd) of the channel's group, kept for ``pyramid_gn_bwd``.  ``gamma``, ``beta``: (C,)
    float32, shared by the levels.  A level may be empty."""
    zs, dtype, B, C, sizes = _gn_maps(zs)
    C, G = _gn_channels(C, groups)
    tensor(gamma, "gamma", F32, (C,))
    tensor(beta, "beta", F32, (C,))
    eps = number(eps, "eps", positive=True)
    on_device([("zs[%d]" % l, z) for l, z in enumerate(zs)] + [("gamma", gamma), ("beta", beta)])
    dev = zs[0].device
    ys = [torch.empty((B, H, W, C), dtype=dtype, device=dev) for H, W in sizes]
    stats = torch.empty((len(sizes), B, C, 2), dtype=F32, device=dev)
    ws, wp, nbytes = _gn_ws(GN_FWD, B, sizes, C, G, dev)
    arr = _gn_table(sizes, zs, y=ys)
    _lib.check(_lib.load().tdn_pyr_gn_fwd(arr, len(zs), B, _ptr(gamma), _ptr(beta), C, G, eps, 1 if relu else 0,
                                          _ptr(stats), wp, nbytes, dtype_code(dtype), _lib.stream_ptr()),
               "tdn_pyr_gn_fwd")
    return [t.permute(0, 3, 1, 2) for t in ys], stats


def pyramid_gn_bwd(gs, ys, zs, stats, gamma, groups, relu=True, dgamma=None, dbeta=None, accumulate=False):
    """-> (dzs, dgamma, dbeta) from the UNMASKED cotangents ``gs[l]`` = dL/dy_l: where ``ys[l] <= 0`` (``relu``) the
    cotangent counts as exactly 0, in the sums and in ``dz``; ``ys`` may be None without ``relu``.  ``dgamma`` / ``dbeta``
    (C,) float32 are the sums over all levels and images, added in level order, finest first; given buffers are
    overwritten, or added to with ``accumulate``.  Three launches; the same bits on every run."""
    zs, dtype, B, C, sizes = _gn_maps(zs)
    C, G = _gn_channels(C, groups)
    gs = cotangents(gs, "gs", dtype, B, C, sizes)
    if relu or ys is not None:
        ys = _gn_same(ys, "ys", dtype, B, C, sizes)
    tensor(stats, "stats", F32, (len(sizes), B, C, 2))
    tensor(gamma, "gamma", F32, (C,))
    dev = zs[0].device
    if dgamma is None:
        dgamma = torch.empty((C,), dtype=F32, device=dev)
    if dbeta is None:
        dbeta = torch.empty((C,), dtype=F32, device=dev)
    tensor(dgamma, "dgamma", F32, (C,))
    tensor(dbeta, "dbeta", F32, (C,))
    on_device([("zs[%d]" % l, z) for l, z in enumerate(zs)] + [("gs[%d]" % l, g) for l, g in enumerate(gs)] +
              [("ys[%d]" % l, y) for l, y in enumerate(ys or [])] +
              [("stats", stats), ("gamma", gamma), ("dgamma", dgamma), ("dbeta", dbeta)])
    dzs = [torch.empty((B, H, W, C), dtype=dtype, device=dev) for H, W in sizes]
    ws, wp, nbytes = _gn_ws(GN_BWD, B, sizes, C, G, dev)
    arr = _gn_table(sizes, zs, y=ys, g=gs, dz=dzs)
    _lib.check(_lib.load().tdn_pyr_gn_bwd(arr, len(zs), B, _ptr(stats), _ptr(gamma), C, G, 1 if relu else 0,
                                          _ptr(dgamma), _ptr(dbeta), 1.0 if accumulate else 0.0, wp, nbytes,
                                          dtype_code(dtype), _lib.stream_ptr()), "tdn_pyr_gn_bwd")
    return [t.permute(0, 3, 1, 2) for t in dzs], dgamma, dbeta
