"""Guard-banded, poisoned allocations for the memory tests (tests/test_gpu_guarded.py; self-test: test_guard_util.py).

Every tensor ``GuardAlloc`` hands out is a view into one ``uint8`` buffer laid out as

    [ lower band | payload | upper band ]

with the payload's ``data_ptr() % 512 == 0`` (what torch's caching allocator gives), both bands filled with a fixed
byte and the payload filled with a poison no kernel legitimately produces: all-ones bytes for floating types (a NaN
with an all-ones mantissa), ``0x5A`` bytes for integer types and ``uint8`` (not a keep flag, not a pool-window index,
and not the ``-1`` that ``tdn_nms`` writes into the tail of ``kept_idx``).  ``check()`` synchronises and reports

  * bytes changed in either band (a store outside the tensor), with the first and last offending byte offset relative
    to the payload's first byte, and
  * for payloads registered as "must be fully written": how many elements still hold the poison, and the first one.

LIMITS.  A band is ``max(1 MiB, one image row of the tensor)`` long: a store further out than that is not seen.  A
store that happens to write the band byte itself is not seen.  Device globals and LDS are out of reach.  Reads are not
checked at all, except through ``guard_copy``: an operand copied into NaN bands turns a stray read into a NaN only if
the value read reaches an output (a read whose result is discarded, ``ok ? v : 0``, is legal and stays invisible).

``TorchProxy`` stands in for the ``torch`` module inside ``torch_detection_amd.ops`` (install it with
``monkeypatch.setattr(ops, "torch", proxy)``): it forwards every attribute to the real ``torch`` except ``empty``,
``empty_like``, ``zeros`` and ``full``, which allocate through the guard, and it counts those allocations per calling
``ops`` function.  ``install(monkeypatch, ops, guard)`` also swaps ``ops._workspace`` / ``ops._aligned_ws`` for
variants that return a fresh, NaN-poisoned, guard-banded buffer of EXACTLY the queried size (rounded up only to the
alignment include/tdn.h demands) on every call.
"""
import collections
import ctypes
import linecache
import math
import re
import sys

import torch as _torch

BAND_MIN = 1 << 20
ALIGN = 512
BAND_BYTE = 0xA5          # output bands: any store of a computed value, of 0, of -1 or of a NaN changes it
NAN_BYTE = 0xFF           # floating poison, workspace poison, and the bands of guarded INPUT copies (reads give NaN)
INT_BYTE = 0x5A

_FLOATS = (_torch.float16, _torch.bfloat16, _torch.float32, _torch.float64)
_INT_VIEW = {1: _torch.uint8, 2: _torch.int16, 4: _torch.int32, 8: _torch.int64}


def poison_byte(dtype):
    return NAN_BYTE if dtype in _FLOATS else INT_BYTE


def _esize(dtype):
    return _torch.empty((), dtype=dtype).element_size()


def _signed(byte, esize):
    """The integer an element of ``esize`` bytes holds when each byte is ``byte`` (as the signed view type sees it)."""
    v = int.from_bytes(bytes([byte]) * esize, "little", signed=False)
    if esize > 1 and v >= 1 << (8 * esize - 1):
        v -= 1 << (8 * esize)
    return v


class _Rec(object):
    __slots__ = ("buf", "off", "nbytes", "label", "must_write", "dtype", "band", "poison", "tensor")


class GuardAlloc(object):
    def __init__(self):
        self.recs = []
        self.retired = []      # buffers of checked records stay referenced until the next check() has synchronised
        self.calls = collections.Counter()         # allocations per ops function (filled by TorchProxy)
        self.ws_calls = collections.Counter()      # exact-size workspaces per ops function
        self.ws_log = []                           # (op, nbytes asked, nbytes given) of this guard's workspaces

    # ---- allocation -------------------------------------------------------------------------------------------
    def alloc(self, shape, dtype=_torch.float32, device=None, interior="poison", label="?", must_write=True,
              band_byte=BAND_BYTE):
        """A contiguous ``shape`` / ``dtype`` tensor between two bands.  ``interior``: "poison" (default), "zero", or a
        number to fill with (neither of the last two can be checked for "was it written": ``must_write`` is dropped)."""
        shape = tuple(int(s) for s in shape)
        es = _esize(dtype)
        n = math.prod(shape) * es
        row = (math.prod(shape[-2:]) if len(shape) >= 2 else 1) * es
        band = -(-max(BAND_MIN, row) // ALIGN) * ALIGN
        buf = _torch.empty(band + n + band + ALIGN, dtype=_torch.uint8, device=device)
        off = band + (-(buf.data_ptr() + band)) % ALIGN
        buf.fill_(band_byte)
        pay = buf[off:off + n]
        r = _Rec()
        r.poison = poison_byte(dtype)
        if interior == "poison":
            pay.fill_(r.poison)
        else:
            must_write = False
        t = pay.view(dtype).view(shape)
        if interior == "zero":
            t.zero_()
        elif interior != "poison":
            t.fill_(interior)
        r.buf, r.off, r.nbytes, r.label, r.must_write, r.dtype, r.band, r.tensor = \
            buf, off, n, label, bool(must_write), dtype, band_byte, t
        self.recs.append(r)
        return t

    def guard_copy(self, t, label="input"):
        """``t``'s values in a guarded buffer with NaN (all-ones) bands: hand it to a kernel as an INPUT."""
        c = self.alloc(tuple(t.shape), t.dtype, t.device, interior="zero", label=label, must_write=False,
                       band_byte=NAN_BYTE)
        c.copy_(t)
        return c

    def shorten(self, t, nbytes):
        """Positive control: register ``t``'s payload as ``nbytes`` long, so whatever lies behind counts as band."""
        for r in self.recs:
            if r.tensor is t:
                r.nbytes = int(nbytes)
                r.must_write = False
                return
        raise KeyError("not a tensor of this guard")

    def workspace(self, nbytes, device, align, op="?"):
        given = -(-int(nbytes) // align) * align
        self.ws_calls[op] += 1
        self.ws_log.append((op, int(nbytes), given))
        return self.alloc((given,), _torch.uint8, device, interior=NAN_BYTE, label="%s: workspace" % op,
                          must_write=False)

    # ---- checking ---------------------------------------------------------------------------------------------
    def check(self):
        """Synchronise, examine every allocation made since the last check, forget them; returns a list of findings
        (strings; empty: clean)."""
        if any(r.buf.is_cuda for r in self.recs):
            _torch.cuda.synchronize()
        self.retired = []
        recs, self.recs = self.recs, []
        flags = []
        for r in recs:
            lo, hi = r.buf[:r.off], r.buf[r.off + r.nbytes:]
            f = [(lo != r.band).sum(), (hi != r.band).sum()]
            if r.must_write and r.nbytes:
                f.append(self._unwritten(r).sum())
            else:
                f.append(_torch.zeros((), dtype=_torch.int64, device=r.buf.device))
            flags.append(_torch.stack(f))
        found = []
        if flags:
            dev = flags[0].device
            table = _torch.stack([f.to(dev) for f in flags]).cpu().tolist()
            for r, (nlo, nhi, nun) in zip(recs, table):
                if nlo:
                    idx = (r.buf[:r.off] != r.band).nonzero().flatten()
                    found.append("%s: %d bytes changed in the LOWER band, payload offsets %d .. %d" %
                                 (r.label, nlo, int(idx[0]) - r.off, int(idx[-1]) - r.off))
                if nhi:
                    idx = (r.buf[r.off + r.nbytes:] != r.band).nonzero().flatten()
                    found.append("%s: %d bytes changed in the UPPER band, payload offsets %d .. %d (payload is %d "
                                 "bytes)" % (r.label, nhi, int(idx[0]) + r.nbytes, int(idx[-1]) + r.nbytes, r.nbytes))
                if nun:
                    first = int(self._unwritten(r).flatten().nonzero()[0])
                    shape = tuple(r.tensor.shape)
                    found.append("%s: %d of %d elements never written (still poison), first at flat index %d = %s of "
                                 "%s" % (r.label, nun, r.tensor.numel(), first,
                                         tuple(int(i) for i in _unravel(first, shape)), shape))
        self.retired = [r.buf for r in recs]
        return found

    @staticmethod
    def _unwritten(r):
        es = _esize(r.dtype)
        return r.buf[r.off:r.off + r.nbytes].view(_INT_VIEW[es]) == _signed(r.poison, es)


def _unravel(i, shape):
    out = []
    for s in reversed(shape):
        out.append(i % s if s else 0)
        i //= s if s else 1
    return reversed(out)


# ---- the torch stand-in ---------------------------------------------------------------------------------------
def _caller(ops_file):
    """(op, argument) of the allocation being made: the outermost-but-public function of ops.py on the stack below the
    proxy, and the name the innermost ops.py line assigns to (best effort)."""
    f = sys._getframe(2)
    op, arg = None, None
    while f is not None:
        if f.f_code.co_filename == ops_file:
            if arg is None:
                m = re.match(r"\s*([\w, ]+?)\s*=[^=]", linecache.getline(ops_file, f.f_lineno))
                arg = (m.group(1) if m else "line") + "@%d" % f.f_lineno
            name = f.f_code.co_name
            if not name.startswith(("_", "<")):
                op = name
                break
            if op is None:
                op = name
        f = f.f_back
    return op or "?", arg or "?"


class TorchProxy(object):
    """``torch`` as ``ops.py`` sees it under the guard."""

    def __init__(self, guard, ops_file):
        self.__dict__["_g"] = guard
        self.__dict__["_file"] = ops_file

    def __getattr__(self, name):
        return getattr(_torch, name)

    def _new(self, shape, dtype, device, interior):
        if len(shape) == 1 and isinstance(shape[0], (tuple, list, _torch.Size)):
            shape = tuple(shape[0])
        op, arg = _caller(self._file)
        dtype = dtype if dtype is not None else _torch.get_default_dtype()
        self._g.calls[op] += 1
        return self._g.alloc(shape, dtype, device, interior, "%s: %s" % (op, arg))

    def empty(self, *shape, dtype=None, device=None):
        return self._new(shape, dtype, device, "poison")

    def zeros(self, *shape, dtype=None, device=None):
        return self._new(shape, dtype, device, "zero")

    def full(self, shape, fill_value, dtype=None, device=None):
        if dtype is None:
            dtype = _torch.get_default_dtype() if isinstance(fill_value, float) else _torch.int64
        return self._new((tuple(shape),), dtype, device, fill_value)

    def empty_like(self, t):
        assert t.is_contiguous(), "ops.py only takes contiguous operands"
        return self._new((tuple(t.shape),), t.dtype, t.device, "poison")


def install(monkeypatch, ops, guard):
    """Put ``ops`` under ``guard`` for the life of ``monkeypatch``: guarded allocations, exact-size workspaces."""
    ops_file = ops.__file__
    proxy = TorchProxy(guard, ops_file)

    def exact_workspace(nbytes, device):          # ops._workspace: users need 16-byte alignment at most
        op, _ = _caller(ops_file)
        return guard.workspace(nbytes, device, 16, op)

    def exact_aligned_ws(nbytes, dev):            # ops._aligned_ws: the header asks for 256-byte alignment
        op, _ = _caller(ops_file)
        ws = guard.workspace(nbytes, dev, 256, op)
        return ws, ctypes.c_void_p(ws.data_ptr())

    monkeypatch.setattr(ops, "torch", proxy)
    monkeypatch.setattr(ops, "_workspace", exact_workspace)
    monkeypatch.setattr(ops, "_aligned_ws", exact_aligned_ws)
    return proxy
