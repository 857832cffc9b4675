"""``SGD``: the parameter update of a training step as two launches of the library (csrc/optim.hip) —
gradient-norm clip, loss unscaling with an overflow check and step skipping, weight decay, momentum (plain / Nesterov)
and the update itself, for all parameters at once, with no host synchronisation.

    opt = SGD(groups, lr=0.02, momentum=0.9, weight_decay=1e-4, max_norm=35, loss_scale='dynamic')
    for batch in loader:
        loss = criterion(model(batch)) * opt.loss_scale     # a device scalar: no synchronisation
        loss.backward()
        reducer.finish()                                    # with dp.attach_reducer: BEFORE the step
        opt.step()

Differences from ``torch.optim.SGD`` + ``clip_grad_norm_`` + ``GradScaler``:
  * gradients are never written: neither unscaled nor clipped in place — ``opt.grad_norm`` (the unscaled norm) and
    ``opt.clip_coef`` are device scalars, the scaled gradients stay as the backward pass left them;
  * a step whose gradients hold an Inf or a NaN is skipped on the device (``skip_nonfinite``): parameters and momentum
    buffers keep their bits, ``steps_skipped`` advances, and with ``loss_scale='dynamic'`` the scale backs off —
    exactly ``torch._amp_update_scale_``;
  * ``lr`` / ``weight_decay`` / ``momentum`` of every group live in a small device array: a schedule changes
    ``param_groups`` and calls ``sync_hyper()`` (``step()`` does, outside a capture); a captured graph or a prepared
    plan needs no recapture;
  * the momentum buffers are views of one flat allocation; a parameter that first gets a gradient after the first taken
    step starts from a zero buffer (torch: from a copy of its gradient — the same value but for the sign of a -0.0).
The arithmetic per element is torch's (``foreach=False``), bit for bit.
"""
import torch

from . import _lib, optim_ops
from ._args import integer, number

_RING = 4


class SGD(torch.optim.Optimizer):
    def __init__(self, params, lr, momentum=0, weight_decay=0, nesterov=False, max_norm=None, loss_scale=None,
                 init_scale=512., growth_factor=2., backoff_factor=.5, growth_interval=2000, skip_nonfinite=True,
                 modules=()):
        defaults = dict(lr=lr, momentum=momentum, dampening=0, weight_decay=weight_decay, nesterov=nesterov,
                        maximize=False, foreach=None, differentiable=False, fused=None)
        super().__init__(params, defaults)
        self._check_groups()
        self.max_norm = 0.0 if max_norm is None else number(max_norm, "max_norm", positive=True)
        self.dynamic = isinstance(loss_scale, str)
        if self.dynamic and loss_scale != 'dynamic':
            raise ValueError("loss_scale must be None, a positive number or 'dynamic', got %r" % (loss_scale,))
        scale = number(init_scale, "init_scale", positive=True) if self.dynamic else \
            1.0 if loss_scale is None else number(loss_scale, "loss_scale", positive=True)
        self.growth = number(growth_factor, "growth_factor")
        self.backoff = number(backoff_factor, "backoff_factor")
        self.interval = integer(growth_interval, "growth_interval", 1, (1 << 31) - 1)
        if self.dynamic and not (self.growth > 1.0 and 0.0 < self.backoff < 1.0):
            raise ValueError("growth_factor must be > 1 and backoff_factor in (0, 1)")
        self.skip_nonfinite = bool(skip_nonfinite)
        self.modules = tuple(modules)
        first = self.param_groups[0]['params'][0]
        for g in self.param_groups:
            for p in g['params']:
                if p.dtype != torch.float32 or not p.is_cuda or p.device != first.device:
                    raise ValueError("params must be float32 CUDA tensors on one device, got %s on %s"
                                     % (str(p.dtype).replace("torch.", ""), p.device))
        self.device = first.device
        self._fstate, self._istate = optim_ops.sgd_state(self.device, scale)
        ng = len(self.param_groups)
        self._hyper = torch.zeros(ng, 3, dtype=torch.float32, device=self.device)
        self._pins = [torch.zeros(ng, 3, dtype=torch.float32).pin_memory() for _ in range(_RING)]
        self._pin_events = [None] * _RING
        self._pin_next = 0
        self._hyper_last = None
        self._bufs = {}            # parameter -> its view of a flat momentum allocation
        self._flats = []
        self._key = None
        self._plan = self._table = self._ws = self._table_ptr = self._ws_ptr = None
        self._updated = []
        self._retired = []
        self._adopted_init = 1     # whether adopted (loaded) momentum buffers count as initialised
        self.sync_hyper()

    # ---- checks -------------------------------------------------------------------------------------------------
    def _check_groups(self):
        nesterov = self.param_groups[0]['nesterov']
        for g in self.param_groups:
            lr, mom, wd = (number(g[k], k) for k in ('lr', 'momentum', 'weight_decay'))
            if lr < 0 or mom < 0 or wd < 0:
                raise ValueError("lr, momentum and weight_decay must be >= 0")
            if g.get('dampening', 0) != 0 or g.get('maximize', False):
                raise ValueError("dampening != 0 and maximize are not supported")
            if bool(g['nesterov']) != bool(nesterov):
                raise ValueError("nesterov must be the same in every parameter group")
            if g['nesterov'] and mom <= 0:
                raise ValueError("Nesterov momentum requires a momentum")
        self.nesterov = bool(nesterov)

    # ---- observable results: device tensors, reading one is the caller's synchronisation --------------------------
    def _f(self, i):
        return self._fstate[i:i + 1]

    def _i(self, i):
        return self._istate[i:i + 1]

    loss_scale = property(lambda self: self._f(_lib.SGD_F_SCALE))
    grad_norm = property(lambda self: self._f(_lib.SGD_F_NORM))
    clip_coef = property(lambda self: self._f(_lib.SGD_F_COEF))
    growth_tracker = property(lambda self: self._i(_lib.SGD_I_TRACKER))
    steps_taken = property(lambda self: self._i(_lib.SGD_I_TAKEN))
    steps_skipped = property(lambda self: self._i(_lib.SGD_I_SKIPPED))
    last_skipped = property(lambda self: self._i(_lib.SGD_I_LAST_SKIPPED))

    # ---- hyper-parameters ---------------------------------------------------------------------------------------
    def sync_hyper(self):
        """Copy ``lr`` / ``weight_decay`` / ``momentum`` of ``param_groups`` to the device array the kernels read
        (fp32, pinned host -> device, non-blocking; nothing is copied when nothing changed).  Call it before a replay
        when a schedule changed them; it cannot run inside a capture."""
        vals = [[float(g['lr']), float(g['weight_decay']), float(g['momentum'])] for g in self.param_groups]
        if vals == self._hyper_last:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("SGD.sync_hyper() inside a graph capture: call it before the replay instead")
        self._check_groups()
        k = self._pin_next
        self._pin_next = (k + 1) % _RING
        if self._pin_events[k] is not None:
            self._pin_events[k].synchronize()      # the copy made _RING changes ago: long done
        self._pins[k].copy_(torch.tensor(vals, dtype=torch.float32))
        self._hyper.copy_(self._pins[k], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._pin_events[k] = ev
        self._hyper_last = vals

    # ---- the table ----------------------------------------------------------------------------------------------
    def _live_key(self):
        key = []
        for gi, g in enumerate(self.param_groups):
            mom = g['momentum'] != 0
            for p in g['params']:
                gr = p.grad
                if gr is not None:
                    key.append((gi, mom, p.data_ptr(), p.stride(), gr.data_ptr(), gr.stride()))
        return key

    def _build(self):
        live = [(gi, g, p) for gi, g in enumerate(self.param_groups) for p in g['params'] if p.grad is not None]
        if not live:
            return False
        need = [p for _, g, p in live if g['momentum'] != 0 and p not in self._bufs]
        if need and not self._flats:      # the usual case: ONE allocation, for every parameter that has momentum
            need = [p for g in self.param_groups if g['momentum'] != 0 for p in g['params']]
        if need:
            flat, offs = optim_ops.sgd_momentum([p.numel() for p in need], self.device)
            self._flats.append(flat)
            for p, o in zip(need, offs):
                self._bufs[p] = flat.as_strided(tuple(p.shape), p.stride(), flat.storage_offset() + o)
        items = []
        for gi, g, p in live:
            buf = None
            if g['momentum'] != 0:
                buf = self._bufs[p]
                if tuple(buf.stride()) != tuple(p.stride()):
                    raise RuntimeError("a parameter changed its memory format after the optimizer's first step")
                st = self.state[p]
                old = st.get('momentum_buffer')
                if old is not None and old is not buf:       # a loaded checkpoint: adopt its values
                    buf.copy_(old)
                    if self._adopted_init:
                        self._i(_lib.SGD_I_BUF_INIT).fill_(1)
                st['momentum_buffer'] = buf
            items.append(optim_ops.sgd_item(p, p.grad, buf, gi, name="params"))
        if self._table is not None:       # a captured graph or a launch plan may still hold the old pointers
            self._retired.append((self._table, self._ws))
        self._plan = optim_ops.sgd_plan(items, len(self.param_groups))
        self._table, self._table_ptr, self._ws, self._ws_ptr = optim_ops.sgd_upload(self._plan, self.device)
        self._updated = [p for _, _, p in live]
        return True

    # ---- the step -----------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        """Two launches on the current stream.  With a gradient reducer (``dp.attach_reducer``) call this AFTER
        ``reducer.finish()``: the step reads the reduced gradients in the reducer's flat buffer."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        capturing = torch.cuda.is_current_stream_capturing()
        key = self._live_key()
        if key != self._key:
            if capturing:
                raise RuntimeError("SGD.step(): the descriptor table would have to be rebuilt during a graph capture "
                                   "(first step, or a parameter / gradient pointer or stride changed): run one eager "
                                   "step with the same gradient tensors before capturing")
            self._key = key if self._build() else None
            if self._key is None:
                return loss
        if not capturing:
            self.sync_hyper()
        optim_ops.sgd_step(self._plan, self._table_ptr, self._hyper, self._fstate, self._istate, self._ws_ptr,
                           self.nesterov, self.skip_nonfinite, self.dynamic, self.max_norm, self.growth, self.backoff,
                           self.interval)
        if not capturing:
            # host only, no launch: ConvUnit.refresh sees the change and repacks on the next forward
            torch.autograd.graph.increment_version(self._updated)
            if self.modules:
                from . import functional
                functional.invalidate_packed(*self.modules)
        return loss

    # ---- checkpoints --------------------------------------------------------------------------------------------
    def state_dict(self):
        """``torch.optim.SGD``'s format (it loads there and back) plus the loss-scale state under ``'tdn_sgd'``."""
        sd = super().state_dict()
        f, i = self._fstate.tolist(), self._istate.tolist()
        sd['tdn_sgd'] = {'loss_scale': f[_lib.SGD_F_SCALE], 'growth_tracker': i[_lib.SGD_I_TRACKER],
                         'steps_taken': i[_lib.SGD_I_TAKEN], 'steps_skipped': i[_lib.SGD_I_SKIPPED],
                         'buf_init': i[_lib.SGD_I_BUF_INIT]}
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._check_groups()
        self._key = None               # the next step adopts the loaded momentum buffers into the flat allocation
        self._hyper_last = None
        extra = state_dict.get('tdn_sgd')
        self._adopted_init = 1 if extra is None else int(extra['buf_init'])
        if extra is not None:
            self._f(_lib.SGD_F_SCALE).fill_(float(extra['loss_scale']))
            for k, idx in (('growth_tracker', _lib.SGD_I_TRACKER), ('steps_taken', _lib.SGD_I_TAKEN),
                           ('steps_skipped', _lib.SGD_I_SKIPPED), ('buf_init', _lib.SGD_I_BUF_INIT)):
                self._i(idx).fill_(int(extra[k]))
        self.sync_hyper()
