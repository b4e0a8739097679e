"""The parameter update on the device: what the reference's training step does behind ``loss.backward()``.

``ev-YOLOv6/yolov6/core/engine.py:547-552`` runs ``scaler.step(optimizer)`` (a host read of ``found_inf``, then torch's SGD with
its own passes over ``p``, ``grad`` and the momentum buffer), ``scaler.update()``, ``optimizer.zero_grad()`` and
``ema.update(model)`` (``yolov6/utils/ema.py:30-41``: a Python loop over the state dict, two launches and a temporary per entry).
Here ``TrainStep(optimizer, scaler, ema)(model)`` is one asynchronous copy of a few floats and one call of ``evrep_train_step``
(csrc/evrep_step.hip): three launches that serve every tensor of the model, each element read and written once, nothing read on
the host.  ``step_host`` is the same statements in numpy float32: the oracle of the kernels and the route of CPU tensors.

The statements (include/evrep.h states them with ``evrep_train_step``), each ONE float32 operation:

    inv = fl32(1 / double(scale))                      1 without a scaler
    if found_inf == 0 and the tensor has a gradient:
        g' = g * inv
        d  = g' + wd * p   if wd != 0 else g'
        buf = d if applied_steps == 0 else buf * momentum + d;  d2 = d + momentum * buf        (momentum != 0)
        d2 = d, buf untouched                                                                   (momentum == 0)
        p  = p + (-lr) * d2
    if the tensor has an EMA entry:  e = e * ema_d;  e = e + ema_1md * p
    with zero_grad:  g = +0.0
    then, once:  the scale automaton of ``_amp_update_scale_``;  applied_steps += (found_inf == 0);  found_inf = 0

Nesterov SGD with float32 parameters only, as every shipped config builds it; Adam, ``RepOptimizer``, half-precision
parameters, gradient clipping and DDP's all-reduce are not mirrored.
"""
import functools
import math
from copy import deepcopy

import numpy as np
import torch

from . import _lib

F32 = np.float32
CHUNK = _lib.STEP_CHUNK
HAS_GRAD, HAS_EMA, EMA_ONLY = _lib.STEP_HAS_GRAD, _lib.STEP_HAS_EMA, _lib.STEP_EMA_ONLY
ZERO_GRAD, NO_CHECK, KEEP_SCALE = _lib.STEP_ZERO_GRAD, _lib.STEP_NO_CHECK, _lib.STEP_KEEP_SCALE

# the two tables as numpy records: evrep_step_tensor and evrep_step_chunk of include/evrep.h
TENSOR_DTYPE = np.dtype([("p", "<u8"), ("g", "<u8"), ("buf", "<u8"), ("ema", "<u8"), ("n", "<i8"), ("group", "<i4"), ("flags", "<u4")])
CHUNK_DTYPE = np.dtype([("first", "<i8"), ("tensor", "<i4"), ("count", "<i4")])


# ------------------------------------------------------------------------------------------------------------ the host route
def ema_decay(updates, decay=0.9999, tau=2000.0):
    """The reference's ``ModelEMA.decay``: ``decay * (1 - exp(-updates / tau))``, in Python floats."""
    return decay * (1 - math.exp(-updates / tau))


def hyper_row(groups, decay=None):
    """The hyper row of ``evrep_train_step``: ``[ema_d, ema_1md, (lr, momentum, weight_decay) per group]`` in float32.  ``groups``:
    param-group dicts or ``(lr, momentum, weight_decay)`` triples; ``decay``: this step's EMA decay or None.  ``1 - decay`` is
    formed in double, as Python forms it, and rounded once."""
    row = np.zeros(_lib.STEP_HYPER_EMA + 3 * len(groups), dtype=F32)
    if decay is not None:
        row[0], row[1] = F32(float(decay)), F32(1.0 - float(decay))
    for k, g in enumerate(groups):
        lr, mom, wd = (g["lr"], g.get("momentum", 0.0), g.get("weight_decay", 0.0)) if isinstance(g, dict) else g
        row[2 + 3 * k: 5 + 3 * k] = F32(float(lr)), F32(float(mom)), F32(float(wd))
    return row


def new_state(scale=1.0, tracker=0, applied_steps=0):
    """The state words of ``step_host``: what the device keeps in ``amp`` and ``applied_steps``."""
    return dict(found_inf=0, scale=F32(scale), tracker=int(tracker), applied_steps=int(applied_steps))


def step_host(rows, hyper, state, amp=None, zero_grad=True, check=True, keep_scale=False, ema_only=False):
    """The statements of the module docstring in numpy float32, in place.

    ``rows``: dicts with ``p``, ``g``, ``buf``, ``ema`` (float32 arrays or None), ``group`` and ``flags`` (``HAS_GRAD``, ``HAS_EMA``,
    ``EMA_ONLY``); ``hyper``: ``hyper_row(...)``; ``state``: ``new_state(...)``, updated in place; ``amp``: ``(growth_factor,
    backoff_factor, growth_interval)`` or None for no scaler; ``check`` / ``keep_scale``: the complements of ``EVREP_STEP_NO_CHECK``
    / ``EVREP_STEP_KEEP_SCALE``; ``ema_only``: ``evrep_ema_update`` (the state is not touched)."""
    hyper = np.asarray(hyper, dtype=F32)
    with np.errstate(all="ignore"):
        if ema_only:
            for r in rows:
                _ema_host(r["ema"], r["p"], hyper)
            return
        if amp is not None and check:
            for r in rows:
                if (r["flags"] & HAS_GRAD) and not (r["flags"] & EMA_ONLY) and not np.isfinite(r["g"]).all():
                    state["found_inf"] = 1
        found = bool(state["found_inf"]) if amp is not None else False
        inv = F32(1.0 / np.float64(state["scale"])) if amp is not None else F32(1.0)
        first = state["applied_steps"] == 0
        for r in rows:
            only = bool(r["flags"] & EMA_ONLY)
            has_grad = bool(r["flags"] & HAS_GRAD) and not only
            if has_grad and not found:
                lr, mom, wd = hyper[2 + 3 * r["group"]: 5 + 3 * r["group"]]
                p, g, buf = r["p"], r["g"], r["buf"]
                d = g * inv
                if wd != 0:
                    d = d + wd * p
                d2 = d
                if mom != 0:
                    buf[...] = d if first else buf * mom + d
                    d2 = d + mom * buf
                p[...] = p + (-lr) * d2
            if (r["flags"] & HAS_EMA) and r["ema"] is not None:
                _ema_host(r["ema"], r["p"], hyper)
            if has_grad and zero_grad:
                r["g"][...] = F32(0.0)
        if amp is not None and not keep_scale:
            growth, backoff, interval = amp
            if found:
                state["scale"], state["tracker"] = F32(np.float64(state["scale"]) * np.float64(backoff)), 0
            else:
                s = state["tracker"] + 1
                if s == int(interval):
                    grown = F32(np.float64(state["scale"]) * np.float64(growth))
                    if np.isfinite(grown):
                        state["scale"] = grown
                    state["tracker"] = 0
                else:
                    state["tracker"] = s
        state["applied_steps"] += 0 if found else 1
        state["found_inf"] = 0


def _ema_host(e, p, hyper):
    e[...] = e * hyper[0]
    e[...] = e + hyper[1] * p


# ---------------------------------------------------------------------------------------------------------------- the tables
def _refuse(key, t, device):
    """The refusals of this module for one tensor, naming its state-dict key."""
    if t.dtype != torch.float32:
        raise ValueError("%s is %s: the step takes float32 tensors (half precision is not mirrored)" % (key, t.dtype))
    if not t.is_contiguous():
        raise ValueError("%s is not contiguous: the step reads it as one span, call .contiguous() on it first" % key)
    if device is not None and t.device != device:
        raise ValueError("%s is on %s, the first tensor on %s: all tensors of a step must share a device" % (key, t.device, device))


_WRAPPERS = (torch.nn.parallel.DataParallel, torch.nn.parallel.DistributedDataParallel)


def _bare(model):
    """The module inside a DataParallel / DistributedDataParallel wrapper; any other module as it is."""
    return model.module if isinstance(model, _WRAPPERS) else model


def _entries(model):
    """The model's state dict with the tensors themselves (not detached copies of their handles)."""
    return _bare(model).state_dict(keep_vars=True)


def _wants_buffer(group):
    """A group keeps momentum buffers unless it was built as plain SGD: momentum 0 and no Nesterov flag."""
    return bool(group.get("momentum", 0) != 0 or group.get("nesterov"))


class _Row:
    __slots__ = ("key", "p", "param", "buf", "ema", "group", "flags", "state")


class _StepTable:
    """The tensor and chunk tables of one set of rows: the parameters of an optimizer in group order (or none), each with its EMA
    entry if there is one, then the EMA-only entries.  ``ensure()`` compares every address with what was uploaded and uploads
    again only on a change (``uploads`` counts)."""

    def __init__(self, optimizer=None, ema=None, model=None):
        self.optimizer, self.ema, self.model = optimizer, ema, model
        self.uploads = 0
        self.rows = self.sig = self.device = self.sizes = self.state = None
        self.tensors_dev = self.chunks_dev = None
        self.n_tensors = self.n_chunks = 0

    def invalidate(self):
        self.rows = self.sig = None

    # the static part: which tensors, in which order
    def _build_rows(self):
        rows, dev = [], None
        pairs = {}
        if self.ema is not None:
            model_sd = _entries(self.model)
            for key, e in self.ema.ema.state_dict(keep_vars=True).items():
                if not e.dtype.is_floating_point:
                    continue                                             # integer entries are left alone, as the reference leaves them
                if key not in model_sd:
                    raise ValueError("%s: the EMA model has this entry and the model does not" % key)
                pairs[key] = (model_sd[key], e)
        by_id = {id(m): key for key, (m, _) in pairs.items()}
        if len(by_id) != len(pairs):
            raise ValueError("two state-dict keys share one tensor (tied weights): %s"
                             % sorted(k for k, (m, _) in pairs.items() if by_id[id(m)] != k))
        if self.optimizer is not None:
            names = self.optimizer._names
            for k, group in enumerate(self.optimizer.param_groups):
                self.optimizer._check_group(group)
                for i, p in enumerate(group["params"]):
                    r = _Row()
                    r.key = by_id.get(id(p)) or names.get(id(p)) or "param_groups[%d]['params'][%d]" % (k, i)
                    r.p = r.param = p
                    r.ema = pairs.pop(by_id[id(p)])[1] if id(p) in by_id else None
                    r.group, r.flags, r.buf = k, (HAS_EMA if r.ema is not None else 0), None
                    r.state = self.optimizer.state[p]
                    rows.append(r)
        for key, (m, e) in pairs.items():
            r = _Row()
            r.key, r.p, r.param, r.ema, r.buf, r.group, r.flags, r.state = key, m, None, e, None, 0, HAS_EMA | EMA_ONLY, None
            rows.append(r)
        for r in rows:
            dev = r.p.device if dev is None else dev
            _refuse(r.key, r.p, dev)
            if r.ema is not None:
                _refuse(r.key + " (EMA)", r.ema, dev)
                if r.ema.shape != r.p.shape:
                    raise ValueError("%s: the EMA entry is %s, the model's %s" % (r.key, tuple(r.ema.shape), tuple(r.p.shape)))
        self.rows, self.device = rows, dev
        self.state = self.optimizer.state if self.optimizer is not None else None

    def _grad(self, r):
        p = r.param
        return p.grad if (p is not None and p.requires_grad) else None

    def _signature(self):
        """Everything the uploaded table was made from that a caller can change between two steps, in two parts.  Where the
        tensors are: per group its size and whether it keeps buffers, per row the address of the tensor and of its EMA entry
        (``.half()``, ``.to()`` and ``.data =`` move them).  What moves with the steps: per row the address of the gradient (0 for
        None or a frozen parameter) and of the momentum buffer the OPTIMIZER holds for it now (``load_state_dict`` and an
        assignment to ``optimizer.state`` replace it).  On the per-step path: one pass, no helper calls."""
        opt = self.optimizer
        where, moving = [], []
        if opt is not None:
            where.append(opt.state is self.state)                       # load_state_dict puts a new dict of states in its place
            for group in opt.param_groups:
                where.append(len(group["params"]))
                where.append(group.get("momentum", 0) != 0 or bool(group.get("nesterov")))
        for r in self.rows:
            p = r.param
            where.append(r.p.data_ptr())
            if r.ema is not None:
                where.append(r.ema.data_ptr())
            if p is not None:
                g = p.grad if p.requires_grad else None
                if g is None:
                    moving.append(0)
                else:
                    moving.append(g.data_ptr())
                    b = r.state.get("momentum_buffer")              # (the parameter's own state dict, kept by the row:
                    moving.append(0 if b is None else b.data_ptr())  #  looking it up hashes a tensor, in Python, on every step)
        return tuple(where), tuple(moving)

    def ensure(self):
        sizes = [len(g["params"]) for g in self.optimizer.param_groups] if self.optimizer is not None else []
        if self.rows is None or sizes != self.sizes:                    # a group was added, or grew
            self._build_rows()
            self.sizes, self.sig = sizes, None
        sig = self._signature()
        if sig == self.sig:
            return
        if self.sig is not None and sig[0] != self.sig[0]:              # a tensor of the model or of the EMA model moved: list them anew
            self._build_rows()
        wants = []
        for group in (self.optimizer.param_groups if self.optimizer is not None else ()):
            self.optimizer._check_group(group)
            wants.append(_wants_buffer(group))
        for r in self.rows:                                             # the part a step can change: addresses, gradients, buffers
            _refuse(r.key, r.p, self.device)
            if r.ema is not None:
                _refuse(r.key + " (EMA)", r.ema, self.device)
            g = self._grad(r)
            r.flags &= ~HAS_GRAD
            r.buf = None
            if g is None:
                continue
            _refuse(r.key + ".grad", g, self.device)
            if g.shape != r.p.shape:
                raise ValueError("%s.grad is %s, the parameter %s" % (r.key, tuple(g.shape), tuple(r.p.shape)))
            r.flags |= HAS_GRAD
            if wants[r.group]:
                r.buf = self.optimizer._buffer(r.param)
                _refuse(r.key + " (momentum_buffer)", r.buf, self.device)
                if r.buf.shape != r.p.shape:
                    raise ValueError("%s: the momentum buffer is %s, the parameter %s" % (r.key, tuple(r.buf.shape), tuple(r.p.shape)))
        self.sig = self._signature()                                    # (again: the pass above may have made buffers)
        self.uploads += 1
        if self.device is not None and self.device.type == "cuda":
            self._upload()

    def _upload(self):
        live = [r for r in self.rows if r.p.numel() > 0]                # an empty tensor contributes no row and no chunk
        tens = np.zeros(len(live), dtype=TENSOR_DTYPE)
        chunks = []
        for i, r in enumerate(live):
            n = r.p.numel()
            g = self._grad(r) if (r.flags & HAS_GRAD) else None
            tens[i] = (r.p.data_ptr(), 0 if g is None else g.data_ptr(), 0 if (g is None or r.buf is None) else r.buf.data_ptr(),
                       0 if r.ema is None else r.ema.data_ptr(), n, r.group, r.flags)
            c = np.zeros((n + CHUNK - 1) // CHUNK, dtype=CHUNK_DTYPE)
            c["first"] = np.arange(len(c), dtype=np.int64) * CHUNK
            c["tensor"] = i
            c["count"] = np.minimum(n - c["first"], CHUNK)
            chunks.append(c)
        chunks = np.concatenate(chunks) if chunks else np.zeros(0, dtype=CHUNK_DTYPE)
        self.n_tensors, self.n_chunks = len(tens), len(chunks)
        to_dev = lambda a: torch.from_numpy(np.frombuffer(a.tobytes() or b"\0" * 8, dtype=np.uint8).copy()).to(self.device)
        self.tensors_dev, self.chunks_dev = to_dev(tens), to_dev(chunks)

    def host_rows(self):
        """The rows as ``step_host`` takes them: numpy views of the CPU tensors."""
        view = lambda t: None if t is None else t.detach().numpy()
        out = []
        for r in self.rows:
            g = self._grad(r) if (r.flags & HAS_GRAD) else None
            out.append(dict(p=view(r.p), g=view(g), buf=view(r.buf) if g is not None else None, ema=view(r.ema), group=r.group,
                            flags=r.flags))
        return out


class _Hyper:
    """The hyper row on the device: refreshed by one asynchronous copy from pinned memory, and only when its bytes changed."""

    def __init__(self):
        self.dev = self.last = None

    def upload(self, row, device):
        if self.last is not None and self.dev is not None and self.dev.device == device and np.array_equal(self.last.view(np.uint32),
                                                                                                         row.view(np.uint32)):
            return self.dev
        if self.dev is None or self.dev.device != device or self.dev.numel() != row.size:
            self.dev = torch.empty(row.size, dtype=torch.float32, device=device)
        # (a fresh pinned block per upload: the host allocator holds it until the copy has run, so the next step's row cannot
        #  overwrite one still in flight)
        self.dev.copy_(torch.from_numpy(row.copy()).pin_memory(), non_blocking=True)
        self.last = row.copy()
        return self.dev


def _run(table, hyper, row, optimizer, scaler, flags, foreign=None):
    """One ``evrep_train_step`` (or ``step_host`` for CPU tensors) over ``table`` with the hyper row ``row``."""
    dev = table.device
    if dev is None:
        return
    n_groups = len(optimizer.param_groups)
    if n_groups > _lib.STEP_MAX_GROUPS:
        raise ValueError("the step takes up to %d parameter groups, got %d" % (_lib.STEP_MAX_GROUPS, n_groups))
    applied = optimizer._applied_on(dev)
    amp, consts = None, (2.0, 0.5, 1)
    if foreign is not None:
        amp = foreign
    elif scaler is not None and scaler.is_enabled():
        amp, consts = scaler._state_on(dev), (scaler._growth_factor, scaler._backoff_factor, scaler._growth_interval)
    if dev.type != "cuda":
        st = new_state(applied_steps=int(applied[0]))
        if amp is not None:
            st.update(found_inf=int(amp[0]), scale=amp[1:2].view(torch.float32).numpy()[0], tracker=int(amp[2]))
        step_host(table.host_rows(), row, st, consts if amp is not None else None, bool(flags & ZERO_GRAD), not (flags & NO_CHECK),
                  bool(flags & KEEP_SCALE))
        applied[0] = st["applied_steps"]
        if amp is not None:
            amp[0], amp[2] = st["found_inf"], st["tracker"]
            amp[1:2].view(torch.float32)[0] = float(st["scale"])
        return
    with torch.cuda.device(dev):
        _lib.api().evrep_train_step(_lib.ptr(table.tensors_dev), table.n_tensors, _lib.ptr(table.chunks_dev), table.n_chunks,
                                    _lib.ptr(hyper.dev), n_groups, _lib.ptr(amp), _lib.ptr(applied), consts[0], consts[1], consts[2],
                                    flags, _lib.stream_ptr())


# -------------------------------------------------------------------------------------------------------------- the optimizer
class SGD(torch.optim.SGD):
    """Nesterov SGD whose ``step()`` is ``evrep_train_step``.  ``param_groups`` are torch's own dicts (``lr``, ``momentum`` and
    ``weight_decay`` are read on every step, so warm-up writes and ``LambdaLR`` work unchanged) and ``state_dict()`` /
    ``load_state_dict()`` speak torch SGD's format.  With ``zero_grad`` (the default) the step leaves every gradient it used at +0.0
    in place, so the gradient tensors stay where they are and the tables are uploaded once (``table_uploads``).  A parameter
    whose ``.grad`` is None or that is frozen is not stepped.  ``names``: ``{id(parameter): state-dict key}`` for messages."""

    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, *, maximize=False,
                 zero_grad=True, names=None):
        self._names = dict(names or {})
        self._check_group(dict(momentum=momentum, dampening=dampening, nesterov=nesterov, maximize=maximize))
        self._row = None
        super().__init__(params, lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                         maximize=maximize)
        self._step_supports_amp_scaling = True       # torch.amp.GradScaler hands grad_scale / found_inf over instead of reading
        self.zero_grad_in_step = bool(zero_grad)
        self._table, self._hyper, self._applied, self._foreign = _StepTable(self), _Hyper(), None, None
        for group in self.param_groups:
            self._check_group(group)
        self._table._build_rows()                    # the refusals, at construction

    @staticmethod
    def _check_group(group):
        if group.get("maximize"):
            raise NotImplementedError("maximize=True is not mirrored")
        if group.get("dampening", 0) != 0:
            raise NotImplementedError("dampening != 0 is not mirrored: the reference builds SGD without it")
        if group.get("momentum", 0) != 0 and not group.get("nesterov"):
            raise NotImplementedError("momentum without nesterov=True is not mirrored: the reference builds Nesterov SGD")

    @property
    def table_uploads(self):
        return self._table.uploads

    def _buffer(self, p):
        """The momentum buffer of ``p``, made on first use as -0.0: ``-0.0 * momentum + d == d`` bit for bit, the same as torch's
        clone of ``d`` for a buffer that is absent."""
        st = self.state[p]
        if st.get("momentum_buffer") is None:
            st["momentum_buffer"] = torch.full_like(p, -0.0, memory_format=torch.contiguous_format)
        return st["momentum_buffer"]

    def _applied_on(self, device):
        if self._applied is None:
            self._applied = torch.zeros(1, dtype=torch.int32, device=device)
        elif self._applied.device != device:
            self._applied = self._applied.to(device)
        return self._applied

    def invalidate(self):
        """Have the next step list the tensors anew.  Addresses, gradients and buffers are compared on every step; this is for
        what a comparison of addresses cannot see, such as a module buffer assigned a new tensor."""
        self._table.invalidate()

    def _flags(self):
        return ZERO_GRAD if self.zero_grad_in_step else 0

    def _launch(self, scaler=None, table=None, decay=None, foreign=None, flags=0, refresh=True):
        table = table or self._table
        if refresh:
            table.ensure()
            row = hyper_row(self.param_groups, decay)
            if table.device is not None and table.device.type == "cuda":
                self._hyper.upload(row, table.device)
            self._row = row
        _run(table, self._hyper, self._row, self, scaler, flags | self._flags(), foreign)
        self._opt_called = True

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        foreign = None
        if hasattr(self, "found_inf"):               # torch.amp.GradScaler.step: its own check has run, it updates its own scale
            self._table.ensure()
            dev = self._table.device
            if self._foreign is None or self._foreign.device != dev:
                self._foreign = torch.zeros(_lib.STEP_AMP_WORDS, dtype=torch.int32, device=dev)
            foreign = self._foreign
            foreign[0:1].copy_(self.found_inf.reshape(1) != 0)
            scale = getattr(self, "grad_scale", None)
            if scale is None:
                foreign[1:2].view(torch.float32).fill_(1.0)
            else:
                foreign[1:2].view(torch.float32).copy_(scale.reshape(1))
        self._launch(foreign=foreign, flags=(NO_CHECK | KEEP_SCALE) if foreign is not None else 0)
        return loss

    def zero_grad(self, set_to_none=False):
        """torch's, but zeroing in place by default: a gradient set to None comes back at another address and the tables are
        uploaded again.  After a step with ``zero_grad`` the gradients are +0.0 already."""
        super().zero_grad(set_to_none=set_to_none)

    def applied_steps(self):
        """The steps that were not skipped.  Reads the device."""
        return 0 if self._applied is None else int(self._applied.item())

    def state_dict(self):
        """torch SGD's format.  A buffer no step has written is left out, as torch leaves it absent (this reads
        ``applied_steps``)."""
        sd = super().state_dict()
        keep = self.applied_steps() > 0
        mom = {}
        for g in sd["param_groups"]:
            for i in g["params"]:
                mom[i] = g.get("momentum", 0) != 0
        for i, st in list(sd["state"].items()):
            if "momentum_buffer" in st and not (keep and mom.get(i)):
                st = dict(st)
                st["momentum_buffer"] = None
                sd["state"][i] = st
            elif st.get("momentum_buffer") is not None:
                st = dict(st)
                st["momentum_buffer"] = st["momentum_buffer"].clone()
                sd["state"][i] = st
        sd["state"] = {i: st for i, st in sd["state"].items() if any(v is not None for v in st.values())}
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        any_buf = False
        for group in self.param_groups:
            for p in group["params"]:
                buf = self.state.get(p, {}).get("momentum_buffer")
                if buf is not None:
                    self.state[p]["momentum_buffer"] = buf.detach().to(p.device, torch.float32).clone(memory_format=torch.contiguous_format)
                    any_buf = True
        dev = self._table.device
        if dev is not None:
            self._applied_on(dev).fill_(1 if any_buf else 0)
        self._table.invalidate()


def build_optimizer(cfg, model, zero_grad=True):
    """The reference's ``solver/build.py:build_optimizer`` for ``cfg.solver.optim == "SGD"``: three groups in its order -- the
    BatchNorm2d weights, the other weights with ``cfg.solver.weight_decay``, the biases -- with ``lr0``, ``momentum`` and Nesterov."""
    if cfg.solver.optim != "SGD":
        raise NotImplementedError("optim=%r: only the Nesterov SGD of the shipped configs is mirrored" % (cfg.solver.optim,))
    bn_weights, weights, biases = [], [], []
    for m in model.modules():
        if isinstance(getattr(m, "bias", None), torch.nn.Parameter):
            biases.append(m.bias)
        if isinstance(m, torch.nn.BatchNorm2d):
            bn_weights.append(m.weight)
        elif isinstance(getattr(m, "weight", None), torch.nn.Parameter):
            weights.append(m.weight)
    names = {id(p): k for k, p in model.named_parameters()}
    opt = SGD(bn_weights, lr=cfg.solver.lr0, momentum=cfg.solver.momentum, nesterov=True, zero_grad=zero_grad, names=names)
    opt.add_param_group({"params": weights, "weight_decay": cfg.solver.weight_decay})
    opt.add_param_group({"params": biases})
    opt._table.invalidate()
    opt._table._build_rows()
    return opt


# ----------------------------------------------------------------------------------------------------------------- the scaler
class GradScaler:
    """``torch.amp.GradScaler``'s interface with the scale, the growth tracker and ``found_inf`` on the device and no read
    but ``get_scale()``.  ``step(optimizer)`` of this module's ``SGD`` is the fused route: check, step and scale update in one
    call, so the ``update()`` behind it has nothing left to do."""

    def __init__(self, init_scale=2.0 ** 16, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, enabled=True, device=None):
        if enabled:
            if not growth_factor > 1.0:
                raise ValueError("The growth factor must be > 1.0.")
            if not 0.0 < backoff_factor < 1.0:
                raise ValueError("The backoff factor must be in (0, 1).")
            if int(growth_interval) < 1:
                raise ValueError("growth_interval must be >= 1")
        self._enabled = bool(enabled)
        self._init_scale, self._init_tracker = float(init_scale), 0
        self._growth_factor, self._backoff_factor, self._growth_interval = float(growth_factor), float(backoff_factor), int(growth_interval)
        self._amp = None if device is None else self._make(torch.device(device))
        self._stepped = False

    def _make(self, device):
        amp = torch.zeros(_lib.STEP_AMP_WORDS, dtype=torch.int32)
        amp[1:2].view(torch.float32)[0] = self._init_scale
        amp[2] = self._init_tracker
        return amp.to(device)

    def _state_on(self, device):
        if self._amp is None:
            self._amp = self._make(device)
        elif self._amp.device != device:
            raise ValueError("the scaler's state is on %s, the step on %s" % (self._amp.device, device))
        return self._amp

    def is_enabled(self):
        return self._enabled

    def scale(self, outputs):
        if not self._enabled:
            return outputs
        amp = self._state_on(outputs.device)
        return outputs * amp[1:2].view(torch.float32).reshape(()).to(outputs.dtype)

    def step(self, optimizer, *args, **kwargs):
        if not self._enabled:
            return optimizer.step(*args, **kwargs)
        if not isinstance(optimizer, SGD):
            raise TypeError("detector_step.GradScaler drives detector_step.SGD; %s takes torch.amp.GradScaler" % type(optimizer).__name__)
        optimizer._launch(scaler=self)
        self._stepped = True

    def update(self, new_scale=None):
        if not self._enabled:
            return
        if new_scale is not None:
            if self._amp is None:                    # no scale() or step() yet: the state is made with this scale
                self._init_scale = float(new_scale)
            else:
                self._amp[1:2].view(torch.float32).fill_(float(new_scale))
            self._stepped = False
            return
        if not self._stepped:
            raise RuntimeError("update() without a step(): the scale is updated by the step's own finish launch")
        self._stepped = False

    def get_scale(self):
        """The scale as a Python float.  The only read of the device in this module's steady state."""
        if not self._enabled:
            return 1.0
        return self._init_scale if self._amp is None else float(self._amp[1:2].view(torch.float32).item())

    def _get_growth_tracker(self):
        if not self._enabled:
            return 0
        return self._init_tracker if self._amp is None else int(self._amp[2].item())

    def get_growth_factor(self):
        return self._growth_factor

    def get_backoff_factor(self):
        return self._backoff_factor

    def get_growth_interval(self):
        return self._growth_interval

    def state_dict(self):
        if not self._enabled:
            return {}
        return {"scale": self.get_scale(), "growth_factor": self._growth_factor, "backoff_factor": self._backoff_factor,
                "growth_interval": self._growth_interval, "_growth_tracker": self._get_growth_tracker()}

    def load_state_dict(self, state_dict):
        if not self._enabled:
            return
        if len(state_dict) == 0:
            raise RuntimeError("The source state dict is empty, possibly because it was saved from a disabled instance of GradScaler.")
        self._init_scale, self._init_tracker = float(state_dict["scale"]), int(state_dict["_growth_tracker"])
        self._growth_factor, self._backoff_factor = float(state_dict["growth_factor"]), float(state_dict["backoff_factor"])
        self._growth_interval = int(state_dict["growth_interval"])
        if self._amp is not None:
            self._amp = self._make(self._amp.device)


# -------------------------------------------------------------------------------------------------------------------- the EMA
class ModelEMA:
    """The reference's ``ModelEMA`` (``yolov6/utils/ema.py``): ``.ema`` a frozen copy of the model in eval mode, ``.updates``,
    ``.decay``.  ``update(model)`` is one ``evrep_ema_update`` launch over all floating entries of the state dict; integer
    entries are left alone.  Inside a ``TrainStep`` the update rides in the step's apply launch instead."""

    def __init__(self, model, decay=0.9999, updates=0):
        self._table, self._hyper = None, _Hyper()
        self.updates = updates
        self.decay = functools.partial(ema_decay, decay=decay)          # updates -> this step's decay
        self.ema = deepcopy(_bare(model))
        self.ema.eval().requires_grad_(False)

    @property
    def table_uploads(self):
        return 0 if self._table is None else self._table.uploads

    def invalidate(self):
        """Have the next ``update`` list the entries anew (after ``.ema`` was given new tensors that no address shows)."""
        if self._table is not None:
            self._table.invalidate()

    def update(self, model):
        self.updates += 1
        row = hyper_row((), self.decay(self.updates))
        if self._table is None or self._table.model is not model:
            self._table = _StepTable(None, self, model)
        table = self._table
        table.ensure()
        if table.device is None:
            return
        with torch.no_grad():
            if table.device.type != "cuda":
                step_host(table.host_rows(), row, None, ema_only=True)
                return
            self._hyper.upload(row, table.device)
            with torch.cuda.device(table.device):
                _lib.api().evrep_ema_update(_lib.ptr(table.tensors_dev), table.n_tensors, _lib.ptr(table.chunks_dev), table.n_chunks,
                                            _lib.ptr(self._hyper.dev), _lib.stream_ptr())

    def update_attr(self, model, include=(), exclude=("process_group", "reducer")):
        """Hand the model's public instance attributes on to ``.ema``: those named in ``include`` (all of them when it is empty),
        without the ones in ``exclude``."""
        public = {name: value for name, value in vars(model).items() if not name.startswith("_") and name not in exclude}
        for name in (include if include else public):
            if name in public:
                setattr(self.ema, name, public[name])


# --------------------------------------------------------------------------------------------------------------- the one call
class TrainStep:
    """``engine.py:548-552`` as one call: ``TrainStep(optimizer, scaler, ema)(model)`` raises ``ema.updates``, forms the decay,
    refreshes the hyper row (one asynchronous copy) and calls ``evrep_train_step`` once.  ``scaler`` and ``ema`` may be None.

    Under stream capture ``__call__`` only launches: call ``refresh(model)`` before the capture and before every replay."""

    def __init__(self, optimizer, scaler=None, ema=None):
        if not isinstance(optimizer, SGD):
            raise TypeError("TrainStep takes detector_step.SGD (build_optimizer), got %s" % type(optimizer).__name__)
        if scaler is not None and not isinstance(scaler, GradScaler):
            raise TypeError("TrainStep takes detector_step.GradScaler, got %s" % type(scaler).__name__)
        self.optimizer, self.scaler, self.ema = optimizer, scaler, ema
        self._table = None

    @property
    def table_uploads(self):
        return (self._table or self.optimizer._table).uploads

    def _table_for(self, model):
        if self.ema is None:
            return self.optimizer._table
        if self._table is None or self._table.model is not model:
            names = {id(p): k for k, p in _entries(model).items()}
            self.optimizer._names.update(names)
            self._table = _StepTable(self.optimizer, self.ema, model)
        return self._table

    def refresh(self, model):
        """What a step does on the host: ``ema.updates += 1``, the hyper row's upload, the tables' comparison."""
        decay = None
        if self.ema is not None:
            self.ema.updates += 1
            decay = self.ema.decay(self.ema.updates)
        opt, table = self.optimizer, self._table_for(model)
        table.ensure()
        opt._row = hyper_row(opt.param_groups, decay)
        if table.device is not None:
            # the state words are made HERE, never by a launch: an allocation captured into a graph would run again on every
            # replay and set applied_steps back to 0
            opt._applied_on(table.device)
            if self.scaler is not None and self.scaler.is_enabled():
                self.scaler._state_on(table.device)
            if table.device.type == "cuda":
                opt._hyper.upload(opt._row, table.device)

    def invalidate(self):
        """Have the next step list the tensors anew (see ``SGD.invalidate``)."""
        if self._table is not None:
            self._table.invalidate()
        self.optimizer.invalidate()

    @torch.no_grad()
    def __call__(self, model):
        table = self._table_for(model)
        capturing = table.device is not None and table.device.type == "cuda" and torch.cuda.is_current_stream_capturing()
        if not capturing:
            self.refresh(model)
        elif table.sig is None:
            raise RuntimeError("TrainStep under capture: call refresh(model) before the capture begins")
        self.optimizer._launch(scaler=self.scaler, table=table, refresh=False)
        if self.scaler is not None:
            self.scaler._stepped = False
