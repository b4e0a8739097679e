"""Device-resident batch engine: the fast path of the package.

A :class:`EventBatch` holds B windows of events as one concatenated ``(total, 4)`` int32 tensor
plus ``B+1`` offsets in HBM, runs the (y,x) binning pass once, and then builds any number of
representations from the binned stream -- all on the caller's HIP stream, no host sync.

The per-sample functions that mirror the reference's Python names
(``representations/*.py``) are thin wrappers over this class with B = 1.
"""
import contextlib
import ctypes
import weakref

import numpy as np
import torch

from . import _lib
from ._lib import Plan, want
from ._lib import ptr as _ptr, require_gpu as _require_gpu, stream_ptr as _stream_ptr

_NO_GUARD = contextlib.nullcontext()


class EventBatch:
    """B event windows resident on one GPU.

    events  : (total, 4) int32 cuda tensor, rows [x, y, t, p], each window time-sorted
    offsets : (B+1,) int64 tensor (host or device); window b = rows [offsets[b], offsets[b+1])
    plan_flags : _lib.PLAN_* bits (None: from the EVREP_BIN_* environment switches of the tests and A/B tools)
    pacing  : store pacing of the wide float64 builders, see evrep_plan_set_pacing (None: EVREP_PACING or automatic)
    """

    def __init__(self, events, offsets, height, width, max_events_per_window=None, plan_flags=None, pacing=None):
        _require_gpu()
        self.lib, self.api = _lib.load(), _lib.api()      # .lib: the raw C ABI (bench.py, tests, tools); .api: what this package calls
        self.events = want(events.contiguous(), "events", torch.int32, (None, 4), device="cuda")
        self.device = events.device
        off_host = offsets.detach().cpu().to(torch.int64) if isinstance(offsets, torch.Tensor) else \
            torch.as_tensor(np.asarray(offsets, dtype=np.int64))
        if max_events_per_window is None:
            max_events_per_window = int((off_host[1:] - off_host[:-1]).max().item()) if off_host.numel() > 1 else 0
        self.offsets_host = off_host
        self.offsets = off_host.to(self.device)
        self.B = int(off_host.numel() - 1)
        self.H, self.W = int(height), int(width)
        self.total = int(self.events.shape[0])
        self.plan = Plan()
        flags = _lib.plan_flags_from_env() if plan_flags is None else int(plan_flags)
        self.api.evrep_plan_init_ex(ctypes.byref(self.plan), self.B, self.H, self.W, self.total, int(max_events_per_window), flags)
        pacing = _lib.pacing_from_env() if pacing is None else int(pacing)
        if pacing is not None:
            self.api.evrep_plan_set_pacing(ctypes.byref(self.plan), pacing)
        self.workspace = _lib.scratch(self.api.evrep_workspace_bytes(ctypes.byref(self.plan)), self.device)
        self._binned = False
        self.t_base = None      # numpy int64 (B,): absolute time of t == 0 per window, set by DeviceRecording.windows; no builder reads it
        # The per-sample wrappers (representations/_common.py) keep one pooled batch per (host thread, device, stream) and only use
        # it there: they pin the stream pointer and skip the device guard (torch.cuda.current_stream() + torch.cuda.device() cost
        # ~8 us per call of the ~100 us a sample takes).  None: look both up per call, as every other user must.
        self._pinned_stream = None

    def _sp(self):
        return self._pinned_stream if self._pinned_stream is not None else _stream_ptr()

    def _dev(self):
        return _NO_GUARD if self._pinned_stream is not None else torch.cuda.device(self.device)

    # ------------------------------------------------------------------ construction helpers
    @classmethod
    def from_numpy(cls, windows, height, width, device="cuda:0"):
        """windows: list of (n_b, 4) int32 arrays (or one array) -> device batch."""
        _require_gpu()
        if isinstance(windows, np.ndarray):
            windows = [windows]
        ws = [np.ascontiguousarray(w, dtype=np.int32).reshape(-1, 4) for w in windows]
        offs = np.zeros(len(ws) + 1, dtype=np.int64)
        np.cumsum([w.shape[0] for w in ws], out=offs[1:])
        cat = np.concatenate(ws, axis=0) if ws else np.zeros((0, 4), np.int32)
        ev = torch.from_numpy(cat).to(device)
        if ev.shape[0] == 0:
            ev = torch.zeros((0, 4), dtype=torch.int32, device=device)
        return cls(ev, torch.from_numpy(offs), height, width)

    def _args(self):
        return ctypes.byref(self.plan), _ptr(self.events), _ptr(self.offsets), _ptr(self.workspace)

    def _launch(self, fn, *args):
        """fn(plan, events, offsets, workspace, *args, stream) with the batch's device current."""
        with self._dev():
            return fn(*self._args(), *args, self._sp())

    def bin(self):
        """Run the (y,x) binning pass (idempotent)."""
        if not self._binned:
            self._launch(self.api.evrep_bin_events)
            self._binned = True
        return self

    def rebin(self):
        self._binned = False
        return self.bin()

    # ------------------------------------------------------------------ read-backs (sync)
    def status(self):
        self.bin()
        st = np.zeros(self.B, dtype=np.uint32)
        with self._dev():
            self.api.evrep_read_status(ctypes.byref(self.plan), _ptr(self.workspace), st.ctypes.data, self._sp())
        return st

    def check_built(self, what="builder"):
        """After a builder call (one synchronisation): raise if a builder kernel set EVREP_ST_HOT_OVERFLOW -- the
        workspace's hot-unit list filled up and a unit was left unwritten.  The builders are asynchronous and the flag is
        raised BY the builder launch, so it can only be seen after it; the per-sample wrappers (`finish`) read it with the
        result, batched callers call this where they synchronise anyway.  Returns the status words."""
        from ._lib import EvrepError, ST_HOT_OVERFLOW
        st = self.status()
        if any(int(v) & ST_HOT_OVERFLOW for v in st):
            raise EvrepError("%s: the workspace's hot-unit list overflowed (EVREP_ST_HOT_OVERFLOW): the tensor is incomplete" % what)
        return st

    def bbox(self):
        self.bin()
        bb = np.zeros((self.B, 4), dtype=np.int32)
        with self._dev():
            self.api.evrep_read_bbox(ctypes.byref(self.plan), _ptr(self.workspace), bb.ctypes.data, self._sp())
        return bb

    # ------------------------------------------------------------------ builders
    def _out(self, out, C, dtype):
        shape = (self.B, self.H, self.W, C)
        if out is None:
            return torch.empty(shape, dtype=dtype, device=self.device)
        return want(out, "out", dtype, shape, device=self.device)

    @staticmethod
    def _dt(dtype):
        if dtype == torch.float64:
            return _lib.F64
        if dtype == torch.float32:
            return _lib.F32
        raise ValueError("dtype must be torch.float64 or torch.float32")

    def sbt_windows(self):
        """The eight "SBT" windows of every window of the batch as rank ranges + their flags (device tensors).  Formed per
        call: a pooled batch is refilled with other events between calls."""
        bounds = torch.empty((self.B, 8, 2), dtype=torch.int32, device=self.device)
        flags = torch.empty((self.B, 2), dtype=torch.int32, device=self.device)
        with self._dev():
            self.api.evrep_mdes_sbt_windows(_ptr(self.events), _ptr(self.offsets), self.B, self.H, self.W, _ptr(bounds), _ptr(flags),
                                            self._sp())
        return bounds, flags

    def mdes(self, windows, funcs, aggs, scale=1.0, dtype=torch.float64, out=None, stacking="SBN"):
        """MixedDensityEventStack.stack for every window -> (B, H, W, C).  ``None`` entries give the
        reference's failed-channel zeros.  More than 16 channels are built 16 at a time.
        stacking "SBN": windows 0..6 cut by event count (the reference's choice); "SBT": windows 0..7 cut by time."""
        if stacking not in ("SBN", "SBT"):
            raise ValueError("stacking_type %r" % (stacking,))
        self.bin()
        C = len(windows)
        w = [-1 if v is None else int(v) for v in windows]
        f = [-1 if v is None else (_lib.FUNCS.index(v) if isinstance(v, str) else int(v)) for v in funcs]
        a = [-1 if v is None else (_lib.AGGS.index(v) if isinstance(v, str) else int(v)) for v in aggs]
        if C <= _lib.MAX_CHANNELS:
            out = self._out(out, C, dtype)
            bounds, flags = self.sbt_windows() if stacking == "SBT" else (None, None)
            self._launch(self.api.evrep_mdes_ex, C, _lib.int32_array(w), _lib.int32_array(f), _lib.int32_array(a), float(scale),
                         self._dt(dtype), _ptr(out), _ptr(bounds), _ptr(flags))
            return out
        parts = [self.mdes(w[i:i + 16], f[i:i + 16], a[i:i + 16], scale, dtype, stacking=stacking) for i in range(0, C, 16)]
        res = torch.cat(parts, dim=3)
        if out is not None:
            out.copy_(res)
            return out
        return res

    def optimized(self, scale=1.0, dtype=torch.float64, out=None):
        """get_optimized_representation (ERGO-12) for every window -> (B, H, W, 12)."""
        self.bin()
        out = self._out(out, 12, dtype)
        self._launch(self.api.evrep_optimized, float(scale), self._dt(dtype), _ptr(out))
        return out

    def event_stack(self, stack_size=12, premap=True, scale=1.0, out=None):
        """EventStack levels -> (B, H, W, stack_size) float32.  premap True/1: p -> (p + 1) // 2 first (the
        dispatcher, gen1_transforms.py:34); False/0: p is {0, 1}, the kernel forms 2p - 1; 2: the p column
        already holds the final int8 polarity value (EventStack.pre_stack forms it on the host)."""
        self.bin()
        out = self._out(out, stack_size, torch.float32)
        self._launch(self.api.evrep_event_stack, int(stack_size), int(premap), float(scale), _ptr(out))
        return out

    def _i32_dev(self, values, per_window):
        """None -> None; else a (B, per_window) int32 device tensor (a list is taken as one row per window)."""
        if values is None:
            return None
        t = torch.as_tensor(np.asarray(values, dtype=np.int32)).reshape(-1)
        if t.numel() == per_window and self.B > 1:
            t = t.repeat(self.B)
        if t.numel() != self.B * per_window:
            raise ValueError("expected %d x %d int32 values" % (self.B, per_window))
        return t.to(self.device)

    def _per_event(self, t, what, dtype=torch.float64):
        return want(t, what, dtype, numel=self.total, device=self.device)

    def time_surface(self, slices=6, tau=50000.0, premap=True, scale=1.0, dtype=torch.float64, out=None, indices=None, times_f64=None):
        """ToTimesurface for every window -> (B, H, W, 2*slices), channel c = 2*s + p.  indices=None: the
        dispatcher's cuts searchsorted(t_norm, 1..slices); else explicit event indices per window.
        premap: True / 1 = p -> int8((p+1)/2) first; + 2 = timestamps not ascending (array-order scan, per-slice exponentials;
        needs explicit indices)."""
        self.bin()
        out = self._out(out, 2 * slices, dtype)
        idx = self._i32_dev(indices, slices)
        if times_f64 is not None:      # float64 timestamps, one per event (the events' own t column then only orders them)
            self._per_event(times_f64, "times_f64")
            if indices is None:
                raise ValueError("times_f64 needs explicit indices")
        self._launch(self.api.evrep_time_surface_ftime, int(slices), _ptr(idx), _ptr(times_f64), float(tau), int(premap),
                     float(scale), self._dt(dtype), _ptr(out))
        return out

    def tore(self, k=6, frame_mode=0, scale=1.0, out=None, sample_times=None, times_f64=None, sample_times_f64=None):
        """TORE.  frame_mode 0 (bounding box, the gen1/gen4 dispatcher's behaviour) returns a list of
        per-window (Hbb, Wbb, 2k) views (needs one host sync for the boxes); modes 1/2 return
        (B, H, W, 2k).  Mode 0 gives a (0, 0, 2k) view for an empty window AND for a window whose out-of-frame events
        stretch its box beyond H x W (nothing is written for either): ``status()`` tells them apart, ST_EMPTY against
        ST_OOB -- a batched caller that must not take the second for the first reads it.  sample_times_f64 (with times_f64): one
        float64 sample time per window, as a host sequence or as a (B,) float64 tensor already on the batch's device."""
        self.bin()
        out = self._out(out, 2 * k, torch.float32)
        st, st_f = self._i32_dev(sample_times, 1), None
        if sample_times_f64 is not None and times_f64 is None:
            # the C ABI rejects the pair (EINVAL); silently falling back to the int32 sample times would return a
            # plausible but different tensor
            raise ValueError("sample_times_f64 needs times_f64 (float64 event times)")
        if times_f64 is not None:      # float64 timestamps, one per event (the events' own t column is then not used)
            self._per_event(times_f64, "times_f64")
            if isinstance(sample_times_f64, torch.Tensor) and sample_times_f64.is_cuda:
                # made on the device (evrep_nimg_study_rows): taken as it lies, nothing crosses to the host and back
                st_f = want(sample_times_f64, "a device sample_times_f64", torch.float64, (self.B,), device=self.device)
            elif sample_times_f64 is not None:
                st_f = torch.as_tensor(np.asarray(sample_times_f64, dtype=np.float64)).reshape(-1).to(self.device)
                if st_f.numel() != self.B:
                    raise ValueError("sample_times_f64 must hold one time per window")
        self._launch(self.api.evrep_tore_ftime, int(k), int(frame_mode), _ptr(st), _ptr(times_f64), _ptr(st_f), float(scale), _ptr(out))
        if frame_mode != 0:
            return out
        bb = self.bbox()
        views = []
        for b in range(self.B):
            hb, wb = int(bb[b, 3]) - int(bb[b, 1]) + 1, int(bb[b, 2]) - int(bb[b, 0]) + 1
            if hb <= 0 or wb <= 0:                      # an empty window has no bounding box: an empty frame
                hb = wb = 0
            if hb > self.H or wb > self.W:              # out-of-frame events (ST_OOB) stretched the box beyond the frame: the
                hb = wb = 0                             # compact array does not fit the window's slice and is not written
            flat = out[b].reshape(-1)
            views.append(flat[: hb * wb * 2 * k].view(hb, wb, 2 * k))
        return views

    def voxel(self, bins=5, mode=0, scale=1.0, out=None, t_range=None):
        """Voxel grids -> (B, H, W, bins) float64.  mode 0: compute_repr; 1: tonic ToVoxelGrid; 2: ev-licious
        events_to_voxel_grid (t_range: optional (B, 2) int64 [t0_us, t1_us] per window, mode 2 only)."""
        self.bin()
        out = self._out(out, bins, torch.float64)
        tr = self._t_range(t_range)
        self._launch(self.api.evrep_voxel_range, int(bins), int(mode), float(scale), _ptr(tr), _ptr(out))
        return out

    def _t_range(self, t_range):
        """None -> None; else the (B, 2) int64 [t0_us, t1_us] per window as a flat device tensor."""
        if t_range is None:
            return None
        tr = torch.as_tensor(np.asarray(t_range, dtype=np.int64)).reshape(-1)
        if tr.numel() != 2 * self.B:
            raise ValueError("t_range must hold (t0, t1) for each of the %d windows" % self.B)
        return tr.to(self.device)

    def voxel_tnorm(self, tnorm, bins=5, scale=1.0, out=None):
        """compute_repr with the caller's own normalised time (gromov_wasserstein.py:72-82) -> (B, H, W, bins) float64.
        tnorm: float64 device tensor, one value per event (indexed like the events)."""
        self.bin()
        self._per_event(tnorm, "tnorm")
        out = self._out(out, bins, torch.float64)
        self._launch(self.api.evrep_voxel_tnorm, _ptr(tnorm), int(bins), float(scale), _ptr(out))
        return out

    def voxel_subpixel(self, xy, bins=5, t_range=None, out=None):
        """ev-licious events_to_voxel_grid for sub-pixel coordinates -> (B, H, W, bins) float32.  The batch holds the
        truncated coordinates; xy: (total, 2) float64 device tensor with every event's original (x, y)."""
        self.bin()
        want(xy, "xy", torch.float64, (self.total, 2), device=self.device)
        out = self._out(out, bins, torch.float32)
        tr = self._t_range(t_range)
        self._launch(self.api.evrep_voxel_subpixel, _ptr(xy), int(bins), _ptr(tr), _ptr(out))
        return out

    def evl_voxel_grid(self, num_bins, normalize=True, t_range=None, xy=None, out=None, return_stats=False):
        """ev-licious events_to_voxel_grid for every window -> (B, num_bins, H, W) float32, channel first, standardised over each
        window's non-zero entries when `normalize` (utils.py:51-85; evrep_voxel_normalize).  xy=None: the integer-pixel grid
        (voxel mode 2); xy = (total, 2) float64 device tensor of the original coordinates: the sub-pixel grid (voxel_subpixel).
        return_stats: also the (B, 4) float64 device tensor {n, mean, std, applied} per window (needs normalize).  Nothing is
        read back: the call stays on the batch's stream."""
        _require_gpu()
        bins = int(num_bins)
        shape = (self.B, bins, self.H, self.W)
        _check_evl_out(out, shape, self.device)           # before anything is launched
        if return_stats and not normalize:
            raise ValueError("the statistics come with the normalisation: return_stats needs normalize=True")
        if xy is None:
            grid = self.voxel(bins=bins, mode=2, t_range=t_range)
        else:
            grid = self.voxel_subpixel(xy, bins=bins, t_range=t_range)
        with self._dev():
            return voxel_normalize(grid, normalize=normalize, out=out, return_stats=return_stats, stream=self._sp())

    def polstats(self, tnorm, pol, stat, tau=0.3, out=None):
        """n_imagenet's per-polarity accumulators (imagenet.py:169-511): channel c = stat[c] over the events of
        polarity class pol[c] at each pixel.  tnorm: float64 device tensor, one normalised time per event."""
        self.bin()
        pol = np.ascontiguousarray(pol, dtype=np.int32)
        stat = np.ascontiguousarray(stat, dtype=np.int32)
        if pol.shape != stat.shape or pol.ndim != 1:
            raise ValueError("pol and stat must be 1-D and of equal length")
        self._per_event(tnorm, "tnorm")
        out = self._out(out, len(pol), torch.float32)
        self._launch(self.api.evrep_polstats, _ptr(tnorm), len(pol), pol.ctypes.data, stat.ctypes.data, float(tau), _ptr(out))
        return out

    def _est_inputs(self, tnorm, segments, buckets):
        self._per_event(tnorm, "tnorm", torch.float32)
        want(segments, "segments", torch.float64, (None, 3), device=self.device)
        want(buckets, "buckets", torch.int32, device=self.device)

    def est_voxel(self, tnorm, C, segments, buckets, lo, hi, out=None):
        """EST quantisation layer forward (learned_repr.py:143-179) -> (B, H, W, 2C) float32; the value MLP is
        passed as its piecewise-linear table (est.PiecewiseLinearKernel.device_table)."""
        self.bin()
        self._est_inputs(tnorm, segments, buckets)
        out = self._out(out, 2 * int(C), torch.float32)
        self._launch(self.api.evrep_est_voxel, _ptr(tnorm), int(C), _ptr(segments), int(segments.shape[0]), _ptr(buckets),
                     int(buckets.numel()), float(lo), float(hi), _ptr(out))
        return out

    def est_voxel_backward(self, tnorm, C, segments, buckets, lo, hi, grad_out):
        """The gradient of a loss with respect to the (a, c) columns of the table ``est_voxel`` was called with, from
        ``grad_out`` = dL/d est_voxel (B, H, W, 2C) float32 contiguous -> (nseg, 2) float64 {dL/da, dL/dc}.  A keyed
        float64 reduction over the events in array order (no binning pass); bit-reproducible between calls."""
        self._est_inputs(tnorm, segments, buckets)
        nseg = int(segments.shape[0])
        if not 1 <= nseg <= _lib.EST_BWD_MAX_SEG:
            raise ValueError("the table has %d pieces; the backward holds at most EVREP_EST_BWD_MAX_SEG = %d"
                             % (nseg, _lib.EST_BWD_MAX_SEG))
        want(grad_out, "grad_out", torch.float32, (self.B, self.H, self.W, 2 * int(C)), device=self.device)
        grad = torch.empty((nseg, 2), dtype=torch.float64, device=self.device)
        if self.total == 0:
            return grad.zero_()
        scratch = _lib.scratch(self.api.evrep_est_backward_scratch_bytes(self.total, nseg), self.device)
        with self._dev():
            self.api.evrep_est_voxel_backward(_ptr(self.events), _ptr(self.offsets), self.B, self.H, self.W, _ptr(tnorm), int(C),
                                              _ptr(segments), nseg, _ptr(buckets), int(buckets.numel()), float(lo), float(hi),
                                              _ptr(grad_out), _ptr(grad), _ptr(scratch), self._sp())
        return grad

    # ------------------------------------------------------------------ event filters (ev-licious tools/filters.py)
    # Each filter returns (keep, state): keep = (total,) uint8 device tensor, one byte per event in array order; state = the
    # reference's per-pixel state array as a (B, H, W) device tensor, updated IN PLACE when it was handed in -- hand it to
    # the next window of the same recording to carry the filter on.  No call waits for the device; with t_base the copy of the
    # window time bases (B * 8 bytes of pageable host memory) is staged by the HIP runtime before the call returns.
    def _filter_state(self, state, dtype, fill):
        shape = (self.B, self.H, self.W)
        if state is None:
            return torch.full(shape, fill, dtype=dtype, device=self.device)
        return want(state, "state", dtype, shape, device=self.device)

    def _t_base(self, t_base):
        """None -> NULL; else one absolute int64 time per window (a scalar serves every window), kept alive on the batch."""
        if t_base is None:
            self._t_base_host = None
            return None
        tb = np.ascontiguousarray(np.broadcast_to(np.asarray(t_base, dtype=np.int64).reshape(-1), (self.B,)))
        self._t_base_host = tb
        return tb.ctypes.data

    def _filter_fsm(self, kind, param, state, dtype, fill, t_base=None):
        if not float(param) > 0:
            raise ValueError("the filter parameter must be positive")
        self.bin()
        state = self._filter_state(state, dtype, fill)
        keep = torch.empty(self.total, dtype=torch.uint8, device=self.device)
        self._launch(self.api.evrep_filter_pixel_fsm, int(kind), float(param), self._t_base(t_base), _ptr(state), _ptr(keep))
        return keep, state

    def filter_refractory(self, period, state=None, t_base=None):
        """RefractoryPeriod (utils.py:193-200): an event passes iff t - last >= period; only a passing event sets last.
        state: (B, H, W) float64 absolute times, -inf at rest; t_base: absolute time of t == 0 of every window's t column."""
        return self._filter_fsm(_lib.FILTER_REFRACTORY, period, state, torch.float64, -np.inf, t_base)

    def filter_contrast(self, factor, state=None):
        """ContrastThresholdIncrease (utils.py:184-191): activity += p; passes iff |activity| >= factor, then activity = 0.
        state: (B, H, W) int32.  p must be in {-1, +1}, as in the reference's Events."""
        return self._filter_fsm(_lib.FILTER_CONTRAST, factor, state, torch.int32, 0)

    def filter_background(self, depth_us, radius, state=None, t_base=None):
        """BackgroundActivity (utils.py:170-179), 1 <= radius <= 4.  state: (B, H, W) float64 = the reference's `timestamps`."""
        self.bin()
        state = self._filter_state(state, torch.float64, -np.inf)
        keep = torch.empty(self.total, dtype=torch.uint8, device=self.device)
        self._launch(self.api.evrep_filter_background, float(depth_us), int(radius), self._t_base(t_base), _ptr(state), _ptr(keep))
        return keep, state

    def filter_resize(self, height, width, state=None):
        """resize_to_resolution's event selection (utils.py:110-158) -> (keep, state, cells): cells = a new EventBatch of
        the SAME events with the coordinates (x // fx, y // fy) on the (H // fy) x (W // fx) sensor, so
        ``cells.compacted(keep)`` is the down-sampled stream.  state: (B, H // fy, W // fx) float32 change map."""
        fx, fy = int(self.W / int(width)), int(self.H / int(height))
        if fx < 1 or fy < 1 or self.W % fx or self.H % fy or self.W // fx != int(width) or self.H // fy != int(height):
            raise ValueError("the sensor %dx%d is not %dx%d whole cells of %dx%d pixels (the reference's change map is "
                             "(height, width): it raises IndexError)" % (self.W, self.H, int(width), int(height), fx, fy))
        ev = torch.empty_like(self.events)
        if self.total:
            with self._dev():
                self.api.evrep_filter_cell_map(_ptr(self.events), self.total, self.H, self.W, fy, fx, _ptr(ev), self._sp())
        cells = EventBatch(ev, self.offsets_host, self.H // fy, self.W // fx,
                           max_events_per_window=int(self.plan.max_events_per_window), plan_flags=int(self.plan.flags))
        cells._pinned_stream = self._pinned_stream
        keep, state = cells._filter_fsm(_lib.FILTER_CHANGE_MAP, fx * fy, state, torch.float32, 0.0)
        return keep, state, cells

    def filter_mask(self, mask):
        """HotPixel.insert (filters.py:53): keep[i] = mask[b, y, x].  mask: (B, H, W) or (H, W) bool / uint8 device tensor."""
        m = mask.to(self.device)
        if m.dtype != torch.uint8:          # (the kernel reads any non-zero byte as True)
            m = m.ne(0).to(torch.uint8)
        if m.dim() == 2:
            m = m.unsqueeze(0).expand(self.B, -1, -1)
        m = m.contiguous()
        if tuple(m.shape) != (self.B, self.H, self.W):
            raise ValueError("mask must be (B, H, W) or (H, W)")
        keep = torch.empty(self.total, dtype=torch.uint8, device=self.device)
        if self.total:
            with self._dev():
                self.api.evrep_filter_mask_gather(_ptr(self.events), _ptr(self.offsets), self.B, self.H, self.W,
                                                  int(self.plan.max_events_per_window), _ptr(m), _ptr(keep), self._sp())
        return keep, m

    def render(self, rendering_type=1, cast=True, rendering=None, check=True, out=None):
        """ev-licious' Events.render for every window -> (B, H, W, 3) uint8 frames, colours in the reference's channel order as
        stored; RenderingType.TIME_SURFACE: (B, H, W, 4) float64 RGBA, a window of <= 2 events an all-zero slot (alpha included).
        rendering_type: evlicious_render.RenderingType (default RED_BLUE_OVERLAP).  cast=False: the 2 x 2 jitter of the three
        colour types (EVENT_FRAME and TIME_SURFACE ignore it, as the reference).  rendering: the canvas the colour types draw
        onto, a device or host uint8 (H, W, 3) or (B, H, W, 3); None: white; anything else ``ValueError``.
        check=True reads the status words once and raises ``ValueError`` naming the first window with rows outside the frame (the
        Events constructor refuses them); check=False reads nothing back and returns (images, status), status a (B,) uint32
        device tensor of _lib.ST_* bits: such a window is drawn from its in-frame events."""
        from . import evlicious_render
        return evlicious_render.render_batch(self, rendering_type, cast=cast, rendering=rendering, check=check, out=out)

    def pixel_counts(self):
        """Events per pixel -> (B, H, W) float32 (the COUNT accumulator of evrep_polstats; HotPixel.calibrate's np.add.at)."""
        tn = torch.zeros(self.total, dtype=torch.float64, device=self.device)
        return self.polstats(tn, [0], [0])[..., 0]

    def compacted(self, keep):
        """The kept rows of every window, in order, as a new EventBatch on the same device and stream (ready for
        .optimized() / .tore() / ...).  The compaction and the new offsets are formed on the device; ONE host
        synchronisation follows: the read of the new offsets, which sizes the new batch's plan."""
        self._per_event(keep, "keep", torch.uint8)
        off_out = torch.zeros(self.B + 1, dtype=torch.int64, device=self.device)
        ev_out = torch.empty((max(self.total, 1), 4), dtype=torch.int32, device=self.device)
        if self.total:
            scratch = _lib.scratch(self.api.evrep_filter_compact_scratch_bytes(self.B, self.total), self.device)
            with self._dev():
                self.api.evrep_filter_compact(_ptr(self.events), _ptr(self.offsets), self.B, _ptr(keep), _ptr(ev_out), _ptr(off_out),
                                              _ptr(scratch), self._sp())
        off_host = off_out.cpu()
        out = EventBatch(ev_out[: int(off_host[-1])], off_host, self.H, self.W, plan_flags=int(self.plan.flags))
        out._pinned_stream = self._pinned_stream
        return out


def _check_evl_out(out, shape, device):
    if out is not None:
        want(out, "out", torch.float32, shape, device=device)


def voxel_normalize(grid, normalize=True, out=None, return_stats=False, stream=None):
    """evrep_voxel_normalize: a contiguous (B, H, W, bins) float64 / float32 device tensor of channel-last voxel grids ->
    (B, bins, H, W) float32, each window standardised over its non-zero entries when `normalize` (ev-licious utils.py:77-83),
    else only cast and transposed.  return_stats: also (B, 4) float64 {n, mean, std, applied}.  Three launches on the current
    stream (`stream`: a stream pointer the caller has pinned), no read-back."""
    _require_gpu()
    api = _lib.api()
    want(grid, "grid", (torch.float64, torch.float32), (None, None, None, None), device="cuda")
    B, H, W, bins = (int(v) for v in grid.shape)
    _check_evl_out(out, (B, bins, H, W), grid.device)
    if return_stats and not normalize:
        raise ValueError("the statistics come with the normalisation: return_stats needs normalize=True")
    dt = EventBatch._dt(grid.dtype)
    if out is None:
        out = torch.empty((B, bins, H, W), dtype=torch.float32, device=grid.device)
    stats = torch.empty((B, 4), dtype=torch.float64, device=grid.device) if return_stats else None
    scratch = _lib.scratch(max(api.evrep_voxel_normalize_scratch_bytes(B, H, W, bins), 16), grid.device) if normalize else None
    with torch.cuda.device(grid.device) if stream is None else _NO_GUARD:
        api.evrep_voxel_normalize(_ptr(grid), dt, B, H, W, bins, _lib.VOXNORM_NORMALIZE if normalize else 0, _ptr(out), _ptr(stats),
                                  _ptr(scratch), _stream_ptr() if stream is None else stream)
    return (out, stats) if return_stats else out


def est_prepare(events5, B, H, W):
    """evrep_est_prepare: the EST layer's ``(n, 5)`` float32 CUDA rows [x, y, t, p, b] (contiguous, n > 0, grouped by b) ->
    ``(rows, offsets, tnorm, status, packed)`` on the same device: rows (n, 4) int32 {x, y, 0, p}, offsets (B + 1,) int64, tnorm
    (n,) float32 = t / t.max() per item, status (1,) int32 holding the EVREP_EST_PREP_* bits.  offsets and status are views of
    ``packed``, (B + 2,) int64 (status is the low half of its last word), so one small copy brings both to the host.
    Asynchronous on the current stream: nothing is read back here."""
    _require_gpu()
    api = _lib.api()
    want(events5, "events5", torch.float32, (None, 5), device="cuda")
    n, B, dev = int(events5.shape[0]), int(B), events5.device
    if n == 0:
        raise ValueError("events5 must be non-empty")
    nbytes = api.evrep_est_prepare_scratch_bytes(n, B)
    if nbytes == 0:
        raise ValueError("1 <= B <= %d batch items, got %d" % (_lib.EST_PREP_MAX_B, B))
    rows = torch.empty((n, 4), dtype=torch.int32, device=dev)
    tnorm = torch.empty(n, dtype=torch.float32, device=dev)
    packed = torch.empty(B + 2, dtype=torch.int64, device=dev)
    scratch = _lib.scratch(nbytes, dev)
    offsets, status = packed[:B + 1], packed[B + 1:].view(torch.int32)[:1]
    with torch.cuda.device(dev):
        api.evrep_est_prepare(_ptr(events5), n, B, int(H), int(W), _ptr(rows), _ptr(offsets), _ptr(tnorm), _ptr(status), _ptr(scratch),
                              _stream_ptr())
    return rows, offsets, tnorm, status, packed


class BinBuildPipeline:
    """Throughput path for a STREAM of batches: the binning pass of batch k+1 runs on a side HIP stream
    while the builder of batch k runs on the caller's stream (the binning kernels are latency-bound and
    barely touch HBM, the builders are HBM-bound, so they overlap almost for free).  Each EventBatch
    owns its workspace, so two batches in flight = double buffering.

        pipe = BinBuildPipeline(device)
        for batch, out in work:              # e.g. alternating between two resident batches
            pipe.submit(batch, lambda b: b.optimized(out=out))
        pipe.drain()

    A batch's events may be refilled (on the caller's stream) once its build has been issued, i.e. after the
    submit() that followed its own; they must not change while its build is still pending.
    """

    def __init__(self, device=None):
        _require_gpu()
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.bin_stream = torch.cuda.Stream(device=self.device)
        self._pending = None          # (batch, build_fn, binned_event)
        # batch -> event recorded after the last build that read its workspace; weak keys: a recycled id() of a
        # collected batch must not hand its event to an unrelated new batch
        self._built = weakref.WeakKeyDictionary()

    def _start_bin(self, batch):
        main = torch.cuda.current_stream(self.device)
        done = self._built.get(batch)
        with torch.cuda.stream(self.bin_stream):
            # the caller may have (re)filled batch.events on its own stream since the last build: ALWAYS order the
            # binning pass behind the caller's stream, and behind the last build that read this workspace
            self.bin_stream.wait_stream(main)
            if done is not None:
                self.bin_stream.wait_event(done)
            batch.rebin()
            ev = torch.cuda.Event()
            ev.record(self.bin_stream)
        return ev

    def submit(self, batch, build_fn):
        """Queue `batch`: its binning starts now on the side stream; the PREVIOUS submission is built now.
        Submitting the batch that is still pending builds it first (its workspace cannot be re-binned while a
        build of it is outstanding)."""
        if self._pending is not None and self._pending[0] is batch:
            self._flush()
        ev = self._start_bin(batch)
        self._flush()
        self._pending = (batch, build_fn, ev)

    def _flush(self):
        if self._pending is None:
            return None
        batch, build_fn, ev = self._pending
        self._pending = None
        main = torch.cuda.current_stream(self.device)
        main.wait_event(ev)
        res = build_fn(batch)
        done = torch.cuda.Event()
        done.record(main)
        self._built[batch] = done
        return res

    def drain(self):
        return self._flush()


def probe_output_placement(shape, dtype, launch=None, candidates=8, launches=10, device="cuda:0", keep_first=False,
                           good_GBps=None, max_candidates=None):
    """Where a large output tensor lies in HBM decides up to 25 % of a builder launch on MI355X (NOTES.md 8: the same
    launch takes 134, 148 or 172 us into different 900 MiB allocations of one process; a linear fill does not care).
    A producer that allocates its output ring once can pick its allocations: this helper allocates `candidates` tensors,
    times a writer into each and returns (best tensor, its us per launch, all timings); the other tensors are released.
    The writer is `launch(out)` if given, else the library's placement probe (evrep_probe_store: the write footprint of
    the float64 12-channel builder and nothing else -- it overwrites the candidates with zeros).
    Fast regions come in runs and some processes find none among their first allocations: with good_GBps set, further
    rounds of `candidates` allocations follow (all kept alive meanwhile, so every round sees new regions) until one
    reaches that rate or max_candidates tensors have been tried.
    keep_first: also return the FIRST candidate (what a caller that does not probe would have got), as a 4th element."""
    _require_gpu()
    device = torch.device(device)
    if launch is None:
        def launch(o):
            with torch.cuda.device(device):
                _lib.api().evrep_probe_store(_ptr(o), o.numel() * o.element_size(), _stream_ptr())
    outs, times = [], []
    limit = int(max_candidates) if max_candidates else int(candidates)
    while len(outs) < limit:
        for _ in range(min(int(candidates), limit - len(outs))):
            o = torch.empty(shape, dtype=dtype, device=device)
            for _ in range(3):
                launch(o)
            torch.cuda.synchronize(device)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(int(launches)):
                launch(o)
            b.record()
            torch.cuda.synchronize(device)
            outs.append(o)
            times.append(a.elapsed_time(b) / launches * 1e3)
        nbytes = outs[0].numel() * outs[0].element_size()
        if good_GBps is None or nbytes / (min(times) * 1e-6) / 1e9 >= good_GBps:
            break
    k = min(range(len(outs)), key=lambda i: times[i])
    best, first = outs[k], outs[0]
    del outs
    return (best, times[k], times, first) if keep_first else (best, times[k], times)


def gwd_padded_l1(Xs, Xt, h=0.7, out=None):
    """OTMI(Xs, Xt, h).solve()[1] on the GPU: Xs (n, ds), Xt (m, dt) array-likes -> 0-dim float64 cuda tensor.
    `out`: optional one-element float64 cuda tensor (e.g. ``costs[i:i+1]``) the kernel writes into directly --
    no host synchronisation, so a list of solves queues back to back."""
    _require_gpu()
    api = _lib.api()
    dev = Xs.device if isinstance(Xs, torch.Tensor) and Xs.is_cuda else torch.device("cuda", torch.cuda.current_device())
    a = torch.as_tensor(np.asarray(Xs) if not isinstance(Xs, torch.Tensor) else Xs).to(dev, torch.float64).contiguous()
    b = torch.as_tensor(np.asarray(Xt) if not isinstance(Xt, torch.Tensor) else Xt).to(dev, torch.float64).contiguous()
    if a.dim() != 2 or b.dim() != 2 or a.shape[0] == 0 or b.shape[0] == 0:
        raise ValueError("Xs and Xt must be non-empty 2-D point clouds")
    n, m = int(a.shape[0]), int(b.shape[0])
    scratch = _lib.scratch(api.evrep_gwd_scratch_bytes(n, m), dev)
    cost = torch.empty((), dtype=torch.float64, device=dev) if out is None else want(out, "out", torch.float64, numel=1, device="cuda")
    with torch.cuda.device(dev):
        api.evrep_gwd_padded_l1(_ptr(a), n, int(a.shape[1]), _ptr(b), m, int(b.shape[1]), float(h), _ptr(scratch), _ptr(cost),
                                _stream_ptr())
    return cost


class GwdWorkspace:
    """Scratch of the batched GWD solves and of the device harness, allocated once and grown on demand (a solve used to
    allocate its scratch per call and synchronise on its scalar)."""

    def __init__(self, device=None):
        _require_gpu()
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self._bufs = {}

    def get(self, name, nbytes):
        buf = self._bufs.get(name)
        if buf is None or buf.numel() < nbytes:
            buf = self._bufs[name] = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
        return buf

    def typed(self, name, shape, dtype):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        return self.get(name, max(n, 256))[:n].view(dtype).view(*shape)


_WORKSPACES = {}


def _default_workspace(device):
    key = str(device)
    if key not in _WORKSPACES:
        _WORKSPACES[key] = GwdWorkspace(device)
    return _WORKSPACES[key]


def gwd_padded_l1_batch(Xs, n, Xt, m, n_cap, m_cap, xs_row=None, xt_row=None, h=0.7, out=None, workspace=None):
    """P solves of OTMI(Xs, Xt, h).solve()[1] in ONE call (six launches in all, no host synchronisation).
    Xs: (rows, ds) float64 cuda tensor holding every source cloud, pair p = rows [xs_row[p], xs_row[p] + n[p])
    (xs_row None: p * n_cap); Xt / xt_row / m likewise.  n, m, xs_row, xt_row: int64 cuda tensors of length P (the sizes
    may come straight from the device harness).  n_cap, m_cap: host upper bounds of the sizes.  Returns (P,) float64
    costs on the device (NaN for an empty or oversized cloud)."""
    _require_gpu()
    api = _lib.api()
    want(Xs, "Xs", torch.float64, (None, None), device="cuda")
    dev = Xs.device
    want(Xt, "Xt", torch.float64, (None, None), device=dev)
    P = int(n.numel())
    for t, nm in ((n, "n"), (m, "m"), (xs_row, "xs_row"), (xt_row, "xt_row")):
        if t is not None:
            want(t, nm, torch.int64, numel=P, device=dev)
    ds, dt = int(Xs.shape[1]), int(Xt.shape[1])
    ws = workspace or _default_workspace(dev)
    nbytes = api.evrep_gwd_batch_scratch_bytes(P, ds, dt, int(n_cap), int(m_cap))
    if nbytes == 0:
        raise ValueError("bad batch geometry (P=%d, ds=%d, dt=%d, n_cap=%d, m_cap=%d)" % (P, ds, dt, n_cap, m_cap))
    scratch = ws.get("gwd_scratch", nbytes)
    out = torch.empty(P, dtype=torch.float64, device=dev) if out is None else want(out, "out", torch.float64, numel=P, device=dev)
    with torch.cuda.device(dev):
        api.evrep_gwd_padded_l1_batch(P, _ptr(Xs), _ptr(xs_row), _ptr(n), ds, _ptr(Xt), _ptr(xt_row), _ptr(m), dt, int(n_cap),
                                      int(m_cap), float(h), _ptr(scratch), _ptr(out), _stream_ptr())
    return out


def otmi_event_clouds(events, offsets, height, width, cap=None, workspace=None):
    """Device half of otmi(): events (total, 4) int32 cuda tensor of B windows (offsets: (B+1,) int64, host or device) ->
    (Xs (B, 3, cap, 4) float64, n (B, 3) int64, quad (B, 3) int32), all on the device, nothing read back.
    The returned tensors are VIEWS of `workspace` (default: the device's shared GwdWorkspace): the next call with the same
    workspace overwrites them -- clone what must outlive it, or pass a GwdWorkspace of your own (one per host thread / stream)."""
    _require_gpu()
    api = _lib.api()
    dev = want(events, "events", torch.int32, (None, 4), device="cuda").device
    off_host = offsets.detach().cpu() if isinstance(offsets, torch.Tensor) else torch.as_tensor(np.asarray(offsets, dtype=np.int64))
    B = int(off_host.numel() - 1)
    if cap is None:
        cap = int((off_host[1:] - off_host[:-1]).max().item())
    off_dev = off_host.to(dev, torch.int64)
    ws = workspace or _default_workspace(dev)
    Xs = ws.typed("otmi_xs", (B, 3, int(cap), 4), torch.float64)
    n = ws.typed("otmi_n", (B, 3), torch.int64)
    quad = ws.typed("otmi_quad", (B, 3), torch.int32)
    scratch = ws.typed("otmi_ev_scratch", (api.evrep_otmi_scratch_bytes(B),), torch.uint8)
    with torch.cuda.device(dev):
        api.evrep_otmi_event_clouds(_ptr(events), _ptr(off_dev), B, int(height), int(width), int(cap), _ptr(Xs), _ptr(n), _ptr(quad),
                                    _ptr(scratch), _stream_ptr())
    return Xs, n, quad


def otmi_rep_clouds(reps, quad, B, workspace=None, slot="otmi_xt"):
    """Device half of otmi(): reps (items, S, S, C) float64/float32 cuda tensor of letterboxed representations (item i
    belongs to window i % B), quad (B, 3) int32 from otmi_event_clouds -> (Xt (items, 3, m_cap, C + 2) float64,
    m (items, 3) int64).  Views of `workspace`, like otmi_event_clouds' results."""
    _require_gpu()
    api = _lib.api()
    dev = reps.device
    reps = reps.contiguous()
    items, S, S2, C = (int(v) for v in reps.shape)
    if S != S2:
        raise ValueError("letterboxed representations are square")
    m_cap = (S - (S // 2 - 1)) ** 2
    ws = workspace or _default_workspace(dev)
    Xt = ws.typed(slot, (items, 3, m_cap, C + 2), torch.float64)
    m = ws.typed(slot + "_m", (items, 3), torch.int64)
    dt = {torch.float64: _lib.F64, torch.float32: _lib.F32}[reps.dtype]
    scratch = ws.typed("otmi_rep_scratch", (api.evrep_otmi_scratch_bytes(items),), torch.uint8)
    with torch.cuda.device(dev):
        api.evrep_otmi_rep_clouds(_ptr(reps), dt, items, int(B), S, C, _ptr(quad), int(m_cap), _ptr(Xt), _ptr(m), _ptr(scratch),
                                  _stream_ptr())
    return Xt, m, m_cap


def otmi_rep_clouds_bank(base, bank, slot, cand, quad, B, workspace=None):
    """The clouds of len(cand) candidate stacks that differ in one channel (one step of the representation search):
    base (B, S, S, C) letterboxed stack of the channels chosen so far, bank (B, S, S, R) letterboxed candidate channels
    (same dtype, float64 / float32), item j * B + b = base[b] with channel `slot` replaced by bank[b, ..., cand[j]].
    cand: host integers in [0, R).  Returns (Xt (items, 3, m_cap, C + 2) float64, m (items, 3) int64, m_cap): what
    otmi_rep_clouds gives for the materialised items, as views of `workspace`."""
    _require_gpu()
    api = _lib.api()
    dt = {torch.float64: _lib.F64, torch.float32: _lib.F32}
    want(base, "base", (torch.float64, torch.float32), (int(B), None, None, None), device="cuda")
    dev = base.device
    Bn, S, S2, C = (int(v) for v in base.shape)
    if S != S2:
        raise ValueError("letterboxed representations are square")
    want(bank, "bank", base.dtype, (Bn, S, S, None), device=dev)
    want(quad, "quad", torch.int32, (Bn, 3), device=dev)
    R = int(bank.shape[3])
    cand = [int(c) for c in cand]
    items = len(cand) * Bn
    m_cap = (S - (S // 2 - 1)) ** 2
    ws = workspace or _default_workspace(dev)
    Xt = ws.typed("otmi_xt", (items, 3, m_cap, C + 2), torch.float64)
    m = ws.typed("otmi_xt_m", (items, 3), torch.int64)
    scratch = ws.typed("otmi_rep_scratch", (api.evrep_otmi_scratch_bytes(items),), torch.uint8)
    with torch.cuda.device(dev):
        api.evrep_otmi_rep_clouds_bank(_ptr(base), _ptr(bank), dt[base.dtype], Bn, S, C, R, int(slot), _lib.int32_array(cand), len(cand),
                                       _ptr(quad), int(m_cap), _ptr(Xt), _ptr(m), _ptr(scratch), _stream_ptr())
    return Xt, m, m_cap


def otmi_batch(events, offsets, reps, height, width, h=0.7, workspace=None):
    """otmi(events_b, rep_{r,b}, height, width, S) for R representations x B windows, entirely on the device:
    events (total, 4) int32 cuda tensor + offsets (B+1), reps (R, B, S, S, C) letterboxed representations ->
    (R, B) float64 cuda tensor of the mean cost over the three scored quadrants, plus the (R, B, 3) quadrant costs.
    The event clouds are built once per window and shared by the R representations."""
    R, B = int(reps.shape[0]), int(reps.shape[1])
    ws = workspace or _default_workspace(events.device)
    Xs, n, quad = otmi_event_clouds(events, offsets, height, width, workspace=ws)
    cap = int(Xs.shape[2])
    Xt, m, m_cap = otmi_rep_clouds(reps.reshape(R * B, *reps.shape[2:]), quad, B, workspace=ws)
    dev = events.device
    P = R * B * 3
    slot = torch.arange(B * 3, device=dev, dtype=torch.int64).repeat(R)       # pair p -> its window's (b, k) slot
    costs = gwd_padded_l1_batch(Xs.view(-1, 4), n.view(-1)[slot].contiguous(), Xt.view(-1, int(Xt.shape[-1])),
                                m.view(-1), cap, m_cap, xs_row=(slot * cap).contiguous(),
                                xt_row=(torch.arange(P, device=dev, dtype=torch.int64) * m_cap), h=h, workspace=ws)
    q = costs.view(R, B, 3)
    return q.mean(dim=2), q
