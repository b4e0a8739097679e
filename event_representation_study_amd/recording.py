"""A recording resident on the device, and windows cut from it there.

``DeviceRecording`` uploads the structure-of-arrays columns of one recording ONCE (x, y uint16, t int64, p int8 -- the dtypes
of ev-licious' ``Events``, io/utils/events.py:7-8) and answers what the reference's ``H5EventHandle`` answers
(ev-licious/src/evlicious/io/h5_event_handle.py, io/utils/event_handle.py) without the events crossing PCIe again:

* the time-to-index searches run on the device (``evrep_time_to_index``: one wavefront per query, a 64-ary search);
* the windows -- sliding by count or by time, overlapping, or anchored on labels as Gen1's samples are
  (ev-YOLOv6/yolov6/data/gen1_2yolo.py:186-198) -- are gathered on the device into the packed int32 ``[x, y, t - base, p]``
  rows of an ``EventBatch`` (``evrep_windows_gather``), whose ``.t_base`` holds the absolute time of every window's t == 0,
  ready for ``RefractoryPeriod.insert_device(batch, t_base=batch.t_base)``.

The reference's names return what the reference returns, quirks included (``compute_time_and_index_windows``).  There is no
CPU fallback: without a HIP device ``DeviceRecording`` raises ``EvrepError``.

Queries.  The reference searches ``np.searchsorted(t, q + 1e-3)`` in float64.  Timestamps are integral microseconds, so the
first ``t >= q + 1e-3`` is the first ``t > ceil(q + 1e-3) - 1``: the host forms that integer (``query_to_int``) and the device
compares integers.  The two agree wherever float64 still resolves 1e-3 next to the query, |q| < 2**43 us (three months);
beyond it ``ValueError`` is raised instead of an answer that could differ.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check
from .engine import EventBatch, _ptr, _require_gpu, _stream_ptr

QUERY_LIMIT_US = 1 << 43
_UNITS = ("nr", "us")


def query_to_int(q):
    """The integer k with (first t > k) == np.searchsorted(t, q + 1e-3) for integral t: ceil(q + 1e-3) - 1, int64, same shape."""
    f = np.asarray(q, dtype=np.float64)
    if f.size and not bool(np.all(np.abs(f) < QUERY_LIMIT_US)):      # (NaN fails the comparison too)
        raise ValueError("time query outside |t| < 2**43 us: float64 no longer resolves the reference's + 1e-3 there")
    return np.ceil(f + 1e-3).astype(np.int64) - 1


def time_and_index_windows(n, take, search, step_size, window, step_size_unit, window_unit):
    """H5EventHandle.compute_time_and_index_windows (h5_event_handle.py:71-103) on a recording of n events, as a pure function:
    ``take(idx)`` returns t[idx] for an int64 index array, ``search(q)`` the reference's ``searchsorted(t, q + 1e-3)`` for an
    array of queries.  -> ((timestamps0, timestamps1), (i0, i1)), numpy arrays.

    The reference's behaviour is kept as it is:
    * ``window_unit`` decides how i1 is STEPPED ("nr": every step_size events, "us": every step_size microseconds), and
      ``step_size_unit`` how i0 is formed from it ("nr": i1 - window events, "us": the index of timestamps1 - window);
    * in the "nr" branch i0 goes through np.unique: clipped duplicates collapse, so i0 can be SHORTER than i1 (timestamps0
      keeps i1's length); ``EventHandle.iterator`` zips the two and so drops the last windows and shifts the others;
    * i1 is clipped to n - 1 only to look its timestamp up; i0 is clipped to n - 1 in both branches.
    """
    assert window_unit in _UNITS
    assert step_size_unit in _UNITS
    if window_unit == "nr":
        i1 = np.arange(step_size, n + 1, step_size)
        timestamps1 = take(np.clip(i1, 0, n - 1))
    else:
        t0, t1 = take(np.array([0, n - 1], dtype=np.int64))
        timestamps1 = np.arange(t0 + step_size, t1 + 1, step_size)
        i1 = search(timestamps1)
    if step_size_unit == "nr":
        i0 = i1 - window
        i0 = np.clip(i0, 0, n - 1)
        i0, inverse = np.unique(i0, return_inverse=True)
        timestamps0 = take(i0)
        timestamps0 = timestamps0[inverse.reshape(-1)]
    else:
        timestamps0 = timestamps1 - window
        i0 = search(timestamps0)
        i0 = np.clip(i0, 0, n - 1)
    return (timestamps0, timestamps1), (i0, i1)


def iterator_pairs(i0, i1):
    """The (i0, i1) pairs ``EventHandle.iterator`` walks (event_handle.py:52-58): zip cuts both to the shorter, and the slice
    ``[i0:i1]`` of ``get_between_idx`` is empty where i0 > i1."""
    k = min(len(i0), len(i1))
    a = np.asarray(i0[:k], dtype=np.int64)
    return a, np.maximum(np.asarray(i1[:k], dtype=np.int64), a)


def _column(values, dtype, name):
    """Range-checked cast of a host column (a wrong dtype upstream fails here, not as a wrapped coordinate)."""
    v = np.asarray(values)
    if v.ndim != 1:
        raise ValueError("column %r must be one-dimensional" % name)
    if v.dtype == np.dtype(dtype):
        return np.ascontiguousarray(v)
    if v.dtype.kind not in "iub":
        raise ValueError("column %r must hold integers, not %s" % (name, v.dtype))
    info = np.iinfo(dtype)
    if v.size and (int(v.min()) < info.min or int(v.max()) > info.max):
        raise ValueError("column %r does not fit %s" % (name, np.dtype(dtype).name))
    return np.ascontiguousarray(v.astype(dtype))


class DeviceRecording:
    """One recording in HBM: x, y uint16, t int64 (ascending), p int8 of n events on an H x W sensor.  ``divider > 1`` (sub-pixel
    coordinates, x / divider) does not fit the int32 row layout of the engine and raises ``ValueError``."""

    def __init__(self, x, y, t, p, height, width, divider=1, device="cuda:0"):
        if int(divider) != 1:
            raise ValueError("divider %r: sub-pixel coordinates do not fit the int32 event rows" % (divider,))
        cols = [_column(x, np.uint16, "x"), _column(y, np.uint16, "y"), _column(t, np.int64, "t"), _column(p, np.int8, "p")]
        if len({len(c) for c in cols}) != 1:
            raise ValueError("x, y, t, p must have the same length")
        _require_gpu()
        self.lib = _lib.load()
        self.device = torch.device(device)
        self.height, self.width, self.divider = int(height), int(width), 1
        self.n = len(cols[2])
        self._limits = (cols[2][0], cols[2][-1]) if self.n else None
        self.x, self.y, self.t, self.p = (torch.from_numpy(c).to(self.device) for c in cols)

    @classmethod
    def from_events(cls, events, device="cuda:0"):
        """Anything with x, y, t, p, width, height (ev-licious ``Events``; ``divider`` is read where present)."""
        return cls(events.x, events.y, events.t, events.p, events.height, events.width,
                   divider=getattr(events, "divider", 1), device=device)

    @classmethod
    def from_h5(cls, path, device="cuda:0"):
        """The ev-licious container (io/utils/h5_writer.py:29-67): events/{x, y, t, p, height, width, divider}, read with h5lite."""
        from . import h5lite
        with h5lite.File(str(path)) as f:
            e = f["events"]
            divider = int(e["divider"][()]) if "divider" in e else 1
            return cls(e["x"][:], e["y"][:], e["t"][:], e["p"][:], int(e["height"][()]), int(e["width"][()]),
                       divider=divider, device=device)

    @classmethod
    def concatenated(cls, recordings):
        """Recordings of one sensor on one device laid end to end (device-to-device copies of the columns), for ONE gather
        over windows of several of them.  t is not ascending across the joints: only ``windows`` may be asked of the result."""
        first = recordings[0]
        rec = cls.__new__(cls)
        rec.lib, rec.device, rec.height, rec.width, rec.divider = first.lib, first.device, first.height, first.width, 1
        rec.x, rec.y, rec.t, rec.p = (torch.cat([getattr(r, c) for r in recordings]) for c in "xytp")
        rec.n, rec._limits = int(rec.t.numel()), None
        return rec

    # ------------------------------------------------------------------ the reference's names
    def __len__(self):
        return self.n

    def get_time_limits(self):
        if self._limits is None:
            raise IndexError("the recording holds no events")
        return self._limits

    def _take(self, idx):
        """t[idx] for a host index array -> int64 numpy array (a B-sized read-back)."""
        idx = np.asarray(idx, dtype=np.int64)
        if idx.size == 0:
            return np.zeros(idx.shape, np.int64)
        return self.t[torch.from_numpy(idx).to(self.device)].cpu().numpy()

    def _search_device(self, k):
        """first index with t > k for an int64 host array k -> int64 DEVICE tensor: ONE evrep_time_to_index call."""
        k = np.ascontiguousarray(k, dtype=np.int64).reshape(-1)
        out = torch.empty(k.size, dtype=torch.int64, device=self.device)
        if k.size:
            q = torch.from_numpy(k).to(self.device)
            with torch.cuda.device(self.device):
                check(self.lib.evrep_time_to_index(_ptr(self.t), self.n, _ptr(q), k.size, _ptr(out), _stream_ptr()),
                      "evrep_time_to_index")
        return out

    def find_index_from_timestamp(self, t_us):
        """np.searchsorted(t, t_us + 1e-3), searched on the device: an int64 array for an array, a numpy integer for a scalar."""
        k = query_to_int(t_us)
        idx = self._search_device(k).cpu().numpy().reshape(k.shape)
        return idx if k.ndim else idx[()]

    def compute_time_and_index_windows(self, step_size, window, step_size_unit, window_unit):
        """((timestamps0, timestamps1), (i0, i1)) exactly as the reference returns them, see ``time_and_index_windows`` for
        the quirks that are kept.  Every search is one device call per array of queries; the arithmetic around them is host
        numpy on B-sized arrays."""
        if self.n == 0:
            raise IndexError("the recording holds no events")
        return time_and_index_windows(self.n, self._take, self.find_index_from_timestamp, step_size, window,
                                      step_size_unit, window_unit)

    # ------------------------------------------------------------------ the engine's surface
    def windows(self, i0, i1, rebase="first"):
        """B windows [i0[b], i1[b]) gathered on the device -> ``EventBatch`` with ``.t_base`` (numpy int64 (B,)).

        i0, i1: host arrays or device tensors; the windows may overlap, repeat or be empty.  rebase: "first" -- t minus the
        window's first timestamp (Gen1's _load_events; 0 for an empty window), "none" -- t as stored, or an int64 array of
        one base per window.  ``ValueError`` for a range outside the recording (i0 < 0, i0 > i1, i1 > n), ``OverflowError``
        when some t - base leaves int32 (a window longer than 2**31 - 1 us), as ``int64_to_int32`` raises on the host route.

        Host traffic: the output is sized by the total, so (i0, i1) are read back ONCE when they are device tensors (the
        result of a device search); after the launch ONE read-back of 12 bytes per window brings the bases and the status
        words -- the only synchronisation of the call.  No event crosses PCIe."""
        dev_in = [v for v in (i0, i1) if isinstance(v, torch.Tensor)]
        if len(dev_in) == 2 and i0.is_cuda and i1.is_cuda:
            both = torch.stack([i0.reshape(-1).to(torch.int64), i1.reshape(-1).to(torch.int64)]).cpu().numpy()   # one read-back
            a, e = both[0], both[1]
        else:
            a, e = (np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v, dtype=np.int64).reshape(-1) for v in (i0, i1))
        if a.shape != e.shape:
            raise ValueError("i0 and i1 must have the same length")
        B = a.size
        if B == 0 or B > 65535:
            raise ValueError("a batch holds 1 .. 65535 windows, not %d" % B)
        if bool(np.any(a < 0)) or bool(np.any(a > e)) or bool(np.any(e > self.n)):
            raise ValueError("window outside the recording: every [i0, i1) needs 0 <= i0 <= i1 <= %d" % self.n)
        if isinstance(rebase, str):
            if rebase not in ("first", "none"):
                raise ValueError("rebase must be 'first', 'none' or an int64 array")
            mode, given = (_lib.REBASE_FIRST if rebase == "first" else _lib.REBASE_NONE), None
        else:
            mode, given = _lib.REBASE_GIVEN, np.ascontiguousarray(np.broadcast_to(np.asarray(rebase, dtype=np.int64).reshape(-1), (B,)))
        batch, meta = self._gather(a, e, mode, given)
        host = meta.cpu().numpy()                                   # the one synchronisation: bases + status
        base = host[:B * 8].view(np.int64).copy()
        status = host[B * 8:B * 12].view(np.uint32)
        if bool(np.any(status & _lib.WST_T_OVERFLOW)):
            bad = np.flatnonzero(status & _lib.WST_T_OVERFLOW)
            raise OverflowError("windows %s: t - base exceeds the int32 range of the device layout (EVREP_WST_T_OVERFLOW)"
                                % bad[:8].tolist())
        if bool(np.any(status)):
            raise _lib.EvrepError("evrep_windows_gather refused windows %s (status %s)"
                                  % (np.flatnonzero(status)[:8].tolist(), status[status != 0][:8].tolist()))
        batch.t_base = base
        return batch

    def _gather(self, a, e, mode, given):
        """Launch the gather of the host ranges [a, e) -> (EventBatch, uint8 device tensor: B int64 bases then B uint32 status
        words).  Nothing is read back."""
        B = a.size
        offs = np.zeros(B + 1, np.int64)
        np.cumsum(e - a, out=offs[1:])
        total = int(offs[-1])
        parts = [a, e, offs] + ([given] if given is not None else [])
        table = torch.from_numpy(np.concatenate(parts)).to(self.device)            # one small upload
        d_i0, d_i1, d_off = table[:B], table[B:2 * B], table[2 * B:3 * B + 1]
        d_given = _ptr(table[3 * B + 1:]) if given is not None else ctypes.c_void_p(None)
        events = torch.empty((max(total, 1), 4), dtype=torch.int32, device=self.device)
        meta = torch.empty(B * 12, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            check(self.lib.evrep_windows_gather(_ptr(self.x), _ptr(self.y), _ptr(self.t), _ptr(self.p), self.n, _ptr(d_i0),
                                                _ptr(d_i1), _ptr(d_off), B, mode, d_given, _ptr(events), _ptr(meta),
                                                _ptr(meta[B * 8:]), _stream_ptr()), "evrep_windows_gather")
        batch = EventBatch(events[:total], torch.from_numpy(offs), self.height, self.width,
                           max_events_per_window=int((e - a).max()))
        return batch, meta

    def get_between_idx(self, i0, i1, rebase="first"):
        """The events [i0:i1] (Python slice semantics, as the reference slices its datasets) as a one-window batch."""
        a, e, _ = slice(None if i0 is None else int(i0), None if i1 is None else int(i1)).indices(self.n)
        return self.windows([a], [max(a, e)], rebase=rebase)

    def get_between_time(self, t0_us, t1_us, rebase="first"):
        i0, i1 = self.find_index_from_timestamp(np.array([t0_us, t1_us]))
        return self.get_between_idx(i0, i1, rebase=rebase)

    def windows_before(self, event_idx, num_events):
        """Gen1's rule (gen1_2yolo.py:186-198): for every label, the num_events events in front of event_idx,
        [max(0, idx - num_events), idx), rebased to the window's first event.  ``IndexError`` for an empty window, as
        ``Gen1H5Events.window`` raises."""
        e = np.asarray(event_idx, dtype=np.int64).reshape(-1)
        a = np.maximum(0, e - int(num_events))
        if bool(np.any(e - a <= 0)):
            raise IndexError("sample %d: no events before its label" % int(np.flatnonzero(e - a <= 0)[0]))
        return self.windows(a, e, rebase="first")

    def iterator(self, step_size, window, step_size_unit, window_unit, batch_size=32):
        """``EventHandle.iterator`` in batches: EventBatches of up to batch_size of the reference's (i0, i1) pairs, in order."""
        _, (i0, i1) = self.compute_time_and_index_windows(step_size, window, step_size_unit, window_unit)
        a, e = iterator_pairs(i0, i1)
        for k in range(0, len(a), int(batch_size)):
            yield self.windows(a[k:k + batch_size], e[k:k + batch_size], rebase="first")
