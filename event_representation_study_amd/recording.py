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

Raw files.  ``DeviceRecording.from_dat`` and ``from_bin`` upload the payload of a Prophesee ``*_td.dat`` file (8 or 28 bytes per
record) or of an N-Caltech / N-MNIST ``.bin`` file (5 bytes per record) as it lies on disk and decode it on the device
(``evrep_decode_dat`` / ``evrep_decode_bin5``); ``load_events_from_path`` dispatches on the suffix as
``evlicious.io.load_events_from_path`` does.  ``DatDeviceRecording`` answers ``get_between_idx``, ``get_between_time`` and
``seek_time`` as the reference's ``DatEventHandle`` does (``dat_seek_index`` states the seek in numpy).
"""
import os
import pathlib

import numpy as np
import torch

from . import _lib
from ._lib import ptr, require_gpu, stream_ptr
from .engine import EventBatch

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


DAT_EVENT_SIZES = {0: 8, 12: 8, 40: 28}           # prophesee_utils.EV_TYPES: bytes per record of the event types the reference reads
DAT_SEEK_TERM = 100000                             # EventBaseReader.seek_time's default term_criterion


def parse_dat_header(path):
    """prophesee_utils.parse_header (io/utils/prophesee_utils.py:64-121) -> (payload_offset, ev_type, ev_size, (height, width)).

    The header is the leading lines that start with "% "; ``% Height h`` and ``% Width w`` give the sensor size (None where a
    line is missing; ``ValueError`` for such a line without a value, where the reference ends in an ``IndexError``).  Behind a
    header come one byte of event type and one of event size; a file without a header is type 0 with 8-byte records from its
    first byte.  ``ValueError`` where the file ends inside the two bytes."""
    size = [None, None]
    with open(str(path), "rb") as f:
        lines = 0
        while True:
            bod = f.tell()
            line = f.readline()
            if line[:2] != b"% ":
                break
            words = line.split()
            if len(words) > 1 and words[1] in (b"Height", b"Width"):
                if len(words) < 3:
                    raise ValueError("%s: the header's %s line holds no value" % (path, words[1].decode()))
                size[words[1] == b"Width"] = int(words[2])
            lines += 1
        if lines == 0:
            return 0, 0, 8, (None, None)
        f.seek(bod)
        two = f.read(2)
        if len(two) != 2:
            raise ValueError("%s: the file ends inside its header" % (path,))
        return bod + 2, int(two[0]), int(two[1]), (size[0], size[1])


def dat_seek_index(t_host, q, term=DAT_SEEK_TERM):
    """EventBaseReader.seek_time(q, term) (prophesee_utils.py:367-418) on an ascending host column, in numpy: the record index
    the reader stands at afterwards.  What ``evrep_dat_seek_time`` computes; a scalar for a scalar, int64 array for an array.

    q above the last timestamp gives n and q <= 0 gives 0.  Otherwise [0, n) is bisected while more than ``term`` records
    remain, and a probe that EQUALS q ends the search at middle + 1 -- the reader has consumed the probed record, which need
    not be the first with that timestamp.  The remaining range gives its first record with t >= q.  A query is truncated
    towards zero, as ``int(expected_time)``."""
    t = np.asarray(t_host)
    n = len(t)
    qs = np.trunc(np.asarray(q, dtype=np.float64)).astype(np.int64) if np.asarray(q).dtype.kind == "f" else np.asarray(q, dtype=np.int64)
    out = np.empty(qs.shape, np.int64)
    for k, v in enumerate(qs.reshape(-1)):
        v = int(v)
        if n == 0 or v <= 0:
            res = 0
        elif v > int(t[n - 1]):
            res = n
        else:
            low, high, res = 0, n, -1
            while high - low > term:
                middle = (low + high) // 2
                m = int(t[middle])
                if m > v:
                    high = middle
                elif m < v:
                    low = middle + 1
                else:
                    res = middle + 1
                    break
            if res < 0:
                res = low + int(np.searchsorted(t[low:high], v, side="left"))
        out.reshape(-1)[k] = res
    return out if out.ndim else out[()]


def dat_between_idx_rows(n, i0, i1):
    """The rows [a, e) DatEventHandle.get_between_idx(i0, i1) returns of n records: seek_event clips i0 into [0, n] and
    load_n_events reads i1 - i0 records or what is left.  i1 < i0 raises what the reference raises: ``ValueError`` (np.empty
    of a negative length), but ``IndexError`` for i1 == i0 - 1 (the buffer of i1 - i0 + 1 == 0 records is indexed)."""
    i0, i1 = int(i0), int(i1)
    if i1 == i0 - 1:
        raise IndexError("get_between_idx(%d, %d): i1 == i0 - 1" % (i0, i1))
    if i1 < i0:
        raise ValueError("get_between_idx(%d, %d): i1 < i0" % (i0, i1))
    a = min(max(i0, 0), n)
    return a, min(a + (i1 - i0), n)


def dat_between_time_rows(n, t0_us, t1_us, seek, lower_bound):
    """The rows [a, e) DatEventHandle.get_between_time(t0_us, t1_us) returns: ``seek(q)`` is the reader's seek_time,
    ``lower_bound(q)`` the first index with t >= q.  The reader seeks to t0 first and load_delta_t(t1 - t0) then refuses a
    delta below 1 us (``ValueError`` with its text).  For t0 <= 0 the reader's clock is reset to 0, NOT to t0, so the end is
    the first t >= t1 - t0; a t0 beyond the last timestamp leaves the reader done: an empty window."""
    t0, t1 = int(t0_us), int(t1_us)
    delta = int(t1_us - t0_us)
    if delta < 1:
        raise ValueError("load_delta_t(): Delta_t must be at least 1 micro-second: {}".format(delta))
    s = int(seek(t0))
    if s >= n:
        return n, n
    if t0 <= 0:
        return s, max(s, int(lower_bound(delta)))
    return s, max(s, int(lower_bound(t0 + delta)))


def load_events_from_path(path, height=None, width=None, divider=1, device="cuda:0"):
    """evlicious.io.load_events_from_path (ev-licious/src/evlicious/io/__init__.py:18-35) for the device: ``.h5`` ->
    ``DeviceRecording.from_h5``, ``.dat`` -> ``from_dat`` (height / width serve a header without a size), ``.bin`` ->
    ``from_bin``.  A ``.bag`` and a directory of ``.npy`` / ``.npz`` files raise ``NotImplementedError``; anything else
    ``ValueError``, as the reference."""
    path = pathlib.Path(path)
    if int(divider) != 1:
        raise ValueError("divider %r: sub-pixel coordinates do not fit the int32 event rows" % (divider,))
    if path.suffix == ".h5":
        return DeviceRecording.from_h5(path, device=device)
    if path.suffix == ".dat":
        return DeviceRecording.from_dat(path, height=height, width=width, device=device)
    if path.suffix == ".bag":
        raise NotImplementedError("%s: rosbags need the ROS Python API, which this package does not depend on" % path)
    if path.suffix == ".bin":
        if height is None or width is None:
            raise ValueError("%s: a .bin file names no sensor size; pass height and width" % path)
        return DeviceRecording.from_bin(path, height, width, device=device)
    if path.is_dir():
        raise NotImplementedError("%s: the reference's NPY / NPZ directory handles search t0_us for BOTH ends of get_between_time "
                                  "(npy_event_handle.py:67-68, npz_event_handle.py:82-83): there is no meaningful result to "
                                  "reproduce" % path)
    raise ValueError("%s: neither .h5, .dat, .bin, .bag nor a directory" % path)


class DeviceRecording:
    """One recording in HBM: x, y uint16, t int64 (ascending), p int8 of n events on an H x W sensor.  ``divider > 1`` (sub-pixel
    coordinates, x / divider) does not fit the int32 row layout of the engine and raises ``ValueError``."""

    _desc_first = -1        # a decoded file: the index of the first record whose t is smaller than its predecessor's
    decode_state = None     # a decoded file: the fields of evrep_decode_state as a dict

    def __init__(self, x, y, t, p, height, width, divider=1, device="cuda:0"):
        if int(divider) != 1:
            raise ValueError("divider %r: sub-pixel coordinates do not fit the int32 event rows" % (divider,))
        cols = [_column(x, np.uint16, "x"), _column(y, np.uint16, "y"), _column(t, np.int64, "t"), _column(p, np.int8, "p")]
        if len({len(c) for c in cols}) != 1:
            raise ValueError("x, y, t, p must have the same length")
        require_gpu()
        self.lib, self.api = _lib.load(), _lib.api()
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
        rec.lib, rec.api, rec.device, rec.height, rec.width, rec.divider = first.lib, first.api, first.device, first.height, first.width, 1
        rec.x, rec.y, rec.t, rec.p = (torch.cat([getattr(r, c) for r in recordings]) for c in "xytp")
        rec.n, rec._limits = int(rec.t.numel()), None
        return rec

    # ------------------------------------------------------------------ raw files
    @classmethod
    def from_dat(cls, path, height=None, width=None, device="cuda:0", out_of_bounds="raise", chunk_events=1 << 24):
        """A Prophesee DAT file (event types 0, 12 and 40) decoded on the device -> ``DatDeviceRecording``.  The sensor size is
        the header's; ``height`` / ``width`` serve a header without one (``ValueError`` if neither gives it, and for an event size
        in the header that is not the size of the event type's records).  A trailing
        partial record is ignored, as the reference's ``(end - start) // ev_size`` ignores it.  See ``_from_raw``."""
        offset, ev_type, ev_size, (h, w) = parse_dat_header(path)
        if ev_type not in DAT_EVENT_SIZES:
            raise ValueError("%s: event type %d is none of %s" % (path, ev_type, sorted(DAT_EVENT_SIZES)))
        if ev_size != DAT_EVENT_SIZES[ev_type]:      # (the reference would count records by one size and read them by the other)
            raise ValueError("%s: event size %d in the header, but records of type %d hold %d bytes"
                             % (path, ev_size, ev_type, DAT_EVENT_SIZES[ev_type]))
        h, w = (height if h is None else h), (width if w is None else w)
        if h is None or w is None:
            raise ValueError("%s: the header names no sensor size; pass height and width" % (path,))
        n = (os.path.getsize(str(path)) - offset) // ev_size
        return DatDeviceRecording._from_raw("dat", path, offset, n, ev_size, h, w, device, out_of_bounds, chunk_events)

    @classmethod
    def from_bin(cls, path, height, width, device="cuda:0", out_of_bounds="raise", chunk_events=1 << 24):
        """An N-Caltech / N-MNIST file of 5-byte records decoded on the device.  ``ValueError`` for a length that is no
        multiple of 5 (the reference's ``np.column_stack`` fails there).  See ``_from_raw``."""
        size = os.path.getsize(str(path))
        if size % 5:
            raise ValueError("%s: %d bytes are no whole number of 5-byte records" % (path, size))
        return DeviceRecording._from_raw("bin", path, 0, size // 5, 5, height, width, device, out_of_bounds, chunk_events)

    @classmethod
    def _from_raw(cls, fmt, path, offset, n, rec_bytes, height, width, device, out_of_bounds, chunk_events):
        """Upload n records of rec_bytes bytes behind ``offset`` in chunks of ``chunk_events`` and decode them where they land.

        A chunk is read from the file into one of two pinned staging buffers and copied to the device on the current stream;
        the decode call follows it there and accumulates into the 64-byte ``evrep_decode_state``.  The host waits only for the
        COPY of the chunk before last, to reuse its staging buffer -- never for a decode -- and reads the state back once, at
        the end.  out_of_bounds: "raise" -- ``ValueError`` naming the first record with x >= width or y >= height and their
        count (ev-licious' ``Events.__init__`` assertion, once, at load time); "drop" -- those records are left out and the
        others keep their order (the mask of ev-YOLOv6/yolov6/data/gen4/dataset.py:109-112).  A file whose timestamps descend
        somewhere is loaded; its time queries raise (``_require_ascending``).  The columns are views of ``n_out`` entries;
        ``decode_state`` holds the state's fields."""
        if out_of_bounds not in ("raise", "drop"):
            raise ValueError("out_of_bounds must be 'raise' or 'drop'")
        chunk_events = int(chunk_events)
        if not 1 <= chunk_events <= _lib.DECODE_MAX_N:
            raise ValueError("chunk_events must lie in 1 .. %d" % _lib.DECODE_MAX_N)
        height, width = int(height), int(width)
        if height < 1 or width < 1:
            raise ValueError("the sensor size must be positive")
        require_gpu()
        rec = cls.__new__(cls)
        rec.lib, rec.api, rec.device = _lib.load(), _lib.api(), torch.device(device)
        rec.height, rec.width, rec.divider = height, width, 1
        api, dev = rec.api, rec.device
        flags = _lib.DECODE_DROP_OOB if out_of_bounds == "drop" else _lib.DECODE_STRICT
        cols = [torch.empty(n, dtype=d, device=dev) for d in (torch.uint16, torch.uint16, torch.int64, torch.int8)]
        state = torch.empty(len(_lib.DECODE_STATE_FIELDS), dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            api.evrep_decode_state_init(ptr(state), stream_ptr())
            if n:
                scratch = _lib.scratch(api.evrep_decode_scratch_bytes(min(n, chunk_events)), dev)
                room = (min(n, chunk_events) * rec_bytes + 15) // 16 * 16        # whole 16-byte pieces: the kernels read those
                pinned = [torch.empty(room, dtype=torch.uint8).pin_memory() for _ in range(2)]
                staged = [torch.empty(room, dtype=torch.uint8, device=dev) for _ in range(2)]
                copied = [torch.cuda.Event() for _ in range(2)]
                with open(str(path), "rb") as f:
                    f.seek(offset)
                    for k, first in enumerate(range(0, n, chunk_events)):
                        m, b = min(chunk_events, n - first), k & 1
                        nbytes = m * rec_bytes
                        if k >= 2:
                            copied[b].synchronize()
                        if f.readinto(memoryview(pinned[b].numpy())[:nbytes]) != nbytes:
                            raise IOError("%s: short read" % (path,))
                        padded = (nbytes + 15) // 16 * 16
                        staged[b][:padded].copy_(pinned[b][:padded], non_blocking=True)
                        copied[b].record()
                        args = (first, height, width, flags, ptr(cols[0]), ptr(cols[1]), ptr(cols[2]), ptr(cols[3]), n,
                                ptr(state), ptr(scratch), stream_ptr())
                        if fmt == "dat":
                            api.evrep_decode_dat(ptr(staged[b]), m, rec_bytes, *args)
                        else:
                            api.evrep_decode_bin5(ptr(staged[b]), m, *args)
            st = dict(zip(_lib.DECODE_STATE_FIELDS, (int(v) for v in state.cpu().numpy())))      # the one read-back
        if st["n_in"] != n:
            raise _lib.EvrepError("decode of %s: state %r after %d records" % (path, st, n))
        rec.decode_state = st
        if st["oob_count"] and out_of_bounds == "raise":
            raise ValueError("%s: %d of %d records lie outside the %d x %d (height x width) sensor, the first at index %d"
                             % (path, st["oob_count"], n, height, width, st["oob_first"]))
        rec.n = st["n_out"]
        rec.x, rec.y, rec.t, rec.p = (c[:rec.n] for c in cols)
        rec._desc_first = st["desc_first"]
        if rec.n == 0:
            rec._limits = None
        elif rec.n == n:
            rec._limits = (np.int64(st["t_first"]), np.int64(st["t_last"]))
        else:       # records were dropped: the state's limits are those of the RAW records, the first or last may be gone
            ends = rec.t[[0, -1]].cpu().numpy()
            rec._limits = (ends[0], ends[1])
        return rec

    def _require_ascending(self):
        if self._desc_first >= 0:
            raise ValueError("the timestamps of this recording descend at record %d (a clock that wrapped is not unwrapped): "
                             "it answers index cuts only, no time query" % self._desc_first)

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
        self._require_ascending()
        k = np.ascontiguousarray(k, dtype=np.int64).reshape(-1)
        out = torch.empty(k.size, dtype=torch.int64, device=self.device)
        if k.size:
            q = torch.from_numpy(k).to(self.device)
            with torch.cuda.device(self.device):
                self.api.evrep_time_to_index(ptr(self.t), self.n, ptr(q), k.size, ptr(out), stream_ptr())
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
        d_given = ptr(table[3 * B + 1:]) if given is not None else None
        events = torch.empty((max(total, 1), 4), dtype=torch.int32, device=self.device)
        meta = torch.empty(B * 12, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            self.api.evrep_windows_gather(ptr(self.x), ptr(self.y), ptr(self.t), ptr(self.p), self.n, ptr(d_i0), ptr(d_i1), ptr(d_off),
                                          B, mode, d_given, ptr(events), ptr(meta), ptr(meta[B * 8:]), stream_ptr())
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

    def render_iterator(self, step_size, window, step_size_unit, window_unit, rendering_type=2, batch_size=32, cast=True):
        """The frames ``Visualizer.update(step, put_text=False)`` renders before its resize (io/utils/visualization.py:162-165),
        in batches: ``EventBatch.render`` of every batch of ``iterator`` -> (b, H, W, 3) uint8 device tensors ((b, H, W, 4) float64
        for TIME_SURFACE; ``evlicious_render.video_frames`` makes them ``convert_to_video``'s uint8 frames).  rendering_type:
        evlicious_render.RenderingType, by default the Visualizer's own RED_BLUE_NO_OVERLAP."""
        for batch in self.iterator(step_size, window, step_size_unit, window_unit, batch_size=batch_size):
            yield batch.render(rendering_type, cast=cast)


class DatDeviceRecording(DeviceRecording):
    """What ``DeviceRecording.from_dat`` returns: the recording of a DAT file with ``DatEventHandle``'s semantics
    (ev-licious/src/evlicious/io/dat_event_handle.py) under the reference's names -- ``get_between_idx`` and
    ``get_between_time`` follow the reader (``dat_between_idx_rows``, ``dat_between_time_rows``, ``dat_seek_index``), not the
    slices and the ``+ 1e-3`` search of the H5 handle.  ``compute_time_and_index_windows`` and ``iterator`` keep the H5 handle's
    arithmetic of the base class: ``DatEventHandle`` itself has none (its base raises ``NotImplemented``)."""

    def seek_time_index(self, t_us, term=DAT_SEEK_TERM):
        """``EventBaseReader.seek_time`` for one query or an array of them, searched on the device in ONE evrep_dat_seek_time
        call -> the record index the reader stands at: a numpy integer for a scalar, an int64 array for an array."""
        self._require_ascending()
        q = np.asarray(t_us)
        q = np.trunc(q.astype(np.float64)).astype(np.int64) if q.dtype.kind == "f" else q.astype(np.int64)
        flat = np.ascontiguousarray(q.reshape(-1))
        out = torch.empty(flat.size, dtype=torch.int64, device=self.device)
        if flat.size:
            d_q = torch.from_numpy(flat).to(self.device)
            with torch.cuda.device(self.device):
                self.api.evrep_dat_seek_time(ptr(self.t), self.n, ptr(d_q), flat.size, int(term), ptr(out), stream_ptr())
        idx = out.cpu().numpy().reshape(q.shape)
        return idx if q.ndim else idx[()]

    def _lower_bound(self, q):
        """The first index with t >= q: the first with t > q - 1."""
        return int(self._search_device(np.array([int(q) - 1], np.int64)).cpu()[0])

    def get_between_idx(self, i0, i1, rebase="first"):
        a, e = dat_between_idx_rows(self.n, i0, i1)
        return self.windows([a], [e], rebase=rebase)

    def get_between_time(self, t0_us, t1_us, rebase="first"):
        a, e = dat_between_time_rows(self.n, t0_us, t1_us, self.seek_time_index, self._lower_bound)
        return self.windows([a], [e], rebase=rebase)
