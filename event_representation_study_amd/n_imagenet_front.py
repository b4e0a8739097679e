"""N-ImageNet's event front end and base_augment("train"), on the host under the reference's names and on the device.

What n_imagenet/real_cnn_model/data/imagenet.py does to every sample in front of its accumulators:

    load_event                   :30-57      columns -> float64 rows [x, y, t / 1e6, p]; p goes through uint8, and where no p is
                                             below -0.5 (always, after uint8) every p <= 0.5 becomes -1
    parse_event                  :128-163    reshape_event_no_sample (sensor 640x480 -> image 224x224, a float64 multiply) and
                                             slice_event (:60-84: "idx", "time", "random")
    base_augment("train")        :1176-1187  random_time_flip, random_flip_events_along_x, random_shift_events (+ crop to the frame)

HOST MIRRORS (same names, same signatures, same in-place side effects on the caller's tensor: the no-flip path mutates it, the
time flip returns a copy): ``load_event``, ``slice_event``, ``reshape_event_no_sample``, ``parse_event``, ``random_time_flip``,
``random_flip_events_along_x``, ``random_shift_events``, ``base_augment``.  They are the restatement the CPU tests pin against
tests/golden/nimg_front.npz, which the reference's own functions wrote.

DEVICE PATH.  ``NImageNetFrontEnd(cfg, mode).prepare(batch)`` runs all of the above for B windows in ONE call of
``evrep_nimg_prepare`` (csrc/evrep_augment.hip: a count launch, one scan workgroup, a write launch) on the packed int32 rows
``[x, y, t - base, p as stored]`` of an ``EventBatch`` -- what ``DeviceRecording.windows`` gathers -- and returns an
``AugmentedBatch``: the kept rows ``[trunc x, trunc y, 0, sign p]`` as a new ``EventBatch`` on the image frame, the float64
``t`` and ``tnorm`` every accumulator forms (:198-199), the untruncated ``xy``, and per-window counts and status words.  One host
read of B counts and status words sizes the next plan, as ``EventBatch.compacted`` does.  ``accumulate_device(name, aug)`` then
builds any of the eleven ``n_imagenet_acc.SPECS`` accumulators from it, ``dist_device(aug)`` builds DiST
(reshape_then_acc_adj_sort) from it: polstats, then evrep_dist, and ``sort_device(aug, ...)`` the sorted timestamp image
(reshape_then_acc_sort, every switch): evrep_time_index on ``aug.t``, polstats, evrep_sort_image -- nothing leaving the device.  The random parameters are drawn on the
host by ``draw_slice`` / ``draw_augment`` from the global ``random`` / ``np.random`` streams in exactly the order B sequential reference
calls consume them, so seeding the two generators reproduces the reference's batch.

THE STUDY'S REPRESENTATIONS.  ``study_device(name, aug)`` builds ERGO-12, EventStack or TORE ("optimized", "event_stack", "tore")
for the whole batch as n_imagenet's reshape_then_optimized / _event_stack / _tore wrappers (imagenet.py:1025-1107) build them per
sample: ``evrep_nimg_study_rows`` (csrc/evrep_study.hip: a reduction per window, a write pass) turns ``aug.t`` and ``aug.xy`` into the
rows those wrappers hand the builders -- whole seconds rebased to the window's first, the past half of the stack, coordinates
shifted to their minimum with the float64 roundings of ``x - min(x) + 1`` --, the batched builder runs on an ``EventBatch`` over
them, and ``voxel_normalize(normalize=False)`` casts and transposes; no event leaves the device.  ``study_rows_host`` is the numpy
restatement of the kernel for one window.

OUT OF SCOPE.  ``reshape_method`` "sample" and "unique" (``reshape_event_with_sample`` / ``reshape_event_unique`` raise
NotImplementedError: the first draws a permutation of the whole sample, the second needs a key sort of it and is off by default
in the reference); ``accumulate_device("acc_sort", aug)`` (acc_sort is no
``SPECS`` accumulator: ``sort_device`` is its device-input form); the ``denoise_*`` options, which the reference reads and never
defines.  There is no CPU fallback for the device path: without a HIP device it raises ``EvrepError``.
"""
import random

import numpy as np
import torch

from . import _lib
from ._lib import ptr, require_gpu, stream_ptr
from .engine import EventBatch

SENSOR_H = 480     # imagenet.py:16-21
SENSOR_W = 640
IMAGE_H = 224
IMAGE_W = 224
TIME_SCALE = 1000000
MAX_SHIFT = 20     # random_shift_events' default (:1140)

# one evrep_nimg_params per window (include/evrep.h)
PARAMS_DTYPE = np.dtype([("s0", "<i8"), ("s1", "<i8"), ("t_lo", "<f8"), ("t_hi", "<f8"), ("x_shift", "<i4"), ("y_shift", "<i4"),
                         ("flags", "<u4"), ("reserved", "<u4")])
assert PARAMS_DTYPE.itemsize == 48


# ---------------------------------------------------------------------------------------------
# host mirrors
# ---------------------------------------------------------------------------------------------
def event_rows(x, y, t, p):
    """The float64 (N, 4) array load_event forms from the four stored columns (:35-55)."""
    ev = np.vstack([x, y, t, np.asarray(p).astype(np.uint8)]).T.astype(np.float64)
    ev[:, 2] /= TIME_SCALE
    if ev[:, 3].min() >= -0.5:                 # zero polarity (:54-55); uint8 is never negative, so -1 arrives here as 255
        ev[:, 3][ev[:, 3] <= 0.5] = -1
    return ev


def load_event(event_path, cfg):
    data = np.load(event_path)
    if getattr(cfg, "compressed", True):
        rec = data["event_data"]
        return event_rows(rec["x"], rec["y"], rec["t"], rec["p"])
    return event_rows(data["x_pos"], data["y_pos"], data["timestamp"], data["polarity"])


def slice_event(event, cfg):
    method = getattr(cfg, "slice_method", "idx")
    if method == "idx":
        return event[getattr(cfg, "slice_start", None):getattr(cfg, "slice_end", None)]
    if method == "time":
        start, end = getattr(cfg, "slice_start", None), getattr(cfg, "slice_end", None)
        return event[(event[:, 2] > start) & (event[:, 2] < end)]
    if method == "random":
        s0, s1 = _draw_random_slice(len(event), cfg)
        return event if (s0, s1) == (0, len(event)) else event[s0:s1]
    return event


def _draw_random_slice(n, cfg):
    """[s0, s1) of slice_method == "random" (:70-82), consuming Python's `random` as the reference does."""
    length = getattr(cfg, "slice_length", None)
    if getattr(cfg, "slice_augment", False) and cfg.mode == "train":
        width = getattr(cfg, "slice_augment_width", 0)
        length = random.randint(length - width, length + width)
    if n > length:
        start = random.choice(range(n - length + 1))
        return _resolve(n, start, start + length)
    return 0, n


def _resolve(n, start, end):
    a, e, _ = slice(start, end).indices(n)
    return a, max(a, e)


def reshape_event_no_sample(event, orig_h, orig_w, new_h, new_w):
    event[:, 0] *= new_w / orig_w
    event[:, 1] *= new_h / orig_h
    return event


def reshape_event_with_sample(event, orig_h, orig_w, new_h, new_w):
    raise NotImplementedError("reshape_method 'sample' is not built (see the module docstring)")


def reshape_event_unique(event, orig_h, orig_w, new_h, new_w):
    raise NotImplementedError("reshape_method 'unique' is not built (see the module docstring)")


_RESHAPE = {"no_sample": reshape_event_no_sample, "sample": reshape_event_with_sample, "unique": reshape_event_unique}


def parse_event(event_path, cfg):
    event = torch.from_numpy(load_event(event_path, cfg))
    if getattr(cfg, "reshape", False):
        fn = _RESHAPE.get(getattr(cfg, "reshape_method", "no_sample"))
        if fn is not None:                        # (an unknown method leaves the events as they are, as the reference's chain does)
            event = fn(event, SENSOR_H, SENSOR_W, IMAGE_H, IMAGE_W)
    if getattr(cfg, "slice_events", False):
        event = slice_event(event, cfg)
    return event


def time_flipped(event_tensor):
    """A reversed COPY with t' = t_last - t and p' = -p (:1168-1172)."""
    rev = torch.flip(event_tensor, [0])
    rev[:, 2] = rev[0, 2] - rev[:, 2]
    rev[:, 3] = -rev[:, 3]
    return rev


def x_flipped_(event_tensor, width):
    event_tensor[:, 0] = width - 1 - event_tensor[:, 0]
    return event_tensor


def shifted_(event_tensor, x_shift, y_shift, resolution):
    """In-place shift, then the rows inside the frame as a copy (:1143-1152)."""
    H, W = resolution
    event_tensor[:, 0] += x_shift
    event_tensor[:, 1] += y_shift
    x, y = event_tensor[:, 0], event_tensor[:, 1]
    return event_tensor[(x >= 0) & (x < W) & (y >= 0) & (y < H)]


def random_shift_events(event_tensor, max_shift=MAX_SHIFT, resolution=(IMAGE_H, IMAGE_W)):
    x_shift, y_shift = np.random.randint(-max_shift, max_shift + 1, size=(2,))
    return shifted_(event_tensor, x_shift, y_shift, resolution)


def random_flip_events_along_x(event_tensor, resolution=(IMAGE_H, IMAGE_W), p=0.5):
    if np.random.random() < p:
        x_flipped_(event_tensor, resolution[1])
    return event_tensor


def random_time_flip(event_tensor, resolution=(IMAGE_H, IMAGE_W), p=0.5):
    if np.random.random() < p:
        event_tensor = time_flipped(event_tensor)
    return event_tensor


def base_augment(mode):
    assert mode in ["train", "eval"]
    if mode == "eval":
        return None

    def augment(event):
        event = random_time_flip(event, resolution=(IMAGE_H, IMAGE_W))
        event = random_flip_events_along_x(event)
        return random_shift_events(event)
    return augment


def apply_augment(event_tensor, time_flip, x_flip, x_shift, y_shift, resolution=(IMAGE_H, IMAGE_W)):
    """base_augment("train") with the draws handed in (the host restatement the device path is tested against)."""
    if time_flip:
        event_tensor = time_flipped(event_tensor)
    if x_flip:
        x_flipped_(event_tensor, resolution[1])
    return shifted_(event_tensor, int(x_shift), int(y_shift), resolution)


# ---------------------------------------------------------------------------------------------
# the random parameters of B windows, drawn as B sequential reference calls draw them
# ---------------------------------------------------------------------------------------------
def draw_augment(B, mode):
    """-> dict of (B,) arrays time_flip, x_flip (bool), x_shift, y_shift (int32).  "train": per window np.random.random(),
    np.random.random(), np.random.randint(-20, 21, size=(2,)), always all three; "eval": nothing is drawn."""
    assert mode in ["train", "eval"]
    out = dict(time_flip=np.zeros(B, bool), x_flip=np.zeros(B, bool), x_shift=np.zeros(B, np.int32), y_shift=np.zeros(B, np.int32))
    if mode == "train":
        for b in range(B):
            out["time_flip"][b] = np.random.random() < 0.5
            out["x_flip"][b] = np.random.random() < 0.5
            out["x_shift"][b], out["y_shift"][b] = np.random.randint(-MAX_SHIFT, MAX_SHIFT + 1, size=(2,))
    return out


def draw_slice(lengths, cfg):
    """-> dict of (B,) arrays s0, s1 (int64 rows of the window, Python slice rules resolved), t_lo, t_hi (float64, the strict
    time predicate; -inf / +inf when unused) for windows of `lengths` events under cfg's slice_* options."""
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    B = lengths.size
    out = dict(s0=np.zeros(B, np.int64), s1=lengths.copy(), t_lo=np.full(B, -np.inf), t_hi=np.full(B, np.inf))
    if not getattr(cfg, "slice_events", False):
        return out
    method = getattr(cfg, "slice_method", "idx")
    if method == "time":
        start, end = getattr(cfg, "slice_start", None), getattr(cfg, "slice_end", None)
        if start is None or end is None:
            raise TypeError("slice_method 'time' needs slice_start and slice_end")    # the reference compares a tensor with None
        out["t_lo"][:], out["t_hi"][:] = float(start), float(end)
    for b in range(B):
        n = int(lengths[b])
        if method == "idx":
            out["s0"][b], out["s1"][b] = _resolve(n, getattr(cfg, "slice_start", None), getattr(cfg, "slice_end", None))
        elif method == "random":
            out["s0"][b], out["s1"][b] = _draw_random_slice(n, cfg)
    return out


def pack_params(slices, augment):
    """The two dicts -> a (B,) PARAMS_DTYPE array, the table evrep_nimg_prepare reads."""
    B = len(slices["s0"])
    par = np.zeros(B, PARAMS_DTYPE)
    for k in ("s0", "s1", "t_lo", "t_hi"):
        par[k] = slices[k]
    par["x_shift"], par["y_shift"] = augment["x_shift"], augment["y_shift"]
    par["flags"] = np.where(augment["time_flip"], _lib.AUG_TIME_FLIP, 0) | np.where(augment["x_flip"], _lib.AUG_X_FLIP, 0)
    return par


def host_rows(x, y, t, p, par, sx=1.0, sy=1.0, train=True, resolution=(IMAGE_H, IMAGE_W)):
    """One window through the host mirrors with the parameters of one PARAMS_DTYPE record: the (N', 4) float64 tensor the
    reference's parse_event + base_augment leave (a stand-in for the files: the columns are handed in)."""
    ev = torch.from_numpy(event_rows(x, y, t, p))
    ev[:, 0] *= sx
    ev[:, 1] *= sy
    ev = ev[int(par["s0"]):int(par["s1"])]
    if np.isfinite(par["t_lo"]) or np.isfinite(par["t_hi"]):
        ev = ev[(ev[:, 2] > float(par["t_lo"])) & (ev[:, 2] < float(par["t_hi"]))]
    flags = int(par["flags"])
    if flags & _lib.AUG_TIME_FLIP:
        ev = time_flipped(ev)
    if flags & _lib.AUG_X_FLIP:
        x_flipped_(ev, resolution[1])
    return shifted_(ev, int(par["x_shift"]), int(par["y_shift"]), resolution) if train else ev


# ---------------------------------------------------------------------------------------------
# the device path
# ---------------------------------------------------------------------------------------------
class AugmentedBatch:
    """What evrep_nimg_prepare leaves: ``batch`` (EventBatch of the kept rows [trunc x, trunc y, 0, sign p] on the image frame),
    ``t`` / ``tnorm`` (float64, one per kept row), ``xy`` (float64 (kept, 2), untruncated), ``status`` (numpy uint32 (B,),
    _lib.AUG_EMPTY / AUG_FLAT_TIME / AUG_BAD_SLICE), ``counts`` (numpy int64 (B,))."""

    def __init__(self, batch, t, tnorm, xy, status, counts):
        self.batch, self.t, self.tnorm, self.xy, self.status, self.counts = batch, t, tnorm, xy, status, counts


class NImageNetFrontEnd:
    """parse_event's reshape and slice + base_augment(mode) for B windows in one device call.  cfg: the reference's config
    object (attributes reshape, reshape_method, slice_events, slice_method, slice_start, slice_end, slice_length, slice_augment,
    slice_augment_width, mode, all optional as there); mode: "train" or "eval", base_augment's argument."""

    def __init__(self, cfg, mode, sensor=(SENSOR_H, SENSOR_W), image=(IMAGE_H, IMAGE_W)):
        assert mode in ["train", "eval"]
        self.cfg, self.mode = cfg, mode
        self.sensor, self.image = (int(sensor[0]), int(sensor[1])), (int(image[0]), int(image[1]))
        self.sx = self.sy = 1.0
        if getattr(cfg, "reshape", False):
            method = getattr(cfg, "reshape_method", "no_sample")
            if method in ("sample", "unique"):
                _RESHAPE[method](None, *self.sensor, *self.image)
            if method == "no_sample":
                self.sx, self.sy = self.image[1] / self.sensor[1], self.image[0] / self.sensor[0]   # new_w / orig_w, new_h / orig_h
        require_gpu()
        self.api = _lib.api()

    def draw(self, lengths):
        """The (B,) PARAMS_DTYPE table of one batch, consuming `random` and `np.random` as B reference calls do."""
        lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
        return pack_params(draw_slice(lengths, self.cfg), draw_augment(lengths.size, self.mode))

    def prepare(self, batch, t_base=None, params=None, want_xy=True, p_as_uint8=True):
        """batch: EventBatch of sensor rows [x, y, t - base, p as stored]; t_base: int64 (B,) absolute time of t == 0 per window
        (default: batch.t_base, else 0); params: a (B,) PARAMS_DTYPE array (default: self.draw); p_as_uint8: read p through
        uint8 as load_event does (False: rows whose p is what load_event's cast would have left).  -> AugmentedBatch."""
        B, total, dev = batch.B, batch.total, batch.device
        lengths = (batch.offsets_host[1:] - batch.offsets_host[:-1]).numpy()
        par = self.draw(lengths) if params is None else np.ascontiguousarray(params, dtype=PARAMS_DTYPE).reshape(-1)
        if par.size != B:
            raise ValueError("one parameter record per window: %d for %d windows" % (par.size, B))
        if t_base is None:
            t_base = batch.t_base
        tb = np.zeros(B, np.int64) if t_base is None else \
            np.ascontiguousarray(np.broadcast_to(np.asarray(t_base, dtype=np.int64).reshape(-1), (B,)))
        table = torch.from_numpy(np.concatenate([par.view(np.uint8), tb.view(np.uint8)])).to(dev)       # one small upload
        rows = max(total, 1)
        ev_out = torch.empty((rows, 4), dtype=torch.int32, device=dev)
        f64 = torch.empty(rows * (4 if want_xy else 2), dtype=torch.float64, device=dev)
        t_out, tn_out = f64[:rows], f64[rows:2 * rows]
        xy_out = f64[2 * rows:].view(rows, 2) if want_xy else None
        meta = torch.empty((B + 1) * 8 + B * 4, dtype=torch.uint8, device=dev)      # offsets_out then status_out
        scratch = _lib.scratch(self.api.evrep_nimg_prepare_scratch_bytes(B, total), dev)
        flags = (_lib.NIMG_P_UINT8 if p_as_uint8 else 0) | (_lib.NIMG_TRAIN if self.mode == "train" else 0)
        with torch.cuda.device(dev):
            self.api.evrep_nimg_prepare(ptr(batch.events), ptr(batch.offsets), B, ptr(table[B * 48:]), ptr(table), float(self.sx),
                                        float(self.sy), self.image[0], self.image[1], flags, ptr(ev_out), ptr(t_out), ptr(tn_out),
                                        ptr(xy_out), ptr(meta), ptr(meta[(B + 1) * 8:]), ptr(scratch), stream_ptr())
        host = meta.cpu().numpy()                                                    # the one synchronisation
        off = host[:(B + 1) * 8].view(np.int64).copy()
        status = host[(B + 1) * 8:].view(np.uint32).copy()
        kept = int(off[-1])
        out = EventBatch(ev_out[:kept], torch.from_numpy(off), self.image[0], self.image[1], plan_flags=int(batch.plan.flags))
        return AugmentedBatch(out, t_out[:kept], tn_out[:kept], xy_out[:kept] if want_xy else None, status, np.diff(off))

    def prepare_recording(self, rec, i0, i1, params=None, want_xy=True):
        """Windows [i0[b], i1[b]) of a DeviceRecording, gathered and prepared on the device (rebased to each window's first
        event; the absolute times come back through the batch's t_base)."""
        batch = rec.windows(i0, i1, rebase="first")
        return self.prepare(batch, t_base=batch.t_base, params=params, want_xy=want_xy)


def accumulate_device(name, aug):
    """One of the eleven n_imagenet_acc.SPECS accumulators from an AugmentedBatch -> (B, C, H, W) float32 device tensor, what
    accumulate_batch(name, [the host-augmented tensors]) returns.  IndexError for a window without events, as there."""
    from . import n_imagenet_acc as ni
    if name not in ni.SPECS:
        raise KeyError(name)
    empty = np.flatnonzero(aug.status & _lib.AUG_EMPTY)
    if empty.size:
        raise IndexError("empty event tensor (sample %d)" % int(empty[0]))     # event_tensor[0, 2], imagenet.py:178
    return ni._accumulate(name, aug.batch, aug.tnorm)


def dist_device(aug):
    """DiST (reshape_then_acc_adj_sort, imagenet.py:873-999) from an AugmentedBatch -> (B, 2, H, W) float32 device tensor, what
    n_imagenet_acc.dist_batch([the host-augmented tensors]) returns, bit for bit: aug.batch.polstats(aug.tnorm, ...) and one
    evrep_dist call, with nothing leaving the GPU (the status words were read by prepare()).

    Windows the reference cannot rank meaningfully are refused: one flagged AUG_EMPTY raises IndexError, as accumulate_device does;
    one flagged AUG_FLAT_TIME (its kept rows share one timestamp) raises ValueError naming the sample -- its tnorm is NaN, and the
    order the reference's sort gives NaNs is not a parity target."""
    from . import n_imagenet_acc as ni
    empty = np.flatnonzero(aug.status & _lib.AUG_EMPTY)
    if empty.size:
        raise IndexError("empty event tensor (sample %d)" % int(empty[0]))     # event_tensor[0, 2], imagenet.py:908
    flat = np.flatnonzero(aug.status & _lib.AUG_FLAT_TIME)
    if flat.size:
        raise ValueError("DiST of a window whose first and last timestamp agree (sample %d): its normalised times are NaN" % int(flat[0]))
    return ni._dist(aug.batch, aug.tnorm)


def study_device(name, aug, check=True):
    """ERGO-12, EventStack or TORE (name "optimized", "event_stack", "tore") from an AugmentedBatch -> (B, 12, H, W) float32 device
    tensor, contiguous and channel first: what torch.stack([n_imagenet_acc.reshape_then_<name>(host rows of window b, height=H,
    width=W) for b]) gives (imagenet.py:1025-1107), bit for bit.  evrep_nimg_study_rows forms the rows those wrappers hand the
    builders from aug.batch, aug.t and aug.xy (see study_rows_host), the batched builder runs on an EventBatch over them with the
    wrappers' arguments -- ERGO-12 in float64; twelve EventStack levels of the past half; TORE with k = 6 on the whole frame, the
    float64 times themselves and each window's last time as its sample time --, evrep_voxel_normalize casts and transposes.  No
    event leaves the device; aug is left as it is.

    check=True reads the (B,) status words once, at the end, and raises what the per-sample wrapper raises on such rows, naming
    the first such sample: for a window without events the wrapper's own exception for an empty tensor (ValueError, for
    "event_stack" IndexError); ValueError for a window with a time that is NaN or not below 2^63, or whose whole seconds span more
    than int32 holds; for "event_stack" ValueError for a window with rows later than its last time (descending or negative
    times: the device form builds the past half only, reshape_then_event_stack builds such a window).  check=False reads
    nothing back and returns (images, status): status a (B,) uint32 device tensor of _lib.STUDY_EMPTY, STUDY_FUTURE,
    STUDY_T_RANGE, STUDY_FLAT and STUDY_UNORDERED; the image of a window flagged as above is not the reference's.

    "time_surface" raises the IndexError reshape_then_time_surface raises (the reference cannot run it), any other name
    KeyError.  TORE needs aug.xy (prepare(want_xy=True))."""
    from . import n_imagenet_acc as ni
    ni._study_name(name)
    images, status = ni._study(name, aug.batch, aug.t, aug.xy)
    if not check:
        return images, status
    err = ni.study_status_error(name, status.cpu().numpy())
    if err is not None:
        raise err
    return images


def study_rows_host(rows, t, xy):
    """What evrep_nimg_study_rows writes for ONE window, in numpy: rows (n, 4) int32 [trunc x, trunc y, 0, sign p], t (n,) float64
    seconds, xy (n, 2) float64 untruncated -> (rows_mdes, rows_stack, rows_tore, t_last, status), the three (n, 4) int32 row
    sets, TORE's sample time and the window's _lib.STUDY_* word.

        rows_mdes   [x, y, ti - ti.min(), p], ti = t.astype(np.int64): MixedDensityEventStack.stack's own casts
                    (mixed_density_event_stack.py:26-33), narrowed to int32
        rows_stack  [x, y, 0, +1 where p > 0 else -1]: 2 * ((p + 1) // 2) - 1 (imagenet.py:1051, event_stack.py:18); the window's
                    past half ti <= t[-1] (event_stack.py:34) only where STUDY_FUTURE is clear
        rows_tore   [int(x - min(x) + 1) - 1, int(y - min(y) + 1) - 1, k, p] on the float64 xy (imagenet.py:1098-1099,
                    tore.py:29-33), k the row's index, counted down under STUDY_UNORDERED (events2ToreFeature's order marker)

    A time that is NaN or not below 2^63 (STUDY_T_RANGE) takes no part in ti.min() and gets the time column 0; an empty window
    is (three empty sets, 0.0, STUDY_EMPTY)."""
    rows = np.asarray(rows, dtype=np.int32).reshape(-1, 4)
    t = np.asarray(t, dtype=np.float64).reshape(-1)
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    n = len(t)
    if len(rows) != n or len(xy) != n:
        raise ValueError("one time and one coordinate pair per row")
    if n == 0:
        return tuple(np.zeros((0, 4), np.int32) for _ in range(3)) + (0.0, np.uint32(_lib.STUDY_EMPTY))
    st = 0
    with np.errstate(invalid="ignore", over="ignore"):
        ok = np.abs(t) < 2.0 ** 63                                     # (NaN compares False)
        ti = np.zeros(n, np.int64)
        ti[ok] = t[ok].astype(np.int64)                                # truncation toward zero
        if not ok.all():
            st |= _lib.STUDY_T_RANGE
        if (ok & ~(ti.astype(np.float64) <= t[-1])).any():             # numpy compares the int64 times with the float64 last one
            st |= _lib.STUDY_FUTURE
        if not np.all(np.diff(t) >= 0):
            st |= _lib.STUDY_UNORDERED
        tc = np.zeros(n, np.int32)
        if ok.any():
            tmin, tmax = int(ti[ok].min()), int(ti[ok].max())
            if tmax - tmin > np.iinfo(np.int32).max:
                st |= _lib.STUDY_T_RANGE
            if tmax == tmin and not st & _lib.STUDY_T_RANGE:
                st |= _lib.STUDY_FLAT
            tc[ok] = (ti[ok] - np.int64(tmin)).astype(np.int32)        # (both steps wrap where the result does not fit)

        def shifted(c):
            v = (c - c.min()) + 1.0                                    # two float64 roundings
            inside = (v > -2147483649.0) & (v < 2147483648.0)
            return (np.where(inside, np.where(inside, v, 0.0).astype(np.int64), np.iinfo(np.int32).min) - 1).astype(np.int32)
        k = np.arange(n, dtype=np.int32)
        mdes, stack, tore = rows.copy(), rows.copy(), rows.copy()
        mdes[:, 2] = tc
        stack[:, 2], stack[:, 3] = 0, np.where(rows[:, 3] > 0, 1, -1)
        tore[:, 0], tore[:, 1], tore[:, 2] = shifted(xy[:, 0]), shifted(xy[:, 1]), -k if st & _lib.STUDY_UNORDERED else k
    return mdes, stack, tore, float(t[-1]), np.uint32(st)


def sort_device(aug, global_time, neglect_polarity, use_image, strict, quantize_sort=None, denoise_image=False, denoise_sort=False,
                check=True):
    """The sorted timestamp image (reshape_then_acc_sort, imagenet.py:513-838) from an AugmentedBatch -> (B, C, H, W) float32 device
    tensor, what n_imagenet_acc.sort_batch([the host-augmented tensors], ...) returns, bit for bit: evrep_time_index on aug.t,
    aug.batch.polstats and evrep_sort_image, with no event leaving the GPU.

    Windows flagged AUG_EMPTY are refused from aug.status, before anything is launched (RuntimeError, the text of the reference's
    max() of an empty selection).  check=True reads the B status words once, at the end, and raises as sort_batch does, naming the
    sample: ValueError for a window whose time indices decrease, RuntimeError for a strict=False polarity class without a positive
    index.  check=False waits for nothing and returns (images, status): status a (B,) uint32 device tensor of _lib.SORT_EMPTY,
    SORT_DECREASING and SORT_NO_INDEX << class bits; the image of a flagged window is not the reference's."""
    from . import n_imagenet_acc as ni
    classes, qs = ni._sort_options(neglect_polarity, use_image, quantize_sort, denoise_image, denoise_sort)
    err = ni.sort_status_error(np.where(aug.status & _lib.AUG_EMPTY, _lib.SORT_EMPTY, 0).astype(np.uint32), strict)
    if err is not None:
        raise err
    images, status = ni._sort(aug.batch, aug.t, global_time, strict, classes, qs, use_image)
    if not check:
        return images, status
    err = ni.sort_status_error(status.cpu().numpy(), strict)
    if err is not None:
        raise err
    return images
