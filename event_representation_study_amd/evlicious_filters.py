"""The ev-licious event filters on the device -- mirrors ev-licious/src/evlicious/tools/filters.py and
``resize_to_resolution`` of tools/utils.py:110-158 under the reference's names and signatures.

``insert(events)`` takes anything with ``x, y, t, p, width, height`` (ev-licious ``Events``), runs the filter's HIP kernel
(engine.EventBatch.filter_*), and returns the surviving events: ``events[mask]`` where the caller's object can be indexed
(the reference's ``Events``), else a small namespace with the same fields (x, y uint16, t int64, p int8, width, height).
The per-pixel state of a filter (last timestamps, activity counters) stays ON THE DEVICE between calls, in absolute time:
int64 timestamps beyond the int32 range of the device layout are rebased per call.  ``insert_device(batch)`` takes an
``EventBatch`` and returns the filtered ``EventBatch`` without leaving the GPU (state: one array per window of the batch).

There is no CPU fallback: without a HIP device every filter raises ``EvrepError``.

Not mirrored: ``Random`` -- ``np.random.choice`` without a seed has no parity target; it raises ``NotImplementedError``.
Unpinned: the reference compiles its loops with numba, which is absent where the fixtures were recorded; the loops ran as
plain Python (``numba.jit`` = identity), with ``x``, ``y`` widened to int64 for ``_background_activity_filter`` as numba
types them (tests/golden/README_evl_filters.md).
"""
import enum
import types

import numpy as np
import torch

from .engine import EventBatch
from .synthetic import int64_to_int32


# the reference's filter codes, 1..5 in its order of declaration
Filtering_Type = enum.IntEnum("Filtering_Type", ["BackgroundActivity", "Random", "ContrastThresholdIncrease", "RefractoryPeriod",
                                                 "HotPixel"])
Filtering_Type.summary = classmethod(lambda cls: "".join(" %s=%d " % (m.name, m.value) for m in cls))


def _to_batch(events):
    """-> (EventBatch of one window, absolute time of its t == 0).  p == 0 reads as -1, as Events.__init__ rewrites it."""
    H, W = int(events.height), int(events.width)
    x, y = np.asarray(events.x), np.asarray(events.y)
    n = len(x)
    t = np.asarray(events.t).astype(np.int64)
    base = int(t[0]) if n else 0
    ev = np.empty((n, 4), np.int32)
    ev[:, 0], ev[:, 1] = x.astype("int32"), y.astype("int32")
    ev[:, 2] = int64_to_int32(t - base, "t")
    p = np.asarray(events.p).astype(np.int32)
    ev[:, 3] = np.where(p == 0, -1, p)
    return EventBatch.from_numpy(ev, H, W), base


def _select(events, mask):
    """events[mask] for an indexable event object, else a namespace of the masked fields."""
    if hasattr(type(events), "__getitem__"):
        return events[mask]
    return types.SimpleNamespace(x=np.asarray(events.x)[mask].astype(np.uint16), y=np.asarray(events.y)[mask].astype(np.uint16),
                                 t=np.asarray(events.t)[mask].astype(np.int64), p=np.asarray(events.p)[mask].astype(np.int8),
                                 width=int(events.width), height=int(events.height))


def _mask(keep):
    return keep.cpu().numpy().astype(bool)


class _StatefulFilter:
    """state: the reference's per-pixel array as a (B, H, W) device tensor, None until the first insert."""
    state = None

    def _run(self, batch, t_base):
        raise NotImplementedError

    def insert(self, events):
        batch, base = _to_batch(events)
        keep, self.state = self._run(batch, base)
        return _select(events, _mask(keep))

    def insert_device(self, batch, t_base=None):
        keep, self.state = self._run(batch, t_base)
        return batch.compacted(keep)


class HotPixel:
    def __init__(self):
        self.hot_pixel_mask = None      # (H, W) bool device tensor: True = the pixel passes

    def calibrate(self, events, debug=False, threshold=0.6):
        batch = events if isinstance(events, EventBatch) else _to_batch(events)[0]
        return self._calibrate(batch, threshold)

    @staticmethod
    def _calibrate(batch, threshold=0.6):
        count = batch.pixel_counts().to(torch.float64).sum(dim=0)      # the first batch inserted, all its windows
        mask = count / count.max() < threshold
        if not bool(mask.any()):        # np.max(count[mask]) of an empty selection (count[~mask] always holds the maximum)
            raise ValueError("zero-size array to reduction operation maximum which has no identity")
        min_count_hotpixel = count[~mask].min()
        max_count_non_hotpixel = count[mask].max()
        if float(min_count_hotpixel / max_count_non_hotpixel) > 2:
            return mask
        return torch.ones_like(mask)

    def insert(self, events):
        batch = _to_batch(events)[0]
        if self.hot_pixel_mask is None:
            self.hot_pixel_mask = self._calibrate(batch)
        keep, _ = batch.filter_mask(self.hot_pixel_mask)
        return _select(events, _mask(keep))

    def insert_device(self, batch, t_base=None):
        if self.hot_pixel_mask is None:
            self.hot_pixel_mask = self._calibrate(batch)
        keep, _ = batch.filter_mask(self.hot_pixel_mask)
        return batch.compacted(keep)


class BackgroundActivity(_StatefulFilter):
    def __init__(self, depth_us, radius):
        self.radius = radius
        self.depth_us = depth_us

    @property
    def timestamps(self):
        return self.state

    def _run(self, batch, t_base):
        return batch.filter_background(self.depth_us, self.radius, state=self.state, t_base=t_base)


class Random:
    def __init__(self, random_downsampling_factor):
        raise NotImplementedError("filters.Random draws np.random.choice without a seed: there is no result to reproduce")


class ContrastThresholdIncrease(_StatefulFilter):
    def __init__(self, contrast_threshold_multiplier):
        self.contrast_threshold_multiplier = contrast_threshold_multiplier

    @property
    def counter_map(self):
        return self.state

    def _run(self, batch, t_base):
        return batch.filter_contrast(self.contrast_threshold_multiplier, state=self.state)


class RefractoryPeriod(_StatefulFilter):
    def __init__(self, depth_us):
        self.depth_us = depth_us

    @property
    def timestamps(self):
        return self.state

    def _run(self, batch, t_base):
        return batch.filter_refractory(self.depth_us, state=self.state, t_base=t_base)


def from_flags(flags):
    """The filter that `flags.filter_type` (a Filtering_Type value) names, built from the flags of the same names as the
    constructor's arguments; each of them must be positive."""
    table = {Filtering_Type.BackgroundActivity: (BackgroundActivity, ("depth_us", "radius")),
             Filtering_Type.Random: (Random, ("random_downsampling_factor",)),
             Filtering_Type.ContrastThresholdIncrease: (ContrastThresholdIncrease, ("contrast_threshold_multiplier",)),
             Filtering_Type.RefractoryPeriod: (RefractoryPeriod, ("depth_us",)),
             Filtering_Type.HotPixel: (HotPixel, ())}
    try:
        cls, names = table[Filtering_Type(flags.filter_type)]
    except ValueError:
        raise ValueError("Filter unknown") from None
    kwargs = {name: getattr(flags, name) for name in names}
    assert all(v > 0 for v in kwargs.values()), kwargs
    return cls(**kwargs)


def resize_to_resolution(events, height, width, chunks=1, pbar=None):
    """Event-level down-sampling (utils.py:110-158): the events that tip a coarse cell's change map past +-1, with the
    coordinates of the coarse sensor.  `chunks` only cuts the reference's loop into pieces that share one change map; the
    result does not depend on it."""
    batch, _ = _to_batch(events)
    keep, _, cells = batch.filter_resize(height, width)
    out = cells.compacted(keep).events.cpu().numpy()
    mask = _mask(keep)
    fx, fy = int(int(events.width) / int(width)), int(int(events.height) / int(height))
    fields = dict(x=out[:, 0].astype(np.uint16), y=out[:, 1].astype(np.uint16), t=np.asarray(events.t)[mask].astype(np.int64),
                  p=np.asarray(events.p)[mask].astype(np.int8), width=int(int(events.width) * (1.0 / fx)),
                  height=int(int(events.height) * (1.0 / fy)))
    if hasattr(events, "divider"):
        try:
            return type(events)(divider=events.divider, **fields)
        except TypeError:
            pass
    return types.SimpleNamespace(**fields)
