#!/usr/bin/env python3
"""Golden vectors at the edges of the int32 time axis -> ``time_edges.npz``, ``time_edges_more.npz``,
``time_edges_ts1000.npz``, ``time_edges_ts50000.npz``.

Run in the build container only (``/root/reference`` must exist): ``python tests/golden/make_golden_time_edges.py``.
Like make_golden_boundary.py it imports the reference where it lies (the in-process stand-ins of make_golden.py) and
stores inputs and outputs only.  The windows come from tests/time_edges_windows.py, which tests/test_gpu_time_edges.py
regenerates on the GPU box from the same seeds.

* ``edge_<name>_*`` (hi, lo, cross0, wide, wrap, flat, two; 40 x 30): the gen1 dispatcher's ERGO-12, EventStack,
  TimeSurface and TORE (gen1_transforms.py:15-87, without the * 255), events2ToreFeature on the full frame with the last
  and a middle sample time, compute_repr (5 bins, gromov_wasserstein.py:96's normalised time).
* ``edgex_<name>_*`` (the same windows, ``time_edges_more.npz``): MixedDensityEventStack with one SBN and one SBT triple
  set, ev-licious events_to_voxel_grid (9 bins, int64 timestamps as ev-licious holds them) and n_imagenet's
  time-dependent reshape_then_* accumulators on [x, y, t, p = -1 / +1] rows.
* ``ts<tau>_s<slices>_<name>`` (20 x 15, one file per tau): ToTimesurface(tau=...) called directly with the dispatcher's cuts
  searchsorted(t_norm, 1..slices): spans of 590 ... 4 600 tau and windows whose cut times sit 695 ... 750 tau after 0.

Where the reference raises on a window, ``err_<key>`` records the exception's type and message instead of the output;
numpy's warnings (int32 overflow, 0 / 0) are silenced, their NaN / wrapped results are part of the contract.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import time_edges_windows as tw  # noqa: E402


def ts_direct(ref, ev, H, W, tau, slices):
    """ToTimesurface(tau)(events, idx) with the dispatcher's cuts (gen1_transforms.py:69-85, any slice count)."""
    rec = mg.to_structured(ev)
    rec["p"] = ((rec["p"] + 1) / 2).astype(np.int8)
    t = rec["t"]
    t_norm = (t - t[0]) / (t[-1] - t[0]) * slices
    idx = np.searchsorted(t_norm, np.arange(slices) + 1)
    tr = ref["ToTimesurface"](sensor_size=(W, H, 2), surface_dimensions=None, tau=tau, decay="exp")
    rep = tr(rec, idx)
    return np.ascontiguousarray(rep.reshape((-1, H, W)).transpose(1, 2, 0)), idx


MDES_SBN = ([0, 3, 5, 1], ["timestamp", "count_neg", "polarity", "timestamp_pos"], ["mean", "sum", "variance", "max"])
MDES_SBT = ([0, 2, 5, 7], ["timestamp", "timestamp_pos", "count", "timestamp_neg"], ["max", "mean", "sum", "variance"])
NI_TIME_ACC = ["acc", "acc_time", "acc_count", "acc_all", "acc_exp", "acc_time_pol"]


def ni_rows(ev):
    """[x, y, t, p] float64 rows with p in {-1, +1}, as parse_event hands them to reshape_then_* (imagenet.py:45-55)."""
    rows = ev.astype(np.float64)
    rows[:, 3] = np.where(ev[:, 3] > 0, 1.0, -1.0)
    return rows


class _Events:
    def __len__(self):
        return len(self.x)


def _evl_events(ev, W, H):
    """an ev-licious Events stand-in: uint16 pixels, int64 microsecond timestamps, int8 polarity."""
    e = _Events()
    e.x, e.y = ev[:, 0].astype(np.uint16), ev[:, 1].astype(np.uint16)
    e.t, e.p = ev[:, 2].astype(np.int64), ev[:, 3].astype(np.int8)
    e.width, e.height = W, H
    return e


def _import_evlicious():
    import importlib.util
    import types
    mod = types.ModuleType("evlicious")
    mod.Events = object
    sys.modules["evlicious"] = mod
    spec = importlib.util.spec_from_file_location(
        "evl_utils", os.path.join(mg.REF, "ev-licious", "src", "evlicious", "tools", "utils.py"))
    evl = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(evl)
    return evl


def _import_imagenet():
    import make_golden_nimagenet as mgn
    return mgn._import_imagenet()


def main():
    ref = mg._import_reference()
    out = {}

    def keep(key, fn):
        try:
            r = fn()
        except Exception as e:      # noqa: BLE001 -- what the reference does is the fixture
            out["err_" + key] = np.array("%s: %s" % (type(e).__name__, e))
            return
        if isinstance(r, tuple):
            out[key], out[key + "_idx"] = r
        else:
            out[key] = r

    with np.errstate(all="ignore"):
        H, W = tw.EDGE_H, tw.EDGE_W
        for name, ev in tw.edge_windows().items():
            k = "edge_" + name
            rec = mg.to_structured(ev)
            out[k + "_events"] = ev
            keep(k + "_ergo12", lambda: ref["opt"](rec.copy(), ev.shape[0], H, W))
            keep(k + "_event_stack", lambda: mg.es_like_dispatch(ref, rec, H, W))
            keep(k + "_time_surface", lambda: mg.ts_like_dispatch(ref, rec, H, W))
            keep(k + "_tore_bbox", lambda: mg.tore_like_dispatch(ref, rec))
            x1, y1, ts, pol = rec["x"] + 1, rec["y"] + 1, rec["t"], rec["p"]
            keep(k + "_tore_last", lambda: ref["tore"](x1, y1, ts, pol, ts[-1], 6, (H, W)))
            keep(k + "_tore_mid", lambda: ref["tore"](x1, y1, ts, pol, ts[ev.shape[0] // 2], 6, (H, W)))
            keep(k + "_voxel5", lambda: mg.voxel5(ref, ev, W, H))
        # MDES (one SBN and one SBT triple set), ev-licious events_to_voxel_grid and n_imagenet's time-dependent accumulators
        evl = _import_evlicious()
        ni = _import_imagenet()
        for name, ev in tw.edge_windows().items():
            k = "edgex_" + name
            keep(k + "_mdes_sbn", lambda: ref["MDES"](4, ev.shape[0], H, W, MDES_SBN, "SBN").stack(mg.to_structured(ev)))
            keep(k + "_mdes_sbt", lambda: ref["MDES"](4, ev.shape[0], H, W, MDES_SBT, "SBT").stack(mg.to_structured(ev)))
            keep(k + "_evl9", lambda: evl.events_to_voxel_grid(_evl_events(ev, W, H), 9, normalize=False))
            rows = ni_rows(ev)
            for acc in NI_TIME_ACC:
                keep(k + "_" + acc, lambda: getattr(ni, "reshape_then_" + acc)(torch.from_numpy(rows.copy()), height=H, width=W).numpy())
        for tau in tw.TAUS:
            for slices in tw.SLICES:
                for name, ev in tw.ts_tau_windows(tau).items():
                    k = "ts%d_s%d_%s" % (tau, slices, name)
                    if slices == tw.SLICES[0]:
                        out["ts%d_%s_events" % (tau, name)] = ev
                    keep(k, lambda: ts_direct(ref, ev, tw.TS_H, tw.TS_W, tau, slices))
    # one file per group, each well under the 1 MiB limit of a committed file
    for fname, prefixes in (("time_edges.npz", ("edge_", "err_edge_")), ("time_edges_more.npz", ("edgex_", "err_edgex_")), ("time_edges_ts1000.npz", ("ts1000_", "err_ts1000_")),
                            ("time_edges_ts50000.npz", ("ts50000_", "err_ts50000_"))):
        part = {k: v for k, v in out.items() if k.startswith(prefixes)}
        np.savez_compressed(os.path.join(HERE, fname), **part)
        print("wrote %s: %d arrays;" % (fname, len(part)), sorted(k for k in part if k.startswith("err_")))


if __name__ == "__main__":
    main()
