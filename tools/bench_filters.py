#!/usr/bin/env python3
"""HIP-event times of the event filters (EventBatch.filter_*) and of the compaction, beside the binning pass of the same
batch -- the natural yardstick: a filter reads the binned records once more and writes one byte per event.

    python tools/bench_filters.py [--shapes gen1,vga,circle,edges] [--reps 30] [--out FILE.jsonl]

Per shape and filter: median us per batch over `reps` launches (after warm-up, rotating over three resident batches so no
launch finds its own inputs in cache from the launch before), events/s, and the ratio to the binning pass.  One GPU process.
Every row is the EventBatch method as a user calls it: it includes the allocation of the keep tensor (torch.empty, from the
caching allocator) and, after the key-sorted pass, the per-key column sort the filter runs first; `compact` is the C call alone.
The `host` figure is the plain-Python restatement of the filter on ONE core for one window (Python, not numba).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from event_representation_study_amd.engine import EventBatch  # noqa: E402
from event_representation_study_amd import synthetic  # noqa: E402

SHAPES = {  # name: (W, H, events per window, windows, generator)
    "gen1": (304, 240, 50000, 32, synthetic.make_events),
    "vga": (640, 480, 50000, 32, synthetic.make_events),
    "circle": (304, 240, 50000, 32, synthetic.make_events_moving_circle),
    "edges": (304, 240, 50000, 32, synthetic.make_events_edges),
}


def batches(name, copies=3):
    W, H, n, B, gen = SHAPES[name]
    out = []
    for c in range(copies):
        wins = [gen(n, W, H, seed=100 * c + b) for b in range(B)]
        out.append(EventBatch.from_numpy(wins, H, W))
    return out, W, H, n, B


def median_us(launch, items, reps, warmup=5):
    for i in range(warmup):
        launch(items[i % len(items)])
    torch.cuda.synchronize()
    times = []
    for i in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch(items[i % len(items)])
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return float(np.median(times))


def host_us(kind, win, W, H):
    x, y, t, p = win[:, 0], win[:, 1], win[:, 2].astype(np.int64), win[:, 3]
    t0 = time.perf_counter()
    if kind == "refractory":
        last = np.full((H, W), -np.inf)
        for i in range(len(x)):
            if t[i] - last[y[i], x[i]] >= 500:
                last[y[i], x[i]] = t[i]
    elif kind == "contrast":
        act = np.zeros((H, W), np.int32)
        for i in range(len(x)):
            act[y[i], x[i]] += p[i]
            if abs(act[y[i], x[i]]) >= 2:
                act[y[i], x[i]] = 0
    elif kind == "background":
        ts = np.full((H, W), -np.inf)
        for i in range(len(x)):
            _ = ts[y[i], x[i]]
            ts[max(y[i] - 1, 0):y[i] + 1, max(x[i] - 1, 0):x[i] + 1] = t[i]
    else:
        cm = np.zeros((H // 2, W // 2), np.float32)
        for i in range(len(x)):
            cm[y[i] // 2, x[i] // 2] += p[i] * 0.25
            if abs(cm[y[i] // 2, x[i] // 2]) >= 1:
                cm[y[i] // 2, x[i] // 2] -= p[i]
    return (time.perf_counter() - t0) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="gen1,vga,circle,edges")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_filters.py needs a HIP device"
    rows = []
    for name in args.shapes.split(","):
        bs, W, H, n, B = batches(name)
        total = n * B
        bin_us = median_us(lambda b: b.rebin(), bs, args.reps)
        states = {}

        def fresh(kind, dtype, fill, shape=(B, H, W)):
            states[kind] = [torch.full(shape, fill, dtype=dtype, device="cuda:0") for _ in bs]

        fresh("refractory", torch.float64, -np.inf)
        fresh("contrast", torch.int32, 0)
        fresh("background", torch.float64, -np.inf)
        idx = {b: i for i, b in enumerate(bs)}
        cells = [b.filter_resize(H // 2, W // 2) for b in bs]       # (keep, state, coarse batch): the coarse batches are binned now
        keeps = [b.filter_refractory(500)[0] for b in bs]
        mask = torch.ones((B, H, W), dtype=torch.uint8, device="cuda:0")      # (B, H, W) uint8: filter_mask hands it over as it is
        runs = {
            "refractory_500": lambda b: b.filter_refractory(500, state=states["refractory"][idx[b]]),
            "contrast_2": lambda b: b.filter_contrast(2, state=states["contrast"][idx[b]]),
            "background_r1_d200": lambda b: b.filter_background(200, 1, state=states["background"][idx[b]]),
            "background_r2_d200": lambda b: b.filter_background(200, 2, state=states["background"][idx[b]]),
            "change_map_2x2": lambda b: cells[idx[b]][2]._filter_fsm(2, 4, cells[idx[b]][1], torch.float32, 0.0),
            "resize_2x2_with_cell_map_and_binning": lambda b: b.filter_resize(H // 2, W // 2),
            "mask_gather": lambda b: b.filter_mask(mask),
            "compact": lambda b: b.lib.evrep_filter_compact(*compact_args(b, keeps[idx[b]])),
        }
        scratch = torch.empty(int(bs[0].lib.evrep_filter_compact_scratch_bytes(B, total)), dtype=torch.uint8, device="cuda:0")
        ev_out = torch.empty((total, 4), dtype=torch.int32, device="cuda:0")
        off_out = torch.empty(B + 1, dtype=torch.int64, device="cuda:0")

        def compact_args(b, keep):
            import ctypes
            p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
            return (p(b.events), p(b.offsets), b.B, p(keep), p(ev_out), p(off_out), p(scratch),
                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

        for b in bs:
            b.bin()
        for fname, fn in runs.items():
            us = median_us(fn, bs, args.reps)
            row = dict(shape=name, W=W, H=H, events_per_window=n, windows=B, binning_pass=int(bs[0].plan.reserved), filter=fname,
                       us_per_batch=round(us, 2), events_per_s=round(total / us * 1e6), bin_us=round(bin_us, 2),
                       ratio_to_binning=round(us / bin_us, 2))
            rows.append(row)
            print(json.dumps(row), flush=True)
        if not args.no_host:
            win = SHAPES[name][4](n, W, H, seed=0)
            for kind in ("refractory", "contrast", "background", "resize"):
                us = host_us(kind, win, W, H)
                row = dict(shape=name, filter="host_python_" + kind, windows=1, us_per_window=round(us), events_per_s=round(n / us * 1e6),
                           note="plain Python loop on one core, not numba")
                rows.append(row)
                print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
