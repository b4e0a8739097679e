#!/usr/bin/env python3
"""HIP-event times of cutting windows from a device-resident recording (recording.DeviceRecording), beside the route it
replaces and two yardsticks measured in the same run.

    python tools/bench_windows.py [--reps 50] [--events 5000000] [--out FILE.json]

A recording of 5 * 10^6 events resident in HBM, on a 304x240 and on a 1280x720 sensor; three sets of windows: 32 x 50 000
events at step 5 000 (90 % overlap), 32 x 50 000 at step 50 000 (back to back), 1024 x 2 000.  Per set, median us over `reps`
launches after warm-up:
  (a) host_route     host slicing + rebasing + EventBatch.from_numpy (the upload included; a host clock around a synchronise);
  (b) gather         evrep_windows_gather alone, tables and output resident (HIP events);
  (c) time_to_index  evrep_time_to_index for 64 and for 4 096 queries (per sensor);
  (d) d2d_copy       torch's device-to-device copy of the gather's byte count (29 B per row), same run;
  (e) binning        the binning pass of the gathered batch.
GB/s is on the algorithmic 29 B per gathered row: 13 B read (x 2, y 2, t 8, p 1), 16 B written.  One JSON line.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from event_representation_study_amd import _lib  # noqa: E402
from event_representation_study_amd.engine import EventBatch  # noqa: E402
from event_representation_study_amd.recording import DeviceRecording  # noqa: E402

ROW_BYTES = 29
SENSORS = {"304x240": (304, 240), "1280x720": (1280, 720)}
SETS = {"32x50000_step5000": (32, 50000, 5000), "32x50000_step50000": (32, 50000, 50000), "1024x2000_step2000": (1024, 2000, 2000)}


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def median_us(launch, reps, warmup=5):
    for _ in range(warmup):
        launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return float(np.median(times))


def median_host_us(run, reps, warmup=3):
    for _ in range(warmup):
        run()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--events", type=int, default=5_000_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_windows.py needs a HIP device"
    assert args.reps >= 50 or args.events < 5_000_000, "at least 50 repetitions at the full size"
    lib = _lib.load()
    result = dict(bench="windows", events=args.events, reps=args.reps, row_bytes=ROW_BYTES, sensors={})
    for sname, (W, H) in SENSORS.items():
        rng = np.random.default_rng(1)
        n = args.events
        x, y = rng.integers(0, W, n).astype(np.uint16), rng.integers(0, H, n).astype(np.uint16)
        t = (np.sort(rng.integers(0, 100_000_000, n)) + 3_000_000_000).astype(np.int64)      # 100 s at 50 kev/s, beyond int32
        p = rng.choice([-1, 1], n).astype(np.int8)
        rec = DeviceRecording(x, y, t, p, H, W)
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        out = dict(time_to_index={})
        for nq in (64, 4096):
            q = torch.from_numpy(rng.integers(int(t[0]), int(t[-1]), nq).astype(np.int64)).cuda()
            idx = torch.empty(nq, dtype=torch.int64, device="cuda")
            us = median_us(lambda: lib.evrep_time_to_index(ptr(rec.t), n, ptr(q), nq, ptr(idx), stream), args.reps)
            assert np.array_equal(idx.cpu().numpy(), np.searchsorted(t, q.cpu().numpy(), side="right"))
            out["time_to_index"][str(nq)] = dict(us=round(us, 2), us_per_query=round(us / nq, 4))
        for wname, (B, size, step) in SETS.items():
            i0 = (np.arange(B, dtype=np.int64) * step) % (n - size)
            i1 = i0 + size
            total = B * size

            def host_route():
                wins = []
                for a, e in zip(i0, i1):
                    w = np.empty((e - a, 4), np.int32)
                    w[:, 0], w[:, 1], w[:, 2], w[:, 3] = x[a:e], y[a:e], t[a:e] - t[a], p[a:e]
                    wins.append(w)
                return EventBatch.from_numpy(wins, H, W)

            offs = np.zeros(B + 1, np.int64)
            np.cumsum(i1 - i0, out=offs[1:])
            table = torch.from_numpy(np.concatenate([i0, i1, offs])).cuda()
            events = torch.empty((total, 4), dtype=torch.int32, device="cuda")
            meta = torch.empty(B * 12, dtype=torch.uint8, device="cuda")

            def gather():
                rc = lib.evrep_windows_gather(ptr(rec.x), ptr(rec.y), ptr(rec.t), ptr(rec.p), n, ptr(table[:B]), ptr(table[B:2 * B]),
                                              ptr(table[2 * B:]), B, _lib.REBASE_FIRST, None, ptr(events), ptr(meta), ptr(meta[B * 8:]),
                                              stream)
                assert rc == 0

            src = torch.empty(total * ROW_BYTES // 2, dtype=torch.uint8, device="cuda")
            dst = torch.empty_like(src)
            row = dict(windows=B, events_per_window=size, step=step, rows=total, bytes=total * ROW_BYTES)
            row["host_route_us"] = round(median_host_us(host_route, max(10, args.reps // 5)), 1)
            us = median_us(gather, args.reps)
            want = host_route()
            assert torch.equal(events, want.events), "the gather and the host route disagree"
            row["gather_us"], row["gather_GBps"] = round(us, 2), round(total * ROW_BYTES / us / 1e3, 1)
            # a copy of N bytes reads N and writes N: the gather's 29 B per row are matched by a copy of 14.5 B per row
            us_c = median_us(lambda: dst.copy_(src), args.reps)
            row["d2d_copy_us"], row["d2d_copy_GBps"] = round(us_c, 2), round(total * ROW_BYTES / us_c / 1e3, 1)
            us_b = median_us(lambda: want.rebin(), args.reps)
            row["binning_us"], row["binning_pass"] = round(us_b, 2), int(want.plan.reserved)
            row["gather_over_copy"], row["gather_over_binning"] = round(us / us_c, 2), round(us / us_b, 2)
            row["host_route_over_gather"] = round(row["host_route_us"] / us, 1)
            out[wname] = row
        result["sensors"][sname] = out
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
