#!/usr/bin/env python3
"""Times of the detector's input batch from TORE's per-window bounding-box frames (DetectorFrontEnd.prepare_frames), beside the
per-window route it replaces and the dense route as the floor, measured in the same run.

    python tools/bench_detector_input_frames.py [--reps 50] [--events 50000] [--out FILE.json]

32 TORE frames (float32, C = 12, scale 255) of clustered windows -- a circle moving with the flow and edge clusters without
background, by turns, so that the bounding boxes differ -- from Gen1 (304x240) and from 1280x720, train mode (warp + flips drawn
per window with the reference's hyp), S = 640.  Median over `reps` runs after warm-up, in us:
  (a) per_window   the loop of 32 ``prepare(frame[None], params=[p])`` calls, on a host clock around the loop (its cost is host
                   work), the device drained at the end: once with gwd_pipeline's resize_taps cache emptied before every run
                   (cold) and once warm;
  (b) frames       ``prepare_frames`` of the same list: the host clock around the call (device drained), and HIP events around
                   the call (what the stream sees: the upload, the descriptor copy and the two launches);
      frames_launch  HIP events around evrep_detector_input_frames alone, every table on the device;
  (c) dense        ``prepare`` of 32 full-sensor TORE frames of the same dtype in one (B, H, W, C) tensor, tables warm, HIP events;
  (d) tap_tables   HIP events around evrep_resize_tap_tables alone, the axis descriptors on the device;
  (e) stage2_share the share of samples whose letterbox needs a resize of its own (taken inside the launch);
      stage2_crops / fused_crops  HIP events around ``prepare_frames`` of 32 equal crops of the full-sensor frames whose long side
                   is one that needs the second resize (303 for Gen1: a window whose events miss one border column), and of
                   crops one column wider that do not: what the second resize inside the launch costs.
The tool checks that (a) and (b) agree bit for bit.  One JSON line per source.
"""
import argparse
import ctypes
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from event_representation_study_amd import _lib, gwd_pipeline  # noqa: E402
from event_representation_study_amd import detector_input as di  # noqa: E402
from event_representation_study_amd.engine import EventBatch  # noqa: E402
from event_representation_study_amd.synthetic import make_events_edges, make_events_moving_circle  # noqa: E402

HYP = {"degrees": 0.373, "translate": 0.245, "scale": 0.898, "shear": 0.602, "flipud": 0.5, "fliplr": 0.5}
SOURCES = {"gen1_304x240": (240, 304), "1280x720": (720, 1280)}
B, S = 32, 640


def windows(n, H, W):
    out = []
    for s in range(B):
        if s % 2:
            out.append(make_events_edges(n, W, H, seed=s, hot_fraction=1.0, hot_pixels=0.02 + 0.01 * (s % 5), n_edges=4 + s % 7))
        else:
            out.append(make_events_moving_circle(n, W, H, seed=s, circle_radius=3.0 + s % 6, flow=(4.0 + s % 5, (s % 3) - 1.0),
                                                 starting_point=(8.0 + s % 4, 9.0 + s % 7)))
    return out


def event_us(launch, reps, warmup=5):
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


def host_us(call, reps, warmup=3, before=None):
    times = []
    for k in range(warmup + reps):
        if before:
            before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        if k >= warmup:
            times.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--events", type=int, default=50000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_detector_input_frames needs the GPU: no time is taken without one")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    rows = []
    for name, (H, W) in SOURCES.items():
        eb = EventBatch.from_numpy(windows(args.events, H, W), H, W, device=dev)
        frames = eb.tore(scale=255.0)                                    # B views (Hbb, Wbb, 12) float32
        dense = eb.tore(frame_mode=2, scale=255.0)                       # (B, H, W, 12) float32
        fe = di.DetectorFrontEnd(S, HYP, augment=True)
        random.seed(7)
        params = fe.draw(B)
        sizes = [tuple(int(v) for v in f.shape[:2]) for f in frames]
        geos = fe.frame_geometries(sizes)
        out = torch.empty((B, 12, S, S), dtype=torch.float32, device=dev)

        def per_window():
            return [fe.prepare(f[None], params=[p])[0] for f, p in zip(frames, params)]

        def ragged():
            return fe.prepare_frames(frames, params=params, out=out)[0]

        same = bool(torch.equal(torch.cat(per_window()).view(torch.int32), ragged().view(torch.int32)))
        t_cold = host_us(per_window, max(args.reps // 5, 3), before=gwd_pipeline._TAPS.clear)
        t_warm = host_us(per_window, args.reps)
        t_frames_host = host_us(ragged, args.reps)
        t_frames_stream = event_us(ragged, args.reps)
        t_dense = event_us(lambda: fe.prepare(dense, params=params), args.reps)
        # the two launches alone, every table on the device
        table, host, n_axes, max_dst, n_rows, n_wt = fe.frame_tables(sizes, geos, params)
        table["src"] = [f.data_ptr() for f in frames]
        up = torch.from_numpy(host).to(dev)
        nf = n_axes * _lib.TAPS_AXIS_FIELDS
        idx = torch.empty(2 * n_rows, dtype=torch.int32, device=dev)
        wt = torch.empty(n_wt, dtype=torch.float64, device=dev)
        scratch = torch.empty(B * ctypes.sizeof(_lib.DetinFrame) // 8, dtype=torch.int64, device=dev)
        pad = di._pad_table(114.0, 12, dev)
        ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        warp = ptr(up[nf:]) if host.size > nf else None

        def tap_tables():
            _lib.check(lib.evrep_resize_tap_tables(ptr(up), n_axes, max_dst, ptr(idx), ptr(idx[n_rows:]), ptr(wt), n_rows, n_wt, stream))

        def launch():
            _lib.check(lib.evrep_detector_input_frames(ctypes.c_void_p(table.ctypes.data), B, _lib.F32, 12, S, ptr(idx), ptr(idx[n_rows:]),
                                                       ptr(wt), n_rows, n_wt, ptr(pad), warp, 1.0 / 255, ptr(scratch), ptr(out), stream))

        t_taps = event_us(tap_tables, args.reps)
        t_launch = event_us(launch, args.reps)
        stage2 = sum(not g.fused for g in geos)
        # crops whose long side needs the second resize, and their neighbours that do not
        long2 = max(w for w in range(2, W + 1) if not fe.geometry(max(w * H // W, 1), w).fused)
        long1 = min(w for w in range(long2 + 1, W + 2) if fe.geometry(max(long2 * H // W, 1), w).fused)
        ch = max(long2 * H // W, 1)
        crops2 = [dense[b, :ch, :long2].contiguous() for b in range(B)]
        crops1 = [dense[b, :ch, :min(long1, W)].contiguous() for b in range(B)]
        assert not fe.geometry(ch, long2).fused and fe.geometry(ch, min(long1, W)).fused
        t_crops2 = event_us(lambda: fe.prepare_frames(crops2, params=params, out=out), args.reps)
        t_crops1 = event_us(lambda: fe.prepare_frames(crops1, params=params, out=out), args.reps)
        row = {"source": name, "B": B, "C": 12, "S": S, "dtype": "float32", "events": args.events, "reps": args.reps,
               "frame_sizes": len(set(sizes)), "min_frame": min(sizes), "max_frame": max(sizes), "axes": n_axes,
               "per_window_cold_host_us": round(t_cold, 1), "per_window_warm_host_us": round(t_warm, 1),
               "frames_host_us": round(t_frames_host, 1), "frames_stream_us": round(t_frames_stream, 1),
               "frames_launch_us": round(t_launch, 1), "dense_us": round(t_dense, 1), "tap_tables_us": round(t_taps, 1),
               "stage2_share": round(stage2 / B, 3), "stage2_crop": [ch, long2], "stage2_crops_stream_us": round(t_crops2, 1),
               "fused_crop": [ch, min(long1, W)], "fused_crops_stream_us": round(t_crops1, 1), "warm_over_frames": round(t_warm / t_frames_host, 2),
               "launch_over_dense": round(t_launch / t_dense, 2), "per_window_equals_frames": same}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    if not all(r["per_window_equals_frames"] for r in rows):
        raise SystemExit("the per-window route and prepare_frames differ")


if __name__ == "__main__":
    main()
