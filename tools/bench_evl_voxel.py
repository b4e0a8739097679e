#!/usr/bin/env python3
"""HIP-event times of the batched ev-licious voxel grid's normalisation and transpose (evrep_voxel_normalize), beside the route it
replaces and two yardsticks measured in the same run.

    python tools/bench_evl_voxel.py [--reps 50] [--events 50000] [--out FILE.json]

32 windows of 50 000 events at 304x240 and at 640x480, 5 bins, uniform events and the moving circle of synthetic.py.  Per set,
median us over `reps` runs after warm-up:
  (a) torch_route     the route this replaces: the torch statements of evlicious_tools.events_to_voxel_grid (mask, gather, mean,
                      std, masked assignment) in a Python loop over the windows of a DEVICE-resident voxel(mode=2) result; a host
                      clock with the device drained before and after, since bool(nz.any()) and float(std) synchronise on their own;
  (b) voxel_normalize evrep_voxel_normalize on the same (B, H, W, 5) float64 tensor, output and scratch allocated once (HIP events);
  (c) voxel_mode2     the voxel(mode=2) launch of the same batch alone (binning done);
  (d) d2d_copy        torch's device-to-device copy of B*H*W*bins*12 bytes: as many as the call reads (8) and writes (4) per value
                      at least.
The tool checks that (a) and (b) agree within rtol 1e-5, atol 1e-6 with the same zero pattern.  One JSON line.
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
from event_representation_study_amd.synthetic import make_events, make_events_moving_circle  # noqa: E402

B, BINS = 32, 5
SIZES = {"304x240": (240, 304), "640x480": (480, 640)}
STREAMS = {"uniform": make_events, "circle": make_events_moving_circle}


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


def median_host_us(run, reps, warmup=2):
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


def torch_route(grid):
    """events_to_voxel_grid's statements after the builder, window by window, on the device."""
    outs = []
    for b in range(grid.shape[0]):
        g = grid[b].permute(2, 0, 1).to(torch.float32)
        nz = g != 0
        if bool(nz.any()):
            vals = g[nz].to(torch.float64)
            mean, std = vals.mean(), vals.std(unbiased=False)
            if float(std) > 0:
                g[nz] = ((vals - mean) / (1e-5 + std)).to(torch.float32)
        outs.append(g.contiguous())
    return torch.stack(outs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--events", type=int, default=50000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_evl_voxel.py needs a HIP device"
    assert args.reps >= 50 or args.events < 50000, "at least 50 repetitions at the full size"
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())       # noqa: E731
    result = dict(bench="evl_voxel", windows=B, bins=BINS, events_per_window=args.events, reps=args.reps, sets={})
    for size, (H, W) in SIZES.items():
        for sname, make in STREAMS.items():
            batch = EventBatch.from_numpy([make(args.events, W, H, seed=s) for s in range(B)], H, W)
            grid = batch.voxel(bins=BINS, mode=2)
            out = torch.empty((B, BINS, H, W), dtype=torch.float32, device=grid.device)
            scratch = torch.empty(lib.evrep_voxel_normalize_scratch_bytes(B, H, W, BINS), dtype=torch.uint8, device=grid.device)
            null = ctypes.c_void_p(None)

            def normalize():
                _lib.check(lib.evrep_voxel_normalize(p(grid), _lib.F64, B, H, W, BINS, _lib.VOXNORM_NORMALIZE, p(out), null, p(scratch),
                                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "evrep_voxel_normalize")

            normalize()
            want = torch_route(grid)
            assert torch.equal(out == 0, want == 0) and torch.allclose(out, want, rtol=1e-5, atol=1e-6), \
                "evrep_voxel_normalize and the torch route disagree (%s %s)" % (size, sname)
            row = dict(nonzero_fraction=round(float((grid != 0).double().mean().item()), 4))
            row["torch_route_us"] = round(median_host_us(lambda: torch_route(grid), max(5, args.reps // 5)), 1)
            row["voxel_normalize_us"] = round(median_us(normalize, args.reps), 2)
            row["voxel_mode2_us"] = round(median_us(lambda: batch.voxel(bins=BINS, mode=2, out=grid), args.reps), 2)
            nbytes = B * H * W * BINS * 12
            src = torch.empty(nbytes, dtype=torch.uint8, device=grid.device)
            dst = torch.empty_like(src)
            row["d2d_copy_us"], row["bytes"] = round(median_us(lambda: dst.copy_(src), args.reps), 2), nbytes
            row["torch_route_over_voxel_normalize"] = round(row["torch_route_us"] / row["voxel_normalize_us"], 1)
            row["voxel_normalize_over_d2d_copy"] = round(row["voxel_normalize_us"] / row["d2d_copy_us"], 2)
            row["voxel_normalize_over_voxel_mode2"] = round(row["voxel_normalize_us"] / row["voxel_mode2_us"], 2)
            result["sets"]["%s_%s" % (size, sname)] = row
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
