#!/usr/bin/env python3
"""HIP-event times of batched DiST on the device (evrep_dist: clip, 5x5 discount, dense rank), beside the route it replaces and two
yardsticks measured in the same run.

    python tools/bench_dist.py [--reps 50] [--events 30000] [--out FILE.json]

32 and 256 windows of 30 000 events, 640x480 -> 224x224, train mode (time flip, x flip, shift + crop drawn per window), prepared on
the device by NImageNetFrontEnd.  Per set, median us over `reps` launches after warm-up:
  (a) torch_route  the route this replaces: the per-window image statements of n_imagenet_acc.reshape_then_acc_adj_sort in a Python
                   loop over the DEVICE-RESIDENT polstats output (the upload is not charged to it); a host clock around a
                   synchronise, since torch.unique, boolean-mask indexing and .shape reads synchronise on their own;
  (b) dist         evrep_dist alone, input, output and scratch resident (HIP events);
  (c) polstats     the polstats launch of the same batch (binning done);
  (d) d2d_copy     torch's device-to-device copy of B*H*W*(6+2)*4 bytes, the input and output of (b).
The tool checks that (a) and (b) agree within the torch route's atol of 1e-6.  One JSON line.
"""
import argparse
import ctypes
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from event_representation_study_amd import _lib  # noqa: E402
from event_representation_study_amd import n_imagenet_acc as ni  # noqa: E402
from event_representation_study_amd import n_imagenet_front as nf  # noqa: E402
from event_representation_study_amd.engine import EventBatch  # noqa: E402

SETS = {"32x30000": 32, "256x30000": 256}
H = W = 224


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


def median_host_us(run, reps, warmup=1):
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


def torch_route(prim):
    """The image statements of n_imagenet_acc.reshape_then_acc_adj_sort, window by window, on a (B, H, W, 6) device tensor."""
    F = torch.nn.functional
    res = []
    for p in prim:
        halves = []
        for k in (0, 3):
            count, out, min_out = p[..., k].clone(), p[..., k + 1].clone(), p[..., k + 2].clone()
            unique_count = torch.unique(count, return_counts=True)[1]
            sum_subset = torch.cumsum(unique_count, dim=0)
            th_clip = sum_subset[sum_subset < H * W * ni.CLIP_COUNT_RATE].shape[0]
            count[count > th_clip] = th_clip
            min_out[count == 0] = 1.0
            neighbor = 25 * F.avg_pool2d(count.unsqueeze(0), 5, stride=1, padding=2)
            disc = (F.max_pool2d(out.unsqueeze(0), 5, stride=1, padding=2) + F.max_pool2d(-min_out.unsqueeze(0), 5, stride=1, padding=2)) / neighbor
            out[count > 0] = out[count > 0] - ni.DISC_ALPHA * disc.squeeze()[count > 0]
            out[out < 0] = 0
            out[neighbor.squeeze() == 1.0] = 0
            flat = out.reshape(H * W)
            val, idx = torch.sort(flat)
            unq, cnt = torch.unique_consecutive(val, return_counts=True)
            srt = torch.zeros_like(flat)
            srt[idx] = torch.repeat_interleave(torch.arange(unq.shape[0], device=flat.device), cnt).float() / unq.shape[0]
            halves.append(srt.reshape(H, W))
        res.append(torch.stack(halves))
    return torch.stack(res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--events", type=int, default=30000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_dist.py needs a HIP device"
    assert args.reps >= 50 or args.events < 30000, "at least 50 repetitions at the full size"
    lib = _lib.load()
    front = nf.NImageNetFrontEnd(types.SimpleNamespace(reshape=True, mode="train"), "train")
    result = dict(bench="dist", events_per_window=args.events, reps=args.reps, sets={})
    for sname, B in SETS.items():
        rng = np.random.default_rng(2)
        n = args.events
        rows, bases = [], []
        for b in range(B):
            x, y = rng.integers(0, 640, n), rng.integers(0, 480, n)
            t = (np.sort(rng.integers(0, 50_000, n)) + 1_600_000_000_000_000 + b * 60_000).astype(np.int64)
            rows.append(np.stack([x, y, t - t[0], rng.integers(0, 2, n)], axis=1).astype(np.int32))
            bases.append(t[0])
        np.random.seed(1)
        aug = front.prepare(EventBatch.from_numpy(rows, 480, 640), t_base=np.asarray(bases, np.int64), params=front.draw([n] * B), want_xy=False)
        assert not aug.status.any()
        prim = aug.batch.polstats(aug.tnorm, ni.DIST_POL, ni.DIST_STAT)
        out = torch.empty((B, 2, H, W), dtype=torch.float32, device="cuda")
        scratch = torch.empty(int(lib.evrep_dist_scratch_bytes(B, H, W)), dtype=torch.uint8, device="cuda")
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

        def dist():
            assert lib.evrep_dist(ptr(prim), B, H, W, ni.CLIP_COUNT_RATE, ni.DISC_ALPHA, ptr(out), ptr(scratch), stream) == 0

        row = dict(windows=B, kept_rows=int(aug.batch.total), scratch_bytes=int(scratch.numel()))
        row["torch_route_us"] = round(median_host_us(lambda: torch_route(prim), max(3, args.reps // 10)), 1)
        row["dist_us"] = round(median_us(dist, args.reps), 2)
        worst = float((out - torch_route(prim)).abs().max())
        assert worst <= 1e-6, "evrep_dist and the torch route disagree by %g" % worst
        row["polstats_us"] = round(median_us(lambda: aug.batch.polstats(aug.tnorm, ni.DIST_POL, ni.DIST_STAT, out=prim), args.reps), 2)
        nbytes = B * H * W * (6 + 2) * 4
        src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        row["d2d_copy_us"], row["bytes"] = round(median_us(lambda: dst.copy_(src), args.reps), 2), nbytes
        row["dist_over_copy"] = round(row["dist_us"] / row["d2d_copy_us"], 2)
        row["dist_over_polstats"] = round(row["dist_us"] / row["polstats_us"], 2)
        row["torch_route_over_dist"] = round(row["torch_route_us"] / row["dist_us"], 1)
        result["sets"][sname] = row
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
