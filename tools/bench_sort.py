#!/usr/bin/env python3
"""HIP-event times of the batched sorted timestamp image on the device (evrep_time_index, polstats, evrep_sort_image), beside the
route it replaces and two yardsticks measured in the same run.

    python tools/bench_sort.py [--reps 50] [--events 30000] [--out FILE.json]

32 and 256 windows of 30 000 events, 640x480 -> 224x224, train mode (time flip, x flip, shift + crop drawn per window), prepared on
the device by NImageNetFrontEnd; strict and non-strict, global_time=True, both polarities, with the event image, no quantisation.
Per set and mode, median us over `reps` runs after warm-up:
  (a) torch_route  the route this replaces: n_imagenet_acc.reshape_then_acc_sort in a Python loop over the windows' HOST tensors
                   (its one form: an upload, a host unique_consecutive and the image statements per window); a host clock around a
                   synchronise, since torch.unique, boolean-mask indexing and bool() synchronise on their own;
  (b) sort_device  n_imagenet_front.sort_device(aug, check=False): the three calls, everything resident (HIP events; the output
                   and scratch allocations of the call included);
  (c) polstats     the polstats launch of the same batch alone (binning done);
  (d) d2d_copy     torch's device-to-device copy of the output bytes of (b).
The tool checks that (a) and (b) agree exactly.  One JSON line.
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from event_representation_study_amd import n_imagenet_acc as ni  # noqa: E402
from event_representation_study_amd import n_imagenet_front as nf  # noqa: E402
from event_representation_study_amd.engine import EventBatch  # noqa: E402

SETS = {"32x30000": 32, "256x30000": 256}
KW = dict(global_time=True, neglect_polarity=False, use_image=True, quantize_sort=None)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--events", type=int, default=30000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sort.py needs a HIP device"
    assert args.reps >= 50 or args.events < 30000, "at least 50 repetitions at the full size"
    front = nf.NImageNetFrontEnd(types.SimpleNamespace(reshape=True, mode="train"), "train")
    result = dict(bench="sort", events_per_window=args.events, reps=args.reps, sets={})
    for sname, B in SETS.items():
        rng = np.random.default_rng(2)
        n = args.events
        rows, bases = [], []
        for b in range(B):
            x, y = rng.integers(0, 640, n), rng.integers(0, 480, n)
            t = (np.sort(rng.integers(0, 50_000, n)) + 3_000_000 + b * 60_000).astype(np.int64)
            rows.append(np.stack([x, y, t - t[0], rng.integers(0, 2, n)], axis=1).astype(np.int32))
            bases.append(t[0])
        np.random.seed(1)
        aug = front.prepare(EventBatch.from_numpy(rows, 480, 640), t_base=np.asarray(bases, np.int64), params=front.draw([n] * B), want_xy=False)
        assert not aug.status.any()
        # the host tensors the torch route takes: the augmented rows, read back once
        ev, tt, off = aug.batch.events.cpu().numpy(), aug.t.cpu().numpy(), aug.batch.offsets_host.numpy()
        host = []
        for b in range(B):
            w = np.zeros((off[b + 1] - off[b], 4))
            w[:, 0], w[:, 1], w[:, 2], w[:, 3] = ev[off[b]:off[b + 1], 0], ev[off[b]:off[b + 1], 1], tt[off[b]:off[b + 1]], ev[off[b]:off[b + 1], 3]
            host.append(w)
        row = dict(windows=B, kept_rows=int(aug.batch.total))
        for strict in (True, False):
            tag = "strict" if strict else "loose"

            def torch_route():
                return torch.stack([ni.reshape_then_acc_sort(torch.from_numpy(w.copy()), strict=strict, denoise_image=False, denoise_sort=False,
                                                             keep_on_device=True, **KW) for w in host])

            out = nf.sort_device(aug, strict=strict, **KW)
            assert torch.equal(out, torch_route()), "sort_device and the torch route disagree (%s)" % tag
            row[tag + "_torch_route_us"] = round(median_host_us(torch_route, max(3, args.reps // 10)), 1)
            row[tag + "_sort_device_us"] = round(median_us(lambda: nf.sort_device(aug, strict=strict, check=False, **KW), args.reps), 2)
            row[tag + "_torch_route_over_sort_device"] = round(row[tag + "_torch_route_us"] / row[tag + "_sort_device_us"], 1)
        pol, stat = [ni.POS, ni.POS, ni.NEG, ni.NEG], [ni.FLAG, ni.TMAX] * 2
        prim = aug.batch.polstats(aug.t, pol, stat)
        row["polstats_us"] = round(median_us(lambda: aug.batch.polstats(aug.t, pol, stat, out=prim), args.reps), 2)
        nbytes = out.numel() * 4
        src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        row["d2d_copy_us"], row["bytes"] = round(median_us(lambda: dst.copy_(src), args.reps), 2), nbytes
        result["sets"][sname] = row
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
