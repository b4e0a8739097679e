#!/usr/bin/env python3
"""HIP-event times of the study's representations on an N-ImageNet batch kept on the device (evrep_nimg_study_rows, the batched
builder, the cast and transpose), beside the route they replace and a yardstick measured in the same run.

    python tools/bench_nimg_study.py [--reps 50] [--events 30000] [--out FILE.json]

32 and 256 windows of 30 000 events, 640x480 -> 224x224, train mode (time flip, x flip, shift + crop drawn per window), prepared on
the device by NImageNetFrontEnd.  Per set and name ("optimized", "event_stack", "tore"), median us over `reps` runs after warm-up:
  (a) per_sample    the route this replaces: n_imagenet_acc.reshape_then_<name> in a Python loop over the windows' HOST tensors
                    (an upload, the builder, a read-back and a host cast per window); a host clock around a synchronise;
  (b) study_device  n_imagenet_front.study_device(name, aug, check=False): everything resident (HIP events; the plan, the
                    workspace, output and scratch allocations of the call included);
  (c) study_rows    evrep_nimg_study_rows alone, writing the one row set the name needs, beside the bytes it moves;
  (d) builder       the builder launch alone on the batch of those rows (binning done);
  (e) d2d_copy      torch's device-to-device copy of the output bytes of (b).
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

from event_representation_study_amd import _lib  # noqa: E402
from event_representation_study_amd import n_imagenet_acc as ni  # noqa: E402
from event_representation_study_amd import n_imagenet_front as nf  # noqa: E402
from event_representation_study_amd.engine import EventBatch  # noqa: E402

SETS = {"32x30000": 32, "256x30000": 256}
WANT = {"optimized": ("mdes", _lib.STUDY_MDES), "event_stack": ("stack", _lib.STUDY_STACK), "tore": ("tore", _lib.STUDY_TORE)}


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


def same(a, b):
    """Bit-equal, NaNs as positions (ERGO-12 of a window inside one whole second holds the reference's 0 / 0)."""
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--events", type=int, default=30000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_nimg_study.py needs a HIP device"
    assert args.reps >= 50 or args.events < 30000, "at least 50 repetitions at the full size"
    front = nf.NImageNetFrontEnd(types.SimpleNamespace(reshape=True, mode="train"), "train")
    result = dict(bench="nimg_study", events_per_window=args.events, reps=args.reps, sets={})
    for sname, B in SETS.items():
        rng = np.random.default_rng(2)
        n = args.events
        rows, bases = [], []
        for b in range(B):
            x, y = rng.integers(0, 640, n), rng.integers(0, 480, n)
            t = (np.sort(rng.integers(0, 50_000, n)) + 1_600_000_000_980_000 + b * 60_000).astype(np.int64)
            rows.append(np.stack([x, y, t - t[0], rng.integers(0, 2, n)], axis=1).astype(np.int32))
            bases.append(t[0])
        np.random.seed(1)
        aug = front.prepare(EventBatch.from_numpy(rows, 480, 640), t_base=np.asarray(bases, np.int64), params=front.draw([n] * B))
        assert not (aug.status & _lib.AUG_EMPTY).any()
        # the host tensors the per-sample route takes: the augmented rows, read back once
        xy, tt, pp, off = aug.xy.cpu().numpy(), aug.t.cpu().numpy(), aug.batch.events[:, 3].cpu().numpy(), aug.batch.offsets_host.numpy()
        host = [np.column_stack([xy[off[b]:off[b + 1]], tt[off[b]:off[b + 1]], pp[off[b]:off[b + 1]]]) for b in range(B)]
        row = dict(windows=B, kept_rows=int(aug.batch.total))
        for name, (key, bit) in WANT.items():
            fn = getattr(ni, "reshape_then_" + name)

            def per_sample():
                return torch.stack([fn(torch.from_numpy(w.copy())) for w in host])

            out = nf.study_device(name, aug)
            assert same(out.cpu(), per_sample()), "study_device and the per-sample route disagree (%s)" % name
            row[name + "_per_sample_us"] = round(median_host_us(per_sample, max(3, args.reps // 10)), 1)
            row[name + "_study_device_us"] = round(median_us(lambda: nf.study_device(name, aug, check=False), args.reps), 2)
            row[name + "_per_sample_over_study_device"] = round(row[name + "_per_sample_us"] / row[name + "_study_device_us"], 1)
            row[name + "_study_rows_us"] = round(median_us(lambda: ni._study_rows(aug.batch, aug.t, aug.xy, bit), args.reps), 2)
            # rows in (16 B) and t (8 B) twice -- both passes read them --, xy (16 B) twice for TORE, one row set out (16 B)
            row[name + "_study_rows_bytes"] = int(aug.batch.total) * (2 * (24 + (16 if name == "tore" else 0)) + 16)
            r = ni._study_rows(aug.batch, aug.t, aug.xy, bit)
            nb = EventBatch(r[key], aug.batch.offsets_host, 224, 224, plan_flags=int(aug.batch.plan.flags)).bin()
            if name == "optimized":
                rep = nb.optimized(scale=1.0, dtype=torch.float64)
                build = lambda: nb.optimized(scale=1.0, dtype=torch.float64, out=rep)
            elif name == "event_stack":
                rep = nb.event_stack(12, premap=2, scale=1.0)
                build = lambda: nb.event_stack(12, premap=2, scale=1.0, out=rep)
            else:
                rep = nb.tore(k=6, frame_mode=2, scale=1.0, times_f64=aug.t, sample_times_f64=r["sample_times"])
                build = lambda: nb.tore(k=6, frame_mode=2, scale=1.0, out=rep, times_f64=aug.t, sample_times_f64=r["sample_times"])
            row[name + "_builder_us"] = round(median_us(build, args.reps), 2)
            del rep, nb, r
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
