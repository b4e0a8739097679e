#!/usr/bin/env python3
"""HIP-event times of N-ImageNet's event front end on the device (n_imagenet_front.NImageNetFrontEnd, evrep_nimg_prepare), beside
the route it replaces and two yardsticks measured in the same run.

    python tools/bench_nimg_front.py [--reps 50] [--events 30000] [--out FILE.json]

32 and 256 windows of 30 000 events, 640x480 -> 224x224, train mode (time flip, x flip, shift + crop drawn per window).  Per
set, median us over `reps` launches after warm-up:
  (a) host_route   the host route: base_augment("train") per sample on the parsed float64 tensors (cloned per repetition, the
                   augmentation works in place) + n_imagenet_acc._window + EventBatch.from_numpy + the tnorm upload (a host clock
                   around a synchronise);
  (b) prepare      evrep_nimg_prepare alone, tables and outputs resident, without xy_out (HIP events);
  (c) d2d_copy     torch's device-to-device copy of the bytes (b) moves algorithmically: 16 B read and 32 B written per kept row;
  (d) binning      the binning pass of the prepared batch.
GB/s is on the algorithmic 48 B per kept row.  One JSON line.
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

ROW_BYTES = 48
SETS = {"32x30000": 32, "256x30000": 256}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--events", type=int, default=30000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_nimg_front.py needs a HIP device"
    assert args.reps >= 50 or args.events < 30000, "at least 50 repetitions at the full size"
    lib = _lib.load()
    cfg = types.SimpleNamespace(reshape=True, mode="train")
    front = nf.NImageNetFrontEnd(cfg, "train")
    result = dict(bench="nimg_front", events_per_window=args.events, reps=args.reps, row_bytes=ROW_BYTES, sets={})
    for sname, B in SETS.items():
        rng = np.random.default_rng(2)
        n = args.events
        wins, rows, bases = [], [], []
        for b in range(B):
            x, y = rng.integers(0, 640, n).astype(np.uint16), rng.integers(0, 480, n).astype(np.uint16)
            t = (np.sort(rng.integers(0, 50_000, n)) + 1_600_000_000_000_000 + b * 60_000).astype(np.int64)
            p = rng.integers(0, 2, n).astype(np.int8)
            wins.append((x, y, t, p))
            rows.append(np.stack([x, y, t - t[0], p], axis=1).astype(np.int32))
            bases.append(t[0])
        np.random.seed(1)
        par = front.draw([n] * B)
        # the parsed float64 tensors the host route starts from (load_event + reshape: not timed)
        parsed = [nf.reshape_event_no_sample(torch.from_numpy(nf.event_rows(*w)), 480, 640, 224, 224) for w in wins]

        def host_route():
            packed = []
            for b, ev in enumerate(parsed):
                f = int(par["flags"][b])
                out = nf.apply_augment(ev.clone(), f & _lib.AUG_TIME_FLIP, f & _lib.AUG_X_FLIP, par["x_shift"][b], par["y_shift"][b])
                packed.append(ni._window(out.numpy(), 224, 224))
            batch = EventBatch.from_numpy([r for r, _ in packed], 224, 224)
            tnorm = torch.from_numpy(np.concatenate([t for _, t in packed])).to(batch.device)
            return batch, tnorm

        batch = EventBatch.from_numpy(rows, 480, 640)
        total = batch.total
        table = torch.from_numpy(np.concatenate([par.view(np.uint8), np.asarray(bases, np.int64).view(np.uint8)])).cuda()
        ev_out = torch.empty((total, 4), dtype=torch.int32, device="cuda")
        t_out, tn_out = torch.empty(total, dtype=torch.float64, device="cuda"), torch.empty(total, dtype=torch.float64, device="cuda")
        meta = torch.empty((B + 1) * 8 + B * 4, dtype=torch.uint8, device="cuda")
        scratch = torch.empty(int(lib.evrep_nimg_prepare_scratch_bytes(B, total)), dtype=torch.uint8, device="cuda")
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

        def prepare():
            rc = lib.evrep_nimg_prepare(ptr(batch.events), ptr(batch.offsets), B, ptr(table[B * 48:]), ptr(table), front.sx, front.sy, 224,
                                        224, _lib.NIMG_TRAIN | _lib.NIMG_P_UINT8, ptr(ev_out), ptr(t_out), ptr(tn_out), None, ptr(meta),
                                        ptr(meta[(B + 1) * 8:]), ptr(scratch), stream)
            assert rc == 0

        row = dict(windows=B, rows=total)
        row["host_route_us"] = round(median_host_us(host_route, max(5, args.reps // 10)), 1)
        us = median_us(prepare, args.reps)
        want, want_tn = host_route()
        kept = int(meta[B * 8:(B + 1) * 8].cpu().numpy().view(np.int64)[0])
        assert kept == want.total and torch.equal(ev_out[:kept], want.events), "the device and the host route disagree"
        assert np.array_equal(tn_out[:kept].cpu().numpy(), want_tn.cpu().numpy(), equal_nan=True)
        row["kept_rows"], row["bytes"] = kept, kept * ROW_BYTES
        row["prepare_us"], row["prepare_GBps"] = round(us, 2), round(kept * ROW_BYTES / us / 1e3, 1)
        # a copy of N bytes reads N and writes N: 48 B per kept row are matched by a copy of 24 B per kept row
        src = torch.empty(kept * ROW_BYTES // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        us_c = median_us(lambda: dst.copy_(src), args.reps)
        row["d2d_copy_us"], row["d2d_copy_GBps"] = round(us_c, 2), round(kept * ROW_BYTES / us_c / 1e3, 1)
        us_b = median_us(lambda: want.rebin(), args.reps)
        row["binning_us"], row["binning_pass"] = round(us_b, 2), int(want.plan.reserved)
        row["prepare_over_copy"], row["prepare_over_binning"] = round(us / us_c, 2), round(us / us_b, 2)
        row["host_route_over_prepare"] = round(row["host_route_us"] / us, 1)
        result["sets"][sname] = row
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
