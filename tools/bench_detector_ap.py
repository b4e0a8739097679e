#!/usr/bin/env python3
"""Times of the evaluator's last step, mAP from the resident statistics: DetectionEvaluator.compute() (one read-back of every
padded tensor, a Python loop over the images, numpy's ap_per_class) beside compute_device() (evrep_det_ap_gather per batch,
evrep_det_ap, one read-back of the result), measured in the same run and process.

    python tools/bench_detector_ap.py [--reps 50] [--rows 100000,1000000] [--nc 2,80] [--out FILE.json]

Input: K scored batches of B = 32 images, max_det = 300 with every row filled, T = 10, pairwise distinct confidences, about
40 labels per batch and class; K is chosen so that K * 9 600 rows is about the number asked for.  Medians over `reps` runs
after warm-up, in us:
  (a) compute           host clock, device drained before and after, the read-back included.
  (b) compute_device    the same clock.
  (c) the launches of (b) apart, HIP events: gather (the 2 K launches of evrep_det_ap_gather), order (evrep_det_ap given no
      labels: keys, class counts, the radix sort, the tp sums -- where it stops), ap_total (evrep_det_ap whole); curves =
      ap_total - order: the count and maximum scans, the curves and the areas.
  (d) copy              HIP events around a device-to-device copy of the bytes (a) reads back.
and the bytes each route moves to the host.  The expectation is (b) < (a); the tool prints the ratio and asserts nothing about
it.  It does assert that the two routes agree (p, r, f1 equal, ap within 2.2e-14).
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

from event_representation_study_amd import _lib  # noqa: E402
from event_representation_study_amd import detector_eval as de  # noqa: E402

B, MAX_DET, T = 32, 300, 10


def batches(seed, K, nc, dev):
    rng = np.random.default_rng(seed)
    n = K * B * MAX_DET
    conf = rng.permutation(np.linspace(0.03, 0.999, n)).astype(np.float32)
    if np.unique(conf).size != n:
        raise SystemExit("the synthetic confidences tie: fewer rows, please")
    out = []
    for k in range(K):
        c = conf[k * B * MAX_DET:(k + 1) * B * MAX_DET].reshape(B, MAX_DET)
        cls = rng.integers(0, nc, (B, MAX_DET)).astype(np.float32)
        correct = (rng.random((B, MAX_DET, 1)) < 0.5 * np.linspace(1.0, 0.3, T)[None, None, :]).astype(np.uint8)
        n_t = 40 * nc
        targets = np.stack([rng.integers(0, B, n_t).astype(np.float32), np.arange(n_t, dtype=np.float32) % nc], axis=1)
        out.append(tuple(torch.from_numpy(a).to(dev) for a in
                         (correct, np.stack([c, cls], axis=2), np.full(B, MAX_DET, np.int32), targets, np.zeros(B, np.int32))))
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


def host_us(call, reps, warmup=3):
    times = []
    for k in range(warmup + reps):
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
    ap.add_argument("--rows", default="100000,1000000")
    ap.add_argument("--nc", default="2,80")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_detector_ap needs the GPU: no time is taken without one")
    dev = torch.device("cuda:0")
    rows = []
    for want in (int(v) for v in args.rows.split(",")):
        K = max(1, round(want / (B * MAX_DET)))
        for nc in (int(v) for v in args.nc.split(",")):
            ev = de.DetectionEvaluator(nc)
            for b in batches(K * 1000 + nc, K, nc, dev):
                ev.add_batch(*b)
            host, device = ev.compute(), ev.compute_device()
            same = all(np.array_equal(host[k], device[k]) for k in ("p", "r", "f1", "ap_class", "nt")) and \
                float(np.abs(host["ap"] - device["ap"]).max()) <= 2.2e-14
            n, m = K * B * MAX_DET, sum(int(b[3].shape[0]) for b in ev._batches)
            read_a = sum(t.numel() * t.element_size() for b in ev._batches for t in b)
            read_b = 8 * (3 * nc * _lib.AP_PX + nc * T + nc) + 8 + 4 * K * B
            t_a = host_us(ev.compute, args.reps)
            t_b = host_us(ev.compute_device, args.reps)
            # (c): the launches apart, on rows gathered once
            tp = torch.empty((n, T), dtype=torch.uint8, device=dev)
            conf, pcls = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
            tcls, cursor = torch.empty(m, dtype=torch.float32, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)

            def gather():
                cursor.zero_()
                for correct, conf_cls, count, tgt, _ in ev._batches:
                    _lib.api().evrep_det_ap_gather(_lib.ptr(correct), _lib.ptr(conf_cls), _lib.ptr(count), B, MAX_DET, T, _lib.ptr(tgt),
                                                   int(tgt.shape[0]), _lib.ptr(tp), _lib.ptr(conf), _lib.ptr(pcls), n, _lib.ptr(tcls), m,
                                                   _lib.ptr(cursor), _lib.stream_ptr())

            t_gather = event_us(gather, args.reps)
            ws = _lib.scratch(de.ap_workspace_bytes(n, T, nc), dev)
            out = de.ap_device(tp, conf, pcls, tcls, nc, workspace=ws)
            t_order = event_us(lambda: de.ap_device(tp, conf, pcls, tcls[:0], nc, out=out, workspace=ws), args.reps)
            t_total = event_us(lambda: de.ap_device(tp, conf, pcls, tcls, nc, out=out, workspace=ws), args.reps)
            src = torch.empty(read_a, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            t_copy = event_us(lambda: dst.copy_(src), args.reps)
            row = {"rows": n, "batches": K, "B": B, "max_det": MAX_DET, "T": T, "nc": nc, "labels": m, "reps": args.reps,
                   "compute_host_us": round(t_a, 1), "compute_device_host_us": round(t_b, 1), "compute_over_compute_device": round(t_a / t_b, 1),
                   "gather_us": round(t_gather, 1), "order_us": round(t_order, 1), "ap_total_us": round(t_total, 1),
                   "curves_us": round(t_total - t_order, 1), "copy_us": round(t_copy, 1), "read_back_bytes_compute": read_a,
                   "read_back_bytes_compute_device": read_b, "map50": round(float(device["map50"]), 6), "routes_agree": same}
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    if not all(r["routes_agree"] for r in rows):
        raise SystemExit("compute() and compute_device() differ")


if __name__ == "__main__":
    main()
