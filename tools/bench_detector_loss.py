#!/usr/bin/env python3
"""Times of the loss terms (detector_loss.loss_batch, forward and backward) beside the reference's route, in the same run.

    python tools/bench_detector_loss.py [--reps 50] [--out FILE.json]

B = 32 images at 640 x 640 (A = 8400 anchors), nc in {2, 80}, 5 and 50 labels per image; the targets are assign_batch's on
tests/detector_assign_cases' head, the logits tests/detector_loss_cases'.  Medians over `reps` runs after warm-up, in us:
  (a) reference_route   the statements of loss.py:176-217 with VarifocalLoss, BboxLoss and IOUloss restated as torch calls on the
                        device in float32 predictions and float64 targets (tests/detector_loss_ref.py): the int64 one-hot, the
                        masked_selects, the softmaxes, the two reads of the device, and autograd's backward.  Host clock, device
                        drained before and after (the route reads the device twice, so events would not bracket it).
  (b) loss_batch        HIP events around loss_batch(...) and loss.backward(): the memset and the four launches, the few scalar
                        torch calls that weight the terms, the two multiplications by grad_output; outputs and scratch from torch's
                        caching allocator.
  (c) kernels           the launches apart, from torch.profiler's device times (null where the profiler gives none).
  (d) copy              HIP events around a device-to-device copy of the two gradient arrays: what writing them once costs.
Also torch.cuda.max_memory_allocated over one call of (a) beside the scratch plus outputs of (b), in MB.
The expectation is (b) < (a); the tool prints the figures and `b_below_a`, and asserts nothing about them.  It does compare
the two routes' losses (1e-5 relative: the reference route runs its BCE and softmaxes in float32)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import detector_assign_cases as acases  # noqa: E402
import detector_loss_cases as lcases  # noqa: E402
import detector_loss_ref as ref  # noqa: E402
from event_representation_study_amd import _lib, detector_assign as da, detector_loss as dl  # noqa: E402

S, R = 640, 16
KERNELS = ("k_detloss_rows", "k_detloss_cls", "k_detloss_box", "k_detloss_fold", "k_detloss_decode")


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


def kernel_us(launch, reps):
    """Mean device time per launch of each of the library's kernels, by name; {} where the profiler gives none."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                launch()
            torch.cuda.synchronize()
        out = {}
        for e in prof.key_averages():
            for name in KERNELS:
                if name in e.key:
                    total = getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0)
                    out[name] = round(float(total) / max(e.count, 1), 1)
        return out
    except Exception as exc:  # the figures of (c) are optional: say why they are missing
        return {"error": repr(exc)[:200]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_detector_loss needs the GPU: no time is taken without one")
    dev, B = torch.device("cuda:0"), args.batch
    rows = []
    for nc in (2, 80):
        scores_h, _, anc_h = acases.head(8000 + nc, B, S, nc)
        z_h = lcases.base(8001 + nc, S=S, B=B, nc=1)["z"]
        anc, stride = (torch.from_numpy(v).to(dev) for v in da.anchor_points(S))
        p0, z0 = torch.from_numpy(scores_h).to(dev), torch.from_numpy(z_h).to(dev)
        A = len(anc_h)
        for n_lab in (5, 50):
            t = torch.from_numpy(acases.targets(8100 + n_lab, [n_lab] * B, nc)).to(dev)
            _, boxes_px = dl.decode_boxes(z0, anc, stride, R, True)
            labels, tb, ts, fg, _ = da.assign_batch(p0, boxes_px, anc, t, (S, S), nc, max_labels=n_lab)

            def reference():
                return ref.loss_terms(p0, z0, anc, stride, labels, tb, ts, fg, nc, R, True, lcases.WEIGHTS, dtype=torch.float32,
                                      scalars=False)

            def ours():
                p, z = p0.detach().requires_grad_(True), z0.detach().requires_grad_(True)
                loss, items = dl.loss_batch(p, z, anc, stride, labels, tb, ts, fg, nc, R, True)
                loss.backward()
                return loss, items, p.grad, z.grad

            def forward_only():
                with torch.no_grad():
                    return dl.loss_batch(p0, z0, anc, stride, labels, tb, ts, fg, nc, R, True)

            r, o = reference(), ours()
            rel = abs(float(r["loss"]) - float(o[0])) / abs(float(o[0]))
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            reference()
            torch.cuda.synchronize()
            ref_mb = (torch.cuda.max_memory_allocated() - base) / 1e6
            out_bytes = sum(x.numel() * x.element_size() for x in o[2:]) + 5 * 8 + B * 4
            ours_mb = (int(_lib.load().evrep_detloss_workspace_bytes(B, A, nc)) + out_bytes) / 1e6
            t_ref = host_us(reference, max(args.reps // 5, 5))
            t_ours = event_us(ours, args.reps)
            t_fwd = event_us(forward_only, args.reps)
            spare = [torch.empty_like(x) for x in o[2:]]
            t_copy = event_us(lambda: [d.copy_(x) for d, x in zip(spare, o[2:])], args.reps)
            t_decode = event_us(lambda: dl.decode_boxes(z0, anc, stride, R, True), args.reps)
            row = {"B": B, "A": A, "nc": nc, "labels_per_image": n_lab, "reps": args.reps, "foreground": int(fg.sum()),
                   "reference_route_host_us": round(t_ref, 1), "loss_batch_fwd_bwd_us": round(t_ours, 1),
                   "loss_batch_no_grad_us": round(t_fwd, 1), "decode_boxes_us": round(t_decode, 1), "copy_us": round(t_copy, 1),
                   "reference_over_loss_batch": round(t_ref / t_ours, 1), "b_below_a": bool(t_ours < t_ref),
                   "kernels_us": kernel_us(ours, 10), "reference_peak_mb": round(ref_mb, 1),
                   "loss_scratch_and_outputs_mb": round(ours_mb, 1), "loss_rel_diff": rel, "losses_agree": bool(rel < 1e-5)}
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
