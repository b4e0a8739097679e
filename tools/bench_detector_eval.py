#!/usr/bin/env python3
"""Times of the detection scoring (detector_eval.match_batch / DetectionEvaluator.update) beside the reference's route,
measured in the same run.

    python tools/bench_detector_eval.py [--reps 50] [--out FILE.json]

Synthetic batches as nms_batch leaves them: B in {1, 32} images, max_det 300 with every row filled, 5 or 50 labels per image
(tests/detector_eval_cases.batch: two thirds of the detections are jittered copies of labels), 10 thresholds, with and without
the confusion matrix.  Medians over `reps` runs after warm-up, in us:
  (a) reference_route   what evaler.py:209-258 does with the padded output of nms_batch: the detections go to the host, and per
                        image scale_coords, the label boxes, process_batch (per threshold: where -> numpy -> argsort -> unique ->
                        unique) and optionally the confusion matrix's pass, as torch / numpy calls in a Python loop.  Host clock,
                        device drained before and after.
  (b) match_batch       HIP events around the one launch (its output tensors from torch's caching allocator and the upload of
                        the B geometry rows included).
  (c) update            DetectionEvaluator.update: (b) + what it keeps for compute(), HIP events.
  (d) copy              HIP events around a device-to-device copy of det: what moving the input once costs.
The expectation is (b) < (a); the tool prints the ratio and asserts nothing about it.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import detector_eval_cases as cases  # noqa: E402
from event_representation_study_amd import detector_eval as de  # noqa: E402

NC = 3


def _scale_coords(coords, img0_shape, ratio_pad):
    gain, pad = ratio_pad[0], ratio_pad[1]
    coords[:, [0, 2]] -= pad[0]
    coords[:, [0, 2]] /= gain[0]
    coords[:, [1, 3]] -= pad[1]
    coords[:, [1, 3]] /= gain[0]
    for k in range(4):
        coords[:, k].clamp_(0, img0_shape[1 - k % 2])
    return coords


def _pairs(iou, mask, second_sort):
    """The reference's matching of one mask: [label, detection, iou] rows, best label per detection, then one per label."""
    x = torch.where(mask)
    if not x[0].shape[0]:
        return np.zeros((0, 3))
    m = torch.cat((torch.stack(x, 1), iou[x[0], x[1]][:, None]), 1).cpu().numpy()
    if x[0].shape[0] > 1:
        m = m[m[:, 2].argsort()[::-1]]
        m = m[np.unique(m[:, 1], return_index=True)[1]]
        if second_sort:
            m = m[m[:, 2].argsort()[::-1]]
        m = m[np.unique(m[:, 0], return_index=True)[1]]
    return m


def reference_route(det, count, targets, img_shape, shapes, iouv, matrix):
    """(a): returns the list of per-image correct matrices."""
    outputs = [det[b, :n].detach().cpu() for b, n in enumerate(count.tolist())]
    H, W = img_shape
    out = []
    for si, pred in enumerate(outputs):
        labels = targets[targets[:, 0] == si, 1:]
        if len(pred) == 0:
            continue
        predn = pred.clone()
        _scale_coords(predn[:, :4], shapes[si][0], shapes[si][1])
        correct = torch.zeros(pred.shape[0], iouv.shape[0], dtype=torch.bool)
        if len(labels):
            tbox = de.xywh2xyxy(labels[:, 1:5])
            tbox[:, [0, 2]] *= W
            tbox[:, [1, 3]] *= H
            _scale_coords(tbox, shapes[si][0], shapes[si][1])
            iou = de.box_iou(tbox, predn[:, :4])
            same = labels[:, 0:1] == predn[:, 5]
            c = np.zeros((pred.shape[0], iouv.shape[0]), bool)
            for i in range(len(iouv)):
                m = _pairs(iou, (iou >= iouv[i]) & same, False)
                c[m[:, 1].astype(int), i] = True
            correct = torch.tensor(c)
            if matrix is not None:
                keep = predn[:, 4] > 0.25
                dcls, gcls = predn[keep, 5].int(), labels[:, 0].int()
                iou_c = iou[:, keep]
                m = _pairs(iou_c, iou_c > 0.45, True)
                m0, m1 = m[:, 0].astype(int), m[:, 1].astype(int)
                for k, gc in enumerate(gcls):
                    j = m0 == k
                    if len(m) and j.sum() == 1:
                        matrix[dcls[m1[j]], gc] += 1
                    else:
                        matrix[NC, gc] += 1
                if len(m):
                    for j, dc in enumerate(dcls):
                        if not (m1 == j).any():
                            matrix[dc, NC] += 1
        out.append(correct)
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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_detector_eval needs the GPU: no time is taken without one")
    dev = torch.device("cuda:0")
    iouv = torch.linspace(0.5, 0.95, 10)
    rows = []
    for B in (1, 32):
        for n_lab in (5, 50):
            det_h, count_h, targets_h, shapes = cases.batch(B * 100 + n_lab, [n_lab] * B, [300] * B, nc=NC, max_det=300)
            det, count = torch.from_numpy(det_h).to(dev), torch.from_numpy(count_h).to(dev)
            targets_cpu, targets = torch.from_numpy(targets_h), torch.from_numpy(targets_h).to(dev)
            spare = torch.empty_like(det)
            for confusion in (False, True):
                cm = de.ConfusionMatrix(NC) if confusion else None
                ref_matrix = np.zeros((NC + 1, NC + 1)) if confusion else None
                ref = reference_route(det, count, targets_cpu, cases.IMG, shapes, iouv, ref_matrix)
                correct = de.match_batch(det, count, targets, cases.IMG, shapes, iouv, cm)[0]
                same = all(np.array_equal(ref[b].numpy(), correct[b, :300].cpu().numpy().astype(bool)) for b in range(B))
                if confusion:
                    same = same and np.array_equal(ref_matrix, cm.matrix)
                t_ref = host_us(lambda: reference_route(det, count, targets_cpu, cases.IMG, shapes, iouv,
                                                        np.zeros((NC + 1, NC + 1)) if confusion else None), args.reps)
                t_match = event_us(lambda: de.match_batch(det, count, targets, cases.IMG, shapes, iouv, cm), args.reps)
                ev = de.DetectionEvaluator(NC, iouv, confusion)

                def update():
                    ev._batches.clear()
                    ev.update(det, count, targets, cases.IMG, shapes)

                t_update = event_us(update, args.reps)
                t_copy = event_us(lambda: spare.copy_(det), args.reps)
                row = {"B": B, "max_det": 300, "labels_per_image": n_lab, "T": 10, "confusion": confusion, "reps": args.reps,
                       "correct_at_50_per_image": round(float(correct[:, :, 0].sum()) / B, 1),
                       "reference_route_host_us": round(t_ref, 1), "match_batch_us": round(t_match, 1), "update_us": round(t_update, 1),
                       "copy_us": round(t_copy, 1), "reference_over_match": round(t_ref / t_match, 1), "equals_reference_route": same}
                rows.append(row)
                print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    if not all(r["equals_reference_route"] for r in rows):
        raise SystemExit("match_batch and the reference's route differ (a label tie in the synthetic input?)")


if __name__ == "__main__":
    main()
