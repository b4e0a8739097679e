#!/usr/bin/env python3
"""Times of the detector's output step (detector_output.nms_batch / non_max_suppression) beside the part of the reference's
route that can run on this stack, measured in the same run.

    python tools/bench_detector_output.py [--reps 50] [--out FILE.json]

Synthetic head outputs at N = 8400 (a 640 x 640 YOLOv6 head), B in {1, 32}, C = 2 (Gen1) and C = 80, under the evaler's
setting (conf 0.03, iou 0.65, multi_label) and the inferer's (0.25, 0.45).  Boxes are jittered around 60 centres per image;
obj = u^6, one class per box scores u, the others 0.2 * u^8 (u uniform): the candidate fraction and the rows per image that
result are printed with every line.  Medians over `reps` runs after warm-up, in us:
  (a) torch_pre_nms   the reference's statements as torch calls on the device, image by image, UP TO BUT NOT INCLUDING the nms
                      call: candidates, products, corners, nonzero / max, the classes filter, the class offset.  Its nonzero
                      waits for the device every image, so it is timed on a host clock with the device drained.  It cannot
                      include torchvision.ops.nms, which is absent here: the column is a LOWER bound of the reference's route.
  (b) nms_batch       HIP events around the one launch (scratch from torch's caching allocator included).
  (c) non_max_suppression   (b) + the read-back of the counts + the split into B views, on a host clock, device drained.
  (d) copy            HIP events around a device-to-device copy of the prediction's bytes: what moving the input once costs.
  (e) the phases of (b) -- rows, sort, greedy pass -- are one launch and are not timed apart.
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

from event_representation_study_amd import detector_output as do  # noqa: E402

N = 8400
SETTINGS = {"evaler": dict(conf_thres=0.03, iou_thres=0.65, multi_label=True), "inferer": dict(conf_thres=0.25, iou_thres=0.45)}


def head_output(B, C, seed=0):
    rng = np.random.default_rng(seed)
    pred = np.empty((B, N, 5 + C), np.float32)
    for b in range(B):
        centres, sizes = rng.uniform(40, 600, (60, 2)), rng.uniform(12, 160, (60, 2))
        pick = rng.integers(0, 60, N)
        pred[b, :, 0:2] = centres[pick] + rng.normal(0, 6, (N, 2))
        pred[b, :, 2:4] = sizes[pick] * rng.uniform(0.8, 1.25, (N, 2))
        pred[b, :, 4] = rng.uniform(0, 1, N) ** 6
        pred[b, :, 5:] = 0.2 * rng.uniform(0, 1, (N, C)) ** 8
        pred[b, np.arange(N), 5 + rng.integers(0, C, N)] = rng.uniform(0, 1, N)
    return pred


def torch_pre_nms(prediction, conf_thres, iou_thres, multi_label=False, classes=None, agnostic=False):
    """What the reference does per image in front of torchvision.ops.nms, as torch calls; returns the nms inputs."""
    C = prediction.shape[2] - 5
    cand = torch.logical_and(prediction[..., 4] > conf_thres, torch.max(prediction[..., 5:], dim=-1)[0] > conf_thres)
    multi_label = multi_label and C > 1
    out = []
    for b, x in enumerate(prediction):
        x = x[cand[b]]
        if not x.shape[0]:
            continue
        x[:, 5:] *= x[:, 4:5]
        box = do.xywh2xyxy(x[:, :4])
        if multi_label:
            bi, ci = (x[:, 5:] > conf_thres).nonzero(as_tuple=False).T
            x = torch.cat((box[bi], x[bi, ci + 5, None], ci[:, None].float()), 1)
        else:
            conf, ci = x[:, 5:].max(1, keepdim=True)
            x = torch.cat((box, conf, ci.float()), 1)[conf.view(-1) > conf_thres]
        if not x.shape[0]:
            continue
        if x.shape[0] > do.MAX_NMS:
            x = x[x[:, 4].argsort(descending=True)[:do.MAX_NMS]]
        off = x[:, 5:6] * (0 if agnostic else do.MAX_WH)
        out.append((x[:, :4] + off, x[:, 4]))
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
        raise SystemExit("bench_detector_output needs the GPU: no time is taken without one")
    dev = torch.device("cuda:0")
    rows = []
    for C in (2, 80):
        for B in (1, 32):
            host = head_output(B, C)
            pred = torch.from_numpy(host).to(dev)
            spare = torch.empty_like(pred)
            for name, kw in SETTINGS.items():
                ct = np.float32(kw["conf_thres"])
                cand = (host[..., 4] > ct) & (host[..., 5:].max(-1) > ct)
                conf = host[..., 5:] * host[..., 4:5]
                n_rows = ((conf > ct) & cand[..., None]).sum((1, 2)) if (kw.get("multi_label") and C > 1) else (cand & (conf.max(-1) > ct)).sum(1)
                det, count = do.nms_batch(pred, **kw)
                listed = do.non_max_suppression(pred, **kw)
                same = all(torch.equal(listed[b], det[b, :int(count[b])]) for b in range(B))
                t_ref = host_us(lambda: torch_pre_nms(pred, **kw), args.reps)
                t_batch = event_us(lambda: do.nms_batch(pred, **kw), args.reps)
                t_list = host_us(lambda: do.non_max_suppression(pred, **kw), args.reps)
                t_copy = event_us(lambda: spare.copy_(pred), args.reps)
                row = {"B": B, "N": N, "C": C, "setting": name, "reps": args.reps,
                       "candidate_fraction": round(float(cand.mean()), 4), "rows_per_image": round(float(n_rows.mean()), 1),
                       "kept_per_image": round(float(count.float().mean()), 1),
                       "torch_pre_nms_host_us": round(t_ref, 1), "nms_batch_us": round(t_batch, 1),
                       "non_max_suppression_host_us": round(t_list, 1), "copy_us": round(t_copy, 1),
                       "phases_us": None, "pre_nms_over_batch": round(t_ref / t_batch, 2), "list_equals_batch": same}
                rows.append(row)
                print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    if not all(r["list_equals_batch"] for r in rows):
        raise SystemExit("non_max_suppression and nms_batch differ")


if __name__ == "__main__":
    main()
