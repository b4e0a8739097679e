#!/usr/bin/env python3
"""Times of the training targets (detector_assign.assign_batch) beside the reference's route, measured in the same run.

    python tools/bench_detector_assign.py [--reps 50] [--out FILE.json]

B = 32 images at 640 x 640 (A = 8400 anchors), nc in {2, 80}, 5 and 50 labels per image (tests/detector_assign_cases: uniform
scores, a predicted box about every anchor).  Medians over `reps` runs after warm-up, in us:
  (a) reference_route   the statements of ComputeLoss.preprocess (targets to the host, a Python loop over every label, back to
                        the device) and of TaskAlignedAssigner.forward restated as torch calls on the device: the (B, M, A)
                        tensors and the int64 one-hot of (B, M, 13, A) included.  Host clock, device drained before and after.
  (b) assign_batch      HIP events around the call: the padding launch, the memset and the four launches of the assigner, the
                        outputs and the scratch from torch's caching allocator (targets already on the device, max_labels given).
  (c) kernels           the launches apart, from torch.profiler's device times (null where the profiler gives none).
  (d) copy              HIP events around a device-to-device copy of the four outputs: what writing them once costs.
Also torch.cuda.max_memory_allocated over one call of (a) beside the scratch plus outputs of (b), in MB.
The expectations are (b) < (a) and, at nc = 80, the score launch near (d); the tool prints the figures and asserts nothing
about them.  It does compare the two routes' labels, boxes and fg, and their scores within 64 * 2^-53 relative."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import detector_assign_cases as cases  # noqa: E402
from event_representation_study_amd import _lib, detector_assign as da  # noqa: E402

S, TOPK, EPS = 640, 13, 1e-9


def reference_preprocess(targets, B, scale):
    """ComputeLoss.preprocess: a host round trip and a Python loop."""
    per_image = [[] for _ in range(B)]
    for row in targets.cpu().numpy().tolist():
        per_image[int(row[0])].append(row[1:])
    M = max(len(r) for r in per_image)
    padded = np.array([r + [[-1, 0, 0, 0, 0]] * (M - len(r)) for r in per_image], dtype=np.float64).reshape(B, M, 5)
    t = torch.from_numpy(padded).to(targets.device)
    box = t[:, :, 1:5] * scale
    x1, y1 = box[..., 0] - box[..., 2] / 2, box[..., 1] - box[..., 3] / 2
    t[..., 1:] = torch.stack([x1, y1, x1 + box[..., 2], y1 + box[..., 3]], -1)
    return t


def reference_assign(pd_scores, pd_bboxes, anc, gt, nc):
    """TaskAlignedAssigner.forward for M <= 100 as torch calls: every (B, M, A) tensor of the reference is made."""
    B, A, M = pd_scores.shape[0], pd_scores.shape[1], gt.shape[1]
    gt_labels, gt_bboxes = gt[:, :, :1], gt[:, :, 1:]
    mask_gt = (gt_bboxes.sum(-1, keepdim=True) > 0).float()
    idx = gt_labels.long().squeeze(-1)
    bbox_scores = pd_scores.permute(0, 2, 1)[torch.arange(B, device=gt.device).view(-1, 1).repeat(1, M), idx]
    g, p = gt_bboxes.unsqueeze(2), pd_bboxes.unsqueeze(1)
    overlap = (torch.minimum(g[..., 2:], p[..., 2:]) - torch.maximum(g[..., :2], p[..., :2])).clip(0).prod(-1)
    area_g, area_p = (g[..., 2:] - g[..., :2]).clip(0).prod(-1), (p[..., 2:] - p[..., :2]).clip(0).prod(-1)
    overlaps = overlap / (area_g + area_p - overlap + EPS)
    align = bbox_scores.pow(1.0) * overlaps.pow(6.0)
    flat = gt_bboxes.reshape(-1, 4)
    centres = anc.unsqueeze(0).repeat(B * M, 1, 1)
    deltas = torch.cat([centres - flat[:, :2].unsqueeze(1).repeat(1, A, 1), flat[:, 2:].unsqueeze(1).repeat(1, A, 1) - centres], -1)
    in_gts = (deltas.reshape(B, M, A, 4).min(-1)[0] > EPS).to(gt.dtype)
    _, topk_idx = torch.topk(align * in_gts, TOPK, dim=-1)
    topk_idx = torch.where(mask_gt.repeat(1, 1, TOPK).bool(), topk_idx, torch.zeros_like(topk_idx))
    in_topk = F.one_hot(topk_idx, A).sum(-2)
    in_topk = torch.where(in_topk > 1, torch.zeros_like(in_topk), in_topk).to(align.dtype)
    mask_pos = in_topk * in_gts * mask_gt
    fg = mask_pos.sum(-2)
    if fg.max() > 1:
        multi = (fg.unsqueeze(1) > 1).repeat(1, M, 1)
        is_max = F.one_hot(overlaps.argmax(1), M).permute(0, 2, 1).to(overlaps.dtype)
        mask_pos = torch.where(multi, is_max, mask_pos)
        fg = mask_pos.sum(-2)
    gt_idx = mask_pos.argmax(-2) + torch.arange(B, device=gt.device)[:, None] * M
    labels = gt_labels.long().flatten()[gt_idx]
    boxes = gt_bboxes.reshape(-1, 4)[gt_idx]
    labels[labels < 0] = 0
    scores = torch.where(fg[:, :, None].repeat(1, 1, nc) > 0, F.one_hot(labels, nc), torch.zeros((), dtype=torch.int64, device=gt.device))
    align = align * mask_pos
    pos_align = align.max(-1, keepdim=True)[0]
    pos_overlaps = (overlaps * mask_pos).max(-1, keepdim=True)[0]
    norm = (align * pos_overlaps / (pos_align + EPS)).max(-2)[0].unsqueeze(-1)
    return labels, boxes, scores * norm, fg.bool()


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
            for name in ("k_det_targets_pad", "k_tal_prepare", "k_tal_select", "k_tal_resolve", "k_tal_scores"):
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
        raise SystemExit("bench_detector_assign needs the GPU: no time is taken without one")
    dev, B = torch.device("cuda:0"), args.batch
    rows = []
    for nc in (2, 80):
        scores_h, boxes_h, anc_h = cases.head(7000 + nc, B, S, nc)
        s, p, a = (torch.from_numpy(v).to(dev) for v in (scores_h, boxes_h, anc_h))
        A = len(anc_h)
        for n_lab in (5, 50):
            t = torch.from_numpy(cases.targets(7100 + n_lab, [n_lab] * B, nc)).to(dev)
            scale = torch.tensor([S, S, S, S], dtype=torch.float32, device=dev)

            def ref():
                return reference_assign(s, p, a, reference_preprocess(t, B, scale), nc)

            def ours():
                return da.assign_batch(s, p, a, t, (S, S), nc, max_labels=n_lab)

            r, o = ref(), ours()
            same = bool(torch.equal(r[0], o[0]) and torch.equal(r[1], o[1]) and torch.equal(r[3], o[3]))
            nz = r[2] != 0
            same_zero = bool(torch.equal(nz, o[2] != 0))
            rel = float(((r[2] - o[2]).abs()[nz] / r[2][nz].abs()).max()) if bool(nz.any()) else 0.0
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            ref()
            torch.cuda.synchronize()
            ref_mb = (torch.cuda.max_memory_allocated() - base) / 1e6
            out_bytes = sum(x.numel() * x.element_size() for x in o[:4])
            ours_mb = (int(_lib.load().evrep_tal_workspace_bytes(B, n_lab, A)) + out_bytes + B * n_lab * 40) / 1e6
            t_ref = host_us(ref, max(args.reps // 5, 5))
            t_ours = event_us(ours, args.reps)
            spare = [torch.empty_like(x) for x in o[:4]]
            t_copy = event_us(lambda: [d.copy_(x) for d, x in zip(spare, o[:4])], args.reps)
            row = {"B": B, "A": A, "nc": nc, "labels_per_image": n_lab, "reps": args.reps, "foreground": int(o[3].sum()),
                   "reference_route_host_us": round(t_ref, 1), "assign_batch_us": round(t_ours, 1), "copy_us": round(t_copy, 1),
                   "reference_over_assign": round(t_ref / t_ours, 1), "kernels_us": kernel_us(ours, 10),
                   "reference_peak_mb": round(ref_mb, 1), "assign_scratch_and_outputs_mb": round(ours_mb, 1),
                   "discrete_outputs_equal": same, "score_zero_pattern_equal": same_zero, "score_rel_err": rel}
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
