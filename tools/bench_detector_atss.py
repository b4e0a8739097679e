#!/usr/bin/env python3
"""Times of the warm-up training targets (detector_assign.atss_assign_batch) beside the reference's route, in the same run.

    python tools/bench_detector_atss.py [--reps 50] [--out FILE.json]

B = 32 images at 640 x 640 (A = 8400 anchor boxes in levels of 6400, 1600 and 400), nc = 80, 5 and 50 labels per image
(tests/detector_atss_cases: a predicted box about every anchor).  Medians over `reps` runs after warm-up, in us:
  (a) reference_route    the statements of ComputeLoss.preprocess (targets to the host, a Python loop over every label, back to
                         the device) and of ATSSAssigner.forward restated as torch calls on the device: the (B, M, A) float64
                         tensors, the int64 one-hot per level and the host decision `fg_mask.max() > 1` included.  Host clock,
                         device drained before and after.
  (b) atss_assign_batch  HIP events around the call: the padding launch, the memset and the four launches of the assigner, the
                         outputs and the scratch from torch's caching allocator (targets on the device, max_labels given).
  (c) copy               HIP events around a device-to-device copy of the four outputs: what writing them once costs.
  (d) kernels            the launches apart, from torch.profiler's device times (null where the profiler gives none).
Also torch.cuda.max_memory_allocated over one call of (a) beside the scratch plus outputs of (b), in MB.
The expectation is (b) < (a); the tool prints the figures and asserts nothing about them.  It does compare the two routes'
labels, boxes, scores and fg for equality (torch's topk and sums may settle ties and last bits otherwise: the count of
differing anchors is reported, not asserted)."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import detector_assign_cases as tal_cases  # noqa: E402
import detector_atss_cases as cases  # noqa: E402
from bench_detector_assign import event_us, host_us, reference_preprocess  # noqa: E402
from event_representation_study_amd import _lib, detector_assign as da  # noqa: E402

S, TOPK = 640, 9


def reference_atss(anchors, counts, gt, pd_bboxes, nc):
    """ATSSAssigner.forward as torch calls: every (B, M, A) tensor of the reference is made."""
    B, M, A = gt.shape[0], gt.shape[1], anchors.shape[0]
    gt_labels, gt_bboxes = gt[:, :, :1], gt[:, :, 1:]
    mask_gt = (gt_bboxes.sum(-1, keepdim=True) > 0).float()
    flat = gt_bboxes.reshape(-1, 4)
    area_g = (flat[:, 2] - flat[:, 0]) * (flat[:, 3] - flat[:, 1])
    area_a = (anchors[:, 2] - anchors[:, 0]) * (anchors[:, 3] - anchors[:, 1])
    wh = (torch.min(flat[:, None, 2:], anchors[None, :, 2:]) - torch.max(flat[:, None, :2], anchors[None, :, :2])).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    union = torch.max(area_g[:, None] + area_a[None, :] - inter, inter.new_tensor([1e-6]))
    overlaps = (inter / union).reshape(B, M, A)
    g_points = torch.stack([(flat[:, 0] + flat[:, 2]) / 2.0, (flat[:, 1] + flat[:, 3]) / 2.0], dim=1)
    a_points = torch.stack([(anchors[:, 0] + anchors[:, 2]) / 2.0, (anchors[:, 1] + anchors[:, 3]) / 2.0], dim=1)
    distances = (g_points[:, None, :] - a_points[None, :, :]).pow(2).sum(-1).sqrt().reshape(B, M, A)
    mask_k = mask_gt.repeat(1, 1, TOPK).bool()
    in_cand, cand_idx, start = [], [], 0
    for level, n in zip(torch.split(distances, counts, dim=-1), counts):
        _, idx = level.topk(TOPK, dim=-1, largest=False)
        cand_idx.append(idx + start)
        idx = torch.where(mask_k, idx, torch.zeros_like(idx))
        hot = F.one_hot(idx, n).sum(dim=-2)
        in_cand.append(torch.where(hot > 1, torch.zeros_like(hot), hot).to(distances.dtype))
        start += n
    in_cand, cand_idx = torch.cat(in_cand, dim=-1), torch.cat(cand_idx, dim=-1)
    cand_over = torch.where(in_cand > 0, overlaps, torch.zeros_like(overlaps))
    at = cand_idx.reshape(B * M, -1) + A * torch.arange(B * M, device=gt.device)[:, None]
    picked = cand_over.reshape(-1)[at].reshape(B, M, -1)
    thr = picked.mean(-1, keepdim=True) + picked.std(-1, keepdim=True)
    is_pos = torch.where(cand_over > thr.repeat(1, 1, A), in_cand, torch.zeros_like(in_cand))
    centres = a_points.unsqueeze(0).repeat(B * M, 1, 1)
    deltas = torch.cat([centres - flat[:, :2].unsqueeze(1).repeat(1, A, 1), flat[:, 2:].unsqueeze(1).repeat(1, A, 1) - centres], -1)
    in_gts = (deltas.reshape(B, M, A, 4).min(-1)[0] > 1e-9).to(gt.dtype)
    mask_pos = is_pos * in_gts * mask_gt
    fg = mask_pos.sum(-2)
    if fg.max() > 1:
        multi = (fg.unsqueeze(1) > 1).repeat(1, M, 1)
        is_max = F.one_hot(overlaps.argmax(1), M).permute(0, 2, 1).to(overlaps.dtype)
        mask_pos = torch.where(multi, is_max, mask_pos)
        fg = mask_pos.sum(-2)
    gt_idx = (mask_pos.argmax(-2) + torch.arange(B, device=gt.device)[:, None] * M).long()
    labels = gt_labels.flatten()[gt_idx.flatten()].reshape(B, A)
    labels = torch.where(fg > 0, labels, torch.full_like(labels, nc))
    boxes = gt_bboxes.reshape(-1, 4)[gt_idx.flatten()].reshape(B, A, 4)
    scores = F.one_hot(labels.long(), nc + 1).float()[:, :, :nc]
    g, p = gt_bboxes.unsqueeze(2), pd_bboxes.unsqueeze(1)
    ov = (torch.minimum(g[..., 2:], p[..., 2:]) - torch.maximum(g[..., :2], p[..., :2])).clip(0).prod(-1)
    a1, a2 = (g[..., 2:] - g[..., :2]).clip(0).prod(-1), (p[..., 2:] - p[..., :2]).clip(0).prod(-1)
    ious = (ov / (a1 + a2 - ov + 1e-9)) * mask_pos
    scores *= ious.max(dim=-2)[0].unsqueeze(-1)
    return labels.long(), boxes, scores, fg.bool()


def kernel_us(launch, reps):
    """Mean device time per launch of each of the route's kernels, by name; an error text where the profiler gives none."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                launch()
            torch.cuda.synchronize()
        out = {}
        for e in prof.key_averages():
            for name in ("k_det_targets_pad", "k_atss_prepare", "k_atss_select", "k_atss_resolve", "k_atss_scores"):
                if name in e.key:
                    total = getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0)
                    out[name] = round(float(total) / max(e.count, 1), 1)
        return out
    except Exception as exc:  # the figures of (d) are optional: say why they are missing
        return {"error": repr(exc)[:200]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_detector_atss needs the GPU: no time is taken without one")
    dev, B, nc = torch.device("cuda:0"), args.batch, 80
    anchors_h, counts = da.anchor_boxes(S)
    a = torch.from_numpy(anchors_h).to(dev)
    p = torch.from_numpy(cases.pred_boxes(7000, B, S)).to(dev)
    A = len(anchors_h)
    rows = []
    for n_lab in (5, 50):
        t = torch.from_numpy(tal_cases.targets(7100 + n_lab, [n_lab] * B, nc)).to(dev)
        scale = torch.tensor([S, S, S, S], dtype=torch.float32, device=dev)

        def ref():
            return reference_atss(a, counts, reference_preprocess(t, B, scale), p, nc)

        def ours():
            return da.atss_assign_batch(a, counts, p, t, (S, S), nc, max_labels=n_lab)

        r, o = ref(), ours()
        differing = int(((r[0] != o[0]) | (r[3] != o[3]) | (r[1] != o[1]).any(-1) | (r[2].double() != o[2]).any(-1)).sum())
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        ref()
        torch.cuda.synchronize()
        ref_mb = (torch.cuda.max_memory_allocated() - base) / 1e6
        out_bytes = sum(x.numel() * x.element_size() for x in o[:4])
        ours_mb = (int(_lib.load().evrep_atss_workspace_bytes(B, n_lab, A)) + out_bytes + B * n_lab * 40) / 1e6
        t_ref = host_us(ref, max(args.reps // 5, 5))
        t_ours = event_us(ours, args.reps)
        spare = [torch.empty_like(x) for x in o[:4]]
        t_copy = event_us(lambda: [d.copy_(x) for d, x in zip(spare, o[:4])], args.reps)
        row = {"B": B, "A": A, "nc": nc, "labels_per_image": n_lab, "reps": args.reps, "foreground": int(o[3].sum()),
               "reference_route_host_us": round(t_ref, 1), "atss_assign_batch_us": round(t_ours, 1), "copy_us": round(t_copy, 1),
               "reference_over_atss": round(t_ref / t_ours, 1), "kernels_us": kernel_us(ours, 10), "reference_peak_mb": round(ref_mb, 1),
               "atss_scratch_and_outputs_mb": round(ours_mb, 1), "anchors_differing_from_the_reference_route": differing}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
