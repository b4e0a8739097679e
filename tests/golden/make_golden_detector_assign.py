#!/usr/bin/env python3
"""Golden vectors for the training targets (tests/golden/detector_assign.npz).

Run where the reference lies (the fixture travels, the reference does not), naming its root:

    python tests/golden/make_golden_detector_assign.py <root of the reference checkout>

The reference's own ``ComputeLoss.preprocess`` (``ev-YOLOv6/yolov6/models/losses/loss.py``, called unbound: it never uses
``self``) and ``TaskAlignedAssigner.forward`` (``yolov6/assigners/tal_assigner.py``) are IMPORTED from where they lie (never
copied) and run on CPU tensors as ``ComputeLoss.__call__`` runs them: float32 predictions, the float64 tensor preprocess
returns, ``mask_gt = (gt_bboxes.sum(-1, keepdim=True) > 0).float()``.  What this image lacks is an empty in-process stand-in
(``cv2``, ``torchvision``, ``wandb``, ``yaml``, ``pkg_resources``); none of them is reached by what runs here.

Every recorded case is one the reference decides without help -- ``torch.topk`` leaves ties open and ``argmax`` the order among
equal IoUs.  Checked with ``tal_image_host`` before saving; a case that fails is refused (AssertionError), not left out:

* at every valid row the keys at places topk and topk + 1 of the order differ by more than 1e-9 relative;
* a row with fewer than topk positive keys has no in-box anchor of key 0;
* the two greatest IoUs of every multiply-claimed anchor differ.

Recorded per case: targets, pd_scores, pd_bboxes, anc, size, and the reference's gt (preprocess), labels (int64), boxes, scores
(float64), fg (bool).
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import detector_assign_cases as cases  # noqa: E402
from event_representation_study_amd import detector_assign as da  # noqa: E402

OUT = os.path.join(HERE, "detector_assign.npz")
TOPK = 13


def _stand_in(name, **attrs):
    mod = types.ModuleType(name)
    mod.__dict__.update(attrs)
    sys.modules.setdefault(name, mod)
    return sys.modules[name]


def _reference(root):
    sys.path.insert(0, os.path.join(root, "ev-YOLOv6"))
    for name in ("cv2", "wandb", "yaml", "pkg_resources"):
        try:
            __import__(name)
        except Exception:
            _stand_in(name, setNumThreads=lambda n: None)
    try:
        import torchvision  # noqa: F401
    except Exception:
        tv = _stand_in("torchvision")
        tv.ops = _stand_in("torchvision.ops")
    from yolov6.models.losses.loss import ComputeLoss
    from yolov6.assigners.tal_assigner import TaskAlignedAssigner
    return ComputeLoss, TaskAlignedAssigner


def decided_without_help(name, scores, boxes, anc, gt, nc):
    """The three conditions of the module docstring, on the host restatement's own keys and IoUs."""
    for b in range(gt.shape[0]):
        d = {}
        da.tal_image_host(scores[b], boxes[b], anc, gt[b], TOPK, nc, 1, 6, details=d)
        for m in np.flatnonzero(d["valid"]):
            k = np.sort(d["key"][m])[::-1]
            if len(k) > TOPK and k[TOPK - 1] > 0:
                assert k[TOPK - 1] - k[TOPK] > 1e-9 * k[TOPK - 1], (name, b, m, "keys at the cut")
            elif len(k) > TOPK:
                assert not (d["in_gt"][m] & (d["key"][m] == 0)).any(), (name, b, m, "an in-box anchor of key 0")
        for a in np.flatnonzero(d["count"] > 1):
            top = np.sort(d["iou"][:, a])[::-1]
            assert top[0] > top[1], (name, b, a, "equal greatest IoUs")


def main(root):
    ComputeLoss, TaskAlignedAssigner = _reference(root)
    out, seen = {}, dict(multi2=0, multi3=0)
    for name, (seed, S, B, nc, targets) in cases.golden_cases().items():
        scores, boxes, anc = cases.head(seed, B, S, nc)
        scale = torch.tensor([S, S, S, S]).float()
        gt = ComputeLoss.preprocess(None, torch.from_numpy(targets.copy()), B, scale)
        assert gt.dtype == torch.float64 and gt.shape[0] == B
        gt_np = gt.numpy().copy()
        if gt_np.shape[1]:
            decided_without_help(name, scores, boxes, anc, gt_np, nc)
        gt_labels, gt_bboxes = gt[:, :, :1], gt[:, :, 1:]
        mask_gt = (gt_bboxes.sum(-1, keepdim=True) > 0).float()
        ref = TaskAlignedAssigner(topk=TOPK, num_classes=nc, alpha=1.0, beta=6.0)
        labels, tb, ts, fg = ref(torch.from_numpy(scores), torch.from_numpy(boxes), torch.from_numpy(anc), gt_labels, gt_bboxes, mask_gt)
        if gt_np.shape[1]:
            assert tb.dtype == torch.float64 and ts.dtype == torch.float64 and labels.dtype == torch.int64 and fg.dtype == torch.bool
            d = {}
            for b in range(B):
                da.tal_image_host(scores[b], boxes[b], anc, gt_np[b], TOPK, nc, 1, 6, details=d)
                seen["multi2"] += int((d["count"] == 2).sum())
                seen["multi3"] += int((d["count"] >= 3).sum())
        pre = name + "/"
        out[pre + "targets"], out[pre + "pd_scores"], out[pre + "pd_bboxes"], out[pre + "anc"] = targets, scores, boxes, anc
        out[pre + "size"] = np.array([S, B, nc], np.int64)
        out[pre + "gt"] = gt_np
        out[pre + "labels"] = labels.numpy().astype(np.int64)
        out[pre + "boxes"] = tb.numpy().astype(np.float64)
        out[pre + "scores"] = ts.numpy().astype(np.float64)
        out[pre + "fg"] = fg.numpy().astype(bool)
        print("%-24s M %3d  fg %5d" % (name, gt_np.shape[1], int(out[pre + "fg"].sum())))
    assert seen["multi2"] > 0 and seen["multi3"] > 0, seen
    np.savez_compressed(OUT, **out)
    print(seen, "->", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
