#!/usr/bin/env python3
"""Golden vectors for the loss terms (tests/golden/detector_loss.npz).

Run where the reference lies (the fixture travels, the reference does not), naming its root:

    python tests/golden/make_golden_detector_loss.py <root of the reference checkout>

The reference's own ``VarifocalLoss``, ``BboxLoss`` (with ``IOUloss`` and ``_df_loss`` behind it) and ``ComputeLoss.bbox_decode``
(``ev-YOLOv6/yolov6/models/losses/loss.py``; bbox_decode is called on a stand-in for ``self`` that holds ``use_dfl``, ``reg_max``
and ``proj``) are IMPORTED from where they lie, never copied, and run on CPU tensors as ``ComputeLoss.__call__`` hands them
over: float32 predictions, float64 targets (float32 ones in the case ``f32_targets``), ``target_bboxes /= stride_tensor``, the
label of background anchors set to ``num_classes`` before ``F.one_hot``, the division by ``target_scores_sum`` when it exceeds 1,
the weighted sum, ``backward()``.  What this image lacks is an empty in-process stand-in, as in make_golden_detector_assign.py.

The cases are tests/detector_loss_cases.py's GOLDEN (all but ``bad_label``, on which the reference's one_hot raises); each is
checked with ``check_decided`` first: no tie of a min / max pair and no clamp argument of exactly 0.

Recorded per case: the inputs, the reference's three normalised terms (float64), both gradients (float32) and pred_bboxes
(float32).  MEASURED and stored under ``measured/*``: the greatest deviation, over all cases, of each recorded quantity from
the float64 restatement tests/detector_loss_ref.py on the same inputs -- the reference's own float32 rounding (its BCE, its
softmaxes and its boxes run in float32).  The losses relatively; the gradients and boxes absolutely, but the elements of
grad_scores whose p is exactly 0 or 1 relatively (they are about 1e11).  The tests allow four times these values.
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import detector_loss_cases as cases  # noqa: E402
from make_golden_detector_assign import _reference as _reference_assign  # noqa: E402  (the stand-ins and the import path)

OUT = os.path.join(HERE, "detector_loss.npz")
QUANTITIES = ("loss_cls", "loss_iou", "loss_dfl", "grad_scores", "grad_scores_saturated", "grad_distri", "pred_bboxes")


def _reference(root):
    _reference_assign(root)
    from yolov6.models.losses.loss import BboxLoss, ComputeLoss, VarifocalLoss
    return ComputeLoss, VarifocalLoss, BboxLoss


def run_reference(mods, c):
    ComputeLoss, VarifocalLoss, BboxLoss = mods
    nc, R, use_dfl = c["nc"], c["R"], c["use_dfl"]
    wc, wi, wd = c["weights"]
    p = torch.from_numpy(c["p"]).requires_grad_(True)
    z = torch.from_numpy(c["z"]).requires_grad_(True)
    anc, stride = torch.from_numpy(c["anc"]), torch.from_numpy(c["stride"]).reshape(-1, 1)
    labels, fg = torch.from_numpy(c["labels"]), torch.from_numpy(c["fg"])
    tb, ts = torch.from_numpy(c["tb"].copy()), torch.from_numpy(c["ts"].copy())
    aps = anc / stride
    me = types.SimpleNamespace(use_dfl=use_dfl, reg_max=R, proj=torch.linspace(0, R, R + 1))
    pred_bboxes = ComputeLoss.bbox_decode(me, aps, z)
    tb /= stride
    labels = torch.where(fg > 0, labels, torch.full_like(labels, nc))
    one_hot = F.one_hot(labels.long(), nc + 1)[..., :-1]
    loss_cls = VarifocalLoss()(p, ts, one_hot)
    tss = ts.sum()
    if tss > 1:
        loss_cls /= tss
    loss_iou, loss_dfl = BboxLoss(nc, R, use_dfl, "giou")(z, pred_bboxes, aps, tb, ts, tss, fg)
    loss = wc * loss_cls + wi * loss_iou + wd * loss_dfl
    loss.backward()
    assert p.grad.dtype == torch.float32 and z.grad.dtype == torch.float32 and pred_bboxes.dtype == torch.float32
    return dict(loss_cls=np.float64(loss_cls.item()), loss_iou=np.float64(loss_iou.item()), loss_dfl=np.float64(loss_dfl.item()),
                grad_scores=p.grad.numpy().copy(), grad_distri=z.grad.numpy().copy(), pred_bboxes=pred_bboxes.detach().numpy().copy())


def deviations(c, got, want):
    """got: the reference's results; want: the float64 restatement's.  One number per quantity."""
    out = {}
    for k in ("loss_cls", "loss_iou", "loss_dfl"):
        out[k] = 0.0 if got[k] == want[k] else abs(got[k] - want[k]) / abs(want[k])
    sat = (c["p"] == 0) | (c["p"] == 1)
    gs, ws = got["grad_scores"].astype(np.float64), want["grad_scores"].numpy()
    out["grad_scores"] = float(np.abs(gs - ws)[~sat].max())
    rel = np.abs(gs - ws)[sat] / np.maximum(np.abs(ws[sat]), 1e-300)
    out["grad_scores_saturated"] = float(np.where(ws[sat] == gs[sat], 0.0, rel).max()) if sat.any() else 0.0
    out["grad_distri"] = float(np.abs(got["grad_distri"].astype(np.float64) - want["grad_distri"].numpy()).max())
    out["pred_bboxes"] = float(np.abs(got["pred_bboxes"].astype(np.float64) - want["pred_bboxes"].numpy()).max())
    return out


def main(root):
    mods = _reference(root)
    out, worst = {}, dict.fromkeys(QUANTITIES, 0.0)
    for name in cases.GOLDEN:
        c = cases.CASES[name]()
        d = {}
        cases.host(c, d)
        cases.check_decided(name, c, d)
        got = run_reference(mods, c)
        dev = deviations(c, got, cases.restated(c))
        for k, v in dev.items():
            assert np.isfinite(v), (name, k)
            worst[k] = max(worst[k], v)
        pre = name + "/"
        for k in ("p", "z", "anc", "stride", "labels", "tb", "ts", "fg"):
            out[pre + k] = c[k]
        out[pre + "meta"] = np.array([c["nc"], c["R"], int(c["use_dfl"])], np.int64)
        out[pre + "weights"] = np.array(c["weights"], np.float64)
        for k, v in got.items():
            out[pre + k] = v
        print("%-20s cls %.6g iou %.6g dfl %.6g  " % (name, got["loss_cls"], got["loss_iou"], got["loss_dfl"])
              + " ".join("%s %.3g" % kv for kv in dev.items()))
    for k, v in worst.items():
        out["measured/" + k] = np.float64(v)
        print("measured/%-22s %.6g" % (k, v))
    np.savez_compressed(OUT, **out)
    print("->", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
