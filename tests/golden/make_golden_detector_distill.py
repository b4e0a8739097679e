#!/usr/bin/env python3
"""Golden vectors for the distillation losses (tests/golden/detector_distill.npz).

Run where the reference lies (the fixture travels, the reference does not), naming its root:

    python tests/golden/make_golden_detector_distill.py <root of the reference checkout>

The reference's own ``VarifocalLoss``, ``BboxLoss`` (``forward`` with ``IOUloss``, ``_df_loss`` and ``distill_loss_dfl`` behind it)
and ``ComputeLoss.bbox_decode`` / ``distill_loss_cls`` / ``distill_loss_cw`` (``ev-YOLOv6/yolov6/models/losses/loss_distill.py``;
the three methods are called on a stand-in for ``self`` that holds ``use_dfl``, ``reg_max`` and ``proj`` -- the constructor moves
its modules to a GPU) are IMPORTED from where they lie, never copied, and run on CPU tensors as ``ComputeLoss.__call__`` hands
them over: float32 predictions of student and teacher, float64 targets (float32 ones in ``f32_targets``), ``target_bboxes /=
stride_tensor``, the background label before ``F.one_hot``, the division of ``loss_cls`` where ``target_scores_sum > 0``, the
decay, the distillation weights, the weighted sum, ``backward()``.  What this image lacks is an empty in-process stand-in, as
in make_golden_detector_assign.py.

The cases are tests/detector_distill_cases.py's GOLDEN and CW_GOLDEN (not ``r8``: the reference views its rows as 17 bins; not
the cases whose result is exactly zero by rule: the reference's float32 need not be exactly zero there); the box cases are
checked with detector_loss_cases.check_decided first.

Recorded per case: a SHA-256 of the inputs (the builders are seeded; the inputs themselves would double the file), the
reference's five terms, ``loss`` and ``loss_items`` (float64 of its float32 / float64 scalars) and both gradients (float32); per
channel-wise case the loss and the three maps' gradients.  MEASURED and stored under ``measured/*``: the greatest deviation,
over all cases, of each recorded quantity from the float64 restatement tests/detector_distill_ref.py on the same inputs -- the
reference's own float32 rounding.  The losses relative to the sum of the absolute values of their terms (the KL sums cancel;
``distill_host`` / ``cw_host`` give those sums), the gradients absolutely.  The tests allow four times these values.
"""
import hashlib
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

import detector_distill_cases as cases  # noqa: E402
import detector_distill_ref as ref  # noqa: E402
import detector_loss_cases as lcases  # noqa: E402
from make_golden_detector_assign import _reference as _reference_assign  # noqa: E402  (the stand-ins and the import path)

OUT = os.path.join(HERE, "detector_distill.npz")
LOSSES = ("loss_cls", "loss_iou", "loss_dfl", "d_loss_cls", "d_loss_dfl")
ABS = ("cls_abs", "iou_abs", "dfl_abs", "dcls_abs", "ddfl_abs")
QUANTITIES = LOSSES + ("grad_scores", "grad_distri", "cw_loss", "cw_grad")


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


def _reference(root):
    _reference_assign(root)
    from yolov6.models.losses.loss_distill import BboxLoss, ComputeLoss, VarifocalLoss
    return ComputeLoss, VarifocalLoss, BboxLoss


def run_reference(mods, c):
    ComputeLoss, VarifocalLoss, BboxLoss = mods
    nc, R, use_dfl, T = c["nc"], c["R"], c["use_dfl"], c["T"]
    lw = dict(zip(("class", "iou", "dfl"), c["weights"]), cwd=10.0)
    dw = {"class": c["dw"][0], "dfl": c["dw"][1]}
    p = torch.from_numpy(c["p"]).requires_grad_(True)
    z = torch.from_numpy(c["z"]).requires_grad_(True)
    tp, tz = torch.from_numpy(c["tp"]), torch.from_numpy(c["tz"])
    anc, stride = torch.from_numpy(c["anc"]), torch.from_numpy(c["stride"]).reshape(-1, 1)
    labels, fg = torch.from_numpy(c["labels"]), torch.from_numpy(c["fg"])
    tb, ts = torch.from_numpy(c["tb"].copy()), torch.from_numpy(c["ts"].copy())
    aps = anc / stride
    me = types.SimpleNamespace(use_dfl=use_dfl, reg_max=R, proj=torch.linspace(0, R, R + 1))
    pred_bboxes = ComputeLoss.bbox_decode(me, aps, z)
    t_pred_bboxes = ComputeLoss.bbox_decode(me, aps, tz)
    tb /= stride
    labels = torch.where(fg > 0, labels, torch.full_like(labels, nc))
    one_hot = F.one_hot(labels.long(), nc + 1)[..., :-1]
    loss_cls = VarifocalLoss()(p, ts, one_hot)
    tss = ts.sum()
    if tss > 0:
        loss_cls /= tss
    loss_iou, loss_dfl, d_loss_dfl = BboxLoss(nc, R, use_dfl, "giou")(z, pred_bboxes, tz, t_pred_bboxes, T, aps, tb, ts, tss, fg)
    d_loss_cls = ComputeLoss.distill_loss_cls(me, p, tp, nc, T)
    raw_cls, raw_dfl = float(d_loss_cls.item()), float(d_loss_dfl.item())
    d_loss_cw = torch.tensor(0.0)
    dec = ref.decay(c["epoch"], c["max_epoch"])
    d_loss_dfl *= dec
    d_loss_cls *= dec
    d_loss_cw *= dec
    loss_cls_all = loss_cls + d_loss_cls * dw["class"]
    loss_dfl_all = loss_dfl + d_loss_dfl * dw["dfl"]
    loss = lw["class"] * loss_cls_all + lw["iou"] * loss_iou + lw["dfl"] * loss_dfl_all + lw["cwd"] * d_loss_cw
    items = torch.cat(((lw["iou"] * loss_iou).unsqueeze(0), (lw["dfl"] * loss_dfl_all).unsqueeze(0),
                       (lw["class"] * loss_cls_all).unsqueeze(0), (lw["cwd"] * d_loss_cw).unsqueeze(0))).detach()
    loss.backward()
    assert p.grad.dtype == torch.float32 and z.grad.dtype == torch.float32
    return dict(loss_cls=np.float64(loss_cls.item()), loss_iou=np.float64(loss_iou.item()), loss_dfl=np.float64(loss_dfl.item()),
                d_loss_cls=np.float64(raw_cls), d_loss_dfl=np.float64(raw_dfl), loss=np.float64(loss.item()),
                loss_items=items.double().numpy().copy(), grad_scores=p.grad.numpy().copy(), grad_distri=z.grad.numpy().copy())


def run_reference_cw(mods, c):
    ComputeLoss = mods[0]
    s = [torch.from_numpy(x).requires_grad_(True) for x in c["s"]]
    t = [torch.from_numpy(x) for x in c["t"]]
    if c["tau"] == 1.0:
        loss = ComputeLoss.distill_loss_cw(None, s, t)                 # as the call site calls it
    else:
        loss = ComputeLoss.distill_loss_cw(None, s, t, c["tau"])
    loss.backward()
    out = dict(loss=np.float64(loss.item()))
    for l in range(3):
        assert s[l].grad.dtype == torch.float32
        out["grad%d" % l] = s[l].grad.numpy().copy()
    assert len(s) < 4 or s[3].grad is None
    return out


def main(root):
    mods = _reference(root)
    out, worst = {}, dict.fromkeys(QUANTITIES, 0.0)
    for name in cases.GOLDEN:
        c = cases.CASES[name]()
        d = {}
        cases.host(c, d)
        lcases.check_decided(name, c, d)
        got, want = run_reference(mods, c), cases.restated(c)
        dev = {}
        for k, a in zip(LOSSES, ABS):
            dev[k] = 0.0 if got[k] == want[k] else abs(got[k] - want[k]) / float(d[a])
        dev["grad_scores"] = float(np.abs(got["grad_scores"].astype(np.float64) - want["grad_scores"].numpy()).max())
        dev["grad_distri"] = float(np.abs(got["grad_distri"].astype(np.float64) - want["grad_distri"].numpy()).max())
        for k, v in dev.items():
            assert np.isfinite(v), (name, k)
            worst[k] = max(worst[k], v)
        pre = name + "/"
        out[pre + "inputs_sha256"] = digest([c[k] for k in cases.KEYS])
        for k, v in got.items():
            out[pre + k] = v
        print("%-18s " % name + " ".join("%s %.6g" % (k, got[k]) for k in LOSSES) + " | " + " ".join("%s %.3g" % kv for kv in dev.items()))
    for name in cases.CW_GOLDEN:
        c = cases.CW_CASES[name]()
        d = {}
        cases.cw_host(c, d)
        got, want = run_reference_cw(mods, c), cases.cw_restated(c)
        dev = dict(cw_loss=0.0 if got["loss"] == want["loss"] else abs(got["loss"] - want["loss"]) / float(sum(d["abs"])),
                   cw_grad=max(float(np.abs(got["grad%d" % l].astype(np.float64) - want["grads"][l].numpy()).max()) for l in range(3)))
        for k, v in dev.items():
            assert np.isfinite(v), (name, k)
            worst[k] = max(worst[k], v)
        pre = "cw_" + name + "/"
        out[pre + "inputs_sha256"] = digest(c["s"] + c["t"])
        for k, v in got.items():
            out[pre + k] = v
        print("cw %-15s loss %.8g | " % (name, got["loss"]) + " ".join("%s %.3g" % kv for kv in dev.items()))
    for k, v in worst.items():
        out["measured/" + k] = np.float64(v)
        print("measured/%-14s %.6g" % (k, v))
    np.savez_compressed(OUT, **out)
    print("->", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
