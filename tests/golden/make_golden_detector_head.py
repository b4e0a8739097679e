#!/usr/bin/env python3
"""Golden vectors for the head's decode and tail (tests/golden/detector_head.npz).

Run where the reference lies (the fixture travels, the reference does not), naming its root:

    python tests/golden/make_golden_detector_head.py <root of the reference checkout>

The reference's own ``Detect`` (``ev-YOLOv6/yolov6/models/effidehead.py``), with ``generate_anchors`` and ``dist2bbox`` behind
it, is IMPORTED from where it lies, never copied, and run on CPU tensors in both branches.  What this image lacks is an empty
in-process stand-in, as in make_golden_detector_assign.py.  The ``head_layers`` are stand-ins of ours: identities for the stems
and convs, channel slices for the two ``*_preds``, so that the module's input per level is ``cat(cls_l, reg_l)`` along the
channels and its last "convolutions" hand the two maps on as they are.  ``initialize_biases`` cannot run on them (they have no
bias), so ``proj`` and ``proj_conv.weight`` are set here to ``linspace(0, reg_max, reg_max + 1)``, which is what its last two
statements do; ``stride`` is set to the case's strides (the constructor knows three or four levels only).

The cases are tests/detector_head_cases.py's GOLDEN.  Recorded per case:
  ref32   the evaluation branch's ``pred`` in float32
  ref64   the same with the module and its inputs in float64
  scores, distri   the training branch's ``cls_score_list`` / ``reg_distri_list`` (float32)
  gcls_l, greg_l   the input gradients of ``(Wc * cls_score_list).sum() + (Wr * reg_distri_list).sum()`` per level, read at the
                   outputs of the two ``*_preds`` stand-ins (``retain_grad``), i.e. at the maps the tail takes: the gradient of the
                   concatenated input is the sum of the two slices' gradients, which would turn a -0.0 into +0.0
MEASURED and stored under ``measured/*`` per output group: E_box = max |ref32 - ref64| / stride over the box columns of all
cases, in grid units; E_cls = max |ref32 - ref64| over the class columns; E_scores the same for ``cls_score_list`` against the
class columns of ref64.  The reference's own float32 rounding; the tests allow four times these values.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import detector_head_cases as cases  # noqa: E402
from make_golden_detector_assign import _reference as _reference_assign  # noqa: E402  (the stand-ins and the import path)

OUT = os.path.join(HERE, "detector_head.npz")


class _Slice(torch.nn.Module):
    def __init__(self, lo, hi):
        super().__init__()
        self.lo, self.hi = lo, hi

    def forward(self, x):
        self.out = x[:, self.lo:self.hi]
        if self.out.requires_grad:
            self.out.retain_grad()
        return self.out


def _reference(root):
    _reference_assign(root)
    from yolov6.models.effidehead import Detect
    return Detect


def _module(Detect, c, dtype):
    nc, K, L = c["nc"], c["K"], len(c["shapes"])
    layers = []
    for _ in range(L):
        layers += [torch.nn.Identity(), torch.nn.Identity(), torch.nn.Identity(), _Slice(0, nc), _Slice(nc, nc + 4 * K)]
    det = Detect(num_classes=nc, num_layers=L, head_layers=layers, use_dfl=c["use_dfl"], reg_max=c["R"])
    det.stride = torch.tensor([int(s) for s in c["strides"]])
    det.proj = torch.nn.Parameter(torch.linspace(0, c["R"], c["R"] + 1), requires_grad=False)
    det.proj_conv.weight = torch.nn.Parameter(det.proj.view([1, c["R"] + 1, 1, 1]).clone().detach(), requires_grad=False)
    return det.to(dtype)


def run_reference(Detect, c):
    out = {}
    for dtype, key in ((torch.float32, "ref32"), (torch.float64, "ref64")):
        det = _module(Detect, c, dtype).eval()
        x = [torch.cat([torch.from_numpy(a), torch.from_numpy(r)], 1).to(dtype) for a, r in zip(c["cls"], c["reg"])]
        with torch.no_grad():
            pred = det(x)
        assert pred.dtype == dtype and tuple(pred.shape) == (c["B"], c["N"], 5 + c["nc"])
        out[key] = pred.numpy().copy()
    det = _module(Detect, c, torch.float32).train()
    cls = [torch.from_numpy(a).clone().requires_grad_(True) for a in c["cls"]]
    reg = [torch.from_numpy(r).clone().requires_grad_(True) for r in c["reg"]]
    _, scores, distri = det([torch.cat([a, r], 1) for a, r in zip(cls, reg)])
    ((torch.from_numpy(c["Wc"]) * scores).sum() + (torch.from_numpy(c["Wr"]) * distri).sum()).backward()
    out["scores"], out["distri"] = scores.detach().numpy().copy(), distri.detach().numpy().copy()
    for l in range(len(cls)):
        out["gcls_%d" % l], out["greg_%d" % l] = det.cls_preds[l].out.grad.numpy().copy(), det.reg_preds[l].out.grad.numpy().copy()
        # (the leaves' own .grad is the SUM of the two slices' gradients, zeros + value: it turns the -0.0 that sigmoid_backward
        #  gives for p = 1 and a negative gradient into +0.0, which is the stand-ins' doing and not the head's)
        assert np.array_equal(out["gcls_%d" % l], cls[l].grad.numpy()) and np.array_equal(out["greg_%d" % l], reg[l].grad.numpy())
    return out


def main(root):
    Detect = _reference(root)
    out, worst = {}, dict(E_box=0.0, E_cls=0.0, E_scores=0.0)
    for name in cases.GOLDEN:
        c = cases.build(name)
        got = run_reference(Detect, c)
        _, _, s = cases.anchors(c["shapes"], c["strides"])
        r32, r64 = got["ref32"].astype(np.float64), got["ref64"]
        assert np.isfinite(r32).all() and np.isfinite(r64).all(), name
        e = dict(E_box=float((np.abs(r32[..., :4] - r64[..., :4]) / s[None, :, None]).max()),
                 E_cls=float(np.abs(r32[..., 5:] - r64[..., 5:]).max()),
                 E_scores=float(np.abs(got["scores"].astype(np.float64) - r64[..., 5:]).max()))
        for k, v in e.items():
            worst[k] = max(worst[k], v)
        for k, v in got.items():
            out[name + "/" + k] = v
        print("%-10s " % name + " ".join("%s %.3g" % kv for kv in e.items()))
    for k, v in worst.items():
        out["measured/" + k] = np.float64(v)
        print("measured/%-10s %.6g" % (k, v))
    np.savez_compressed(OUT, **out)
    print("->", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
