#!/usr/bin/env python3
"""Golden vectors for the head's decode and tail under 16 bits (tests/golden/detector_head_amp.npz).

Run where the reference lies (the fixture travels, the reference does not), naming its root:

    python tests/golden/make_golden_detector_head_amp.py <root of the reference checkout>

The reference's own ``Detect`` is imported and dressed exactly as make_golden_detector_head.py does (its ``_reference``,
``_module`` and ``_Slice`` stand-ins are reused by import), and run on CPU tensors with the MODULE AND THE MAPS in float16 and
in bfloat16: the GOLDEN cases of tests/detector_head_cases.py, their maps clamped to the dtype's largest finite value and
rounded to it (tests/detector_head_amp_cases.py).

This module-in-16-bit run is NOT what CUDA autocast does: autocast keeps ``softmax`` in float32 and is therefore closer to
the project's tail, which widens a 16-bit map exactly and computes as for float32 maps.  Here softmax, the projection, the
sigmoid, the box arithmetic and the backward all round to 16 bits, which is the widest gap the tail has to be held to.

Recorded per case and dtype under ``<case>/<dtype>/``, every 16-bit array as its bits (uint16; numpy has no bfloat16):
  pred             the evaluation branch's output, FLOAT32: the side distances and class scores are formed in 16 bits, but the
                   reference's anchor points and strides are float32 tensors and promote the box arithmetic and the last cat
  scores, distri   the training branch's ``cls_score_list`` / ``reg_distri_list``
  gcls_l, greg_l   the gradients of ``(Wc * cls_score_list).sum() + (Wr * reg_distri_list).sum()`` per level, read at the outputs of
                   the ``*_preds`` stand-ins (Wc, Wr float32: the products are float32, the gradients arrive in the dtype)
MEASURED per dtype against the reference's FLOAT64 run on the same (widened) maps, stored under ``measured/<dtype>/``:
E_box = max |pred - pred64| / stride over the box columns in grid units, E_cls the same over the class columns, E_scores for
``cls_score_list`` against the class columns of pred64, E_gcls = max |gcls - gcls64|.  That distance is the reference's own
16-bit rounding; the tests allow four times these values.  distri and greg carry no arithmetic and must agree exactly.
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
import detector_head_amp_cases as amp  # noqa: E402
from make_golden_detector_head import _module, _reference  # noqa: E402

OUT = os.path.join(HERE, "detector_head_amp.npz")
KEYS = ("E_box", "E_cls", "E_scores", "E_gcls")


def _bits(t):
    return t.detach().contiguous().view(torch.int16).numpy().view(np.uint16).copy()


def _train(Detect, c, dtype):
    det = _module(Detect, c, dtype).train()
    cls = [m.to(dtype).clone().requires_grad_(True) for m in c["cls"]]
    reg = [m.to(dtype).clone().requires_grad_(True) for m in c["reg"]]
    _, scores, distri = det([torch.cat([a, r], 1) for a, r in zip(cls, reg)])
    wdt = torch.float64 if dtype == torch.float64 else torch.float32
    ((torch.from_numpy(c["Wc"]).to(wdt) * scores).sum() + (torch.from_numpy(c["Wr"]).to(wdt) * distri).sum()).backward()
    L = len(cls)
    return scores.detach(), distri.detach(), [det.cls_preds[l].out.grad for l in range(L)], [det.reg_preds[l].out.grad for l in range(L)]


def run_reference(Detect, c, dtype):
    out = {}
    preds = {}
    for dt in (dtype, torch.float64):
        det = _module(Detect, c, dt).eval()
        with torch.no_grad():
            preds[dt] = det([torch.cat([a, r], 1).to(dt) for a, r in zip(c["cls"], c["reg"])])
        # (the anchor points and strides are float32, so the 16-bit module's concatenated output is promoted to float32)
        assert preds[dt].dtype == (torch.float64 if dt == torch.float64 else torch.float32)
        assert tuple(preds[dt].shape) == (c["B"], c["N"], 5 + c["nc"])
    scores, distri, gcls, greg = _train(Detect, c, dtype)
    _, _, gcls64, _ = _train(Detect, c, torch.float64)
    assert scores.dtype == distri.dtype == gcls[0].dtype == greg[0].dtype == dtype
    out["pred"], out["scores"], out["distri"] = preds[dtype].numpy().copy(), _bits(scores), _bits(distri)
    for l in range(len(gcls)):
        out["gcls_%d" % l], out["greg_%d" % l] = _bits(gcls[l]), _bits(greg[l])
    _, _, s = cases.anchors(c["shapes"], c["strides"])
    p16, p64 = preds[dtype].double().numpy(), preds[torch.float64].numpy()
    assert np.isfinite(p16).all() and np.isfinite(p64).all(), c["name"]
    e = dict(E_box=float((np.abs(p16[..., :4] - p64[..., :4]) / s[None, :, None]).max()),
             E_cls=float(np.abs(p16[..., 5:] - p64[..., 5:]).max()),
             E_scores=float(np.abs(scores.double().numpy() - p64[..., 5:]).max()),
             E_gcls=max(float((a.double() - b).abs().max()) for a, b in zip(gcls, gcls64)))
    return out, e


def main(root):
    Detect = _reference(root)
    out = {}
    for dname, dtype in sorted(amp.DTYPES.items()):
        worst = dict.fromkeys(KEYS, 0.0)
        for name in cases.GOLDEN:
            got, e = run_reference(Detect, amp.build(name, dtype), dtype)
            for k, v in e.items():
                worst[k] = max(worst[k], v)
            for k, v in got.items():
                out["%s/%s/%s" % (name, dname, k)] = v
            print("%-9s %-10s " % (dname, name) + " ".join("%s %.3g" % kv for kv in e.items()))
        for k, v in worst.items():
            out["measured/%s/%s" % (dname, k)] = np.float64(v)
            print("measured/%s/%-10s %.6g" % (dname, k, v))
    np.savez_compressed(OUT, **out)
    print("->", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
