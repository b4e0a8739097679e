#!/usr/bin/env python3
"""Golden vectors for the detection scoring (tests/golden/detector_eval.npz).

Run where the reference lies (the fixture travels, the reference does not), naming its root:

    python tests/golden/make_golden_detector_eval.py <root of the reference checkout>

The reference's own ``ev-YOLOv6/yolov6/utils/metrics.py`` (with ``general.py`` behind it), ``yolov6/utils/nms.py`` and
``yolov6/core/evaler.py`` are IMPORTED from where they lie (never copied), on CPU float32 tensors.  What this image lacks is
an empty in-process stand-in: ``wandb``, ``cv2``, ``torchvision``, ``pycocotools`` and the three yolov6 modules evaler.py
imports for its data loader and checkpoints (``data.data_load``, ``utils.checkpoint``, ``utils.torch_utils``); none of them
is reached by what runs here.

Recorded, for inputs WITHOUT label ties (asserted: no detection has two same-class labels of equal IoU at or above iouv[0],
nor two labels of equal IoU above 0.45 -- there the reference's unstable argsort decides):

* native cases: ``process_batch(detections, labels, iouv)`` for T = 10, 1 and 16 thresholds and
  ``ConfusionMatrix(nc).process_batch(detections, labels)``;
* an evaluation of two batches: the statements of evaler.py:209-258 with the reference's ``Evaler.scale_coords`` (an instance
  made without ``__init__``, ``scale_exact = False``), ``xywh2xyxy``, ``process_batch`` and ``ConfusionMatrix`` -- the native
  detections and label boxes, ``correct``, the matrix -- and evaler.py:260-283 with ``ap_per_class(plot=False)``: p, r, ap, f1,
  ap_class, the best-F1 index, mp, mr, map50, map, nt.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import detector_eval_cases as cases  # noqa: E402

OUT = os.path.join(HERE, "detector_eval.npz")
NC = 3


def _stand_in(name, **attrs):
    mod = types.ModuleType(name)
    mod.__dict__.update(attrs)
    sys.modules[name] = mod
    return mod


def _reference(root):
    sys.path.insert(0, os.path.join(root, "ev-YOLOv6"))
    _stand_in("wandb")
    _stand_in("cv2", setNumThreads=lambda n: None)
    tv = _stand_in("torchvision")
    tv.ops = _stand_in("torchvision.ops")
    _stand_in("pycocotools")
    _stand_in("pycocotools.coco", COCO=None)
    _stand_in("pycocotools.cocoeval", COCOeval=None)
    _stand_in("yolov6.data.data_load", create_dataloader=None)
    _stand_in("yolov6.utils.checkpoint", load_checkpoint=None)
    _stand_in("yolov6.utils.torch_utils", time_sync=None, get_model_info=None)
    metrics = importlib.import_module("yolov6.utils.metrics")
    nms = importlib.import_module("yolov6.utils.nms")
    evaler = importlib.import_module("yolov6.core.evaler")
    ev = evaler.Evaler.__new__(evaler.Evaler)
    ev.scale_exact = False
    return metrics, nms, ev


def native_cases():
    """name -> (detections (n, 6), labels (M, 5), nc)"""
    return {
        "native_small": cases.native(1, 39, 11) + (3,),
        "native_dups": cases.native(2, 30, 8, dup=10) + (3,),
        "native_many": cases.native(3, 120, 40, nc=5) + (5,),
        "native_one": cases.native(4, 1, 1, nc=1) + (1,),
        "native_grid": (cases.grid_detections(100, 30), cases.grid_labels(30), 3),
    }


IOUVS = {"T10": torch.linspace(0.5, 0.95, 10), "T1": torch.tensor([0.5]), "T16": torch.linspace(0.3, 0.975, 16)}


def eval_batches():
    return [cases.batch(11, [5, 0, 9, 3], [20, 7, 0, 33], nc=NC, max_det=40),
            cases.batch(12, [11, 2, 6], [36, 12, 25], nc=NC, max_det=40, dup=3)]


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    metrics, nms, ev = _reference(sys.argv[1])
    flat, names = {}, []
    for name, (det, lab, nc) in native_cases().items():
        assert not cases.label_ties(det, lab, 0.3), name
        names.append(name)
        flat[name + "/det"], flat[name + "/labels"], flat[name + "/nc"] = det, lab, np.array(nc)
        for key, iouv in IOUVS.items():
            flat[name + "/iouv_" + key] = iouv.numpy()
            correct = metrics.process_batch(torch.from_numpy(det.copy()), torch.from_numpy(lab.copy()), iouv)
            flat[name + "/correct_" + key] = correct.numpy().astype(np.uint8)
        cm = metrics.ConfusionMatrix(nc)
        cm.process_batch(torch.from_numpy(det.copy()), torch.from_numpy(lab.copy()))
        assert np.array_equal(cm.matrix, np.round(cm.matrix))
        flat[name + "/matrix"] = cm.matrix.astype(np.int64)
        print("%-14s det %s labels %s correct@.5 %d matrix sum %d" % (name, det.shape, lab.shape, flat[name + "/correct_T10"][:, 0].sum(), cm.matrix.sum()))
    flat["names"] = np.array(names)

    # evaler.py:209-258, statement for statement, on two batches
    iouv = IOUVS["T10"]
    niou = iouv.numel()
    cm = metrics.ConfusionMatrix(NC)
    stats, seen = [], 0
    H, W = cases.IMG
    for bi, (det, count, targets_np, shapes) in enumerate(eval_batches()):
        B, max_det = det.shape[0], det.shape[1]
        targets = torch.from_numpy(targets_np.copy())
        eval_outputs = [torch.from_numpy(det[b, :count[b]].copy()) for b in range(B)]
        predn_all = np.zeros_like(det)
        tbox_all = np.zeros((len(targets_np), 4), np.float32)
        correct_all = np.zeros((B, max_det, niou), np.uint8)
        for si, pred in enumerate(eval_outputs):
            sel = targets[:, 0] == si
            labels = targets[sel, 1:]
            nl = len(labels)
            tcls = labels[:, 0].tolist() if nl else []
            seen += 1
            if len(pred) == 0:
                if nl:
                    stats.append((torch.zeros(0, niou, dtype=torch.bool), torch.Tensor(), torch.Tensor(), tcls))
                continue
            predn = pred.clone()
            ev.scale_coords((H, W), predn[:, :4], shapes[si][0], shapes[si][1])
            correct = torch.zeros(pred.shape[0], niou, dtype=torch.bool)
            if nl:
                tbox = nms.xywh2xyxy(labels[:, 1:5])
                tbox[:, [0, 2]] *= W
                tbox[:, [1, 3]] *= H
                ev.scale_coords((H, W), tbox, shapes[si][0], shapes[si][1])
                labelsn = torch.cat((labels[:, 0:1], tbox), 1)
                assert not cases.label_ties(predn.numpy(), labelsn.numpy()), (bi, si)
                correct = metrics.process_batch(predn, labelsn, iouv)
                cm.process_batch(predn, labelsn)
                tbox_all[sel.numpy()] = tbox.numpy()
            stats.append((correct.cpu(), pred[:, 4].cpu(), pred[:, 5].cpu(), tcls))
            predn_all[si, :len(pred)] = predn.numpy()
            correct_all[si, :len(pred)] = correct.numpy()
        pre = "eval%d/" % bi
        flat[pre + "det"], flat[pre + "count"], flat[pre + "targets"] = det, count, targets_np
        flat[pre + "shapes"] = cases.shapes_to_array(shapes)
        # (tbox of an image without detections is not formed by the evaler: those rows are recorded as NaN = "not held")
        for si in range(B):
            if count[si] == 0:
                tbox_all[targets_np[:, 0] == si] = np.nan
        flat[pre + "detn"], flat[pre + "tbox"], flat[pre + "correct"] = predn_all, tbox_all, correct_all
        print("eval batch %d: counts %s correct@.5 %d" % (bi, count.tolist(), correct_all[:, :, 0].sum()))
    flat["eval/matrix"] = cm.matrix.astype(np.int64)
    flat["eval/img"] = np.array(cases.IMG)
    # evaler.py:260-283
    stats = [np.concatenate(x, 0) for x in zip(*stats)]
    assert len(stats) and stats[0].any()
    p, r, ap, f1, ap_class = metrics.ap_per_class(*stats, plot=False)
    best = len(f1.mean(0)) - f1.mean(0)[::-1].argmax() - 1
    ap50, ap_mean = ap[:, 0], ap.mean(1)
    flat["eval/p"], flat["eval/r"], flat["eval/ap"], flat["eval/f1"], flat["eval/ap_class"] = p, r, ap, f1, ap_class
    flat["eval/summary"] = np.array([p[:, best].mean(), r[:, best].mean(), ap50.mean(), ap_mean.mean()], np.float64)
    flat["eval/best_f1_index"] = np.array(best)
    flat["eval/nt"] = np.bincount(stats[3].astype(np.int64), minlength=NC)
    flat["eval/seen"] = np.array(seen)
    for k, v in zip(("tp", "conf", "pred_cls", "target_cls"), stats):
        flat["eval/stats_" + k] = v
    print("mp %.4f mr %.4f map50 %.4f map %.4f" % tuple(flat["eval/summary"]), "nt", flat["eval/nt"].tolist(), "seen", seen)
    np.savez_compressed(OUT, **flat)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
