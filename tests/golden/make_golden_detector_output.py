#!/usr/bin/env python3
"""Golden vectors for the detector's output (tests/golden/detector_output.npz).

Run where the reference lies (the fixture travels, the reference does not):

    python tests/golden/make_golden_detector_output.py

The reference's own ``ev-YOLOv6/yolov6/utils/nms.py`` is IMPORTED from where it lies (never copied) and its
``non_max_suppression`` runs on CPU float32 tensors.  The module imports ``cv2`` and ``torchvision`` at its top, and this image
has neither, so both are in-process stand-ins: ``cv2`` with the one function the module calls when it is imported
(``setNumThreads``; ``non_max_suppression`` uses nothing of it), and ``torchvision.ops.nms`` = the package's restatement of
torchvision's CPU kernel (``detector_output.torchvision_nms_host``).

What the file therefore pins to the reference's own torch statements: the candidate test, the products, the corners, the rows
and their order (multi_label's nonzero, the single-label max), the ``classes`` filter, the class offset handed to nms and the
cut to ``max_det`` -- every input of the nms call and everything done with its result.  What sits behind the ``torchvision``
boundary, the stable sort and the greedy pass, is the restated kernel on both sides: PARITY UNPINNED (torchvision absent).
``max_nms`` is a local constant of the reference (30000) that no case here reaches.

Per case the file holds the prediction, the arguments and the reference's outputs padded to (B, max_det, 6) with their
counts.  It also holds the class-offset rounding pair found by search (detector_output_cases.offset_rounding_pair): two boxes
of class 1 whose decision at iou_thres 0.65 differs between the float32-offset boxes and the un-offset ones.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import detector_output_cases as cases  # noqa: E402
from event_representation_study_amd import detector_output as do  # noqa: E402

REF_NMS = "/root/reference/ev-YOLOv6/yolov6/utils/nms.py"
OUT = os.path.join(HERE, "detector_output.npz")


def _reference():
    cv2 = types.ModuleType("cv2")
    cv2.setNumThreads = lambda n: None
    tv = types.ModuleType("torchvision")
    tv.ops = types.ModuleType("torchvision.ops")

    def nms(boxes, scores, iou_threshold):
        return torch.from_numpy(do.torchvision_nms_host(boxes.numpy(), scores.numpy(), iou_threshold))

    tv.ops.nms = nms
    sys.modules["cv2"], sys.modules["torchvision"], sys.modules["torchvision.ops"] = cv2, tv, tv.ops
    spec = importlib.util.spec_from_file_location("reference_nms", REF_NMS)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def golden_cases():
    """name -> (pred, kwargs)"""
    a, b, _, _ = cases.offset_rounding_pair()
    return {
        "evaler_C3": (cases.head_output(1, 3, 300, 3), dict(conf_thres=0.03, iou_thres=0.65, multi_label=True)),
        "evaler_C80": (cases.head_output(2, 1, 150, 80, lo=-0.6), dict(conf_thres=0.03, iou_thres=0.65, multi_label=True)),
        "inferer_C2": (cases.head_output(3, 3, 300, 2), dict(conf_thres=0.25, iou_thres=0.45)),
        "agnostic_C1": (cases.head_output(4, 1, 200, 1), dict(conf_thres=0.25, iou_thres=0.45, agnostic=True, multi_label=True)),
        "classes1_det3": (cases.head_output(5, 3, 300, 3), dict(conf_thres=0.1, iou_thres=0.5, classes=[1], multi_label=True, max_det=3)),
        "classes02_single": (cases.head_output(6, 1, 300, 3), dict(conf_thres=0.1, iou_thres=0.5, classes=[0, 2], agnostic=True)),
        "candidate_edges_multi": (cases.edges_of_candidates(), dict(conf_thres=0.25, iou_thres=0.45, multi_label=True)),
        "candidate_edges_single": (cases.edges_of_candidates(), dict(conf_thres=0.25, iou_thres=0.45)),
        "float32_threshold": (cases.float32_threshold_rows(), dict(conf_thres=0.1, iou_thres=0.45)),
        "argmax_tie": (cases.argmax_tie(), dict(conf_thres=0.25, iou_thres=0.45)),
        "duplicates": (cases.duplicates(), dict(conf_thres=0.25, iou_thres=0.45, multi_label=True)),
        "two_classes_one_box": (cases.two_classes_one_box(), dict(conf_thres=0.25, iou_thres=0.45, multi_label=True)),
        "two_classes_one_box_agnostic": (cases.two_classes_one_box(), dict(conf_thres=0.25, iou_thres=0.45, multi_label=True, agnostic=True)),
        "offset_pair": (cases.pair(a, b, C=3, cls=1), dict(conf_thres=0.25, iou_thres=0.65)),
        "offset_pair_agnostic": (cases.pair(a, b, C=3, cls=1), dict(conf_thres=0.25, iou_thres=0.65, agnostic=True)),
    }


def main():
    ref = _reference()
    flat = {}
    names = []
    for name, (pred, kw) in golden_cases().items():
        with np.errstate(all="ignore"):
            out = ref.non_max_suppression(torch.from_numpy(pred.copy()), **kw)
        max_det = kw.get("max_det", 300)
        det, count = cases.pad([o.numpy() for o in out], max_det)
        names.append(name)
        flat[name + "/pred"] = pred
        flat[name + "/det"] = det
        flat[name + "/count"] = count
        flat[name + "/args"] = np.array([kw["conf_thres"], kw["iou_thres"], float(kw.get("agnostic", False)),
                                         float(kw.get("multi_label", False)), float(max_det)], np.float64)
        flat[name + "/classes"] = np.array(kw["classes"] if kw.get("classes") is not None else [-1], np.int64)
        print("%-30s pred %s count %s" % (name, pred.shape, count.tolist()))
    a, b, o1, o0 = cases.offset_rounding_pair()
    flat["offset_pair_boxes"] = np.array([a, b], np.float32)
    flat["offset_pair_ovr"] = np.array([o1, o0], np.float32)
    flat["names"] = np.array(names)
    np.savez_compressed(OUT, **flat)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
