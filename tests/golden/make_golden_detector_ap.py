#!/usr/bin/env python3
"""Golden vectors for the average precision (tests/golden/detector_ap.npz).

Run where the reference lies (the fixture travels, the reference does not), naming its root:

    python tests/golden/make_golden_detector_ap.py <root of the reference checkout>

The reference's own ``ev-YOLOv6/yolov6/utils/metrics.py`` is IMPORTED from where it lies (never copied), with the empty
stand-ins of make_golden_detector_eval.py for what this stack lacks.  Recorded, per case of
``detector_ap_cases.golden_cases()``: the inputs (``tp``, ``conf``, ``pred_cls``, ``target_cls``, ``nc``) and the reference's
``ap_per_class(tp, conf, pred_cls, target_cls, plot=False)``: ``p``, ``r``, ``ap``, ``f1``, ``classes``.

Every case has pairwise distinct confidences within every class (asserted by the case builder): there the reference's
unstable ``argsort(-conf)`` leaves nothing open.  The file holds data only.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import detector_ap_cases as cases  # noqa: E402
from make_golden_detector_eval import _reference  # noqa: E402

OUT = os.path.join(HERE, "detector_ap.npz")


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    metrics = _reference(sys.argv[1])[0]
    flat, names = {}, []
    for name, (tp, conf, pcls, tcls, nc) in cases.golden_cases().items():
        p, r, ap, f1, classes = metrics.ap_per_class(tp.copy(), conf.copy(), pcls.copy(), tcls.copy(), plot=False)
        names.append(name)
        flat[name + "/tp"], flat[name + "/conf"], flat[name + "/pred_cls"] = tp, conf, pcls
        flat[name + "/target_cls"], flat[name + "/nc"] = tcls, np.array(nc)
        flat[name + "/p"], flat[name + "/r"], flat[name + "/ap"], flat[name + "/f1"] = p, r, ap, f1
        flat[name + "/classes"] = classes
        print("%-12s n %5d T %2d classes %s map50 %.4f" % (name, conf.size, tp.shape[1], classes.tolist(), ap[:, 0].mean() if len(ap) else 0.0))
    flat["names"] = np.array(names)
    np.savez_compressed(OUT, **flat)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) < 512 * 1024


if __name__ == "__main__":
    main()
