"""Seeded inputs for the ATSS assigner tests (test_detector_atss_cpu.py, test_gpu_detector_atss.py) and for
tests/golden/make_golden_detector_atss.py, which records the reference's outputs on GOLDEN's cases.

The anchor boxes are those of ``generate_anchors`` in training mode (squares of 5 strides about the anchor points, level after
level); a head's output is stood in for by a predicted box around every anchor's centre with random extent and jitter."""
import numpy as np

import detector_assign_cases as tal_cases
from event_representation_study_amd.detector_assign import anchor_boxes

F32 = np.float32
TOPK = 9


def hw(size):
    return (int(size), int(size)) if np.isscalar(size) else (int(size[0]), int(size[1]))


def pred_boxes(seed, B, size, strides=(8, 16, 32)):
    """(B, A, 4) float32 xyxy pixels."""
    rng = np.random.default_rng(seed)
    H, W = hw(size)
    anchors, _ = anchor_boxes((H, W), strides)
    centre = np.stack([(anchors[:, 0] + anchors[:, 2]) / 2, (anchors[:, 1] + anchors[:, 3]) / 2], axis=1)
    half = rng.uniform(0.04, 0.3, (B, len(anchors), 2)) * np.array([W, H])
    c = centre[None] + rng.normal(0, 0.02, (B, len(anchors), 2)) * np.array([W, H])
    return np.concatenate([c - half, c + half], axis=2).astype(F32)


def xyxy_rows(b, cls_boxes, size):
    """Rows [b, cls, cx, cy, w, h] for pixel boxes [(cls, x1, y1, x2, y2), ...] of an H x W image (the divisions round: the padded
    box is close to, not exactly, the pixel box -- exactly where the pixel values and the sizes are powers of two apart)."""
    H, W = hw(size)
    out = [[b, cls, (x1 + x2) / 2 / W, (y1 + y2) / 2 / H, (x2 - x1) / W, (y2 - y1) / H] for cls, x1, y1, x2, y2 in cls_boxes]
    return np.array(out, F32).reshape(-1, 6)


def nested_targets(size):
    """Three nested boxes about one point off every grid line and two that overlap them: anchors claimed by several rows."""
    H, W = hw(size)
    cx, cy = 0.4713 * W, 0.5291 * H
    boxes = [(0, cx - 0.45 * W, cy - 0.45 * H, cx + 0.45 * W, cy + 0.45 * H), (1, cx - 0.36 * W, cy - 0.38 * H, cx + 0.4 * W, cy + 0.37 * H),
             (0, cx - 0.3 * W, cy - 0.27 * H, cx + 0.28 * W, cy + 0.31 * H), (1, 0.05 * W, 0.1 * H, 0.6 * W, 0.7 * H),
             (0, 0.31 * W, 0.25 * H, 0.95 * W, 0.9 * H)]
    return xyxy_rows(0, boxes, size)


# name -> (seed of the predicted boxes or None for pd_bboxes=None, size, B, nc, targets): what the golden script records
def golden_cases():
    t = tal_cases.targets
    return {
        "s96_b2": (101, 96, 2, 3, t(201, [4, 2], 3)),
        "s128_b3_one_empty": (102, 128, 3, 80, t(202, [5, 0, 3], 80)),
        "s160_nc1_m12": (103, 160, 1, 1, t(203, [12], 1)),
        "s96_large20": (104, 96, 1, 2, t(204, [20], 2, lo=0.4, hi=0.9)),
        "s640_b1": (105, 640, 1, 2, t(205, [8], 2)),
        "no_labels_m0": (106, 96, 2, 2, t(206, [0, 0], 2)),
        "nested": (107, 128, 1, 2, nested_targets(128)),
        "no_pd": (None, 128, 2, 2, t(208, [6, 3], 2, lo=0.1, hi=0.6)),
        "rect_96x160": (109, (96, 160), 2, 2, t(209, [5, 7], 2, lo=0.1, hi=0.6)),
    }


def case_inputs(name):
    """(anchors (A, 4), level counts, pd_bboxes (B, A, 4) or None, targets, (H, W), B, nc) of a golden case."""
    seed, size, B, nc, targets = golden_cases()[name]
    anchors, counts = anchor_boxes(hw(size))
    return anchors, counts, (None if seed is None else pred_boxes(seed, B, size)), targets, hw(size), B, nc
