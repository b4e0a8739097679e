"""Seeded inputs for the assigner tests (test_detector_assign_cpu.py, test_gpu_detector_assign.py) and for
tests/golden/make_golden_detector_assign.py, which records the reference's outputs on GOLDEN's cases.

A head's output is stood in for by pd_scores uniform in (0.05, 1) and, per anchor, a predicted box around the anchor's centre
with random extent and jitter: an anchor inside a label's box then has a positive IoU with it, so its key is positive."""
import numpy as np

from event_representation_study_amd.detector_assign import anchor_points, _in_gt_host

F32 = np.float32


def head(seed, B, S, nc, strides=(8, 16, 32)):
    """(pd_scores (B, A, nc), pd_bboxes (B, A, 4) xyxy pixels, anc (A, 2)), float32."""
    rng = np.random.default_rng(seed)
    anc, _ = anchor_points(S, strides)
    A = len(anc)
    scores = rng.uniform(0.05, 1.0, (B, A, nc)).astype(F32)
    half = rng.uniform(0.04, 0.3, (B, A, 2)) * S
    c = anc[None] + rng.normal(0, 0.02 * S, (B, A, 2))
    boxes = np.concatenate([c - half, c + half], axis=2).astype(F32)
    return scores, boxes, anc


def label_rows(rng, b, n, nc, lo=0.05, hi=0.5):
    """n rows [b, cls, cx, cy, w, h], normalised, boxes of lo..hi of the frame lying inside it."""
    wh = rng.uniform(lo, hi, (n, 2))
    c = wh / 2 + rng.uniform(0, 1, (n, 2)) * (1 - wh)
    return np.concatenate([np.full((n, 1), b), rng.integers(0, nc, (n, 1)), c, wh], axis=1).astype(F32)


def targets(seed, counts, nc, lo=0.05, hi=0.5, shuffle=True):
    """(n_t, 6) float32 for images with counts[b] labels, the images' rows interleaved."""
    rng = np.random.default_rng(seed)
    rows = [label_rows(rng, b, n, nc, lo, hi) for b, n in enumerate(counts)]
    t = np.concatenate(rows, 0) if rows else np.zeros((0, 6), F32)
    return t[rng.permutation(len(t))] if shuffle else t


def xyxy_rows(b, cls_boxes, S):
    """Rows for pixel boxes [(cls, x1, y1, x2, y2), ...] of an S x S image (the division by S rounds: the padded box is close
    to, not exactly, the pixel box)."""
    out = []
    for cls, x1, y1, x2, y2 in cls_boxes:
        out.append([b, cls, (x1 + x2) / 2 / S, (y1 + y2) / 2 / S, (x2 - x1) / S, (y2 - y1) / S])
    return np.array(out, F32).reshape(-1, 6)


def box_with_centres(rng, anc, S, n, tries=20000):
    """A pixel box (x1, y1, x2, y2) with exactly n anchor centres strictly inside."""
    for _ in range(tries):
        w, h = rng.uniform(0.03, 0.7, 2) * S
        x1, y1 = rng.uniform(0, S - w), rng.uniform(0, S - h)
        box = np.array([[x1, y1, x1 + w, y1 + h]])
        if int(_in_gt_host(box, anc).sum()) == n:
            return (x1, y1, x1 + w, y1 + h)
    raise AssertionError("no box with %d centres" % n)


def nested_targets(S):
    """Three nested boxes about one centre and two that overlap them: anchors claimed by two and by three rows."""
    c = S / 2
    boxes = [(0, c - 0.45 * S, c - 0.45 * S, c + 0.45 * S, c + 0.45 * S), (1, c - 0.4 * S, c - 0.4 * S, c + 0.4 * S, c + 0.4 * S),
             (0, c - 0.35 * S, c - 0.35 * S, c + 0.35 * S, c + 0.35 * S), (1, 0.05 * S, 0.1 * S, 0.6 * S, 0.7 * S),
             (0, 0.3 * S, 0.25 * S, 0.95 * S, 0.9 * S)]
    return xyxy_rows(0, boxes, S)


def centre_count_targets(seed, S, counts=(0, 1, 12, 13, 14)):
    rng = np.random.default_rng(seed)
    anc, _ = anchor_points(S)
    return xyxy_rows(0, [(i % 2,) + box_with_centres(rng, anc, S, n) for i, n in enumerate(counts)], S)


# name -> (head seed, S, B, nc, targets): what the golden script records the reference on
def golden_cases():
    return {
        "s64_b1_nc1": (101, 64, 1, 1, targets(201, [3], 1)),
        "s64_b4_nc80": (102, 64, 4, 80, targets(202, [2, 0, 5, 1], 80)),
        "s128_b4_nc2": (103, 128, 4, 2, targets(203, [6, 0, 3, 9], 2)),
        "s128_b1_nc2": (104, 128, 1, 2, targets(204, [5], 2)),
        "s640_b1_nc2": (105, 640, 1, 2, targets(205, [8], 2)),
        "no_labels_m0": (106, 64, 2, 2, targets(206, [0, 0], 2)),
        "nested": (107, 64, 1, 2, nested_targets(64)),
        "centres_0_1_12_13_14": (108, 64, 1, 2, centre_count_targets(208, 64)),
        "m101": (109, 128, 2, 2, targets(209, [101, 3], 2)),
    }
