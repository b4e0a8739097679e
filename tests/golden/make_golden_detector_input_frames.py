#!/usr/bin/env python3
"""Golden vectors for the detector's input batch from TORE's per-window frames (tests/golden/detector_input_frames.npz).

Run where the reference lies (the fixture travels, the reference does not):

    python tests/golden/make_golden_detector_input_frames.py

Modelled on make_golden_detector_input.py, whose stand-ins and helpers are imported: the reference's own
``yolov6.data.gen1_2yolo.Gen1H5`` and ``representations.tore.events2ToreFeature`` are IMPORTED (never copied), and
``Gen1H5.__getitem__`` runs on a bare instance whose transform is ``events2ToreFeature``, reached through the reference's own
``get_item_transform`` (its TORE branch crops the frame to the events' bounding box, representations/gen1_transforms.py:51-67).
The events are drawn inside a sub-rectangle of the sensor, with one event on each of two opposite corners, so the frame is a
bounding box of a chosen size, smaller than the sensor.  What the reference's own statements decide is thereby pinned: the
bounding-box frame, the order of the stages, the label arithmetic on the resized bounding-box frame, the draws from ``random``
and ``shapes``.

What sits behind the ``cv2`` stand-in of make_golden_detector_input.py (resize, copyMakeBorder, warpAffine, written there in
numpy from OpenCV's published algorithms) is NOT pinned against OpenCV: PARITY UNPINNED (cv2 absent).  One stand-in is
widened here: ``letterbox`` hands ``cv2.resize`` the whole 12-channel image when the bounding box needs a resize of its own
(data_augment.py:63), where that file's ``resize`` stops at 4 channels; here it goes channel by channel for any number of
them, with the same tables.  What OpenCV itself does with such an image is likewise not pinned.

Per case the file holds: the ``random.seed``, the events, the boxes _load_bbox returned, the representation, M (identity
without augment), s, the image, ``labels_out``, ``shapes`` and the flips.
"""
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_detector_input as base  # noqa: E402

OUT = os.path.join(HERE, "detector_input_frames.npz")
HYP = base.HYP
SENSOR = (100, 120)          # height, width
S = 48


def _resize_any_channels(cv2):
    """cv2.resize of the stand-in, channel by channel whatever their number."""
    narrow = cv2.resize

    def resize(im, dsize, interpolation=1):
        if im.ndim == 2 or im.shape[2] <= 4:
            return narrow(im, dsize, interpolation=interpolation)
        return np.stack([narrow(np.ascontiguousarray(im[..., c]), dsize, interpolation=interpolation) for c in range(im.shape[2])], -1)

    return resize


def _window(rng, n, box_h, box_w, y0, x0):
    """n events inside the box_h x box_w rectangle at (y0, x0); the first two sit on opposite corners."""
    x = rng.integers(0, box_w, n) + x0
    y = rng.integers(0, box_h, n) + y0
    x[0], y[0], x[1], y[1] = x0, y0, x0 + box_w - 1, y0 + box_h - 1
    t = np.sort(rng.integers(0, 100000, n)) + 1000
    p = rng.integers(0, 2, n) * 2 - 1
    return np.stack([x, y, t], -1).astype(np.int64), p.astype(np.int64)


def run_case(mods, tore, seed, augment, return_int, box_h, box_w, n_events=600, n_boxes=3):
    data_augment, gen1_2yolo, _ = mods
    Gen1H5 = gen1_2yolo.Gen1H5
    height, width = SENSOR
    rng = np.random.default_rng(5000 + seed)
    y0, x0 = int(rng.integers(0, height - box_h + 1)), int(rng.integers(0, width - box_w + 1))
    xyt, pol = _window(rng, n_events, box_h, box_w, y0, x0)
    raw_boxes = base._boxes(rng, n_boxes)
    ds = Gen1H5.__new__(Gen1H5)
    hyp = dict(HYP)
    if return_int is not None:
        hyp["letterbox_return_int"] = bool(return_int)
    ds.augment, ds.hyp, ds.rect, ds.img_size = augment, hyp, False, S
    ds.height, ds.width, ds.num_events, ds.time_window = height, width, n_events, 100000
    ds.transform, ds.vis_paths_to_indexes = tore, {}
    handle = {"bbox": None, "events": None}
    ds.convert_idx_to_rel_idx = lambda item: (0, handle, "synthetic")
    seen = {}

    def load_bbox(h, idx):
        bbox = Gen1H5._adjust_bbox(ds, raw_boxes, 0, 1)          # the reference's own clipping and centring
        bbox[:, 1:3] += 0.5 * bbox[:, 3:5]
        seen["boxes"] = bbox.copy()
        return bbox, 0

    ds._load_bbox = load_bbox
    ds._load_events = lambda h, event_idx: (xyt.copy(), pol.copy())
    # listeners on the reference's own functions: what they returned, not what they do
    real_gtm, real_git = data_augment.get_transform_matrix, gen1_2yolo.get_item_transform

    def gtm(*a, **k):
        M, s = real_gtm(*a, **k)
        seen["M"], seen["s"] = M.copy(), s
        return M, s

    def git(*a, **k):
        rep = real_git(*a, **k)
        seen["rep"] = np.array(rep, copy=True)
        return rep

    data_augment.get_transform_matrix, gen1_2yolo.get_item_transform = gtm, git
    try:
        random.seed(seed)
        img, labels_out, _, shapes = ds[0]
    finally:
        data_augment.get_transform_matrix, gen1_2yolo.get_item_transform = real_gtm, real_git
    assert seen["rep"].shape == (box_h, box_w, 12), seen["rep"].shape
    (h0, w0), ((rh, rw), pad) = shapes
    return {"seed": np.int64(seed), "augment": np.bool_(augment), "return_int": np.int64(-1 if return_int is None else int(return_int)),
            "img_size": np.int64(S), "sensor": np.array(SENSOR, dtype=np.int64),
            "events": np.concatenate([xyt, pol[:, None]], 1).astype(np.int32),
            "boxes": seen["boxes"], "rep": seen["rep"], "M": seen.get("M", np.eye(3)), "s": np.float64(seen.get("s", 1.0)),
            "image": img.numpy(), "labels_out": labels_out.numpy(),
            "shapes": np.array([h0, w0, rh, rw, pad[0], pad[1]], dtype=np.float64),
            "flips": np.array(base._flips_of(seed, hyp) if augment else [0, 0], dtype=np.int64)}


def main():
    mods = base._install()
    sys.modules["cv2"].resize = _resize_any_channels(sys.modules["cv2"])
    from representations.tore import events2ToreFeature
    want, seeds = {(0, 0), (0, 1), (1, 0), (1, 1)}, {}
    seed = 0
    while want:
        f = tuple(base._flips_of(seed, HYP))
        if f in want:
            want.discard(f)
            seeds[f] = seed
        seed += 1
    sd = [s for _, s in sorted(seeds.items())]
    cases = [
        run_case(mods, events2ToreFeature, sd[0], True, None, 31, 47),     # long side 47: letterbox resizes once more
        run_case(mods, events2ToreFeature, sd[1], True, False, 48, 20),    # long side 48: r == 1
        run_case(mods, events2ToreFeature, sd[2], True, True, 70, 96),     # larger than S
        run_case(mods, events2ToreFeature, sd[3], True, True, 5, 7),       # much smaller
        run_case(mods, events2ToreFeature, 101, False, True, 70, 96),      # validation: INTER_AREA
        run_case(mods, events2ToreFeature, 102, False, False, 20, 30),     # validation: smaller, no scale-up
        run_case(mods, events2ToreFeature, 103, False, None, 30, 48),      # validation: r == 1
    ]
    flat = {"n_cases": np.int64(len(cases)), "hyp": np.array([HYP[k] for k in ("degrees", "translate", "scale", "shear", "flipud", "fliplr")])}
    for i, c in enumerate(cases):
        for k, v in c.items():
            flat["c%d_%s" % (i, k)] = v
        print("case %d seed %d augment %d rep %s %s image %s labels %s flips %s shapes %s" % (
            i, c["seed"], c["augment"], c["rep"].shape, c["rep"].dtype, c["image"].shape, c["labels_out"].shape, c["flips"], c["shapes"]))
    np.savez_compressed(OUT, **flat)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
