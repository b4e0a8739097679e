#!/usr/bin/env python3
"""Golden generator for the study's representations on N-ImageNet batches: runs the REFERENCE's own parse_event and
base_augment (n_imagenet/real_cnn_model/data/imagenet.py:128-163,1140-1187) on small synthetic samples and then its own
reshape_then_optimized, reshape_then_event_stack and reshape_then_tore (:1025-1107) on every augmented tensor, and records
inputs, drawn parameters, augmented tensors and the three images in tests/golden/nimg_study.npz.

    python tests/golden/make_golden_nimg_study.py

The reference is imported as make_golden_nimg_front.py imports it (make_golden_nimagenet._import_imagenet() with its stand-ins
for the absent packages, np.float = float).  To keep the fixture small the frames are 24 x 32 on a 48 x 64 sensor: the
reference module's SENSOR_H / SENSOR_W / IMAGE_H / IMAGE_W are set in process before its parse_event runs, and the `resolution`
defaults of its random_flip_events_along_x / random_shift_events -- bound to (224, 224) when the module was loaded -- are set to
the same frame.  Its shift stays at up to 20 pixels, so most of a sample is cropped away; the seeds are chosen so that every
case keeps rows.

stream<k>.x, .y (uint16), .t (int64 microseconds), .p (int8): the stored columns of sample k.  Per case ``<name>``:
<name>.out float64 (N', 4), what parse_event followed by base_augment(mode) returns; <name>.draw int64 [time_flip, x_flip,
x_shift, y_shift, s0, s1]; <name>.optimized / .event_stack / .tore float32 (12, 24, 32), the reference's images of that tensor;
manifest (JSON): stream, seed, config, mode, layout, sensor and image size.  Data only.
"""
import json
import os
import random
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_nimagenet as mgn  # noqa: E402
import make_golden_nimg_front as mgf  # noqa: E402

N = 1500
SENSOR_H, SENSOR_W = 48, 64
IMAGE_H, IMAGE_W = 24, 32
NAMES = ("optimized", "event_stack", "tore")
MIN_ROWS = 150


def stream(seed, t0, span=50_000, n=N):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, SENSOR_W, n).astype(np.uint16)
    y = rng.integers(0, SENSOR_H, n).astype(np.uint16)
    t = (np.sort(rng.integers(0, span, n)) + t0).astype(np.int64)
    p = rng.integers(0, 2, n).astype(np.int8)
    return x, y, t, p


def draws_of(seed):
    np.random.seed(seed)
    tf, xf = int(np.random.random() < 0.5), int(np.random.random() < 0.5)
    xs, ys = (int(v) for v in np.random.randint(-20, 21, size=(2,)))
    return tf, xf, xs, ys


def main():
    np.float = float                       # the alias numpy removed; load_event (:48) needs it
    ref = mgn._import_imagenet()
    ref.SENSOR_H, ref.SENSOR_W, ref.IMAGE_H, ref.IMAGE_W = SENSOR_H, SENSOR_W, IMAGE_H, IMAGE_W
    assert ref.random_shift_events.__defaults__ == (20, (224, 224)) and ref.random_flip_events_along_x.__defaults__ == ((224, 224), 0.5)
    ref.random_shift_events.__defaults__ = (20, (IMAGE_H, IMAGE_W))
    ref.random_flip_events_along_x.__defaults__ = ((IMAGE_H, IMAGE_W), 0.5)
    # the four (time flip, x flip) combinations with shifts that leave rows on the 24 x 32 frame: search the seeds
    found = {}
    for seed in range(4096):
        tf, xf, xs, ys = draws_of(seed)
        if abs(xs) <= 6 and abs(ys) <= 5:
            found.setdefault((tf, xf), seed)
    assert sorted(found) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    base = dict(reshape=True, reshape_method="no_sample", mode="train")
    # whole seconds: 1.6e9 s + 0.98 .. 1.03 s straddles one, + 0.10 .. 0.15 s lies inside one
    straddle = stream(21, 1_600_000_000_980_000)
    inside = stream(22, 1_600_000_000_100_000)
    cases = []                             # (name, columns, layout, cfg, mode, seed)
    for (tf, xf), seed in sorted(found.items()):
        cases.append(("flip_%d%d" % (tf, xf), straddle, "compressed" if tf == xf else "columns", dict(base), "train", seed))
    cases.append(("inside_00", inside, "compressed", dict(base), "train", found[(0, 0)]))
    cases.append(("inside_11", inside, "columns", dict(base), "train", found[(1, 1)]))
    cases.append(("eval", straddle, "compressed", dict(base, mode="val"), "eval", 5))
    cases.append(("slice", straddle, "compressed", dict(base, slice_events=True, slice_method="idx", slice_start=200, slice_end=-300),
                  "train", found[(0, 1)]))

    g, manifest, streams = {}, [], []
    tmp = tempfile.mkdtemp()
    for name, cols, layout, cfg, mode, seed in cases:
        cfg = dict(cfg, compressed=(layout == "compressed"))
        path = os.path.join(tmp, name + ".npz")
        mgf.write_sample(path, cols, layout)
        out = mgf.run_reference(ref, path, cfg, mode, seed)
        after = mgf.state_digests()
        np.random.seed(seed)
        random.seed(seed)
        draw = mgf.replay_draws(len(cols[0]), cfg, mode)
        assert mgf.state_digests() == after, name + ": the replayed draws leave another generator state than the reference"
        assert len(out) >= MIN_ROWS, (name, len(out))
        sid = [i for i, c in enumerate(streams) if c is cols] or [len(streams)]
        if sid[0] == len(streams):
            streams.append(cols)
            for k, c in zip("xytp", cols):
                g["stream%d.%s" % (sid[0], k)] = c
        g[name + ".out"] = out.numpy().copy()
        g[name + ".draw"] = np.asarray(draw, np.int64)
        for rep in NAMES:
            img = getattr(ref, "reshape_then_" + rep)(torch.from_numpy(g[name + ".out"].copy()), height=IMAGE_H, width=IMAGE_W).numpy()
            assert img.dtype == np.float32 and img.shape == (12, IMAGE_H, IMAGE_W), (name, rep, img.dtype, img.shape)
            g["%s.%s" % (name, rep)] = np.ascontiguousarray(img)
        manifest.append(dict(name=name, stream=sid[0], seed=seed, cfg=cfg, mode=mode, layout=layout,
                             sensor=[SENSOR_H, SENSOR_W], image=[IMAGE_H, IMAGE_W]))
    sec = {m["name"]: np.unique(g[m["name"] + ".out"][:, 2].astype(np.int64)).size for m in manifest}
    assert sec["flip_00"] == 2 and sec["inside_00"] == 1 and sec["flip_11"] == 1, sec     # rebased whole seconds {0, 1} / {0}
    g["manifest"] = np.array(json.dumps(manifest))
    out_path = os.path.join(HERE, "nimg_study.npz")
    np.savez_compressed(out_path, **g)
    print("wrote %s: %d cases, %d bytes" % (out_path, len(cases), os.path.getsize(out_path)))
    for m in manifest:
        print(m["name"], m["seed"], g[m["name"] + ".draw"].tolist(), g[m["name"] + ".out"].shape, sec[m["name"]])


if __name__ == "__main__":
    main()
