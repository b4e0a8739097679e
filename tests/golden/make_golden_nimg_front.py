#!/usr/bin/env python3
"""Golden generator for N-ImageNet's event front end: runs the REFERENCE's own load_event / parse_event / base_augment
(n_imagenet/real_cnn_model/data/imagenet.py:30-163,1140-1187) and three of its accumulators on small synthetic samples and
records inputs, drawn parameters and outputs in tests/golden/nimg_front.npz.

    python tests/golden/make_golden_nimg_front.py

The reference is imported through make_golden_nimagenet._import_imagenet() (its stand-ins for the absent packages).  One more
stand-in is made here, in process: ``np.float = float`` -- load_event calls np.float (:48), which numpy >= 1.24 no longer has.
Every sample is written to a temporary .npz in one of the two layouts load_event reads and parsed from there.

stream<k>.x, .y (uint16), .t (int64), .p (int8): the stored columns of sample k (several cases share one).
Per case ``<name>``:  <name>.out  float64 (N', 4), what
parse_event followed by base_augment(mode) returns;  <name>.draw  int64 [time_flip, x_flip, x_shift, y_shift, s0, s1], the
parameters the reference drew ([s0, s1) = the index range its slice took);  manifest (JSON): stream, seed, config, mode, layout and the
digests of both generators' states after the call.  The drawn parameters are captured by restoring the generator states saved
in front of the reference's call and drawing again in the order the reference does; the states after both runs must agree.
"""
import hashlib
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

N = 800
SENSOR_W, SENSOR_H = 640, 480
IMAGE_CASES = ("flip_00", "flip_11", "eval")


def state_digests():
    a = np.random.get_state()
    h_np = hashlib.sha1(np.asarray(a[1], np.uint32).tobytes() + repr(tuple(a[2:])).encode()).hexdigest()
    h_py = hashlib.sha1(repr(random.getstate()).encode()).hexdigest()
    return h_np, h_py


def stream(seed, pol, t0=3_000_000_000, dup=False, n=N):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, SENSOR_W, n).astype(np.uint16)
    y = rng.integers(0, SENSOR_H, n).astype(np.uint16)
    t = (np.sort(rng.integers(0, 50_000, n)) + t0).astype(np.int64)       # 50 ms: repeated microseconds occur
    if dup:
        t[:3], t[-4:] = t[0], t[-1]
    p = {"01": rng.integers(0, 2, n), "pm1": rng.choice([-1, 1], n), "ones": np.ones(n), "zeros": np.zeros(n)}[pol].astype(np.int8)
    return x, y, t, p


def write_sample(path, cols, layout):
    x, y, t, p = cols
    if layout == "compressed":
        rec = np.zeros(len(x), dtype=[("x", "<u2"), ("y", "<u2"), ("t", "<i8"), ("p", "i1")])
        rec["x"], rec["y"], rec["t"], rec["p"] = x, y, t, p
        np.savez(path, event_data=rec)
    else:
        np.savez(path, x_pos=x, y_pos=y, timestamp=t, polarity=p)


def replay_draws(n_rows, cfg, mode):
    """The reference's draws, again, in its order: slice_event's (Python random), then base_augment's (np.random)."""
    s0, s1 = 0, n_rows
    if cfg.get("slice_events") and cfg.get("slice_method", "idx") == "random":
        length = cfg["slice_length"]
        if cfg.get("slice_augment") and cfg["mode"] == "train":
            w = cfg.get("slice_augment_width", 0)
            length = random.randint(length - w, length + w)
        if n_rows > length:
            s0 = random.choice(range(n_rows - length + 1))
            s1 = s0 + length
    elif cfg.get("slice_events") and cfg.get("slice_method", "idx") == "idx":
        s0, s1, _ = slice(cfg.get("slice_start"), cfg.get("slice_end")).indices(n_rows)
        s1 = max(s0, s1)
    tf = xf = xs = ys = 0
    if mode == "train":
        tf = int(np.random.random() < 0.5)
        xf = int(np.random.random() < 0.5)
        xs, ys = (int(v) for v in np.random.randint(-20, 21, size=(2,)))
    return [tf, xf, xs, ys, s0, s1]


def run_reference(ref, path, cfg, mode, seed):
    np.random.seed(seed)
    random.seed(seed)
    ns = types.SimpleNamespace(**cfg)
    event = ref.parse_event(path, ns)
    aug = ref.base_augment(mode)
    return event if aug is None else aug(event)


def main():
    np.float = float                       # the alias numpy removed; load_event (:48) needs it
    ref = mgn._import_imagenet()
    base = dict(reshape=True, reshape_method="no_sample", mode="train")
    cases = []                             # (name, columns, layout, cfg, mode, seed)
    cols01 = stream(11, "01")
    # the four (time flip, x flip) combinations: search the seeds
    found = {}
    for seed in range(64):
        np.random.seed(seed)
        key = (int(np.random.random() < 0.5), int(np.random.random() < 0.5))
        found.setdefault(key, seed)
    assert sorted(found) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    for (tf, xf), seed in sorted(found.items()):
        cases.append(("flip_%d%d" % (tf, xf), cols01, "compressed" if tf == xf else "columns", dict(base), "train", seed))
    cases.append(("eval", cols01, "compressed", dict(base, mode="val"), "eval", 5))
    cases.append(("no_reshape", tuple(np.minimum(c, 223) if i < 2 else c for i, c in enumerate(cols01)), "compressed",
                  dict(mode="train"), "train", 6))
    s1 = found[(1, 0)]
    cases.append(("pol_pm1", stream(12, "pm1"), "compressed", dict(base), "train", s1))
    cases.append(("pol_ones", stream(13, "ones"), "columns", dict(base), "train", 8))
    cases.append(("pol_zeros", stream(14, "zeros"), "compressed", dict(base), "train", s1))
    cases.append(("dup_times", stream(15, "01", dup=True), "compressed", dict(base), "train", found[(0, 0)]))
    cases.append(("dup_times_flip", cases[-1][1], "compressed", dict(base), "train", found[(1, 1)]))
    for k, (a, e) in enumerate([(None, -100), (-400, None), (50, 500), (-5000, 5000), (500, 50)]):
        cases.append(("idx_%d" % k, cols01, "compressed", dict(base, slice_events=True, slice_method="idx", slice_start=a, slice_end=e),
                      "train", 20 + k if k < 4 else found[(0, 0)]))
    cd = stream(16, "01", dup=True)
    lo, hi = float(cd[2][N // 5]) / 1e6, float(cd[2][2 * N // 3]) / 1e6            # bounds that occur as timestamps
    assert (cd[2] == cd[2][N // 5]).sum() >= 1 and cd[2][2] == cd[2][0]
    cases.append(("time_slice", cd, "compressed", dict(base, slice_events=True, slice_method="time", slice_start=lo, slice_end=hi), "train", s1))
    cases.append(("time_slice_ends", cd, "columns", dict(base, slice_events=True, slice_method="time", slice_start=float(cd[2][0]) / 1e6,
                                                         slice_end=float(cd[2][-1]) / 1e6), "train", found[(0, 1)]))
    rnd = dict(base, slice_events=True, slice_method="random")
    cases.append(("random_500", cols01, "compressed", dict(rnd, slice_length=500), "train", 31))
    cases.append(("random_aug", cols01, "compressed", dict(rnd, slice_length=500, slice_augment=True, slice_augment_width=100), "train", 32))
    cases.append(("random_aug_eval", cols01, "compressed", dict(rnd, slice_length=500, slice_augment=True, slice_augment_width=100, mode="val"), "eval", 33))
    cases.append(("random_short", cols01, "compressed", dict(rnd, slice_length=N), "train", 34))
    cases.append(("random_short_aug", cols01, "columns", dict(rnd, slice_length=N + 300, slice_augment=True, slice_augment_width=100), "train", 35))
    cases.append(("abs_1p6e15", stream(17, "01", t0=1_600_000_000_000_000), "compressed", dict(base), "train", s1))
    cases.append(("abs_1p6e15_time", cases[-1][1], "compressed",
                  dict(base, slice_events=True, slice_method="time", slice_start=1_600_000_000.01, slice_end=1_600_000_000.04), "train", 9))

    g, manifest, streams = {}, [], []
    tmp = tempfile.mkdtemp()
    for name, cols, layout, cfg, mode, seed in cases:
        cfg = dict(cfg, compressed=(layout == "compressed"))
        path = os.path.join(tmp, name + ".npz")
        write_sample(path, cols, layout)
        out = run_reference(ref, path, cfg, mode, seed)
        after = state_digests()
        np.random.seed(seed)
        random.seed(seed)
        draw = replay_draws(len(cols[0]), cfg, mode)
        assert state_digests() == after, name + ": the replayed draws leave another generator state than the reference"
        sid = [i for i, c in enumerate(streams) if c is cols] or [len(streams)]
        if sid[0] == len(streams):
            streams.append(cols)
            for k, c in zip("xytp", cols):
                g["stream%d.%s" % (sid[0], k)] = c
        g[name + ".out"] = out.numpy().copy()
        g[name + ".draw"] = np.asarray(draw, np.int64)
        manifest.append(dict(name=name, stream=sid[0], seed=seed, cfg=cfg, mode=mode, layout=layout, np_state=after[0], py_state=after[1]))
        if name in IMAGE_CASES:
            for acc in ("acc_all", "acc_exp", "acc_intensity"):
                np.random.seed(seed)
                random.seed(seed)
                event = ref.parse_event(path, types.SimpleNamespace(**cfg))
                g["%s.%s" % (name, acc)] = getattr(ref, "reshape_then_" + acc)(event, augment=ref.base_augment(mode)).numpy()
    flips = {(int(g[c[0] + ".draw"][0]), int(g[c[0] + ".draw"][1])) for c in cases if c[4] == "train"}
    assert flips == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert len(g["random_short.out"]) > 0 and g["random_short.draw"][4:].tolist() == [0, N]
    assert len(g["idx_4.out"]) == 0
    g["manifest"] = np.array(json.dumps(manifest))
    out_path = os.path.join(HERE, "nimg_front.npz")
    np.savez_compressed(out_path, **g)
    print("wrote %s: %d cases, %d bytes" % (out_path, len(cases), os.path.getsize(out_path)))
    for m in manifest:
        print(m["name"], m["seed"], g[m["name"] + ".draw"].tolist(), g[m["name"] + ".out"].shape)


if __name__ == "__main__":
    main()
