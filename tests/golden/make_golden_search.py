#!/usr/bin/env python3
"""Golden vectors for one step of the representation search (tests/golden/search_step.npz).

Run where the reference lies (the fixture travels, the reference does not):

    python tests/golden/make_golden_search.py

The reference's ``MixedDensityEventStack``, ``Gen1H5.resize_image``, ``letterbox`` and ``otmi`` are IMPORTED (never copied)
with the stand-ins of make_golden.py and the ``cv2`` stand-in of make_golden_detector_input.py, and run as
``Gen1H5_Optimization.get_item_transform`` + ``measure_otmi`` chain them (representation_search/optimization.py:35-80,116-145):
the lists of the K chosen channels plus the candidate are padded with ``None`` to 12 entries, stacked ("SBN"), resized
keeping the ratio, letterboxed, and scored per window.  The sensor is 36 x 48 and ``img_size`` 48, so the resize is the
identity and ``letterbox`` only pads six rows of 114 above and below: of the cv2 stand-in only ``copyMakeBorder`` is reached.

``optimization.py`` itself cannot be imported here (it needs Gryffin and a dataset module), so the source of its
``known_constraints_cat`` is read from the file and executed in this process; the admissible table is what that function
returns over all 28 (function, aggregation) pairs.
"""
import ast
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
import make_golden_detector_input as mgdi  # noqa: E402

OUT = os.path.join(HERE, "search_step.npz")
HEIGHT, WIDTH, IMG_SIZE, N_CHANNELS = 36, 48, 48, 12
FUNCTIONS = ["timestamp", "polarity", "count", "timestamp_pos", "timestamp_neg", "count_pos", "count_neg"]
AGGREGATIONS = ["mean", "max", "sum", "variance"]
CHOSEN = [(0, "polarity", "variance"), (3, "timestamp_neg", "variance"), (2, "count_neg", "mean")]
CANDIDATES = [(0, "timestamp", "mean"), (1, "polarity", "sum"), (2, "count", "sum"), (3, "timestamp_pos", "max"),
              (4, "timestamp_neg", "variance"), (5, "count_pos", "mean"), (6, "count_neg", "sum"), (6, "timestamp", "variance")]
STACKS_OF = [1, 4]          # the candidates whose raw stacks are recorded


def _known_constraints_cat():
    path = os.path.join(mg.REF, "representations", "representation_search", "optimization.py")
    tree = ast.parse(open(path).read())
    node = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "known_constraints_cat")
    scope = {}
    exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), scope)
    return scope["known_constraints_cat"]


def _windows():
    """Two windows of about 2000 events, every quadrant populated, the densest quadrant different in the two."""
    out = []
    for seed, n, heavy in ((41, 2000, (0, 0)), (42, 2100, (1, 1))):
        rng = np.random.default_rng(seed)
        ev = mg.make_events(n, WIDTH, HEIGHT, seed=seed)
        k = n // 4                                             # a quarter of the events gathered in one quadrant
        idx = rng.choice(n, k, replace=False)
        ev[idx, 0] = rng.integers(0, WIDTH // 2, k) + heavy[0] * (WIDTH // 2)
        ev[idx, 1] = rng.integers(0, HEIGHT // 2, k) + heavy[1] * (HEIGHT // 2)
        out.append(ev)
    return out


def main():
    data_augment, gen1_2yolo, _ = mgdi._install()
    from representations.representation_search.mixed_density_event_stack import MixedDensityEventStack
    from representations.representation_search.compute_otmi import otmi
    ds = gen1_2yolo.Gen1H5.__new__(gen1_2yolo.Gen1H5)
    ds.img_size, ds.augment = IMG_SIZE, False
    kc = _known_constraints_cat()
    admissible = np.array([[bool(kc({"function": f, "aggregation": a})) for a in AGGREGATIONS] for f in FUNCTIONS])
    assert int(admissible.sum()) == 21
    wins = _windows()
    costs = np.zeros((len(CANDIDATES), len(wins)))
    stacks = {}
    for j, cand in enumerate(CANDIDATES):
        triples = CHOSEN + [cand]
        pad = [None] * (N_CHANNELS - len(triples))             # optimization.py:48-52
        lists = ([t[0] for t in triples] + pad, [t[1] for t in triples] + pad, [t[2] for t in triples] + pad)
        for b, ev in enumerate(wins):
            with np.errstate(all="ignore"):
                rep = MixedDensityEventStack(N_CHANNELS, ev.shape[0], HEIGHT, WIDTH, lists, "SBN").stack(mg.to_structured(ev))
            img, _, _ = ds.resize_image(rep)
            img, _, _ = data_augment.letterbox(img, IMG_SIZE, auto=False, scaleup=ds.augment)
            img = np.ascontiguousarray(img)
            assert img.shape == (IMG_SIZE, IMG_SIZE, N_CHANNELS) and (img[:6] == 114).all() and (img[-6:] == 114).all()
            assert np.array_equal(img[6:-6], rep)
            costs[j, b] = float(otmi(torch.from_numpy(ev), img, HEIGHT, WIDTH, IMG_SIZE))
            if j in STACKS_OF:
                stacks[(j, b)] = rep
    assert np.isfinite(costs).all()
    np.savez_compressed(
        OUT, height=HEIGHT, width=WIDTH, img_size=IMG_SIZE,
        **{"events_%d" % b: ev for b, ev in enumerate(wins)},
        chosen_windows=np.array([t[0] for t in CHOSEN]), chosen_functions=np.array([t[1] for t in CHOSEN]),
        chosen_aggregations=np.array([t[2] for t in CHOSEN]),
        cand_windows=np.array([t[0] for t in CANDIDATES]), cand_functions=np.array([t[1] for t in CANDIDATES]),
        cand_aggregations=np.array([t[2] for t in CANDIDATES]),
        stacks_of=np.array(STACKS_OF), stacks=np.stack([np.stack([stacks[(j, b)] for b in range(len(wins))]) for j in STACKS_OF]),
        costs=costs, functions=np.array(FUNCTIONS), aggregations=np.array(AGGREGATIONS), admissible=admissible)
    print("wrote", OUT, os.path.getsize(OUT), "bytes; costs", costs.mean(1))


if __name__ == "__main__":
    main()
