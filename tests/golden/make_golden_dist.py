#!/usr/bin/env python3
"""Golden generator for DiST: runs the REFERENCE's own reshape_then_acc_adj_sort
(n_imagenet/real_cnn_model/data/imagenet.py:873-999) on small event tensors and records inputs and images in
tests/golden/nimg_dist.npz.

    python tests/golden/make_golden_dist.py

The reference is imported through make_golden_nimagenet._import_imagenet() (its stand-ins for the absent packages), never copied.

Per case ``<name>``: <name>.events float64 (N, 4) rows [x, y, t_seconds, p] -- the tensor the accumulator sees, i.e. AFTER the
augmentation for ``flip_11`` --, <name>.H, <name>.W, <name>.dist float32 (2, H, W); ``manifest`` is the JSON list of names.
``flip_11`` goes through the reference's base_augment("train") with a seed whose draws flip time and x (found as
make_golden_nimg_front.py finds them); <name>.draw = [time_flip, x_flip, x_shift, y_shift].  The augmented tensor is recorded by
running the reference's augmentation a second time from the same seed; the image is checked to be the same from both.

``nb_rounding``: the reference forms the 5x5 neighbour count as 25 * avg_pool2d(count), i.e. 25 * (s / 25) in float32, which is
not s for some s.  Seeds of a small dense frame are searched (at most NB_SEEDS of them) for a stream whose IMAGE changes when s is
used instead, judged with the numpy restatement of tests/test_dist_cpu.py; the first one found is kept.  (With the seeds below one
is found; if none were, the case would be missing and test_goldens_hold_the_cases_they_are_there_for skips that check.)
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden_nimagenet as mgn  # noqa: E402

NB_SEEDS = 200


def stream(n, W, H, seed, pol=(-1, 1), n_times=None, span=40_000):
    """(n, 4) float64 rows on the W x H frame, time-sorted microsecond stamps / 1e6 (n_times: that many distinct stamps)."""
    rng = np.random.default_rng(seed)
    ev = np.zeros((n, 4))
    ev[:, 0], ev[:, 1] = rng.integers(0, W, n), rng.integers(0, H, n)
    t = np.sort(rng.integers(0, span, n)) if n_times is None else np.sort(rng.choice(np.arange(n_times) * (span // n_times), n))
    t[0], t[-1] = 0, span
    ev[:, 2] = (t + 3_000_000) / 1e6
    ev[:, 3] = rng.choice(pol, n)
    return ev


def hot_pixel(W, H, seed):
    """Positive counts {0, 1, 2, 7, 5000}: one pixel with 5 000 events, three with 7, five with 2, twenty with 1."""
    rng = np.random.default_rng(seed)
    pix = rng.permutation(W * H)[:29]
    reps = [5000] + [7] * 3 + [2] * 5 + [1] * 20
    where = np.repeat(pix, reps)
    neg = rng.integers(0, W * H, 300)
    where = np.concatenate([where, neg])
    p = np.concatenate([np.ones(len(where) - 300), -np.ones(300)])
    order = rng.permutation(len(where))
    ev = np.zeros((len(where), 4))
    ev[:, 0], ev[:, 1], ev[:, 3] = where[order] % W, where[order] // W, p[order]
    t = np.sort(rng.integers(0, 40_000, len(where)))
    t[0], t[-1] = 0, 40_000
    ev[:, 2] = (t + 3_000_000) / 1e6
    return ev


def main():
    import test_dist_cpu as oracle
    torch.set_num_threads(1)
    ref = mgn._import_imagenet()

    def run(ev, H, W, augment=None):
        return ref.reshape_then_acc_adj_sort(torch.from_numpy(ev.copy()), augment=augment, height=H, width=W).numpy()

    cases = [("tiny_3x7", stream(30, 7, 3, 801), 3, 7),
             ("tiny_5x5", stream(40, 5, 5, 802), 5, 5),
             ("dense_24x32", stream(3000, 32, 24, 803), 24, 32),
             ("c224", stream(10_000, 224, 224, 804), 224, 224),
             ("hot_pixel", hot_pixel(12, 10, 805), 10, 12),
             ("single_pol", stream(600, 20, 16, 806, pol=(1,)), 16, 20),
             ("ties", stream(2500, 32, 24, 807, n_times=20), 24, 32)]
    # a stream whose image depends on nb = 25 * (s / 25) rather than s
    for seed in range(900, 900 + NB_SEEDS):
        ev = stream(1500, 32, 24, seed, n_times=400)
        prim = oracle.prim_from_events(ev, 24, 32)[None]
        if not np.array_equal(oracle.dist_from_prim(prim), oracle.dist_from_prim(prim, nb_exact=True)):
            cases.append(("nb_rounding", ev, 24, 32))
            print("nb_rounding: seed", seed)
            break
    else:
        print("nb_rounding: no seed in %d changes the image" % NB_SEEDS)

    g, names = {}, []
    for name, ev, H, W in cases:
        g[name + ".events"], g[name + ".H"], g[name + ".W"], g[name + ".dist"] = ev, H, W, run(ev, H, W)
        names.append(name)

    # time flip + x flip through the reference's base_augment
    seed = next(s for s in range(64) if (np.random.seed(s), np.random.random() < 0.5, np.random.random() < 0.5)[1:] == (True, True))
    ev = stream(2000, 224, 224, 808)
    np.random.seed(seed)
    image = run(ev, 224, 224, augment=ref.base_augment("train"))
    np.random.seed(seed)
    augmented = ref.base_augment("train")(torch.from_numpy(ev.copy())).numpy().copy()
    np.random.seed(seed)
    draw = [int(np.random.random() < 0.5), int(np.random.random() < 0.5)] + [int(v) for v in np.random.randint(-20, 21, size=(2,))]
    assert draw[:2] == [1, 1] and np.array_equal(run(augmented, 224, 224), image)
    g["flip_11.events"], g["flip_11.H"], g["flip_11.W"], g["flip_11.dist"] = augmented, 224, 224, image
    g["flip_11.draw"] = np.asarray(draw, np.int64)
    names.append("flip_11")

    for name in names:
        assert g[name + ".dist"].dtype == np.float32 and not np.isnan(g[name + ".dist"]).any(), name
    g["manifest"] = np.array(json.dumps(names))
    out = os.path.join(HERE, "nimg_dist.npz")
    np.savez_compressed(out, **g)
    print("wrote %s: %d cases, %d bytes" % (out, len(names), os.path.getsize(out)))


if __name__ == "__main__":
    main()
