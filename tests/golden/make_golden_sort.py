#!/usr/bin/env python3
"""Golden generator for the sorted timestamp image: runs the REFERENCE's own reshape_then_acc_sort
(n_imagenet/real_cnn_model/data/imagenet.py:513-838) on small event tensors and records inputs and images in
tests/golden/nimg_sort.npz.

    python tests/golden/make_golden_sort.py

The reference is imported through make_golden_nimagenet._import_imagenet() (its stand-ins for the absent packages), never copied.
Every strict=True image is computed twice, with the scatter_max stand-in naming the first and the last of several tied events,
and must not depend on it.

``stream.<s>``: float64 (N, 4) rows [x, y, t_seconds, p], the tensor the accumulator sees (for ``flipped`` AFTER the reference's
random_time_flip, drawn from a seed that flips; ``flipped.draw`` = [1]).  ``<name>.image``: float32 (C, H, W).  ``manifest``: the
JSON list of cases {name, stream, H, W, kw}, kw the reference's keyword arguments without the denoise options (both False).
Frames are at most 16x24; the 224x224 frame is checked against the numpy restatement of tests/test_sort_cpu.py only.

Streams: ``base`` all sixteen switch combinations and the quantisations 4 and [2, 8, 255]; ``small`` a 5x7 frame; ``single_pol``
no negative event (the stand-in event of strict=True); ``ties`` 2 000 events on 12 stamps; ``flipped``; ``trunc`` stamps k / 1e6
whose product with 1e6 truncates to k - 1; ``index0`` several events at t = 0; ``epoch`` absolute times near 1.6e9 s; ``late`` a
window 20 s into a recording in which two pixels' latest indices differ by 1 us and agree in float32 (``late.pixels``).
"""
import itertools
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden_nimagenet as mgn  # noqa: E402

H, W = 16, 24


def stream(n, seed, stamps, w=W, h=H, pol=(-1, 1)):
    """(n, 4) float64 rows on the w x h frame; `stamps`: sorted int64 microsecond stamps, divided by 1e6 as load_event does."""
    rng = np.random.default_rng(seed)
    ev = np.zeros((n, 4))
    ev[:, 0], ev[:, 1] = rng.integers(0, w, n), rng.integers(0, h, n)
    ev[:, 2] = np.asarray(stamps, np.int64) / 1e6
    ev[:, 3] = rng.choice(pol, n)
    return ev


def stamps(n, seed, base, span=40_000, distinct=None):
    rng = np.random.default_rng(seed + 1000)
    t = np.sort(rng.integers(0, span, n)) if distinct is None else np.sort(rng.choice(np.arange(distinct) * (span // distinct), n))
    return t + base


def kw_name(kw):
    q = kw["quantize_sort"]
    qn = "" if q is None else "_q" + ("x".join(map(str, q)) if isinstance(q, list) else str(q))
    return "g%dn%du%ds%d%s" % (kw["global_time"], kw["neglect_polarity"], kw["use_image"], kw["strict"], qn)


def KW(g, n, u, s, q=None):
    return dict(global_time=bool(g), neglect_polarity=bool(n), use_image=bool(u), strict=bool(s), quantize_sort=q)


def main():
    torch.set_num_threads(1)
    ref = mgn._import_imagenet()

    def run(ev, h, w, kw):
        outs = []
        for pick in (("first", "last") if kw["strict"] else ("first",)):
            mgn.ARG_PICK = pick
            outs.append(ref.reshape_then_acc_sort(torch.from_numpy(ev.copy()), height=h, width=w, denoise_image=False,
                                                  denoise_sort=False, **kw).numpy())
        mgn.ARG_PICK = "first"
        assert all(np.array_equal(outs[0], o) for o in outs), "the image depends on which tied event scatter_max names"
        return outs[0]

    streams = {"base": (stream(700, 811, stamps(700, 811, 3_000_000)), H, W),
               "small": (stream(60, 812, stamps(60, 812, 3_000_000), w=7, h=5), 5, 7),
               "single_pol": (stream(300, 813, stamps(300, 813, 3_000_000), pol=(1,)), H, W),
               "ties": (stream(2000, 814, stamps(2000, 814, 3_000_000, distinct=12)), H, W),
               "epoch": (stream(500, 817, stamps(500, 817, 1_600_000_000_000_000)), H, W)}
    # the reference's time flip, from a seed whose draw flips
    seed = next(s for s in range(64) if (np.random.seed(s), np.random.random() < 0.5)[1])
    np.random.seed(seed)
    flipped = ref.random_time_flip(torch.from_numpy(stream(400, 815, stamps(400, 815, 3_000_000)))).numpy().copy()
    assert flipped[0, 2] == 0.0 and (np.diff(flipped[:, 2]) >= 0).all()
    streams["flipped"] = (flipped, H, W)
    # stamps k / 1e6 whose index is k - 1
    ks = np.array([k for k in range(1, 400_000) if int(np.float64(k) / 1e6 * 1e6) == k - 1][:300], np.int64)
    assert ks.size >= 100
    tr = np.sort(np.concatenate([ks, ks[::3] - 1, ks[::5] + 1]))
    streams["trunc"] = (stream(tr.size, 816, tr), H, W)
    i0 = stamps(200, 818, 0, span=3000)
    i0[:5] = 0
    streams["index0"] = (stream(200, 818, i0), H, W)
    # 20 s in: pixels a and b are last hit at indices one microsecond apart that agree in float32
    ev = stream(500, 819, stamps(500, 819, 20_000_000, span=30_000))
    idx = (ev[:, 2] * 1e6).astype(np.int64)
    la = next(int(v) for v in range(int(idx[-1]) + 10, int(idx[-1]) + 100) if np.float32(v) == np.float32(v + 1))
    a, b = 5 * W + 3, 11 * W + 17
    keep = ~np.isin(ev[:, 0] + ev[:, 1] * W, [a, b])
    tail = np.array([[a % W, a // W, la / 1e6, 1], [b % W, b // W, (la + 1) / 1e6, -1]])
    late = np.concatenate([ev[keep], tail])
    assert (late[-2:, 2] * 1e6).astype(np.int64).tolist() == [la, la + 1]
    streams["late"] = (late, H, W)

    combos16 = [KW(*c) for c in itertools.product((0, 1), repeat=4)]
    quant = [KW(1, 0, 1, 1, 4), KW(1, 0, 1, 1, [2, 8, 255]), KW(0, 1, 0, 1, [2, 8, 255]), KW(0, 0, 1, 0, 4), KW(0, 0, 1, 0, [2, 8, 255]),
             KW(1, 1, 0, 0, [2, 8, 255])]
    few = [KW(1, 0, 1, 1), KW(0, 1, 0, 1, [2, 8, 255]), KW(0, 0, 1, 0), KW(1, 1, 1, 0, 4)]
    plan = {"base": combos16 + quant, "small": few, "ties": few + [KW(0, 0, 0, 1, 4)], "flipped": few, "trunc": few, "index0": few,
            "epoch": few, "late": [KW(0, 1, 0, 1), KW(0, 0, 1, 1, [2, 8, 255]), KW(1, 1, 0, 1), KW(0, 1, 1, 0)],
            # strict=False raises for the polarity without events unless it is neglected
            "single_pol": [KW(1, 0, 1, 1), KW(0, 0, 0, 1, [2, 8, 255]), KW(0, 0, 1, 1, 4), KW(1, 1, 1, 0), KW(0, 1, 0, 1)]}

    g, cases = {}, []
    for sname, (ev, h, w) in streams.items():
        g["stream." + sname] = ev
        for kw in plan[sname]:
            name = "%s.%s" % (sname, kw_name(kw))
            img = run(ev, h, w, kw)
            assert img.dtype == np.float32 and not np.isnan(img).any(), name
            g[name + ".image"] = img
            cases.append(dict(name=name, stream=sname, H=h, W=w, kw=kw))
    g["flipped.draw"] = np.asarray([1], np.int64)
    g["late.pixels"] = np.asarray([a, b], np.int64)
    g["manifest"] = np.array(json.dumps(cases))
    out = os.path.join(HERE, "nimg_sort.npz")
    np.savez_compressed(out, **g)
    print("wrote %s: %d cases, %d bytes" % (out, len(cases), os.path.getsize(out)))


if __name__ == "__main__":
    main()
