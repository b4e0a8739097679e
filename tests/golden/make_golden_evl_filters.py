"""Record tests/golden/evl_filters.npz: inputs, parameters, keep masks, outgoing state arrays and (for the resize) output
events of the ev-licious event filters, computed by the REFERENCE's own code.

    python tests/golden/make_golden_evl_filters.py /path/to/event_representation_study

The reference's modules ev-licious/src/evlicious/tools/utils.py, tools/filters.py and io/utils/events.py are imported from the
given checkout with `numba.jit` stood in by the identity (numba is absent here: the loops run as plain Python -- compiled numba
is NOT pinned), `matplotlib` and the `render` module of `Events` stubbed, and the real `Events` class in place.
One deviation, forced by the stand-in: `_background_activity_filter` gets `x`, `y` widened to int64.  numba types
`x_ - radius` as int64; plain numpy 2 wraps the uint16 instead (different masks, overflow warnings), so the recorded
BackgroundActivity results are those of the loop with int64 coordinates, which is what the compiled function computes.
Only data is written; no program text of the reference.
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)


RECORDED = []      # the keep masks the reference's loops returned during one insert


def load_reference(ref_root):
    src = os.path.join(ref_root, "ev-licious", "src", "evlicious")

    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    def jit(*a, **k):
        if len(a) == 1 and callable(a[0]) and not k:
            return a[0]
        return lambda f: f

    stub("numba", jit=jit)
    stub("matplotlib")
    stub("matplotlib.pyplot", hot=None)

    def load(name, path, package=None):
        spec = importlib.util.spec_from_file_location(name, path)
        m = importlib.util.module_from_spec(spec)
        if package:
            m.__package__ = package
        sys.modules[name] = m
        spec.loader.exec_module(m)
        return m

    pkg = stub("evlicious")
    pkg.__path__ = []
    for sub in ("evlicious.io", "evlicious.io.utils", "evlicious.tools"):
        stub(sub).__path__ = []
    stub("evlicious.io.utils.render", _render=None, RenderingType=types.SimpleNamespace(RED_BLUE_OVERLAP=0))
    events_mod = load("evlicious.io.utils.events", os.path.join(src, "io", "utils", "events.py"), "evlicious.io.utils")
    pkg.Events = events_mod.Events
    utils = load("evlicious.tools.utils", os.path.join(src, "tools", "utils.py"), "evlicious.tools")
    # the stand-in for numba's typing: int64 coordinates into the BackgroundActivity loop (module docstring)
    raw = utils._background_activity_filter
    utils._background_activity_filter = lambda mask, ts, x, y, t, depth_us, radius=1: raw(
        mask, ts, x.astype(np.int64), y.astype(np.int64), t, depth_us, radius)
    filters = load("evlicious.tools.filters", os.path.join(src, "tools", "filters.py"), "evlicious.tools")

    def recording(fn):
        def wrapped(*a, **k):
            m = fn(*a, **k)
            RECORDED.append(m)
            return m
        return wrapped

    for fn in ("_background_activity_filter", "_contrast_threshold_control", "_refractory_period"):
        setattr(filters, fn, recording(getattr(filters, fn)))
    return events_mod.Events, utils, filters


def streams():
    from event_representation_study_amd.synthetic import make_events_edges
    out = {}
    W, H = 72, 48
    ev = make_events_edges(20000, W, H, seed=0, span_us=100000)
    t = ev[:, 2].astype(np.int64) + 3_000_000_000          # absolute times beyond int32
    out["clustered"] = (ev[:, 0], ev[:, 1], t, ev[:, 3], W, H)
    # the same with one planted pixel of 5 000 events spread over the span
    rng = np.random.default_rng(1)
    th = np.sort(rng.integers(0, 100000, 5000)).astype(np.int64) + 3_000_000_000
    x = np.concatenate([ev[:, 0], np.full(5000, 40)])
    y = np.concatenate([ev[:, 1], np.full(5000, 20)])
    p = np.concatenate([ev[:, 3], rng.choice([-1, 1], 5000)])
    tt = np.concatenate([t, th])
    o = np.argsort(tt, kind="stable")
    out["planted"] = (x[o], y[o], tt[o], p[o], W, H)
    # edges: a 16 x 12 sensor, absolute times from -100 (the `t_last > 0` quirk) with many ties, events on every border
    rng = np.random.default_rng(2)
    n, W2, H2 = 600, 16, 12
    x = rng.integers(0, W2, n)
    y = rng.integers(0, H2, n)
    x[::7] = 0
    y[3::7] = 0
    x[5::7] = W2 - 1
    y[6::7] = H2 - 1
    x[:4], y[:4] = [0, W2 - 1, 0, W2 - 1], [0, 0, H2 - 1, H2 - 1]
    t = np.sort(rng.integers(-100, 400, n)).astype(np.int64)
    out["edges"] = (x, y, t, rng.choice([-1, 1], n), W2, H2)
    out["one"] = (np.array([5]), np.array([7]), np.array([3_000_000_123], np.int64), np.array([1]), W2, H2)
    out["none"] = (np.zeros(0, int), np.zeros(0, int), np.zeros(0, np.int64), np.zeros(0, int), W2, H2)
    return {k: (v[0].astype(np.uint16), v[1].astype(np.uint16), v[2].astype(np.int64), np.asarray(v[3]).astype(np.int8), v[4], v[5])
            for k, v in out.items()}


def cases():
    c = []
    for s in ("clustered",):
        for per in (50, 500, 5000):
            c.append(dict(name="refractory_%d" % per, filter="refractory", param=per, stream=s, strict=True))
        for f in (2, 3, 5):
            c.append(dict(name="contrast_%d" % f, filter="contrast", param=f, stream=s, strict=True))
        for r in (1, 2):
            for d in (20, 200, 2000):
                c.append(dict(name="background_r%d_d%d" % (r, d), filter="background", param=d, radius=r, stream=s, strict=True))
        for fx, fy in ((2, 2), (3, 3), (4, 2)):
            c.append(dict(name="resize_%dx%d" % (fx, fy), filter="resize", fx=fx, fy=fy, stream=s, strict=True))
    c.append(dict(name="hotpixel_planted", filter="hotpixel", stream="planted", strict=True))
    c.append(dict(name="hotpixel_none", filter="hotpixel", stream="clustered", strict=False))     # ratio <= 2: everything passes
    # two consecutive inserts into one filter object
    c.append(dict(name="refractory_500_two", filter="refractory", param=500, stream="clustered", split=2, strict=True))
    c.append(dict(name="contrast_3_two", filter="contrast", param=3, stream="clustered", split=2, strict=True))
    c.append(dict(name="background_r1_d200_two", filter="background", param=200, radius=1, stream="clustered", split=2, strict=True))
    c.append(dict(name="hotpixel_planted_two", filter="hotpixel", stream="planted", split=2, strict=True))
    # one pixel holding 5 000 events
    c.append(dict(name="refractory_500_hot", filter="refractory", param=500, stream="planted", strict=True))
    c.append(dict(name="contrast_3_hot", filter="contrast", param=3, stream="planted", strict=True))
    c.append(dict(name="background_r1_d200_hot", filter="background", param=200, radius=1, stream="planted", strict=True))
    c.append(dict(name="resize_2x2_hot", filter="resize", fx=2, fy=2, stream="planted", strict=True))
    # borders, t <= 0, ties
    c.append(dict(name="refractory_20_edges", filter="refractory", param=20, stream="edges", strict=True))
    c.append(dict(name="contrast_2_edges", filter="contrast", param=2, stream="edges", strict=True))
    for r in (1, 2, 4):
        c.append(dict(name="background_r%d_d5_edges" % r, filter="background", param=5, radius=r, stream="edges", strict=True))
    c.append(dict(name="resize_2x2_edges", filter="resize", fx=2, fy=2, stream="edges", strict=False))
    for s in ("one", "none"):
        c.append(dict(name="refractory_50_%s" % s, filter="refractory", param=50, stream=s, strict=False))
        c.append(dict(name="contrast_2_%s" % s, filter="contrast", param=2, stream=s, strict=False))
        c.append(dict(name="background_r1_d20_%s" % s, filter="background", param=20, radius=1, stream=s, strict=False))
    return c


def main(ref_root):
    Events, utils, filters = load_reference(ref_root)
    arrays, manifest = {}, []
    st = streams()
    for k, (x, y, t, p, W, H) in st.items():
        arrays["stream.%s.x" % k], arrays["stream.%s.y" % k] = x, y
        arrays["stream.%s.t" % k], arrays["stream.%s.p" % k] = t, p
        arrays["stream.%s.size" % k] = np.array([W, H], np.int32)
    for c in cases():
        x, y, t, p, W, H = st[c["stream"]]
        ev = Events(x=x.copy(), y=y.copy(), t=t.copy(), p=p.copy(), width=W, height=H)
        n = len(x)
        split = c.get("split", 1)
        cuts = [n * i // split for i in range(split + 1)]
        name = c["name"]
        if c["filter"] == "resize":
            out = utils.resize_to_resolution(ev, H // c["fy"], W // c["fx"], chunks=1)
            mask = np.zeros(n, bool)
            cm = np.zeros((H // c["fy"], W // c["fx"]), "float32")
            mask, cm = utils._filter_events_resize(ev.x, ev.y, ev.p, mask, cm, c["fx"], c["fy"])
            assert np.array_equal(out.t, ev.t[mask])
            out3 = utils.resize_to_resolution(ev, H // c["fy"], W // c["fx"], chunks=3)      # chunks do not change the result
            assert np.array_equal(out3.x, out.x) and np.array_equal(out3.t, out.t)
            arrays[name + ".mask0"], arrays[name + ".state"] = mask, cm
            arrays[name + ".out_x"], arrays[name + ".out_y"] = out.x, out.y
            arrays[name + ".out_t"], arrays[name + ".out_p"] = out.t, out.p
            arrays[name + ".out_size"] = np.array([out.width, out.height], np.int32)
            masks = [mask]
        else:
            if c["filter"] == "refractory":
                f = filters.RefractoryPeriod(c["param"])
            elif c["filter"] == "contrast":
                f = filters.ContrastThresholdIncrease(c["param"])
            elif c["filter"] == "background":
                f = filters.BackgroundActivity(c["param"], c["radius"])
            else:
                f = filters.HotPixel()
            masks = []
            for i in range(split):
                sub = ev[cuts[i]:cuts[i + 1]]
                RECORDED.clear()
                got = f.insert(sub)
                # the filters hand back events[mask]; the mask itself is what their loop returned (recorded below)
                mask = f.hot_pixel_mask[sub.y, sub.x] if c["filter"] == "hotpixel" else RECORDED[0]
                mask = np.asarray(mask, bool).copy()
                assert np.array_equal(got.t, sub.t[mask]) and np.array_equal(got.x, sub.x[mask])
                masks.append(mask)
                arrays[name + ".mask%d" % i] = mask
            state = {"refractory": lambda: f.timestamps, "contrast": lambda: f.counter_map, "background": lambda: f.timestamps,
                     "hotpixel": lambda: f.hot_pixel_mask}[c["filter"]]()
            arrays[name + ".state"] = np.asarray(state)
        if c["strict"]:      # a constant mask cannot pass
            for m in masks:
                assert m.sum() >= 50 and (~m).sum() >= 50, (name, int(m.sum()), int((~m).sum()))
        c["cuts"] = cuts
        c["kept"] = [int(m.sum()) for m in masks]
        manifest.append(c)
        print(name, c["kept"], [len(m) for m in masks])
    arrays["manifest"] = np.array(json.dumps(manifest))
    np.savez_compressed(os.path.join(HERE, "evl_filters.npz"), **arrays)


if __name__ == "__main__":
    main(sys.argv[1])
