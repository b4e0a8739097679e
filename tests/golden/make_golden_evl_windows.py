"""Record tests/golden/evl_windows.npz: what the REFERENCE's own event handle returns for sliding windows and time queries.

    python tests/golden/make_golden_evl_windows.py /path/to/event_representation_study

The reference's modules ev-licious/src/evlicious/io/h5_event_handle.py, io/utils/event_handle.py and io/utils/events.py are
imported from the given checkout with `h5py`, `hdf5plugin`, `tqdm`, the `H5Writer` and `Visualizer` modules and the `render`
module of `Events` stubbed (none of them is on the path of the recorded calls).  The `handle` an `H5EventHandle` is built on
is a dict of numpy arrays -- `handle["events"]["t"]` indexes and slices as the h5py dataset does, 0-d arrays serve `[()]`.
Recorded per stream: the columns; per case and unit combination (step_size_unit x window_unit): timestamps0, timestamps1,
i0, i1 of `compute_time_and_index_windows`; per stream a list of `find_index_from_timestamp` queries (int and float, equal
to a timestamp, between two, before the first, after the last) and of `get_between_time` pairs (the length and the first and
last timestamp of the returned Events).  Only data is written; no program text of the reference.
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
UNITS = [(s, w) for s in ("nr", "us") for w in ("nr", "us")]       # (step_size_unit, window_unit)


def load_reference(ref_root):
    src = os.path.join(ref_root, "ev-licious", "src", "evlicious")

    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    def load(name, path, package):
        spec = importlib.util.spec_from_file_location(name, path)
        m = importlib.util.module_from_spec(spec)
        m.__package__ = package
        sys.modules[name] = m
        spec.loader.exec_module(m)
        return m

    stub("h5py")
    stub("hdf5plugin")
    stub("tqdm")
    for pkg in ("evlicious", "evlicious.io", "evlicious.io.utils"):
        stub(pkg).__path__ = []
    stub("evlicious.io.utils.render", _render=None, RenderingType=types.SimpleNamespace(RED_BLUE_OVERLAP=0))
    stub("evlicious.io.utils.h5_writer", H5Writer=None)
    stub("evlicious.io.utils.visualization", Visualizer=None)
    load("evlicious.io.utils.events", os.path.join(src, "io", "utils", "events.py"), "evlicious.io.utils")
    sys.modules["evlicious.io.utils"].event_handle = load("evlicious.io.utils.event_handle",
                                                          os.path.join(src, "io", "utils", "event_handle.py"), "evlicious.io.utils")
    return load("evlicious.io.h5_event_handle", os.path.join(src, "io", "h5_event_handle.py"), "evlicious.io").H5EventHandle


def streams():
    """name -> (x u16, y u16, t i64 ascending, p i8 in {-1, +1}, W, H)"""
    out = {}
    W, H = 72, 48

    def cols(rng, t):
        n = len(t)
        return (rng.integers(0, W, n).astype(np.uint16), rng.integers(0, H, n).astype(np.uint16), np.asarray(t, np.int64),
                rng.choice([-1, 1], n).astype(np.int8), W, H)

    # 20 000 events over 100 ms at absolute times near 3e9 (beyond int32), with long runs of equal timestamps: 2 000 distinct
    # values drawn with repetition, plus three planted runs of 300, 64 and 65 equal stamps
    rng = np.random.default_rng(11)
    t = rng.choice(np.arange(0, 100000, 50), 20000 - 429)
    t = np.sort(np.concatenate([t, np.full(300, 40000), np.full(64, 70050), np.full(65, 90100)])) + 3_000_000_000
    out["ties"] = cols(rng, t)
    # two silences of 30 ms and 45 ms, longer than every window used on this stream
    rng = np.random.default_rng(12)
    t = np.sort(np.concatenate([rng.integers(0, 20000, 2500), rng.integers(50000, 60000, 1500), rng.integers(105000, 125000, 2000)]))
    out["gaps"] = cols(rng, t + 1_000_000)
    rng = np.random.default_rng(13)
    out["n6000"] = cols(rng, np.sort(rng.integers(0, 60000, 6000)) + 5_000_000_000)      # divisible by the step 500
    out["n6007"] = cols(rng, np.sort(rng.integers(0, 60000, 6007)) + 5_000_000_000)      # not divisible
    out["short"] = cols(rng, np.sort(rng.integers(0, 3000, 300)) + 2_000_000)
    out["one"] = cols(rng, np.array([3_000_000_123]))
    return out


def cases():
    c = [dict(name="ties_s1000_w5000", stream="ties", step=1000, window=5000, strict=True),       # nr/nr: six clipped zeros collapse
         dict(name="ties_s2500_w2500", stream="ties", step=2500, window=2500, strict=True),
         dict(name="ties_s777_w3001", stream="ties", step=777, window=3001, strict=True),
         dict(name="gaps_s600_w1500", stream="gaps", step=600, window=1500, strict=True),
         dict(name="gaps_s500_w700", stream="gaps", step=500, window=700, strict=True),           # us/us: empty windows in the silences
         dict(name="n6000_s500_w1500", stream="n6000", step=500, window=1500, strict=True),
         dict(name="n6007_s500_w1500", stream="n6007", step=500, window=1500, strict=True),
         dict(name="short_window_gt_n", stream="short", step=100, window=5000, strict=False),
         dict(name="short_step_gt_n", stream="short", step=4000, window=50, strict=False),
         dict(name="one_event", stream="one", step=1, window=1, strict=False)]
    return c


def queries(t):
    """find_index_from_timestamp queries: ints and floats, on a timestamp, between two, before the first, after the last."""
    rng = np.random.default_rng(5)
    t0, t1 = int(t[0]), int(t[-1])
    on = rng.choice(t, min(len(t), 12))
    qi = np.concatenate([[t0 - 1000, t0 - 1, t0, t0 + 1, t1 - 1, t1, t1 + 1, t1 + 1000], on, on - 1, on + 1,
                         rng.integers(t0 - 10, t1 + 10, 24)]).astype(np.int64)
    qf = np.concatenate([qi[:20].astype(np.float64), on + 0.5, on - 0.0005, on - 0.001, on - 0.002, on + 0.9995, on - 0.9985,
                         rng.uniform(t0 - 5, t1 + 5, 24)])
    return qi, qf


def main(ref_root):
    H5EventHandle = load_reference(ref_root)
    arrays, manifest = {}, []
    st = streams()
    handles = {}
    for k, (x, y, t, p, W, H) in st.items():
        assert np.all(np.diff(t) >= 0)
        for f, v in zip("xytp", (x, y, t, p)):
            arrays["stream.%s.%s" % (k, f)] = v
        arrays["stream.%s.size" % k] = np.array([W, H], np.int32)
        handles[k] = H5EventHandle({"events": {"x": x, "y": y, "t": t, "p": p, "height": np.array(H), "width": np.array(W),
                                               "divider": np.array(1)}})
        h = handles[k]
        assert len(h) == len(t) and h.get_time_limits() == (t[0], t[-1])
        qi, qf = queries(t)
        arrays["query.%s.int" % k], arrays["query.%s.float" % k] = qi, qf
        arrays["query.%s.int_idx" % k] = np.asarray(h.find_index_from_timestamp(qi))
        arrays["query.%s.float_idx" % k] = np.asarray(h.find_index_from_timestamp(qf))
        one = h.find_index_from_timestamp(int(qi[2]))                      # a scalar query returns a numpy integer
        assert np.ndim(one) == 0 and one == arrays["query.%s.int_idx" % k][2]
        # get_between_time: pairs of the int queries (ordered and reversed) and of the float queries
        pairs = [(int(qi[a % len(qi)]), int(qi[b % len(qi)])) for a, b in ((0, 7), (2, 5), (3, 4), (5, 2), (8, 9), (10, 30), (31, 12), (1, 1))]
        fpairs = [(float(qf[a % len(qf)]), float(qf[b % len(qf)])) for a, b in ((20, 50), (33, 60), (70, 25))]
        rec = []
        for a, b in pairs + fpairs:
            ev = h.get_between_time(a, b)
            rec.append([len(ev), int(ev.t[0]) if len(ev) else -1, int(ev.t[-1]) if len(ev) else -1])
        arrays["between.%s.int_pairs" % k] = np.array(pairs, np.int64)
        arrays["between.%s.float_pairs" % k] = np.array(fpairs, np.float64)
        arrays["between.%s.result" % k] = np.array(rec, np.int64)
    shorter, empty = [], []
    for c in cases():
        h, n = handles[c["stream"]], len(st[c["stream"]][2])
        c["counts"] = {}
        for su, wu in UNITS:
            (ts0, ts1), (i0, i1) = h.compute_time_and_index_windows(c["step"], c["window"], su, wu)
            key = "%s.%s_%s." % (c["name"], su, wu)
            arrays[key + "timestamps0"], arrays[key + "timestamps1"] = np.asarray(ts0), np.asarray(ts1)
            arrays[key + "i0"], arrays[key + "i1"] = np.asarray(i0), np.asarray(i1)
            nwin = len(list(zip(i0, i1)))
            assert nwin == sum(1 for _ in h.iterator(c["step"], c["window"], su, wu))
            c["counts"][su + "_" + wu] = [int(len(i0)), int(len(i1))]
            if c["strict"]:
                assert nwin >= 8, (c["name"], su, wu, nwin)
                if len(i0) < len(i1):
                    shorter.append(key)
                if np.any(np.asarray(i0)[:nwin] == np.asarray(i1)[:nwin]):
                    empty.append(key)
        manifest.append(c)
        print(c["name"], c["counts"])
    assert "ties_s1000_w5000.nr_nr." in shorter, shorter      # the np.unique quirk: i0 shorter than i1
    assert "gaps_s500_w700.us_us." in empty, empty            # an empty window inside a silence
    assert sorted(c["name"] for c in manifest if not c["strict"]) == ["one_event", "short_step_gt_n", "short_window_gt_n"]
    arrays["manifest"] = np.array(json.dumps(manifest))
    path = os.path.join(HERE, "evl_windows.npz")
    np.savez_compressed(path, **arrays)
    with open(os.path.join(HERE, "README_evl_windows.md"), "w") as f:
        f.write(README % dict(size=os.path.getsize(path), shorter=", ".join(s.rstrip(".") for s in shorter),
                              empty=", ".join(s.rstrip(".") for s in empty)))
    print("wrote", path, os.path.getsize(path))


README = """# evl_windows.npz

Written by `make_golden_evl_windows.py <reference checkout>` (%(size)d bytes): what the reference's `H5EventHandle`
(ev-licious/src/evlicious/io/h5_event_handle.py, io/utils/event_handle.py) returns on six small streams held as numpy
arrays -- `compute_time_and_index_windows` for every case under the four (step_size_unit, window_unit) combinations,
`find_index_from_timestamp` for int and float queries, `get_between_time` for pairs of them.  Data only.

Keys: `stream.<s>.{x,y,t,p,size}`; `<case>.<step_unit>_<window_unit>.{timestamps0,timestamps1,i0,i1}`;
`query.<s>.{int,float,int_idx,float_idx}`; `between.<s>.{int_pairs,float_pairs,result}` (rows: length, first t, last t of
the returned Events, -1 where empty); `manifest` (JSON: name, stream, step, window, strict, counts).

Conditions the generator asserts (the tests assert them again):
- every strict case yields at least 8 windows in every unit combination;
- i0 shorter than i1 (the `np.unique` quirk) in: %(shorter)s;
- an empty window (i0 == i1) in: %(empty)s;
- the only non-strict cases are window > N, step > N and the one-event stream.
"""


if __name__ == "__main__":
    main(sys.argv[1])
