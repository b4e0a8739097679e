"""Record tests/golden/evl_render.npz: small event windows and the images ev-licious' ``Events.render`` draws of them, computed
by the REFERENCE's own code.

    python tests/golden/make_golden_evl_render.py /path/to/event_representation_study

The reference's modules ev-licious/src/evlicious/io/utils/render.py, io/utils/events.py and tools/utils.py are imported from the
given checkout with ``numba.jit`` stood in by the identity (numba is absent here: ``_render_no_overlap_numba`` runs as plain
Python -- compiled numba is NOT pinned) and ``cv2`` stood in by a stub whose ``cvtColor(GRAY2BGR)`` stacks three copies of the
gray image, which is all that conversion does.  matplotlib is the real one: ``plt.get_cmap("jet")`` colours the time surface.

For every case (a frame size and a stream) and every rendering type x cast in {True, False} x canvas in {None, a random uint8
canvas} the image is recorded.  The reference ignores ``cast`` and the canvas for TIME_SURFACE and EVENT_FRAME: the script checks
that and stores those images once; ``manifest`` names the stored array of every combination.  Also recorded: matplotlib's jet
table (``jet_lut``) and, for every case, the float32 image numpy's ``np.add.at`` leaves for the time surface (``.surface``).
Only data is written; no program text of the reference.
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TYPES = ("RED_BLUE_OVERLAP", "RED_BLUE_NO_OVERLAP", "BLACK_WHITE_NO_OVERLAP", "TIME_SURFACE", "EVENT_FRAME")


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
    stub("cv2", COLOR_GRAY2BGR=8, cvtColor=lambda img, code: np.stack([img, img, img], axis=-1))

    def load(name, path, package):
        spec = importlib.util.spec_from_file_location(name, path)
        m = importlib.util.module_from_spec(spec)
        m.__package__ = package
        sys.modules[name] = m
        spec.loader.exec_module(m)
        return m

    pkg = stub("evlicious")
    pkg.__path__ = []
    for sub in ("evlicious.io", "evlicious.io.utils", "evlicious.tools"):
        stub(sub).__path__ = []
    render = load("evlicious.io.utils.render", os.path.join(src, "io", "utils", "render.py"), "evlicious.io.utils")
    events = load("evlicious.io.utils.events", os.path.join(src, "io", "utils", "events.py"), "evlicious.io.utils")
    pkg.Events = events.Events
    utils = load("evlicious.tools.utils", os.path.join(src, "tools", "utils.py"), "evlicious.tools")
    pkg.tools = sys.modules["evlicious.tools"]
    pkg.tools.stack = utils.stack
    return events.Events, render.RenderingType


def cases():
    """name -> (x, y, t, p, H, W)"""
    rng = np.random.default_rng(20)
    out = {}

    def rand(n, H, W, t_hi=100000, pol=(-1, 1)):
        return [rng.integers(0, W, n), rng.integers(0, H, n), np.sort(rng.integers(0, t_hi, n)), rng.choice(pol, n)]

    def put(name, H, W, x, y, t, p):
        out[name] = (np.asarray(x).astype(np.uint16), np.asarray(y).astype(np.uint16), np.asarray(t).astype(np.int64),
                     np.asarray(p).astype(np.int8), H, W)

    def few(prefix, H, W):
        for n in range(4):      # the TIME_SURFACE quirk: <= 2 events give a uint8 zero image
            put("%s_n%d" % (prefix, n), H, W, *rand(n, H, W))

    def one_pixel(name, H, W, x, y):      # net passes +-7, the last-event flag flips
        n = 300
        p = np.where(np.arange(n) % 2 == 0, 1, -1)
        p[:40] = 1
        p[200:260] = -1
        put(name, H, W, np.full(n, x), np.full(n, y), np.arange(n) * 997, p)

    one_pixel("1x1_onepixel", 1, 1, 0, 0)
    few("1x1", 1, 1)
    for H, W in ((1, 5), (5, 1)):
        put("%dx%d_random" % (H, W), H, W, *rand(40, H, W, t_hi=60000))
        x, y, t, p = rand(12, H, W)
        x[::2], y[::2] = W - 1, H - 1
        put("%dx%d_edges" % (H, W), H, W, x, y, t, p)
    H, W = 3, 7
    put("3x7_random", H, W, *rand(60, H, W, t_hi=90000))
    put("3x7_positive", H, W, *rand(30, H, W, pol=(1,)))
    put("3x7_negative_as_zero", H, W, *rand(30, H, W, pol=(0,)))      # Events.__init__ turns p == 0 into -1
    x, y, t, p = rand(50, H, W)
    put("3x7_ties", H, W, x, y, np.sort(rng.integers(0, 4, 50)) * 20000, p)
    x, y, t, p = rand(50, H, W, t_hi=120000)
    put("3x7_unsorted", H, W, x, y, rng.permutation(t), p)
    x, y, t, p = rand(50, H, W, t_hi=150000)
    put("3x7_big_t", H, W, x, y, t + 1_600_000_000_000_000, p)
    x, y, t, p = rand(30, H, W)
    x[::3], y[1::3] = W - 1, H - 1
    x[-1], y[-1] = W - 1, H - 1
    put("3x7_edges", H, W, x, y, t, p)
    one_pixel("3x7_onepixel", H, W, 6, 2)
    few("3x7", H, W)
    H, W = 9, 130
    put("9x130_random", H, W, *rand(800, H, W))
    x, y, t, p = rand(300, H, W)
    x[::3], y[1::3] = W - 1, H - 1
    x[2::9] = 127
    x[5::9] = 128
    put("9x130_edges", H, W, x, y, t, p)
    x, y, t, p = rand(400, H, W, t_hi=200000)
    put("9x130_unsorted", H, W, x, y, rng.permutation(t), p)
    one_pixel("9x130_onepixel", H, W, 128, 4)
    H, W = 240, 304
    x, y, t, p = rand(2000, H, W, t_hi=2000)      # many tied timestamps
    put("240x304_random", H, W, x, y, t * 50, p)
    return out


def main(ref_root):
    Events, RT = load_reference(ref_root)
    import matplotlib
    import matplotlib.pyplot as plt
    arrays, manifest = {}, {}
    cm = plt.get_cmap("jet")
    arrays["jet_lut"] = np.asarray(cm(np.arange(256)), dtype=np.float64)
    versions = dict(numpy=np.__version__, matplotlib=matplotlib.__version__)
    rng = np.random.default_rng(21)
    for name, (x, y, t, p, H, W) in cases().items():
        for k, v in zip("xytp", (x, y, t, p)):
            arrays["%s.%s" % (name, k)] = v.copy()
        arrays[name + ".size"] = np.array([H, W], np.int32)
        canvas = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
        if H * W > 5000:      # (the file stays small: the big frame's canvas is random per 8 x 8 block)
            canvas = np.kron(canvas[:H // 8, :W // 8], np.ones((8, 8, 1), np.uint8))
        arrays[name + ".canvas"] = canvas
        ev = Events(x=x.copy(), y=y.copy(), t=t.copy(), p=p.copy(), width=W, height=H)
        surface = np.zeros((H, W), np.float32)
        if len(x):
            np.add.at(surface, (ev.y, ev.x), np.exp(-(ev.t.astype("int")[-1] - ev.t.astype("int")) / 3e4))
        arrays[name + ".surface"] = surface
        entry = {}
        for tname in TYPES:
            for cast in (True, False):
                for with_canvas in (False, True):
                    given = canvas.copy() if with_canvas else None
                    img = ev.render(given, getattr(RT, tname), cast)
                    if with_canvas:
                        assert np.array_equal(given, canvas), "the reference drew into the caller's canvas"
                    key = "%s.%s.cast%d.canvas%d" % (name, tname, cast, with_canvas)
                    if tname in ("TIME_SURFACE", "EVENT_FRAME"):      # cast and the canvas are ignored: stored once
                        first = "%s.%s.cast1.canvas0" % (name, tname)
                        if key != first:
                            assert img.dtype == arrays[first].dtype and np.array_equal(img, arrays[first]), key
                            entry[key] = first
                            continue
                    arrays[key] = img
                    entry[key] = key
        manifest[name] = entry
        print(name, len(x), "events", (H, W))
    arrays["manifest"] = np.array(json.dumps(dict(cases=manifest, versions=versions, types={n: i + 1 for i, n in enumerate(TYPES)},
                                                  reference_types={m.name: int(m.value) for m in RT})))
    np.savez_compressed(os.path.join(HERE, "evl_render.npz"), **arrays)


if __name__ == "__main__":
    main(sys.argv[1])
