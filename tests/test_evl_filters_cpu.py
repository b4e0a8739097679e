"""CPU-only: the ev-licious event filters (event_representation_study_amd.evlicious_filters, evrep_filter_*).

* a plain numpy restatement of the five filters, held BIT-EQUAL to tests/golden/evl_filters.npz (the reference's own loops,
  see tests/golden/make_golden_evl_filters.py): masks, outgoing states, resize outputs.  This pins the restatement the GPU
  tests (test_gpu_evl_filters.py) use on larger streams;
* the closed form of BackgroundActivity (what the kernels evaluate) against the loop form;
* the C ABI's argument checks of every new entry point (nothing is launched);
* the Python module imports, raises EvrepError without a device, and refuses `Random`.
"""
import ctypes
import json
import types

import numpy as np
import pytest

from conftest import load_golden


# ------------------------------------------------------------------------------------------------ the restatement
def restate_refractory(x, y, t, period, last):
    """per pixel: pass iff t - last >= period; only a passing event sets last.  last: float64 (H, W), updated in place."""
    mask = np.ones(len(x), bool)
    for i in range(len(x)):
        if float(t[i]) - last[y[i], x[i]] < period:
            mask[i] = False
        else:
            last[y[i], x[i]] = t[i]
    return mask


def restate_contrast(x, y, p, factor, activity):
    """activity int32 (H, W) += p; pass iff |activity| >= factor, then reset."""
    mask = np.zeros(len(x), bool)
    for i in range(len(x)):
        a = int(activity[y[i], x[i]]) + int(p[i])
        if abs(a) >= factor:
            mask[i] = True
            a = 0
        activity[y[i], x[i]] = a
    return mask


def restate_change_map(x, y, p, fx, fy, change):
    """change float32 (H // fy, W // fx): the float64 sum change + p / (fx * fy) rounded to float32; |change| >= 1: pass, -= p."""
    mask = np.zeros(len(x), bool)
    cells = float(fx * fy)
    for i in range(len(x)):
        cy, cx = int(y[i]) // fy, int(x[i]) // fx
        c = np.float32(float(change[cy, cx]) + float(p[i]) * 1.0 / cells)
        if abs(c) >= 1:
            mask[i] = True
            c = np.float32(float(c) - float(p[i]))
        change[cy, cx] = c
    return mask


def restate_resize(x, y, t, p, W, H, height, width, change=None):
    fx, fy = int(W / width), int(H / height)
    if W % fx or H % fy:
        raise ValueError("not a whole number of cells")
    if change is None:
        change = np.zeros((height, width), np.float32)
    mask = restate_change_map(x, y, p, fx, fy, change)
    out = dict(x=(x[mask] * (1.0 / fx)).astype(np.uint16), y=(y[mask] * (1.0 / fy)).astype(np.uint16), t=t[mask], p=p[mask],
               width=int(W * (1.0 / fx)), height=int(H * (1.0 / fy)))
    return mask, change, out


def restate_background_loop(x, y, t, depth, radius, ts):
    """The loop form: read timestamps[y, x], then EVERY event writes t into [max(y - r, 0), y + r) x [max(x - r, 0), x + r)."""
    mask = np.ones(len(x), bool)
    for i in range(len(x)):
        xi, yi, ti = int(x[i]), int(y[i]), int(t[i])
        t_last = ts[yi, xi]
        mask[i] = not (t_last > 0 and ti - t_last > depth)
        ts[max(yi - radius, 0):yi + radius, max(xi - radius, 0):xi + radius] = ti
    return mask


def restate_background_closed(x, y, t, depth, radius, ts):
    """The closed form: t_last(i) = t of the latest earlier event j with x_i - r + 1 <= x_j <= x_i + r and
    y_i - r + 1 <= y_j <= y_i + r, else the incoming state.  No sequential dependence; quadratic, small inputs only."""
    x, y, t = x.astype(np.int64), y.astype(np.int64), t.astype(np.int64)
    mask = np.ones(len(x), bool)
    H, W = ts.shape
    for i in range(len(x)):
        near = (x[:i] >= x[i] - radius + 1) & (x[:i] <= x[i] + radius) & (y[:i] >= y[i] - radius + 1) & (y[:i] <= y[i] + radius)
        j = np.flatnonzero(near)
        t_last = float(t[j[-1]]) if j.size else ts[y[i], x[i]]
        mask[i] = not (t_last > 0 and t[i] - t_last > depth)
    out = ts.copy()
    for py in range(H):
        for px in range(W):
            near = (x >= px - radius + 1) & (x <= px + radius) & (y >= py - radius + 1) & (y <= py + radius)
            j = np.flatnonzero(near)
            if j.size:
                out[py, px] = t[j[-1]]
    ts[...] = out
    return mask


def restate_hotpixel_mask(x, y, H, W, threshold=0.6):
    count = np.zeros((H, W))
    np.add.at(count, (y, x), 1.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        mask = count / np.max(count) < threshold
        if not mask.any() or mask.all():
            raise ValueError("zero-size array to reduction operation")
        if float(np.min(count[~mask])) / np.max(count[mask]) > 2:
            return mask
    return np.ones((H, W)) > 0


class Restated:
    """One filter object with carried state, the shape of the reference's classes."""
    def __init__(self, kind, param=None, radius=None):
        self.kind, self.param, self.radius, self.state = kind, param, radius, None

    def insert(self, x, y, t, p, W, H):
        if self.state is None and self.kind != "hotpixel":
            self.state = np.zeros((H, W), np.int32) if self.kind == "contrast" else np.full((H, W), -np.inf)
        if self.kind == "refractory":
            return restate_refractory(x, y, t, self.param, self.state)
        if self.kind == "contrast":
            return restate_contrast(x, y, p, self.param, self.state)
        if self.kind == "background":
            return restate_background_loop(x, y, t, self.param, self.radius, self.state)
        if self.state is None:
            self.state = restate_hotpixel_mask(x, y, H, W)
        return self.state[y, x]


# ------------------------------------------------------------------------------------------------ goldens
def golden_cases():
    g = load_golden("evl_filters")
    return g, json.loads(str(g["manifest"]))


def golden_stream(g, name):
    W, H = (int(v) for v in g["stream.%s.size" % name])
    return g["stream.%s.x" % name], g["stream.%s.y" % name], g["stream.%s.t" % name], g["stream.%s.p" % name], W, H


_G, _CASES = golden_cases()


def assert_same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), what


def check_strict(case, masks):
    """A constant mask cannot pass: every strict case keeps at least 50 events and drops at least 50."""
    if case["strict"]:
        for m in masks:
            assert m.sum() >= 50 and (~m).sum() >= 50, case["name"]


@pytest.mark.parametrize("case", _CASES, ids=[c["name"] for c in _CASES])
def test_restatement_is_bit_equal_to_the_reference(case):
    x, y, t, p, W, H = golden_stream(_G, case["stream"])
    name = case["name"]
    if case["filter"] == "resize":
        mask, change, out = restate_resize(x, y, t, p, W, H, H // case["fy"], W // case["fx"])
        assert_same(mask, _G[name + ".mask0"], name)
        assert_same(change, _G[name + ".state"], name + " change map")
        for k in "xytp":
            assert_same(out[k], _G[name + ".out_" + k], name + " out " + k)
        assert [out["width"], out["height"]] == [int(v) for v in _G[name + ".out_size"]]
        check_strict(case, [_G[name + ".mask0"]])
        return
    f = Restated(case["filter"], case.get("param"), case.get("radius"))
    cuts = case["cuts"]
    masks = []
    for i in range(len(cuts) - 1):
        s = slice(cuts[i], cuts[i + 1])
        mask = f.insert(x[s], y[s], t[s], p[s], W, H)
        assert_same(mask, _G[name + ".mask%d" % i], "%s insert %d" % (name, i))
        assert int(mask.sum()) == case["kept"][i]
        masks.append(_G[name + ".mask%d" % i])
    if len(x) or case["filter"] != "hotpixel":
        assert_same(f.state, _G[name + ".state"], name + " state")
    check_strict(case, masks)


def test_golden_covers_the_cases_the_filters_are_specified_on():
    names = {c["name"] for c in _CASES}
    for want in ["refractory_50", "refractory_500", "refractory_5000", "contrast_2", "contrast_3", "contrast_5",
                 "background_r1_d20", "background_r1_d200", "background_r1_d2000", "background_r2_d20", "background_r2_d200",
                 "background_r2_d2000", "resize_2x2", "resize_3x3", "resize_4x2", "hotpixel_planted", "hotpixel_none",
                 "refractory_500_two", "contrast_3_two", "background_r1_d200_two", "refractory_500_hot",
                 "background_r1_d5_edges", "refractory_50_one", "refractory_50_none"]:
        assert want in names
    t = _G["stream.clustered.t"]
    assert t.dtype == np.int64 and t.min() > 2 ** 31                        # absolute times beyond int32
    te = _G["stream.edges.t"]
    assert te.min() <= 0 and len(np.unique(te)) < len(te)                      # t <= 0 and ties
    xe, ye = _G["stream.edges.x"], _G["stream.edges.y"]
    assert xe.min() == 0 and ye.min() == 0 and xe.max() == 15 and ye.max() == 11
    xp, yp = _G["stream.planted.x"], _G["stream.planted.y"]
    assert np.bincount(yp.astype(np.int64) * 72 + xp).max() >= 5000          # one pixel holding 5 000 events
    assert not _G["hotpixel_planted.state"].all() and _G["hotpixel_none.state"].all()


@pytest.mark.parametrize("radius", [1, 2, 4])
def test_background_closed_form_equals_the_loop(radius):
    x, y, t, p, W, H = golden_stream(_G, "edges")
    for depth, first in ((5, None), (5, 250)):
        a, b = np.full((H, W), -np.inf), np.full((H, W), -np.inf)
        if first:                                             # a carried state: two inserts
            restate_background_loop(x[:first], y[:first], t[:first], depth, radius, a)
            b[...] = a
        s = slice(first or 0, None)
        m_loop = restate_background_loop(x[s], y[s], t[s], depth, radius, a)
        m_closed = restate_background_closed(x[s], y[s], t[s], depth, radius, b)
        assert np.array_equal(m_loop, m_closed)
        assert_same(a, b, "timestamps")
        assert 10 <= m_loop.sum() <= len(m_loop) - 10      # neither mask is constant


def test_background_closed_form_on_the_clustered_stream():
    x, y, t, p, W, H = golden_stream(_G, "clustered")
    n = 3000
    a, b = np.full((H, W), -np.inf), np.full((H, W), -np.inf)
    assert np.array_equal(restate_background_loop(x[:n], y[:n], t[:n], 200, 1, a),
                          restate_background_closed(x[:n], y[:n], t[:n], 200, 1, b))
    assert_same(a, b, "timestamps")


def test_resize_refuses_a_sensor_the_cells_do_not_divide():
    x, y, t, p, W, H = golden_stream(_G, "edges")
    with pytest.raises(ValueError):
        restate_resize(x, y, t, p, 64, 48, 16, 21)            # 64 / 3


def test_cell_coordinates_are_floor_division():
    """x * (1.0 / fx) truncated == x // fx for every coordinate of a sensor, which is what the cell-map kernel computes; and
    the kernel's multiply-shift reciprocal is exact."""
    x = np.arange(4096, dtype=np.uint16)
    for f in (2, 3, 4, 5, 6, 7):
        assert np.array_equal((x * (1.0 / f)).astype(np.uint16), x // f)
    for f in range(2, 4097):
        m = (1 << 32) // f + 1
        assert m < 1 << 32
        assert np.array_equal((x.astype(np.uint64) * np.uint64(m)) >> np.uint64(32), x.astype(np.uint64) // np.uint64(f)), f


# ------------------------------------------------------------------------------------------------ the C ABI, no launch
@pytest.fixture(scope="module")
def lib():
    from event_representation_study_amd import build, _lib
    build.build()
    return _lib.load()


def _plan(lib, B=1, H=8, W=8, n=4):
    from event_representation_study_amd._lib import Plan
    p = Plan()
    assert lib.evrep_plan_init(ctypes.byref(p), B, H, W, n, n) == 0
    return p


P = ctypes.c_void_p


def test_filter_symbols_are_declared_bound_and_exported(lib):
    from event_representation_study_amd import _lib
    for name in ("evrep_filter_pixel_fsm", "evrep_filter_background", "evrep_filter_mask_gather", "evrep_filter_cell_map",
                 "evrep_filter_compact", "evrep_filter_compact_scratch_bytes"):
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
    assert (_lib.FILTER_REFRACTORY, _lib.FILTER_CONTRAST, _lib.FILTER_CHANGE_MAP) == (0, 1, 2)
    assert lib.evrep_abi_version() == 3


def test_pixel_fsm_refuses_bad_arguments(lib):
    from event_representation_study_amd._lib import EVREP_EINVAL
    p = _plan(lib)
    ok = dict(ev=P(256), off=P(256), ws=P(256), kind=0, param=50.0, tb=None, state=P(256), keep=P(256))

    def call(**kw):
        a = dict(ok, **kw)
        return lib.evrep_filter_pixel_fsm(ctypes.byref(p), a["ev"], a["off"], a["ws"], a["kind"], a["param"], a["tb"], a["state"],
                                          a["keep"], None)
    for bad in (dict(ev=None), dict(off=None), dict(ws=None), dict(ev=P(8)), dict(ws=P(128)), dict(kind=3), dict(kind=-1),
                dict(param=0.0), dict(param=-1.0), dict(param=float("nan")), dict(state=None), dict(state=P(260)),
                dict(kind=1, state=P(258)), dict(kind=2, state=P(257)), dict(keep=None)):
        assert call(**bad) == EVREP_EINVAL, bad
    assert lib.evrep_filter_pixel_fsm(None, P(256), P(256), P(256), 0, 50.0, None, P(256), P(256), None) == EVREP_EINVAL


def test_background_refuses_bad_arguments(lib):
    from event_representation_study_amd._lib import EVREP_EINVAL
    p = _plan(lib)
    ok = dict(ev=P(256), off=P(256), ws=P(256), depth=20.0, radius=1, state=P(256), keep=P(256))

    def call(**kw):
        a = dict(ok, **kw)
        return lib.evrep_filter_background(ctypes.byref(p), a["ev"], a["off"], a["ws"], a["depth"], a["radius"], None, a["state"],
                                           a["keep"], None)
    for bad in (dict(ev=None), dict(off=None), dict(ws=None), dict(ev=P(8)), dict(depth=0.0), dict(depth=-5.0),
                dict(depth=float("nan")), dict(radius=0), dict(radius=5), dict(radius=-1), dict(state=None), dict(state=P(260)),
                dict(keep=None)):
        assert call(**bad) == EVREP_EINVAL, bad


def test_gather_cell_map_and_compact_refuse_bad_arguments(lib):
    from event_representation_study_amd._lib import EVREP_EINVAL
    a = P(256)
    for args in ((None, a, 1, 8, 8, 4, a, a), (a, None, 1, 8, 8, 4, a, a), (a, a, 0, 8, 8, 4, a, a), (a, a, 1, 0, 8, 4, a, a),
                 (a, a, 1, 8, 5000, 4, a, a), (a, a, 1, 8, 8, -1, a, a), (a, a, 1, 8, 8, 4, None, a), (a, a, 1, 8, 8, 4, a, None),
                 (P(8), a, 1, 8, 8, 4, a, a), (a, a, 65536, 8, 8, 4, a, a)):
        assert lib.evrep_filter_mask_gather(*args, None) == EVREP_EINVAL, args
    for args in ((None, 4, 8, 8, 2, 2, a), (a, 4, 8, 8, 2, 2, None), (a, -1, 8, 8, 2, 2, a), (a, 4, 0, 8, 2, 2, a),
                 (a, 4, 8, 8, 0, 2, a), (a, 4, 8, 8, 2, 0, a), (a, 4, 8, 8, 9, 2, a), (a, 4, 8, 8, 2, 9, a), (P(8), 4, 8, 8, 2, 2, a),
                 (a, 4, 8, 8, 2, 2, P(8)), (a, 4, 8, 5000, 2, 2, a)):
        assert lib.evrep_filter_cell_map(*args, None) == EVREP_EINVAL, args
    for args in ((None, a, 1, a, a, a, a), (a, None, 1, a, a, a, a), (a, a, 0, a, a, a, a), (a, a, 1, None, a, a, a),
                 (a, a, 1, a, None, a, a), (a, a, 1, a, a, None, a), (a, a, 1, a, a, a, None), (P(8), a, 1, a, a, a, a),
                 (a, a, 1, a, P(8), a, a), (a, a, 1, a, a, P(4), a), (a, a, 1, a, a, a, P(8)), (a, a, 65536, a, a, a, a)):
        assert lib.evrep_filter_compact(*args, None) == EVREP_EINVAL, args
    assert lib.evrep_filter_compact_scratch_bytes(0, 10) == 0 and lib.evrep_filter_compact_scratch_bytes(1, -1) == 0
    n = lib.evrep_filter_compact_scratch_bytes(32, 1600000)
    assert 4096 <= n <= 1 << 16 and n % 256 == 0


# ------------------------------------------------------------------------------------------------ the Python module
def test_module_mirrors_the_reference_names():
    from event_representation_study_amd import evlicious_filters as f
    assert [(k, int(v)) for k, v in f.Filtering_Type.__members__.items()] == [
        ("BackgroundActivity", 1), ("Random", 2), ("ContrastThresholdIncrease", 3), ("RefractoryPeriod", 4), ("HotPixel", 5)]
    assert "HotPixel=5" in f.Filtering_Type.summary()
    flags = types.SimpleNamespace(filter_type=1, depth_us=200, radius=2, contrast_threshold_multiplier=3, random_downsampling_factor=2)
    ba = f.from_flags(flags)
    assert isinstance(ba, f.BackgroundActivity) and (ba.depth_us, ba.radius, ba.timestamps) == (200, 2, None)
    flags.filter_type = 3
    assert f.from_flags(flags).contrast_threshold_multiplier == 3 and f.from_flags(flags).counter_map is None
    flags.filter_type = 4
    assert f.from_flags(flags).depth_us == 200
    flags.filter_type = 5
    assert f.from_flags(flags).hot_pixel_mask is None
    flags.filter_type = 9
    with pytest.raises(ValueError):
        f.from_flags(flags)
    flags.filter_type = 2
    with pytest.raises(NotImplementedError, match="seed"):
        f.from_flags(flags)
    with pytest.raises(NotImplementedError):
        f.Random(2)


def test_filters_raise_without_a_device():
    import torch
    if torch.cuda.is_available():
        return                      # a HIP device is visible: test_gpu_evl_filters.py covers the path
    from event_representation_study_amd import evlicious_filters as f
    from event_representation_study_amd._lib import EvrepError
    x, y, t, p, W, H = golden_stream(_G, "edges")
    ev = types.SimpleNamespace(x=x, y=y, t=t, p=p, width=W, height=H)
    for flt in (f.RefractoryPeriod(50), f.ContrastThresholdIncrease(2), f.BackgroundActivity(20, 1), f.HotPixel()):
        with pytest.raises(EvrepError):
            flt.insert(ev)
    with pytest.raises(EvrepError):
        f.resize_to_resolution(ev, H // 2, W // 2)
