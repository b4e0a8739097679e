"""CPU: the host side of the device-resident recording (event_representation_study_amd/recording.py) against
tests/golden/evl_windows.npz, which the reference's own H5EventHandle wrote (tests/golden/make_golden_evl_windows.py).

The window arithmetic is a pure function that takes the search as a callable: here it is driven by np.searchsorted on the
integer the host forms from a query (``query_to_int``), which is exactly what the device is asked (first t > k).  Everything
is array-equal INCLUDING dtype and length -- integers, no tolerance.  The two new C entry points are checked for their
EVREP_EINVAL cases; nothing is launched.
"""
import ctypes
import json

import numpy as np
import pytest

from conftest import load_golden

_G = load_golden("evl_windows")
_CASES = json.loads(str(_G["manifest"]))
UNITS = [(s, w) for s in ("nr", "us") for w in ("nr", "us")]       # (step_size_unit, window_unit)
STREAMS = sorted({k.split(".")[1] for k in _G if k.startswith("stream.")})


def golden_stream(name):
    x, y, t, p = (_G["stream.%s.%s" % (name, f)] for f in "xytp")
    W, H = (int(v) for v in _G["stream.%s.size" % name])
    return x, y, t, p, W, H


def assert_same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), (what, int((got != want).sum()))


def host_search(t):
    """What DeviceRecording.find_index_from_timestamp computes, with numpy in the device's place."""
    from event_representation_study_amd.recording import query_to_int
    return lambda q: np.searchsorted(t, query_to_int(q), side="right")


def check_windows(case, su, wu, result):
    (ts0, ts1), (i0, i1) = result
    key = "%s.%s_%s." % (case["name"], su, wu)
    for name, got in (("timestamps0", ts0), ("timestamps1", ts1), ("i0", i0), ("i1", i1)):
        assert_same(got, _G[key + name], key + name)


def test_the_golden_meets_its_conditions():
    """Asserted by the generator, and again here: the cases are chosen so that only the reference's behaviour passes."""
    assert sorted(c["name"] for c in _CASES if not c["strict"]) == ["one_event", "short_step_gt_n", "short_window_gt_n"]
    shorter, empty = [], []
    for c in _CASES:
        for su, wu in UNITS:
            key = "%s.%s_%s." % (c["name"], su, wu)
            i0, i1 = _G[key + "i0"], _G[key + "i1"]
            k = min(len(i0), len(i1))
            if c["strict"]:
                assert k >= 8, key
                if len(i0) < len(i1):
                    shorter.append(key)
                if np.any(i0[:k] == i1[:k]):
                    empty.append(key)
    assert "ties_s1000_w5000.nr_nr." in shorter and "gaps_s500_w700.us_us." in empty
    t = _G["stream.ties.t"]
    assert len(t) == 20000 and t[0] >= 3_000_000_000 and np.max(np.bincount((t - t[0]).astype(np.int64))) >= 300


@pytest.mark.parametrize("su,wu", UNITS)
@pytest.mark.parametrize("case", _CASES, ids=[c["name"] for c in _CASES])
def test_window_arithmetic_equals_the_reference(case, su, wu):
    from event_representation_study_amd.recording import time_and_index_windows
    t = golden_stream(case["stream"])[2]
    check_windows(case, su, wu, time_and_index_windows(len(t), lambda idx: t[idx], host_search(t), case["step"], case["window"], su, wu))


@pytest.mark.parametrize("stream", STREAMS)
def test_query_rule_equals_the_reference(stream):
    from event_representation_study_amd.recording import query_to_int
    t = golden_stream(stream)[2]
    for kind in ("int", "float"):
        q = _G["query.%s.%s" % (stream, kind)]
        k = query_to_int(q)
        assert k.dtype == np.int64 and k.shape == q.shape
        assert_same(np.searchsorted(t, k, side="right"), _G["query.%s.%s_idx" % (stream, kind)], "%s %s" % (stream, kind))
    assert np.array_equal(query_to_int(_G["query.%s.int" % stream]), _G["query.%s.int" % stream])      # an int query asks for itself
    assert query_to_int(7).shape == () and int(query_to_int(7)) == 7 and int(query_to_int(6.9995)) == 7 and int(query_to_int(6.5)) == 6


def test_query_rule_refuses_what_float64_cannot_resolve():
    from event_representation_study_amd.recording import query_to_int
    lim = 1 << 43
    assert int(query_to_int(lim - 1)) == lim - 1 and int(query_to_int(-(lim - 1))) == -(lim - 1)
    for bad in (lim, -lim, float(lim), np.array([0, lim + 5]), float("nan"), float("inf")):
        with pytest.raises(ValueError):
            query_to_int(bad)


def test_iterator_pairs_follow_zip_and_slice_semantics():
    from event_representation_study_amd.recording import iterator_pairs
    a, e = iterator_pairs(np.array([3, 7]), np.array([5, 5, 5, 9]))
    assert a.tolist() == [3, 7] and e.tolist() == [5, 7]          # zip stops at the shorter; [7:5] is empty


@pytest.fixture(scope="module")
def lib():
    from event_representation_study_amd import build, _lib
    build.build()
    return _lib.load()


def _p(v):
    return ctypes.c_void_p(v)


def test_time_to_index_refuses_bad_arguments_before_any_launch(lib):
    from event_representation_study_amd._lib import EVREP_EINVAL, EVREP_OK, WINDOWS_MAX_QUERIES
    f = lib.evrep_time_to_index
    ok = (_p(256), 100, _p(512), 4, _p(1024), None)
    for i, bad in ((0, None), (0, _p(260)), (1, -1), (2, None), (2, _p(516)), (3, -1), (3, WINDOWS_MAX_QUERIES + 1), (4, None), (4, _p(1028))):
        args = list(ok)
        args[i] = bad
        assert f(*args) == EVREP_EINVAL, (i, bad)
    assert f(_p(256), 100, None, 0, None, None) == EVREP_OK        # no query: nothing to launch


def test_windows_gather_refuses_bad_arguments_before_any_launch(lib):
    from event_representation_study_amd._lib import (EVREP_EINVAL, EVREP_OK, REBASE_FIRST, REBASE_GIVEN, WINDOWS_MAX_B)
    f = lib.evrep_windows_gather
    #     x        y        t         p        n    i0        i1        offsets   B  mode          base_in events    base_out  status   stream
    ok = (_p(256), _p(512), _p(1024), _p(64), 100, _p(2048), _p(4096), _p(8192), 4, REBASE_FIRST, None, _p(16384), _p(32768), _p(65536), None)
    bad = [(0, None), (0, _p(257)), (1, None), (1, _p(513)), (2, None), (2, _p(1028)), (3, None), (4, -1),
           (5, None), (5, _p(2052)), (6, None), (6, _p(4100)), (7, None), (7, _p(8196)), (8, -1), (8, WINDOWS_MAX_B + 1),
           (9, 3), (9, -1), (9, REBASE_GIVEN), (10, _p(12)), (11, None), (11, _p(16392)), (12, None), (12, _p(32772)),
           (13, None), (13, _p(65538))]
    for i, v in bad:
        args = list(ok)
        args[i] = v
        assert f(*args) == EVREP_EINVAL, (i, v)
    args = list(ok)
    args[8] = 0
    assert f(*args) == EVREP_OK                                     # no window: nothing to launch


def test_device_recording_arguments_and_no_cpu_fallback():
    import torch
    from event_representation_study_amd import _lib
    from event_representation_study_amd.engine import EventBatch
    from event_representation_study_amd.recording import DeviceRecording
    x, y, t, p, W, H = golden_stream("short")
    with pytest.raises(ValueError):
        DeviceRecording(x, y, t, p, H, W, divider=2)
    with pytest.raises(ValueError):
        DeviceRecording(x.astype(np.int64) + 70000, y, t, p, H, W)          # x does not fit uint16
    with pytest.raises(ValueError):
        DeviceRecording(x, y, t, p.astype(np.int32) * 200, H, W)            # p does not fit int8
    with pytest.raises(ValueError):
        DeviceRecording(x, y, t.astype(np.float64), p, H, W)
    with pytest.raises(ValueError):
        DeviceRecording(x[:-1], y, t, p, H, W)
    assert "t_base" not in EventBatch.__dict__                              # a plain instance attribute, None by default
    if torch.cuda.is_available():
        return                      # a HIP device is visible: test_gpu_evl_windows.py covers the path
    with pytest.raises(_lib.EvrepError):
        DeviceRecording(x, y, t, p, H, W)
    with pytest.raises(_lib.EvrepError):
        DeviceRecording.from_h5(__file__.replace("test_evl_windows_cpu.py", "golden/h5/events_evlicious_blosc.h5"))


def test_tree_writer_round_trips_a_gen1_shaped_container(tmp_path):
    """h5lite.write_tree_file: nested old-style groups of contiguous datasets, scalars included, read back by h5lite.File and cut
    by Gen1H5Events as the committed h5py-written container is."""
    from event_representation_study_amd import h5lite
    from event_representation_study_amd.gen1_h5 import Gen1H5Events
    rng = np.random.default_rng(0)
    tree = {}
    for name, n in (("rec_b", 900), ("rec_a", 2000)):
        t = np.sort(rng.integers(0, 10 ** 6, n)).astype(np.int64) + 3_000_000_000
        tree[name] = {"events": {"x": rng.integers(0, 304, n).astype("u2"), "y": rng.integers(0, 240, n).astype("u2"), "t": t,
                                 "p": rng.integers(0, 2, n).astype("i1"), "height": np.array(240, "i4"), "width": np.array(304, "i4")},
                      "bbox": {"event_idx": np.array([150, 700, n], np.int64), "t_unique": t[[149, 699, n - 1]]}}
    path = str(tmp_path / "tree.h5")
    h5lite.write_tree_file(path, tree)

    def check(group, want):
        assert sorted(group.keys()) == sorted(want)
        for k, v in want.items():
            if isinstance(v, dict):
                check(group[k], v)
            else:
                assert_same(group[k][()], v, k)
    with h5lite.File(path) as f:
        check(f, tree)
    d = Gen1H5Events(path, num_events=300)
    assert len(d) == 6 and (d.height, d.width) == (240, 304) and d.locate(3) == (0, "rec_b")
    e = tree["rec_a"]["events"]
    w = d.window(1)
    assert_same(w, np.stack([e["x"][400:700], e["y"][400:700], e["t"][400:700] - e["t"][400], e["p"][400:700]], axis=1).astype(np.int32), "window")
    assert len(d.window(0)) == 150
    with pytest.raises(ValueError):
        h5lite.write_tree_file(path, {str(i): np.zeros(1) for i in range(9)})
