"""CPU: the study's representations on N-ImageNet batches, the parts that need no device.

study_rows_host (event_representation_study_amd/n_imagenet_front.py), the numpy restatement of evrep_nimg_study_rows, against
the statements of the reference it restates, written out here on float64 rows:

    MixedDensityEventStack.stack (mixed_density_event_stack.py:26-33)    t.astype(np.int64), then t - t.min()
    reshape_then_tore + events2ToreFeature (imagenet.py:1098-1099, tore.py:29-33)    x - min(x) + 1, then int()
    EventStack.pre_stack (event_stack.py:34)                             t.astype(np.int64) <= t[-1]

then the C ABI without a launch (symbols, argument errors, scratch sizes), study_device's name handling, and the new golden
tied to this package's host front end under the recorded parameters.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from conftest import assert_bit_equal, load_golden

_G = load_golden("nimg_study")
CASES = json.loads(str(_G["manifest"]))
T0 = 1.6e9


def rows_of(xy, p):
    r = np.zeros((len(xy), 4), np.int32)
    r[:, 0], r[:, 1], r[:, 3] = xy[:, 0].astype(np.int64), xy[:, 1].astype(np.int64), np.sign(p)
    return r


def statements(xy, t, p):
    """The reference's statements on one window's float64 fields -> (rebased int64 t, 0-based TORE x, y, past-half mask)."""
    ti = t.astype(np.int64)
    reb = ti - ti.min()
    x = xy[:, 0] - min(xy[:, 0]) + 1
    y = xy[:, 1] - min(xy[:, 1]) + 1
    tx = np.array([int(v) for v in x]) - 1
    ty = np.array([int(v) for v in y]) - 1
    return reb, tx, ty, ti <= t[-1]


def window(n, seed, t):
    rng = np.random.default_rng(seed)
    xy = np.stack([rng.random(n) * 32, rng.random(n) * 24], axis=1)
    return xy, np.asarray(t, np.float64), rng.choice([-1.0, 1.0], n)


def run(xy, t, p):
    from event_representation_study_amd import n_imagenet_front as nf
    rows = rows_of(xy, p)
    before = rows.copy(), t.copy(), xy.copy()
    out = nf.study_rows_host(rows, t, xy)
    assert np.array_equal(rows, before[0]) and np.array_equal(t, before[1], equal_nan=True) and np.array_equal(xy, before[2])
    for r in out[:3]:
        assert r.dtype == np.int32 and r.shape == rows.shape
    return rows, out


def check_statements(xy, t, p, st_want, marker_sign=1):
    rows, (mdes, stack, tore, t_last, st) = run(xy, t, p)
    reb, tx, ty, past = statements(xy, t, p)
    n = len(t)
    assert int(st) == st_want, (int(st), st_want)
    assert np.array_equal(mdes[:, [0, 1, 3]], rows[:, [0, 1, 3]]) and np.array_equal(mdes[:, 2], reb)
    assert np.array_equal(stack[:, :2], rows[:, :2]) and not stack[:, 2].any() and np.array_equal(stack[:, 3], np.where(p > 0, 1, -1))
    assert np.array_equal(tore[:, 0], tx) and np.array_equal(tore[:, 1], ty) and np.array_equal(tore[:, 3], rows[:, 3])
    assert np.array_equal(tore[:, 2], marker_sign * np.arange(n))
    assert t_last == t[-1]
    return mdes, stack, tore, past


def test_times_that_straddle_one_whole_second():
    from event_representation_study_amd import _lib
    n = 300
    xy, t, p = window(n, 1, T0 + np.linspace(0.98, 1.03, n))
    mdes, _, _, past = check_statements(xy, t, p, 0)
    assert set(mdes[:, 2].tolist()) == {0, 1} and past.all()
    assert _lib.STUDY_FLAT == 8


def test_times_inside_one_second_are_flat():
    from event_representation_study_amd import _lib
    xy, t, p = window(200, 2, T0 + np.linspace(0.10, 0.15, 200))
    mdes, _, _, past = check_statements(xy, t, p, _lib.STUDY_FLAT)
    assert not mdes[:, 2].any() and past.all()


def test_time_flipped_window():
    """base_augment's time flip: t' = T - t, descending rows reversed, so t' ascends from 0 and lies inside one second."""
    from event_representation_study_amd import _lib, n_imagenet_front as nf
    n = 150
    xy, t, p = window(n, 3, T0 + np.linspace(0.98, 1.03, n))
    ev = nf.time_flipped(torch.from_numpy(np.column_stack([xy, t, p]))).numpy()
    assert ev[0, 2] == 0.0 and (np.diff(ev[:, 2]) >= 0).all()
    check_statements(np.ascontiguousarray(ev[:, :2]), np.ascontiguousarray(ev[:, 2]), np.ascontiguousarray(ev[:, 3]), _lib.STUDY_FLAT)


def test_coordinate_minimum_in_the_last_row():
    n = 100
    xy, t, p = window(n, 4, T0 + np.linspace(0.98, 1.03, n))
    xy[:-1] += 3.0
    xy[-1] = (0.25, 0.75)
    _, _, tore, _ = check_statements(xy, t, p, 0)
    assert tore[-1, 0] == 0 and tore[-1, 1] == 0 and tore[:-1, 0].min() >= 2


def test_one_row():
    from event_representation_study_amd import _lib
    xy, t, p = window(1, 5, [T0 + 0.5])
    _, _, tore, _ = check_statements(xy, t, p, _lib.STUDY_FLAT)
    assert tore[0, :3].tolist() == [0, 0, 0]


def test_shifted_value_truncates_differently_from_the_shifted_truncated_value():
    """x = 31.85 with min 0.35: int(31.85 - 0.35 + 1) - 1 = 31, where the truncated coordinates give 31 - 0 = 31 but
    x = 31.25 with min 0.35 gives int(31.9) - 1 = 30 against 31 - 0 = 31: the float64 xy decide, not the int32 rows."""
    xy = np.array([[31.85, 0.35], [0.35, 23.9], [31.25, 0.95], [5.0, 5.0]])
    t = T0 + np.array([0.98, 0.99, 1.0, 1.03])
    p = np.array([1.0, -1.0, -1.0, 1.0])
    _, _, tore, _ = check_statements(xy, t, p, 0)
    assert tore[:, 0].tolist() == [31, 0, 30, 4] and tore[:, 1].tolist() == [0, 23, 0, 4]
    trunc = xy.astype(np.int64) - xy.astype(np.int64).min(axis=0)
    assert trunc[2, 0] == 31 != tore[2, 0]
    # every step rounds once: (x - xmin) + 1.0, never x - (xmin - 1.0)
    xy = np.array([[0.1, 0.0], [0.7 + 2.0 ** -52, 0.0], [1.1 - 2.0 ** -53, 0.0]])
    check_statements(xy, T0 + np.array([0.1, 0.2, 0.3]), np.ones(3), 8)


def test_descending_window_is_future():
    from event_representation_study_amd import _lib
    n = 120
    xy, t, p = window(n, 6, T0 + np.linspace(3.5, 0.2, n))
    rows, (mdes, stack, tore, t_last, st) = run(xy, t, p)
    reb, tx, ty, past = statements(xy, t, p)
    assert int(st) == _lib.STUDY_FUTURE | _lib.STUDY_UNORDERED and not past.all()
    assert np.array_equal(mdes[:, 2], reb) and np.array_equal(tore[:, 0], tx) and np.array_equal(tore[:, 1], ty)
    assert np.array_equal(tore[:, 2], -np.arange(n))          # events2ToreFeature's marker for times that do not ascend
    # negative times: trunc(-0.5) = 0 lies behind t[-1] = -0.5
    xy, t, p = window(3, 7, [-2.5, -1.5, -0.5])
    assert int(run(xy, t, p)[1][4]) == _lib.STUDY_FUTURE
    # a dip inside one whole second: unordered, yet every row in the past half
    xy, t, p = window(3, 8, [T0 + 0.2, T0 + 0.1, T0 + 0.3])
    assert int(run(xy, t, p)[1][4]) == _lib.STUDY_UNORDERED | _lib.STUDY_FLAT


def test_times_that_cannot_be_cast():
    from event_representation_study_amd import _lib
    for bad in (np.nan, 1e19, -1e19, np.inf, 2.0 ** 63):
        xy, t, p = window(4, 9, [T0 + 0.1, bad, T0 + 0.2, T0 + 1.3])
        rows, (mdes, stack, tore, t_last, st) = run(xy, t, p)
        assert int(st) & _lib.STUDY_T_RANGE and not int(st) & _lib.STUDY_FLAT, bad
        assert mdes[:, 2].tolist() == [0, 0, 0, 1], bad          # the bad row takes no part in the minimum; its column is 0
    xy, t, p = window(2, 10, [0.0, 2.0 ** 31])                # whole seconds that span more than int32 holds
    st = int(run(xy, t, p)[1][4])
    assert st == _lib.STUDY_T_RANGE
    xy, t, p = window(2, 10, [1.0, 2.0 ** 31])                # 2^31 - 1: the largest span that fits
    rows, out = run(xy, t, p)
    assert int(out[4]) == 0 and out[0][:, 2].tolist() == [0, 2 ** 31 - 1]
    xy, t, p = window(2, 11, [np.nan, np.nan])
    rows, out = run(xy, t, p)
    assert int(out[4]) == _lib.STUDY_T_RANGE | _lib.STUDY_UNORDERED and not out[0][:, 2].any()


def test_empty_window():
    from event_representation_study_amd import _lib, n_imagenet_front as nf
    mdes, stack, tore, t_last, st = nf.study_rows_host(np.zeros((0, 4), np.int32), np.zeros(0), np.zeros((0, 2)))
    assert int(st) == _lib.STUDY_EMPTY and t_last == 0.0 and mdes.shape == stack.shape == tore.shape == (0, 4)
    with pytest.raises(ValueError):
        nf.study_rows_host(np.zeros((2, 4), np.int32), np.zeros(3), np.zeros((2, 2)))


# ------------------------------------------------------------------------------------------------ the C ABI, without a device
@pytest.fixture(scope="module")
def lib():
    from event_representation_study_amd import build, _lib
    build.build()
    return _lib.load()


def test_symbols_are_declared_bound_and_exported(lib):
    from event_representation_study_amd import _lib
    i32, i64, vp, u32 = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_uint32
    want = {"evrep_nimg_study_rows_scratch_bytes": (ctypes.c_size_t, [i32, i64]),
            "evrep_nimg_study_rows": (ctypes.c_int, [vp, vp, vp, vp, i32, i32, i32, u32, vp, vp, vp, vp, vp, vp, vp])}
    header = open(os.path.join(_lib._PKG, "..", "include", "evrep.h")).read()
    for name, (res, args) in want.items():
        assert _lib.SYMBOLS[name] == (res, args), name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
        assert name + "(" in header
    assert lib.evrep_abi_version() == 3 == _lib.ABI_VERSION
    for name, value in (("MDES", 1), ("STACK", 2), ("TORE", 4)):
        assert getattr(_lib, "STUDY_" + name) == value and "#define EVREP_STUDY_%s %du" % (name, value) in header
    for name, value in (("EMPTY", 1), ("FUTURE", 2), ("T_RANGE", 4), ("FLAT", 8), ("UNORDERED", 16)):
        assert getattr(_lib, "STUDY_" + name) == value and "#define EVREP_STUDY_%s %du" % (name, value) in header


def test_argument_errors_come_back_before_any_launch(lib):
    from event_representation_study_amd._lib import EVREP_EINVAL
    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4104)      # never dereferenced on the host
    ALL = 7
    #     rows t  xy off B  H   W   want mdes stack tore st_times status scratch stream
    ok = [p, p, p, p, 1, 24, 32, ALL, p, p, p, p, p, p, None]
    for pos in (0, 1, 2, 3, 8, 9, 10, 11, 12, 13):             # NULL inputs, wanted outputs, status, scratch
        args = list(ok)
        args[pos] = None
        assert lib.evrep_nimg_study_rows(*args) == EVREP_EINVAL, pos
    for pos in (0, 2, 8, 9, 10, 13):                           # 16-byte alignment
        args = list(ok)
        args[pos] = odd
        assert lib.evrep_nimg_study_rows(*args) == EVREP_EINVAL, pos
    for B in (-1, (1 << 24) + 1):
        assert lib.evrep_nimg_study_rows(p, p, p, p, B, 24, 32, ALL, p, p, p, p, p, p, None) == EVREP_EINVAL
    for want in (0, 8, 15):
        assert lib.evrep_nimg_study_rows(p, p, p, p, 1, 24, 32, want, p, p, p, p, p, p, None) == EVREP_EINVAL
    for H, W in ((0, 32), (24, 0), (4097, 32), (24, -1)):
        assert lib.evrep_nimg_study_rows(p, p, p, p, 1, H, W, ALL, p, p, p, p, p, p, None) == EVREP_EINVAL
    # a wanted output that is NULL, one set at a time; an unwanted one may be NULL (B = 0: accepted, nothing is launched)
    for bit, pos in ((1, 8), (2, 9), (4, 10)):
        args = [p, p, p, p, 1, 24, 32, bit, None, None, None, p, p, p, None]
        assert lib.evrep_nimg_study_rows(*args) == EVREP_EINVAL, bit
        args[4], args[pos] = 0, p
        if bit != 4:
            args[2] = args[11] = None                          # xy and the sample times go with TORE
        assert lib.evrep_nimg_study_rows(*args) == 0, bit
    assert lib.evrep_nimg_study_rows(p, p, None, p, 1, 24, 32, 4, None, None, p, p, p, p, None) == EVREP_EINVAL   # TORE without xy
    assert lib.evrep_nimg_study_rows(p, p, p, p, 1, 24, 32, 4, None, None, p, None, p, p, None) == EVREP_EINVAL  # ... sample times


def test_scratch_size(lib):
    f = lib.evrep_nimg_study_rows_scratch_bytes
    assert f(1, 0) > 0
    sizes = [f(B, 1000) for B in (1, 2, 7, 256, 4096, 1 << 20)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1]
    by_total = [f(8, n) for n in (0, 1, 1000, 10 ** 6, 10 ** 10)]
    assert all(a <= b for a, b in zip(by_total, by_total[1:]))
    assert f(256, 1 << 23) >= 256 * 40                         # four minima and the flags per window
    assert f(0, 10) == 0 and f(-1, 10) == 0 and f(1, -1) == 0 and f((1 << 24) + 1, 10) == 0


def test_study_device_names_need_no_device():
    from event_representation_study_amd import n_imagenet_acc as ni, n_imagenet_front as nf
    with pytest.raises(KeyError):
        nf.study_device("acc_all", None)
    with pytest.raises(KeyError):
        ni.study_batch("acc_sort", [])
    with pytest.raises(IndexError) as a:
        nf.study_device("time_surface", None)
    with pytest.raises(IndexError) as b:
        ni.reshape_then_time_surface(None)
    assert str(a.value) == str(b.value)
    with pytest.raises(KeyError):
        nf.accumulate_device("optimized", None)                # accumulate_device keeps to SPECS
    assert ni.STUDY_NAMES == ("optimized", "event_stack", "tore")


def test_status_words_become_the_wrappers_exceptions():
    from event_representation_study_amd import _lib, n_imagenet_acc as ni
    E, F, R, L, U = _lib.STUDY_EMPTY, _lib.STUDY_FUTURE, _lib.STUDY_T_RANGE, _lib.STUDY_FLAT, _lib.STUDY_UNORDERED
    ok = np.array([0, L, U, L | U], np.uint32)
    for name in ni.STUDY_NAMES:
        assert ni.study_status_error(name, ok) is None
        err = ni.study_status_error(name, np.array([0, R, E, E], np.uint32))
        assert isinstance(err, IndexError if name == "event_stack" else ValueError) and "sample 2" in str(err)
        err = ni.study_status_error(name, np.array([L, 0, F | U, R], np.uint32))
        assert isinstance(err, ValueError) and "sample 3" in str(err)
    err = ni.study_status_error("event_stack", np.array([L, F | U, F], np.uint32))
    assert isinstance(err, ValueError) and "sample 1" in str(err) and "reshape_then_event_stack" in str(err)
    assert ni.study_status_error("optimized", np.array([F | U], np.uint32)) is None      # ERGO-12 and TORE take any order
    assert ni.study_status_error("tore", np.array([F | U], np.uint32)) is None


# ------------------------------------------------------------------------------------------------ the golden and the host front end
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_golden_tensors_equal_the_host_front_end(case):
    """The augmented tensors the reference left equal host_rows under the recorded parameters: the new fixture stands on the
    same front-end semantics as nimg_front.npz."""
    from event_representation_study_amd import _lib, n_imagenet_front as nf
    cols = tuple(_G["stream%d.%s" % (case["stream"], k)] for k in "xytp")
    tf, xf, xs, ys, s0, s1 = (int(v) for v in _G[case["name"] + ".draw"])
    par = np.zeros(1, nf.PARAMS_DTYPE)
    par["s0"], par["s1"], par["t_lo"], par["t_hi"] = s0, s1, -np.inf, np.inf
    par["x_shift"], par["y_shift"] = xs, ys
    par["flags"] = (_lib.AUG_TIME_FLIP if tf else 0) | (_lib.AUG_X_FLIP if xf else 0)
    (sh, sw), (ih, iw) = case["sensor"], case["image"]
    got = nf.host_rows(*cols, par[0], sx=iw / sw, sy=ih / sh, train=case["mode"] == "train", resolution=(ih, iw)).numpy()
    assert_bit_equal(got, _G[case["name"] + ".out"], case["name"])
    for name in ("optimized", "event_stack", "tore"):
        img = _G["%s.%s" % (case["name"], name)]
        assert img.dtype == np.float32 and img.shape == (12, ih, iw)
    # the rows of the device form, from the reference's tensor: in frame, no refusal
    ev = _G[case["name"] + ".out"]
    mdes, stack, tore, t_last, st = nf.study_rows_host(rows_of(ev[:, :2], ev[:, 3]), ev[:, 2], np.ascontiguousarray(ev[:, :2]))
    assert not int(st) & (_lib.STUDY_EMPTY | _lib.STUDY_FUTURE | _lib.STUDY_T_RANGE | _lib.STUDY_UNORDERED)
    assert tore[:, 0].min() == 0 and tore[:, 1].min() == 0 and tore[:, 0].max() < iw and tore[:, 1].max() < ih and t_last == ev[-1, 2]
