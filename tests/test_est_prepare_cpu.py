"""CPU-only: evrep_est_prepare's argument checks (no kernel is launched), and the input streams of tests/test_gpu_est_prepare.py:
each "good" stream is accepted by the host route's checks, restated here, and really contains what its name claims, so that
the GPU tests cannot pass vacuously.  Expected values are those of test_est_cpu.wrapper_restated_inputs."""
import ctypes

import numpy as np
import pytest

from test_est_cpu import WRAPPER_KINDS, wrapper_events, wrapper_restated_inputs

H, W = 17, 65
WAVE, GROUP = 64, 256
EDGE_LENGTHS = (1, 63, 64, 65, 255, 256, 257, 1025)          # the lengths of the issue, in its order
EDGE_LENGTHS_ON_EDGES = (255, 1, 257, 63, 64, 65, 256, 1025)  # the same lengths, ordered so that boundaries sit at lanes 63 / 0 / 1


def item(n, b, rng, tlo=1, thi=40000, sort=True):
    e = np.zeros((n, 5), dtype=np.float32)
    e[:, 0], e[:, 1] = rng.integers(0, W, size=n), rng.integers(0, H, size=n)
    t = rng.integers(tlo, thi, size=n)
    e[:, 2] = np.sort(t) if sort else t
    e[:, 3], e[:, 4] = rng.integers(0, 2, size=n), b
    return e


def good_stream(name, seed=0):
    """-> (events (N, 5) float32, batch_size or None)"""
    rng = np.random.default_rng(900 + seed)
    if name in WRAPPER_KINDS:
        return wrapper_events(name, H, W), None
    if name == "edge_lengths":
        return np.concatenate([item(n, b, rng) for b, n in enumerate(EDGE_LENGTHS)]), None
    if name == "edge_lengths_on_edges":
        return np.concatenate([item(n, b, rng) for b, n in enumerate(EDGE_LENGTHS_ON_EDGES)]), None
    if name == "tiny_items":                       # 40 items of 1-3 events: several boundaries inside one wave
        return np.concatenate([item(int(rng.integers(1, 4)), b, rng) for b in range(40)]), None
    if name == "leading_empty":                    # b starts at 2
        return np.concatenate([item(700, 2, rng), item(900, 3, rng)]), None
    if name == "jump_0_7":                         # six consecutive empty items
        return np.concatenate([item(500, 0, rng), item(800, 7, rng)]), None
    if name == "trailing_empty":                   # explicit batch_size = 1 + last + 3
        return np.concatenate([item(600, 0, rng), item(400, 1, rng)]), 5
    if name == "unsorted_max_in_first_wave":       # item 1 spans five waves; its maximum is its 6th row
        e = item(320, 1, rng, sort=False)
        e[5, 2] = 50000.0
        return np.concatenate([item(64, 0, rng), e, item(100, 2, rng)]), None
    if name == "all_negative":
        e = item(300, 1, rng)
        e[:, 2] = -e[::-1, 2].copy()                # ascending, all below zero
        return np.concatenate([item(200, 0, rng), e, item(200, 2, rng)]), None
    if name == "inf":
        e = item(300, 1, rng)
        e[-1, 2] = np.inf
        return np.concatenate([item(200, 0, rng), e, item(200, 2, rng)]), None
    if name == "nan":
        e = item(300, 1, rng)
        e[70, 2] = np.nan
        return np.concatenate([item(200, 0, rng), e, item(200, 2, rng)]), None
    if name == "subnormal":                        # subnormal quotients from normal times, and subnormal times themselves
        e = item(200, 1, rng)
        e[:, 2] = (np.arange(1, 201) * 3 + 1).astype(np.float32) * np.float32(2.0 ** -125)
        e[-1, 2] = np.float32(2.0 ** 20) * np.float32(1.5)
        f = item(100, 2, rng)
        f[:, 2] = (np.arange(1, 101) * 7).astype(np.float32) * np.float32(2.0 ** -149)
        f[-1, 2] = 3.0
        return np.concatenate([item(150, 0, rng), e, f]), None
    if name == "truncation":
        e = item(400, 0, rng)
        e[0, 0], e[1, 0], e[2, 1], e[3, 1] = 3.7, -0.5, 5.9, -0.25
        e[4, 0], e[5, 1] = W - 0.001, H - 0.5
        return e, None
    raise ValueError(name)


GOOD = tuple(WRAPPER_KINDS) + ("edge_lengths", "edge_lengths_on_edges", "tiny_items", "leading_empty", "jump_0_7", "trailing_empty",
                               "unsorted_max_in_first_wave", "all_negative", "inf", "nan", "subnormal", "truncation")


def restated(ev, batch_size=None):
    """(rows int32 (N, 4), offsets int64 (B + 1,), tnorm float32 (N,)) of wrapper_restated_inputs; an explicit batch_size beyond
    1 + last b appends empty items"""
    rows, offs, tn = wrapper_restated_inputs(ev, H, W)
    if batch_size is not None:
        assert batch_size + 1 >= len(offs)
        offs = np.concatenate([offs, np.full(batch_size + 1 - len(offs), offs[-1], dtype=np.int64)])
    return rows, offs, tn


def host_route_accepts(ev, batch_size=None):
    """the checks of est._prepare_events_host, restated: grouped b, p in {0, 1}, truncated coordinates inside the frame"""
    b, p = ev[:, 4], ev[:, 3]
    nb = int(1 + ev[-1, 4]) if batch_size is None else batch_size
    x, y = ev[:, 0].astype(np.int64), ev[:, 1].astype(np.int64)
    return bool(ev.ndim == 2 and ev.shape[1] == 5 and len(ev) > 0 and (b[1:] >= b[:-1]).all() and ((p == 0) | (p == 1)).all()
                and (b == np.floor(b)).all() and b.min() >= 0 and b.max() < nb
                and x.min() >= 0 and x.max() < W and y.min() >= 0 and y.max() < H)


def bad_stream(name, seed=0):
    """-> (events, batch_size or None, the exception prepare_events_device raises)"""
    rng = np.random.default_rng(950 + seed)
    ev = np.concatenate([item(300, 0, rng), item(300, 1, rng)])
    if name == "descending":
        ev[:300, 4], ev[300:, 4] = 1, 0
        return ev, None, NotImplementedError
    if name == "p_2":
        ev[10, 3] = 2
        return ev, None, ValueError
    if name == "p_half":
        ev[400, 3] = 0.5
        return ev, None, ValueError
    if name == "x_W":
        ev[20, 0] = W
        return ev, None, IndexError
    if name == "y_minus_1":
        ev[599, 1] = -1
        return ev, None, IndexError
    if name == "b_1_5":
        ev[300:, 4] = 1.5
        return ev, None, ValueError
    if name == "b_beyond_batch_size":
        return ev, 1, ValueError
    raise ValueError(name)


BAD = ("descending", "p_2", "p_half", "x_W", "y_minus_1", "b_1_5", "b_beyond_batch_size")


def nan_equal_bits(got, want, what=""):
    """bit equality of two float32 arrays as uint32 views, NaNs compared by position (their sign and payload are not defined
    by IEEE 754 for 0/0 or inf/inf, and differ between x86 and the device)"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape, got.dtype, want.dtype)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "%s: NaN positions differ at %r" % (what, np.flatnonzero(gn != wn)[:8])
    gb, wb = got.view(np.uint32)[~gn], want.view(np.uint32)[~wn]
    bad = np.flatnonzero(gb != wb)
    assert bad.size == 0, "%s: %d mismatches, first %r vs %r" % (what, bad.size, got[~gn][bad[0]], want[~wn][bad[0]])


# ---------------------------------------------------------------------------------------------------------------------
# the generators
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOOD)
def test_good_streams_are_accepted_and_restated(name):
    ev, bs = good_stream(name)
    assert ev.dtype == np.float32 and host_route_accepts(ev, bs)
    with np.errstate(all="ignore"):
        rows, offs, tn = restated(ev, bs)
    nb = bs if bs is not None else int(1 + ev[-1, 4])
    assert offs.shape == (nb + 1,) and offs[0] == 0 and offs[-1] == len(ev) and (np.diff(offs) >= 0).all()
    assert rows.dtype == np.int32 and (rows[:, 2] == 0).all() and tn.dtype == np.float32
    assert len(ev) <= 6000                                                       # a few thousand events


def _boundaries(ev):
    return np.flatnonzero(ev[1:, 4] != ev[:-1, 4]) + 1


def test_streams_contain_what_they_claim():
    ev, _ = good_stream("edge_lengths")
    assert tuple(np.diff(restated(ev)[1])) == EDGE_LENGTHS
    ev, _ = good_stream("edge_lengths_on_edges")
    assert sorted(np.diff(restated(ev)[1])) == sorted(EDGE_LENGTHS)
    bd = _boundaries(ev)
    assert {63, 0, 1} <= set(bd % WAVE) and {GROUP - 1, 0, 1} <= set(bd % GROUP) and len(ev) > 4 * GROUP   # more than one workgroup
    ev, _ = good_stream("tiny_items")
    cnt = np.diff(restated(ev)[1])
    assert len(cnt) == 40 and cnt.min() >= 1 and cnt.max() <= 3 and {1, 2, 3} <= set(cnt)
    assert np.bincount(_boundaries(ev) // WAVE).max() >= 20                       # many boundaries inside one wave
    ev, _ = good_stream("leading_empty")
    assert tuple(np.diff(restated(ev)[1])) == (0, 0, 700, 900)
    ev, _ = good_stream("jump_0_7")
    assert tuple(np.diff(restated(ev)[1])) == (500, 0, 0, 0, 0, 0, 0, 800)
    ev, bs = good_stream("trailing_empty")
    assert bs == int(1 + ev[-1, 4]) + 3 and tuple(np.diff(restated(ev, bs)[1])) == (600, 400, 0, 0, 0)
    ev, _ = good_stream("unsorted_max_in_first_wave")
    _, offs, tn = restated(ev)
    s, e = offs[1], offs[2]
    t = ev[s:e, 2]
    assert e - s > 4 * WAVE and s % WAVE == 0 and (np.diff(t) < 0).any()
    assert np.argmax(t) == 5 and t[5] > t[-1] and tn[s + 5] == 1.0 and tn[s:e].max() == 1.0
    ev, _ = good_stream("all_negative")
    _, offs, tn = restated(ev)
    s, e = offs[1], offs[2]
    assert (ev[s:e, 2] < 0).all() and ev[s:e, 2].max() != ev[s, 2] and (tn[s:e] >= 1.0).all() and tn[s:e].max() > 2.0
    ev, _ = good_stream("inf")
    with np.errstate(all="ignore"):
        _, offs, tn = restated(ev)
    s, e = offs[1], offs[2]
    assert np.isinf(ev[s:e, 2]).sum() == 1 and np.isnan(tn[s:e]).sum() == 1 and (tn[s:e - 1] == 0).all() and not np.isnan(tn[:s]).any()
    ev, _ = good_stream("nan")
    with np.errstate(all="ignore"):
        _, offs, tn = restated(ev)
    s, e = offs[1], offs[2]
    assert np.isnan(ev[:, 2]).sum() == 1 and np.isnan(ev[s + 70, 2]) and np.isnan(tn[s:e]).all()
    assert not np.isnan(tn[:s]).any() and not np.isnan(tn[e:]).any()
    clean = ev.copy()
    clean[s + 70, 2] = clean[s + 69, 2]
    tc = restated(clean)[2]
    assert np.array_equal(tc[:s], tn[:s]) and np.array_equal(tc[e:], tn[e:])    # the neighbours do not see the NaN
    ev, _ = good_stream("subnormal")
    _, offs, tn = restated(ev)
    tiny = np.finfo(np.float32).tiny
    for k in (1, 2):
        q = tn[offs[k]:offs[k + 1] - 1]
        assert ((q > 0) & (q < tiny)).all() and len(np.unique(q)) > 50          # float32 subnormals, not flushed to zero
    assert (ev[offs[1]:offs[2], 2] >= tiny).all() and (ev[offs[2]:offs[3] - 1, 2] < tiny).all()
    q, t, m = tn[offs[1]:offs[2] - 1], ev[offs[1]:offs[2] - 1, 2], ev[offs[2] - 1, 2]
    assert (q.astype(np.float64) != t.astype(np.float64) / np.float64(m)).any()   # the division rounds: a flush or a truncation shows
    ev, _ = good_stream("truncation")
    rows = restated(ev)[0]
    assert (ev[0, 0], ev[1, 0]) == (np.float32(3.7), np.float32(-0.5)) and tuple(rows[:2, 0]) == (3, 0)
    assert tuple(rows[2:4, 1]) == (5, 0) and rows[4, 0] == W - 1 and rows[5, 1] == H - 1


def test_item_maximum_is_not_the_last_row_somewhere():
    """a kernel that took the last row of an item for its maximum must fail one of the streams"""
    hit = 0
    for name in ("unsorted_max_in_first_wave", "all_negative"):
        ev, _ = good_stream(name)
        offs = restated(ev)[1]
        hit += int(ev[offs[1]:offs[2], 2].max() != ev[offs[2] - 1, 2])
    assert hit >= 1


@pytest.mark.parametrize("name", BAD)
def test_bad_streams_are_refused_by_the_host_routes_checks(name):
    ev, bs, exc = bad_stream(name)
    assert not host_route_accepts(ev, bs) and issubclass(exc, Exception)
    good = np.concatenate([item(300, 0, np.random.default_rng(950)), item(300, 1, np.random.default_rng(951))])
    assert host_route_accepts(good)                                               # the stream the bad ones were made from


# ---------------------------------------------------------------------------------------------------------------------
# the entry points' host side
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from event_representation_study_amd import build, _lib
    build.build()
    return _lib.load()


def test_scratch_bytes(lib):
    f = lib.evrep_est_prepare_scratch_bytes
    for n, B in ((0, 4), (-1, 4), (100, 0), (100, -3), (100, 65536)):
        assert f(n, B) == 0
    sizes = [f(1000, B) for B in (1, 2, 63, 64, 65, 1000, 65535)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and sizes[-1] >= 4 * 65536
    assert f(1, 32) > 0 and f(1 << 40, 32) >= f(1, 32) >= 4 * 33


def test_prepare_refuses_bad_arguments_before_any_launch(lib):
    """every refusal returns before the first HIP call: this runs without a device"""
    from event_representation_study_amd._lib import EVREP_EINVAL
    p = ctypes.c_void_p
    good = dict(ev=p(4096), n=100, B=3, H=H, W=W, rows=p(8192), offs=p(16384), tn=p(32768), st=p(65536), scr=p(131072))

    def call(**kw):
        a = dict(good, **kw)
        return lib.evrep_est_prepare(a["ev"], a["n"], a["B"], a["H"], a["W"], a["rows"], a["offs"], a["tn"], a["st"], a["scr"], None)
    for key in ("ev", "rows", "offs", "tn", "st", "scr"):
        assert call(**{key: None}) == EVREP_EINVAL, key
    for kw in (dict(n=0), dict(n=-5), dict(B=0), dict(B=-1), dict(B=65536), dict(H=0), dict(H=4097), dict(W=0), dict(W=4097),
               dict(W=-1), dict(rows=p(8192 + 8)), dict(rows=p(8192 + 4)), dict(ev=p(4098)), dict(offs=p(16388))):
        assert call(**kw) == EVREP_EINVAL, kw
