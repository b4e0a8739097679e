"""Seeded windows at the edges of the int32 time axis, shared by tests/golden/make_golden_time_edges.py (which pins the
reference's answers on them in time_edges.npz) and tests/test_gpu_time_edges.py (which regenerates them on the GPU box,
where the golden file's generator cannot run).  Every window is an (n, 4) int32 array of [x, y, t, p] rows.

edge_windows(): 40 x 30 sensor, both polarity encodings
  hi      ascending, ends exactly at INT32_MAX, the last 7 events tied there (INT32_MAX is the binning pass's padding)
  lo      ascending, starts exactly at INT32_MIN (INT32_MIN is the builders' "never written" timestamp)
  cross0  negative to positive times
  wide    INT32_MIN + 1 ... INT32_MAX: t_last - t0 does not fit in int32 (numpy's int32 arithmetic wraps)
  wrap    an int64 recording that straddles 2^31, cast to int32 as gen1_2yolo.py:567-571 does: +2^31 - 1 -> -2^31
  flat    all timestamps equal
  two     exactly two distinct timestamps
ts_tau_windows(tau): 20 x 15 sensor, time-surface windows whose spans (in tau) land on both sides of the factorised form's
  600-tau switch, the 708-tau end of the normal float64 range and the 745-tau underflow; "abs*" windows put the cut times
  themselves 695-750 tau after 0, where the untouched pixels' background exp((-(3 tau + 1) - t_cut) / tau) underflows;
  "front719.9" packs 40 % of a 719.9-tau window into its first 3 tau.
"""
import numpy as np

from event_representation_study_amd.synthetic import make_events

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
EDGE_W, EDGE_H, EDGE_N = 40, 30, 2000
TS_W, TS_H, TS_N = 20, 15, 1500
TS_SPANS = (590, 690, 705, 715, 719.9, 725, 760, 4400, 4600)
TS_ABS = ((695, 20), (705, 30), (690, 60))        # (first event, span), in tau
TAUS = (1000, 50000)
SLICES = (6, 8)


def _with_t(ev, t):
    ev = ev.copy()
    ev[:, 2] = np.asarray(t, dtype=np.int64).astype(np.int32)
    return ev


def _sorted_t(rng, n, lo, hi):
    """n ascending int64 timestamps in [lo, hi], the first == lo and the last == hi."""
    t = np.sort(rng.integers(lo, hi, size=n, endpoint=True))
    t[0], t[-1] = lo, hi
    return t


def edge_windows():
    out = {}
    for i, name in enumerate(("hi", "lo", "cross0", "wide", "wrap", "flat", "two")):
        pol = ("pm1", "01")[i % 2]
        ev = make_events(EDGE_N, EDGE_W, EDGE_H, seed=900 + i, polarity=pol)
        rng = np.random.default_rng(950 + i)
        t = ev[:, 2].astype(np.int64)                     # 0 ... ~50 000, ascending
        if name == "hi":
            t = t - t[-1] + I32_MAX
            t[-7:] = I32_MAX
        elif name == "lo":
            t = t + I32_MIN
        elif name == "cross0":
            t = t - 25000
        elif name == "wide":
            t = _sorted_t(rng, EDGE_N, I32_MIN + 1, I32_MAX)
        elif name == "wrap":
            t = t + (1 << 31) - 20000                     # int64 times 2^31 - 20 000 ... 2^31 + ~30 000
        elif name == "flat":
            t = np.full(EDGE_N, 123456, np.int64)
        elif name == "two":
            t = np.where(np.arange(EDGE_N) < EDGE_N // 3, -7, 40000)
        out[name] = _with_t(ev, t)
    return out


def ts_tau_windows(tau):
    """name -> window for one tau: "s<span>" spans that many tau from t = 0, "abs<first>_<span>" starts <first> tau after 0."""
    out = {}
    for j, span in enumerate(TS_SPANS):
        ev = make_events(TS_N, TS_W, TS_H, seed=1000 + 37 * j + tau % 997, polarity=("pm1", "01")[j % 2])
        rng = np.random.default_rng(2000 + j + tau % 991)
        out["s%g" % span] = _with_t(ev, _sorted_t(rng, TS_N, 0, int(round(span * tau))))
    # 40 % of the events in the first 3 tau of a 719.9-tau window: the dispatcher's cuts keep the factorised form (the first cut
    # lies 599.9 tau before the last), while those events' E = exp((t - tref) / tau) lie deep in the subnormal range
    ev = make_events(TS_N, TS_W, TS_H, seed=1200 + tau % 997, polarity="pm1")
    rng = np.random.default_rng(2200 + tau % 991)
    nf = TS_N * 2 // 5
    t = np.sort(np.concatenate([rng.integers(0, 3 * tau, size=nf), rng.integers(3 * tau, 719.9 * tau, size=TS_N - nf)]))
    t[0], t[-1] = 0, int(round(719.9 * tau))
    out["front719.9"] = _with_t(ev, t)
    for j, (first, span) in enumerate(TS_ABS):
        ev = make_events(TS_N, TS_W, TS_H, seed=1100 + j + tau % 997, polarity=("01", "pm1")[j % 2])
        rng = np.random.default_rng(2100 + j + tau % 991)
        out["abs%d_%d" % (first, span)] = _with_t(ev, _sorted_t(rng, TS_N, first * tau, (first + span) * tau))
    return out
