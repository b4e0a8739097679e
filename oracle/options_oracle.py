"""Float64 numpy restatements of the builder OPTIONS the C oracle has no entry point for -- TEST INFRASTRUCTURE ONLY.

Each function is written from the reference's own statement (cited by file:line, relative to the reference tree) and is
pinned on the CPU by tests/test_options_oracle_cpu.py against goldens recorded from the reference and against the C
oracle wherever the two overlap.  Everything is vectorised over events (np.add.at, np.maximum.at, last write by event
index): a window of 40 000 events takes well under a second.

Outputs are channel-last, as the builders write them: (H, W, C).

`scale` is applied the way each kernel applies it (include/evrep.h says so at every entry point):
  time_surface   every surface value exp(.) * scale in float64, before the one rounding to the output type;
  tonic_voxel    the finished float64 sum of a (pixel, bin) cell times scale, at pixels that hold an event (an empty
                 pixel stays +0 whatever the sign of scale).
tore and voxel_tnorm take no scale.
"""
import math

import numpy as np

PS_ANY, PS_POS, PS_NEG = 0, 1, 2
PS_COUNT, PS_TMAX, PS_TMIN, PS_FLAG, PS_EXP, PS_SIGNED = 0, 1, 2, 3, 4, 5


def _last_write(size, cell, first_index):
    """Per cell, the index of the LAST event (array order) that writes it, -1 where none does."""
    last = np.full(size, -1, dtype=np.int64)
    np.maximum.at(last, cell, np.arange(first_index, first_index + cell.shape[0], dtype=np.int64))
    return last


def time_surface(ev, H, W, indices, tau, premap=1, times=None, scale=1.0):
    """ToTimesurface.__call__ + to_timesurface_numpy (representations/time_surface.py:25-74) -> (H, W, 2 * len(indices))
    float64, channel 2 * pos + p.

    The memory starts at -(3 * tau + 1) (:26-29).  The scan runs in ARRAY order (:66): event `index` writes
    memory[p, y, x] = t[index] (:67) BEFORE the test index == indices[pos] (:69); surface `pos` is then
    exp((memory - t[index]) / tau) (:70-71) and pos advances; the scan stops after the last cut (:73-74).  The test is
    an `if` against the CURRENT cut only, so a repeated or descending cut is never hit again and a cut outside [0, n)
    never is: that surface and every later one stay exactly 0.
    times: float64 times that replace the t column (:66-74 is dtype-agnostic).  premap bit 0: p -> int8((p + 1) / 2)
    first (gen1_transforms.py:70-72); without it p is the index itself (numpy wraps -1, -2)."""
    ev = np.asarray(ev)
    n = ev.shape[0]
    S = len(indices)
    x, y = ev[:, 0].astype(np.int64), ev[:, 1].astype(np.int64)
    p = ev[:, 3].astype(np.int64)
    if int(premap) & 1:
        p = np.trunc((p + 1) / 2.0).astype(np.int8).astype(np.int64)
    if n and (p.min() < -2 or p.max() >= 2 or x.min() < -W or x.max() >= W or y.min() < -H or y.max() >= H):
        raise IndexError("event outside the (2, H, W) memory")
    t = np.asarray(ev[:, 2] if times is None else times, dtype=np.float64)
    cell = ((p % 2) * H + (y % H)) * W + (x % W)
    mem = np.full(2 * H * W, -(tau * 3 + 1), dtype=np.float64)
    out = np.zeros((S, 2 * H * W), dtype=np.float64)
    done = 0                     # events [0, done) are in the memory
    for pos in range(S):
        c = int(indices[pos])
        if c < done or c >= n:   # the scan is already past it (repeat / descent), or never reaches it: nothing later fires
            break
        last = _last_write(2 * H * W, cell[done:c + 1], done)
        hit = last >= 0
        mem[hit] = t[last[hit]]
        done = c + 1
        out[pos] = np.exp((mem - t[c]) / tau) * scale
    return np.ascontiguousarray(out.reshape(S, 2, H, W).transpose(2, 3, 0, 1).reshape(H, W, 2 * S))


def tore(x, y, t, p, sample_time, k, frame):
    """events2ToreFeature(x, y, ts, pol, sampleTimes, k, frameSize) (representations/tore.py:6-83) for one sample time and
    float64 times -> (frame[0], frame[1], 2k) float32, positive FIFOs then negative ones.

    Events with ts < sample_time take part (:17), pol > 0 in the first half, pol <= 0 in the second (:19,34); the pixel is
    [int(y) - 1, int(x) - 1] (:25-32, numpy wraps an index below 0).  Per (pixel, polarity) a k-vector v of
    dt = sample_time - ts, +inf where missing; every event, in ARRAY order, replaces it by
    np.partition([dt] + v[:k-1], k - 1)[:k] (:23-27): dt enters, the LAST entry of v leaves.  Not-ascending timestamps:
    the rule include/evrep.h states at evrep_tore -- the partition of so short a vector comes back sorted (numpy >= 2.0 on
    AVX2+ hosts), so v stays ascending and the entry that leaves is its largest.  On ascending timestamps this is a k-deep
    FIFO, newest first.  The old FIFOs are +inf (:9-11,49-61).  Then float32 (:63-65): clamp to 5e8 (:74-75),
    log(v + 1) in float32, minus the float64 log(151) with one rounding back (numpy 2: float32 array -= float64 scalar),
    floor 0 (:76-78)."""
    x, y = np.trunc(np.asarray(x, dtype=np.float64)).astype(np.int64), np.trunc(np.asarray(y, dtype=np.float64)).astype(np.int64)
    t, p = np.asarray(t, dtype=np.float64), np.asarray(p)
    Hf, Wf = int(frame[0]), int(frame[1])
    T = float(sample_time)
    take = t < T
    r, c = y[take] - 1, x[take] - 1
    if r.size and (r.min() < -Hf or r.max() >= Hf or c.min() < -Wf or c.max() >= Wf):
        raise IndexError("event outside the frame")
    cell = ((r % Hf) * Wf + (c % Wf)) * 2 + (p[take] <= 0)
    dt = T - t[take]
    fifo = np.full((Hf * Wf * 2, k), np.inf, dtype=np.float64)
    # round j handles the j-th event (array order) of every (pixel, polarity) cell at once
    order = np.argsort(cell, kind="stable")
    cs, ds = cell[order], dt[order]
    start = np.flatnonzero(np.r_[True, cs[1:] != cs[:-1]]) if cs.size else np.zeros(0, np.int64)
    count = np.diff(np.r_[start, cs.size])
    j = 0
    while start.size:
        cells, d = cs[start + j], ds[start + j]
        v = np.concatenate([d[:, None], fifo[cells, :k - 1]], axis=1)
        v.sort(axis=1)
        fifo[cells] = v
        j += 1
        keep = count > j
        start, count = start[keep], count[keep]
    # the FIFO ages as float32, capped at 5e8 (an empty entry's +inf and a NaN take the cap too); the level of an age is its
    # float32 log(age + 1) above that of the 150 us floor, the difference formed in float64 and rounded once, never below 0
    cap = np.float32(500e6)
    age = fifo.reshape(Hf, Wf, 2 * k).astype(np.float32)
    age = np.where(np.isnan(age) | (age > cap), cap, age)
    level = np.log(age + np.float32(1.0)).astype(np.float64) - math.log(151.0)
    return np.maximum(level.astype(np.float32), np.float32(0.0))


def _touched(cell, size):
    m = np.zeros(size, dtype=bool)
    m[cell] = True
    return m


def tonic_voxel(ev, H, W, bins, scale=1.0):
    """tonic.transforms.ToVoxelGrid as gen1_transforms.py:22-25 consumes it, restated from tonic's published algorithm
    (tonic is absent: parity unpinned) -> (H, W, bins) float64.  ts = bins * (t - t[0]) / (t[-1] - t[0]); p == 0 counts as
    -1; tis = int(ts), dts = ts - tis; every event adds p * (1 - dts) to bin tis where tis < bins -- ALL of these first --
    then p * dts to bin tis + 1 where tis + 1 < bins.  A flat window divides by zero, as the reference does."""
    ev = np.asarray(ev).astype(np.int64)       # tonic's t column is int64: t[-1] - t[0] of an int32 window must not wrap
    T = int(bins)
    ref = np.zeros(T * H * W)
    ts = T * (ev[:, 2].astype(float) - ev[0, 2]) / (ev[-1, 2] - ev[0, 2])
    pol = np.where(ev[:, 3] == 0, -1, ev[:, 3]).astype(float)
    tis = ts.astype(int)
    dts = ts - tis
    base = ev[:, 0] + ev[:, 1] * W
    ok = tis < T
    np.add.at(ref, base[ok] + tis[ok] * W * H, (pol * (1.0 - dts))[ok])
    ok = (tis + 1) < T
    np.add.at(ref, base[ok] + (tis[ok] + 1) * W * H, (pol * dts)[ok])
    out = np.ascontiguousarray(np.moveaxis(ref.reshape(T, H, W), 0, -1))
    if scale != 1.0:
        m = _touched(base, H * W).reshape(H, W)
        out[m] = out[m] * scale
    return out


def voxel_tnorm(x, y, t, p, H, W, bins):
    """compute_repr(x, y, t, p, width, height, bins) (representations/representation_search/gromov_wasserstein.py:72-82)
    with the caller's own t -> (H, W, bins) float64.  An event sits at the fractional bin position (bins - 1) * t (:74) and
    feeds the two bins around it: the one its position truncates to (:75) and the next (:77), each with the share
    1 - |bin - position| times p, a bin at or beyond `bins` being left out (:78-79).  np.add.at runs once per side (:80):
    the lower bins of EVERY event are added first, in array order, then the upper bins -- the order that fixes every sum's
    rounding.  t in [0, 1]: a negative position would index from the end of the bin axis in the reference."""
    t = np.asarray(t, dtype=np.float64)
    polarity = np.asarray(p).astype(np.float64)
    place = t * (bins - 1)
    lower = np.trunc(place).astype(np.int64)
    if lower.size and lower.min() < 0:
        raise IndexError("bin position below 0")
    first_cell = (np.asarray(y, dtype=np.int64) * W + np.asarray(x, dtype=np.int64)) * bins
    flat = np.zeros(H * W * bins, dtype=np.float64)
    for side in (0, 1):
        k = lower + side
        inside = k < bins
        share = 1.0 - np.abs(k - place)
        np.add.at(flat, (first_cell + k)[inside], (share * polarity)[inside])
    return flat.reshape(H, W, bins)


def polstats(ev, tn, H, W, pol, stat, tau=0.3):
    """The 3 x 6 table include/evrep.h documents at evrep_polstats (n_imagenet/real_cnn_model/data/imagenet.py:169-511,
    841-871) -> (H, W, C) float32, channel c = stat[c] over the events of class pol[c] at each pixel.

    ev: rows [x, y, *, p], x and y truncated toward zero as .long() does (:187,200); tn: one float64 time per event.
    Classes: ANY every event, POS p > 0, NEG p < 0 (:176-177) -- an event with p == 0 belongs to ANY only.
    COUNT = bincount (:187-189); FLAG = count > 0 (:405-406); TMAX / TMIN = float32(max / min of the float64 times), 0
    where the class has no event at the pixel (scatter_max / scatter_min, :203-206,236-239); EXP = exp(-(1 - TMAX) / tau)
    in float64 over the WHOLE frame with TMAX = 0 at empty pixels (:461-465), rounded once; SIGNED = count(p > 0) -
    count(p < 0), whatever the class (:866)."""
    ev = np.asarray(ev)
    tn = np.asarray(tn, dtype=np.float64)
    idx = ev[:, 0].astype(np.int64) + ev[:, 1].astype(np.int64) * W
    pv = ev[:, 3]
    member = {PS_ANY: np.ones(len(ev), dtype=bool), PS_POS: pv > 0, PS_NEG: pv < 0}
    cnt, mx, mn = {}, {}, {}
    for k, m in member.items():
        cnt[k] = np.bincount(idx[m], minlength=H * W)
        hi = np.full(H * W, -np.inf)
        lo = np.full(H * W, np.inf)
        np.maximum.at(hi, idx[m], tn[m])
        np.minimum.at(lo, idx[m], tn[m])
        mx[k] = np.where(cnt[k] > 0, hi, 0.0)
        mn[k] = np.where(cnt[k] > 0, lo, 0.0)
    out = np.empty((H * W, len(pol)), dtype=np.float32)
    for c, (k, st) in enumerate(zip(pol, stat)):
        k, st = int(k), int(st)
        if st == PS_COUNT:
            v = cnt[k]
        elif st == PS_TMAX:
            v = mx[k]
        elif st == PS_TMIN:
            v = mn[k]
        elif st == PS_FLAG:
            v = cnt[k] > 0
        elif st == PS_EXP:
            v = np.exp(-(1 - mx[k]) / tau)
        elif st == PS_SIGNED:
            v = cnt[PS_POS].astype(np.float32) - cnt[PS_NEG].astype(np.float32)
        else:
            raise ValueError(st)
        out[:, c] = v
    return out.reshape(H, W, len(pol))
