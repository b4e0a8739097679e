"""The point clouds of the GWD harness otmi(events, rep, height, width, rep_size) restated in numpy ONE QUADRANT AT A TIME
(citations: representations/representation_search/compute_otmi.py of the reference, as in oracle/oracle.py).

oracle.otmi_point_clouds answers for a whole window and, like the reference, raises when a quadrant is vacant (min() of
nothing, :140-147; t[0] of nothing, :167).  The helpers here answer for a single quadrant and a chosen quadrant table, so
that a vacant quadrant's neighbours and a hand-made `quad` can be checked too.  tests/test_otmi_ref_cpu.py pins them to the
oracle wherever the oracle answers; tests/test_gpu_otmi_edges.py holds the device kernels to them.  Nothing here touches
a device.
"""
import numpy as np


def _members(ev, q, H, W):
    """Boolean mask of the events of quadrant q (0 left-top, 1 right-top, 2 left-bottom, 3 right-bottom) in the SENSOR
    frame, :97-132: closed at 0 and at width / 2 - 1 (true division) on the left / top, open there and closed at
    width - 1 on the right / bottom.  An event outside the frame is in no quadrant."""
    x, y = ev[:, 0].astype(np.int64), ev[:, 1].astype(np.int64)
    hx, hy = W / 2 - 1, H / 2 - 1
    in_x = ((x > hx) & (x <= W - 1)) if q & 1 else ((x >= 0) & (x <= hx))
    in_y = ((y > hy) & (y <= H - 1)) if q & 2 else ((y >= 0) & (y <= hy))
    return in_x & in_y


def quadrant_counts(ev, H, W):
    ev = np.asarray(ev)
    return [int(_members(ev, q, H, W).sum()) for q in range(4)]


def scored_quadrants(ev, H, W):
    """The three quadrants the harness scores, in slot order: all but the most populated one, FIRST maximum
    (shape_sizes.index(max(shape_sizes)), :134-135)."""
    counts = quadrant_counts(ev, H, W)
    skip = counts.index(max(counts))
    return [q for q in range(4) if q != skip]


def event_cloud(ev, q, H, W):
    """The (n, 4) float32 rows [x, y, t, p] of quadrant q, or None when the quadrant holds no event.
    Quadrants 1-3 are moved to their own minimum (:140-147); an integer tensor divided by a python int is float32 in torch,
    so each operand is rounded to float32 and each value is one float32 division (:164-169): x / ((W - 1) // 2),
    y / ((H - 1) // 2), (t - t[0]) / (t[-1] - t[0]) in ARRAY order, (p - min p) / (max p - min p); rows with
    x < (W - 1) // 2 and y < (H - 1) // 2 are kept (:170-173).  0 / 0 is NaN and a / 0 is an infinity, as there."""
    ev = np.asarray(ev)
    rows = ev[_members(ev, q, H, W)].astype(np.int64)
    if rows.shape[0] == 0:
        return None
    if q != 0:
        rows[:, 0] -= rows[:, 0].min()
        rows[:, 1] -= rows[:, 1].min()
    dx, dy = (W - 1) // 2, (H - 1) // 2
    f32 = np.float32
    t, p = rows[:, 2], rows[:, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        cols = [rows[:, 0].astype(f32) / f32(dx),
                rows[:, 1].astype(f32) / f32(dy),
                (t - t[0]).astype(f32) / f32(t[-1] - t[0]),
                (p - p.min()).astype(f32) / f32(p.max() - p.min())]
    keep = (rows[:, 0] < dx) & (rows[:, 1] < dy)
    return np.stack(cols, axis=-1)[keep]


def rep_box(S, q):
    """(y0, y1, x0, x1), inclusive, of the cut of an (S, S, C) letterboxed representation for quadrant q (:150-155,177-179):
    the bounds are 0, rep_size / 2 - 1 (true division) and rep_size - 1, indexed through int()."""
    half = S / 2 - 1
    x0, x1 = (int(half), S - 1) if q & 1 else (0, int(half) if q else S // 2 - 1)
    y0, y1 = (int(half), S - 1) if q & 2 else (0, int(half))
    return y0, y1, x0, x1


def rep_cloud(rep, q):
    """The (m, C + 2) float64 rows of the cut of quadrant q: the C channels, then row / (rows - 1) and column / (columns - 1)
    (:181-198), pixels in row-major order, those with sum |channels| > 0 kept (:200-202; a NaN channel makes the sum NaN,
    which is not > 0)."""
    rep = np.asarray(rep)
    y0, y1, x0, x1 = rep_box(rep.shape[0], q)
    cut = rep[y0: y1 + 1, x0: x1 + 1, :].astype(np.float64)
    nr, nc, C = cut.shape
    out = np.empty((nr, nc, C + 2), np.float64)
    out[..., :C] = cut
    out[..., C] = (np.arange(nr) / (nr - 1))[:, None]
    out[..., C + 1] = (np.arange(nc) / (nc - 1))[None, :]
    out = out.reshape(nr * nc, C + 2)
    with np.errstate(invalid="ignore", over="ignore"):
        keep = np.abs(out[:, :C]).sum(-1) > 0
    return out[keep]


def same_cloud(got, want):
    """None when the two arrays agree under the rule of the edge tests -- same shape and dtype, NaN in the same cells, every
    other cell equal BIT FOR BIT (so -0.0 is not +0.0 and the infinities keep their sign) -- else a description of the
    first difference."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return "shape / dtype %r %s vs %r %s" % (got.shape, got.dtype, want.shape, want.dtype)
    gn, wn = np.isnan(got), np.isnan(want)
    if not np.array_equal(gn, wn):
        i = np.argwhere(gn != wn)[0]
        return "NaN placement differs at %s: %r vs %r" % (tuple(i), got[tuple(i)], want[tuple(i)])
    u = "u%d" % got.itemsize
    bad = (got.view(u) != want.view(u)) & ~gn
    if bad.any():
        i = np.argwhere(bad)[0]
        return "%d cells differ, first at %s: %r vs %r" % (int(bad.sum()), tuple(i), got[tuple(i)], want[tuple(i)])
    return None
