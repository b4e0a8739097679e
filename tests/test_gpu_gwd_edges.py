"""Every form of the GWD tile kernel, single and batched, against the oracle's float64 closed form at its edges.

test_gpu_gwd_forms.py reaches five float32 and some split single-solve forms on uniform clouds at h = 0.7, and every batched
test of the suite runs split form <2, 6>.  This module holds the rest to `oracle.gwd` on the arrays the kernel gets, within
the project's budget |got - ref| <= 1e-5 * ref (bit-equality where stated):

A. one (ds, dt) per reachable form (four split, five float32) plus the dimension edges, each on one ragged pair list that
   reaches every branch of the tile epilogue (interior, one-sided, masked; diagonal and doubled off-diagonal tiles): single
   solves against the oracle, one batched call bit-equal to them, and once more with explicit row tables and caps no pair
   fills (tiles of the grid that no pair owns);
B. the workload's cloud shapes (binary and mostly-zero columns, duplicates, letterbox rows, constant columns, clusters,
   outliers) at three bandwidths; identical clouds cost exactly 0.0;
C. degenerate clouds (one point, all points equal): NaN as in the reference, alone and inside a batch whose other pairs are
   untouched;
D. translated clouds: the cost must not depend on where a cloud sits (the statistics take the variance about the cloud's
   first row, not from sum x^2 - (sum x)^2 / N).

The one-masked-tile pair of A is (3, 2), not the smallest pair (2, 2): two clouds of two points have the same kernel matrix
whatever their coordinates (sigma^2 = d^2 / 4, K_01 = exp(-2 / h^2) on both sides), so the (2, 2) cost is 0 and a relative
bound has nothing to hold.

Every case asserts np.isfinite(ref) and ref > 1e-4 before the relative bound.  Every test prints its largest relative error
(`pytest -s`); NOTES.md records them.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BUDGET = 1e-5


@pytest.fixture(scope="module")
def eng():
    from event_representation_study_amd import engine
    return engine


# ---- the dispatch of evrep_capi_gwd.hip (gwd_use_split / gwd_split_steps / gwd_steps), restated
def form(ds, dt):
    split = ds <= 15 and dt <= 15
    steps = (lambda d: 2 if 6 * d + 6 <= 32 else 6) if split else (lambda d: 3 if d + 2 <= 6 else (8 if d + 2 <= 16 else 17))
    return ("split" if split else "f32", steps(ds), steps(dt))


FORM_DIMS = [(4, 4), (4, 14), (14, 4), (14, 14),                       # split <2,2> <2,6> <6,2> <6,6>
             (4, 16), (14, 16), (16, 4), (16, 14), (16, 16)]           # float32 <3,17> <8,17> <17,3> <17,8> <17,17>
EDGE_DIMS = [(1, 1), (5, 4), (15, 15), (16, 15), (15, 16), (32, 32)]
REACHABLE = {("split", 2, 2), ("split", 2, 6), ("split", 6, 2), ("split", 6, 6),
             ("f32", 3, 17), ("f32", 8, 17), ("f32", 17, 3), ("f32", 17, 8), ("f32", 17, 17)}
# (n, m): one masked tile | one tile, one cloud full | one interior tile | three interior tiles, the off-diagonal one doubled |
# one-sided tiles only behind an interior one, no masked tile (2) | masked tiles on both clouds at different places (2) |
# masked first tile, then one-sided diagonal and off-diagonal tiles (2)
PAIRS = [(3, 2), (127, 128), (128, 128), (256, 256), (128, 256), (256, 128), (129, 257), (257, 129), (100, 384), (384, 100)]
CAP = 384


def test_the_parameter_list_reaches_all_nine_forms():
    assert {form(ds, dt) for ds, dt in FORM_DIMS} == REACHABLE
    assert len(FORM_DIMS) == len(REACHABLE)
    assert {form(ds, dt) for ds, dt in EDGE_DIMS} <= REACHABLE
    # the four float32 instantiations the dispatch cannot reach: a cloud of <= 14 dimensions beside another one is split
    assert all(form(ds, dt) in REACHABLE for ds in range(1, 33) for dt in range(1, 33))


def uniform_pair(rng, n, m, ds, dt):
    """The clouds of test_forms_against_oracle: uniform source, target columns scaled by linspace(1, 255, dt)."""
    return rng.random((n, ds)), rng.random((m, dt)) * np.linspace(1.0, 255.0, dt)


def single(eng, Xs, Xt, h=0.7):
    return float(eng.gwd_padded_l1(Xs, Xt, h).item())


def batch(eng, pairs, n_cap, m_cap, h=0.7, slot=None, reverse=False):
    """One gwd_padded_l1_batch call over `pairs` ([(Xs, Xt)]), clouds in slots of `slot` rows (default: the caps, so the
    implicit row table p * cap applies).  Rows no cloud owns are NaN: one of them read into a sum shows.  reverse: explicit
    row tables that walk the slots backwards; the costs then come back in reverse pair order."""
    dev = torch.device("cuda:0")
    P, ds, dt = len(pairs), pairs[0][0].shape[1], pairs[0][1].shape[1]
    ss, st = (n_cap, m_cap) if slot is None else (slot, slot)
    big_s, big_t = np.full((P * ss, ds), np.nan), np.full((P * st, dt), np.nan)
    for p, (a, b) in enumerate(pairs):
        big_s[p * ss: p * ss + len(a)] = a
        big_t[p * st: p * st + len(b)] = b
    order = list(range(P))[::-1] if reverse else list(range(P))
    n = torch.tensor([len(pairs[p][0]) for p in order], dtype=torch.int64, device=dev)
    m = torch.tensor([len(pairs[p][1]) for p in order], dtype=torch.int64, device=dev)
    rows = {}
    if reverse or slot is not None:
        rows = dict(xs_row=torch.tensor([p * ss for p in order], dtype=torch.int64, device=dev),
                    xt_row=torch.tensor([p * st for p in order], dtype=torch.int64, device=dev))
    return eng.gwd_padded_l1_batch(torch.from_numpy(big_s).to(dev), n, torch.from_numpy(big_t).to(dev), m, n_cap, m_cap,
                                   h=h, **rows).cpu().numpy()


def rel_errors(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert np.all(np.isfinite(ref)) and np.all(ref > 1e-4), ref        # the relative bound has something to bite on
    return np.abs(got - ref) / ref


# ---------------------------------------------------------------------------------------------- A
@pytest.fixture(scope="module")
def case_a(eng, oracle):
    """(ds, dt) -> the ten pairs, their oracle values and their single solves, computed once."""
    cache = {}

    def get(ds, dt):
        if (ds, dt) not in cache:
            rng = np.random.default_rng(1000 * ds + 10 * dt)
            pairs = [uniform_pair(rng, n, m, ds, dt) for n, m in PAIRS]
            ref = np.array([oracle.gwd(a, b) for a, b in pairs])
            cache[(ds, dt)] = (pairs, ref, np.array([single(eng, a, b) for a, b in pairs]))
        return cache[(ds, dt)]
    return get


@pytest.mark.parametrize("ds,dt", FORM_DIMS + EDGE_DIMS)
def test_a_single_solves_against_oracle(case_a, ds, dt):
    pairs, ref, got = case_a(ds, dt)
    err = rel_errors(got, ref)
    print("\nGWD-EDGES A single %s (%d, %d): max rel err %.2e at (n, m) = %s" % (form(ds, dt), ds, dt, err.max(), PAIRS[int(err.argmax())]))
    assert np.all(np.isfinite(got)) and np.all(err <= BUDGET), (got, ref, err)


@pytest.mark.parametrize("ds,dt", FORM_DIMS + EDGE_DIMS)
def test_a_batch_equals_single_solves_bit_for_bit(eng, case_a, ds, dt):
    pairs, ref, got = case_a(ds, dt)
    costs = batch(eng, pairs, CAP, CAP)
    assert np.array_equal(costs, got), (costs, got)


@pytest.mark.parametrize("ds,dt", FORM_DIMS + EDGE_DIMS)
def test_a_row_tables_and_unowned_tiles(eng, case_a, ds, dt):
    """Explicit xs_row / xt_row in reverse pair order and caps of 600 rows (five tiles a side, no pair has more than three):
    the grid holds tiles that no pair owns."""
    pairs, ref, got = case_a(ds, dt)
    costs = batch(eng, pairs, 600, 600, slot=CAP, reverse=True)
    assert np.array_equal(costs, got[::-1]), (costs, got[::-1])


# ---------------------------------------------------------------------------------------------- B
KINDS = ["binary", "duplicates", "letterbox", "constant_column", "two_clusters", "outliers"]
DIMS_BD = [(4, 14), (4, 16)]            # split <2, 6> and float32 <3, 17>
SIZES_BD = [(300, 400), (400, 300)]
BANDWIDTHS = [0.2, 0.7, 3.0]


def grid_columns(m):
    """Two positional columns: a regular 20-column grid in [0, 1]."""
    i = np.arange(m)
    rows = (m + 19) // 20
    return np.stack([(i % 20) / 19.0, (i // 20) / max(rows - 1, 1)], axis=1)


def structured_pair(kind, rng, n, m, ds, dt):
    Xs, Xt = uniform_pair(rng, n, m, ds, dt)
    if kind == "binary":                 # polarity column; channels zero on 70 % of the points; positions on a grid
        Xs[:, 3] = rng.integers(0, 2, n)
        Xt[rng.random(m) < 0.7, : dt - 2] = 0.0
        Xt[:, dt - 2:] = grid_columns(m)
    elif kind == "duplicates":           # every distinct point eight times in the source, four times in the target
        Xs = np.repeat(Xs[: (n + 7) // 8], 8, axis=0)[:n]
        Xt = np.repeat(Xt[: (m + 3) // 4], 4, axis=0)[:m]
    elif kind == "letterbox":            # a quarter of the target: 114.0 in every channel, only the position differs
        Xt[:, dt - 2:] = grid_columns(m)
        Xt[: m // 4, : dt - 2] = 114.0
    elif kind == "constant_column":      # a dimension of zero variance contributes nothing
        Xs[:, 1] = 0.3
        Xt[:, 0] = 114.0
        Xt[:, dt - 3] = 0.0
    elif kind == "two_clusters":
        Xs = 0.01 * rng.random((n, ds)) + 5.0 * rng.integers(0, 2, (n, 1))
        Xt = 0.01 * rng.random((m, dt)) + 100.0 * rng.integers(0, 3, (m, 1))
    elif kind == "outliers":             # row 0 (the pivot of the statistics) is itself an outlier
        Xs[0] += 1000.0
        Xt[:3] += 1e5
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(Xs), np.ascontiguousarray(Xt)


def structured_pairs(kind, ds, dt):
    rng = np.random.default_rng(7000 + 100 * KINDS.index(kind) + dt)
    return [structured_pair(kind, rng, n, m, ds, dt) for n, m in SIZES_BD]


@pytest.fixture(scope="module")
def pairs_b():
    cache = {}

    def get(kind, ds, dt):
        if (kind, ds, dt) not in cache:
            cache[(kind, ds, dt)] = structured_pairs(kind, ds, dt)
        return cache[(kind, ds, dt)]
    return get


@pytest.mark.parametrize("h", BANDWIDTHS)
@pytest.mark.parametrize("ds,dt", DIMS_BD)
@pytest.mark.parametrize("kind", KINDS)
def test_b_structured_clouds_and_bandwidths(eng, oracle, pairs_b, kind, ds, dt, h):
    pairs = pairs_b(kind, ds, dt)
    ref = np.array([oracle.gwd(a, b, h) for a, b in pairs])
    got = np.array([single(eng, a, b, h) for a, b in pairs])
    err = rel_errors(got, ref)
    print("\nGWD-EDGES B %s %s h=%g: max rel err %.2e" % (kind, form(ds, dt), h, err.max()))
    assert np.all(np.isfinite(got)) and np.all(err <= BUDGET), (got, ref, err)
    costs = batch(eng, pairs, 400, 400, h=h)
    assert np.array_equal(costs, got), (costs, got)


@pytest.mark.parametrize("kind", KINDS)
def test_b_identical_structured_clouds_cost_exactly_zero(eng, pairs_b, kind):
    for ds, dt in DIMS_BD:               # the source cloud (split), the target cloud split (14) and float32 (16)
        Xs, Xt = pairs_b(kind, ds, dt)[0]
        for X in ((Xs, Xt) if dt == 14 else (Xt,)):
            for h in BANDWIDTHS:
                assert single(eng, X, X, h) == 0.0, (kind, X.shape, h)


# ---------------------------------------------------------------------------------------------- C
@pytest.mark.parametrize("ds,dt", DIMS_BD)
def test_c_degenerate_clouds_cost_nan_like_the_reference(eng, oracle, ds, dt):
    """A cloud of one point, or of equal points, has sigma = 0: the reference divides 0 by 0 and so must the kernel, alone and
    inside a batch whose ordinary pairs keep their single-solve bits."""
    rng = np.random.default_rng(31 + dt)
    ok = [uniform_pair(rng, n, m, ds, dt) for n, m in ((300, 200), (129, 257), (40, 300))]
    a1, b2 = uniform_pair(rng, 1, 2, ds, dt)
    a2, b1 = uniform_pair(rng, 2, 1, ds, dt)
    a300, b300 = uniform_pair(rng, 300, 300, ds, dt)
    same_s = np.repeat(rng.random((1, ds)), 200, axis=0)
    same_t = np.repeat(rng.random((1, dt)) * np.linspace(1.0, 255.0, dt), 200, axis=0)
    bad = [(a1, b2), (a2, b1), (same_s, b300), (a300, same_t)]
    with np.errstate(all="ignore"):
        assert all(np.isnan(oracle.gwd(a, b)) for a, b in bad)
    got_ok = np.array([single(eng, a, b) for a, b in ok])
    assert np.all(rel_errors(got_ok, [oracle.gwd(a, b) for a, b in ok]) <= BUDGET)
    for a, b in bad:
        assert np.isnan(single(eng, a, b)), (a.shape, b.shape)
    pairs = [ok[0], bad[0], bad[1], ok[1], bad[2], bad[3], ok[2]]
    costs = batch(eng, pairs, 300, 300)
    assert np.all(np.isnan(costs[[1, 2, 4, 5]])), costs
    assert np.array_equal(costs[[0, 3, 6]], got_ok), (costs, got_ok)


# ---------------------------------------------------------------------------------------------- D
SHIFTS = [1e3, 1e6, 1e9, "timestamp"]


def shifted_pairs(shift, ds, dt):
    """The clouds of A at SIZES_BD, moved.  A number: added to every column of both clouds.  "timestamp": only column 2 of
    the source, scaled to a spread of 5e4 and moved to 1.7e15 (microseconds since the epoch).  The moved arrays are the input:
    the oracle gets them as they are, rounding of the sum included."""
    rng = np.random.default_rng(9000 + dt)
    out = []
    for n, m in SIZES_BD:
        Xs, Xt = uniform_pair(rng, n, m, ds, dt)
        if shift == "timestamp":
            Xs[:, 2] = Xs[:, 2] * 5e4 + 1.7e15
        else:
            Xs, Xt = Xs + shift, Xt + shift
        out.append((Xs, Xt))
    return out


@pytest.mark.parametrize("ds,dt", DIMS_BD)
@pytest.mark.parametrize("shift", SHIFTS)
def test_d_translated_clouds(eng, oracle, shift, ds, dt):
    pairs = shifted_pairs(shift, ds, dt)
    ref = np.array([oracle.gwd(a, b) for a, b in pairs])
    got = np.array([single(eng, a, b) for a, b in pairs])
    costs = batch(eng, pairs, 400, 400)
    err, err_b = rel_errors(got, ref), rel_errors(costs, ref)
    print("\nGWD-EDGES D shift %s %s: max rel err single %.2e batched %.2e" % (shift, form(ds, dt), err.max(), err_b.max()))
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(costs)), (got, costs)
    assert np.all(err <= BUDGET) and np.all(err_b <= BUDGET), (got, costs, ref)
    assert np.array_equal(costs, got), (costs, got)
