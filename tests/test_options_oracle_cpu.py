"""Pin oracle/options_oracle.py -- the float64 numpy restatements the GPU option tests compare with -- against goldens
recorded from the reference and against the C oracle wherever the two overlap.  CPU only.  Tolerances are the ones the
suite already uses for the same pair; every non-exact pair prints its largest difference (pytest -s), NOTES.md records them."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, assert_bit_equal, load_golden

from event_representation_study_amd.synthetic import make_events


@pytest.fixture(scope="module")
def opt():
    from oracle import options_oracle
    return options_oracle


def _close(got, want, rtol, atol, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    g64, w64 = got.astype(np.float64), want.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(w64 != 0, np.abs(g64 - w64) / np.abs(w64), 0.0)
    print("%s: max abs diff %.3e, max rel diff %.3e" % (what, float(np.abs(g64 - w64).max()), float(rel.max())))
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, err_msg=what)
    assert np.array_equal(got == 0, want == 0), what + ": exact-zero pattern"


def _ref_layout(surf):
    """(S, 2, H, W) of ToTimesurface.__call__ -> the builders' (H, W, 2S), channel 2s + p."""
    S, _, H, W = surf.shape
    return np.ascontiguousarray(surf.transpose(2, 3, 0, 1).reshape(H, W, 2 * S))


@pytest.mark.parametrize("tag", ["asc", "unsorted"])
def test_time_surface_vs_reference_golden_float_times(opt, tag):
    """Float seconds, tau = 0.01, the cuts [300, 1100, 1101, 2499], ascending and not (make_golden_r04.py)."""
    g = load_golden("time_surface_float_t_40x30")
    H, W, n = int(g["H"]), int(g["W"]), len(g["x"])
    ev = np.stack([g["x"], g["y"], np.zeros(n, np.int64), g["p"]], axis=1)
    got = opt.time_surface(ev, H, W, g["idx"], 0.01, premap=0, times=g["t_" + tag])
    _close(got, _ref_layout(g["surf_" + tag]), 1e-10, 0, "time_surface vs golden surf_" + tag)


@pytest.mark.parametrize("H,W,n,enc", [(60, 200, 9000, "pm1"), (60, 200, 3001, "01"), (48, 160, 40000, "pm1")])
@pytest.mark.parametrize("slices,tau", [(6, 50000.0), (8, 20000.0)])
def test_time_surface_vs_c_oracle_on_its_own_cuts(oracle, opt, H, W, n, enc, slices, tau):
    ev = make_events(n, W, H, seed=50 + n % 7, polarity=enc)
    want, idx = oracle.time_surface(ev, H, W, slices=slices, tau=tau, return_idx=True)
    got = opt.time_surface(ev, H, W, idx, tau, premap=1)
    _close(got, want, 1e-12, 0, "time_surface vs oracle.time_surface %dx%d n=%d S=%d" % (W, H, n, slices))


def test_time_surface_dead_cuts(opt):
    """A repeated cut, a descending one and one at n are never hit: that surface and every later one are exactly 0."""
    H, W = 12, 16
    ev = make_events(500, W, H, seed=3)
    for cuts, live in (([100, 100, 300], 1), ([100, 300, 200, 400], 2), ([100, 500, 499], 1), ([50, 200, 499], 3)):
        got = opt.time_surface(ev, H, W, cuts, 50000.0)
        for s in range(len(cuts)):
            assert bool(got[..., 2 * s:2 * s + 2].all()) == (s < live) and bool(got[..., 2 * s:2 * s + 2].any()) == (s < live), (cuts, s)
    # scale: every value times scale in float64, dead surfaces stay exactly 0
    cuts = [100, 300, 300]
    assert_bit_equal(opt.time_surface(ev, H, W, cuts, 50000.0, scale=255.0), opt.time_surface(ev, H, W, cuts, 50000.0) * 255.0)
    # the event AT the cut index is in the memory of its own surface: exp(0) at its pixel
    got = opt.time_surface(ev, H, W, [100], 50000.0)
    assert got[ev[100, 1], ev[100, 0], (ev[100, 3] + 1) // 2] == 1.0


@pytest.mark.parametrize("order", ["sorted", "unsorted"])
@pytest.mark.parametrize("k", [1, 4, 8])
def test_tore_vs_c_oracle_integer_times(oracle, opt, order, k):
    H, W = 30, 40
    ev = make_events(6000, W, H, seed=21)           # 5 events per pixel: every FIFO depth is reached and passed
    if order == "unsorted":
        ev = np.ascontiguousarray(ev[np.random.default_rng(5).permutation(len(ev))])
    x, y, t, p = ev[:, 0] + 1, ev[:, 1] + 1, ev[:, 2], ev[:, 3]
    for T in (int(ev[-1, 2]), int(np.median(t))):
        _close(opt.tore(x, y, t, p, T, k, (H, W)), oracle.tore(x, y, t, p, T, k, (H, W)), 1e-6, 1e-6,
               "tore vs oracle.tore %s k=%d T=%d" % (order, k, T))


@pytest.mark.parametrize("tag", ["tf_a", "tf_b"])
def test_tore_vs_reference_golden_float_seconds(opt, tag):
    """Float coordinates (truncated by the reference) and float times, sample time = the last time and mid-window."""
    g = load_golden("boundary")
    x, y, t, p = g[tag + "_x"], g[tag + "_y"], g[tag + "_t"], g[tag + "_p"]
    H, W = int(g[tag + "_H"]), int(g[tag + "_W"])
    x1, y1 = x - min(x) + 1, y - min(y) + 1
    got = opt.tore(x1, y1, t, p, t[-1], 6, (H, W))
    _close(got, g[tag + "_tore"], 1e-6, 1e-6, "tore vs golden " + tag)
    assert np.array_equal(got == got.max(), g[tag + "_tore"] == g[tag + "_tore"].max())      # the empty-FIFO pattern
    _close(opt.tore(x1, y1, t, p, float(t[len(t) // 2]) + 1e-9, 4, (H, W)), g[tag + "_tore_mid"], 1e-6, 1e-6, "tore vs golden %s_mid" % tag)


@pytest.mark.parametrize("enc", ["pm1", "01"])
def test_tore_vs_reference_golden_unsorted(opt, enc):
    g = load_golden("tore_unsorted_40x30_n3000")
    H, W = int(g["H"]), int(g["W"])
    ev = g["events_" + enc]
    x, y, ts, pol = ev[:, 0] + 1, ev[:, 1] + 1, ev[:, 2], ev[:, 3]
    _close(opt.tore(x, y, ts, pol, ts[-1], 6, (H, W)), g["tore6_" + enc], 1e-6, 1e-6, "tore vs golden tore6_" + enc)
    _close(opt.tore(x, y, ts, pol, 30000, 3, (H, W)), g["tore3_mid_" + enc], 1e-6, 1e-6, "tore vs golden tore3_mid_" + enc)


def test_voxel_tnorm_vs_reference_golden_and_c_oracle(oracle, opt):
    g = load_golden("compute_repr_float_t_64x48")
    H, W = int(g["H"]), int(g["W"])
    for bins in (5, 9):
        assert_bit_equal(opt.voxel_tnorm(g["x"], g["y"], g["t"], g["p"], H, W, bins), g["voxel%d" % bins], "voxel_tnorm bins=%d" % bins)
    # the demo's normalisation (gromov_wasserstein.py:96) of integer timestamps is the C oracle's entry point
    for n, enc in ((9000, "pm1"), (3001, "01")):
        ev = make_events(n, 200, 60, seed=n, polarity=enc)
        t = ev[:, 2].astype(np.float64)
        t = (t - t[0]) / (t[-1] - t[0])
        for bins in (5, 9):
            assert_bit_equal(opt.voxel_tnorm(ev[:, 0], ev[:, 1], t, ev[:, 3], 60, 200, bins), oracle.voxel(ev, 60, 200, bins), "voxel_tnorm vs oracle.voxel")


def _ni_tnorm(ev):
    """The normalised float64 time the builder is handed (imagenet.py:198-199); polstats truncates x, y and reads p's sign itself."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return (ev[:, 2] - ev[0, 2]) / (ev[-1, 2] - ev[0, 2])


@pytest.mark.parametrize("tag", ["a", "b", "pos", "c224"])
def test_polstats_vs_reference_goldens(oracle, opt, tag):
    """Every array of nimagenet_acc.npz that is a channel list of the builder (n_imagenet_acc.SPECS), and the numpy
    restatement oracle.nimagenet_acc of the same functions."""
    from event_representation_study_amd.n_imagenet_acc import EXP_TAU, SPECS
    g = np.load(os.path.join(GOLDEN, "nimagenet_acc.npz"))
    ev, H, W = g[tag + "_events"], int(g[tag + "_H"]), int(g[tag + "_W"])
    rows, tn = ev, _ni_tnorm(ev)
    seen = []
    for name in ("acc_all", "acc_exp", "flat", "flat_pol", "acc_count_only", "acc_count_pol", "acc_time_pol", "acc_intensity",
                 "acc_time", "acc_count"):
        pol, stat = SPECS[name]
        got = np.ascontiguousarray(np.moveaxis(opt.polstats(rows, tn, H, W, pol, stat, EXP_TAU), -1, 0))
        if name == "acc_intensity":      # the builder's channel is the intensity BEFORE its min-max (imagenet.py:867), float32
            with np.errstate(divide="ignore", invalid="ignore"):
                got = (got - got.min()) / (got.max() - got.min())
        wants = [oracle.nimagenet_acc(name, ev, H, W)]
        if "%s_%s" % (tag, name) in g.files:
            wants.append(g["%s_%s" % (tag, name)])
            seen.append(name)
        for want in wants:
            if name == "acc_exp":
                _close(got, want, 1e-6, 1e-7, "polstats EXP vs %s_%s" % (tag, name))
            else:
                np.testing.assert_array_equal(got, want, err_msg="%s %s" % (tag, name))     # NaN (0/0) equal to NaN
    every = ["acc_all", "acc_exp", "flat", "flat_pol", "acc_count_only", "acc_count_pol", "acc_time_pol", "acc_intensity", "acc_time", "acc_count"]
    assert seen == (["acc_all", "acc_exp"] if tag == "c224" else every), seen       # every golden array was found by its key


def test_polstats_zero_polarity_and_signed(opt):
    """p == 0 belongs to ANY only; SIGNED ignores its class; a negative time is an extreme like any other, not 'empty'."""
    ev = np.array([[1, 0, 0, 0], [1, 0, 0, 1], [1, 0, 0, -1], [2, 0, 0, 0], [3, 0, 0, -1], [3, 0, 0, -1]])
    tn = np.array([-0.5, 0.25, 0.75, 1.5, -0.25, -0.125])
    got = opt.polstats(ev, tn, 1, 4, [0, 1, 2, 0, 0, 2, 0, 1, 0], [0, 0, 0, 1, 2, 1, 3, 3, 5], 0.3)
    want = np.array([[0, 0, 0, 0, 0, 0, 0, 0, 0], [3, 1, 1, 0.75, -0.5, 0.75, 1, 1, 0], [1, 0, 0, 1.5, 1.5, 0, 1, 0, 0],
                     [2, 0, 2, -0.125, -0.25, -0.125, 1, 0, -2]], dtype=np.float32)
    np.testing.assert_array_equal(got[0], want)
    e = opt.polstats(ev, tn, 1, 4, [0, 1], [4, 4], 0.05)[0]
    np.testing.assert_allclose(e[:, 0], np.exp(-(1 - np.array([0, 0.75, 1.5, -0.125])) / 0.05).astype(np.float32), rtol=1e-7)
    np.testing.assert_allclose(e[:, 1], np.exp(-(1 - np.array([0, 0.25, 0, 0])) / 0.05).astype(np.float32), rtol=1e-7)


def test_tonic_voxel_guards(opt):
    """The event at t[-1] has tis == bins: both adds skip it; an event in the last bin has no upper bin."""
    ev = np.array([[0, 0, 0, 1], [1, 0, 50, 0], [2, 0, 95, 1], [3, 0, 100, 1]])
    got = opt.tonic_voxel(ev, 1, 4, 4)
    want = np.zeros((1, 4, 4))
    want[0, 0, 0] = 1.0
    want[0, 1, 2] = -1.0
    want[0, 2, 3] = 1.0 - (3.8 - 3)
    assert_bit_equal(got, want)
    assert_bit_equal(opt.tonic_voxel(ev, 1, 4, 4, scale=255.0), want * 255.0)
