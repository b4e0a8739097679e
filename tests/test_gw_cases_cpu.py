"""The case lists of tests/gw_edge_cases.py held to what tests/test_gpu_gw_edges.py needs of them -- no device, no library.

coverage:    the shapes reach every path of csrc/evrep_gw.hip that depends on a size, in both element sizes
sensitivity: the asymmetric problems move the oracle's answer, under a transposition of C1 or of C2, by far more than the
             tolerance the device is held to -- a solver that confuses rows and columns cannot pass
conditions:  every plan the device test compares by rtol alone (atol = 0) is finite and far from underflow, and the float32
             cases keep the Gibbs exponent where exp() stays a normal float32
zero mass:   what oracle/gw_oracle.py does with zero-mass points, which is what the device test relies on (zeros in one
             marginal) or departs from in words (zeros in both: NaN)
"""
import numpy as np
import pytest

import gw_edge_cases as g
from oracle import gw_oracle


def _all_paths(elem):
    return [g.paths(n, m, elem) for (n, m) in g.SHAPES]


def test_gw_ld_and_paths_restate_the_kernel():
    assert [g.gw_ld(c, 8) for c in (1, 63, 64, 65, 128, 192, 100)] == [1, 63, 72, 65, 136, 200, 100]
    assert [g.gw_ld(c, 4) for c in (1, 64, 127, 128, 129, 256, 192)] == [1, 64, 127, 144, 129, 272, 192]
    p = g.paths(130, 257, 8)
    assert p["gemm1"] == {"K": 130, "a_vec": True, "b_vec": False, "k_class": "partial"}
    assert p["gemm2"] == {"K": 257, "a_vec": False, "b_vec": False, "k_class": "partial"}
    assert (p["row_tiles"], p["col_tiles"], p["col_blocks"], p["per"], p["per_mod4"], p["idle_slice"]) == (2, 3, 2, 3, 3, True)
    p = g.paths(256, 256, 4)
    assert (p["ldn"], p["ldm"], p["pad_n"], p["pad_m"], p["per"], p["idle_slice"]) == (272, 272, True, True, 4, False)


def test_sym_kind_is_the_solver_tests_problem():
    from test_gpu_gw_solver import _problem
    for got, want in zip(g.problem(17, 129, 3, "sym"), _problem(17, 129, 3)):
        assert np.array_equal(got, want)


def test_problem_kinds():
    for n, m in [(33, 47), (130, 257), (1, 1), (2, 3)]:
        C1, C2, p, q = g.case_problem(n, m, "asym")
        assert C1.shape == (n, n) and C2.shape == (m, m) and all(a.dtype == np.float64 for a in (C1, C2, p, q))
        assert C1.min() > 0 and C1.max() <= 1 and abs(p.sum() - 1) < 1e-15 and abs(q.sum() - 1) < 1e-15
        if min(n, m) >= 15:
            assert np.abs(C1 - C1.T).max() > 0.1 and np.abs(C2 - C2.T).max() > 0.1
    n, m = 33, 47
    S1, S2, _, _ = g.case_problem(n, m, "sym")
    assert np.array_equal(S1, S1.T) and np.array_equal(S2, S2.T)
    B1, B2, _, _ = g.case_problem(n, m, "binary")
    assert set(np.unique(B1)) == {0.0, 1.0} and not np.array_equal(B2, B2.T) and 0 < np.diag(B2).sum() < m
    D1, D2, _, _ = g.case_problem(n, m, "dup")
    assert np.array_equal(D1[n - n // 3:, :n // 3], D1[:n // 3, :n // 3]) and np.array_equal(D1[:, n - n // 3:], D1[:, :n // 3])
    assert np.array_equal(D2[m - m // 3:, :], D2[:m // 3, :]) and not np.array_equal(D1, D1.T)
    _, _, p, q = g.case_problem(n, m, "spread")
    assert p.max() / p.min() > 1e3 and q.max() / q.min() > 1e3


@pytest.mark.parametrize("elem", [8, 4])
def test_shapes_cover_every_size_dependent_path(elem):
    P = _all_paths(elem)
    assert max(max(s) for s in g.SHAPES) <= 260
    assert {(p["gemm1"]["a_vec"], p["gemm1"]["b_vec"]) for p in P} == {(True, True), (True, False), (False, True), (False, False)}
    assert {p["gemm2"]["a_vec"] for p in P} == {True, False}
    assert all(p["gemm2"]["a_vec"] == p["gemm2"]["b_vec"] for p in P)
    assert {(p["pad_n"], p["pad_m"]) for p in P} >= {(True, False), (False, True), (True, True), (False, False)}
    Ks = {p[gm]["K"] for p in P for gm in ("gemm1", "gemm2")}
    assert {1, 16, 17} <= Ks and any(1 < k < 16 for k in Ks)
    assert any(k > 128 and k % 16 == 0 for k in Ks) and any(k > 128 and k % 16 for k in Ks)
    assert {p[gm]["k_class"] for p in P for gm in ("gemm1", "gemm2")} == {"below", "multiple", "partial"}
    for axis in ("M", "N"):
        vals = {p[axis]["value"] for p in P}
        assert {1, 64, 65, 128, 129} <= vals and any(1 < v < 64 for v in vals) and any(v > 256 for v in vals), (axis, vals)
        assert {(p[axis]["vs_quad"], p[axis]["vs_tile"]) for p in P} == {(-1, -1), (0, -1), (1, -1), (1, 0), (1, 1)}
    assert {1, 2, 3} <= {p["row_tiles"] for p in P} and {1, 2, 3} <= {p["col_tiles"] for p in P}
    assert {1, 2} <= {p["col_blocks"] for p in P}
    pers = {(p["per"], p["idle_slice"]) for p in P}
    assert (1, True) in pers and (2, True) in pers
    assert any(p["per"] >= 4 and p["per_mod4"] != 0 for p in P) and any(p["per"] >= 4 and p["per_mod4"] == 0 for p in P)
    assert any(not p["idle_slice"] for p in P)


def _asym_shapes():
    return [(n, m) for (n, m) in g.SHAPES if min(n, m) >= 15]


def _moves(C1, C2, p, q, loss, eps, iters):
    """How far the oracle moves when C2 / C1 is replaced by its transpose -> [(gw move, largest plan-entry move)] x 2."""
    T, gw = gw_oracle.entropic_gromov_wasserstein(C1, C2, p, q, loss, eps, *iters)
    out = []
    for A, B in ((C1, np.ascontiguousarray(C2.T)), (np.ascontiguousarray(C1.T), C2)):
        Tt, gt = gw_oracle.entropic_gromov_wasserstein(A, B, p, q, loss, eps, *iters)
        out.append((abs(gt - gw) / abs(gw), float(np.max(np.abs(Tt - T) / T))))
    return out


def test_asymmetric_cases_are_sensitive_to_a_transposition():
    """Float64 full solves: gw itself moves by more than 100 x the 1e-9 it is held to (measured: 9e-6 to 2.5e-2), for C2.T
    and for C1.T.
    Float32 full solves: gw CANNOT carry this -- under C2.T it moves by 1.6e-6 (256 x 256, square_loss, eps 0.5) to 2e-2, and
    the float32 tolerance on gw is 1e-5 -- so there the plan has to: its largest entry-wise move (1.1e-2 to 1.5, against an
    rtol of 2e-4) must exceed 10 x rtol.  (A wrong plan fails as soon as the move exceeds rtol plus the device's own error,
    which the float32 emulation puts at 1.3e-5; ten is the margin asked for, fifty-seven the smallest one found.)
    One outer, one Sinkhorn iteration: the plan moves by more than twice the derived bound of the case, so a plan within the
    bound of the transposed problem's answer lies outside the bound of the right one."""
    seen = {}
    for n, m, kind, loss, eps, prec in g.FULL_CASES:
        if (n, m) not in _asym_shapes() or kind != "asym":
            continue
        key = (n, m, loss, eps)
        if key not in seen:
            seen[key] = _moves(*g.case_problem(n, m, kind), loss, eps, g.FULL)
        gw_tol, plan_rtol = g.TOL[prec]
        for gw_move, plan_move in seen[key]:
            if prec == "f64":
                assert gw_move > 100 * gw_tol, (n, m, loss, eps, gw_move)
            assert plan_move > (100 if prec == "f64" else 10) * plan_rtol, (n, m, loss, eps, prec, plan_move)
    assert len(seen) == len(_asym_shapes()) * 2 * 2 + 2 * 2          # eps 0.1 and 0.5 everywhere, 0.05 at two of the shapes
    for n, m, kind, loss, eps, prec in g.ONE_ITER_CASES:
        if (n, m) in _asym_shapes():
            C1, C2, p, q = g.case_problem(n, m, kind)
            bound = g.one_iter_bound(C1, C2, p, q, loss, eps, prec)
            for _, plan_move in _moves(C1, C2, p, q, loss, eps, g.ONE_ITER):
                assert plan_move > 2 * bound, (n, m, loss, prec, plan_move, bound)


def test_conditions_of_every_device_case():
    """Finite plans with no entry below 1e-30 (all marginals here are positive), so rtol alone checks every entry; float32
    cases keep |2 tens / eps| below 60 in every outer iteration (exp(-60) = 9e-27, float32's smallest normal is 1e-38)."""
    count = 0
    for cases, iters in ((g.PRODUCT_CASES, g.PRODUCT), (g.ONE_ITER_CASES, g.ONE_ITER), (g.FULL_CASES, g.FULL), (g.VALUE_CASES, g.FULL)):
        for case in cases:
            n, m, kind, loss, eps, prec = case
            C1, C2, p, q = g.case_problem(n, m, kind)
            T, gw, (lo, hi) = g.oracle_trace(C1, C2, p, q, loss, eps, iters)
            Tc, gc = g.case_oracle(case, iters)
            assert np.array_equal(T, Tc) and gw == gc, case         # the trace IS the oracle
            assert p.min() > 0 and q.min() > 0
            assert np.isfinite(T).all() and np.isfinite(gw) and T.min() >= 1e-30, (case, T.min())
            if prec == "f32":
                assert -60 < lo and hi < 60, (case, lo, hi)
            count += 1
    assert count == 64 + 64 + (32 + 6 + 64) + (8 + 16)
    # the lists are what the issue names
    assert len({c[:2] for c in g.FULL_CASES}) == 16 and {c[4] for c in g.FULL_CASES if c[5] == "f32"} == {0.5, 0.1}
    assert {(c[0], c[1]) for c in g.FULL_CASES if c[4] == 0.05} == set(g.LOW_EPS_SHAPES)


@pytest.mark.parametrize("loss", g.LOSSES)
def test_zero_mass_in_the_oracle(loss):
    """Zeros in p only or in q only: the oracle is finite, those rows / columns are exactly 0, and gw and the remaining
    block are those of the problem without the points (measured: 6e-15 at most; held to 7e-15).  Zeros in both: NaN -- POT's
    recurrence forms Kp = (1 / a) * K, a row of inf, and dot(Kp, v) then meets inf * 0 at the columns whose v is 0."""
    for which in ("p", "q"):
        C1, C2, p, q, rows, cols = g.zero_mass(which)
        assert (~rows).sum() == (3 if which == "p" else 0) and (~cols).sum() == (3 if which == "q" else 0)
        with np.errstate(divide="ignore"):
            T, gw = gw_oracle.entropic_gromov_wasserstein(C1, C2, p, q, loss, 0.1, *g.FULL)
        Tr, gr = gw_oracle.entropic_gromov_wasserstein(*g.reduced(C1, C2, p, q, rows, cols), loss, 0.1, *g.FULL)
        assert np.isfinite(T).all() and np.isfinite(gw)
        assert (T[~rows] == 0).all() and (T[:, ~cols] == 0).all()
        assert abs(gw - gr) <= 7e-15 * abs(gr)
        np.testing.assert_allclose(T[np.ix_(rows, cols)], Tr, rtol=7e-15, atol=0)
        assert Tr.min() >= 1e-30
    C1, C2, p, q, rows, cols = g.zero_mass("both")
    assert (~rows).sum() == 3 and (~cols).sum() == 3
    with np.errstate(divide="ignore", invalid="ignore"):
        T, gw = gw_oracle.entropic_gromov_wasserstein(C1, C2, p, q, loss, 0.1, *g.FULL)
    assert np.isnan(gw) and np.isnan(T).any()


def test_unknown_precision_is_a_value_error_before_any_device_work():
    from event_representation_study_amd.gw_solver import entropic_gromov_wasserstein
    C1, C2, p, q = g.case_problem(2, 3, "asym")
    for bad in ("f16", "F32", None):
        with pytest.raises(ValueError, match="precision"):
            entropic_gromov_wasserstein(C1, C2, p, q, precision=bad)
