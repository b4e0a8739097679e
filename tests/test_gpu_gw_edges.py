"""-m gpu: the entropic Gromov-Wasserstein solver (csrc/evrep_gw.hip: the MFMA GEMM k_gw_gemm and nine streaming kernels) held
to oracle/gw_oracle.py on every path that depends on a size, a precision or a value -- the cases of tests/gw_edge_cases.py,
which tests/test_gw_cases_cpu.py holds to the kernel's paths and to the conditions the tolerances below rest on.

Every problem is ASYMMETRIC unless it says otherwise: k_gw_init lays h2(C2) down transposed, and with the symmetric Gaussian
kernels of test_gpu_gw_solver.py a wrong row / column sense of C1, C2, a_i or b_j moves nothing.

product plan (outer_iters = 0): T_out is p q^T bit for bit (float32: rounded once), and gw is the loss of that plan -- init,
    both GEMMs and k_gw_lossrows, with no exp and no Sinkhorn -- against np.longdouble, within the bound below.
one outer, one Sinkhorn iteration: every element of the second GEMM shows in one plan entry; every entry within a DERIVED
    bound of the oracle's, atol = 0.
full solves (3 outer x 20 Sinkhorn): the project's own tolerances -- float64 gw 1e-9 relative and plan rtol 1e-8, float32
    gw 1e-5 and plan rtol 2e-4 -- with atol = 0 (test_gw_cases_cpu.py: no plan entry below 1e-30, float32 Gibbs exponents
    below 60).  A numpy emulation of the float32 data flow stayed at or below 3.6e-7 on gw and 1.3e-5 on the plan over these
    shapes: an emulation, not a measurement of the kernel.

The bound.  u_T = 2^-53 or 2^-24, gamma_k = k u_T / (1 - k u_T).  The device forms tens_ij = a_i + b_j - (hC1 T hC2^T)_ij from
a_i, b_j (summed in float64, rounded once to T), hC1, hC2, T (rounded once) and two GEMMs that accumulate n and m products in
precision T in some order, so its tens lies within
    delta_ij = (gamma_{n+2} + gamma_{m+2}) S_ij,   S = |a_i| + |b_j| + (|hC1| |p q^T| |hC2|^T)_ij
of the exact one (the final a + b - x is float64).  With outer_iters = 0 gw = sum tens_ij T_ij, so |gw - exact| <= sum
delta_ij T_ij: that is the product-plan bound.  (k_gw_lossrows' float64 sum of the products adds about ten more float64
roundings per term; the bound does not count them, and at 1 x 1 in float64, where it is 6 u S, they are of its order.  It
is kept as derived: the largest measured error is 0.063 of it, at 1 x 5.)  After exp(-2 tens / eps), rounded to
T, a Gibbs entry is within rho = max expm1(2 delta / eps) + u_T of exact, relatively.  The Sinkhorn sums have positive terms
and run in float64 in both precisions: v = q / (K^T u0) inherits rho, u = p / (K v) 2 rho, and T = u K v, rounded to T, is
within 5 rho + 8 gamma64_{max(n, m) + 2} to first order (rho <= 4e-3 here: the second order is below 2 % of the bound).
Twice that is allowed, because the float64 oracle carries an error of its own.  Measured ratios of error to bound are
printed (-s) and recorded in NOTES.md: 3.5e-3 (float64) and 4.5e-3 (float32) at most on one MI355X -- a worst-case bound
against errors that average out -- and tests/test_gw_cases_cpu.py asserts that a transposition of C1 or C2 moves every such
plan by more than twice its bound.

PARITY UNPINNED against POT itself (POT is not installed: `import ot` fails); the oracle restates its published recurrences.
"""
import numpy as np
import pytest
import torch

import gw_edge_cases as g

# (the shared problems are read-only arrays; the door copies them to the device and never writes to them)
pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]

_WORST = {}


def _note(name, prec, value, case):
    key = (name, prec)
    if key not in _WORST or value > _WORST[key][0]:
        _WORST[key] = (value, g.case_id(case) if isinstance(case, tuple) else case)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for (name, prec), (value, where) in sorted(_WORST.items()):
        print("\n[gw edges] largest %-28s %s: %.3e  (%s)" % (name, prec, value, where))


def _solve(C1, C2, p, q, loss, eps, iters, prec, **kw):
    from event_representation_study_amd.gw_solver import entropic_gromov_wasserstein
    T, gw = entropic_gromov_wasserstein(C1, C2, p, q, loss, epsilon=eps, outer_iters=iters[0], sinkhorn_iters=iters[1],
                                        precision=prec, **kw)
    return (None if T is None else T.cpu().numpy()), float(gw)


def _solve_case(case, iters):
    n, m, kind, loss, eps, prec = case
    return _solve(*g.case_problem(n, m, kind), loss, eps, iters, prec)


def _rel_err(T, Tref):
    """Largest |T - Tref| / |Tref| over the entries; an entry that is 0 in both counts as 0, 0 in one only as inf."""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.abs(T - Tref) / np.abs(Tref)
    r[(T == 0) & (Tref == 0)] = 0.0
    return float(np.max(r))


def _hold(case_or_name, prec, T, gw, Tref, gref, what=""):
    """The project's tolerances of precision `prec`, atol = 0."""
    gw_tol, plan_rtol = g.TOL[prec]
    ge, pe = abs(gw - gref) / abs(gref), _rel_err(T, Tref)
    _note("full-solve gw error" + what, prec, ge, case_or_name)
    _note("full-solve plan error" + what, prec, pe, case_or_name)
    assert np.isfinite(T).all() and np.isfinite(gw)
    assert ge <= gw_tol, (case_or_name, gw, gref, ge)
    np.testing.assert_allclose(T, Tref, rtol=plan_rtol, atol=0)


# ------------------------------------------------------------------------------------------------------- product plan
def _product_reference(C1, C2, p, q, loss, T):
    """sum((a_i + b_j - hC1 T hC2^T) * T) in np.longdouble.  log() takes the float64 sum C + 1e-15, as the oracle and the device
    define it."""
    L = np.longdouble
    c1, c2, pl, ql, Tl = C1.astype(L), C2.astype(L), p.astype(L), q.astype(L), T.astype(L)
    if loss == "square_loss":
        a, b, h1, h2 = (c1 * c1) @ pl, (c2 * c2) @ ql, c1, 2 * c2
    else:
        a, b = (c1 * np.log((C1 + 1e-15).astype(L)) - c1) @ pl, c2 @ ql
        h1, h2 = c1, np.log((C2 + 1e-15).astype(L))
    tens = a[:, None] + b[None, :] - h1 @ Tl @ h2.T
    return float(np.sum(tens * Tl))


@pytest.mark.parametrize("case", g.PRODUCT_CASES, ids=g.case_id)
def test_product_plan(case):
    n, m, kind, loss, eps, prec = case
    C1, C2, p, q = g.case_problem(n, m, kind)
    T, gw = _solve(C1, C2, p, q, loss, eps, g.PRODUCT, prec)
    want = p[:, None] * q[None, :]
    if prec == "f32":
        want = want.astype(np.float32).astype(np.float64)           # rounded once, widened
    assert T.dtype == np.float64 and np.array_equal(T.view(np.uint64), want.view(np.uint64))
    ref = _product_reference(C1, C2, p, q, loss, T)
    bound = float(np.sum(g.tens_delta(C1, C2, p, q, loss, prec, T=T) * T))
    ratio = abs(gw - ref) / bound
    _note("product-plan gw error / bound", prec, ratio, case)
    print("%s: gw %.17g reference %.17g error/bound %.3e" % (g.case_id(case), gw, ref, ratio))
    assert abs(gw - ref) <= bound, (gw, ref, bound)


# ------------------------------------------------------------------------------------- one outer, one Sinkhorn iteration
@pytest.mark.parametrize("case", g.ONE_ITER_CASES, ids=g.case_id)
def test_one_outer_one_sinkhorn_iteration(case):
    n, m, kind, loss, eps, prec = case
    C1, C2, p, q = g.case_problem(n, m, kind)
    T, gw = _solve(C1, C2, p, q, loss, eps, g.ONE_ITER, prec)
    Tref, gref = g.case_oracle(case, g.ONE_ITER)
    bound = g.one_iter_bound(C1, C2, p, q, loss, eps, prec)
    err = _rel_err(T, Tref)
    _note("one-iteration plan error / bound", prec, err / bound, case)
    print("%s: plan error %.3e bound %.3e ratio %.3e; gw error %.3e" % (g.case_id(case), err, bound, err / bound,
                                                                         abs(gw - gref) / abs(gref)))
    assert np.isfinite(T).all() and Tref.min() > 0
    assert (np.abs(T - Tref) <= bound * Tref).all(), (err, bound)


# ----------------------------------------------------------------------------------------------------------- full solves
@pytest.mark.parametrize("case", g.FULL_CASES, ids=g.case_id)
def test_full_solve(case):
    T, gw = _solve_case(case, g.FULL)
    _hold(case, case[5], T, gw, *g.case_oracle(case, g.FULL))


@pytest.mark.parametrize("case", g.VALUE_CASES, ids=g.case_id)
def test_values_at_the_edges(case):
    """Zeros in C (kl_loss: log(1e-15) in h2(C2), 0 * log(1e-15) in f1), duplicate points, marginals over four decades."""
    T, gw = _solve_case(case, g.FULL)
    _hold(case, case[5], T, gw, *g.case_oracle(case, g.FULL), what=" (values)")
    n, m, kind = case[:3]
    if kind == "dup":                                               # equal points: rows in the ratio of their masses
        _, _, p, q = g.case_problem(n, m, kind)
        np.testing.assert_allclose(T[n - n // 3:] / p[n - n // 3:, None], T[:n // 3] / p[:n // 3, None], rtol=g.TOL[case[5]][1])
        np.testing.assert_allclose(T[:, m - m // 3:] / q[m - m // 3:], T[:, :m // 3] / q[:m // 3], rtol=g.TOL[case[5]][1])


# ------------------------------------------------------------------------------------------------------------- zero mass
@pytest.mark.parametrize("prec", g.PRECISIONS)
@pytest.mark.parametrize("loss", g.LOSSES)
@pytest.mark.parametrize("which", ["p", "q"])
def test_zero_mass_in_one_marginal(which, loss, prec):
    """Equal to the oracle; the rows / columns of the zero-mass points are exactly 0.0; gw and the surviving block are those
    of the device's own solve of the problem without the points (float64: the float64 tolerances; float32: its own)."""
    eps = g.ONE_ITER_EPS[prec]
    C1, C2, p, q, rows, cols = g.zero_mass(which)
    from oracle import gw_oracle
    with np.errstate(divide="ignore"):                              # 1 / a at the zero-mass rows: inf, and 1 / inf = 0
        Tref, gref = gw_oracle.entropic_gromov_wasserstein(C1, C2, p, q, loss, eps, *g.FULL)
    T, gw = _solve(C1, C2, p, q, loss, eps, g.FULL, prec)
    name = "zero mass in %s, %s" % (which, loss)
    _hold(name, prec, T, gw, Tref, gref, what=" (zero mass)")
    assert (~rows).sum() + (~cols).sum() == 3
    assert not T[~rows].any() and not T[:, ~cols].any() and not np.signbit(T).any()
    Tr, gr = _solve(*g.reduced(C1, C2, p, q, rows, cols), loss, eps, g.FULL, prec)
    _hold(name + ", reduced", prec, T[np.ix_(rows, cols)], gw, Tr, gr, what=" (zero mass)")


@pytest.mark.parametrize("prec", g.PRECISIONS)
@pytest.mark.parametrize("loss", g.LOSSES)
def test_zero_mass_in_both_marginals(loss, prec):
    """The oracle is NaN here and cannot be the reference: POT's published recurrence forms Kp = (1 / a) * K, which is a row
    of inf where a_i = 0, and dot(Kp, v) then multiplies inf by the v_j = 0 of a zero-mass column (test_gw_cases_cpu.py
    asserts the NaN).  The device computes u = p / (K v), which is 0 / s = 0 at such a row: it is finite, its zero-mass rows
    and columns are exactly 0, and the rest equals its own solve of the problem without the points."""
    eps = g.ONE_ITER_EPS[prec]
    C1, C2, p, q, rows, cols = g.zero_mass("both")
    T, gw = _solve(C1, C2, p, q, loss, eps, g.FULL, prec)
    assert np.isfinite(T).all() and np.isfinite(gw)
    assert (~rows).sum() == 3 and (~cols).sum() == 3 and not T[~rows].any() and not T[:, ~cols].any()
    Tr, gr = _solve(*g.reduced(C1, C2, p, q, rows, cols), loss, eps, g.FULL, prec)
    _hold("zero mass in both, %s, reduced" % loss, prec, T[np.ix_(rows, cols)], gw, Tr, gr, what=" (zero mass)")


# ------------------------------------------------------------------------------------------------------------- asymmetry
@pytest.mark.parametrize("n,m", [(63, 65), (130, 257)])
@pytest.mark.parametrize("loss", g.LOSSES)
def test_transposing_c2_moves_the_device_as_it_moves_the_oracle(n, m, loss):
    from oracle import gw_oracle
    C1, C2, p, q = g.case_problem(n, m, "asym")
    C2t = np.ascontiguousarray(C2.T)
    _, gref = g.case_oracle((n, m, "asym", loss, 0.1, "f64"), g.FULL)
    _, gref_t = gw_oracle.entropic_gromov_wasserstein(C1, C2t, p, q, loss, 0.1, *g.FULL)
    _, gw = _solve(C1, C2, p, q, loss, 0.1, g.FULL, "f64")
    _, gw_t = _solve(C1, C2t, p, q, loss, 0.1, g.FULL, "f64")
    tol = g.TOL["f64"][0]
    assert abs(gref_t - gref) > 100 * tol * abs(gref)               # the problem tells the two apart ...
    assert abs(gw_t - gref_t) <= tol * abs(gref_t) and abs(gw - gref) <= tol * abs(gref)
    assert abs((gw_t - gw) - (gref_t - gref)) <= 2 * tol * abs(gref)        # ... and the device moves by the oracle's move


# ---------------------------------------------------------------------------------------------------------------- reruns
@pytest.mark.parametrize("prec", g.PRECISIONS)
@pytest.mark.parametrize("n,m", [(129, 128), (257, 66)])
def test_reruns_are_bit_equal(n, m, prec):
    for loss in g.LOSSES:
        case = (n, m, "asym", loss, g.ONE_ITER_EPS[prec], prec)
        T1, g1 = _solve_case(case, g.FULL)
        T2, g2 = _solve_case(case, g.FULL)
        assert np.array_equal(T1.view(np.uint64), T2.view(np.uint64)) and np.float64(g1).tobytes() == np.float64(g2).tobytes()


# ------------------------------------------------------------------------------------------------------- the Python door
def _bits(res):
    T, gw = res
    return (None if T is None else T.cpu().numpy().tobytes()), np.float64(float(gw)).tobytes()


def _door(*a, **kw):
    from event_representation_study_amd.gw_solver import entropic_gromov_wasserstein
    kw.setdefault("epsilon", 0.1)
    kw.setdefault("outer_iters", 2)
    kw.setdefault("sinkhorn_iters", 5)
    return entropic_gromov_wasserstein(*a, **kw)


@pytest.mark.parametrize("prec", g.PRECISIONS)
def test_door_input_forms(prec):
    C1, C2, p, q = g.case_problem(16, 17, "asym")
    f32 = [a.astype(np.float32) for a in (C1, C2, p, q)]            # values float32 holds exactly
    want = _bits(_door(*[a.astype(np.float64) for a in f32], "kl_loss", precision=prec))
    assert _bits(_door(*[torch.from_numpy(a).cuda() for a in f32], "kl_loss", precision=prec)) == want
    assert all(t.dtype == torch.float32 for t in [torch.from_numpy(a) for a in f32])
    assert _bits(_door(*[a.astype(np.float64).tolist() for a in f32], "kl_loss", precision=prec)) == want
    # a non-contiguous view: the transpose of an asymmetric matrix, as numpy and as a CUDA tensor
    base = np.ascontiguousarray(C1.T)
    assert not base.T.flags.c_contiguous and not np.array_equal(base, base.T)
    want = _bits(_door(np.ascontiguousarray(base.T), C2, p, q, precision=prec))
    assert _bits(_door(base.T, C2, p, q, precision=prec)) == want
    dev = torch.from_numpy(base).cuda().T
    assert not dev.is_contiguous() and _bits(_door(dev, C2, p, q, precision=prec)) == want
    assert _bits(_door(base, C2, p, q, precision=prec)) != want     # the view's strides matter
    col = np.ascontiguousarray(np.stack([q, q], 1))[:, 0]           # a strided vector
    assert not col.flags.c_contiguous and _bits(_door(base.T, C2, p, col, precision=prec)) == want


@pytest.mark.parametrize("prec", g.PRECISIONS)
def test_door_defaults_and_plan_switch(prec):
    n, m = 15, 16
    C1, C2, _, _ = g.case_problem(n, m, "asym")
    want = _bits(_door(C1, C2, np.full(n, 1.0 / n), np.full(m, 1.0 / m), precision=prec))
    assert _bits(_door(C1, C2, precision=prec)) == want
    assert _bits(_door(C1, C2, None, None, precision=prec)) == want
    T, gw = _door(C1, C2, precision=prec, return_plan=False)
    assert T is None and np.float64(float(gw)).tobytes() == want[1]
    T, gw = _door(C1, C2, precision=prec)
    assert T.dtype == torch.float64 and tuple(T.shape) == (n, m) and T.is_cuda and gw.dtype == torch.float64 and gw.dim() == 0


def test_door_rejects_an_unknown_precision():
    C1, C2, p, q = g.case_problem(5, 1, "asym")
    for bad in ("f16", "F64", "float64", "", None, 0):
        with pytest.raises(ValueError):
            _door(C1, C2, p, q, precision=bad)
