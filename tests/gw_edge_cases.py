"""The case lists of the entropic Gromov-Wasserstein solver's edge tests, shared by tests/test_gw_cases_cpu.py (which holds
the lists to the paths of csrc/evrep_gw.hip and to the conditions the tolerances rest on) and tests/test_gpu_gw_edges.py (the
device against oracle/gw_oracle.py).  Everything is numpy and deterministic; nothing here touches a device or the library.
"""
import functools

import numpy as np

LOSSES = ("square_loss", "kl_loss")
PRECISIONS = ("f64", "f32")
ELEM = {"f64": 8, "f32": 4}
KINDS = ("asym", "sym", "binary", "dup", "spread")

# kernel constants restated from csrc/evrep_gw.hip (kGwBM = kGwBN, kGwBK, the wave quadrant, kGwSlices, k_gw_colsum's block)
TILE, BK, QUAD, SLICES, COL_BLOCK = 128, 16, 64, 64, 256

# nothing above 260: the smallest sizes that reach three row tiles (257) and two column-sum blocks (m > 256)
SHAPES = [(1, 1), (1, 5), (5, 1), (2, 3), (15, 16), (16, 17), (63, 65), (65, 63), (64, 128), (128, 64), (127, 129), (128, 132),
          (129, 128), (130, 257), (257, 66), (256, 256)]
# (outer_iters, sinkhorn_iters): the product plan (init, both GEMMs, k_gw_lossrows; no exp, no Sinkhorn); one Gibbs kernel and
# one Sinkhorn sweep, where every element of the second GEMM shows in one plan entry; a short full solve
PRODUCT, ONE_ITER, FULL = (0, 1), (1, 1), (3, 20)
ITERS = [PRODUCT, ONE_ITER, FULL]
ONE_ITER_EPS = {"f32": 0.5, "f64": 0.1}
# the project's own tolerances (tests/test_gpu_gw_solver.py): relative on gw, rtol on every plan entry (atol = 0 here)
TOL = {"f64": (1e-9, 1e-8), "f32": (1e-5, 2e-4)}
# float64 only: at (2, 3), kl_loss, the plan's smallest entry is 5e-26 (another draw of the same shape reached 1.3e-43, below
# float32's range); compared entry by entry with rtol like the rest
LOW_EPS_SHAPES = [(2, 3), (15, 16), (63, 65)]
VALUE_SHAPES = [(33, 47), (130, 257)]
ZERO_SHAPE = (33, 47)


def seed_of(n, m):
    return 1000 * n + m


def _gauss_kernel(X, h=0.7):
    D2 = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    sig2 = D2.mean() / 2.0
    return np.exp(-D2 / (2.0 * h * h * sig2)) if sig2 > 0 else np.ones_like(D2)   # one point (or all points equal): 0 / 0


def problem(n, m, seed, kind="asym"):
    """-> C1 (n, n), C2 (m, m), p (n), q (m), float64.  "sym" is test_gpu_gw_solver._problem draw for draw; the other kinds
    draw from the same generator after it, so the points and (except "spread") the marginals are those of "sym".
    asym:   the Gaussian kernels times a factor uniform in [0.25, 1) per ENTRY: C[i][k] != C[k][i], values in (0, 1]
    binary: entries 0 / 1 with P(1) = 0.3, not symmetrised, the diagonal as drawn
    dup:    asym, with the last third of the points copies of the first third (equal rows AND columns, factor included)
    spread: asym, with p and q proportional to 10 ** uniform(-4, 0)"""
    if kind not in KINDS:
        raise ValueError(kind)
    rng = np.random.default_rng(seed)
    X1 = rng.random((n, 4))
    X2 = rng.random((m, 6)) * np.array([3.0, 3, 3, 3, 1, 1])
    p = rng.random(n) + 0.5
    q = rng.random(m) + 0.5
    if kind == "binary":
        C1 = (rng.random((n, n)) < 0.3).astype(np.float64)
        C2 = (rng.random((m, m)) < 0.3).astype(np.float64)
    else:
        src1, src2 = np.arange(n), np.arange(m)
        if kind == "dup":
            src1[n - n // 3:] = np.arange(n // 3)
            src2[m - m // 3:] = np.arange(m // 3)
        C1, C2 = _gauss_kernel(X1[src1]), _gauss_kernel(X2[src2])
        if kind != "sym":
            C1 = C1 * (0.25 + 0.75 * rng.random((n, n)))[np.ix_(src1, src1)]
            C2 = C2 * (0.25 + 0.75 * rng.random((m, m)))[np.ix_(src2, src2)]
    if kind == "spread":
        p = 10.0 ** rng.uniform(-4, 0, n)
        q = 10.0 ** rng.uniform(-4, 0, m)
    return np.ascontiguousarray(C1), np.ascontiguousarray(C2), p / p.sum(), q / q.sum()


@functools.lru_cache(maxsize=None)
def _problem_cached(n, m, kind):
    out = problem(n, m, seed_of(n, m), kind)
    for a in out:
        a.setflags(write=False)
    return out


def case_problem(n, m, kind="asym"):
    """The problem of a listed case: seed_of(n, m), computed once and read-only."""
    return _problem_cached(n, m, kind)


def gw_ld(cols, elem):
    """csrc/evrep_gw.hip gw_ld(): a row pitch that is a multiple of 512 bytes gets 64 bytes more."""
    return cols + 64 // elem if cols * elem % 512 == 0 else cols


def _k_class(K):
    return "below" if K < BK else ("multiple" if K % BK == 0 else "partial")


def _rel(x):
    """x against the wave quadrant and the workgroup tile."""
    return {"value": x, "vs_quad": (x > QUAD) - (x < QUAD), "vs_tile": (x > TILE) - (x < TILE)}


def paths(n, m, elem):
    """The paths a solve of an (n, m) problem takes at element size `elem`, from the kernel's own rules.
    gemm1: G = hC1 T (M = n, N = m, K = n, lda = ldn, ldb = ldm);  gemm2: G hC2^T (M = n, N = m, K = m, lda = ldb = ldm).
    a_vec / b_vec: the operand is staged with 16-byte loads (pitch a multiple of 16 / elem elements), else element-wise."""
    vec = 16 // elem
    ldn, ldm = gw_ld(n, elem), gw_ld(m, elem)
    per = -(-n // SLICES)
    return {
        "ldn": ldn, "ldm": ldm, "pad_n": ldn != n, "pad_m": ldm != m,
        "gemm1": {"K": n, "a_vec": ldn % vec == 0, "b_vec": ldm % vec == 0, "k_class": _k_class(n)},
        "gemm2": {"K": m, "a_vec": ldm % vec == 0, "b_vec": ldm % vec == 0, "k_class": _k_class(m)},
        "row_tiles": -(-n // TILE), "col_tiles": -(-m // TILE), "M": _rel(n), "N": _rel(m),
        "per": per, "per_mod4": per % 4, "idle_slice": (SLICES - 1) * per >= n, "col_blocks": -(-m // COL_BLOCK),
    }


# ----------------------------------------------------------------------------------------------------------- the lists
# every entry: (n, m, kind, loss, eps, precision)
PRODUCT_CASES = [(n, m, "asym", loss, 0.1, prec) for (n, m) in SHAPES for loss in LOSSES for prec in PRECISIONS]
ONE_ITER_CASES = [(n, m, "asym", loss, ONE_ITER_EPS[prec], prec) for (n, m) in SHAPES for loss in LOSSES for prec in PRECISIONS]
FULL_CASES = ([(n, m, "asym", loss, 0.1, "f64") for (n, m) in SHAPES for loss in LOSSES]
              + [(n, m, "asym", loss, 0.05, "f64") for (n, m) in LOW_EPS_SHAPES for loss in LOSSES]
              + [(n, m, "asym", loss, eps, "f32") for (n, m) in SHAPES for loss in LOSSES for eps in (0.5, 0.1)])
# zeros in C (kl_loss multiplies by log(1e-15): a larger eps keeps the Gibbs kernel in range), duplicate points, marginals
# over four decades
VALUE_CASES = ([(n, m, "binary", loss, eps, prec) for (n, m) in VALUE_SHAPES for prec in PRECISIONS
                for loss, eps in (("square_loss", 0.5), ("kl_loss", 5.0))]
               + [(n, m, kind, loss, ONE_ITER_EPS[prec], prec) for (n, m) in VALUE_SHAPES for prec in PRECISIONS
                  for kind in ("dup", "spread") for loss in LOSSES])


def case_id(case):
    n, m, kind, loss, eps, prec = case
    return "%dx%d-%s-%s-eps%g-%s" % (n, m, kind, loss.split("_")[0], eps, prec)


def zero_mass(which):
    """The (33, 47) asymmetric problem with mass taken from some points -> C1, C2, p, q, keep_rows, keep_cols (bool masks).
    which: "p" (rows 0, 7, 32), "q" (columns 0, 20, 46), "both"."""
    n, m = ZERO_SHAPE
    C1, C2, p, q = case_problem(n, m, "asym")
    p, q = p.copy(), q.copy()
    if which in ("p", "both"):
        p[[0, 7, n - 1]] = 0.0
    if which in ("q", "both"):
        q[[0, 20, m - 1]] = 0.0
    return C1, C2, p / p.sum(), q / q.sum(), p > 0, q > 0


def reduced(C1, C2, p, q, rows, cols):
    """The problem with only the points of the masks `rows` / `cols`."""
    return (np.ascontiguousarray(C1[np.ix_(rows, rows)]), np.ascontiguousarray(C2[np.ix_(cols, cols)]),
            np.ascontiguousarray(p[rows]), np.ascontiguousarray(q[cols]))


# ----------------------------------------------------------------------------------------------------------- the oracle
def oracle_trace(C1, C2, p, q, loss, eps, iters):
    """oracle/gw_oracle.py's entropic_gromov_wasserstein, call for call, which also reports the range of the Gibbs
    exponent -> T, gw, (min, max) of 2 * tens / eps over the outer iterations ((0, 0) without one)."""
    from oracle import gw_oracle as o
    outer, sink = iters
    T = np.outer(p, q)
    constC, hC1, hC2 = o.init_matrix(C1, C2, p, q, loss)
    lo = hi = 0.0
    for _ in range(outer):
        M = 2.0 * o.tensor_product(constC, hC1, hC2, T)
        lo, hi = min(lo, float(M.min()) / eps), max(hi, float(M.max()) / eps)
        T = o.sinkhorn_knopp(p, q, M, eps, sink)
    return T, o.gwloss(constC, hC1, hC2, T), (lo, hi)


@functools.lru_cache(maxsize=None)
def _oracle_cached(n, m, kind, loss, eps, iters):
    from oracle import gw_oracle
    C1, C2, p, q = case_problem(n, m, kind)
    T, gw = gw_oracle.entropic_gromov_wasserstein(C1, C2, p, q, loss, eps, iters[0], iters[1])
    T.setflags(write=False)
    return T, gw


def case_oracle(case, iters):
    """oracle/gw_oracle.py on a listed case -> (T read-only, gw); computed once per (problem, loss, eps, iters), whatever
    the precision the device is asked for."""
    n, m, kind, loss, eps, _ = case
    return _oracle_cached(n, m, kind, loss, float(eps), tuple(iters))


# ----------------------------------------------------------------------------------------------------------- the bounds
U = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}


def gamma(k, u):
    return k * u / (1.0 - k * u)


def tens_delta(C1, C2, p, q, loss, prec, T=None):
    """delta[i][j] = (gamma_{n+2} + gamma_{m+2}) * S[i][j], S = |a_i| + |b_j| + (|hC1| |T| |hC2|^T)[i][j] (T: p q^T), in
    float64: what the device's a_i + b_j - (hC1 T hC2^T)[i][j] can lie from the exact value in precision `prec`.
    The k of gamma_k: one rounding of each operand entry to the precision (hC1, T, hC2: 3 in all, a_i and b_j: 1 each) and
    the n (first GEMM) and m (second GEMM) accumulation steps, in any order."""
    from oracle import gw_oracle as o
    n, m = len(p), len(q)
    _, hC1, hC2 = o.init_matrix(C1, C2, p, q, loss)
    f1, f2 =((lambda x: x ** 2), (lambda x: x ** 2)) if loss == "square_loss" else \
        ((lambda x: x * np.log(x + 1e-15) - x), (lambda x: x))
    a, b = f1(C1) @ p, f2(C2) @ q
    T = np.outer(p, q) if T is None else T
    S = np.abs(a)[:, None] + np.abs(b)[None, :] + np.abs(hC1) @ np.abs(T) @ np.abs(hC2).T
    return (gamma(n + 2, U[prec]) + gamma(m + 2, U[prec])) * S


def one_iter_bound(C1, C2, p, q, loss, eps, prec):
    """The relative bound on every plan entry after one outer and one Sinkhorn iteration (see test_gpu_gw_edges.py)."""
    n, m = len(p), len(q)
    delta = tens_delta(C1, C2, p, q, loss, prec)
    rho = float(np.expm1(2.0 * delta / eps).max()) + U[prec]
    return 2.0 * (5.0 * rho + 8.0 * gamma(max(n, m) + 2, U["f64"]))
