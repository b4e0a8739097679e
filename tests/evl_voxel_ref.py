"""The normalisation of ev-licious' events_to_voxel_grid restated in numpy (include/evrep.h, evrep_voxel_normalize), and the
bound that any other order of the two float64 sums keeps to it.  Shared by test_evl_voxel_batch_cpu.py and
test_gpu_evl_voxel_batch.py; nothing here touches a device.

The restatement, for one window of any layout, with v = float32(grid):
    n = #{v != 0};  mean = fsum(v[nz]) / n;  std = sqrt(fsum((float64(v[nz]) - mean)^2) / n)
    n > 0 and std > 0:  out = float32((float64(v) - mean) / (1e-5 + std)) at nz, +0 elsewhere;  otherwise out = v.

The bound (u = 2^-53, gamma(k) = k u / (1 - k u); A = sum |v[nz]|; every quantity below with index r is the restatement's):
  * Any order of n float64 additions is within gamma(n-1) A of the exact sum s, math.fsum within u |s| <= u A.  One division
    each: the two means are within gamma(n) A/n and gamma(2) A/n of s/n, so
        E_m = gamma(n + 2) A / n                                     >= |mean - mean_r|.
  * Q(m) = sum (v - m)^2 = Q(s/n) + n (m - s/n)^2, so the EXACT sums of squares about the two means differ by at most n E_m^2,
    their square roots sigma (>= the true sigma) by at most E_m^2 / (2 sigma).  Computed: a term takes three roundings
    (subtract, multiply; gamma(3) with the one of the sum it enters), n non-negative terms in any order gamma(n-1), the
    division by n one, a square root within one unit in the last place two: relative gamma(n + 5) here, gamma(6) for the
    restatement (fsum: one rounding; numpy's sqrt is correctly rounded).  The square root halves a relative error; that is not
    used.  With a factor two for the products of these small terms
        E_s = 2 gamma(n + 11) std_r + E_m^2 / std_r                  >= |std - std_r|.
  * Numerator N = fl(v - mean): |N - N_r| <= E_m + u (|N| + |N_r|); denominator D = fl(1e-5 + std): |D - D_r| <= E_s + u (D + D_r);
    quotient q = fl(N / D).  |N/D - N_r/D_r| <= |N - N_r| / D + |q_r| |D - D_r| / D, and D differs from D_r by a relative E_s / D_r;
    with a factor two for that and the other second-order terms
        E_q = 2 (E_m / D_r + |q_r| E_s / D_r + 6 u |q_r|)             >= |q - q_r|.
  * Rounding to float32 moves each side by at most 2^-24 of itself (2^-150 below the normal range):
        tol = E_q (1 + 2^-24) + 2^-23 |q_r| + 2^-149                  >= |out - out_r|   at the non-zero elements;
    elsewhere, and in a window that is not normalised, out == out_r exactly.
"""
import math

import numpy as np

U = 2.0 ** -53


def gamma(k):
    return k * U / (1.0 - k * U)


def restate(grid, normalize=True):
    """-> (out float32 of grid's shape, stats dict(n, mean, std, applied), tol float64 of grid's shape: the bound above, 0 where
    the result is exact)."""
    v = np.asarray(grid).astype(np.float32)
    tol = np.zeros(v.shape, np.float64)
    nz = v != 0
    n = int(nz.sum())
    stats = dict(n=n, mean=0.0, std=0.0, applied=0, e_mean=0.0, e_std=0.0)
    if not normalize or n == 0:
        return v, stats, tol
    vals = v[nz].astype(np.float64)
    mean = math.fsum(vals.tolist()) / n
    dev = vals - mean
    std = math.sqrt(math.fsum((dev * dev).tolist()) / n)
    A = float(np.abs(vals).sum()) * (1 + gamma(n))            # (an upper bound of A)
    e_m = gamma(n + 2) * A / n
    stats.update(mean=mean, std=std, e_mean=e_m)
    if not std > 0:
        return v, stats, tol
    e_s = 2 * gamma(n + 11) * std + e_m * e_m / std
    den = 1e-5 + std
    q = dev / den
    e_q = 2 * (e_m / den + np.abs(q) * e_s / den + 6 * U * np.abs(q))
    out = np.zeros(v.shape, np.float32)
    out[nz] = q.astype(np.float32)
    tol[nz] = e_q * (1 + 2.0 ** -24) + 2.0 ** -23 * np.abs(q) + 2.0 ** -149
    stats.update(applied=1, e_std=e_s)
    return out, stats, tol


def assert_matches_restatement(got, stats_got, grid, what=""):
    """got: the kernel's window in grid's layout; stats_got: its {n, mean, std, applied} row or None."""
    want, st, tol = restate(grid, True)
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape)
    assert np.array_equal(got == 0, want == 0), what + ": zero pattern"
    exact = tol == 0
    assert np.array_equal(got[exact].view(np.uint32), want[exact].view(np.uint32)), what + ": elements that take no arithmetic"
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    worst = float((err - tol).max()) if err.size else 0.0
    print("%s: n=%d max|diff|=%.3g max bound=%.3g bit-equal=%.4f" % (what, st["n"], float(err.max()) if err.size else 0.0,
                                                                    float(tol.max()) if tol.size else 0.0,
                                                                    float((got.view(np.uint32) == want.view(np.uint32)).mean())))
    assert worst <= 0, "%s: %g beyond the bound" % (what, worst)
    if stats_got is not None:
        n, mean, std, applied = (float(x) for x in stats_got)
        assert n == st["n"] and applied == st["applied"], (what, n, applied, st)
        assert abs(mean - st["mean"]) <= st["e_mean"], (what, mean, st)
        assert abs(std - st["std"]) <= st["e_std"], (what, std, st)
    return st
