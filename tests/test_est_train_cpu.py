"""CPU: the training path of the EST quantisation layer (est.ValueLayer, est.piece_coefficients, the C ABI of the backward)
and the float64 RESTATEMENT of the backward kernel (est_backward_restated) that tests/test_gpu_est_train.py compares k_est_bwd
with, together with every input of those GPU tests and their selectivity checks.

The arithmetic the kernel is held to (include/evrep.h): per event n and bin i, u = fl32(tn - fl32(i/(C-1))), piece k by the
forward's contract (the first piece with u < its end, else the last), g = G * tn exactly in float64, ga = fl64(g * u), and
grad[k] = (sum ga, sum g) in float64 in some fixed order.

Measured on the fixture (tests/golden/est_grad.npz), recorded in NOTES.md: the chain error and err32, see the tests below."""
import os
import re
from collections import namedtuple

import numpy as np
import pytest

from event_representation_study_amd.est import (PiecewiseLinearKernel, TrainableQuantizationLayer, ValueLayer,  # noqa: F401
                                                mlp_weights, piece_coefficients)           # (the feature: no module of this file loads without it)
from test_est_cpu import GOLDEN_EST, _weights, step_table, wrapper_restated_inputs

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN_GRAD = os.path.join(HERE, "golden", "est_grad.npz")
KEYS = ["mlp.%d.%s" % (i, n) for i in range(3) for n in ("weight", "bias")]
U64 = 2.0 ** -53
SLICE = 1024           # kEbSlice of evrep_est_bwd.hip: events per slice
CHAIN_LIMIT = 4 * 3.1e-9


@pytest.fixture(scope="module")
def grad_golden():
    return np.load(GOLDEN_GRAD)


@pytest.fixture(scope="module")
def est_golden():
    return np.load(GOLDEN_EST)


def loss_weights(shape, seed):
    """Wt of the fixture's loss (Wt * forward(events)).sum(): the statement of tests/golden/make_golden_est_grad.py"""
    return np.random.default_rng(int(seed)).standard_normal(tuple(shape), dtype=np.float32)


def state_of(g):
    return {k[2:]: g[k] for k in g.files if k.startswith("w_")}


# ---------------------------------------------------------------------------------------------------------------------
# The restatement
# ---------------------------------------------------------------------------------------------------------------------
BackRestated = namedtuple("BackRestated", "grad abs count")


def est_backward_restated(rows, offsets, tn, C, ends, H, W, G):
    """rows (N, 4) [x, y, t, p], offsets (B + 1,), tn (N,) float32, ends (nseg,) float64 ascending, G (B, H, W, 2C) float32 ->
    BackRestated(grad (nseg, 2) float64 {dL/da, dL/dc}, abs = the same sums of magnitudes, count (nseg,) terms per piece).
    Events outside the frame or with p not in {0, 1} contribute nothing.  Sums by np.bincount (float64, array order)."""
    rows, offsets, tn, G = np.asarray(rows), np.asarray(offsets, dtype=np.int64), np.asarray(tn), np.asarray(G)
    ends = np.asarray(ends, dtype=np.float64)
    assert tn.dtype == np.float32 and G.dtype == np.float32 and G.shape == (len(offsets) - 1, H, W, 2 * C)
    nseg = len(ends)
    b = np.repeat(np.arange(len(offsets) - 1, dtype=np.int64), np.diff(offsets))
    x, y, p = (rows[:, j].astype(np.int64) for j in (0, 1, 3))
    ok = (x >= 0) & (x < W) & (y >= 0) & (y < H) & ((p == 0) | (p == 1))
    b, x, y, p, t32 = b[ok], x[ok], y[ok], p[ok], tn[ok]
    shift = np.array([np.float32(i / (C - 1)) for i in range(C)], dtype=np.float32)
    u = (t32[:, None] - shift[None, :]).astype(np.float32).astype(np.float64)
    k = np.minimum(np.searchsorted(ends, u, side="right"), nseg - 1)
    cell = (((b * H + y) * W + x) * 2 * C + p * C)[:, None] + np.arange(C, dtype=np.int64)[None, :]
    g = G.reshape(-1)[cell].astype(np.float64) * t32.astype(np.float64)[:, None]       # exact: 24 x 24 bits
    ga = g * u                                                                          # one float64 rounding
    kf = k.reshape(-1)
    grad = np.stack([np.bincount(kf, weights=ga.reshape(-1), minlength=nseg), np.bincount(kf, weights=g.reshape(-1), minlength=nseg)], axis=1)
    mag = np.stack([np.bincount(kf, weights=np.abs(ga).reshape(-1), minlength=nseg),
                    np.bincount(kf, weights=np.abs(g).reshape(-1), minlength=nseg)], axis=1)
    return BackRestated(grad, mag, np.bincount(kf, minlength=nseg))


def gamma64(m):
    m = np.asarray(m, dtype=np.float64)
    return m * U64 / (1.0 - m * U64)


def backward_bound(r):
    """Piece k is the float64 sum of n_k terms in some order: at most n_k - 1 roundings on any chain, one more for the product
    g * u, and one spare: |got - sum| <= gamma(n_k + 2) * sum |terms|.  Nothing here is measured on the kernel."""
    return gamma64(r.count + 2.0)[:, None] * r.abs


def assert_within_backward_bound(got, r, what=""):
    """got (nseg, 2) float64: exactly 0 at the pieces no term fell into, within the bound elsewhere.  Returns the largest
    |got - sum| / bound (a record, never a threshold)."""
    got = np.asarray(got)
    assert got.dtype == np.float64 and got.shape == r.grad.shape, (what, got.dtype, got.shape)
    empty = r.count == 0
    assert not got[empty].any() and not np.signbit(got[empty]).any(), "%s: a piece without a term is not +0.0" % what
    err, bound = np.abs(got - r.grad), backward_bound(r)
    bad = err > bound
    assert not bad.any(), "%s: %d of %d sums beyond the bound, worst %.3e > %.3e" % (
        what, int(bad.sum()), bad.size, err[bad].max(), bound[bad].min())
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.where(bound > 0, err / bound, 0.0).max())


def backward_selective_share(r):
    """Share of the non-empty pieces whose |d/da| and |d/dc| both exceed their bound: a dropped or doubled term there shows."""
    live = r.count > 0
    return float((np.abs(r.grad[live]) > backward_bound(r)[live]).all(axis=1).mean()) if live.any() else 1.0


# ---------------------------------------------------------------------------------------------------------------------
# Inputs of the GPU tests
# ---------------------------------------------------------------------------------------------------------------------
BackCase = namedtuple("BackCase", "rows offsets tn C H W table G")
EXACT_COUNTS = (1, 63, 64, 65, SLICE, SLICE + 1, 3 * SLICE + 1)
EXACT_H, EXACT_W = 5, 7


def _offsets(sizes):
    offs = np.zeros(len(sizes) + 1, dtype=np.int64)
    np.cumsum(sizes, out=offs[1:])
    return offs


def exact_case(n, C, nseg, layout, seed=0):
    """Frame 5x7, B = 3 with an empty middle window (n events split 2:0:1, at least one in the first), tn multiples of 2^-10, C in
    {2, 3, 5} (shifts i/(C-1) dyadic: u is exact), G small integers: every g = G tn is a multiple of 2^-10 below 2^4, every
    ga = g u a multiple of 2^-20 (2^-12 for C = 5) below 2^4, every partial sum stays below 2^53 units: exact whatever the order.
    layout 'one_pixel': every event on pixel (3, 2), polarity 1; 'own_piece': the times walk through the table so that
    neighbouring events fall into different pieces (for 300 pieces: 64 distinct pieces in most batches of 64)."""
    assert C in (2, 3, 5)
    rng = np.random.default_rng(1000 * n + 10 * C + seed)
    n0 = max(1, (2 * n) // 3)
    offs = _offsets([n0, 0, n - n0])
    rows = np.zeros((n, 4), dtype=np.int32)
    if layout == "one_pixel":
        rows[:, 0], rows[:, 1], rows[:, 3] = 3, 2, 1
        tn = (rng.integers(0, 1025, size=n) * 2.0 ** -10).astype(np.float32)
    else:
        rows[:, 0], rows[:, 1], rows[:, 3] = rng.integers(0, EXACT_W, n), rng.integers(0, EXACT_H, n), rng.integers(0, 2, n)
        tn = (((np.arange(n) * 37) % 1025) * 2.0 ** -10).astype(np.float32)       # 37 / 1024 per step: a new piece of 300 each event
    tab = step_table(C, nseg, 64, -1.0, 1.0, "mixed", seed=seed)
    G = rng.integers(-8, 9, size=(3, EXACT_H, EXACT_W, 2 * C)).astype(np.float32)
    return BackCase(rows, offs, tn, C, EXACT_H, EXACT_W, tab, G)


def general_case(kind, C, seed=0):
    """17x65, the 300-piece table, B = 3 (one window empty), ~9000 events (nine slices): 'uniform' = ascending random times,
    'tied' = times from a set of 400 values (runs of equal times: one piece per batch and bin, exact ties), 'descending' = the last window's times fall."""
    H, W = 17, 65
    rng = np.random.default_rng(77 + seed + C)
    sizes = [5000, 0, 4001]
    n = sum(sizes)
    rows = np.zeros((n, 4), dtype=np.int32)
    rows[:, 0], rows[:, 1], rows[:, 3] = rng.integers(0, W, n), rng.integers(0, H, n), rng.integers(0, 2, n)
    offs = _offsets(sizes)
    tn = np.zeros(n, dtype=np.float32)
    for s, e in zip(offs[:-1], offs[1:]):
        if e > s:
            t = np.sort(rng.choice(rng.random(400), size=e - s)) if kind == "tied" else np.sort(rng.random(e - s))
            t = (t / t.max()).astype(np.float32)
            tn[s:e] = t[::-1] if (kind == "descending" and s > 0) else t
    tab = step_table(C, 300, 64, -1.0, 1.0, "mixed", seed=seed)
    G = rng.standard_normal((3, H, W, 2 * C)).astype(np.float32)
    return BackCase(rows, offs, tn, C, H, W, tab, G)


GENERAL = [(kind, C) for kind in ("uniform", "tied", "descending") for C in (2, 8)]


def restate(case):
    return est_backward_restated(case.rows, case.offsets, case.tn, case.C, case.table.seg[:, 0], case.H, case.W, case.G)


# ---------------------------------------------------------------------------------------------------------------------
# float64 autograd through the MLP itself (the truth of the chain test and of the fixture's float64 run)
# ---------------------------------------------------------------------------------------------------------------------
def mlp_autograd(state, rows, offsets, tn, C, H, W, G):
    """dL/dweights for L = sum G * vox, vox from f = the MLP in float64 torch on u = fl32(tn - shift) -> {key: array}"""
    import torch
    from event_representation_study_amd.est import ValueLayer
    vl = ValueLayer(state).double()
    shift = np.array([np.float32(i / (C - 1)) for i in range(C)], dtype=np.float32)
    u = torch.from_numpy((tn[:, None] - shift[None, :]).astype(np.float32).astype(np.float64))
    b = np.repeat(np.arange(len(offsets) - 1, dtype=np.int64), np.diff(offsets))
    cell = (((b * H + rows[:, 1]) * W + rows[:, 0]) * 2 * C + rows[:, 3] * C)[:, None] + np.arange(C)[None, :]
    w = torch.from_numpy(G.reshape(-1)[cell].astype(np.float64) * tn.astype(np.float64)[:, None])
    (w * vl(u)).sum().backward()
    return {k: p.grad.numpy() for k, p in vl.named_parameters()}


def table_chain(state, grad_seg, kernel):
    """(dL/da, dL/dc) pushed through est.piece_coefficients -> {key: array}"""
    import torch
    from event_representation_study_amd.est import ValueLayer, piece_coefficients
    vl = ValueLayer(state).double()
    a, c = piece_coefficients([p for _, p in vl.named_parameters()], kernel)
    torch.autograd.backward([a, c], [torch.from_numpy(np.ascontiguousarray(grad_seg[:, 0])), torch.from_numpy(np.ascontiguousarray(grad_seg[:, 1]))])
    return {k: p.grad.numpy() for k, p in vl.named_parameters()}


def rel_err(got, want):
    """per tensor: the largest |got - want| over the largest |want|"""
    return {k: float(np.abs(np.asarray(got[k], dtype=np.float64) - want[k]).max() / np.abs(want[k]).max()) for k in KEYS}


# ---------------------------------------------------------------------------------------------------------------------
# Tests
# ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_lib_binds_the_backward():
    from event_representation_study_amd import _lib
    header = open(os.path.join(ROOT, "include", "evrep.h")).read()
    for name in ("evrep_est_backward_scratch_bytes", "evrep_est_voxel_backward"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.SYMBOLS
    assert int(re.search(r"#define\s+EVREP_EST_BWD_MAX_SEG\s+(\d+)", header).group(1)) == _lib.EST_BWD_MAX_SEG == 8192
    assert len(_lib.SYMBOLS["evrep_est_voxel_backward"][1]) == 17
    lib = _lib.load()
    assert lib.evrep_est_backward_scratch_bytes(0, 8193) == 0 and lib.evrep_est_backward_scratch_bytes(-1, 10) == 0
    small, big = lib.evrep_est_backward_scratch_bytes(1, 97), lib.evrep_est_backward_scratch_bytes(10 ** 9, 97)
    assert 0 < small < big and big == lib.evrep_est_backward_scratch_bytes(10 ** 10, 97)      # the rows are capped


def test_backward_refuses_bad_arguments_without_a_gpu():
    """every refusal comes before any launch, so it can be seen on a machine without a device"""
    import ctypes
    from event_representation_study_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 255) & ~255)

    def call(nseg=10, C=3, grad_out=p, lo=-1.0, hi=1.0, events=p, grad_seg=p):
        return lib.evrep_est_voxel_backward(events, p, 1, 4, 4, p, C, p, nseg, p, 8, lo, hi, grad_out, grad_seg, p, None)
    for kw in (dict(nseg=_lib.EST_BWD_MAX_SEG + 1), dict(nseg=0), dict(C=9), dict(C=1), dict(grad_out=None), dict(hi=-1.0),
               dict(events=None), dict(grad_seg=None)):
        assert call(**kw) == _lib.EVREP_EINVAL, kw


def test_piece_coefficients_equal_the_kernels_bit_for_bit(est_golden):
    import torch
    from event_representation_study_amd.est import PiecewiseLinearKernel, ValueLayer, piece_coefficients
    state = {k[2:]: est_golden[k] for k in est_golden.files if k.startswith("w_")}
    for vl in (ValueLayer(state), ValueLayer.from_trilinear(6)):
        from event_representation_study_amd.est import mlp_weights
        k = PiecewiseLinearKernel(mlp_weights(vl))
        a, c = piece_coefficients([p for _, p in vl.named_parameters()], k)
        assert a.dtype == torch.float64 and a.requires_grad and c.requires_grad
        assert np.array_equal(a.detach().numpy().view(np.uint64), k.a.view(np.uint64))
        assert np.array_equal(c.detach().numpy().view(np.uint64), k.c.view(np.uint64))


def test_piece_coefficients_gradient_is_the_adjoint_of_its_formulas(est_golden):
    """the hand-written adjoint against torch autograd through the same formulas in float64 torch, masks as constants: both are
    sums of <= 100 x 100 products in another order, so they agree to float64 rounding of the largest entry (1e-12: 10^4 terms x 2^-53)"""
    import torch
    from event_representation_study_amd.est import PiecewiseLinearKernel, ValueLayer, mlp_weights, piece_coefficients
    vl = ValueLayer({k[2:]: est_golden[k] for k in est_golden.files if k.startswith("w_")}).double()
    k = PiecewiseLinearKernel(mlp_weights(vl))
    rng = np.random.default_rng(3)
    ga, gc = torch.from_numpy(rng.standard_normal(len(k))), torch.from_numpy(rng.standard_normal(len(k)))
    params = [p for _, p in vl.named_parameters()]
    a, c = piece_coefficients(params, k)
    mine = torch.autograd.grad([a, c], params, [ga, gc])
    w1, b1, W2, b2, w3, b3 = (p.reshape(s) for p, s in zip(params, ((-1,), (-1,), (100, 100), (-1,), (-1,), (1,))))
    mids = torch.from_numpy(0.5 * (k.edges[:-1] + k.edges[1:]))
    with torch.no_grad():
        one, slope = torch.tensor(1.0, dtype=torch.float64), torch.tensor(k.slope, dtype=torch.float64)
        a1 = torch.where(torch.outer(mids, w1) + b1 > 0, one, slope)
    A2, B2 = (a1 * w1) @ W2.T, (a1 * b1) @ W2.T + b2
    a2 = torch.where(A2.detach() * mids[:, None] + B2.detach() > 0, one, slope)
    ta, tc = (a2 * A2) @ w3, (a2 * B2) @ w3 + b3
    assert np.abs(ta.detach().numpy() - k.a).max() <= 1e-12 * np.abs(k.a).max()
    theirs = torch.autograd.grad([ta, tc], params, [ga, gc])
    for m, t in zip(mine, theirs):
        assert m.shape == t.shape and float((m - t).abs().max()) <= 1e-12 * float(t.abs().max())


def test_chain_gradient_matches_autograd_through_the_mlp(grad_golden):
    """est_backward_restated -> piece_coefficients against float64 autograd through the MLP itself, on the fixture, both image
    sizes' voxel-level problem (G = Wt for image_size None).  Limit: the 3.1e-9 of the largest entry measured when the identity
    was derived, times 4 (which events sit within rounding of a breakpoint changes with the stream).  Measured here: 4.4e-15 (the restatement and the MLP see the same float32-rounded u)."""
    from event_representation_study_amd.est import PiecewiseLinearKernel, mlp_weights
    g = grad_golden
    C, H, W = (int(v) for v in g["dim"])
    state = state_of(g)
    rows, offs, tn = wrapper_restated_inputs(g["events"], H, W)
    G = np.ascontiguousarray(np.moveaxis(loss_weights((3, 2 * C, H, W), g["seed"]), 1, -1))
    kern = PiecewiseLinearKernel(mlp_weights(state))
    assert len(kern) == 97
    r = est_backward_restated(rows, offs, tn, C, kern.edges[1:], H, W, G)
    err = rel_err(table_chain(state, r.grad, kern), mlp_autograd(state, rows, offs, tn, C, H, W, G))
    print("chain error per tensor:", {k: "%.2e" % v for k, v in err.items()})
    assert max(err.values()) <= CHAIN_LIMIT, err


def err32_of(g, size):
    """per tensor: the largest |float32-run gradient - float64-run gradient| over the largest |float64-run gradient|"""
    return rel_err({k: g["grad_f32_%d_%s" % (size, k)] for k in KEYS}, {k: g["grad_f64_%d_%s" % (size, k)] for k in KEYS})


def test_fixture_sanity(grad_golden):
    """the two runs of the reference describe the same gradient: err32 is float32 rounding (recorded in NOTES.md), the float64
    run for image_size None is autograd through the MLP on the restated inputs, and the gradients are not trivially zero"""
    g = grad_golden
    C, H, W = (int(v) for v in g["dim"])
    for size in (96, 0):
        e = err32_of(g, size)
        print("err32, image_size %s:" % (size or None), {k: "%.2e" % v for k, v in e.items()})
        assert 0 < max(e.values()) < 1e-3            # float32 accumulation over 8000 x 6 terms, far from a different gradient
        assert all(np.abs(g["grad_f64_%d_%s" % (size, k)]).max() > 0 for k in KEYS)
    rows, offs, tn = wrapper_restated_inputs(g["events"], H, W)
    G = np.ascontiguousarray(np.moveaxis(loss_weights((3, 2 * C, H, W), g["seed"]), 1, -1))
    mine = mlp_autograd(state_of(g), rows, offs, tn, C, H, W, G)
    # the reference's float64 run rounds nothing to float32 (its u is a float64 difference of float64 times): it differs from
    # the restated inputs by the float32 rounding of tn and u, 2^-24 relative per term
    assert max(rel_err(mine, {k: g["grad_f64_0_%s" % k] for k in KEYS}).values()) <= 1e-5


def test_value_layer_round_trips_the_state_dict(grad_golden):
    import torch
    from event_representation_study_amd.est import ValueLayer, mlp_weights
    state = state_of(grad_golden)
    vl = ValueLayer(state)
    assert isinstance(vl.mlp, torch.nn.ModuleList) and all(isinstance(m, torch.nn.Linear) for m in vl.mlp)
    sd = vl.state_dict()
    assert sorted(sd) == sorted(KEYS) and all(np.array_equal(sd[k].numpy(), state[k]) for k in KEYS)
    for a, b in zip(mlp_weights(vl), mlp_weights(state)):
        assert np.array_equal(a, b)
    again = ValueLayer()
    again.load_state_dict(sd)
    u = torch.linspace(-1, 1, 101)
    assert torch.equal(again(u), vl(u))


@pytest.mark.parametrize("C", [2, 6, 8])
def test_from_trilinear_reproduces_the_trilinear_kernel(C):
    """at its own grid: the kinks 0 and +-1/(C-1), the bin centres i/(C-1) - j/(C-1), and points between them.  The closed form is
    exact up to the float32 storage of 1/0.99, 0.1/0.99, 1/1.1: <= 12 products of <= 3 rounded factors and magnitude <= 2(C-1) + 2"""
    from event_representation_study_amd.est import PiecewiseLinearKernel, ValueLayer, mlp_weights, trilinear_kernel
    vl = ValueLayer.from_trilinear(C)
    kern = PiecewiseLinearKernel(mlp_weights(vl))
    grid = np.unique(np.concatenate([np.arange(-(C - 1), C) / (C - 1), np.arange(-2 * (C - 1), 2 * C - 1) / (2.0 * (C - 1)),
                                     np.linspace(-1, 1, 201)]))
    bound = 12 * 3 * 2.0 ** -24 * (2 * (C - 1) + 2)
    assert np.abs(kern.mlp(grid) - trilinear_kernel(grid, C)).max() <= bound
    assert np.abs(kern(grid) - trilinear_kernel(grid, C)).max() <= bound
    assert 2 <= len(kern) <= 8          # kinks at 0 and +-1/(C-1) (C = 2: those are the ends of the range)


def test_trainable_layer_names_the_limit(monkeypatch):
    from event_representation_study_amd import _lib, est
    layer = est.TrainableQuantizationLayer((6, 4, 4), est.ValueLayer.from_trilinear(6), image_size=None, device="cpu")
    assert sorted(layer.state_dict()) == sorted("value_layer." + k for k in KEYS)
    monkeypatch.setattr(_lib, "EST_BWD_MAX_SEG", 2)
    with pytest.raises(ValueError, match="EVREP_EST_BWD_MAX_SEG"):
        layer.table()


@pytest.mark.parametrize("layout", ["one_pixel", "own_piece"])
def test_exact_inputs_are_exact(layout):
    """every term of the exact cases is a multiple of 2^-20 below 2^5 and the sums of magnitudes stay below 2^32: any order of
    float64 additions is exact.  The own-piece layout of 300 pieces puts >= 32 distinct pieces into a batch of 64."""
    for n in EXACT_COUNTS:
        for C in (2, 3, 5):
            for nseg in (1, 2, 300):
                case = exact_case(n, C, nseg, layout)
                assert case.offsets[1] == case.offsets[2] and case.offsets[-1] == n
                r = restate(case)
                assert np.all(r.grad * 2.0 ** 20 == np.rint(r.grad * 2.0 ** 20)) and r.abs.max() < 2.0 ** 32
                assert r.count.sum() == n * C
    case = exact_case(3 * SLICE + 1, 5, 300, "own_piece")
    u = (case.tn[:64] - np.float32(0.25)).astype(np.float64)
    assert len(np.unique(np.searchsorted(case.table.seg[:, 0], u, side="right"))) >= 32
    assert (restate(case).count == 0).any()           # some pieces stay untouched: they must hold exact zeros


@pytest.mark.parametrize("kind,C", GENERAL)
def test_general_inputs_are_selective(kind, C):
    case = general_case(kind, C)
    r = restate(case)
    assert backward_selective_share(r) >= 0.99, backward_selective_share(r)
    assert assert_within_backward_bound(r.grad, r) == 0.0
    if kind == "descending":
        s = case.offsets[2]
        assert np.all(np.diff(case.tn[s:]) <= 0) and case.tn[s] == 1.0
