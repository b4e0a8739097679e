"""-m gpu: the EST builder (k_est / evrep_est_voxel / EventBatch.est_voxel / est.QuantizationLayer) against the float64 restatement
of tests/test_est_cpu.py, under the summation bound derived there from the kernel's number formats, and bit for bit where the
inputs make the image exact (the order of a cell's additions; the choice of the piece at, one ulp beside and far from the
breakpoints).  Every input is built and checked for selectivity on the CPU in tests/test_est_cpu.py.

Set EVREP_EST_RATIO_LOG to a file name to append the largest |got - sum64| / bound of every case (a record of how much of the
derived bound the kernel uses; never a threshold)."""
import os

import numpy as np
import pytest

from conftest import assert_bit_equal
from test_est_cpu import (BOUND_CASES, GOLDEN_EST, ORDER_CASES, STEP_RANGES, TABLES, WRAPPER_KINDS, _weights,
                          assert_within_summation_bound, est_terms, order_case, order_expected, selective_share, step_case,
                          step_expected, step_tables, trained_table, unit_table, wrapper_events, wrapper_restated_inputs)
from test_gpu_clustered import PASSES

pytestmark = pytest.mark.gpu


def _log(name, ratio):
    print("est bound used, %s: %.4f" % (name, ratio))
    path = os.environ.get("EVREP_EST_RATIO_LOG")
    if path:
        with open(path, "a") as f:
            f.write("%s %.6f\n" % (name, ratio))


def _event_batch(case, flags):
    import torch
    from event_representation_study_amd import engine as eng
    return eng.EventBatch(torch.from_numpy(case.rows).cuda(), torch.from_numpy(case.offsets), case.H, case.W, plan_flags=flags)


def _dev_table(tab):
    import torch
    return (torch.from_numpy(tab.seg).cuda(), torch.from_numpy(np.ascontiguousarray(tab.bucket, dtype=np.int32)).cuda())


def _run(eb, case, tab, dev=None):
    import torch
    seg, bucket = dev or _dev_table(tab)
    return eb.est_voxel(torch.from_numpy(case.tn).cuda(), case.C, seg, bucket, tab.lo, tab.hi).cpu().numpy()


@pytest.mark.parametrize("name", list(BOUND_CASES))
def test_est_within_the_summation_bound_under_every_pass(name):
    """frames 1x1 .. Gen1, B in {1, 3}, an empty and a one-event window, C in {2, 3, 4, 8}, both polarity encodings, uniform /
    circle / edges / hot-unit streams, the trained and a hand-made table: within the derived bound per cell, exactly 0 where no
    record fell, and the bound is selective (>= 99 % of the values exceed the bound of their cell)."""
    case = BOUND_CASES[name]()
    tab = TABLES[case.table]()
    r = est_terms(case.rows, case.offsets, case.tn, case.C, tab.seg, case.H, case.W)
    assert selective_share(r) >= 0.99
    dev = _dev_table(tab)
    first, worst = None, 0.0
    for pass_name, flags in PASSES.items():
        got = _run(_event_batch(case, flags), case, tab, dev)
        worst = max(worst, assert_within_summation_bound(got, r, "%s %s" % (name, pass_name)))
        if first is None:
            first = got
        else:
            assert_bit_equal(got, first, "%s: %s vs %s" % (name, pass_name, next(iter(PASSES))))
    _log(name, worst)


@pytest.mark.parametrize("name", list(ORDER_CASES))
def test_est_adds_in_array_order(name):
    """f = 1: the image is the float32 sum of the times in ARRAY order per cell (np.cumsum in float32), bit for bit, under every
    pass -- 1.0 followed by many 2^-25 and the reverse on neighbouring pixels, random magnitudes and their reverse, filler events
    in between, all timestamps equal; the long case puts 5000 records on one pixel (beyond every record stage)."""
    case = order_case(*ORDER_CASES[name])
    want = order_expected(case)
    tab = unit_table()
    for pass_name, flags in PASSES.items():
        assert_bit_equal(_run(_event_batch(case, flags), case, tab), want, "order %s %s" % (name, pass_name))


@pytest.mark.parametrize("C", [3, 8])
@pytest.mark.parametrize("lohi", STEP_RANGES)
def test_est_piece_selection_is_exact(C, lohi):
    """Step tables (f = k + 1 on piece k) and times in {0, 0.5, 1, m 2^-10}: every product and sum is exact, so the image is
    bit-equal whatever the order.  Breakpoints exactly at float32 u values that occur (u == breakpoint takes the NEXT piece), one
    float32 ulp above and below them, and on bucket edges; 1 / 2 / 300 pieces under 1 / 3 / 1000 / 4096 buckets (300 pieces under
    one bucket: the walk crosses every piece); u = lo and u = hi (bucket index nbucket, clamped) occur."""
    lo, hi = lohi
    case = step_case(C)
    ebs = {p: _event_batch(case, PASSES[p]) for p in ("auto", "classic")}
    for tname, tab in step_tables(C, lo, hi).items():
        want = step_expected(case, tab)
        for p, eb in ebs.items():
            assert_bit_equal(_run(eb, case, tab), want, "C=%d [%g, %g] %s %s" % (C, lo, hi, tname, p))


@pytest.mark.parametrize("kind", WRAPPER_KINDS)
def test_quantization_layer_voxel_edges(oracle, kind):
    """est.QuantizationLayer.voxel: a batch index that never occurs (an empty item in the middle), a single-event item (t_n = 1),
    an item whose times are all 0 (the reference divides 0 by 0: NaN at exactly the oracle's NaN cells) -- against
    oracle.est_voxel at the fixture's 1e-5 * scale and against est_restated under the summation bound."""
    import torch
    from event_representation_study_amd import est
    H, W, C = 17, 65, 5
    weights = _weights(np.load(GOLDEN_EST))
    ev = wrapper_events(kind, H, W)
    keep = ev.copy()
    tensor = torch.from_numpy(ev)
    layer = est.QuantizationLayer((C, H, W), est.PiecewiseLinearKernel(weights), image_size=None)
    got = layer.voxel(tensor).cpu().numpy()                              # (B, 2C, H, W)
    assert got.shape == (3, 2 * C, H, W) and got.dtype == np.float32
    assert np.array_equal(ev, keep)                                      # the caller's tensor (it shares ev's memory) is left alone
    with np.errstate(all="ignore"):
        want = oracle.est_voxel(keep, (C, H, W), weights)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and nan.any() == (kind == "zero_times")
    scale = np.abs(want[~nan]).max()
    assert np.abs(got.astype(np.float64) - want)[~nan].max() <= 1e-5 * scale
    rows, offs, tn = wrapper_restated_inputs(keep, H, W)
    tab = trained_table()
    r = est_terms(rows, offs, tn, C, tab.seg, H, W)
    assert selective_share(r) >= 0.99
    _log("wrapper " + kind, assert_within_summation_bound(np.ascontiguousarray(np.moveaxis(got, 1, -1)), r, "wrapper " + kind))
    if kind == "skipped_index":
        assert not got[1].any()


def test_quantization_layer_bin_counts():
    """C = 2 and C = 8 (16 channels: the whole of the builder's value array) are accepted and right; C = 1 and C = 9 raise."""
    import torch
    from event_representation_study_amd import est
    H, W = 17, 65
    kern = est.PiecewiseLinearKernel(_weights(np.load(GOLDEN_EST)))
    ev = wrapper_events("single_event", H, W)
    rows, offs, tn = wrapper_restated_inputs(ev, H, W)
    for C in (2, 8):
        got = est.QuantizationLayer((C, H, W), kern, image_size=None).voxel(torch.from_numpy(ev.copy())).cpu().numpy()
        r = est_terms(rows, offs, tn, C, trained_table().seg, H, W)
        _log("wrapper C=%d" % C, assert_within_summation_bound(np.ascontiguousarray(np.moveaxis(got, 1, -1)), r, "C=%d" % C))
    for C in (1, 9):
        with pytest.raises(ValueError):
            est.QuantizationLayer((C, H, W), kern, image_size=None)
