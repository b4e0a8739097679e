"""GPU: the average precision on the device (csrc/evrep_detap.hip through detector_eval.ap_device / ap_per_class /
DetectionEvaluator.compute_device) against the host restatement ap_host BIT FOR BIT on all eight outputs -- the device and
ap_host perform the same integer counts and the same float64 statements, tied confidences included (array order) -- with guard
bands around every output and the workspace; against the golden recorded from the reference's own ap_per_class and against
compute() under the bounds of test_detector_ap_cpu.py.

Shapes (detector_ap_cases.py): row counts around a wave, a workgroup, a scan tile (512) and a radix tile (2 048), 20 000 rows
for several workgroups and every digit, nc on both sides of the second class pass of the sort, T of 1, 10 and 16."""
import numpy as np
import pytest
import torch

from conftest import assert_bit_equal, load_golden
import detector_ap_cases as cases
from guarded import Arena
from test_detector_ap_cpu import AP_TOL, against_compute, against_reference, golden_inputs, golden_outputs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAMES = ("p", "r", "ap", "f1", "n_labels", "n_pred", "any_correct", "status")
ALL = cases.all_cases()


def _de():
    from event_representation_study_amd import detector_eval
    return detector_eval


def _inputs(case):
    tp, conf, pcls, tcls, nc = case
    return (torch.from_numpy(tp.astype(np.uint8)).to(DEV), torch.from_numpy(conf).to(DEV), torch.from_numpy(pcls).to(DEV),
            torch.from_numpy(tcls).to(DEV), nc)


def device(case, guarded=True, fill="random"):
    """ap_device's eight outputs as numpy (the two words as ints); guarded: every output and the workspace carved with bands."""
    de = _de()
    tp, conf, pcls, tcls, nc = _inputs(case)
    out = ws = arena = None
    if guarded:
        from event_representation_study_amd import _lib
        arena = Arena(DEV, seed=11)
        n, T = int(conf.shape[0]), int(tp.shape[1])
        f64, i64, i32 = torch.float64, torch.int64, torch.int32
        out = tuple(arena.carve_shape(shape, dtype, fill=fill, name=name) for name, shape, dtype in
                    (("p", (nc, _lib.AP_PX), f64), ("r", (nc, _lib.AP_PX), f64), ("ap", (nc, T), f64), ("f1", (nc, _lib.AP_PX), f64),
                     ("n_labels", (nc,), i64), ("n_pred", (nc,), i64), ("any_correct", (1,), i32), ("status", (1,), i32)))
        ws = arena.carve(de.ap_workspace_bytes(n, T, nc), fill=fill, name="workspace")
    got = de.ap_device(tp, conf, pcls, tcls, nc, out=out, workspace=ws)
    torch.cuda.synchronize()
    if arena is not None:
        arena.check()
    host = [t.cpu().numpy() for t in got]
    return tuple(host[:6]) + (int(host[6][0]), int(host[7][0]))


def equal(got, want, what):
    for g, w, name in zip(got, want, NAMES):
        assert_bit_equal(np.asarray(g), np.asarray(w), "%s %s" % (what, name))


@pytest.mark.parametrize("name", list(ALL))
def test_device_equals_ap_host(name):
    case = ALL[name]
    # (the poison: 0xFF bytes or pseudo-random ones; the large outputs of many classes get the one that is cheap to make)
    equal(device(case, fill="ones" if len(name) % 2 or case[4] > 80 else "random"), _de().ap_host(*case), name)


def test_two_runs_give_equal_bits():
    case = ALL["n20000_ties"]
    equal(device(case, guarded=False), device(case, guarded=False), "n20000_ties")


def test_nan_confidence_sets_its_bit_and_counts_hold():
    de = _de()
    case = cases.nan_conf_case()
    got, want = device(case), de.ap_host(*case)
    assert got[7] == want[7] == de.AP_ST_NAN_CONF
    for k in (4, 5, 6):
        assert_bit_equal(np.asarray(got[k]), np.asarray(want[k]), NAMES[k])


def test_counts_on_the_device_make_the_sizes_capacities():
    """n and m known on the device only: the rows and targets behind them are junk and must not be read into anything."""
    de = _de()
    tp, conf, pcls, tcls, nc = ALL["n513"]
    junk = cases.random_case(99, 700, levels=5)
    tp2, conf2, pcls2, tcls2 = (np.concatenate([a, b]) for a, b in zip((tp, conf, pcls, tcls), junk[:4]))
    pcls2[-3], tcls2[-1], conf2[-2] = 9.0, -1.0, np.nan
    counts = torch.tensor([conf.size, tcls.size], dtype=torch.int64, device=DEV)
    t = _inputs((tp2, conf2, pcls2, tcls2, nc))
    got = de.ap_device(*t, counts=counts)
    torch.cuda.synchronize()
    host = [x.cpu().numpy() for x in got]
    equal(tuple(host[:6]) + (int(host[6][0]), int(host[7][0])), de.ap_host(tp, conf, pcls, tcls, nc), "counts")


@pytest.mark.parametrize("name", cases.GOLDEN_NAMES)
def test_ap_per_class_on_cuda_tensors_equals_the_reference(name):
    g = load_golden("detector_ap")
    tp, conf, pcls, tcls, nc = golden_inputs(g, name)
    p, r, ap, f1, classes = _de().ap_per_class(torch.from_numpy(tp).to(DEV), torch.from_numpy(conf).to(DEV),
                                                torch.from_numpy(pcls).to(DEV), torch.from_numpy(tcls).to(DEV))
    wp, wr, wap, wf1, wclasses = golden_outputs(g, name)
    assert_bit_equal(classes, wclasses, name)
    assert_bit_equal(p, wp, name + " p")
    assert_bit_equal(r, wr, name + " r")
    assert_bit_equal(f1, wf1, name + " f1")
    assert np.abs(ap - wap).max() <= AP_TOL
    # the class list from host targets (no read for nc) and an explicit nc give the same
    again = _de().ap_per_class(torch.from_numpy(tp).to(DEV), torch.from_numpy(conf).to(DEV), torch.from_numpy(pcls).to(DEV), tcls, nc=nc)
    for a, b in zip(again, (p, r, ap, f1, classes)):
        assert_bit_equal(a, b, name)


def _evaluator(batches, nc=3, T=10, check=False, device=DEV):
    ev = _de().DetectionEvaluator(nc, iouv=np.linspace(0.5, 0.95, T).astype(np.float32), check=check)
    for b in batches:
        ev.add_batch(*(torch.from_numpy(t).to(device) for t in b))
    return ev


def test_compute_device_equals_compute():
    """Three small batches, B in {1, 4}, max_det 8 and 300, counts of 0, max_det and out of range, junk behind the counts,
    target rows of no image: tie-free by construction."""
    batches = cases.padded_batches(3)[:3]
    assert sorted({b[0].shape[0] for b in batches}) == [1, 4] and sorted({b[0].shape[1] for b in batches}) == [8, 300]
    ev = _evaluator(batches)
    got, want = ev.compute_device(), ev.compute()
    against_compute(got, want)
    cpu = _evaluator(batches, device="cpu").compute_device()
    for k in ("p", "r", "f1", "ap", "ap_class", "nt"):
        assert_bit_equal(got[k], cpu[k], k)


def test_compute_device_without_a_correct_prediction_and_with_status():
    ev = _evaluator(cases.padded_batches(4, fill="false"))
    assert ev.compute_device() == (0.0, 0.0) == ev.compute()
    batches = cases.padded_batches(5)
    batches[0][1][0, 0, 1] = 7.0
    batches[0][2][0] = 3
    with pytest.raises(ValueError, match="AP status 1"):
        _evaluator(batches, check=True).compute_device()


def test_update_then_compute_device():
    """Through the real chain: match_batch's launch per batch, then the device route, against compute()."""
    import detector_eval_cases as ec
    from test_detector_eval_cpu import eval_batch
    de = _de()
    ev = de.DetectionEvaluator(3)
    g = load_golden("detector_eval")
    for det, count, targets, shapes in (eval_batch(g, 0), eval_batch(g, 1)):
        ev.update(torch.from_numpy(det).to(DEV), torch.from_numpy(count).to(DEV), torch.from_numpy(targets).to(DEV), ec.IMG, shapes)
    got, want = ev.compute_device(), ev.compute()
    assert isinstance(want, dict) and isinstance(got, dict)
    # the declared rule, whatever the fixture's confidences do: ap_host on the rows compute() gathers, bit for bit
    host = [[t.cpu().numpy() for t in b] for b in ev._batches]
    tp, conf, pcls, tcls = de._gather_host(host, 10)
    p, r, ap, f1, n_labels = de.ap_host(tp, conf, pcls, tcls, 3)[:5]
    present = n_labels > 0
    for k, w in (("p", p[present]), ("r", r[present]), ("ap", ap[present]), ("f1", f1[present]), ("nt", n_labels)):
        assert_bit_equal(got[k], w, k)
    # and compute() itself: the fixture has no two rows of one class with equal confidence, so nothing is left open
    assert cases.tie_free((tp, conf, pcls, tcls, 3))
    against_compute(got, want)


def test_compute_device_at_the_gather_rounds():
    """The compaction's own rounds: 1023 / 1024 / 1025 / 2560 target rows of which a third name no image, 256 to 1100 images
    (detector_ap_cases.gather_edge_batches) -- against compute(), and bit for bit against the CPU route."""
    batches = cases.gather_edge_batches(6)
    ev = _evaluator(batches)
    got = ev.compute_device()
    against_compute(got, ev.compute())
    cpu = _evaluator(batches, device="cpu").compute_device()
    for k in ("p", "r", "f1", "ap", "ap_class", "nt"):
        assert_bit_equal(got[k], cpu[k], k)
    assert int(got["nt"].sum()) < sum(b[3].shape[0] for b in batches)
