"""GPU: the batched non_max_suppression (csrc/evrep_nms.hip through detector_output.nms_batch / non_max_suppression) against the
host restatement nms_host and against the golden recorded from the reference's own function, bit for bit: the rows, the counts
and the zero tail.  No tolerance anywhere -- the device and nms_host perform the same float32 statements.

Shapes: B in {1, 3}, N <= 1100, C in {1, 2, 3, 80}.  The kernel sweeps boxes in rounds of 1024, sorts in chunks of 4096 pairs
and runs the greedy pass in rounds of 1024 rows, a wave of 64 at a time: survivor counts sit on both sides of 64, 256 and 1024,
and kept counts cross the multiples of 64 and the round at 1024."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import assert_bit_equal, load_golden
import detector_output_cases as cases
from guarded import FILLS, Arena
from test_detector_output_cpu import golden_kwargs, golden_names

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = np.float32


def _do():
    from event_representation_study_amd import detector_output
    return detector_output


def check(pred, what="", **kw):
    """nms_batch on the device == nms_host, padded: rows, counts, zero tail.  Returns the host rows."""
    do = _do()
    max_det = kw.get("max_det", 300)
    want_det, want_count = cases.pad(do.nms_host(pred, **kw), max_det)
    det, count = do.nms_batch(torch.from_numpy(pred).to(DEV), **kw)
    assert det.dtype == torch.float32 and count.dtype == torch.int32 and tuple(det.shape) == want_det.shape
    assert_bit_equal(count.cpu().numpy(), want_count, what + " count")
    assert_bit_equal(det.cpu().numpy(), want_det, what + " det")
    return want_det, want_count


# ------------------------------------------------------------------------------------------------ the golden, the settings
@pytest.mark.parametrize("name", golden_names())
def test_device_equals_the_reference(name):
    g = load_golden("detector_output")
    kw = golden_kwargs(g, name)
    det, count = _do().nms_batch(torch.from_numpy(g[name + "/pred"]).to(DEV), **kw)
    assert_bit_equal(count.cpu().numpy(), g[name + "/count"], name)
    assert_bit_equal(det.cpu().numpy(), g[name + "/det"], name)


SETTINGS = {"evaler": dict(conf_thres=0.03, iou_thres=0.65, multi_label=True), "inferer": dict(conf_thres=0.25, iou_thres=0.45),
            "agnostic_multi": dict(conf_thres=0.25, iou_thres=0.45, multi_label=True, agnostic=True),
            "classes1": dict(conf_thres=0.1, iou_thres=0.5, multi_label=True, classes=[1]),
            "classes_none_listed": dict(conf_thres=0.1, iou_thres=0.5, classes=[])}


@pytest.mark.parametrize("setting", sorted(SETTINGS))
@pytest.mark.parametrize("shape", [(3, 1100, 3), (1, 1025, 1), (3, 333, 2), (1, 300, 80)], ids=lambda s: "B%d_N%d_C%d" % s)
def test_head_outputs(shape, setting):
    B, N, C = shape
    pred = cases.head_output(B * 1000 + N + C, B, N, C, lo=-0.5 if C == 80 else 0.0)
    _, count = check(pred, "%s %s" % (shape, setting), **SETTINGS[setting])
    assert setting == "classes_none_listed" or (C == 1 and setting == "classes1") or count.min() > 0


# ------------------------------------------------------------------------------------------------ step (a)
@pytest.mark.parametrize("multi", [False, True], ids=["single", "multi"])
def test_candidate_edges(multi):
    """No candidate beside full images, every row a candidate, NaN obj / cls, values equal to ct, products below ct."""
    pred = cases.edges_of_candidates()
    _, count = check(pred, "edges", conf_thres=0.25, iou_thres=0.45, multi_label=multi)
    assert count[0] == (128 if multi else 64) and count[1] == 0 and 0 < count[2] < count[0]
    lone = np.zeros((1, 5, 7), F32)
    check(lone, "no candidate at all", conf_thres=0.25, iou_thres=0.45, multi_label=multi)


def test_threshold_is_compared_in_float32():
    _, count = check(cases.float32_threshold_rows(), "0.1", conf_thres=0.1, iou_thres=0.45)
    assert count.tolist() == [6]


@pytest.mark.parametrize("N,C", [(1100, 1), (1100, 3), (300, 80)])
def test_every_row_a_candidate(N, C):
    pred = cases.head_output(5, 1, N, C, lo=0.6)
    _, count = check(pred, "all candidates", conf_thres=0.25, iou_thres=0.45, multi_label=True, max_det=1024)
    assert count[0] > 64


# ------------------------------------------------------------------------------------------------ step (b)
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1024, 1025])
def test_survivor_counts(n):
    """Exactly n rows reach the sort; disjoint boxes, so all are kept: the kept count crosses every multiple of 64 up to
    max_det, where the pass stops."""
    pred = cases.survivors(n)
    _, count = check(pred, "n=%d" % n, conf_thres=0.25, iou_thres=0.45, max_det=1024)
    assert count.tolist() == [min(n, 1024)]
    _, count = check(pred, "n=%d max_det 300" % n, conf_thres=0.25, iou_thres=0.45)
    assert count.tolist() == [min(n, 300)]


def test_duplicate_scores_are_ordered_by_index():
    for multi in (False, True):
        check(cases.duplicates(), "duplicates", conf_thres=0.25, iou_thres=0.45, multi_label=multi)
    pred = cases.survivors(700, distinct=False)                        # 700 equal scores on disjoint boxes: index order
    det, _ = check(pred, "equal scores", conf_thres=0.25, iou_thres=0.45, max_det=1024)
    where = np.flatnonzero(pred[0, :, 4] > 0)
    assert_bit_equal(det[0, :700, 0], pred[0, where, 0] - F32(5))


@pytest.mark.parametrize("n", [49, 50, 51])
def test_max_nms_cut(n):
    """(No tie anywhere in these scores: the reference leaves ties at the cut open, the device takes the lower row first.)"""
    pred = cases.cut_rows(n)
    check(pred, "max_nms", conf_thres=0.25, iou_thres=0.45, max_nms=50)
    check(pred, "max_nms 1", conf_thres=0.25, iou_thres=0.45, max_nms=1)


def test_single_label_takes_the_first_maximum():
    det, _ = check(cases.argmax_tie(), "argmax", conf_thres=0.25, iou_thres=0.45)
    assert sorted(det[0, :4, 5].tolist()) == [0.0, 0.0, 1.0, 2.0]


# ------------------------------------------------------------------------------------------------ step (c)
@pytest.mark.parametrize("max_det", [1, 3, 300])
def test_the_pass_stops_at_max_det(max_det):
    pred = cases.head_output(21, 3, 1100, 2)
    det, count = check(pred, "max_det", conf_thres=0.05, iou_thres=0.45, multi_label=True, max_det=max_det)
    assert count.tolist() == [max_det] * 3


def test_chains_and_the_far_cluster():
    _, count = check(cases.chain(), "chain", conf_thres=0.25, iou_thres=0.4)
    assert count.tolist() == [2]
    _, count = check(cases.cluster(), "cluster", conf_thres=0.25, iou_thres=0.45)
    assert count.tolist() == [101]


def test_kept_count_crosses_the_round_boundary():
    """1100 rows, about a third of them suppressed: rows are still kept in the second round of 1024, past kept entries of the
    first; max_det = 1024, the list's capacity."""
    pred = cases.survivors(1100)
    pred[0, 1::3, :4] = pred[0, 0::3, :4][:len(pred[0, 1::3])]
    _, count = check(pred, "second round", conf_thres=0.25, iou_thres=0.45, max_det=1024)
    assert 700 < count[0] < 1024


def test_ovr_equal_to_the_threshold_is_kept_and_one_ulp_above_is_not():
    _, count = check(cases.pair(cases.EXACT_A, cases.EXACT_B), "ovr == 0.5", conf_thres=0.25, iou_thres=0.5)
    assert count.tolist() == [2]
    _, count = check(cases.pair(cases.EXACT_A, cases.EXACT_B), "thr below", conf_thres=0.25, iou_thres=float(np.nextafter(0.5, 0.0)))
    assert count.tolist() == [1]
    a, b = cases.one_ulp_above_half()
    _, count = check(cases.pair(a, b), "one ulp above", conf_thres=0.25, iou_thres=0.5)
    assert count.tolist() == [1]


def test_degenerate_boxes():
    for agnostic in (False, True):
        check(cases.degenerate(), "degenerate", conf_thres=0.25, iou_thres=0.45, agnostic=agnostic)
    check(cases.degenerate(), "degenerate, iou 0", conf_thres=0.25, iou_thres=0.0)


def test_one_box_under_two_classes():
    _, count = check(cases.two_classes_one_box(), "two classes", conf_thres=0.25, iou_thres=0.45, multi_label=True)
    assert count.tolist() == [3]
    _, count = check(cases.two_classes_one_box(), "agnostic", conf_thres=0.25, iou_thres=0.45, multi_label=True, agnostic=True)
    assert count.tolist() == [2]


def test_the_class_offset_is_added_in_float32():
    g = load_golden("detector_output")
    a, b = g["offset_pair_boxes"]
    pred = cases.pair(a, b, C=3, cls=1)
    _, with_offset = check(pred, "offset", conf_thres=0.25, iou_thres=0.65)
    _, without = check(pred, "no offset", conf_thres=0.25, iou_thres=0.65, agnostic=True)
    assert with_offset.tolist() != without.tolist()
    assert_bit_equal(with_offset, g["offset_pair/count"])


# ------------------------------------------------------------------------------------------------ consistency
def test_list_route_batch_position_repeat_and_refusals():
    do = _do()
    pred = cases.head_output(31, 3, 700, 3)
    kw = dict(conf_thres=0.03, iou_thres=0.65, multi_label=True)
    d = torch.from_numpy(pred).to(DEV)
    det, count = do.nms_batch(d, **kw)
    out = do.non_max_suppression(d, **kw)
    assert len(out) == 3
    for b in range(3):
        assert out[b].device == d.device and out[b].dtype == torch.float32
        assert_bit_equal(out[b].cpu().numpy(), det[b, :int(count[b])].cpu().numpy(), "list %d" % b)
    det2, count2 = do.nms_batch(d, **kw)
    assert torch.equal(det, det2) and torch.equal(count, count2)
    for b in range(3):                                                 # alone, and at another place of a batch
        alone = do.nms_batch(d[b:b + 1].contiguous(), **kw)
        assert torch.equal(alone[0][0], det[b]) and int(alone[1][0]) == int(count[b])
    rolled = do.nms_batch(d.roll(1, 0).contiguous(), **kw)
    assert torch.equal(rolled[0].roll(-1, 0), det) and torch.equal(rolled[1].roll(-1, 0), count)
    assert_bit_equal(d.cpu().numpy(), pred, "the input is left as it was")
    with pytest.raises(ValueError, match=r"\.float\(\)"):
        do.non_max_suppression(d.half(), **kw)
    with pytest.raises(ValueError, match=r"\.float\(\)"):
        do.nms_batch(d.double(), **kw)
    with pytest.raises(ValueError, match="max_det"):
        do.nms_batch(d, max_det=1025)
    with pytest.raises(AssertionError, match="iou_thres must be in 0.0 to 1.0, however 2 is provided."):
        do.non_max_suppression(d, iou_thres=2)
    empty = do.non_max_suppression(d[:, :0].contiguous())
    assert [tuple(o.shape) for o in empty] == [(0, 6)] * 3


def test_capture_and_replay():
    do = _do()
    pred = cases.head_output(41, 3, 500, 2)
    kw = dict(conf_thres=0.25, iou_thres=0.45, max_det=100)
    static = torch.from_numpy(pred).to(DEV)
    eager_det, eager_count = do.nms_batch(static, **kw)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        det, count = do.nms_batch(static, **kw)
    other = cases.head_output(42, 3, 500, 2)
    static.copy_(torch.from_numpy(other))
    graph.replay()
    torch.cuda.synchronize()
    want_det, want_count = cases.pad(do.nms_host(other, **kw), 100)
    assert_bit_equal(det.cpu().numpy(), want_det, "replay on new contents")
    assert_bit_equal(count.cpu().numpy(), want_count)
    static.copy_(torch.from_numpy(pred))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(det, eager_det) and torch.equal(count, eager_count)


# ------------------------------------------------------------------------------------------------ the scratch contract
@pytest.mark.parametrize("case", [(1, 16, 1, False), (3, 333, 3, True), (1, 64, 2, True), (3, 1100, 2, False)],
                         ids=lambda c: "B%d_N%d_C%d_%s" % (c[0], c[1], c[2], "multi" if c[3] else "single"))
def test_scratch_and_outputs_are_as_long_as_stated(case):
    """The scratch is exactly evrep_dense_rank_scratch_bytes(B, 5 * ceil(B * R / 4)) bytes and det / count exactly
    (B, max_det, 6) / (B), each between guard bands, the prediction registered read-only; interior fills zeros, 0xFF and
    random and a second arena seed give the same bytes (nothing needs initialisation, every output byte is written), no band
    and no input byte changes.  Every row is a candidate: the worst case the size is stated for.  (1, 16, 1): B * R = 16,
    total = 20 -> four arrays of exactly 256 bytes hold five of 64 with no slack in use; (1, 64, 2) multi: B * R = 128, the five
    arrays end 512 bytes before the region does."""
    from event_representation_study_amd import _lib
    do = _do()
    B, N, C, multi = case
    lib = _lib.load()
    pred = cases.head_output(N + C, B, N, C, lo=0.6)
    kw = dict(conf_thres=0.25, iou_thres=0.45, multi_label=multi, max_det=7)
    want_det, want_count = cases.pad(do.nms_host(pred, **kw), 7)
    total = do.nms_scratch_total(B, N, C, multi)
    nbytes = int(lib.evrep_dense_rank_scratch_bytes(B, total))
    R = N * C if multi and C > 1 else N
    assert nbytes >= 20 * B * R and (case != (1, 16, 1, False) or nbytes == 1024)
    for seed, fill in tuple((1, f) for f in FILLS) + ((2, "random"),):
        arena = Arena(DEV, seed)
        d_pred = arena.carve_like(torch.from_numpy(pred), name="pred")
        p_pred = arena.ptr()
        det = arena.carve_shape((B, 7, 6), torch.float32, fill=fill, name="det")
        p_det = arena.ptr()
        count = arena.carve_shape((B,), torch.int32, fill=fill, name="count")
        p_count = arena.ptr()
        arena.carve(nbytes, fill=fill, name="scratch")
        p_sc = arena.ptr()
        flags = _lib.NMS_MULTI_LABEL if multi else 0
        rc = lib.evrep_nms(ctypes.c_void_p(p_pred), B, N, C, 0.25, 0.45, flags, None, -1, 30000, 7, ctypes.c_void_p(p_det),
                           ctypes.c_void_p(p_count), ctypes.c_void_p(p_sc), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        _lib.check(rc, "evrep_nms")
        torch.cuda.synchronize()
        arena.check()
        arena.check_inputs()
        got = (det.cpu().numpy(), count.cpu().numpy())
        assert_bit_equal(got[0], want_det, "seed %d fill %s" % (seed, fill))
        assert_bit_equal(got[1], want_count, "seed %d fill %s" % (seed, fill))
        assert d_pred.data_ptr() == p_pred
