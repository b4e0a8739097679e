"""CPU-only: the host restatement of the detection scoring (detector_eval.match_host, the CPU routes of process_batch and
ConfusionMatrix) against the golden recorded from the reference's own metrics.py and evaler.py (tests/golden/detector_eval.npz),
bit for bit and integer for integer; ap_per_class / compute_ap within 1e-12 (the same numpy statements: the margin is for another
numpy build's summation order only); the tie rule, the threshold edges, the evaler's guard; the C surface of evrep_det_match."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, assert_bit_equal, load_golden
import detector_eval_cases as cases

F32 = np.float32
IOUV_KEYS = ("T10", "T1", "T16")


def _de():
    from event_representation_study_amd import detector_eval
    return detector_eval


@pytest.fixture(scope="module")
def golden():
    return load_golden("detector_eval")


def golden_names():
    return [str(n) for n in load_golden("detector_eval")["names"]]


def eval_batch(g, bi):
    pre = "eval%d/" % bi
    return g[pre + "det"], g[pre + "count"], g[pre + "targets"], cases.shapes_from_array(g[pre + "shapes"])


# ------------------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("key", IOUV_KEYS)
@pytest.mark.parametrize("name", golden_names())
def test_match_host_equals_process_batch(golden, name, key):
    de = _de()
    det, lab, iouv = golden[name + "/det"], golden[name + "/labels"], golden[name + "/iouv_" + key]
    d, count, targets = cases.native_batch([det], [lab])
    correct, detn, tbox, n_labels, status = de.match_host(d, count, targets, iouv=iouv, native=True)
    assert correct.dtype == np.uint8 and status.tolist() == [0] and n_labels.tolist() == [len(lab)]
    assert_bit_equal(correct[0], golden[name + "/correct_" + key], name)
    assert_bit_equal(detn, d, "native mode takes the detections as they are")
    assert_bit_equal(tbox, lab[:, 1:], "and the labels")
    got = de.process_batch(torch.from_numpy(det.copy()), torch.from_numpy(lab.copy()), torch.from_numpy(iouv))
    assert got.dtype == torch.bool and tuple(got.shape) == (len(det), len(iouv))
    assert_bit_equal(got.numpy().astype(np.uint8), golden[name + "/correct_" + key], name + " process_batch")


@pytest.mark.parametrize("name", golden_names())
def test_confusion_matrix_equals_the_reference(golden, name):
    de = _de()
    det, lab, nc = golden[name + "/det"], golden[name + "/labels"], int(golden[name + "/nc"])
    cm = de.ConfusionMatrix(nc)
    cm.process_batch(torch.from_numpy(det.copy()), torch.from_numpy(lab.copy()))
    assert cm.status == 0 and cm.matrix.dtype == np.float64 and cm.matrix.shape == (nc + 1, nc + 1)
    assert np.array_equal(cm.counts(), golden[name + "/matrix"]), name
    tp, fp = cm.tp_fp()
    want = golden[name + "/matrix"].astype(np.float64)
    assert np.array_equal(tp, want.diagonal()[:-1]) and np.array_equal(fp, (want.sum(1) - want.diagonal())[:-1])
    cm.process_batch(torch.from_numpy(det.copy()), torch.from_numpy(lab.copy()))
    assert np.array_equal(cm.counts(), 2 * golden[name + "/matrix"]), "a second call accumulates"


@pytest.mark.parametrize("bi", [0, 1])
def test_normalised_mode_equals_the_evaler(golden, bi):
    """Geometry, correct and the matrix of evaler.py:209-258 with the reference's own Evaler.scale_coords and xywh2xyxy."""
    de = _de()
    det, count, targets, shapes = eval_batch(golden, bi)
    correct, detn, tbox, n_labels, status = de.match_host(det, count, targets, cases.IMG, shapes)
    pre = "eval%d/" % bi
    assert not status.any()
    assert_bit_equal(detn, golden[pre + "detn"], "detn")
    assert_bit_equal(correct, golden[pre + "correct"], "correct")
    held = ~np.isnan(golden[pre + "tbox"][:, 0])                       # (the evaler forms no tbox for an image without detections)
    assert held.sum() >= 8 and (bi == 1 or not held.all())
    assert_bit_equal(tbox[held], golden[pre + "tbox"][held], "tbox")
    assert_bit_equal(n_labels, np.array([(targets[:, 0] == b).sum() for b in range(len(count))], np.int32))
    from event_representation_study_amd import detector_output
    scb = detector_output.scale_coords_batch(torch.from_numpy(det), torch.from_numpy(count), cases.IMG, shapes)
    assert_bit_equal(detn, scb.numpy(), "detn == scale_coords_batch")


def test_two_batch_matrix_and_compute_equal_the_evaler(golden):
    de = _de()
    matrix = np.zeros(16, np.int64)
    stats, seen = [[], [], [], []], 0
    for bi in (0, 1):
        det, count, targets, shapes = eval_batch(golden, bi)
        correct = de.match_host(det, count, targets, cases.IMG, shapes, matrix=matrix, nc=3, skip_empty=True)[0]
        for b in range(len(count)):
            stats[0].append(correct[b, :count[b]].astype(bool))
            stats[1].append(det[b, :count[b], 4])
            stats[2].append(det[b, :count[b], 5])
            stats[3].append(targets[targets[:, 0] == b, 1])
            seen += 1
    assert np.array_equal(matrix.reshape(4, 4), golden["eval/matrix"])
    stats = [np.concatenate(s, 0) for s in stats]
    for k, v in zip(("tp", "conf", "pred_cls", "target_cls"), stats):
        assert np.array_equal(v, golden["eval/stats_" + k]), k
    out = de.summarize(stats, 3, seen)
    for k in ("p", "r", "ap", "f1"):
        assert np.abs(out[k] - golden["eval/" + k]).max() <= 1e-12, k
    assert np.array_equal(out["ap_class"], golden["eval/ap_class"]) and out["ap_class"].dtype == np.int32
    assert np.abs(np.array([out["mp"], out["mr"], out["map50"], out["map"]]) - golden["eval/summary"]).max() <= 1e-12
    assert out["best_f1_index"] == int(golden["eval/best_f1_index"]) and out["seen"] == int(golden["eval/seen"]) == 7
    assert np.array_equal(out["nt"], golden["eval/nt"])
    p, r, ap, f1, ap_class = de.ap_per_class(*stats)
    assert np.abs(ap - golden["eval/ap"]).max() <= 1e-12
    a, mpre, mrec = de.compute_ap(np.array([0.0, 0.5, 1.0]), np.array([1.0, 0.5, 0.25]))
    assert mrec[0] == 0.0 and mrec[-1] == 1.01 and mpre[0] == 1.0 and mpre[-1] == 0.0 and 0.0 < a < 1.0
    assert de.summarize((np.zeros((3, 10), bool), np.ones(3, F32), np.zeros(3, F32), np.zeros(2, F32)), 3, 1) == (0.0, 0.0)


def test_golden_has_no_label_ties_and_covers_what_it_says(golden):
    for name in golden_names():
        assert not cases.label_ties(golden[name + "/det"], golden[name + "/labels"], 0.3), name
        assert golden[name + "/correct_T10"].any() or name == "native_one"
    dups = golden["native_dups/det"]
    assert len(np.unique(dups[:, :4], axis=0)) < len(dups), "duplicated detections are in the golden"
    assert golden["native_grid/correct_T10"][:, 0].sum() == 30 and len(golden["native_grid/det"]) == 100
    assert golden["eval0/count"].tolist() == [20, 7, 0, 33] and (golden["eval0/targets"][:, 0] == 1).sum() == 0


# ---------------------------------------------------------------------------------------------------------------- the tie rule
def test_duplicated_labels_give_the_lowest_index():
    """Two identical labels: rule 4's k* is the lower one, so the FIRST detection claims label 0 and a second detection of
    the same box finds label 0 taken (it does not fall through to label 1); in the matrix label 0 is matched, label 1 is
    background."""
    de = _de()
    lab = np.array([[1, 10, 10, 50, 50], [1, 10, 10, 50, 50], [1, 100, 100, 140, 140]], F32)
    det = np.array([[10, 10, 50, 48, 0.9, 1], [10, 10, 50, 49, 0.8, 1], [100, 100, 140, 139, 0.7, 1]], F32)
    d, count, targets = cases.native_batch([det], [lab])
    matrix = np.zeros(9, np.int64)
    correct = de.match_host(d, count, targets, iouv=[0.5], native=True, matrix=matrix, nc=2)[0]
    assert correct[0, :, 0].tolist() == [1, 0, 1]
    want = np.zeros((3, 3), np.int64)
    want[1, 1] = 2          # labels 0 and 2 matched (label 0 by detection 1: IoU 39/40 beats detection 0's 38/40)
    want[2, 1] = 1          # label 1: background
    want[1, 2] = 1          # detection 0 won no label
    assert np.array_equal(matrix.reshape(3, 3), want)
    # swapped label order: still the lowest index, now the other copy
    targets2 = targets[[1, 0, 2]]
    assert_bit_equal(de.match_host(d, count, targets2, iouv=[0.5], native=True)[0], correct)


def test_two_different_labels_of_equal_iou_give_the_lowest_index():
    de = _de()
    det, lab = cases.label_tie()
    assert de.iou_host(lab[:, 1:], det[:1, :4])[:, 0].tolist() == [0.5, 0.5] and cases.label_ties(det, lab)
    d, count, targets = cases.native_batch([det], [lab])
    matrix = np.zeros(9, np.int64)
    correct = de.match_host(d, count, targets, iouv=[0.5, 0.75], native=True, matrix=matrix, nc=2)[0]
    assert correct[0].tolist() == [[1, 0], [0, 1]], "label 0 is claimed by detection 0 at 0.5 and by detection 1 at 0.75"
    want = np.zeros((3, 3), np.int64)
    want[1, 1] = 1          # label 0, won by detection 1
    want[2, 1] = 1          # label 1: detection 0's tie went to label 0
    want[1, 2] = 1          # detection 0 won nothing
    assert np.array_equal(matrix.reshape(3, 3), want)
    assert de.process_batch(torch.from_numpy(det), torch.from_numpy(lab), torch.tensor([0.5]))[:, 0].tolist() == [True, False]


def test_equal_iou_detections_on_one_label_take_the_lowest_detection_in_the_matrix():
    de = _de()
    lab = np.array([[0, 10, 10, 50, 50]], F32)
    det = np.array([[10, 10, 50, 48, 0.9, 1], [10, 10, 50, 48, 0.8, 0]], F32)
    d, count, targets = cases.native_batch([det], [lab])
    matrix = np.zeros(9, np.int64)
    de.match_host(d, count, targets, iouv=[0.5], native=True, matrix=matrix, nc=2)
    want = np.zeros((3, 3), np.int64)
    want[1, 0] = 1          # detection 0 (class 1) wins label 0 (class 0)
    want[0, 2] = 1          # detection 1 won nothing
    assert np.array_equal(matrix.reshape(3, 3), want)


# ------------------------------------------------------------------------------------------------------------ threshold edges
def test_iou_exactly_at_the_thresholds():
    de = _de()
    lab = np.array([[2, 0, 0, 2, 1]], F32)
    det = np.array([[0, 0, 1, 1, 0.9, 2]], F32)
    assert de.iou_host(lab[:, 1:], det[:, :4])[0, 0] == F32(0.5)
    d, count, targets = cases.native_batch([det], [lab])
    matrix = np.zeros(16, np.int64)
    correct = de.match_host(d, count, targets, iouv=[0.5, np.nextafter(F32(0.5), F32(1))], native=True, matrix=matrix, nc=3, iou_thres=0.5)[0]
    assert correct[0, 0].tolist() == [1, 0], "iou >= iouv is not strict"
    want = np.zeros((4, 4), np.int64)
    want[3, 2] = 1          # iou > iou_thres is strict: the label is background, and with no match the detection is not counted
    assert np.array_equal(matrix.reshape(4, 4), want)
    matrix[:] = 0
    de.match_host(d, count, targets, iouv=[0.5], native=True, matrix=matrix, nc=3, iou_thres=float(np.nextafter(F32(0.5), F32(0))))
    assert matrix.reshape(4, 4)[2, 2] == 1 and matrix.sum() == 1


def test_conf_exactly_at_the_threshold_is_left_out_of_the_matrix():
    de = _de()
    lab = np.array([[0, 0, 0, 10, 10], [1, 20, 20, 30, 30]], F32)
    det = np.array([[0, 0, 10, 10, 0.25, 0], [20, 20, 30, 30, np.nextafter(F32(0.25), F32(1)), 1]], F32)
    d, count, targets = cases.native_batch([det], [lab])
    matrix = np.zeros(9, np.int64)
    correct = de.match_host(d, count, targets, native=True, matrix=matrix, nc=2)[0]
    assert correct[0, :, 0].tolist() == [1, 1], "conf plays no part in correct"
    want = np.zeros((3, 3), np.int64)
    want[2, 0] = 1          # label 0: its only detection has conf == 0.25
    want[1, 1] = 1
    assert np.array_equal(matrix.reshape(3, 3), want)


def test_nan_zero_area_and_class_equality():
    de = _de()
    lab = np.array([[2, 0, 0, 10, 10], [2, np.nan, 0, 10, 10], [2, 40, 40, 40, 40], [2.5, 60, 60, 70, 70]], F32)
    det = np.array([[0, 0, 10, np.nan, 0.9, 2],       # a NaN corner: matches nothing
                    [40, 40, 40, 40, 0.9, 2],         # zero area on zero area: 0 / 0
                    [60, 60, 70, 70, 0.9, 2],         # class 2.0 against 2.5
                    [60, 60, 70, 70, 0.9, 2.5],       # float equality holds for 2.5 == 2.5
                    [0, 0, 10, 10, 0.9, 2]], F32)
    d, count, targets = cases.native_batch([det], [lab])
    matrix = np.zeros(16, np.int64)
    correct, _, _, _, status = de.match_host(d, count, targets, native=True, matrix=matrix, nc=3)
    assert correct[0, :, 0].tolist() == [0, 0, 0, 1, 1] and status.tolist() == [0]
    m = matrix.reshape(4, 4)
    # labels 0 and 3 matched (int(2.5) == 2; detections 2 and 3 tie on label 3, the lower wins), labels 1 and 2 background,
    # detections 0, 1 and 3 won nothing
    assert m[2, 2] == 2 and m[3, 2] == 2 and m[2, 3] == 3 and m.sum() == 7


def test_bad_class_bad_count_and_label_overflow():
    de = _de()
    lab = np.array([[5, 0, 0, 10, 10], [0, 20, 20, 30, 30]], F32)
    det = np.array([[0, 0, 10, 10, 0.9, 0], [20, 20, 30, 30, 0.9, -3]], F32)
    d, count, targets = cases.native_batch([det], [lab])
    matrix = np.zeros(9, np.int64)
    status = de.match_host(d, count, targets, native=True, matrix=matrix, nc=2)[4]
    assert status.tolist() == [de.ST_BAD_CLASS] and matrix.sum() == 0, "both updates name a class outside [0, 2)"
    correct, _, _, _, status = de.match_host(d, [7], targets, native=True)
    assert status.tolist() == [de.ST_BAD_COUNT] and correct.shape == (1, 2, 10)
    many = cases.grid_labels(de.MAX_LABELS + 1)
    dd = cases.grid_detections(5, 5)
    d, count, targets = cases.native_batch([dd, dd], [many, cases.grid_labels(5)])
    matrix = np.zeros(16, np.int64)
    correct, _, tbox, n_labels, status = de.match_host(d, count, targets, native=True, matrix=matrix, nc=3)
    assert status.tolist() == [de.ST_LABEL_OVERFLOW, 0] and n_labels.tolist() == [de.MAX_LABELS + 1, 5]
    assert not correct[0].any() and correct[1, :, 0].all() and matrix.sum() == 5
    assert_bit_equal(tbox, targets[:, 2:])


# ------------------------------------------------------------------------------------------------------------ the evaler's guard
def test_the_guard_and_the_no_match_quirk():
    de = _de()
    lab = np.array([[0, 0, 0, 10, 10], [1, 20, 20, 30, 30]], F32)
    none = np.zeros((0, 6), F32)
    d, count, targets = cases.native_batch([none], [lab])
    plain, guarded = np.zeros(9, np.int64), np.zeros(9, np.int64)
    de.match_host(d, count, targets, native=True, matrix=plain, nc=2)
    de.match_host(d, count, targets, native=True, matrix=guarded, nc=2, skip_empty=True)
    assert plain.reshape(3, 3)[2].tolist() == [1, 1, 0] and plain.sum() == 2, "ConfusionMatrix.process_batch: every label is background"
    assert guarded.sum() == 0, "the evaler never calls it for an image without detections"
    far = np.array([[100, 100, 110, 110, 0.9, 0], [200, 200, 210, 210, 0.9, 1]], F32)
    d, count, targets = cases.native_batch([far], [lab])
    m = np.zeros(9, np.int64)
    de.match_host(d, count, targets, native=True, matrix=m, nc=2, skip_empty=True)
    assert m.reshape(3, 3)[2].tolist() == [1, 1, 0] and m.sum() == 2, "no match in the image: no detection row is counted"
    near = np.array([[0, 0, 10, 10, 0.9, 0], [200, 200, 210, 210, 0.9, 1]], F32)
    d, count, targets = cases.native_batch([near], [lab])
    m[:] = 0
    de.match_host(d, count, targets, native=True, matrix=m, nc=2)
    assert m.reshape(3, 3).tolist() == [[1, 0, 0], [0, 0, 1], [0, 1, 0]], "one match: now the other detection is counted"


# ------------------------------------------------------------------------------------------------------------ the C surface
def _argcheck_lib():
    from event_representation_study_amd import build, _lib
    build.build(verbose=False)
    return _lib, _lib.load()


N_ARGS = 22


def test_symbol_is_declared_bound_and_a_status_entry():
    _lib, lib = _argcheck_lib()
    assert _lib.ABI_VERSION == 3 and lib.evrep_abi_version() == 3
    entry = _lib.SYMBOLS["evrep_det_match"]
    assert isinstance(entry, _lib.Status) and entry[0] is ctypes.c_int and len(entry[1]) == N_ARGS
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "evrep.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+evrep_det_match\s*\(([^)]*)\)", text)
    assert decl and len(decl.group(1).split(",")) == N_ARGS
    assert getattr(lib, "evrep_det_match") is not None
    assert not [n for n in _lib.SYMBOLS if "det_match" in n and n.endswith("_scratch_bytes")]
    defines = dict(re.findall(r"^#define\s+EVREP_(DETEVAL_[A-Z_]+)\s+\(?([0-9<u ]+)\)?\s*$", text, flags=re.M))
    assert set(defines) == {"DETEVAL_" + n for n in ("NATIVE", "SKIP_EMPTY", "MAX_LABELS", "MAX_T", "MAX_TARGETS", "ST_LABEL_OVERFLOW",
                                                     "ST_BAD_CLASS", "ST_BAD_COUNT")}
    for name, value in defines.items():
        assert eval(value.replace("u", "")) == getattr(_lib, name), name
    assert _lib.DETEVAL_MAX_LABELS == 1024 and _lib.DETEVAL_MAX_T == 16


def test_kernel_source_is_part_of_the_detector_unit():
    from event_representation_study_amd import build
    deps = [os.path.basename(p) for p in build.unit_deps("evrep_capi_detin.hip")]
    assert "evrep_deteval.hip" in deps and "evrep_nms.hip" in deps
    assert len(build.SOURCES) == 15 and "evrep_deteval.hip" not in build.SOURCES
    src = open(os.path.join(ROOT, "event_representation_study_amd", "csrc", "evrep_deteval.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "-ffp-contract=off" in src


def test_header_names_every_rule():
    text = open(os.path.join(ROOT, "include", "evrep.h")).read()
    at = text.index("Scoring the detections in ONE launch")
    doc = text[at:text.index("int evrep_det_match", at)]
    for phrase in ("scale_coords", "xywh2xyxy", "x *= img_w", "EVREP_DETEVAL_NATIVE", "general.box_iou", "0 / 0 is NaN",
                   "cls_k == cls_j", "iou*(j) >= iouv[i]", "LOWEST label index", "unstable", "conf > `conf`", "iou > iou_thres (strict)",
                   "lowest label index, then lowest detection index", "[int(cls_det), int(cls_label)]", "[nc, int(cls_label)]",
                   "[int(cls_det), nc]", "at least one match", "integer atomics", "EVREP_DETEVAL_ST_BAD_CLASS", "EVREP_DETEVAL_SKIP_EMPTY",
                   "EVREP_DETEVAL_MAX_LABELS", "EVREP_DETEVAL_ST_LABEL_OVERFLOW", "every byte written", "-ffp-contract=off",
                   "Needs no scratch", "captured into a graph", "HOST float [T]"):
        assert phrase in doc, phrase
    for other in ("detector_eval.py", "DESIGN.md"):
        path = os.path.join(ROOT, "event_representation_study_amd", other) if other.endswith(".py") else os.path.join(ROOT, other)
        body = open(path).read()
        assert "unstable" in body and "LOWEST label index" in body, other


def test_arguments_outside_the_stated_ranges_are_einval_before_any_launch():
    """No device is needed: every refusal comes before the launch.  The pointers are aligned host addresses never read
    (iouv_host is a real host array: the call reads it)."""
    _lib, lib = _argcheck_lib()
    buf = (ctypes.c_char * 8192)()
    base = (ctypes.addressof(buf) + 255) & ~255
    P = ctypes.c_void_p
    iouv = (ctypes.c_float * 16)(*[0.5 + 0.02 * i for i in range(16)])
    nan_iouv = (ctypes.c_float * 2)(0.5, float("nan"))
    odd_iouv = ctypes.cast(base + 4097, ctypes.POINTER(ctypes.c_float))

    def call(det=base, count=base + 256, B=1, max_det=300, targets=base + 512, n_t=4, geom=base + 768, img_h=640, img_w=640,
             iouv=iouv, T=10, flags=0, matrix=base + 1024, nc=3, conf=0.25, iou_thres=0.45, correct=base + 1280, detn=base + 1536,
             tbox=base + 1792, n_labels=base + 2048, status=base + 2304):
        return lib.evrep_det_match(P(det), P(count), B, max_det, P(targets), n_t, P(geom), img_h, img_w, iouv, T, flags, P(matrix), nc,
                                   conf, iou_thres, P(correct), P(detn), P(tbox), P(n_labels), P(status), None)

    bad = [dict(B=0), dict(B=65536), dict(max_det=0), dict(max_det=1025), dict(n_t=-1), dict(n_t=(1 << 24) + 1), dict(T=0), dict(T=17),
           dict(flags=4), dict(flags=8), dict(img_h=0), dict(img_w=0), dict(img_h=4097), dict(img_w=4097), dict(nc=0), dict(nc=4097),
           dict(conf=float("nan")), dict(iou_thres=float("nan")), dict(iouv=nan_iouv, T=2), dict(iouv=None), dict(iouv=odd_iouv),
           dict(det=0), dict(count=0), dict(targets=0), dict(geom=0), dict(correct=0), dict(n_labels=0), dict(status=0),
           dict(det=base + 2), dict(count=base + 257), dict(targets=base + 514), dict(geom=base + 770), dict(matrix=base + 1028),
           dict(detn=base + 1538), dict(tbox=base + 1793), dict(n_labels=base + 2050), dict(status=base + 2305),
           dict(flags=1, geom=base + 770), dict(n_t=0, targets=base + 514)]
    for kw in bad:
        assert call(**kw) == _lib.EVREP_EINVAL, kw
