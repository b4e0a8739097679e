"""CPU-only: the host restatement of the detector's output (detector_output.nms_host, the CPU route of non_max_suppression)
against the golden recorded from the reference's own non_max_suppression (tests/golden/detector_output.npz: torchvision behind
a stand-in there, so the greedy pass is parity unpinned); scale_coords_batch against a per-image loop of the reference's
statements; the refusals; the C surface of evrep_nms.  Everything is compared bit for bit."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, assert_bit_equal, load_golden
import detector_output_cases as cases

F32 = np.float32


def _do():
    from event_representation_study_amd import detector_output
    return detector_output


@pytest.fixture(scope="module")
def golden():
    return load_golden("detector_output")


def golden_kwargs(g, name):
    conf, iou, agnostic, multi, max_det = g[name + "/args"].tolist()
    classes = g[name + "/classes"].tolist()
    return dict(conf_thres=conf, iou_thres=iou, classes=None if classes == [-1] else classes, agnostic=bool(agnostic),
                multi_label=bool(multi), max_det=int(max_det))


def golden_names():
    return [str(n) for n in load_golden("detector_output")["names"]]


@pytest.mark.parametrize("name", golden_names())
def test_nms_host_equals_the_reference(golden, name):
    kw = golden_kwargs(golden, name)
    det, count = cases.pad(_do().nms_host(golden[name + "/pred"], **kw), kw["max_det"])
    assert_bit_equal(count, golden[name + "/count"], name)
    assert_bit_equal(det, golden[name + "/det"], name)


@pytest.mark.parametrize("name", ["evaler_C3", "inferer_C2", "candidate_edges_multi", "classes1_det3"])
def test_cpu_route_of_non_max_suppression(golden, name):
    kw = golden_kwargs(golden, name)
    pred = torch.from_numpy(golden[name + "/pred"].copy())
    out = _do().non_max_suppression(pred, **kw)
    assert len(out) == pred.shape[0] and all(o.dtype == torch.float32 and o.device == pred.device and o.shape[1] == 6 for o in out)
    det, count = cases.pad([o.numpy() for o in out], kw["max_det"])
    assert_bit_equal(count, golden[name + "/count"], name)
    assert_bit_equal(det, golden[name + "/det"], name)
    assert_bit_equal(pred.numpy(), golden[name + "/pred"], "the input is left as it was")


def test_golden_covers_what_it_says(golden):
    """The edge rows of the candidate test are decided as the module's text says, in the REFERENCE's output."""
    single = golden["candidate_edges_single/det"][2, :golden["candidate_edges_single/count"][2]]
    boxes = cases.grid_boxes(64)
    kept = {int(np.flatnonzero((boxes[:, 0] == F32(r[0] + r[2]) / 2) & (boxes[:, 1] == F32(r[1] + r[3]) / 2))[0]) for r in single}
    assert kept.isdisjoint({1, 2, 3, 4, 5, 7, 9, 10, 11}) and {0, 6, 8} <= kept
    assert golden["float32_threshold/count"].tolist() == [6]          # rows 1 and 2 equal float32(0.1): dropped
    tie = golden["argmax_tie/det"][0, :4]
    by_x = tie[np.argsort(tie[:, 0])]
    assert by_x[:, 5].tolist() == [1.0, 0.0, 0.0, 2.0]                # the FIRST maximum
    assert golden["two_classes_one_box/count"].tolist() == [3] and golden["two_classes_one_box_agnostic/count"].tolist() == [2]


def test_the_offset_rounding_pair_is_decided_by_the_float32_addition(golden):
    """Rule 6: the class offset is added in float32 and rounds the corners.  On this pair (found by search in the golden
    script) the restated kernel decides differently on the offset boxes and on the un-offset ones -- a kernel that skips the
    addition keeps the wrong number of rows."""
    do = _do()
    a, b = golden["offset_pair_boxes"]
    o1, o0 = cases.ovr_f32(a, b, 4096.0), cases.ovr_f32(a, b, 0.0)
    assert_bit_equal(np.array([o1, o0]), golden["offset_pair_ovr"])
    assert (float(o1) > 0.65) != (float(o0) > 0.65)
    boxes = do.xywh2xyxy(np.array([a, b], F32))
    scores = np.array([0.9, 0.8], F32)
    with_offset = do.torchvision_nms_host(boxes + F32(4096), scores, 0.65)
    without = do.torchvision_nms_host(boxes, scores, 0.65)
    assert len(with_offset) != len(without)
    assert golden["offset_pair/count"].tolist() == [len(with_offset)]
    assert golden["offset_pair_agnostic/count"].tolist() == [len(without)]
    pred = cases.pair(a, b, C=3, cls=1)
    assert len(do.nms_host(pred, 0.25, 0.65)[0]) == len(with_offset)
    assert len(do.nms_host(pred, 0.25, 0.65, max_wh=0)[0]) == len(without)


def test_the_strict_comparison_and_the_double_threshold():
    do = _do()
    assert cases.ovr_f32(cases.EXACT_A, cases.EXACT_B) == F32(0.5)
    pred = cases.pair(cases.EXACT_A, cases.EXACT_B)
    assert len(do.nms_host(pred, 0.25, 0.5)[0]) == 2                                   # ovr == iou_thres: kept
    assert len(do.nms_host(pred, 0.25, float(np.nextafter(0.5, 0.0)))[0]) == 1         # a double below: suppressed
    a, b = cases.one_ulp_above_half()
    assert cases.ovr_f32(a, b) == np.nextafter(F32(0.5), F32(1))
    assert len(do.nms_host(cases.pair(a, b), 0.25, 0.5)[0]) == 1
    assert len(do.nms_host(cases.chain(), 0.25, 0.4)[0]) == 2                          # A and C
    assert len(do.nms_host(cases.cluster(), 0.25, 0.45)[0]) == 101                     # 100 disjoint boxes and one of the 600


def test_max_nms_cut_and_max_det():
    do = _do()
    for n in (49, 50, 51):
        pred = cases.cut_rows(n)
        full = do.nms_host(pred, 0.25, 0.45, max_nms=1000)[0]
        cut = do.nms_host(pred, 0.25, 0.45, max_nms=50)[0]
        if n <= 50:
            assert_bit_equal(cut, full)
        else:       # the row of smallest score never enters: the cut equals the call without that row
            low = np.argmin(np.where(pred[0, :, 4] > 0, pred[0, :, 5], 2.0))
            less = pred.copy()
            less[0, low, 4] = 0.0
            assert_bit_equal(cut, do.nms_host(less, 0.25, 0.45, max_nms=1000)[0])
    pred = cases.survivors(65)
    for max_det in (1, 3, 300):
        rows = do.nms_host(pred, 0.25, 0.45, max_det=max_det)[0]
        assert len(rows) == min(max_det, 65)
        assert_bit_equal(rows, do.nms_host(pred, 0.25, 0.45, max_det=1000)[0][:max_det])


def test_xywh2xyxy_in_float32():
    do = _do()
    x = cases.head_output(9, 1, 50, 1)[0, :, :4]
    y = do.xywh2xyxy(x)
    assert y.dtype == F32
    assert_bit_equal(y[:, 0], x[:, 0] - x[:, 2] / F32(2))
    assert_bit_equal(y[:, 3], x[:, 1] + x[:, 3] / F32(2))
    assert_bit_equal(do.xywh2xyxy(torch.from_numpy(x)).numpy(), y)


def _scale_coords_reference(coords, img0_shape, ratio_pad):
    """core/evaler.py's scale_coords with ratio_pad given and scale_exact False, statement for statement."""
    gain, pad = ratio_pad[0], ratio_pad[1]
    coords[:, [0, 2]] -= pad[0]
    coords[:, [0, 2]] /= gain[0]
    coords[:, [1, 3]] -= pad[1]
    coords[:, [1, 3]] /= gain[0]
    coords[:, 0].clamp_(0, img0_shape[1])
    coords[:, 1].clamp_(0, img0_shape[0])
    coords[:, 2].clamp_(0, img0_shape[1])
    coords[:, 3].clamp_(0, img0_shape[0])
    return coords


def test_scale_coords_batch_equals_the_per_image_loop():
    do = _do()
    pred = cases.head_output(11, 3, 200, 2)
    pred[1, :, 4] = 0.0                                               # an image without detections
    pred[2, :5, 0] = [-50, 900, 320, 1, 639.5]                        # corners outside the frame: clamped
    rows = do.nms_host(pred, 0.25, 0.45, max_det=40)
    det, count = cases.pad(rows, 40)
    # what DetectorFrontEnd.prepare returns: ((h0, w0), ((gain_y, gain_x), (pad_x, pad_y)))
    shapes = [((240, 304), ((640 / 304 * 304 / 304, 640 / 304), (0.0, 67.36842105263158))),
              ((480, 640), ((1.0, 1.0), (0.0, 80.0))),
              ((100, 333), ((1.9219219219219218, 1.921921921921922), (0.3, 223.9))),]
    got = do.scale_coords_batch(torch.from_numpy(det), torch.from_numpy(count), (640, 640), shapes)
    assert got.dtype == torch.float32 and tuple(got.shape) == det.shape
    for b in range(3):
        want = torch.from_numpy(rows[b].copy())
        _scale_coords_reference(want[:, :4], shapes[b][0], shapes[b][1])
        assert_bit_equal(got[b, :count[b]].numpy(), want.numpy(), "image %d" % b)
        assert not got[b, count[b]:].numpy().view(np.uint32).any(), "rows beyond count stay 0"
    assert_bit_equal(det, cases.pad(rows, 40)[0], "the input is left as it was")
    with pytest.raises(ValueError):
        do.scale_coords_batch(torch.from_numpy(det), torch.from_numpy(count), (640, 640), shapes[:2])


def test_refusals():
    do = _do()
    pred = torch.from_numpy(cases.head_output(1, 1, 8, 2))
    for fn in (do.non_max_suppression, do.nms_host):
        with pytest.raises(AssertionError, match="conf_thresh must be in 0.0 to 1.0, however 1.5 is provided."):
            fn(pred, conf_thres=1.5)
        with pytest.raises(AssertionError, match="iou_thres must be in 0.0 to 1.0, however -0.1 is provided."):
            fn(pred, iou_thres=-0.1)
    with pytest.raises(AssertionError, match="conf_thresh"):
        do.nms_batch(pred, conf_thres=-1)
    with pytest.raises(ValueError, match="CUDA"):
        do.nms_batch(pred)


def _argcheck_lib():
    from event_representation_study_amd import build, _lib
    build.build(verbose=False)
    return _lib, _lib.load()


def test_symbol_is_declared_bound_and_a_status_entry():
    import re
    _lib, lib = _argcheck_lib()
    assert _lib.ABI_VERSION == 3 and lib.evrep_abi_version() == 3
    entry = _lib.SYMBOLS["evrep_nms"]
    assert isinstance(entry, _lib.Status) and entry[0] is ctypes.c_int and len(entry[1]) == 15
    assert entry[1][4] is ctypes.c_float and entry[1][5] is ctypes.c_double
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "evrep.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+evrep_nms\s*\(([^)]*)\)", text)
    assert decl and len(decl.group(1).split(",")) == 15
    assert getattr(lib, "evrep_nms") is not None
    assert not [n for n in _lib.SYMBOLS if "nms" in n and n.endswith("_scratch_bytes")]
    defines = dict(re.findall(r"^#define\s+EVREP_(NMS_[A-Z_]+)\s+\(?([0-9<u ]+)\)?\s*$", text, flags=re.M))
    assert eval(defines["NMS_MAX_ROWS"]) == _lib.NMS_MAX_ROWS and int(defines["NMS_MAX_DET"]) == _lib.NMS_MAX_DET
    assert int(defines["NMS_MAX_CLASSES"]) == _lib.NMS_MAX_CLASSES
    assert int(defines["NMS_MULTI_LABEL"].rstrip("u")) == _lib.NMS_MULTI_LABEL and int(defines["NMS_AGNOSTIC"].rstrip("u")) == _lib.NMS_AGNOSTIC


def test_kernel_source_is_part_of_the_detector_unit():
    from event_representation_study_amd import build
    deps = [os.path.basename(p) for p in build.unit_deps("evrep_capi_detin.hip")]
    assert "evrep_nms.hip" in deps and "evrep_ranksort.h" in deps
    assert len(build.SOURCES) == 15 and "evrep_nms.hip" not in build.SOURCES


def test_arguments_outside_the_stated_ranges_are_einval_before_any_launch():
    """No device is needed: every refusal comes before the launch.  The pointers are aligned host addresses never read."""
    _lib, lib = _argcheck_lib()
    buf = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(buf) + 255) & ~255
    P = ctypes.c_void_p

    def call(pred=base, B=1, N=8, C=2, conf=0.25, iou=0.45, flags=0, classes=None, n_classes=-1, max_nms=30000, max_det=300,
             det=base + 256, count=base + 512, scratch=base + 1024):
        return lib.evrep_nms(P(pred), B, N, C, conf, iou, flags, classes, n_classes, max_nms, max_det, P(det), P(count), P(scratch), None)

    bad = [dict(B=0), dict(B=65536), dict(N=0), dict(C=0), dict(C=4097), dict(N=1 << 23, C=3), dict(max_det=0), dict(max_det=1025),
           dict(max_nms=0), dict(conf=-0.1), dict(conf=1.5), dict(conf=float("nan")), dict(iou=1.01), dict(iou=float("nan")),
           dict(flags=4), dict(n_classes=-2), dict(n_classes=1, classes=None), dict(n_classes=(1 << 24) + 1, classes=_lib.int32_array([1])), dict(pred=0), dict(det=0), dict(count=0), dict(scratch=0),
           dict(pred=base + 2), dict(det=base + 258), dict(count=base + 513), dict(scratch=base + 1032),
           dict(B=65535, N=1 << 24, C=1)]
    for kw in bad:
        assert call(**kw) == _lib.EVREP_EINVAL, kw
    # the scratch of the worst case is stated through an existing size function: five arrays of B * R as four of `total`
    do = _do()
    for B, N, C, multi in [(1, 1, 1, False), (3, 1100, 80, True), (3, 1100, 80, False), (32, 8400, 80, True), (1, 7, 3, True)]:
        R = N * C if multi and C > 1 else N
        total = do.nms_scratch_total(B, N, C, multi)
        assert int(lib.evrep_dense_rank_scratch_bytes(B, total)) >= 5 * B * R * 4
        assert total <= 5 * (B * R // 4 + 1)
