"""CPU: the host restatement of the training targets (detector_assign.preprocess_host / tal_host) against the golden recorded
from the reference's own ComputeLoss.preprocess and TaskAlignedAssigner.forward, hand-built cases with stated expectations,
the registry against the header, and the refusals.

Tolerance.  Labels, boxes, fg, the padded labels and the zero pattern of the scores are compared bit for bit.  The scores are
compared within rtol = 64 * 2^-53: both sides are float64; a key differs by at most six roundings (the repeated multiplication
of iou^6 and the product with the score) against torch's pow of about one ulp, and a score is two keys and three further
operations.  Observed against the golden: 6.5e-16.

HAND holds the hand-built cases as builders; test_gpu_detector_assign.py runs the device on every one of them."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, assert_bit_equal, load_golden

F32, F64 = np.float32, np.float64
RTOL = 64 * 2.0 ** -53


def _da():
    from event_representation_study_amd import detector_assign
    return detector_assign


def golden_names():
    return ["s64_b1_nc1", "s64_b4_nc80", "s128_b4_nc2", "s128_b1_nc2", "s640_b1_nc2", "no_labels_m0", "nested",
            "centres_0_1_12_13_14", "m101"]


def test_the_golden_holds_the_cases_the_builders_name():
    import detector_assign_cases as cases
    g = load_golden("detector_assign")
    assert sorted({k.split("/")[0] for k in g}) == sorted(golden_names()) == sorted(cases.golden_cases())
    assert g["m101/gt"].shape == (2, 101, 5) and g["no_labels_m0/gt"].shape == (2, 0, 5) and g["s640_b1_nc2/anc"].shape == (8400, 2)
    for name, (seed, S, B, nc, targets) in cases.golden_cases().items():
        assert_bit_equal(g[name + "/targets"], targets, name)


# ------------------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("name", golden_names())
def test_preprocess_host_equals_the_reference(name):
    g = load_golden("detector_assign")
    S, B, nc = (int(v) for v in g[name + "/size"])
    gt, n_labels, status = _da().preprocess_host(g[name + "/targets"], B, S, S)
    assert_bit_equal(gt, g[name + "/gt"], name)
    assert not status.any() and n_labels.max(initial=0) == gt.shape[1]


@pytest.mark.parametrize("name", golden_names())
def test_tal_host_equals_the_reference(name):
    g = load_golden("detector_assign")
    labels, boxes, scores, fg, status = _da().tal_host(g[name + "/pd_scores"], g[name + "/pd_bboxes"], g[name + "/anc"], g[name + "/gt"])
    assert_bit_equal(labels, g[name + "/labels"], name + " labels")
    assert_bit_equal(boxes, g[name + "/boxes"], name + " boxes")
    assert_bit_equal(fg, g[name + "/fg"], name + " fg")
    want = g[name + "/scores"]
    assert np.array_equal(scores != 0, want != 0), name + ": the zero pattern"
    nz = want != 0
    err = float((np.abs(scores - want)[nz] / np.abs(want[nz])).max()) if nz.any() else 0.0
    print("%s: greatest relative score error %.3g (rtol %.3g)" % (name, err, RTOL))
    assert err <= RTOL
    assert not status.any()


def test_the_drop_in_class_on_cpu_tensors_equals_the_reference_and_keeps_its_dtypes():
    da = _da()
    g = load_golden("detector_assign")
    name = "s64_b4_nc80"
    gt = torch.from_numpy(g[name + "/gt"])
    tal = da.TaskAlignedAssigner(topk=13, num_classes=80, alpha=1.0, beta=6.0)
    out = tal(torch.from_numpy(g[name + "/pd_scores"]), torch.from_numpy(g[name + "/pd_bboxes"]), torch.from_numpy(g[name + "/anc"]),
              gt[:, :, :1], gt[:, :, 1:], (gt[:, :, 1:].sum(-1, keepdim=True) > 0).float())
    assert [t.dtype for t in out] == [torch.int64, torch.float64, torch.float64, torch.bool]
    assert_bit_equal(out[0].numpy(), g[name + "/labels"])
    assert_bit_equal(out[3].numpy(), g[name + "/fg"])
    np.testing.assert_allclose(out[2].numpy(), g[name + "/scores"], rtol=RTOL, atol=0)
    # float32 gt tensors (the reference's CPU fall-back) are widened; the result is the float64 one rounded once
    out32 = tal(torch.from_numpy(g[name + "/pd_scores"]), torch.from_numpy(g[name + "/pd_bboxes"]), torch.from_numpy(g[name + "/anc"]),
                gt[:, :, :1].float(), gt[:, :, 1:].float(), None)
    assert out32[1].dtype == torch.float32 and out32[2].dtype == torch.float32 and tal.last_status.tolist() == [0, 0, 0, 0]
    gt32 = torch.cat([gt[:, :, :1], gt[:, :, 1:].float().double()], 2).numpy()
    want = da.tal_host(g[name + "/pd_scores"], g[name + "/pd_bboxes"], g[name + "/anc"], gt32, out_dtype=F32)
    assert_bit_equal(out32[2].numpy(), want[2])


def test_preprocess_of_cpu_targets_gives_the_reference_m():
    da = _da()
    g = load_golden("detector_assign")
    gt = da.preprocess(torch.from_numpy(g["s128_b4_nc2/targets"]), 4, 128, 128)
    assert gt.dtype == torch.float64 and not gt.is_cuda
    assert_bit_equal(gt.numpy(), g["s128_b4_nc2/gt"])
    assert tuple(da.preprocess(torch.zeros((0, 6)), 3, 64, 64).shape) == (3, 0, 5)


# ------------------------------------------------------------------------------------------------------------ hand-built cases
def _line(n=5):
    """n anchors on a line, 8 apart, y = 4."""
    return np.stack([np.arange(n, dtype=F32) * 8 + 4, np.full(n, 4, F32)], 1)


def _around(anc, half=5.0):
    return np.concatenate([anc - half, anc + half], 1).astype(F32)[None]


def case_zero_key_tie():
    """Box over anchors 0..3; the predictions of 0 and 1 lie far away (IoU 0, key 0).  topk = 3: the two positive keys, then the
    zero key of LOWEST index, anchor 0 -- in the box, so it becomes foreground with score 0; anchor 1 does not."""
    anc = _line()
    boxes = _around(anc)
    boxes[0, 0] = boxes[0, 1] = [100, 100, 110, 110]
    return dict(scores=np.full((1, 5, 1), 0.5, F32), boxes=boxes, anc=anc, gt=np.array([[[0, 0, 0, 32, 8]]], F64), topk=3)


def case_equal_keys():
    """Anchors 2 and 3 carry the same prediction and score: equal keys, topk = 1 keeps the lower index."""
    anc = _line()
    boxes = _around(anc)
    boxes[0, 2] = boxes[0, 3] = [14, 0, 30, 8]
    return dict(scores=np.full((1, 5, 2), 0.25, F32), boxes=boxes, anc=anc, gt=np.array([[[1, 12.5, 0, 32, 8]]], F64), topk=1)


def case_centre_on_an_edge():
    """x1 = 12 exactly: anchor 1 (x = 12) is outside, anchors 2 and 3 inside.  Row 1: y2 = 4 + 1125899 * 2^-50 leaves
    d = 9.9999992e-10 (the subtraction is exact), not > 1e-9: it reaches no anchor; one ulp more (1.00000000008e-9) and it reaches all."""
    anc = _line()
    gt = np.array([[[0, 12, 0, 32, 8], [0, 0, 0, 40, 4 + 1125899 * 2.0 ** -50]]], F64)
    return dict(scores=np.full((1, 5, 1), 0.5, F32), boxes=_around(anc), anc=anc, gt=gt, topk=13)


def case_greatest_iou_row_is_no_candidate():
    """Anchor 2 is a candidate of rows 0 and 1 (IoU 0.377 and 0.327); row 2's box is the right half of its prediction, the centre
    on its edge: IoU 0.5, the greatest, so row 2 wins although anchor 2 is not in its box (which holds no centre at all)."""
    anc = _line()
    boxes = _around(anc)                                                # anchor 2: [15, -1, 25, 9]
    gt = np.array([[[0, 8, 0, 32, 8], [1, 16, 0, 40, 8], [1, 20, -1, 25, 9]]], F64)
    return dict(scores=np.full((1, 5, 2), 0.5, F32), boxes=boxes, anc=anc, gt=gt, topk=2)


def case_padded_row_in_the_middle():
    anc = _line()
    gt = np.array([[[1, 0, 0, 16, 8], [-1, 0, 0, 0, 0], [0, 24, 0, 40, 8]]], F64)
    return dict(scores=np.full((1, 5, 2), 0.5, F32), boxes=_around(anc), anc=anc, gt=gt, topk=13)


def case_class_out_of_range():
    anc = _line()
    gt = np.array([[[2, 0, 0, 16, 8], [1, 24, 0, 40, 8], [-3, 8, 0, 24, 8]]], F64)
    return dict(scores=np.full((1, 5, 2), 0.5, F32), boxes=_around(anc), anc=anc, gt=gt, topk=13)


def case_nan_and_inf():
    anc = _line()
    scores = np.full((3, 5, 2), 0.5, F32)
    boxes = np.repeat(_around(anc), 3, 0)
    scores[1, 4, 1] = np.nan
    boxes[2, 0, 2] = np.inf
    gt = np.repeat(np.array([[[1, 0, 0, 16, 8]]], F64), 3, 0)
    return dict(scores=scores, boxes=boxes, anc=anc, gt=gt, topk=13)


def case_float32_area():
    """Both predictions contain the box; their exact areas differ by 6.5e-9 relative (the second is smaller) and their float32
    areas are equal.  The reference's float32 area gives equal IoUs and keys, topk = 1 keeps anchor 0; a float64 area would give
    anchor 1 the greater IoU.  Found by search over float32 widths and heights."""
    anc = np.array([[12, 16], [20, 16]], F32)
    boxes = np.array([[[0, 0, 40.8724250793457, 29.69145965576172], [0, 0, 39.10895538330078, 31.030282974243164]]], F32)
    return dict(scores=np.full((1, 2, 1), 0.5, F32), boxes=boxes, anc=anc, gt=np.array([[[0, 8, 8, 24, 24]]], F64), topk=1)


HAND = {f.__name__[5:]: f for f in (case_zero_key_tie, case_equal_keys, case_centre_on_an_edge, case_greatest_iou_row_is_no_candidate,
                                    case_padded_row_in_the_middle, case_class_out_of_range, case_nan_and_inf, case_float32_area)}


def run_host(c, out_dtype=F64):
    return _da().tal_host(c["scores"], c["boxes"], c["anc"], c["gt"], topk=c["topk"], out_dtype=out_dtype)


def test_zero_key_tie_goes_to_the_lowest_index():
    labels, boxes, scores, fg, status = run_host(case_zero_key_tie())
    assert fg[0].tolist() == [True, False, True, True, False]
    assert scores[0, 0, 0] == 0 and scores[0, 2, 0] > 0 and scores[0, 3, 0] > 0 and status.tolist() == [0]


def test_equal_keys_keep_the_lower_index():
    labels, boxes, scores, fg, status = run_host(case_equal_keys())
    assert fg[0].tolist() == [False, False, True, False, False] and labels[0].tolist() == [1] * 5
    assert scores[0, 2, 1] > 0 and scores[0, 2, 0] == 0


def test_a_centre_on_an_edge_is_outside():
    c = case_centre_on_an_edge()
    labels, boxes, scores, fg, status = run_host(c)
    assert fg[0].tolist() == [False, False, True, True, False], "row 1 reaches no anchor: d = 1125899 * 2^-50 is not > 1e-9"
    c["gt"][0, 1, 4] = 4 + 1125900 * 2.0 ** -50
    assert run_host(c)[3][0].tolist() == [True, True, True, True, True]


def test_the_greatest_iou_row_wins_without_being_a_candidate():
    da = _da()
    c = case_greatest_iou_row_is_no_candidate()
    d = {}
    da.tal_image_host(c["scores"][0], c["boxes"][0], c["anc"], c["gt"][0], 2, 2, 1, 6, details=d)
    assert d["count"][2] == 2 and not d["in_gt"][2, 2] and d["iou"][:, 2].argmax() == 2
    labels, boxes, scores, fg, status = run_host(c)
    assert fg[0, 2] and boxes[0, 2].tolist() == [20, -1, 25, 9] and labels[0, 2] == 1
    # pos_al of row 2 is the out-of-box metric of its only anchor: the score is pos_ov * al / (al + 1e-9)
    al, iou = d["al"][2, 2], d["iou"][2, 2]
    assert scores[0, 2, 1] == (al * iou) / (al + 1e-9) > 0


def test_background_anchors_carry_row_0_and_a_padded_row_in_the_middle_claims_nothing():
    labels, boxes, scores, fg, status = run_host(case_padded_row_in_the_middle())
    assert fg[0].tolist() == [True, True, False, True, True]
    assert labels[0].tolist() == [1, 1, 1, 0, 0], "the background anchor 2 carries row 0's class"
    assert boxes[0, 2].tolist() == [0, 0, 16, 8] and boxes[0, 3].tolist() == [24, 0, 40, 8] and status.tolist() == [0]
    assert not scores[0, 2].any() and scores[0, 0, 1] > 0 and scores[0, 3, 0] > 0


def test_a_class_out_of_range_sets_its_bit_and_counts_as_padding():
    da = _da()
    labels, boxes, scores, fg, status = run_host(case_class_out_of_range())
    assert status.tolist() == [da.ST_BAD_CLASS]
    assert fg[0].tolist() == [False, False, False, True, True], "rows 0 (class 2 of 2) and 2 (class -3) claim nothing"
    assert labels[0].tolist() == [0, 0, 0, 1, 1] and boxes[0, 0].tolist() == [0, 0, 16, 8]


def test_nan_and_inf_blank_their_image_only():
    da = _da()
    labels, boxes, scores, fg, status = run_host(case_nan_and_inf())
    assert status.tolist() == [0, da.ST_NONFINITE, da.ST_NONFINITE]
    assert fg[0].any() and not fg[1:].any() and not scores[1:].any() and np.isfinite(scores).all()
    assert labels[1].tolist() == [1] * 5 and boxes[2, 0].tolist() == [0, 0, 16, 8]


def test_more_than_m_labels_keep_the_first_m():
    da = _da()
    t = np.array([[0, 1, .5, .5, .2, .2], [1, 0, .5, .5, .2, .2], [0, 2, .25, .25, .1, .1], [0, 3, .75, .75, .1, .1]], F32)
    gt, n_labels, status = da.preprocess_host(t, 2, 64, 64, max_labels=2)
    assert status.tolist() == [da.ST_LABEL_OVERFLOW, 0] and n_labels.tolist() == [3, 1]
    assert gt[0, :, 0].tolist() == [1, 2] and gt[1, :, 0].tolist() == [0, -1] and gt[1, 1].tolist() == [-1, 0, 0, 0, 0]
    whole = da.preprocess_host(t, 2, 64, 64)[0]
    assert whole.shape == (2, 3, 5) and whole[0, :, 0].tolist() == [1, 2, 3]


def test_preprocess_forms_x2_from_the_updated_x1():
    """x2 = x1 + bw, not bx + bw / 2: values (found by search) at which the two differ in the last place."""
    da = _da()
    cx, w, W = F32(0.13167430460453033), F32(0.0005333033623173833), F32(333.3)
    gt = da.preprocess_host(np.array([[0, 0, cx, cx, w, w]], F32), 1, W, W)[0]
    bx, bw = F64(cx) * F64(W), F64(w) * F64(W)
    x1 = bx - bw * 0.5
    assert gt[0, 0, 1] == x1 and gt[0, 0, 3] == x1 + bw == 43.97591911941277 and x1 + bw != bx + bw * 0.5
    assert gt[0, 0, 2] == x1 and gt[0, 0, 4] == x1 + bw


def test_the_predicted_area_is_float32():
    c = case_float32_area()
    labels, boxes, scores, fg, status = run_host(c)
    assert fg[0].tolist() == [True, False], "equal float32 areas: equal keys, the lower index"
    p = c["boxes"][0].astype(F64)
    area64 = (p[:, 2] - p[:, 0]) * (p[:, 3] - p[:, 1])
    area32 = ((c["boxes"][0][:, 2] - c["boxes"][0][:, 0]) * (c["boxes"][0][:, 3] - c["boxes"][0][:, 1]))
    assert area32[0] == area32[1] and area64[1] < area64[0], "a float64 area would have preferred anchor 1"
    assert 256.0 / (area64[1] + 1e-9) > 256.0 / (area64[0] + 1e-9)


def test_exponents_are_integers_in_0_to_16():
    da = _da()
    c = case_zero_key_tie()
    a0 = da.tal_host(c["scores"], c["boxes"], c["anc"], c["gt"], topk=3, alpha=0, beta=0)
    assert a0[3][0].tolist() == [True, True, True, False, False], "x^0 = 1: every in-box key is 1, the lowest indices win"
    pos_ov = da._iou_host(c["gt"][0, :, 1:], c["boxes"][0])[0, 2]      # anchors 0 and 1 have IoU 0
    assert a0[2][0, :, 0].tolist() == [(1.0 * pos_ov) / (1.0 + 1e-9)] * 3 + [0.0, 0.0] and pos_ov > 0
    for bad in (0.5, 17, -1):
        with pytest.raises(NotImplementedError):
            da.tal_host(c["scores"], c["boxes"], c["anc"], c["gt"], beta=bad)
        with pytest.raises(NotImplementedError):
            da.TaskAlignedAssigner(alpha=bad)


def test_anchor_points_are_generate_anchors_points():
    da = _da()
    anc, strides = da.anchor_points(640)
    g = load_golden("detector_assign")
    assert_bit_equal(anc, g["s640_b1_nc2/anc"])
    assert anc.shape == (8400, 2) and strides.shape == (8400, 1) and anc[0].tolist() == [4, 4] and anc[6400].tolist() == [8, 8]
    assert strides[6399, 0] == 8 and strides[6400, 0] == 16 and strides[-1, 0] == 32 and anc[-1].tolist() == [624, 624]
    assert da.anchor_points((64, 128))[0].shape == (8 * 16 + 4 * 8 + 2 * 4, 2)


# ---------------------------------------------------------------------------------------------- the registry and the refusals
def test_registry_header_and_library_agree():
    from event_representation_study_amd import _lib, build
    build.build()
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "evrep.h")).read(), flags=re.S)
    for name, nargs in (("evrep_det_targets_pad", 10), ("evrep_tal_workspace_bytes", 3), ("evrep_tal_assign", 19)):
        decl = re.search(r"\b%s\s*\(([^;]*)\);" % name, text)
        assert decl and len(decl.group(1).split(",")) == nargs == len(_lib.SYMBOLS[name][1]), name
        assert getattr(lib, name) is not None
    assert isinstance(_lib.SYMBOLS["evrep_tal_assign"], _lib.Status) and isinstance(_lib.SYMBOLS["evrep_det_targets_pad"], _lib.Status)
    full = open(os.path.join(ROOT, "include", "evrep.h")).read()
    for name in ("F32_OUT", "MAX_TOPK", "MAX_LABELS", "MAX_CLASSES", "MAX_POWER", "ST_LABEL_OVERFLOW", "ST_BAD_CLASS", "ST_NONFINITE"):
        m = re.search(r"^#define\s+EVREP_TAL_%s\s+(\d+)u?\s*$" % name, full, flags=re.M)
        assert m and int(m.group(1)) == getattr(_lib, "TAL_" + name), name
    assert re.search(r"^#define\s+EVREP_TAL_MAX_ANCHORS\s+\(1 << 24\)", full, flags=re.M) and _lib.TAL_MAX_ANCHORS == 1 << 24
    assert lib.evrep_abi_version() == 3 and len(build.SOURCES) == 15


# (B, M, A) -> bytes: three 32-bit words and one double per (image, anchor), two 64-bit words per (image, row), each array
# rounded up to 256 bytes (an empty one takes none); 0 for a shape evrep_tal_assign refuses.  One tuple per edge of the formula.
_TAL_WORKSPACE_SIZES = [
    ((0, 5, 84), 0), ((1, -1, 84), 0), ((1, 1025, 84), 0), ((1, 5, 0), 0), ((65536, 5, 84), 0), ((1, 5, (1 << 24) + 1), 0),
    ((1, 0, 84), 3 * 512 + 768), ((1, 1, 64), 3 * 256 + 512 + 2 * 256), ((1, 1, 65), 3 * 512 + 768 + 2 * 256),
    ((2, 33, 84), 3 * 768 + 1536 + 2 * 768), ((32, 50, 8400), 3 * 1075200 + 2150400 + 2 * 12800),
    ((65535, 1024, 1 << 24), 20 * 65535 * (1 << 24) + 2 * 8 * 65535 * 1024),
]


def test_the_workspace_size_is_the_published_one():
    """The size is a contract: callers size allocations they keep across library versions with it.  The expectations are the
    layout stated in include/evrep.h worked out by hand, not what the library returned."""
    from event_representation_study_amd import _lib, build
    build.build()
    lib = _lib.load()
    assert _lib.SYMBOLS["evrep_tal_workspace_bytes"][0] is ctypes.c_size_t
    for args, size in _TAL_WORKSPACE_SIZES:
        assert lib.evrep_tal_workspace_bytes(*args) == size, args


def test_the_entry_points_refuse_bad_arguments_before_any_launch():
    import ctypes
    from event_representation_study_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    good = [P(0x1000), P(0x2000), P(0x3000), P(0x4000), 2, 3, 84, 2, 13, 1, 6, 0, P(0x5000), P(0x6000), P(0x7000), P(0x8000), P(0x9000),
            P(0xA000), None]
    def call(**change):
        args = list(good)
        for i, v in change.items():
            args[int(i[1:])] = v
        return lib.evrep_tal_assign(*args)
    for change in (dict(a4=0), dict(a4=65536), dict(a5=-1), dict(a5=1025), dict(a6=0), dict(a7=0), dict(a7=4097), dict(a8=0), dict(a8=65),
                   dict(a9=-1), dict(a9=17), dict(a10=17), dict(a11=2), dict(a0=None), dict(a1=P(0x2002)), dict(a3=None), dict(a3=P(0x4004)),
                   dict(a12=P(0x5004)), dict(a13=P(0x6004)), dict(a16=None), dict(a17=P(0xA080)), dict(a17=None),
                   dict(a6=1 << 24, a7=4096)):
        assert call(**change) == _lib.EVREP_EINVAL, change
    pad = [P(0x1000), 4, 2, 3, 64.0, 64.0, P(0x2000), P(0x3000), P(0x4000), None]
    for i, v in ((0, None), (2, 0), (3, -1), (3, 1025), (4, float("nan")), (5, float("inf")), (6, None), (6, P(0x2004)), (7, None), (8, None), (1, -1)):
        args = list(pad)
        args[i] = v
        assert lib.evrep_det_targets_pad(*args) == _lib.EVREP_EINVAL, (i, v)


def test_the_python_routes_refuse_what_they_do_not_compute():
    da = _da()
    c = case_equal_keys()
    s, p, a, gt = (torch.from_numpy(c[k]) for k in ("scores", "boxes", "anc", "gt"))
    with pytest.raises(ValueError, match="1e-9"):
        da.TaskAlignedAssigner(eps=1e-7)
    with pytest.raises(ValueError, match="topk"):
        da.TaskAlignedAssigner(topk=65)
    tal = da.TaskAlignedAssigner(topk=1, num_classes=2)
    with pytest.raises(ValueError, match=r"\.float\(\)"):
        tal(s.double(), p, a, gt[:, :, :1], gt[:, :, 1:], None)
    with pytest.raises(ValueError, match="classes"):
        da.TaskAlignedAssigner(num_classes=3)(s, p, a, gt[:, :, :1], gt[:, :, 1:], None)
    with pytest.raises(ValueError, match="CUDA"):
        da.assign_batch(s, p, a, torch.zeros((0, 6)), (64, 64), 2)
    with pytest.raises(ValueError, match="topk"):
        da.tal_host(c["scores"], c["boxes"], c["anc"], c["gt"], topk=0)
