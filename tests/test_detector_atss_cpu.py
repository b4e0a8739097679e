"""CPU: the ATSS assigner of the warm-up epochs.  The host restatement detector_assign.atss_host against the golden recorded from
the reference's own ATSSAssigner.forward (tests/golden/make_golden_detector_atss.py) BIT FOR BIT in every output -- the cases
are ones the reference decides without help, so no tolerance is due --, the drop-in class on CPU tensors, the refusals, the
registry and the published workspace size, and ComputeLoss(warmup_assigner="atss") on CPU tensors.

HAND holds the cases the golden must not hold (the reference leaves them open, or fails on them) with what the rules say
about each; test_gpu_detector_atss.py runs the kernel on the same cases."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import assert_bit_equal, load_golden
import detector_assign_cases as tal_cases
import detector_atss_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64


def _da():
    from event_representation_study_amd import detector_assign
    return detector_assign


def golden_names():
    return sorted(cases.golden_cases())


def golden_case(name):
    g = load_golden("detector_atss")
    pd = g[name + "/pd_bboxes"] if name + "/pd_bboxes" in g else None
    H, W, B, nc = (int(v) for v in g[name + "/size"])
    return g, pd, (H, W), B, nc


# ------------------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("name", golden_names())
def test_host_equals_the_reference(name):
    da = _da()
    g, pd, (H, W), B, nc = golden_case(name)
    anchors, counts = da.anchor_boxes((H, W))
    assert_bit_equal(anchors, g[name + "/anchors"], name + " anchors")
    assert counts == g[name + "/levels"].tolist()
    gt, _, st = da.preprocess_host(g[name + "/targets"], B, W, H)
    assert_bit_equal(gt, g[name + "/gt"], name + " preprocess")
    labels, boxes, scores, fg, status = da.atss_host(anchors, counts, gt, pd, cases.TOPK, nc)
    assert labels.dtype == np.int64 and boxes.dtype == F64 and scores.dtype == F32 and fg.dtype == bool
    assert_bit_equal(labels, g[name + "/labels"], name + " labels")
    assert_bit_equal(boxes, g[name + "/boxes"], name + " boxes")
    assert_bit_equal(scores, g[name + "/scores"], name + " scores")
    assert_bit_equal(fg, g[name + "/fg"], name + " fg")
    assert not status.any() and not st.any()
    assert (labels[~fg] == nc).all() and (labels[fg] < nc).all()


def test_the_golden_holds_what_it_was_recorded_for():
    g = load_golden("detector_atss")
    assert sorted({k.split("/")[0] for k in g}) == golden_names()
    assert g["no_labels_m0/gt"].shape == (2, 0, 5) and not g["no_labels_m0/fg"].any() and (g["no_labels_m0/labels"] == 2).all()
    assert "no_pd/pd_bboxes" not in g and set(np.unique(g["no_pd/scores"])) == {0.0, 1.0}
    assert g["s96_b2/levels"].tolist() == [144, 36, 9] and g["rect_96x160/levels"].tolist() == [240, 60, 15]
    assert g["s640_b1/anchors"].shape == (8400, 4) and g["s640_b1/anchors"][0].tolist() == [-16, -16, 24, 24]
    assert not g["s128_b3_one_empty/fg"][1].any() and g["s128_b3_one_empty/fg"][0].any()
    assert g["s160_nc1_m12/gt"].shape[1] == 12 and g["s96_large20/gt"].shape[1] == 20
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "detector_atss.npz")) <= os.path.getsize(
        os.path.join(ROOT, "tests", "golden", "detector_assign.npz"))


# -------------------------------------------------------------------------------------------------------- the hand-built cases
def grid_anchors(levels, cell=5.0):
    """Anchor boxes as generate_anchors lays them out, for levels [(rows, columns, stride), ...]: ((A, 4) float32, counts)."""
    boxes, counts = [], []
    for nh, nw, s in levels:
        x, y = ((np.arange(nw, dtype=F32) + F32(0.5)) * F32(s)).astype(F32), ((np.arange(nh, dtype=F32) + F32(0.5)) * F32(s)).astype(F32)
        yy, xx = np.meshgrid(y, x, indexing="ij")
        half = F32(cell * s * 0.5)
        boxes.append(np.stack([xx - half, yy - half, xx + half, yy + half], axis=-1).reshape(-1, 4).astype(F32))
        counts.append(nh * nw)
    return np.concatenate(boxes, 0), counts


def rows(*cls_boxes, M=None):
    """gt (1, M, 5) float64 from (cls, x1, y1, x2, y2) rows, padded with [-1, 0, 0, 0, 0]."""
    gt = np.zeros((1, M or len(cls_boxes), 5), F64)
    gt[:, :, 0] = -1.0
    gt[0, :len(cls_boxes)] = np.array(cls_boxes, F64)
    return gt


def _pd_for(seed, B, anchors):
    rng = np.random.default_rng(seed)
    c = np.stack([(anchors[:, 0] + anchors[:, 2]) / 2, (anchors[:, 1] + anchors[:, 3]) / 2], axis=1)[None] + rng.normal(0, 3, (B, len(anchors), 2))
    half = rng.uniform(4, 40, (B, len(anchors), 2))
    return np.concatenate([c - half, c + half], axis=2).astype(F32)


def _case(anchors, counts, gt, nc=2, topk=9, pd_seed=1):
    return dict(anchors=anchors, counts=counts, gt=gt, nc=nc, topk=topk, pd=None if pd_seed is None else _pd_for(pd_seed, gt.shape[0], anchors))


def case_grid_corner():
    """A label centred exactly on (64, 64), a corner of the grid at all three levels of S = 128: the four anchors about it are
    equally far at every level, and so are the rings behind them."""
    anchors, counts = _da().anchor_boxes(128)
    return _case(anchors, counts, rows((1, 32, 32, 96, 96), (0, 40, 48, 88, 80)))


def case_equal_overlaps():
    """Rows 0 and 2 are one box under two classes, row 1 lies inside them: every positive anchor of row 0 is one of row 2 with the
    same IoU, and the first row wins."""
    anchors, counts = _da().anchor_boxes(128)
    return _case(anchors, counts, rows((1, 20.5, 30.25, 100.5, 110.75), (0, 41.0, 47.5, 85.25, 90.0), (0, 20.5, 30.25, 100.5, 110.75)))


def _chunk_case(levels, seed):
    anchors, counts = grid_anchors(levels)
    rng = np.random.default_rng(seed)
    nh, nw, s = levels[0]
    W, H = nw * s, nh * s
    boxes = []
    for i in range(6):                                                  # the last labels lie at the far end of the first level
        w, h = rng.uniform(0.3, 0.9) * min(W, 6 * s), rng.uniform(0.3, 0.9) * min(H, 6 * s)
        x1 = rng.uniform(0, W - w) if i < 3 else W - w - rng.uniform(0, s)
        y1 = rng.uniform(0, H - h) if i < 3 else H - h - rng.uniform(0, min(s, H - h))
        boxes.append((i % 2, x1, y1, x1 + w, y1 + h))
    return _case(anchors, counts, rows(*boxes), pd_seed=seed)


def case_level_of_256():
    return _chunk_case([(16, 16, 8), (8, 8, 16), (4, 4, 32)], 11)       # S = 128


def case_level_of_257():
    return _chunk_case([(1, 257, 8), (1, 128, 16)], 12)


def case_level_of_289():
    return _chunk_case([(17, 17, 8), (8, 8, 16), (4, 4, 32)], 13)       # S = 136


def case_one_level_of_9():
    anchors, counts = grid_anchors([(3, 3, 32)])
    return _case(anchors, counts, rows((0, 10.5, 20.0, 80.0, 90.25), (1, 30.0, 5.0, 95.0, 60.5)))


def case_five_levels():
    anchors, counts = grid_anchors([(48, 48, 8), (24, 24, 16), (12, 12, 32), (6, 6, 64), (3, 3, 128)])
    gt = _da().preprocess_host(tal_cases.targets(31, [7], 2, lo=0.1, hi=0.8), 1, 384, 384)[0]
    return _case(anchors, counts, gt)


def case_topk_1_one_level():
    """n = 1: the deviation is 0 / 0, the threshold NaN, nothing is positive."""
    anchors, counts = grid_anchors([(8, 8, 16)])
    return _case(anchors, counts, rows((0, 10.5, 20.0, 80.0, 90.25), (1, 30.0, 5.0, 95.0, 60.5)), topk=1)


def case_topk_1_three_levels():
    anchors, counts = _da().anchor_boxes(128)
    return _case(anchors, counts, rows((0, 10.5, 20.0, 80.0, 90.25), (1, 30.0, 5.0, 95.0, 60.5)), topk=1)


def case_topk_32():
    anchors, counts = _da().anchor_boxes(256)
    gt = _da().preprocess_host(tal_cases.targets(32, [5, 9], 3, lo=0.1, hi=0.8), 2, 256, 256)[0]
    return _case(anchors, counts, gt, nc=3, topk=32)


def case_m101():
    anchors, counts = _da().anchor_boxes(128)
    gt = _da().preprocess_host(tal_cases.targets(33, [101, 3], 2), 2, 128, 128)[0]
    return _case(anchors, counts, gt)


def case_bad_class():
    anchors, counts = _da().anchor_boxes(128)
    return _case(anchors, counts, rows((1, 20.5, 30.25, 100.5, 110.75), (5, 41.0, 47.5, 85.25, 90.0), (-1, 10.0, 10.0, 60.0, 50.0)))


def case_nan_prediction():
    """A NaN among image 1's predicted boxes: that image is all background, the others are not touched."""
    anchors, counts = _da().anchor_boxes(96)
    gt = _da().preprocess_host(tal_cases.targets(34, [3, 4, 2], 2, lo=0.2, hi=0.7), 3, 96, 96)[0]
    c = _case(anchors, counts, gt)
    c["pd"][1, 77, 2] = np.nan
    return c


def case_inf_label_no_predictions():
    anchors, counts = _da().anchor_boxes(96)
    gt = _da().preprocess_host(tal_cases.targets(35, [3, 4], 2, lo=0.2, hi=0.7), 2, 96, 96)[0]
    gt[0, 1, 3] = np.inf
    return _case(anchors, counts, gt, pd_seed=None)


HAND = {f.__name__[5:]: f for f in (case_grid_corner, case_equal_overlaps, case_level_of_256, case_level_of_257, case_level_of_289,
                                    case_one_level_of_9, case_five_levels, case_topk_1_one_level, case_topk_1_three_levels, case_topk_32,
                                    case_m101, case_bad_class, case_nan_prediction, case_inf_label_no_predictions)}


def host(c, **kw):
    return _da().atss_host(c["anchors"], c["counts"], c["gt"], c["pd"], c["topk"], c["nc"], **kw)


def image_details(c, b=0):
    d = {}
    _da().atss_image_host(c["anchors"], c["counts"], c["gt"][b], None if c["pd"] is None else c["pd"][b], c["topk"], c["nc"], details=d)
    return d


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_built_cases_hold_what_they_are_for(name):
    da = _da()
    c = HAND[name]()
    labels, boxes, scores, fg, status = host(c)
    nc, B = c["nc"], c["gt"].shape[0]
    assert (labels[~fg] == nc).all() and (labels[fg] < nc).all() and not scores[~fg].any()
    assert (scores.astype(bool).sum(-1) <= 1).all()
    for b in range(B):                                                  # background carries row 0's box
        assert_bit_equal(boxes[b][~fg[b]], np.broadcast_to(c["gt"][b, 0, 1:], (int((~fg[b]).sum()), 4)))
    d = image_details(c)
    if name == "grid_corner":
        # the four nearest anchors of every level are equally far; the order takes them by index
        s0, want = 0, []
        for n_l in c["counts"]:
            dist = np.sort(d["distance"][0, s0:s0 + n_l])
            assert (dist[:4] == dist[0]).all() and (n_l == 16 or dist[8] == dist[9]), "ties at the nearest ring and at the cut"
            want += (np.argsort(d["distance"][0, s0:s0 + n_l], kind="stable")[:9] + s0).tolist()
            s0 += n_l
        assert d["candidates"][0].tolist() == want
        assert fg.any()
    elif name == "equal_overlaps":
        both = d["positive"][0] & d["positive"][2]
        assert both.any() and (d["overlap"][0] == d["overlap"][2]).all()
        multi = d["count"] > 1
        assert multi.any() and (labels[0][both] != 0).any()
        top = d["overlap"][:, both].argmax(0)
        assert set(top.tolist()) <= {0, 1} and (labels[0][both][top == 0] == 1).all()
    elif name.startswith("level_of_"):
        n0 = c["counts"][0]
        assert n0 == int(name.split("_")[-1])
        assert fg[0, :n0].any() and np.flatnonzero(fg[0, :n0]).max() >= n0 - 40, "anchors of the last chunk take part"
    elif name == "one_level_of_9":
        assert c["counts"] == [9] and all(sorted(v.tolist()) == list(range(9)) for v in d["candidates"].values())
    elif name == "five_levels":
        assert len(c["counts"]) == 5 and c["counts"][-1] == 9 and fg.any()
    elif name == "topk_1_one_level":
        assert np.isnan(d["thr"][:2]).all() and not fg.any() and not status.any()
    elif name == "topk_1_three_levels":
        assert np.isfinite(d["thr"][:2]).all()
    elif name == "topk_32":
        assert all(len(v) == 96 for v in d["candidates"].values()) and fg.all(1).sum() == 0 and fg.any(1).all()
    elif name == "m101":
        assert c["gt"].shape[1] == 101 and fg[0].sum() > fg[1].sum() > 0
    elif name == "bad_class":
        assert status.tolist() == [da.ST_BAD_CLASS] and fg.any() and not d["valid"][1] and not d["valid"][2]
    elif name == "nan_prediction":
        assert status.tolist() == [0, da.ST_NONFINITE, 0] and not fg[1].any() and fg[0].any() and fg[2].any()
        clean = dict(c, pd=np.nan_to_num(c["pd"], nan=1.0))
        for got, want in zip(host(c), host(clean)):
            assert_bit_equal(got[[0, 2]], want[[0, 2]])
    elif name == "inf_label_no_predictions":
        assert status.tolist() == [da.ST_NONFINITE, 0] and not fg[0].any() and set(np.unique(scores[1])) == {0.0, 1.0}


def test_storage_widths_hold_the_same_values():
    c = case_five_levels()
    ref = host(c)
    for bd in (F64, F32):
        for sd in (F64, F32):
            got = host(c, boxes_dtype=bd, scores_dtype=sd)
            assert got[1].dtype == bd and got[2].dtype == sd
            assert_bit_equal(got[1], ref[1].astype(bd))
            assert np.array_equal(got[2].astype(F64), ref[2].astype(F64)), "a float32 value in either width"


# ------------------------------------------------------------------------------------------------------------ the drop-in class
def test_the_drop_in_class_on_cpu_tensors():
    da = _da()
    name = "s128_b3_one_empty"
    g, pd, (H, W), B, nc = golden_case(name)
    gt = torch.from_numpy(g[name + "/gt"])
    anchors, counts = da.anchor_boxes((H, W))
    atss = da.ATSSAssigner(9, num_classes=nc)
    assert atss.topk == 9 and atss.bg_idx == nc and atss.last_status is None
    mask_gt = (gt[:, :, 1:].sum(-1, keepdim=True) > 0).float()
    out = atss(torch.from_numpy(anchors), counts, gt[:, :, :1], gt[:, :, 1:], mask_gt, torch.from_numpy(pd))
    assert [o.dtype for o in out] == [torch.int64, torch.float64, torch.float32, torch.bool]
    for o, key in zip(out, ("labels", "boxes", "scores", "fg")):
        assert_bit_equal(o.numpy(), g[name + "/" + key], key)
    assert atss.last_status.tolist() == [0, 0, 0] and atss.last_status.dtype == torch.int32
    # float32 labels (the reference's CPU fall-back hands such): widened, the boxes rounded back
    out32 = atss(torch.from_numpy(anchors), counts, gt[:, :, :1].float(), gt[:, :, 1:].float(), None, None)
    assert [o.dtype for o in out32] == [torch.int64, torch.float32, torch.float32, torch.bool]
    want = da.atss_host(anchors, counts, gt.float().double().numpy(), None, 9, nc, boxes_dtype=F32)
    for o, w in zip(out32, want):
        assert_bit_equal(o.numpy(), w)
    # M = 0: the early return
    e = atss(torch.from_numpy(anchors), counts, torch.zeros((2, 0, 1), dtype=torch.float64), torch.zeros((2, 0, 4), dtype=torch.float64), None, None)
    assert (e[0] == nc).all() and not e[1].any() and not e[2].any() and not e[3].any() and e[2].shape == (2, len(anchors), nc)


def test_the_python_routes_refuse_what_they_do_not_compute():
    da = _da()
    anchors, counts = da.anchor_boxes(64)                                # levels 64, 16, 4: the reference fails on the last
    gt = rows((0, 10.0, 10.0, 50.0, 50.0))
    with pytest.raises(ValueError, match="below topk"):
        da.atss_host(anchors, counts, gt, None, 9, 2)
    da.atss_host(anchors, counts, gt, None, 4, 2)
    a128, c128 = da.anchor_boxes(128)
    with pytest.raises(ValueError, match="add up"):
        da.atss_host(a128, [256, 64, 15], gt, None, 9, 2)
    with pytest.raises(ValueError, match="topk"):
        da.atss_host(a128, c128, gt, None, 33, 2)
    with pytest.raises(ValueError, match="topk"):
        da.atss_host(a128, c128, gt, None, 0, 2)
    with pytest.raises(ValueError, match="topk"):
        da.ATSSAssigner(topk=33)
    with pytest.raises(ValueError, match="levels"):
        da.atss_host(np.tile(a128[:32], (9, 1)), [32] * 9, gt, None, 9, 2)
    da.atss_host(np.tile(a128[:64], (8, 1)), [64] * 8, gt, None, 32, 2)       # 8 levels * 32 = 256 candidates: the most there can be
    atss = da.ATSSAssigner(9, num_classes=2)
    t = torch.from_numpy
    g = t(gt)
    with pytest.raises(ValueError, match=r"\.float\(\)"):
        atss(t(a128).double(), c128, g[:, :, :1], g[:, :, 1:], None, None)
    with pytest.raises(ValueError, match=r"\.float\(\)"):
        atss(t(a128), c128, g[:, :, :1], g[:, :, 1:], None, torch.zeros((1, 336, 4), dtype=torch.float64))
    with pytest.raises(ValueError, match="float64"):
        atss(t(a128), c128, g[:, :, :1], g[:, :, 1:].half(), None, None)
    with pytest.raises(ValueError, match="pd_bboxes must be"):
        da.atss_host(a128, c128, gt, np.zeros((1, 335, 4), F32), 9, 2)
    with pytest.raises(ValueError, match="CUDA"):
        da.atss_assign_batch(t(a128), c128, torch.zeros((1, 336, 4)), torch.zeros((0, 6)), (128, 128), 2)
    with pytest.raises(ValueError, match="CUDA"):
        da.atss_assign_batch(t(a128), c128, None, torch.zeros((0, 6)), (128, 128), 2)


# ---------------------------------------------------------------------------------------------- the registry and the refusals
def test_registry_header_and_library_agree():
    from event_representation_study_amd import _lib, build
    build.build()
    lib = _lib.load()
    full = open(os.path.join(ROOT, "include", "evrep.h")).read()
    text = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    for name, nargs in (("evrep_atss_workspace_bytes", 3), ("evrep_atss_assign", 18)):
        decl = re.search(r"\b%s\s*\(([^;]*)\);" % name, text)
        assert decl and len(decl.group(1).split(",")) == nargs == len(_lib.SYMBOLS[name][1]), name
        assert getattr(lib, name) is not None
    assert isinstance(_lib.SYMBOLS["evrep_atss_assign"], _lib.Status)
    for name in ("F32_BOXES", "F32_SCORES", "MAX_TOPK", "MAX_LEVELS", "MAX_CANDIDATES"):
        m = re.search(r"^#define\s+EVREP_ATSS_%s\s+(\d+)u?\s*$" % name, full, flags=re.M)
        assert m and int(m.group(1)) == getattr(_lib, "ATSS_" + name), name
    assert (_lib.ATSS_F32_BOXES, _lib.ATSS_F32_SCORES, _lib.ATSS_MAX_TOPK, _lib.ATSS_MAX_LEVELS, _lib.ATSS_MAX_CANDIDATES) == (1, 2, 32, 8, 256)
    assert lib.evrep_abi_version() == 3 == _lib.ABI_VERSION, "symbols only added"


# (B, M, A) -> bytes: three 32-bit words and one double per (image, anchor), each array rounded up to 256 bytes; M only decides
# whether the shape is refused; 0 for a shape evrep_atss_assign refuses.  Worked out by hand from the layout the header states.
_ATSS_WORKSPACE_SIZES = [
    ((0, 5, 189), 0), ((1, -1, 189), 0), ((1, 1025, 189), 0), ((1, 5, 0), 0), ((65536, 5, 189), 0), ((1, 5, (1 << 24) + 1), 0),
    ((1, 0, 189), 3 * 768 + 1536), ((1, 1024, 189), 3 * 768 + 1536), ((1, 1, 64), 3 * 256 + 512), ((1, 1, 65), 3 * 512 + 768),
    ((2, 33, 189), 3 * 1536 + 3072), ((32, 50, 8400), 3 * 1075200 + 2150400), ((65535, 1024, 1 << 24), 20 * 65535 * (1 << 24)),
]


def test_the_workspace_size_is_the_published_one():
    from event_representation_study_amd import _lib, build
    build.build()
    lib = _lib.load()
    assert _lib.SYMBOLS["evrep_atss_workspace_bytes"][0] is ctypes.c_size_t
    for args, size in _ATSS_WORKSPACE_SIZES:
        assert lib.evrep_atss_workspace_bytes(*args) == size, args


def test_the_entry_point_refuses_bad_arguments_before_any_launch():
    from event_representation_study_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p

    def levels(*n):
        return (ctypes.c_int32 * len(n))(*n)
    #       anchors    counts               n  gt         pd         B  M  A    nc topk flags labels    boxes      scores     fg         status
    good = [P(0x1000), levels(144, 36, 9), 3, P(0x2000), P(0x3000), 2, 3, 189, 2, 9, 0, P(0x4000), P(0x5000), P(0x6000), P(0x7000), P(0x8000),
            P(0x9000), None]

    def call(**change):
        args = list(good)
        for i, v in change.items():
            args[int(i[1:])] = v
        return lib.evrep_atss_assign(*args)
    for change in (dict(a5=0), dict(a5=65536), dict(a6=-1), dict(a6=1025), dict(a7=0), dict(a7=188), dict(a7=190), dict(a8=0), dict(a8=4097),
                   dict(a9=0), dict(a9=33), dict(a9=10), dict(a10=4), dict(a0=None), dict(a0=P(0x1002)), dict(a1=None), dict(a2=0), dict(a2=9),
                   dict(a2=2), dict(a1=levels(144, 37, 8)), dict(a1=levels(144, 36, 10)), dict(a1=levels(200, -20, 9)),
                   dict(a1=levels(2 ** 31 - 1, 2 ** 31 - 1, 191)), dict(a3=None), dict(a3=P(0x2004)), dict(a4=P(0x3002)),
                   dict(a11=P(0x4004)), dict(a12=P(0x5004)), dict(a13=P(0x6004)), dict(a10=1, a12=P(0x5002)), dict(a10=2, a13=P(0x6002)),
                   dict(a14=None), dict(a15=None), dict(a16=P(0x9080)), dict(a16=None),
                   dict(a1=levels(*[36] * 8), a2=8, a7=288, a9=33),
                   dict(a1=levels(*[21] * 9), a2=9, a7=189)):
        assert call(**change) == _lib.EVREP_EINVAL, change


# --------------------------------------------------------------------------------------------------------------- ComputeLoss
def _loss_inputs(seed, B, S, nc):
    import detector_loss_cases as lcases
    c = lcases.base(seed, S=S, B=B, nc=nc)
    rng = np.random.default_rng(seed)
    feats = [torch.zeros((B, 1, S // s, S // s)) for s in (8, 16, 32)]
    p = torch.from_numpy(rng.uniform(0.05, 0.95, c["p"].shape).astype(F32))
    return feats, p, torch.from_numpy(c["z"])


def test_compute_loss_warms_up_with_atss_on_cpu_tensors():
    from event_representation_study_amd import detector_loss as dl
    da = _da()
    B, S, nc = 2, 96, 2
    feats, p, z = _loss_inputs(71, B, S, nc)
    targets = torch.from_numpy(tal_cases.targets(72, [4, 3], nc, lo=0.2, hi=0.7))
    seen = {}

    def wrapped(anchors, n_list, gt_labels, gt_bboxes, mask_gt, pd):
        gt = torch.cat([gt_labels, gt_bboxes], dim=2).numpy()
        labels, boxes, scores, fg, _ = da.atss_host(anchors.numpy(), n_list, gt, pd.numpy(), 9, nc)
        seen["fg"] = int(fg.sum())
        return tuple(torch.from_numpy(v) for v in (labels, boxes, scores, fg))
    results = []
    for assigner in ("atss", da.ATSSAssigner(9, num_classes=nc), wrapped):
        crit = dl.ComputeLoss(num_classes=nc, ori_img_size=S, warmup_assigner=assigner)
        pp, zz = p.clone().requires_grad_(True), z.clone().requires_grad_(True)
        loss, items = crit((feats, pp, zz), targets, 0, 0, S, S)
        loss.backward()
        results.append((loss.detach(), items, pp.grad, zz.grad))
        assert crit.last_status.tolist() == [0, 0]
    assert seen["fg"] > 0 and results[0][0].item() > 0 and results[0][1][0].item() > 0
    for other in results[1:]:
        for a, b in zip(results[0], other):
            assert torch.equal(a, b)
    # the assigner changes at warmup_epoch
    crit = dl.ComputeLoss(num_classes=nc, ori_img_size=S, warmup_assigner="atss")
    late, _ = crit((feats, p, z), targets, 4, 0, S, S)
    assert late.item() != results[0][0].item()
    # what the default and the refusals say
    with pytest.raises(NotImplementedError, match="ATSSAssigner.*warmup_assigner='atss'"):
        dl.ComputeLoss(num_classes=nc)((feats, p, z), targets, 0, 0, S, S)
    with pytest.raises(ValueError, match="warmup_assigner"):
        dl.ComputeLoss(num_classes=nc, warmup_assigner="tal")
    with pytest.raises(ValueError, match="classes"):
        dl.ComputeLoss(num_classes=nc, warmup_assigner=da.ATSSAssigner(9, num_classes=nc + 1))
    with pytest.raises(ValueError, match="below topk"):                 # S = 64: the coarsest level holds 4 anchors
        f64, p64, z64 = _loss_inputs(73, B, 64, nc)
        dl.ComputeLoss(num_classes=nc, warmup_assigner="atss")((f64, p64, z64), targets, 0, 0, 64, 64)
