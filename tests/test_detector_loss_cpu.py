"""CPU: the host restatement of the loss terms (detector_loss.loss_host, values and gradients) against a torch float64
restatement of the reference's statements under autograd (tests/detector_loss_ref.py) within the DERIVED bound of
tests/detector_loss_cases.py, and against the golden recorded from the reference's own VarifocalLoss / BboxLoss / bbox_decode
within four times the MEASURED float32 rounding of the reference (stored in the fixture under measured/*); the registry against
the header, the refusals, the workspace size, and ComputeLoss on CPU tensors end to end.

Observed here (greatest error over bound, all cases): losses 0.03, grad_scores 0.02, grad_distri 0.001 of the derived bound;
against the golden 0.25 .. 1.0 of the measured deviation (the host route is the restatement but for the last places)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, assert_bit_equal, load_golden
import detector_loss_cases as cases

F32, F64 = np.float32, np.float64
MARGIN = 4.0                                                           # on the measured deviations of the golden


def _dl():
    from event_representation_study_amd import detector_loss
    return detector_loss


def golden_case(g, name):
    c = {k: g["%s/%s" % (name, k)] for k in ("p", "z", "anc", "stride", "labels", "tb", "ts", "fg")}
    nc, R, use_dfl = (int(v) for v in g[name + "/meta"])
    c.update(nc=nc, R=R, use_dfl=bool(use_dfl), weights=tuple(float(v) for v in g[name + "/weights"]))
    return c


def check_against_bounds(name, c, losses, gs, gz, ref_losses, ref_gs, ref_gz, bd, extra_rel=0.0):
    """|a - b| <= bound (+ extra_rel * |b| for gradients stored in float32), every figure printed first."""
    for k, key in enumerate(("cls", "iou", "dfl")):
        err = abs(float(losses[k]) - float(ref_losses[k]))
        print("%s loss_%s: error %.3g, bound %.3g" % (name, key, err, bd[key]))
        assert err <= bd[key], (name, key)
    for what, a, b, bound in (("grad_scores", gs, ref_gs, bd["gs"]), ("grad_distri", gz, ref_gz, bd["gz"])):
        err = np.abs(np.asarray(a, F64) - np.asarray(b, F64))
        # one float32 rounding: relative in the normal range, half the least subnormal (2^-150) below it
        lim = bound + extra_rel * np.abs(np.asarray(b, F64)) + (2.0 ** -150 if extra_rel else 0.0)
        print("%s %s: greatest error %.3g, greatest error / bound %.3g" % (name, what, err.max(), (err / np.maximum(lim, 1e-300)).max()))
        assert (err <= lim).all(), (name, what)


def check_against_golden(name, c, g, losses, gs, gz, boxes=None):
    """Within MARGIN times the reference's own measured float32 rounding: losses relatively, gradients and boxes absolutely, the
    grad_scores elements whose p is exactly 0 or 1 relatively."""
    m = {k: float(g["measured/" + k]) for k in ("loss_cls", "loss_iou", "loss_dfl", "grad_scores", "grad_scores_saturated", "grad_distri",
                                                "pred_bboxes")}
    for k, key in enumerate(("loss_cls", "loss_iou", "loss_dfl")):
        want = float(g["%s/%s" % (name, key)])
        err = 0.0 if losses[k] == want else abs(float(losses[k]) - want) / abs(want)
        print("%s %s: relative error %.3g, allowed %.3g" % (name, key, err, MARGIN * m[key]))
        assert err <= MARGIN * m[key], (name, key)
    sat = (c["p"] == 0) | (c["p"] == 1)
    want = g[name + "/grad_scores"].astype(F64)
    err = np.abs(np.asarray(gs, F64) - want)
    print("%s grad_scores: %.3g, allowed %.3g" % (name, err[~sat].max(), MARGIN * m["grad_scores"]))
    assert (err[~sat] <= MARGIN * m["grad_scores"]).all(), name
    if sat.any():
        rel = np.where(err[sat] == 0, 0.0, err[sat] / np.maximum(np.abs(want[sat]), 1e-300))
        print("%s grad_scores at p in {0, 1}: relative %.3g, allowed %.3g" % (name, rel.max(), MARGIN * m["grad_scores_saturated"]))
        assert (rel <= MARGIN * m["grad_scores_saturated"]).all(), name
    err = np.abs(np.asarray(gz, F64) - g[name + "/grad_distri"].astype(F64)).max()
    print("%s grad_distri: %.3g, allowed %.3g" % (name, err, MARGIN * m["grad_distri"]))
    assert err <= MARGIN * m["grad_distri"], name
    if boxes is not None:
        err = np.abs(np.asarray(boxes, F64) - g[name + "/pred_bboxes"].astype(F64)).max()
        print("%s pred_bboxes: %.3g, allowed %.3g" % (name, err, MARGIN * m["pred_bboxes"]))
        assert err <= MARGIN * m["pred_bboxes"], name


# ---------------------------------------------------------------------------------------------- against the float64 restatement
@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_loss_host_equals_the_restatement_within_the_derived_bound(name):
    c = cases.CASES[name]()
    d = {}
    losses, gs, gz, status = cases.host(c, d)
    cases.check_decided(name, c, d)
    r = cases.restated(c)
    bd = cases.bounds(c, losses, d)
    check_against_bounds(name, c, losses, d["gs"], d["gz"], (r["loss_cls"], r["loss_iou"], r["loss_dfl"]), r["grad_scores"].numpy(),
                         r["grad_distri"].numpy(), bd)
    assert abs(losses[3] - r["tss"]) <= 286 * cases.U * r["tss"] and losses[4] == c["fg"].sum()
    assert_bit_equal(gs, d["gs"].astype(F32))
    assert_bit_equal(gz, d["gz"].astype(F32))
    box = _dl().decode_host(c["z"], c["anc"], c["stride"], c["R"], c["use_dfl"])
    K = c["R"] + 1 if c["use_dfl"] else 1
    assert (np.abs(box - r["pred_bboxes"].numpy()) <= 12 * K * cases.U * np.abs(np.concatenate([box, d["box"]], -1)).max(-1, keepdims=True)).all()
    assert status.tolist() == ([1, 0, 1] if name == "bad_label" else [0] * len(status))


def test_the_cases_hold_their_edges():
    dl = _dl()
    d = {}
    c = cases.no_positives()
    losses, gs, gz, _ = cases.host(c, d)
    assert losses[1] == 0 and losses[2] == 0 and losses[3] == 0 and losses[4] == 0 and not gz.any() and gs.any()
    below, above = cases.host(cases.tss_below_one())[0], cases.host(cases.tss_just_above_one())[0]
    assert below[3] == 0.7 and 1 < above[3] < 1 + 1e-6
    c = cases.saturated()
    losses, gs, gz, _ = cases.host(c, d)
    sat = (c["p"] == 0) | (c["p"] == 1)
    assert sat.sum() == 18 and np.isfinite(gs).all() and np.abs(gs[sat]).max() > 1e10
    lab = c["fg"][..., None] & (c["labels"][..., None] == np.arange(2))
    assert (sat & lab & (c["ts"] > 0) & (c["ts"] < 1)).sum() == 4 and (sat & ~lab & (c["ts"] > 0) & (c["ts"] < 1)).sum() >= 4
    c = cases.disjoint()
    cases.host(c, d)
    iw, ih = d["clamps"]
    assert (iw < 0).sum() >= 2 and (ih < 0).sum() >= 2 and ((iw < 0) & (ih < 0)).sum() >= 1
    c = cases.clipped()
    cases.host(c, d)
    dist = d["dist"]
    assert (dist < 0).any() and (dist > 16 - 0.01).any() and ((dist == np.round(dist)) & (dist > 0) & (dist < 15)).sum() >= 3
    c = cases.big_logits()
    assert np.abs(c["z"]).max() == 80 and np.isfinite(cases.host(c)[0]).all()
    assert dl.BCE_EPS == F64(F32(1e-12)) != 1e-12


# ------------------------------------------------------------------------------------------------------ against the reference
def test_the_golden_holds_the_cases_the_builders_name():
    g = load_golden("detector_loss")
    assert sorted({k.split("/")[0] for k in g} - {"measured"}) == sorted(cases.GOLDEN)
    for name in cases.GOLDEN:
        c = cases.CASES[name]()
        for k in ("p", "z", "anc", "stride", "labels", "tb", "ts", "fg"):
            assert_bit_equal(g["%s/%s" % (name, k)], c[k], name + " " + k)
    assert g["f32_targets/ts"].dtype == F32 and g["plain/ts"].dtype == F64 and g["plain/grad_scores"].dtype == F32
    for k in ("loss_cls", "loss_iou", "loss_dfl", "grad_scores", "grad_scores_saturated", "grad_distri", "pred_bboxes"):
        assert 0 < float(g["measured/" + k]) < 1e-5, k


@pytest.mark.parametrize("name", cases.GOLDEN)
def test_loss_host_equals_the_reference_within_its_measured_rounding(name):
    g = load_golden("detector_loss")
    c = golden_case(g, name)
    losses, gs, gz, status = cases.host(c)
    box = _dl().decode_host(c["z"], c["anc"], c["stride"], c["R"], c["use_dfl"])
    check_against_golden(name, c, g, losses, gs, gz, box)
    assert not status.any()


# ---------------------------------------------------------------------------------------------- the registry and the refusals
def test_registry_header_and_library_agree():
    from event_representation_study_amd import _lib, build
    build.build()
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "evrep.h")).read(), flags=re.S)
    for name, nargs in (("evrep_detloss_decode", 10), ("evrep_detloss_workspace_bytes", 3), ("evrep_detloss", 22)):
        decl = re.search(r"\b%s\s*\(([^;]*)\);" % name, text)
        assert decl and len(decl.group(1).split(",")) == nargs == len(_lib.SYMBOLS[name][1]), name
        assert getattr(lib, name) is not None
    assert isinstance(_lib.SYMBOLS["evrep_detloss"], _lib.Status) and isinstance(_lib.SYMBOLS["evrep_detloss_decode"], _lib.Status)
    assert _lib.SYMBOLS["evrep_detloss_workspace_bytes"][0] is ctypes.c_size_t
    assert not [n for n in _lib.SYMBOLS if "detloss" in n and n.endswith("_scratch_bytes")]
    full = open(os.path.join(ROOT, "include", "evrep.h")).read()
    for name in ("USE_DFL", "NO_GRAD", "F32_TARGETS", "MAX_REG", "ST_BAD_LABEL"):
        m = re.search(r"^#define\s+EVREP_DETLOSS_%s\s+(\d+)u?\s*$" % name, full, flags=re.M)
        assert m and int(m.group(1)) == getattr(_lib, "DETLOSS_" + name), name
    assert lib.evrep_abi_version() == 3 and len(build.SOURCES) == 15
    csrc = os.path.join(ROOT, "event_representation_study_amd", "csrc")
    assert '#include "evrep_detloss.hip"' in open(os.path.join(csrc, "evrep_capi_detin.hip")).read()


# (B, A, nc) -> bytes: B * A doubles; min(ceil(B * A / 256), 256) doubles; B * min(ceil(A * nc / 256), ceil(2048 / B)) doubles;
# three times B * ceil(A / 256) doubles; each array rounded up to 256 bytes; 0 for a refused shape.  One tuple per edge.
_WORKSPACE_SIZES = [
    ((0, 84, 2), 0), ((65536, 84, 2), 0), ((1, 0, 2), 0), ((1, (1 << 24) + 1, 1), 0), ((1, 84, 0), 0), ((1, 84, 4097), 0),
    ((1, 1 << 24, 4096), 0),
    ((1, 84, 2), 768 + 256 + 256 + 3 * 256),
    ((3, 525, 80), 12800 + 256 + 4096 + 3 * 256),
    ((32, 8400, 80), 2150400 + 2048 + 16384 + 3 * 8448),
    ((32, 8400, 1), 2150400 + 2048 + 8448 + 3 * 8448),
    ((1, 65536, 1), 524288 + 2048 + 2048 + 3 * 2048),
    ((1, 65537, 1), 524544 + 2048 + 2304 + 3 * 2304),
    ((2049, 1, 1), 16640 + 256 + 16640 + 3 * 16640),
]


def test_the_workspace_size_is_the_published_one():
    """The expectations are the layout stated in include/evrep.h worked out by hand, not what the library returned."""
    from event_representation_study_amd import _lib, build
    build.build()
    lib = _lib.load()
    for args, size in _WORKSPACE_SIZES:
        assert lib.evrep_detloss_workspace_bytes(*args) == size, args


def test_the_entry_points_refuse_bad_arguments_before_any_launch():
    from event_representation_study_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    DFL, NOGRAD, F32T = _lib.DETLOSS_USE_DFL, _lib.DETLOSS_NO_GRAD, _lib.DETLOSS_F32_TARGETS
    good = [P(0x1000), P(0x2000), P(0x3000), P(0x4000), P(0x5000), P(0x6000), P(0x7000), P(0x8000), 3, 84, 2, 16, 1.0, 2.5, 0.5, DFL,
            P(0x9000), P(0xA000), P(0xB000), P(0xC000), P(0xD000), None]

    def call(**change):
        args = list(good)
        for i, v in change.items():
            args[int(i[1:])] = v
        return lib.evrep_detloss(*args)
    for change in (dict(a8=0), dict(a8=65536), dict(a9=0), dict(a9=(1 << 24) + 1), dict(a10=0), dict(a10=4097), dict(a9=1 << 24, a10=4096),
                   dict(a11=-1), dict(a11=33), dict(a11=0), dict(a15=8), dict(a15=DFL | 16), dict(a0=None), dict(a1=None), dict(a1=P(0x2002)),
                   dict(a2=None), dict(a3=P(0x4001)), dict(a4=None), dict(a4=P(0x5004)), dict(a5=None), dict(a5=P(0x6004)),
                   dict(a6=P(0x7004)), dict(a6=P(0x7002), a15=DFL | F32T), dict(a7=None), dict(a16=None), dict(a16=P(0x9004)),
                   dict(a17=None), dict(a18=None), dict(a18=P(0xB002)), dict(a17=P(0xA002), a15=DFL | NOGRAD), dict(a19=None),
                   dict(a19=P(0xC002)), dict(a20=None), dict(a20=P(0xD080))):
        assert call(**change) == _lib.EVREP_EINVAL, change
    dec = [P(0x1000), P(0x2000), P(0x3000), 3, 84, 16, DFL, P(0x4000), P(0x5000), None]
    for i, v in ((0, None), (0, P(0x1002)), (1, None), (2, None), (3, 0), (3, 65536), (4, 0), (4, (1 << 24) + 1), (5, -1), (5, 33), (5, 0),
                 (6, 2), (7, None), (8, None), (8, P(0x5001))):
        args = list(dec)
        args[i] = v
        assert lib.evrep_detloss_decode(*args) == _lib.EVREP_EINVAL, (i, v)


def test_the_python_routes_refuse_what_they_do_not_compute():
    dl = _dl()
    c = cases.plain_small()
    t = {k: torch.from_numpy(np.asarray(c[k])) for k in ("p", "z", "anc", "stride", "labels", "tb", "ts", "fg")}
    args = (t["anc"], t["stride"], t["labels"], t["tb"], t["ts"], t["fg"], 1)
    with pytest.raises(ValueError, match=r"\.float\(\)"):
        dl.loss_batch(t["p"].double(), t["z"], *args)
    with pytest.raises(ValueError, match=r"\.float\(\)"):
        dl.loss_batch(t["p"], t["z"].half(), *args)
    with pytest.raises(ValueError, match=r"\.float\(\)"):
        dl.decode_boxes(t["z"].double(), t["anc"], t["stride"])
    with pytest.raises(ValueError, match="num_classes"):
        dl.loss_batch(t["p"], t["z"], *args[:-1], 3)
    with pytest.raises(ValueError, match="reg_max"):
        dl.loss_batch(t["p"], t["z"], *args, reg_max=0)
    with pytest.raises(ValueError, match="reg_max"):
        dl.ComputeLoss(num_classes=1, reg_max=33)
    for iou_type in ("siou", "ciou", "diou"):
        with pytest.raises(NotImplementedError, match="giou"):
            dl.ComputeLoss(num_classes=1, iou_type=iou_type)
    assert dl.ComputeLoss(num_classes=1, use_dfl=False, reg_max=0).warmup_epoch == 4


# --------------------------------------------------------------------------------------------------------- the public routes
def test_loss_batch_on_cpu_tensors_carries_the_host_gradients():
    dl = _dl()
    c = cases.plain_nc2()
    want, gs, gz, _ = cases.host(c)
    t = {k: torch.from_numpy(np.asarray(c[k])) for k in ("p", "z", "anc", "stride", "labels", "tb", "ts", "fg")}
    p, z = t["p"].clone().requires_grad_(True), t["z"].clone().requires_grad_(True)
    loss, items = dl.loss_batch(p, z, t["anc"], t["stride"], t["labels"], t["tb"], t["ts"], t["fg"], 2)
    assert loss.dtype == torch.float64 and loss.dim() == 0 and loss.requires_grad and not items.requires_grad
    assert loss.item() == (want[0] * 1.0 + want[1] * 2.5) + want[2] * 0.5
    assert items.tolist() == [want[1] * 2.5, want[2] * 0.5, want[0] * 1.0]
    (loss * 3.0).backward()
    assert_bit_equal(p.grad.numpy(), gs * F32(3))
    assert_bit_equal(z.grad.numpy(), gz * F32(3))
    with torch.no_grad():
        quiet, items2 = dl.loss_batch(p, z, t["anc"], t["stride"], t["labels"], t["tb"], t["ts"], t["fg"], 2)
    assert not quiet.requires_grad and quiet.item() == loss.item() and torch.equal(items, items2)


def _head(seed, B, S, nc, R=16):
    rng = np.random.default_rng(seed)
    c = cases.base(seed, S=S, B=B, nc=nc, R=R)
    feats = [torch.zeros((B, 1, S // s, S // s)) for s in (8, 16, 32)]
    p = torch.from_numpy((rng.uniform(0.05, 0.95, c["p"].shape)).astype(F32))
    return feats, p, torch.from_numpy(c["z"]), c


def test_compute_loss_on_cpu_tensors_end_to_end():
    from event_representation_study_amd import detector_assign as da
    import detector_assign_cases as acases
    dl = _dl()
    B, S, nc = 3, 64, 2
    feats, p, z, c = _head(31, B, S, nc)
    targets = torch.from_numpy(acases.targets(32, [3, 0, 4], nc, lo=0.2, hi=0.7))
    crit = dl.ComputeLoss(num_classes=nc, ori_img_size=S)
    p.requires_grad_(True)
    z.requires_grad_(True)
    loss, items = crit((feats, p, z), targets, 5, 0, S, S)
    anc, stride = da.anchor_points(S)
    assert_bit_equal(crit.anchors(feats, "cpu")[1].numpy(), anc)
    box = dl.decode_host(z.detach().numpy(), anc, stride, 16, True)
    px = (box * stride.reshape(1, -1, 1).astype(F64)).astype(F32)
    gt = da.preprocess_host(targets.numpy(), B, S, S)[0]
    labels, tb, ts, fg, st = da.tal_host(p.detach().numpy(), px, anc, gt)
    assert fg.any() and not fg[1].any()
    want, gs, gz, _ = dl.loss_host(p.detach().numpy(), z.detach().numpy(), anc, stride, labels, tb, ts, fg)
    assert loss.item() == (want[0] * 1.0 + want[1] * 2.5) + want[2] * 0.5 and items.tolist() == [want[1] * 2.5, want[2] * 0.5, want[0]]
    loss.backward()
    assert_bit_equal(p.grad.numpy(), gs)
    assert_bit_equal(z.grad.numpy(), gz)
    assert crit.last_status.tolist() == [0, 0, 0]
    # the restatement on the same targets
    r = cases.restated(dict(p=p.detach().numpy(), z=z.detach().numpy(), anc=anc, stride=stride.reshape(-1), labels=labels, tb=tb, ts=ts,
                            fg=fg, nc=nc, R=16, use_dfl=True, weights=cases.WEIGHTS))
    assert abs(loss.item() - r["loss"]) <= 1e-12 * abs(r["loss"])
    # empty targets: M = 0, the assigner's early return
    empty, items0 = crit((feats, p, z), torch.zeros((0, 6)), 5, 0, S, S)
    assert items0[0].item() == 0 and items0[1].item() == 0 and items0[2].item() > 0 and empty.item() == items0[2].item()
    p.grad = z.grad = None
    empty.backward()
    assert not z.grad.any() and p.grad.any()


def test_warm_up_epochs_need_an_assigner():
    from event_representation_study_amd import detector_assign as da
    import detector_assign_cases as acases
    dl = _dl()
    B, S, nc = 2, 64, 2
    feats, p, z, c = _head(33, B, S, nc)
    targets = torch.from_numpy(acases.targets(34, [3, 2], nc, lo=0.2, hi=0.7))
    with pytest.raises(NotImplementedError, match="ATSSAssigner"):
        dl.ComputeLoss(num_classes=nc)((feats, p, z), targets, 0, 0, S, S)
    formal, _ = dl.ComputeLoss(num_classes=nc)((feats, p, z), targets, 4, 0, S, S)
    seen = {}

    def warmup(anchors, n_anchors_list, gt_labels, gt_bboxes, mask_gt, pred_bboxes):
        seen.update(anchors=anchors, n=n_anchors_list, mask=mask_gt)
        anc = (anchors[:, :2] + anchors[:, 2:]) / 2
        return da.TaskAlignedAssigner(13, nc)(p.detach(), pred_bboxes, anc, gt_labels, gt_bboxes, mask_gt)
    warm, _ = dl.ComputeLoss(num_classes=nc, warmup_assigner=warmup)((feats, p, z), targets, 0, 0, S, S)
    assert warm.item() == formal.item()
    assert seen["n"] == [64, 16, 4] and tuple(seen["anchors"].shape) == (84, 4) and seen["anchors"][0].tolist() == [-16, -16, 24, 24]
    assert seen["mask"].dtype == torch.float32 and tuple(seen["mask"].shape) == (2, 3, 1)
    assert dl.ComputeLoss(num_classes=nc, warmup_epoch=0)((feats, p, z), targets, 0, 0, S, S)[0].item() == formal.item()
