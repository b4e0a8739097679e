"""CPU: the host restatements of the distillation losses (detector_distill.distill_host and cw_host, values and gradients)
against a torch float64 restatement of the reference's statements under autograd (tests/detector_distill_ref.py) within the
DERIVED bounds of tests/detector_distill_cases.py, and against the golden recorded from the reference's own VarifocalLoss /
BboxLoss / distill_loss_cls / distill_loss_cw within four times the MEASURED float32 rounding of the reference (stored in the
fixture under measured/*); the edges the cases pin, the registry against the header, the workspace sizes, the refusals, and
distill_batch, distill_cw and ComputeLossDistill on CPU tensors end to end."""
import ctypes
import hashlib
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, assert_bit_equal, load_golden
import detector_distill_cases as cases
import detector_loss_cases as lcases

F32, F64 = np.float32, np.float64
MARGIN = 4.0                                                           # on the measured deviations of the golden
LOSSES = ("loss_cls", "loss_iou", "loss_dfl", "d_loss_cls", "d_loss_dfl")
BOUND_KEYS = ("cls", "iou", "dfl", "dcls", "ddfl")
ABS_KEYS = ("cls_abs", "iou_abs", "dfl_abs", "dcls_abs", "ddfl_abs")


def _dd():
    from event_representation_study_amd import detector_distill
    return detector_distill


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


def check_against_bounds(name, losses, gs, gz, ref_losses, ref_gs, ref_gz, bd, extra_rel=0.0):
    """|a - b| <= bound (+ extra_rel * |b| for gradients stored in float32), every figure printed first."""
    for k, key in enumerate(BOUND_KEYS):
        err = abs(float(losses[k]) - float(ref_losses[k]))
        print("%s %s: error %.3g, bound %.3g" % (name, LOSSES[k], err, bd[key]))
        assert err <= bd[key], (name, key)
    for what, a, b, bound in (("grad_scores", gs, ref_gs, bd["gs"]), ("grad_distri", gz, ref_gz, bd["gz"])):
        err = np.abs(np.asarray(a, F64) - np.asarray(b, F64))
        lim = bound + extra_rel * np.abs(np.asarray(b, F64)) + (2.0 ** -150 if extra_rel else 0.0)
        print("%s %s: greatest error %.3g, greatest error / bound %.3g" % (name, what, err.max(), (err / np.maximum(lim, 1e-300)).max()))
        assert (err <= lim).all(), (name, what)


def check_against_golden(name, g, d, losses, gs, gz):
    """Within MARGIN times the reference's own measured float32 rounding: the losses relative to the sums of the absolute values
    of their terms (``d``: distill_host's details on the case), the gradients absolutely.  Returns the five allowances."""
    allowances = []
    for k, key in enumerate(LOSSES):
        want, allowed = float(g["%s/%s" % (name, key)]), MARGIN * float(g["measured/" + key]) * float(d[ABS_KEYS[k]])
        err = abs(float(losses[k]) - want)
        print("%s %s: error %.3g, allowed %.3g" % (name, key, err, allowed))
        assert err <= allowed, (name, key)
        allowances.append(allowed)
    for key, got in (("grad_scores", gs), ("grad_distri", gz)):
        err = np.abs(np.asarray(got, F64) - g["%s/%s" % (name, key)].astype(F64)).max()
        print("%s %s: %.3g, allowed %.3g" % (name, key, err, MARGIN * float(g["measured/" + key])))
        assert err <= MARGIN * float(g["measured/" + key]), (name, key)
    return allowances


def check_cw_against_bounds(name, c, out, grads, ref, d, extra_rel=0.0):
    levels, gb, total = cases.cw_bounds(c, d)
    err = abs(float(out[0]) - ref["loss"])
    print("%s cw loss: error %.3g, bound %.3g" % (name, err, total))
    assert err <= total, name
    for l in range(3):
        err = abs(float(out[1 + l]) - ref["levels"][l])
        assert err <= levels[l], (name, l)
        want = np.asarray(ref["grads"][l], F64)
        e = np.abs(np.asarray(grads[l], F64) - want)
        lim = gb[l] + extra_rel * np.abs(want) + (2.0 ** -150 if extra_rel else 0.0)
        print("%s cw grad %d: greatest error / bound %.3g" % (name, l, (e / np.maximum(lim, 1e-300)).max()))
        assert (e <= lim).all(), (name, l)


def check_cw_against_golden(name, g, d, out, grads):
    pre = "cw_%s/" % name
    allowed = MARGIN * float(g["measured/cw_loss"]) * float(sum(d["abs"]))
    err = abs(float(out[0]) - float(g[pre + "loss"]))
    print("%s cw loss: error %.3g, allowed %.3g" % (name, err, allowed))
    assert err <= allowed, name
    for l in range(3):
        err = np.abs(np.asarray(grads[l], F64) - g[pre + "grad%d" % l].astype(F64)).max()
        assert err <= MARGIN * float(g["measured/cw_grad"]), (name, l, err)


def tensors(c):
    return {k: torch.from_numpy(np.asarray(c[k])) for k in cases.KEYS}


# ---------------------------------------------------------------------------------------------- against the float64 restatement
@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_distill_host_equals_the_restatement_within_the_derived_bound(name):
    c = cases.CASES[name]()
    d = {}
    losses, gs, gz, status = cases.host(c, d)
    lcases.check_decided(name, c, d)
    r = cases.restated(c)
    bd = cases.bounds(c, losses, d)
    check_against_bounds(name, losses, d["gs"], d["gz"], [r[k] for k in LOSSES], r["grad_scores"].numpy(), r["grad_distri"].numpy(), bd)
    assert abs(losses[5] - r["tss"]) <= 286 * cases.U * r["tss"] and losses[6] == c["fg"].sum() and not status.any()
    assert_bit_equal(gs, d["gs"].astype(F32))
    assert_bit_equal(gz, d["gz"].astype(F32))
    # rule 8's sum: the five bounds with its weights, and at most 16 roundings on the absolute values of the weighted terms
    loss, items = cases.total(c, losses)
    (kc, kd), (wc, wi, wd) = cases.k_of(c), c["weights"]
    terms = (wc * losses[0], wc * kc * losses[3], wi * losses[1], wd * losses[2], wd * kd * losses[4])
    allowed = wc * (bd["cls"] + kc * bd["dcls"]) + wi * bd["iou"] + wd * (bd["dfl"] + kd * bd["ddfl"]) + 16 * cases.U * sum(abs(float(v)) for v in terms)
    assert abs(loss - r["loss"]) <= allowed
    assert not gz[~c["fg"]].any()


@pytest.mark.parametrize("name", sorted(cases.CW_CASES))
def test_cw_host_equals_the_restatement_within_the_derived_bound(name):
    c = cases.CW_CASES[name]()
    d = {}
    out, grads = cases.cw_host(c, d)
    assert len(grads) == 3 and all(g.dtype == F32 and g.shape == s.shape for g, s in zip(grads, c["s"]))
    check_cw_against_bounds(name, c, out, d["g"], cases.cw_restated(c), d)
    assert out[0] == (out[1] + out[2]) + out[3]


def test_the_cases_hold_their_edges():
    from event_representation_study_amd import detector_loss as dl
    dd = _dd()
    shapes = {(c["p"].shape[1], c["p"].shape[0], c["nc"]) for c in (f() for f in cases.CASES.values())}
    assert {s[0] for s in shapes} == {84, 525} and {s[1] for s in shapes} == {1, 3} and {s[2] for s in shapes} == {1, 2, 80}
    assert cases.plain()["T"] == 20 and cases.t_one()["T"] == 1 and cases.t_three()["T"] == 3
    # nc = 1: the class distillation and its part of every gradient are exactly 0
    c = cases.nc_one()
    d = {}
    losses, gs, gz, _ = cases.host(c, d)
    base = {}
    dl.loss_host(c["p"], c["z"], c["anc"], c["stride"], c["labels"], c["tb"], c["ts"], c["fg"], c["R"], c["use_dfl"],
                 dict(zip(("class", "iou", "dfl"), c["weights"])), details=base, norm_floor=0.0)
    assert losses[3] == 0 and np.array_equal(d["gs"], base["gs"]) and losses[4] > 0
    # the teacher is the student: both distillation losses exactly 0
    losses = cases.host(cases.teacher_is_student())[0]
    assert losses[3] == 0 and losses[4] == 0 and losses[6] == 6
    # no positives: nothing from the boxes, the class distillation still acts on every row
    c = cases.no_positives()
    losses, gs, gz, _ = cases.host(c, d)
    assert losses[4] == 0 and losses[1] == 0 and losses[2] == 0 and losses[6] == 0 and losses[7] == 0 and losses[3] > 0
    assert not gz.any() and (gs != 0).all()
    assert cases.host(cases.one_positive())[0][6] == 1
    # tss = 0.7: normalised here, not in loss.py's rule -- the two disagree on loss_iou by that factor
    c = cases.tss_below_one()
    here = cases.host(c)[0]
    there = lcases.host(c)[0]
    assert here[5] == there[3] == 0.7 and there[1] > 0
    assert here[1] == pytest.approx(there[1] / 0.7, rel=1e-15) and abs(here[1] - there[1]) > 0.2 * there[1]
    assert here[0] == pytest.approx(there[0] / 0.7, rel=1e-15)
    # foreground anchors without scores: W = 0, tss = 0
    c = cases.tss_zero_with_fg()
    losses, gs, gz, _ = cases.host(c, d)
    assert losses[6] == 4 and losses[7] == 0 and losses[5] == 0 and losses[4] == 0 and not gz.any()
    # background rows with scores: W / norm != 1
    losses = cases.host(cases.w_not_tss())[0]
    assert 0 < losses[7] < 0.9 * losses[5] and losses[4] > 0
    assert cases.host(cases.no_dfl())[0][4] == 0
    c = cases.big_logits()
    assert np.abs(c["z"]).max() == 80 and np.abs(c["tz"]).max() == 80 and np.isfinite(cases.host(c)[0]).all()
    assert cases.r8()["z"].shape[-1] == 36 and cases.f32_targets()["ts"].dtype == F32
    # the decay: 1 at epoch 0, 0.505 half way, 0.01 at the end
    assert dd.decay(0, 10) == 1.0 and dd.decay(5, 10) == pytest.approx(0.505, rel=1e-15) and dd.decay(10, 10) == pytest.approx(0.01, rel=1e-13)
    assert [cases.CASES[n]()["epoch"] for n in ("decay_start", "decay_mid", "decay_end")] == [0, 5, 10]
    # channel-wise: one value per row is exactly 0, in the loss and in every gradient
    out, grads = cases.cw_host(cases.CW_CASES["one_value"]())
    assert not out.any() and not any(g.any() for g in grads)
    hw = sorted({int(np.prod(s.shape[2:])) for n in cases.CW_CASES for s in cases.CW_CASES[n]()["s"][:3]})
    assert {1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 6400} <= set(hw)
    four = cases.CW_CASES["four_levels"]()
    assert len(four["s"]) == 4 and np.array_equal(cases.cw_host(four)[0], cases.cw_host(dict(four, s=four["s"][:3], t=four["t"][:3]))[0])


# ------------------------------------------------------------------------------------------------------ against the reference
def test_the_golden_holds_the_cases_the_builders_name():
    g = load_golden("detector_distill")
    names = {k.split("/")[0] for k in g} - {"measured"}
    assert names == set(cases.GOLDEN) | {"cw_" + n for n in cases.CW_GOLDEN}
    for name in cases.GOLDEN:
        c = cases.CASES[name]()
        assert_bit_equal(g[name + "/inputs_sha256"], digest([c[k] for k in cases.KEYS]), name)
        assert g[name + "/grad_scores"].dtype == F32 and g[name + "/loss_items"].shape == (4,) and g[name + "/loss_items"][3] == 0
    for name in cases.CW_GOLDEN:
        c = cases.CW_CASES[name]()
        assert_bit_equal(g["cw_%s/inputs_sha256" % name], digest(c["s"] + c["t"]), name)
    for k in LOSSES + ("grad_scores", "grad_distri", "cw_loss", "cw_grad"):
        assert 0 < float(g["measured/" + k]) < 1e-4, k
    size = os.path.getsize(os.path.join(ROOT, "tests", "golden", "detector_distill.npz"))
    assert size <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "detector_loss.npz"))


@pytest.mark.parametrize("name", cases.GOLDEN)
def test_distill_host_equals_the_reference_within_its_measured_rounding(name):
    g = load_golden("detector_distill")
    c = cases.CASES[name]()
    d = {}
    losses, gs, gz, _ = cases.host(c, d)
    a = check_against_golden(name, g, d, losses, gs, gz)
    # the reference's weighted sum: the five allowances with the weights of rule 8, and its own float32 operations on the
    # way -- two products and an addition per term and three additions, at most 8 roundings of 2^-24 on the sum of the
    # absolute values of the weighted terms
    loss, items = cases.total(c, losses)
    (kc, kd), (wc, wi, wd) = cases.k_of(c), c["weights"]
    terms = (wc * losses[0], wc * kc * losses[3], wi * losses[1], wd * losses[2], wd * kd * losses[4])
    allowed = wc * (a[0] + kc * a[3]) + wi * a[1] + wd * (a[2] + kd * a[4]) + 8 * 2.0 ** -24 * sum(abs(float(v)) for v in terms)
    assert abs(loss - float(g[name + "/loss"])) <= allowed
    assert np.abs(np.array(items) - g[name + "/loss_items"][:3]).max() <= allowed


@pytest.mark.parametrize("name", cases.CW_GOLDEN)
def test_cw_host_equals_the_reference_within_its_measured_rounding(name):
    c = cases.CW_CASES[name]()
    d = {}
    out, grads = cases.cw_host(c, d)
    check_cw_against_golden(name, load_golden("detector_distill"), d, out, grads)


# ---------------------------------------------------------------------------------------------- the registry and the refusals
def test_registry_header_and_library_agree():
    from event_representation_study_amd import _lib, build
    build.build()
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "evrep.h")).read(), flags=re.S)
    for name, nargs in (("evrep_detloss_distill_workspace_bytes", 3), ("evrep_detloss_distill", 27), ("evrep_detloss_cwd_workspace_bytes", 2),
                        ("evrep_detloss_cwd", 7)):
        decl = re.search(r"\b%s\s*\(([^;]*)\);" % name, text)
        assert decl and len(decl.group(1).split(",")) == nargs == len(_lib.SYMBOLS[name][1]), name
        assert getattr(lib, name) is not None
    assert isinstance(_lib.SYMBOLS["evrep_detloss_distill"], _lib.Status) and isinstance(_lib.SYMBOLS["evrep_detloss_cwd"], _lib.Status)
    assert _lib.SYMBOLS["evrep_detloss_distill_workspace_bytes"][0] is ctypes.c_size_t
    assert not [n for n in _lib.SYMBOLS if "distill" in n and n.endswith("_scratch_bytes")]
    full = open(os.path.join(ROOT, "include", "evrep.h")).read()
    for name in ("CWD_MAX_LEVELS", "CWD_STAGE", "DISTILL_MAX_CLASSES"):
        m = re.search(r"^#define\s+EVREP_%s\s+(\d+)u?\s*$" % name, full, flags=re.M)
        assert m and int(m.group(1)) == getattr(_lib, name), name
    assert ctypes.sizeof(_lib.CwdLevel) == 40 and lib.evrep_abi_version() == _lib.ABI_VERSION and len(build.SOURCES) == 15
    csrc = os.path.join(ROOT, "event_representation_study_amd", "csrc")
    assert '#include "evrep_detdistill.hip"' in open(os.path.join(csrc, "evrep_capi_detin.hip")).read()


# (B, A, nc) -> bytes: B * A doubles; three times min(ceil(B * A / 256), 256) doubles; two times B * min(ceil(A / rt), ceil(2048 /
# B)) doubles with rt = min(256, 2048 / nc); four times B * ceil(A / 256) doubles; each rounded up to 256 bytes
_WORKSPACE_SIZES = [
    ((0, 84, 2), 0), ((65536, 84, 2), 0), ((1, 0, 2), 0), ((1, (1 << 24) + 1, 1), 0), ((1, 84, 0), 0), ((1, 84, 2049), 0),
    ((1, 84, 2), 768 + 3 * 256 + 2 * 256 + 4 * 256),
    ((3, 525, 80), 12800 + 3 * 256 + 2 * 512 + 4 * 256),               # rt = 25: 21 tiles per image
    ((32, 8400, 80), 2150400 + 3 * 2048 + 2 * 16384 + 4 * 8448),       # 336 tiles per image, capped at 64 workgroups
    ((32, 8400, 2), 2150400 + 3 * 2048 + 2 * 8448 + 4 * 8448),         # rt = 256: 33 tiles
    ((1, 300, 2048), 2560 + 3 * 256 + 2 * 2560 + 4 * 256),             # rt = 1
]


def test_the_workspace_sizes_are_the_published_ones():
    """The expectations are the layouts stated in include/evrep.h worked out by hand, not what the library returned."""
    from event_representation_study_amd import _lib, build
    build.build()
    lib = _lib.load()
    for args, size in _WORKSPACE_SIZES:
        assert lib.evrep_detloss_distill_workspace_bytes(*args) == size, args
    lv = (_lib.CwdLevel * 3)()
    for l, (n, c, h, w) in enumerate(((2, 3, 8, 8), (2, 3, 4, 4), (32, 5, 2, 2))):
        lv[l].n, lv[l].c, lv[l].h, lv[l].w = n, c, h, w
    P = ctypes.cast(lv, ctypes.c_void_p)
    assert lib.evrep_detloss_cwd_workspace_bytes(P, 3) == 1536 and lib.evrep_detloss_cwd_workspace_bytes(P, 2) == 256   # 172, 12 rows
    assert lib.evrep_detloss_cwd_workspace_bytes(P, 0) == 0 and lib.evrep_detloss_cwd_workspace_bytes(P, 4) == 0
    assert lib.evrep_detloss_cwd_workspace_bytes(None, 3) == 0
    lv[1].h = 0
    assert lib.evrep_detloss_cwd_workspace_bytes(P, 3) == 0 and lib.evrep_detloss_cwd_workspace_bytes(P, 1) == 256
    lv[1].h, lv[0].n, lv[0].c = 4, 1 << 12, (1 << 12) + 1
    assert lib.evrep_detloss_cwd_workspace_bytes(P, 3) == 0


def test_the_entry_points_refuse_bad_arguments_before_any_launch():
    """Every refusal through a call that is valid but for one thing; nothing is launched (the pointers are not memory)."""
    from event_representation_study_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    DFL, NOGRAD, F32T = _lib.DETLOSS_USE_DFL, _lib.DETLOSS_NO_GRAD, _lib.DETLOSS_F32_TARGETS
    good = [P(0x1000), P(0x2000), P(0x1100), P(0x2100), P(0x3000), P(0x4000), P(0x5000), P(0x6000), P(0x7000), P(0x8000), 3, 84, 2, 16,
            1.0, 2.5, 0.5, 20.0, 1.0, 1.0, DFL, P(0x9000), P(0xA000), P(0xB000), P(0xC000), P(0xD000), None]

    def call(**change):
        args = list(good)
        for i, v in change.items():
            args[int(i[1:])] = v
        return lib.evrep_detloss_distill(*args)
    for change in (dict(a10=0), dict(a10=65536), dict(a11=0), dict(a11=(1 << 24) + 1), dict(a12=0), dict(a12=2049), dict(a11=1 << 24, a12=2048),
                   dict(a13=-1), dict(a13=33), dict(a13=0), dict(a20=8), dict(a20=DFL | 16), dict(a0=None), dict(a1=None), dict(a1=P(0x2002)),
                   dict(a2=None), dict(a2=P(0x1102)), dict(a3=None), dict(a3=P(0x2101)), dict(a4=None), dict(a5=P(0x4001)), dict(a6=None),
                   dict(a6=P(0x5004)), dict(a7=None), dict(a7=P(0x6004)), dict(a8=P(0x7004)), dict(a8=P(0x7002), a20=DFL | F32T),
                   dict(a9=None), dict(a17=0.0), dict(a17=-1.0), dict(a17=float("inf")), dict(a17=float("nan")), dict(a21=None),
                   dict(a21=P(0x9004)), dict(a22=None), dict(a23=None), dict(a23=P(0xB002)), dict(a22=P(0xA002), a20=DFL | NOGRAD),
                   dict(a24=None), dict(a24=P(0xC002)), dict(a25=None), dict(a25=P(0xD080))):
        assert call(**change) == _lib.EVREP_EINVAL, change
    lv = (_lib.CwdLevel * 3)()
    for l, hw in enumerate((8, 4, 2)):
        lv[l].s, lv[l].t, lv[l].grad_s = 0x1000 * (l + 1), 0x10000 * (l + 1), 0x100000 * (l + 1)
        lv[l].n, lv[l].c, lv[l].h, lv[l].w = 2, 3, hw, hw
    L = ctypes.cast(lv, ctypes.c_void_p)
    good_cw = [L, 3, 1.0, 0, P(0x9000), P(0xD000), None]
    for i, v in ((0, None), (1, 0), (1, 4), (2, 0.0), (2, -2.0), (2, float("nan")), (2, float("inf")), (3, 1), (3, 4), (4, None), (4, P(0x9004)),
                 (5, None), (5, P(0xD010))):
        args = list(good_cw)
        args[i] = v
        assert lib.evrep_detloss_cwd(*args) == _lib.EVREP_EINVAL, (i, v)
    for field, v in (("s", None), ("s", 0x1002), ("t", None), ("t", 0x10001), ("grad_s", None), ("grad_s", 0x100002), ("n", 0), ("c", 0), ("h", 0),
                     ("w", -1), ("h", (1 << 22) + 1), ("n", (1 << 23) + 1)):   # h * w = 2^24 + 4, n * c = 3 * 2^23 + 3
        old = getattr(lv[1], field)
        setattr(lv[1], field, v)
        assert lib.evrep_detloss_cwd(*good_cw) == _lib.EVREP_EINVAL, (field, v)
        setattr(lv[1], field, old)


def test_the_python_routes_refuse_what_they_do_not_compute():
    dd = _dd()
    c = cases.nc_one()
    t = tensors(c)
    tail = (t["anc"], t["stride"], t["labels"], t["tb"], t["ts"], t["fg"], 1, 20.0, 3, 10)
    dd.distill_batch(t["p"], t["z"], t["tp"], t["tz"], *tail)
    for change, match in ((dict(p=t["p"].double()), r"\.float\(\)"), (dict(z=t["z"].half()), r"\.float\(\)"), (dict(tp=t["tp"].double()), r"\.float\(\)"),
                          (dict(tz=t["tz"].half()), r"\.float\(\)"), (dict(tp=t["tp"][:, :-1]), "t_pred_scores"), (dict(tz=t["tz"][..., :-4]), "t_pred_distri")):
        a = dict(p=t["p"], z=t["z"], tp=t["tp"], tz=t["tz"])
        a.update(change)
        with pytest.raises(ValueError, match=match):
            dd.distill_batch(a["p"], a["z"], a["tp"], a["tz"], *tail)
    with pytest.raises(ValueError, match="num_classes"):
        dd.distill_batch(t["p"], t["z"], t["tp"], t["tz"], *tail[:6], 3, 20.0, 3, 10)
    for T in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="temperature"):
            dd.distill_batch(t["p"], t["z"], t["tp"], t["tz"], *tail[:7], T, 3, 10)
    with pytest.raises(ValueError, match="reg_max"):
        dd.distill_batch(t["p"], t["z"], t["tp"], t["tz"], *tail, reg_max=0)
    for iou_type in ("siou", "ciou", "diou"):
        with pytest.raises(NotImplementedError, match="giou"):
            dd.ComputeLossDistill(num_classes=1, iou_type=iou_type)
    crit = dd.ComputeLossDistill(num_classes=1)
    assert crit.warmup_epoch == 0 and crit.loss_weight["cwd"] == 10.0 and crit.distill_weight == {"class": 1.0, "dfl": 1.0} and not crit.distill_feat
    cw = cases.CW_CASES["plain"]()
    s, tt = [torch.from_numpy(x) for x in cw["s"]], [torch.from_numpy(x) for x in cw["t"]]
    dd.distill_cw(s, tt)
    with pytest.raises(ValueError, match="at least 3"):
        dd.distill_cw(s[:2], tt[:2])
    with pytest.raises(ValueError, match=r"t_feats\[1\]"):
        dd.distill_cw(s, [tt[0], tt[1][:, :2], tt[2]])
    with pytest.raises(ValueError, match=r"\.float\(\)"):
        dd.distill_cw([s[0].double(), s[1], s[2]], tt)
    with pytest.raises(ValueError, match=r"s_feats\[2\]"):
        dd.distill_cw([s[0], s[1], s[2][0]], [tt[0], tt[1], tt[2][0]])
    with pytest.raises(ValueError, match="temperature"):
        dd.distill_cw(s, tt, 0)


# --------------------------------------------------------------------------------------------------------- the public routes
def test_distill_batch_on_cpu_tensors_carries_the_host_gradients():
    dd = _dd()
    c = cases.t_one()
    want, gs, gz, _ = cases.host(c)
    t = tensors(c)
    p, z = t["p"].clone().requires_grad_(True), t["z"].clone().requires_grad_(True)
    tp = t["tp"].clone().requires_grad_(True)                          # a teacher that requires grad is detached
    args = (t["anc"], t["stride"], t["labels"], t["tb"], t["ts"], t["fg"], 2, c["T"], c["epoch"], c["max_epoch"])
    loss, items, st = dd.distill_batch(p, z, tp, t["tz"], *args, return_status=True)
    assert loss.dtype == torch.float64 and loss.dim() == 0 and loss.requires_grad and not items.requires_grad and tuple(items.shape) == (3,)
    total, parts = cases.total(c, want)
    assert loss.item() == total and items.tolist() == parts and st.tolist() == [0, 0, 0]
    (loss * 2.0).backward()
    assert_bit_equal(p.grad.numpy(), gs * F32(2))
    assert_bit_equal(z.grad.numpy(), gz * F32(2))
    assert tp.grad is None
    with torch.no_grad():
        quiet, items2 = dd.distill_batch(p, z, tp, t["tz"], *args)
    assert not quiet.requires_grad and quiet.item() == loss.item() and torch.equal(items, items2)


def test_distill_cw_on_cpu_tensors_carries_the_host_gradients():
    dd = _dd()
    c = cases.CW_CASES["four_levels"]()
    out, grads = cases.cw_host(c)
    s = [torch.from_numpy(x).clone().requires_grad_(True) for x in c["s"]]
    t = [torch.from_numpy(x) for x in c["t"]]
    loss = dd.distill_cw(s, t)
    assert loss.dtype == torch.float64 and loss.dim() == 0 and loss.item() == out[0]
    (loss * 2.0).backward()
    for l in range(3):
        assert_bit_equal(s[l].grad.numpy(), grads[l] * F32(2))
    assert s[3].grad is None
    with torch.no_grad():
        assert not dd.distill_cw(s, t).requires_grad
    c2 = cases.CW_CASES["tau_two"]()
    assert dd.distill_cw([torch.from_numpy(x) for x in c2["s"]], [torch.from_numpy(x) for x in c2["t"]], 2).item() == cases.cw_host(c2)[0][0]


@pytest.mark.parametrize("distill_feat", [False, True])
def test_compute_loss_distill_on_cpu_tensors_end_to_end(distill_feat):
    from event_representation_study_amd import detector_assign as da
    from event_representation_study_amd import detector_loss as dl
    import detector_assign_cases as acases
    import detector_distill_ref as ref
    dd = _dd()
    B, S, nc, T, epoch, max_epoch = 3, 64, 2, 20.0, 4, 12
    rng = np.random.default_rng(31)
    c = lcases.base(31, S=S, B=B, nc=nc)
    feats = [torch.zeros((B, 1, S // s, S // s)) for s in (8, 16, 32)]
    p = torch.from_numpy(rng.uniform(0.05, 0.95, c["p"].shape).astype(F32)).requires_grad_(True)
    z = torch.from_numpy(c["z"]).requires_grad_(True)
    tp = torch.from_numpy(rng.uniform(0.05, 0.95, c["p"].shape).astype(F32))
    tz = torch.from_numpy((c["z"] + rng.normal(0, 0.5, c["z"].shape)).astype(F32))
    cw = cases.cw_case(32, [(8, 8), (4, 4), (2, 2)], N=B, C=4)
    sf = [torch.from_numpy(x).requires_grad_(True) for x in cw["s"]]
    tf = [torch.from_numpy(x) for x in cw["t"]]
    targets = torch.from_numpy(acases.targets(32, [3, 0, 4], nc, lo=0.2, hi=0.7))
    crit = dd.ComputeLossDistill(num_classes=nc, ori_img_size=S, distill_feat=distill_feat)
    loss, items = crit((feats, p, z), (feats, tp, tz), sf, tf, targets, epoch, max_epoch, T, 0, S, S)
    assert tuple(items.shape) == (4,) and items.dtype == torch.float64 and crit.last_status.tolist() == [0, 0, 0]
    loss.backward()
    # the same targets by hand, then the restatement
    anc, stride = da.anchor_points(S)
    box = dl.decode_host(z.detach().numpy(), anc, stride, 16, True)
    px = (box * stride.reshape(1, -1, 1).astype(F64)).astype(F32)
    gt = da.preprocess_host(targets.numpy(), B, S, S)[0]
    labels, tb, ts, fg, _ = da.tal_host(p.detach().numpy(), px, anc, gt)
    assert fg.any() and not fg[1].any()
    r = ref.distill_terms(p, z, tp, tz, torch.from_numpy(anc), torch.from_numpy(stride), torch.from_numpy(labels), torch.from_numpy(tb),
                          torch.from_numpy(ts), torch.from_numpy(fg), nc, 16, True, lcases.WEIGHTS, T, epoch, max_epoch)
    want, gs_want = r["loss"], r["grad_scores"].numpy()
    if distill_feat:
        rc = ref.cw_terms(sf, tf)
        k = ref.decay(epoch, max_epoch) * 10.0
        want = want + rc["loss"] * k
        assert items[3].item() == pytest.approx(rc["loss"] * k, rel=1e-12)
        for l in range(3):
            assert np.abs(sf[l].grad.numpy() - rc["grads"][l].numpy() * k).max() <= 1e-6 * np.abs(rc["grads"][l].numpy() * k).max()
    else:
        assert items[3].item() == 0 and all(x.grad is None for x in sf)
    assert loss.item() == pytest.approx(want, rel=1e-12)
    assert items[:3].tolist() == pytest.approx([r["loss_iou"] * 2.5, (r["loss_dfl"] + r["d_loss_dfl"] * ref.decay(epoch, max_epoch)) * 0.5,
                                                r["loss_cls"] + r["d_loss_cls"] * ref.decay(epoch, max_epoch)], rel=1e-12)
    assert np.abs(p.grad.numpy() - gs_want).max() <= 2.0 ** -23 * np.abs(gs_want).max()
    assert np.abs(z.grad.numpy() - r["grad_distri"].numpy()).max() <= 2.0 ** -23 * np.abs(r["grad_distri"].numpy()).max()
    # the warm-up epochs need an assigner, as in ComputeLoss
    with pytest.raises(NotImplementedError, match="ATSSAssigner"):
        dd.ComputeLossDistill(num_classes=nc, warmup_epoch=4)((feats, p, z), (feats, tp, tz), sf, tf, targets, 0, max_epoch, T, 0, S, S)
    with pytest.raises(ValueError, match="t_pred_scores"):
        crit((feats, p, z), (feats, tp[:, :-1], tz), sf, tf, targets, epoch, max_epoch, T, 0, S, S)
