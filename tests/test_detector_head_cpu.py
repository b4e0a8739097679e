"""CPU-only: the host mirror of the head's decode and tail (detector_head.predict_host / train_outputs_host /
train_backward_host) against the golden recorded from the reference's own Detect.forward (tests/golden/README_detector_head.md),
the CPU-tensor routes, the refusals of the C entries and of the Python module.

BOUNDS.  u = 2^-53.
  host against ref64 (both float64): they differ in the order in which torch adds the K exponentials of the softmax, the order
    of proj_conv's K products, and exp's last bit.  Per side: each e_k carries the relative error of one exp (<= 1 ulp = 2u each
    side), Z that and K - 1 additions ((K + 1)u relatively), pr_k one division more, d another K additions: about (2K + 4)u
    relatively on each side, so the two d differ by at most (4K + 8)u * R <= 8 * K * u * R.  The box statements that follow are
    the same float64 operations on both sides and add their own roundings, u * (|ax| + R) each.  Per box column, in grid
    units: 8 * K * u * (|a| + R) with a the anchor's coordinate (for w and h the same: both x1 and x2 enter); times the stride.
    Without DFL both sides run the same operations on the same numbers and K = 1 leaves 8u(|a| + R), R read as the greatest d.
    Scores: 1 / (1 + exp(-x)) is an exp, an addition and a division on our side and some float64 sigmoid on torch's: a few ulp
    relatively, 8 * u * p.
  host against ref32: within 4 x E of the output group (E: the reference's own float32 rounding, MEASURED by the golden maker
    against its own float64 run; 4: the margin the loss fixture uses, for summation orders that differ between torch builds),
    plus one float32 ulp of the value.
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import assert_bit_equal, load_golden
import detector_head_cases as cases

F32, F64 = np.float32, np.float64
U = 2.0 ** -53


def _dh():
    from event_representation_study_amd import detector_head
    return detector_head


@pytest.fixture(scope="module")
def golden():
    return load_golden("detector_head")


def _ulp32(v):
    return np.spacing(np.abs(v).astype(F32)).astype(F64)


def check_pred_against_golden(name, c, pred, g):
    """pred (B, N, 5 + nc) float32 against the case's ref32: 4 x E per group plus one float32 ulp."""
    _, _, s = cases.anchors(c["shapes"], c["strides"])
    ref = g[name + "/ref32"].astype(F64)
    diff = np.abs(pred.astype(F64) - ref)
    box = 4.0 * float(g["measured/E_box"]) * s[None, :, None] + _ulp32(pred[..., :4])
    assert (diff[..., :4] <= box).all(), (name, "box", float((diff[..., :4] / box).max()))
    cls = 4.0 * float(g["measured/E_cls"]) + _ulp32(pred[..., 5:])
    assert (diff[..., 5:] <= cls).all(), (name, "class", float((diff[..., 5:] / cls).max()))
    assert_bit_equal(pred[..., 4], np.ones(pred.shape[:2], F32), name + " column 4")


@pytest.mark.parametrize("name", sorted(cases.GOLDEN))
def test_predict_host_against_the_reference(name, golden):
    dh = _dh()
    c = cases.build(name)
    pred = dh.predict_host(c["cls"], c["reg"], c["strides"], c["R"], c["use_dfl"])
    assert pred.dtype == F32 and pred.shape == (c["B"], c["N"], 5 + c["nc"])
    check_pred_against_golden(name, c, pred, golden)
    # against ref64: the derived bound, plus the one rounding to float32 of the value the mirror stores
    ax, ay, s = cases.anchors(c["shapes"], c["strides"])
    ref = golden[name + "/ref64"]
    assert ref.dtype == F64
    dmax = float(c["R"]) if c["use_dfl"] else float(max(np.abs(r).max() for r in c["reg"]))
    coord = np.stack([ax, ay, ax, ay], -1)[None]
    bound = 8.0 * c["K"] * U * (coord + dmax) * s[None, :, None]
    diff = np.abs(pred.astype(F64) - ref)
    half_ulp = 0.5 * _ulp32(pred[..., :4]) * (1 + 2.0 ** -20)
    assert (diff[..., :4] <= bound + half_ulp).all(), (name, float((diff[..., :4] - half_ulp).max()), float(bound.min()))
    p64 = ref[..., 5:]
    assert (diff[..., 5:] <= 8.0 * U * p64 + 0.5 * _ulp32(pred[..., 5:]) * (1 + 2.0 ** -20)).all(), name


@pytest.mark.parametrize("name", sorted(cases.GOLDEN))
def test_train_host_against_the_reference(name, golden):
    dh = _dh()
    c = cases.build(name)
    scores, distri = dh.train_outputs_host(c["cls"], c["reg"], c["R"], c["use_dfl"])
    assert_bit_equal(distri, golden[name + "/distri"], name + " pred_distri")
    ref = golden[name + "/scores"]
    assert scores.dtype == F32 and scores.shape == ref.shape
    tol = 4.0 * float(golden["measured/E_scores"]) + _ulp32(scores)
    assert (np.abs(scores.astype(F64) - ref.astype(F64)) <= tol).all(), name
    # the backward on the golden's own scores: bit for bit what torch's autograd recorded
    gcls, greg = dh.train_backward_host(ref, c["Wc"], c["Wr"], c["shapes"])
    for l in range(len(c["shapes"])):
        assert_bit_equal(gcls[l], golden["%s/gcls_%d" % (name, l)], "%s gcls %d" % (name, l))
        assert_bit_equal(greg[l], golden["%s/greg_%d" % (name, l)], "%s greg %d" % (name, l))
    only_c = dh.train_backward_host(ref, c["Wc"], None, c["shapes"])
    assert only_c[1] is None and all(np.array_equal(a, b) for a, b in zip(only_c[0], gcls))


def test_the_measured_quantities_are_what_the_readme_says(golden):
    assert 0 < float(golden["measured/E_box"]) < 2.0 ** -16          # a few float32 ulp of 16 grid units
    assert 0 < float(golden["measured/E_cls"]) < 2.0 ** -22
    assert cases.TILE == _dh().TILE


@pytest.mark.parametrize("name", ["default", "odd", "no_dfl", "eight_levels"])
def test_cpu_tensor_routes(name):
    dh = _dh()
    c = cases.build(name)
    cls = [torch.from_numpy(a.copy()).requires_grad_(True) for a in c["cls"]]
    reg = [torch.from_numpy(a.copy()).requires_grad_(True) for a in c["reg"]]
    pred = dh.predict(cls, reg, c["strides"], c["R"], c["use_dfl"])
    assert_bit_equal(pred.numpy(), dh.predict_host(c["cls"], c["reg"], c["strides"], c["R"], c["use_dfl"]), name)
    scores, distri = dh.train_outputs(cls, reg, c["R"], c["use_dfl"])
    hs, hd = dh.train_outputs_host(c["cls"], c["reg"], c["R"], c["use_dfl"])
    assert_bit_equal(scores.detach().numpy(), hs, name)
    assert_bit_equal(distri.detach().numpy(), hd, name)
    ((torch.from_numpy(c["Wc"]) * scores).sum() + (torch.from_numpy(c["Wr"]) * distri).sum()).backward()
    gcls, greg = dh.train_backward_host(hs, c["Wc"], c["Wr"], c["shapes"])
    for l in range(len(cls)):
        assert_bit_equal(cls[l].grad.numpy(), gcls[l], "%s gcls %d" % (name, l))
        assert_bit_equal(reg[l].grad.numpy(), greg[l], "%s greg %d" % (name, l))
    # one output alone
    cls2 = [torch.from_numpy(a.copy()).requires_grad_(True) for a in c["cls"]]
    reg2 = [torch.from_numpy(a.copy()).requires_grad_(True) for a in c["reg"]]
    s2, _ = dh.train_outputs(cls2, reg2, c["R"], c["use_dfl"])
    (torch.from_numpy(c["Wc"]) * s2).sum().backward()
    assert all(r.grad is None for r in reg2)
    assert_bit_equal(cls2[0].grad.numpy(), gcls[0], name)
    tail = dh.DetectTail(c["nc"], c["strides"], c["use_dfl"], c["R"])
    assert not list(tail.parameters())
    tail.eval()
    assert_bit_equal(tail(cls, reg).numpy(), pred.numpy(), name)
    tail.train()
    ts, td = tail(cls, reg)
    assert_bit_equal(ts.detach().numpy(), hs, name)
    assert_bit_equal(td.detach().numpy(), hd, name)


def _maps(B=2, nc=3, K=17, shapes=((2, 3), (1, 2))):
    return ([torch.zeros((B, nc, h, w)) for h, w in shapes], [torch.zeros((B, 4 * K, h, w)) for h, w in shapes])


@pytest.mark.parametrize("fault,level", [("half", 1), ("double", 0), ("channels_last", 0), ("sliced", 1), ("meta_device", 1),
                                         ("reg_shape", 1), ("reg_channels", 0), ("cls_channels", 1), ("batch", 1)])
def test_python_refusals_name_the_level(fault, level):
    dh = _dh()
    cls, reg = _maps(shapes=((2, 3), (2, 2)))
    if fault == "half":
        reg[level] = reg[level].half()
    elif fault == "double":
        cls[level] = cls[level].double()
    elif fault == "channels_last":
        cls[level] = cls[level].contiguous(memory_format=torch.channels_last)
        assert not cls[level].is_contiguous()
    elif fault == "sliced":
        reg[level] = torch.zeros((2, 68, 2, 4))[..., ::2]
    elif fault == "meta_device":
        reg[level] = reg[level].to("meta")
    elif fault == "reg_shape":
        reg[level] = torch.zeros((2, 68, 3, 2))
    elif fault == "reg_channels":
        reg[level] = torch.zeros((2, 64, 2, 3))
    elif fault == "cls_channels":
        cls[level] = torch.zeros((2, 4, 2, 2))
    elif fault == "batch":
        cls[level] = torch.zeros((3, 3, 2, 2))
    for call in (lambda: dh.predict(cls, reg, (8, 16)), lambda: dh.train_outputs(cls, reg),
                 lambda: dh.predict_batch(cls, reg, 0.25, 0.45, strides=(8, 16))):
        with pytest.raises(ValueError, match="level %d" % level):
            call()


def test_other_python_refusals():
    dh = _dh()
    cls, reg = _maps()
    with pytest.raises(ValueError):
        dh.predict(cls, reg, (8, 16, 32))
    with pytest.raises(ValueError, match="level 1"):
        dh.predict(cls, reg, (8, 0))
    with pytest.raises(ValueError):
        dh.predict(cls * 5, reg * 5, (8,) * 10)
    with pytest.raises(ValueError):
        dh.predict(cls, reg, (8, 16), reg_max=33)
    with pytest.raises(ValueError, match="level 0"):
        dh.DetectTail(4, (8, 16))(cls, reg)


def test_check_proj():
    dh = _dh()
    tail = dh.DetectTail(2, (8, 16, 32), reg_max=16)
    tail.check_proj(torch.linspace(0, 16, 17).view(1, 17, 1, 1))
    tail.check_proj(torch.linspace(0, 16, 17))
    with pytest.raises(ValueError):
        tail.check_proj(torch.linspace(0, 16, 17).flip(0))
    with pytest.raises(ValueError):
        tail.check_proj(torch.linspace(0, 15, 16))
    with pytest.raises(ValueError):
        tail.check_proj(torch.linspace(0, 16, 17) * 1.0001)
    dh.DetectTail(2, (8,), reg_max=7).check_proj(torch.linspace(0, 7, 8).view(1, 8, 1, 1))


# ------------------------------------------------------------------------------------------------- the C entries, no device
@pytest.fixture(scope="module")
def lib():
    from event_representation_study_amd import build, _lib
    build.build()
    return _lib.load()


def _tables(L=3, h=2, w=3, stride=8.0, base=0x10000000):
    from event_representation_study_amd import _lib
    lv, gl = (_lib.DetheadLevel * max(L, 1))(), (_lib.DetheadGradLevel * max(L, 1))()
    for l in range(max(L, 1)):
        lv[l] = _lib.DetheadLevel(base + 0x100000 * l, base + 0x100000 * l + 0x80000, h, w, stride)
        gl[l] = _lib.DetheadGradLevel(base + 0x100000 * l, base + 0x100000 * l + 0x80000, h, w)
    return lv, gl


_OUT = (0x30000000, 0x31000000, 0x32000000)
#           what: keyword overrides of _call
_REFUSED = {
    "L = 0": dict(L=0), "L = 9": dict(L=9), "B = 0": dict(B=0), "B = 65536": dict(B=65536), "nc = 0": dict(nc=0), "nc = 4097": dict(nc=4097),
    "R = -1": dict(R=-1, flags=0), "R = 33": dict(R=33), "R = 0 with DFL": dict(R=0), "unknown flag": dict(flags=3),
    "h = 0": dict(h=0), "w = 0": dict(w=0), "N > 2^24": dict(h=4096, w=2048), "NULL table": dict(table=None),
    "NULL output": dict(out=(None, None, None)), "misaligned output": dict(out=(0x30000002, 0x31000002, 0x32000002)),
    "NULL map": dict(base=0), "misaligned map": dict(base=0x10000002),
}
_REFUSED_FORWARD = {"stride = 0": dict(stride=0.0), "stride < 0": dict(stride=-8.0), "stride inf": dict(stride=float("inf")),
                    "stride NaN": dict(stride=float("nan"))}


def _call(lib, entry, L=3, B=2, nc=3, R=16, flags=1, h=2, w=3, stride=8.0, base=0x10000000, table="own", out=_OUT):
    lv, gl = _tables(min(L, 8) if L > 0 else 1, h, w, stride, base)
    if L == 9:
        lv, gl = _tables(9, h, w, stride, base)
    vp = ctypes.c_void_p
    if entry == "predict":
        return lib.evrep_dethead_predict(None if table is None else lv, L, B, nc, R, flags, vp(out[0]), None)
    if entry == "train":
        return lib.evrep_dethead_train(None if table is None else lv, L, B, nc, R, flags, vp(out[0]), vp(out[1]), None)
    return lib.evrep_dethead_train_backward(None if table is None else gl, L, B, nc, R, flags, vp(out[0]), vp(out[1]), vp(out[2]), None)


@pytest.mark.parametrize("entry", ["predict", "train", "backward"])
def test_c_entries_refuse_before_any_launch(lib, entry):
    """Made-up addresses, as tests/test_capi_cpu.py's pointer test: skipped where a device could be reached."""
    if torch.cuda.is_available():
        pytest.skip("GPU present: made-up addresses must never be able to reach a launch")
    from event_representation_study_amd._lib import EVREP_EINVAL
    assert _call(lib, entry) != EVREP_EINVAL                             # past the checks (and fails in HIP: there is no device)
    assert _call(lib, entry, R=0, flags=0) != EVREP_EINVAL
    assert _call(lib, entry, L=8, h=1, w=1) != EVREP_EINVAL
    refused = dict(_REFUSED, **(_REFUSED_FORWARD if entry != "backward" else {}))
    for what, kw in refused.items():
        assert _call(lib, entry, **kw) == EVREP_EINVAL, (entry, what)


def test_backward_halves_come_whole_or_not_at_all(lib):
    if torch.cuda.is_available():
        pytest.skip("GPU present: made-up addresses must never be able to reach a launch")
    from event_representation_study_amd import _lib
    vp = ctypes.c_void_p
    _, gl = _tables()

    def call(table, p, gs, gd):
        return lib.evrep_dethead_train_backward(table, 3, 2, 3, 16, 1, p, gs, gd, None)
    only_reg = (_lib.DetheadGradLevel * 3)(*[_lib.DetheadGradLevel(None, g.greg, g.h, g.w) for g in gl])
    only_cls = (_lib.DetheadGradLevel * 3)(*[_lib.DetheadGradLevel(g.gcls, None, g.h, g.w) for g in gl])
    assert call(only_reg, None, None, vp(_OUT[2])) != _lib.EVREP_EINVAL
    assert call(only_cls, vp(_OUT[0]), vp(_OUT[1]), None) != _lib.EVREP_EINVAL
    assert call(gl, None, None, None) == _lib.EVREP_EINVAL                # nothing asked for
    assert call(gl, None, None, vp(_OUT[2])) == _lib.EVREP_EINVAL         # gcls given without grad_scores
    assert call(only_reg, vp(_OUT[0]), vp(_OUT[1]), vp(_OUT[2])) == _lib.EVREP_EINVAL   # grad_scores without gcls
    assert call(only_cls, None, vp(_OUT[1]), None) == _lib.EVREP_EINVAL   # grad_scores without the stored scores
    mixed = (_lib.DetheadGradLevel * 3)(gl[0], _lib.DetheadGradLevel(None, gl[1].greg, 2, 3), gl[2])
    assert call(mixed, vp(_OUT[0]), vp(_OUT[1]), vp(_OUT[2])) == _lib.EVREP_EINVAL


def test_entries_are_declared_and_bound(lib):
    from event_representation_study_amd import _lib
    for name, nargs in (("evrep_dethead_predict", 8), ("evrep_dethead_train", 9), ("evrep_dethead_train_backward", 10)):
        assert isinstance(_lib.SYMBOLS[name], _lib.Status) and len(_lib.SYMBOLS[name][1]) == nargs and getattr(lib, name) is not None
    assert not [n for n in _lib.SYMBOLS if "dethead" in n and n.endswith("_scratch_bytes")]
    assert ctypes.sizeof(_lib.DetheadLevel) == 32 and ctypes.sizeof(_lib.DetheadGradLevel) == 24
    assert (_lib.DETHEAD_USE_DFL, _lib.DETHEAD_MAX_LEVELS, _lib.DETHEAD_TILE) == (1, 8, 64)
