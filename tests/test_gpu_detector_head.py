"""GPU: the head's decode and tail (csrc/evrep_dethead.hip through detector_head.predict / train_outputs / DetectTail /
predict_batch) against the host mirror, on every case of tests/detector_head_cases.py and every host-only case (the edges of
the kernel's tile of T anchors, eight levels).

BOUNDS.  u = 2^-53.  The kernel and the mirror run the same float64 statements in the same order on the same numbers; they
differ only in exp (the device library's against the host's), each within 1 ulp of the true value, so two results are within
2 ulp = 4u of each other relatively.  Through E1 that is at most 4u on every e_k, 4u + (K - 1)u on Z once the additions round
differently, another 4u + u on pr_k and K more roundings on d: below (2K + 8)u * R on d, and below 8 * K * u * (|a| + R) per box
column in grid units once the same box statements have run on both sides (a the anchor's coordinate; times the stride).  The
sigmoid is one exp, an addition and a division: 8 * u * p.  Both are the error IN FRONT of the one rounding to float32, which can
then fall on the other side of a rounding boundary: plus one float32 ulp of the mirror's value.
Column 4, pred_distri and both backward outputs (the class one given the device's own pred_scores) are bit for bit.
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import assert_bit_equal
import detector_head_cases as cases
from guarded import Arena

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, F64 = np.float32, np.float64
U = 2.0 ** -53
ALL = sorted(cases.GOLDEN) + sorted(cases.HOST_ONLY)


def _dh():
    from event_representation_study_amd import detector_head
    return detector_head


def on_device(c, grad=False):
    cls = [torch.from_numpy(a).to(DEV).requires_grad_(grad) for a in c["cls"]]
    reg = [torch.from_numpy(a).to(DEV).requires_grad_(grad) for a in c["reg"]]
    return cls, reg


def _ulp32(v):
    return np.spacing(np.abs(v).astype(F32)).astype(F64)


def check_pred(name, c, pred, host):
    ax, ay, s = cases.anchors(c["shapes"], c["strides"])
    dmax = float(c["R"]) if c["use_dfl"] else float(max(np.abs(r).max() for r in c["reg"]))
    coord = np.stack([ax, ay, ax, ay], -1)[None]
    diff = np.abs(pred.astype(F64) - host.astype(F64))
    box = 8.0 * c["K"] * U * (coord + dmax) * s[None, :, None] + _ulp32(host[..., :4])
    assert (diff[..., :4] <= box).all(), (name, "box", float((diff[..., :4] / box).max()))
    check_scores(name, pred[..., 5:], host[..., 5:])
    assert_bit_equal(pred[..., 4], np.ones(pred.shape[:2], F32), name + " column 4")
    n_box, n_cls = int((pred[..., :4] != host[..., :4]).sum()), int((pred[..., 5:] != host[..., 5:]).sum())
    print("%s: not bit-equal to the mirror: %d of %d box values (%.3g), %d of %d class values (%.3g)"
          % (name, n_box, pred[..., :4].size, n_box / pred[..., :4].size, n_cls, pred[..., 5:].size, n_cls / pred[..., 5:].size))


def check_scores(name, scores, host):
    diff = np.abs(scores.astype(F64) - host.astype(F64))
    assert (diff <= 8.0 * U * host.astype(F64) + _ulp32(host)).all(), (name, "class", float(diff.max()))


@pytest.mark.parametrize("name", ALL)
def test_every_case_on_the_device(name):
    dh = _dh()
    c = cases.build(name)
    cls, reg = on_device(c)
    before = [t.clone() for t in cls + reg]
    pred = dh.predict(cls, reg, c["strides"], c["R"], c["use_dfl"])
    assert pred.is_cuda and pred.dtype == torch.float32 and tuple(pred.shape) == (c["B"], c["N"], 5 + c["nc"])
    check_pred(name, c, pred.cpu().numpy(), dh.predict_host(c["cls"], c["reg"], c["strides"], c["R"], c["use_dfl"]))
    scores, distri = dh.train_outputs(cls, reg, c["R"], c["use_dfl"])
    hs, hd = dh.train_outputs_host(c["cls"], c["reg"], c["R"], c["use_dfl"])
    check_scores(name, scores.cpu().numpy(), hs)
    assert_bit_equal(distri.cpu().numpy(), hd, name + " pred_distri")
    assert_bit_equal(pred[..., 5:].cpu().numpy(), scores.cpu().numpy(), name + " E4 is T1")
    # the backward launch on the device's own scores
    gs, gd = torch.from_numpy(c["Wc"]).to(DEV), torch.from_numpy(c["Wr"]).to(DEV)
    gcls, greg = dh._backward_device(scores, gs, gd, c["shapes"], c["B"], c["nc"], c["R"], c["K"], c["use_dfl"], torch.device(DEV))
    hcls, hreg = dh.train_backward_host(scores.cpu().numpy(), c["Wc"], c["Wr"], c["shapes"])
    for l in range(len(c["shapes"])):
        assert_bit_equal(gcls[l].cpu().numpy(), hcls[l], "%s gcls %d" % (name, l))
        assert_bit_equal(greg[l].cpu().numpy(), hreg[l], "%s greg %d" % (name, l))
    # determinism, inputs unchanged
    again = dh.predict(cls, reg, c["strides"], c["R"], c["use_dfl"])
    s2, d2 = dh.train_outputs(cls, reg, c["R"], c["use_dfl"])
    assert torch.equal(again.view(torch.int32), pred.view(torch.int32))
    assert torch.equal(s2.view(torch.int32), scores.view(torch.int32)) and torch.equal(d2.view(torch.int32), distri.view(torch.int32))
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(cls + reg, before))


def _shifted(arena, shape, k, name):
    """A NaN-filled float32 view of `shape` that starts k floats into a guarded, 256-byte aligned buffer of numel + 3 floats."""
    n = int(np.prod(shape))
    buf = arena.carve_shape((n + 3,), torch.float32, name=name)
    buf.fill_(float("nan"))
    return buf, buf[k:k + n].view(shape)


@pytest.mark.parametrize("name", ["odd", "coco", "k33", "tile_1x65_nc3"])
@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_no_stale_bytes_at_every_alignment(name, k):
    """Outputs that start 0, 4, 8 and 12 bytes behind a 16-byte boundary, filled with NaN: every element is written, the
    floats in front and behind stay NaN, the guard bands stay, and the values are those of the aligned call."""
    dh = _dh()
    c = cases.build(name)
    dev = torch.device(DEV)
    B, N, nc, K, R = c["B"], c["N"], c["nc"], c["K"], c["R"]
    cls, reg = on_device(c)
    arena = Arena(DEV, seed=k)
    pbuf, pred = _shifted(arena, (B, N, 5 + nc), k, "pred")
    sbuf, scores = _shifted(arena, (B, N, nc), k, "pred_scores")
    dbuf, distri = _shifted(arena, (B, N, 4 * K), (k + 1) % 4, "pred_distri")
    assert dh.predict(cls, reg, c["strides"], R, c["use_dfl"], out=pred) is pred
    dh._train_device(cls, reg, c["shapes"], B, nc, R, K, c["use_dfl"], dev, scores=scores, distri=distri)
    want = dh.predict(cls, reg, c["strides"], R, c["use_dfl"])
    ws, wd = dh.train_outputs(cls, reg, R, c["use_dfl"])
    for got, ref, buf, kk in ((pred, want, pbuf, k), (scores, ws, sbuf, k), (distri, wd, dbuf, (k + 1) % 4)):
        assert not torch.isnan(got).any()
        assert torch.equal(got.view(torch.int32), ref.view(torch.int32))
        assert torch.isnan(buf[:kk]).all() and torch.isnan(buf[kk + got.numel():]).all()
    # the backward: gradients read at the same shifts, maps filled with NaN
    gsb, gs = _shifted(arena, (B, N, nc), k, "grad_scores")
    gdb, gd = _shifted(arena, (B, N, 4 * K), (k + 2) % 4, "grad_distri")
    gs.copy_(torch.from_numpy(c["Wc"]))
    gd.copy_(torch.from_numpy(c["Wr"]))
    gcls = [arena.carve_shape((B, nc, h, w), torch.float32, name="gcls%d" % l).fill_(float("nan")) for l, (h, w) in enumerate(c["shapes"])]
    greg = [arena.carve_shape((B, 4 * K, h, w), torch.float32, name="greg%d" % l).fill_(float("nan")) for l, (h, w) in enumerate(c["shapes"])]
    dh._backward_device(scores, gs, gd, c["shapes"], B, nc, R, K, c["use_dfl"], dev, gcls=gcls, greg=greg)
    hcls, hreg = dh.train_backward_host(scores.cpu().numpy(), c["Wc"], c["Wr"], c["shapes"])
    for l in range(len(c["shapes"])):
        assert_bit_equal(gcls[l].cpu().numpy(), hcls[l], "%s gcls %d" % (name, l))
        assert_bit_equal(greg[l].cpu().numpy(), hreg[l], "%s greg %d" % (name, l))
    torch.cuda.synchronize()
    arena.check()


def test_a_row_wider_than_a_chunk():
    """nc = 300: rows of 305 and 300 floats go through in chunks of 132 columns, a span per anchor."""
    dh = _dh()
    rng = np.random.default_rng(5)
    shapes, B, nc = ((1, cases.TILE + 3), (2, 3)), 2, 300
    cls = [(rng.normal(size=(B, nc, h, w)) * 3).astype(F32) for h, w in shapes]
    reg = [(rng.normal(size=(B, 68, h, w)) * 2).astype(F32) for h, w in shapes]
    c = dict(B=B, nc=nc, R=16, K=17, use_dfl=True, shapes=shapes, strides=(8, 16), N=sum(h * w for h, w in shapes), cls=cls, reg=reg)
    dcls, dreg = on_device(c, grad=True)
    pred = dh.predict(dcls, dreg, c["strides"])
    check_pred("wide", c, pred.cpu().numpy(), dh.predict_host(cls, reg, c["strides"]))
    scores, distri = dh.train_outputs(dcls, dreg)
    check_scores("wide", scores.detach().cpu().numpy(), dh.train_outputs_host(cls, reg)[0])
    Wc = torch.from_numpy(rng.normal(size=(B, c["N"], nc)).astype(F32)).to(DEV)
    (Wc * scores).sum().backward()
    hcls, _ = dh.train_backward_host(scores.detach().cpu().numpy(), Wc.cpu().numpy(), None, shapes)
    for l in range(2):
        assert_bit_equal(dcls[l].grad.cpu().numpy(), hcls[l], "wide gcls %d" % l)
    assert all(r.grad is None for r in dreg)


@pytest.mark.parametrize("name", ["default", "four", "no_dfl"])
def test_train_outputs_end_to_end(name):
    dh = _dh()
    c = cases.build(name)
    cls, reg = on_device(c, grad=True)
    scores, distri = dh.train_outputs(cls, reg, c["R"], c["use_dfl"])
    Wc, Wr = torch.from_numpy(c["Wc"]).to(DEV), torch.from_numpy(c["Wr"]).to(DEV)
    ((Wc * scores).sum() + (Wr * distri).sum()).backward()
    hcls, hreg = dh.train_backward_host(scores.detach().cpu().numpy(), c["Wc"], c["Wr"], c["shapes"])
    for l in range(len(cls)):
        assert_bit_equal(cls[l].grad.cpu().numpy(), hcls[l], "%s gcls %d" % (name, l))
        assert_bit_equal(reg[l].grad.cpu().numpy(), hreg[l], "%s greg %d" % (name, l))
    # one output alone
    for which in (0, 1):
        cls2, reg2 = on_device(c, grad=True)
        out = dh.train_outputs(cls2, reg2, c["R"], c["use_dfl"])
        ((Wc, Wr)[which] * out[which]).sum().backward()
        used, unused, want = ((cls2, reg2, hcls), (reg2, cls2, hreg))[which]
        assert all(t.grad is None for t in unused)
        for l in range(len(used)):
            assert_bit_equal(used[l].grad.cpu().numpy(), want[l], "%s alone %d level %d" % (name, which, l))


def test_detect_tail_in_both_modes():
    dh = _dh()
    c = cases.build("four")
    cls, reg = on_device(c)
    tail = dh.DetectTail(c["nc"], c["strides"], c["use_dfl"], c["R"]).to(DEV)
    tail.eval()
    pred = tail(cls, reg)
    assert torch.equal(pred.view(torch.int32), dh.predict(cls, reg, c["strides"], c["R"], c["use_dfl"]).view(torch.int32))
    tail.train()
    scores, distri = tail(cls, reg)
    ws, wd = dh.train_outputs(cls, reg, c["R"], c["use_dfl"])
    assert torch.equal(scores.view(torch.int32), ws.view(torch.int32)) and torch.equal(distri.view(torch.int32), wd.view(torch.int32))
    tail.eval()
    assert torch.equal(tail(cls, reg).view(torch.int32), pred.view(torch.int32))


def test_predict_batch_is_nms_of_predict():
    from event_representation_study_amd.detector_output import nms_batch
    dh = _dh()
    c = cases.build("default")
    cls, reg = on_device(c)
    det, count = dh.predict_batch(cls, reg, 0.25, 0.45, strides=c["strides"], reg_max=c["R"], use_dfl=c["use_dfl"])
    wdet, wcount = nms_batch(dh.predict(cls, reg, c["strides"], c["R"], c["use_dfl"]), 0.25, 0.45)
    assert torch.equal(count, wcount) and torch.equal(det.view(torch.int32), wdet.view(torch.int32))
    assert int(count.sum()) > 0


def test_refusals_without_a_launch():
    from event_representation_study_amd import _lib
    dh = _dh()
    lib = _lib.load()
    # B = 65536
    cls, reg = [torch.zeros((65536, 1, 1, 1), device=DEV)], [torch.zeros((65536, 68, 1, 1), device=DEV)]
    out = torch.full((65536, 1, 6), float("nan"), device=DEV)
    with pytest.raises(ValueError):
        dh.predict(cls, reg, (8,), out=out)
    with pytest.raises(ValueError):
        dh.train_outputs(cls, reg)
    table = (_lib.DetheadLevel * 1)(_lib.DetheadLevel(cls[0].data_ptr(), reg[0].data_ptr(), 1, 1, 8.0))
    assert lib.evrep_dethead_predict(table, 1, 65536, 1, 16, 1, ctypes.c_void_p(out.data_ptr()), None) == _lib.EVREP_EINVAL
    assert lib.evrep_dethead_predict(table, 1, 65535, 1, 16, 1, ctypes.c_void_p(out.data_ptr()), None) == _lib.EVREP_OK
    torch.cuda.synchronize()
    assert torch.isnan(out[65535]).all() and not torch.isnan(out[:65535]).any()
    # L = 9
    cls, reg = [torch.zeros((1, 2, 1, 1), device=DEV)] * 9, [torch.zeros((1, 68, 1, 1), device=DEV)] * 9
    with pytest.raises(ValueError):
        dh.predict(cls, reg, (8,) * 9)
    table = (_lib.DetheadLevel * 9)(*[_lib.DetheadLevel(cls[0].data_ptr(), reg[0].data_ptr(), 1, 1, 8.0)] * 9)
    out = torch.full((1, 9, 7), float("nan"), device=DEV)
    assert lib.evrep_dethead_predict(table, 9, 1, 2, 16, 1, ctypes.c_void_p(out.data_ptr()), None) == _lib.EVREP_EINVAL
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
