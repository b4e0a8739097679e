"""GPU: float16 and bfloat16 maps into the head's tail (csrc/evrep_dethead.hip's 16-bit instances through detector_head), rules W1
and W2 of include/evrep.h.  Everything is exact:
  * predict and train_outputs on 16-bit maps are BIT-EQUAL to the float32 entries on map.float(), the backward to the float32
    entries' gradient rounded with torch's .to(dtype) (on the host: the comparison does not rest on the device's own cast);
  * the float32 results are held to the host mirrors by the bounds of tests/test_gpu_detector_head.py (imported);
  * every bit pattern of the dtype goes through pred_distri, every rounding boundary through greg;
  * maps that start 0, 1, 2, 3 and 7 ELEMENTS into a 256-byte aligned guarded buffer (2-, 4- and 16-byte phases), gradient maps
    filled with NaN: every element written, nothing around it;
  * DetectTail + ComputeLoss on 16-bit leaves with a loss scale of 65536, inside and outside torch.autocast, and captured into
    a graph.
No test provokes a fault: every refusal returns before a launch."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import assert_bit_equal
import detector_assign_cases as acases
import detector_head_cases as cases
import detector_head_amp_cases as amp
from guarded import Arena
from test_detector_head_amp_cpu import assert_same16, assert_same32
from test_gpu_detector_head import check_pred, check_scores

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = np.float32
DTYPES = sorted(amp.DTYPES)
ALL = sorted(cases.GOLDEN) + sorted(cases.HOST_ONLY)


def _dh():
    from event_representation_study_amd import detector_head
    return detector_head


def _i(t):
    return t.contiguous().reshape(-1).view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape) and torch.equal(_i(a), _i(b))


def on_device(c, grad=False):
    return ([m.to(DEV).requires_grad_(grad) for m in c["cls"]], [m.to(DEV).requires_grad_(grad) for m in c["reg"]])


def widened(maps):
    return [m.detach().float() for m in maps]


def backward(dh, c, scores, gs, gd, dtype, **kw):
    return dh._backward_device(scores, gs, gd, c["shapes"], c["B"], c["nc"], c["R"], c["K"], c["use_dfl"], torch.device(DEV), dtype=dtype, **kw)


@pytest.mark.parametrize("dname", DTYPES)
@pytest.mark.parametrize("name", ALL)
def test_every_case_is_the_float32_entry_on_the_widened_maps(name, dname):
    dh = _dh()
    dtype = amp.DTYPES[dname]
    c = amp.build(name, dtype)
    cls, reg = on_device(c)
    before = [t.clone() for t in cls + reg]
    pred = dh.predict(cls, reg, c["strides"], c["R"], c["use_dfl"])
    assert pred.is_cuda and pred.dtype == torch.float32 and tuple(pred.shape) == (c["B"], c["N"], 5 + c["nc"])
    assert same_bits(pred, dh.predict(widened(cls), widened(reg), c["strides"], c["R"], c["use_dfl"]))
    c32 = dict(c, cls=c["cls32"], reg=c["reg32"])
    check_pred(name, c32, pred.cpu().numpy(), dh.predict_host(c["cls32"], c["reg32"], c["strides"], c["R"], c["use_dfl"]))
    scores, distri = dh.train_outputs(cls, reg, c["R"], c["use_dfl"])
    assert scores.dtype == distri.dtype == torch.float32
    s32, d32 = dh.train_outputs(widened(cls), widened(reg), c["R"], c["use_dfl"])
    assert same_bits(scores, s32) and same_bits(distri, d32)
    hs, hd = dh.train_outputs_host(c["cls32"], c["reg32"], c["R"], c["use_dfl"])
    check_scores(name, scores.cpu().numpy(), hs)
    assert_bit_equal(distri.cpu().numpy(), hd, name + " pred_distri")
    assert same_bits(pred[..., 5:], scores)
    # the backward: the float32 entry's gradient, rounded once
    gs, gd = torch.from_numpy(c["Wc"]).to(DEV), torch.from_numpy(c["Wr"]).to(DEV)
    gcls, greg = backward(dh, c, scores, gs, gd, dtype)
    fcls, freg = backward(dh, c, scores, gs, gd, torch.float32)
    hcls, hreg = dh.train_backward_host(scores.cpu().numpy(), c["Wc"], c["Wr"], c["shapes"])
    for l in range(len(c["shapes"])):
        assert gcls[l].dtype == greg[l].dtype == dtype
        assert_same16(gcls[l].cpu(), fcls[l].cpu().to(dtype), "%s gcls %d" % (name, l))
        assert_same16(greg[l].cpu(), freg[l].cpu().to(dtype), "%s greg %d" % (name, l))
        assert_bit_equal(fcls[l].cpu().numpy(), hcls[l], "%s float32 gcls %d" % (name, l))
        assert_bit_equal(freg[l].cpu().numpy(), hreg[l], "%s float32 greg %d" % (name, l))
    # determinism, inputs unchanged
    assert same_bits(dh.predict(cls, reg, c["strides"], c["R"], c["use_dfl"]), pred)
    s2, d2 = dh.train_outputs(cls, reg, c["R"], c["use_dfl"])
    assert same_bits(s2, scores) and same_bits(d2, distri)
    g2, r2 = backward(dh, c, scores, gs, gd, dtype)
    assert all(same_bits(a, b) for a, b in zip(g2 + r2, gcls + greg))
    assert all(same_bits(a, b) for a, b in zip(cls + reg, before))


@pytest.mark.parametrize("dname", DTYPES)
def test_every_bit_pattern_on_the_device(dname):
    dh = _dh()
    c = amp.bits16(amp.DTYPES[dname])
    cls, reg = on_device(c)
    scores, distri = dh.train_outputs(cls, reg, c["R"], c["use_dfl"])
    want = torch.cat([r.float().reshape(1, 68, -1).transpose(1, 2) for r in c["reg"]], 1).contiguous().numpy()
    assert_same32(distri.cpu().numpy(), want, dname + ": pred_distri is reg.float(), NaN where reg is NaN")
    s32, d32 = dh.train_outputs(widened(cls), widened(reg), c["R"], c["use_dfl"])
    assert same_bits(scores, s32)
    assert_same32(distri.cpu().numpy(), d32.cpu().numpy(), dname + ": the float32 entry")
    with np.errstate(all="ignore"):
        check_scores("bits16", scores.cpu().numpy(), dh.train_outputs_host(c["cls32"], c["reg32"], c["R"], c["use_dfl"])[0])
    assert torch.isfinite(scores).all()


@pytest.mark.parametrize("dname", DTYPES)
def test_every_rounding_boundary_on_the_device(dname):
    dh = _dh()
    dtype = amp.DTYPES[dname]
    c = amp.rounding(dtype)
    cls, reg = on_device(c)
    scores, _ = dh.train_outputs(cls, reg, c["R"], c["use_dfl"])
    gs, gd = torch.from_numpy(c["grad_scores"]).to(DEV), torch.from_numpy(c["grad_distri"]).to(DEV)
    gcls, greg = backward(dh, c, scores, gs, gd, dtype)
    fcls, freg = backward(dh, c, scores, gs, gd, torch.float32)
    want = torch.from_numpy(c["grad_distri"]).reshape(1, -1, 68).transpose(1, 2).reshape(1, 68, 1, -1).to(dtype)
    assert_same16(greg[0].cpu(), want, dname + ": greg is grad_distri.to(dtype)")
    assert_same16(greg[0].cpu(), freg[0].cpu().to(dtype), dname + ": greg")
    assert_same16(gcls[0].cpu(), fcls[0].cpu().to(dtype), dname + ": gcls")


def _shifted_input(arena, t, k, name):
    """A read-only guarded copy of `t` that starts k elements into a 256-byte aligned buffer of numel + 7 elements."""
    n = t.numel()
    padded = torch.zeros(n + 7, dtype=t.dtype)
    padded[k:k + n] = t.reshape(-1)
    buf = arena.carve_like(padded, name=name)
    view = buf[k:k + n].view(t.shape)
    assert view.is_contiguous() and view.data_ptr() % 256 == (k * t.element_size()) % 256
    return view


def _shifted_output(arena, shape, dtype, k, name):
    n = int(np.prod(shape))
    buf = arena.carve_shape((n + 7,), dtype, name=name)
    buf.fill_(float("nan"))
    return buf, buf[k:k + n].view(shape)


@pytest.mark.parametrize("dname", DTYPES)
@pytest.mark.parametrize("name", ["odd", "coco", "k33", "tile_1x65_nc3"])
@pytest.mark.parametrize("k", [0, 1, 2, 3, 7])
def test_every_alignment_and_no_stale_bytes(name, k, dname):
    dh = _dh()
    dtype = amp.DTYPES[dname]
    c = amp.build(name, dtype)
    B, nc, K = c["B"], c["nc"], c["K"]
    arena = Arena(DEV, seed=k)
    cls = [_shifted_input(arena, m, k, "cls%d" % l) for l, m in enumerate(c["cls"])]
    reg = [_shifted_input(arena, m, (k + l) % 8, "reg%d" % l) for l, m in enumerate(c["reg"])]
    ref_cls, ref_reg = on_device(c)
    pred = dh.predict(cls, reg, c["strides"], c["R"], c["use_dfl"])
    assert same_bits(pred, dh.predict(ref_cls, ref_reg, c["strides"], c["R"], c["use_dfl"]))
    scores, distri = dh.train_outputs(cls, reg, c["R"], c["use_dfl"])
    rs, rd = dh.train_outputs(ref_cls, ref_reg, c["R"], c["use_dfl"])
    assert same_bits(scores, rs) and same_bits(distri, rd)
    gs, gd = torch.from_numpy(c["Wc"]).to(DEV), torch.from_numpy(c["Wr"]).to(DEV)
    outs = [_shifted_output(arena, (B, nc, h, w), dtype, k, "gcls%d" % l) for l, (h, w) in enumerate(c["shapes"])]
    outs += [_shifted_output(arena, (B, 4 * K, h, w), dtype, (k + 1 + l) % 8, "greg%d" % l) for l, (h, w) in enumerate(c["shapes"])]
    L = len(c["shapes"])
    gcls, greg = [v for _, v in outs[:L]], [v for _, v in outs[L:]]
    backward(dh, c, scores, gs, gd, dtype, gcls=gcls, greg=greg)
    wcls, wreg = backward(dh, c, scores, gs, gd, dtype)
    torch.cuda.synchronize()
    for (buf, view), want in zip(outs, wcls + wreg):
        assert not torch.isnan(view.float()).any() and same_bits(view, want)
        off = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
        assert torch.isnan(buf[:off].float()).all() and torch.isnan(buf[off + view.numel():].float()).all()
    arena.check()
    arena.check_inputs()


@pytest.mark.parametrize("dname", DTYPES)
def test_a_view_with_an_odd_storage_offset(dname):
    dh = _dh()
    dtype = amp.DTYPES[dname]
    c = amp.build("odd", dtype)
    ref_cls, ref_reg = on_device(c)

    def odd_view(m):
        big = torch.zeros(m.numel() + 3, dtype=dtype, device=DEV)
        v = big[1:1 + m.numel()].view(m.shape)
        v.copy_(m)
        assert v.is_contiguous() and v.storage_offset() == 1 and v.data_ptr() % 4 == 2
        return v
    cls, reg = [odd_view(m).requires_grad_(True) for m in ref_cls], [odd_view(m).requires_grad_(True) for m in ref_reg]
    rc, rr = [m.clone().requires_grad_(True) for m in ref_cls], [m.clone().requires_grad_(True) for m in ref_reg]
    assert same_bits(dh.predict(cls, reg, c["strides"], c["R"], c["use_dfl"]), dh.predict(rc, rr, c["strides"], c["R"], c["use_dfl"]))
    Wc, Wr = torch.from_numpy(c["Wc"]).to(DEV), torch.from_numpy(c["Wr"]).to(DEV)
    for a, b in ((cls, reg), (rc, rr)):
        scores, distri = dh.train_outputs(a, b, c["R"], c["use_dfl"])
        ((Wc * scores).sum() + (Wr * distri).sum()).backward()
    for a, b in zip(cls + reg, rc + rr):
        assert a.grad.dtype == dtype and same_bits(a.grad, b.grad)


def _step(dh, dl, c, leaves_cls, leaves_reg, targets, crit, autocast_dtype=None):
    tail = dh.DetectTail(c["nc"], c["strides"], c["use_dfl"], c["R"]).train()
    with torch.autocast("cuda", dtype=autocast_dtype or torch.float16, enabled=autocast_dtype is not None):
        scores, distri = tail(leaves_cls, leaves_reg)
        loss, items = crit((leaves_cls, scores, distri), targets, 4, 0, 64, 64)
    (loss * 65536.0).backward()                                          # GradScaler's scale
    return loss.detach(), items


@pytest.mark.parametrize("dname", DTYPES)
def test_end_to_end_with_the_loss_under_autocast_and_in_a_graph(dname):
    """`default`'s 64 x 64 shape: DetectTail + ComputeLoss(warmup_epoch=0) on 16-bit leaves, the backward seeded with a loss
    scale of 65536.  Against the float32 run on the widened leaves: the loss bit-equal, .grad in the leaves' dtype and equal
    to that run's .grad.to(dtype); the same inside torch.autocast; one such step captured and replayed, on one stream."""
    from event_representation_study_amd import detector_loss as dl
    dh = _dh()
    dtype = amp.DTYPES[dname]
    c = amp.build("default", dtype)
    targets = torch.from_numpy(acases.targets(7, [3, 2], c["nc"], lo=0.2, hi=0.7)).to(DEV)
    crit = dl.ComputeLoss(num_classes=c["nc"], ori_img_size=64, warmup_epoch=0, max_labels=4)

    def leaves(to_float):
        cls, reg = on_device(c)
        if to_float:
            cls, reg = widened(cls), widened(reg)
        return [m.requires_grad_(True) for m in cls], [m.requires_grad_(True) for m in reg]
    c32, r32 = leaves(True)
    loss32, _ = _step(dh, dl, c, c32, r32, targets, crit)
    assert torch.isfinite(loss32) and loss32.item() > 0 and any(t.grad.abs().max().item() > 0 for t in c32 + r32)
    for ac in (None, dtype):
        c16, r16 = leaves(False)
        loss16, _ = _step(dh, dl, c, c16, r16, targets, crit, autocast_dtype=ac)
        assert same_bits(loss16, loss32)
        for a, b in zip(c16 + r16, c32 + r32):
            assert a.grad.dtype == dtype
            assert_same16(a.grad.cpu(), b.grad.cpu().to(dtype), "%s autocast %s" % (dname, ac))
    # one step captured into a graph and replayed: equal bits
    c16, r16 = leaves(False)
    eager = [t.grad.clone() for t in _run_once(dh, dl, c, c16, r16, targets, crit)]
    for t in c16 + r16:
        t.grad = None
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss_g, _ = _step(dh, dl, c, c16, r16, targets, crit)
    grads = [t.grad for t in c16 + r16]
    for g in grads:
        g.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(loss_g, loss32)
    assert all(same_bits(a, b) for a, b in zip(grads, eager))


def _run_once(dh, dl, c, c16, r16, targets, crit):
    _step(dh, dl, c, c16, r16, targets, crit)
    return c16 + r16


def test_typed_entries_refuse_without_a_launch():
    from event_representation_study_amd import _lib
    dh = _dh()
    lib = _lib.load()
    vp = ctypes.c_void_p
    cls, reg = torch.zeros((2, 2, 1, 4), dtype=torch.float16, device=DEV), torch.zeros((2, 68, 1, 4), dtype=torch.float16, device=DEV)
    out = torch.full((2, 4, 7), float("nan"), device=DEV)

    def predict(dt, cp=cls.data_ptr(), rp=reg.data_ptr(), L=1, B=2):
        table = (_lib.DetheadLevel * max(L, 1))(*[_lib.DetheadLevel(cp or None, rp or None, 1, 4, 8.0)] * max(L, 1))
        return lib.evrep_dethead_predict_typed(table, L, B, 2, 16, 1, dt, vp(out.data_ptr()), None)
    for what, rc in (("unknown code", predict(3)), ("unknown code", predict(-1)), ("odd cls address", predict(_lib.DT_F16, cp=cls.data_ptr() + 1)),
                     ("odd reg address", predict(_lib.DT_BF16, rp=reg.data_ptr() + 1)), ("% 4 == 2 with F32", predict(_lib.DT_F32, cp=cls.data_ptr() + 2)),
                     ("NULL cls", predict(_lib.DT_F16, cp=0)), ("NULL reg", predict(_lib.DT_F16, rp=0)), ("B = 65536", predict(_lib.DT_F16, B=65536)),
                     ("L = 9", predict(_lib.DT_F16, L=9))):
        assert rc == _lib.EVREP_EINVAL, what
    gl = (_lib.DetheadGradLevel * 1)(_lib.DetheadGradLevel(cls.data_ptr() + 1, reg.data_ptr(), 1, 4))
    sc = torch.zeros((2, 4, 2), device=DEV)
    gd = torch.zeros((2, 4, 68), device=DEV)
    assert lib.evrep_dethead_train_backward_typed(gl, 1, 2, 2, 16, 1, _lib.DT_F16, vp(sc.data_ptr()), vp(sc.data_ptr()), vp(gd.data_ptr()), None) == _lib.EVREP_EINVAL
    gl[0].gcls = cls.data_ptr()
    assert lib.evrep_dethead_train_backward_typed(gl, 1, 2, 2, 16, 1, 7, vp(sc.data_ptr()), vp(sc.data_ptr()), vp(gd.data_ptr()), None) == _lib.EVREP_EINVAL
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and not cls.any() and not reg.any()
    assert predict(_lib.DT_F16) == _lib.EVREP_OK                          # and the same table is accepted as it stands
    torch.cuda.synchronize()
    assert not torch.isnan(out).any()
    # the module: mixed dtypes and float64 on the device
    with pytest.raises(ValueError, match="level 0: reg map"):
        dh.predict([cls], [reg.bfloat16()], (8,))
    with pytest.raises(ValueError, match="level 0: cls map is torch.float64"):
        dh.train_outputs([cls.double()], [reg.double()])
