"""GPU: the distillation losses and their gradients (csrc/evrep_detdistill.hip and the shared kernels of csrc/evrep_detloss.hip
through the C entries, detector_distill.distill_batch, distill_cw and ComputeLossDistill) against the host restatements
distill_host / cw_host within the DERIVED bounds of tests/detector_distill_cases.py plus one float32 rounding for the stored
gradients, and against the golden recorded from the reference's own loss_distill.py within four times its MEASURED float32
rounding.

Shapes: A = 84 (S = 64: less than one workgroup) and A = 525 (S = 160: three workgroups per image, the last one of 13 anchors;
with nc = 80 twenty-one tiles of 25 rows per image); B in {1, 3}; nc in {1, 2, 80}; R = 16, R = 8, and R = 0 without DFL;
feature rows of 1 .. 6400 values on both sides of 64, 256 and the staging limit 4096; one smoke case at 8400 anchors."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import assert_bit_equal, load_golden
import detector_assign_cases as acases
import detector_distill_cases as cases
import detector_loss_cases as lcases
from guarded import FILLS, Arena
from test_detector_distill_cpu import check_against_bounds, check_against_golden, check_cw_against_bounds, check_cw_against_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, F64 = np.float32, np.float64
F32_ROUND = 2.0 ** -24


def _dd():
    from event_representation_study_amd import detector_distill
    return detector_distill


def on_device(c):
    return {k: torch.from_numpy(np.asarray(c[k])).to(DEV) for k in cases.KEYS}


def entry(c, t, grad=True):
    """The C entry through the package's thin wrapper: (losses (8,), grad_scores, grad_distri, status) as numpy."""
    K = c["R"] + 1 if c["use_dfl"] else 1
    kc, kd = cases.k_of(c)
    out = _dd()._distill_device(t["p"], t["z"], t["tp"], t["tz"], t["anc"], t["stride"], t["labels"], t["tb"], t["ts"], t["fg"], c["R"], K,
                                c["use_dfl"], c["weights"], c["T"], kc, kd, grad)
    torch.cuda.synchronize()
    return tuple(None if o is None else o.cpu().numpy() for o in out)


def batch(dd, c, t, p, z, **kw):
    return dd.distill_batch(p, z, t["tp"], t["tz"], t["anc"], t["stride"], t["labels"], t["tb"], t["ts"], t["fg"], c["nc"], c["T"], c["epoch"],
                            c["max_epoch"], c["R"], c["use_dfl"], dict(zip(("class", "iou", "dfl"), c["weights"])),
                            {"class": c["dw"][0], "dfl": c["dw"][1]}, **kw)


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_every_case_on_the_device(name):
    dd = _dd()
    c = cases.CASES[name]()
    d = {}
    want, gs_h, gz_h, st_h = cases.host(c, d)
    bd = cases.bounds(c, want, d)
    t = on_device(c)
    losses, gs, gz, status = entry(c, t)
    assert gs.dtype == F32 and gz.dtype == F32 and losses.dtype == F64 and losses.shape == (8,)
    check_against_bounds(name + " [entry]", losses, gs, gz, want, d["gs"], d["gz"], bd, extra_rel=F32_ROUND)
    assert losses[5] == pytest.approx(want[5], rel=286 * cases.U, abs=0) and losses[6] == want[6]
    assert losses[7] == pytest.approx(want[7], rel=(2 * (c["nc"] - 1) + 128) * cases.U, abs=0)
    assert_bit_equal(status.view(np.uint32), st_h, name + " status")
    assert not gz[~c["fg"]].any(), "background rows of grad_distri are zeros"
    if name == "nc_one":
        assert losses[3] == 0
        kc, kd = cases.k_of(c)                                         # whatever its weight: the distillation part of grad_scores is exactly 0
        other = dd._distill_device(t["p"], t["z"], t["tp"], t["tz"], t["anc"], t["stride"], t["labels"], t["tb"], t["ts"], t["fg"], c["R"], 17,
                                   True, c["weights"], c["T"], 1000.0 * kc, kd, True)[1].cpu().numpy()
        assert_bit_equal(other, gs, "nc = 1: grad_scores does not depend on k_class")
    if name == "teacher_is_student":
        assert losses[3] == 0 and losses[4] == 0
    if name in ("no_positives", "tss_zero_with_fg", "no_dfl"):
        assert losses[4] == 0 and losses[3] > 0
    if not c["fg"].any():
        assert losses[1] == 0 and losses[2] == 0 and not gz.any() and (gs != 0).all()
    if name == "tss_zero_with_fg":
        assert losses[7] == 0 and losses[6] == 4
    if name == "w_not_tss":
        assert 0 < losses[7] < 0.9 * losses[5]
    if name == "tss_below_one":                                        # the two entries DISAGREE on loss_iou by the factor tss
        from event_representation_study_amd import detector_loss as dl
        there = dl._loss_device(t["p"], t["z"], t["anc"], t["stride"], t["labels"], t["tb"], t["ts"], t["fg"], c["R"], 17, True, c["weights"],
                                False)[0].cpu().numpy()
        assert there[3] == losses[5] == 0.7 and there[1] > 0
        assert losses[1] == pytest.approx(there[1] / 0.7, rel=4 * cases.U) and abs(losses[1] - there[1]) > 0.2 * there[1]
    again = entry(c, t)
    for a, b in zip((losses, gs, gz, status), again):
        assert_bit_equal(a, b, name + ": two calls give equal bits")
    quiet = entry(c, t, grad=False)
    assert quiet[1] is None and quiet[2] is None
    assert_bit_equal(quiet[0], losses, name + ": NO_GRAD gives the same losses")
    # distill_batch, autograd
    p, z = t["p"].clone().requires_grad_(True), t["z"].clone().requires_grad_(True)
    loss, items, st = batch(dd, c, t, p, z, return_status=True)
    assert loss.is_cuda and loss.dtype == torch.float64 and loss.dim() == 0 and items.dtype == torch.float64
    total, parts = cases.total(c, losses)
    assert loss.item() == total and items.tolist() == parts
    (loss * 2.0).backward()
    assert_bit_equal(p.grad.cpu().numpy(), gs * F32(2), name + ": backward of 2 * loss gives twice the entry's grad_scores")
    assert_bit_equal(z.grad.cpu().numpy(), gz * F32(2), name + ": and twice its grad_distri")
    assert_bit_equal(st.cpu().numpy().view(np.uint32), st_h)
    with torch.no_grad():
        quiet_loss, _ = batch(dd, c, t, p, z)
    assert not quiet_loss.requires_grad and quiet_loss.item() == loss.item()
    if name in cases.GOLDEN:
        check_against_golden(name, load_golden("detector_distill"), d, losses, gs, gz)


def cw_entry(c, grad=True):
    s = [torch.from_numpy(x).to(DEV) for x in c["s"][:3]]
    t = [torch.from_numpy(x).to(DEV) for x in c["t"][:3]]
    out, grads = _dd()._cw_device(s, t, c["tau"], grad)
    torch.cuda.synchronize()
    return out.cpu().numpy(), (None if grads is None else [g.cpu().numpy() for g in grads])


@pytest.mark.parametrize("name", sorted(cases.CW_CASES))
def test_every_channel_wise_case_on_the_device(name):
    dd = _dd()
    c = cases.CW_CASES[name]()
    d = {}
    want, grads_h = cases.cw_host(c, d)
    out, grads = cw_entry(c)
    assert out.dtype == F64 and out.shape == (4,) and all(g.dtype == F32 for g in grads)
    check_cw_against_bounds(name, c, out, grads, dict(loss=want[0], levels=list(want[1:]), grads=d["g"]), d, extra_rel=F32_ROUND)
    assert out[0] == (out[1] + out[2]) + out[3]
    if name == "one_value":
        assert not out.any() and not any(g.any() for g in grads)
    again = cw_entry(c)
    assert_bit_equal(out, again[0], name + ": two calls give equal bits")
    for a, b in zip(grads, again[1]):
        assert_bit_equal(a, b, name + ": two calls give equal bits")
    quiet = cw_entry(c, grad=False)
    assert quiet[1] is None
    assert_bit_equal(quiet[0], out, name + ": NO_GRAD gives the same losses")
    # distill_cw, autograd; a fourth level is ignored
    s = [torch.from_numpy(x).to(DEV).requires_grad_(True) for x in c["s"]]
    t = [torch.from_numpy(x).to(DEV) for x in c["t"]]
    loss = dd.distill_cw(s, t, c["tau"])
    assert loss.is_cuda and loss.dtype == torch.float64 and loss.dim() == 0 and loss.item() == out[0]
    (loss * 2.0).backward()
    for l in range(3):
        assert_bit_equal(s[l].grad.cpu().numpy(), grads[l] * F32(2), name + ": backward of 2 * loss")
    assert all(x.grad is None for x in s[3:])
    with torch.no_grad():
        assert not dd.distill_cw(s, t, c["tau"]).requires_grad
    if name in cases.CW_GOLDEN:
        check_cw_against_golden(name, load_golden("detector_distill"), d, out, grads)


@pytest.mark.parametrize("distill_feat", [False, True])
def test_compute_loss_distill_is_its_parts(distill_feat):
    from event_representation_study_amd import detector_assign as da
    from event_representation_study_amd import detector_loss as dl
    dd = _dd()
    B, S, nc, T, epoch, max_epoch = 3, 160, 2, 20.0, 4, 12
    rng = np.random.default_rng(41)
    c = lcases.base(41, S=S, B=B, nc=nc)
    feats = [torch.zeros((B, 1, S // s, S // s), device=DEV) for s in (8, 16, 32)]
    p = torch.from_numpy(rng.uniform(0.05, 0.95, c["p"].shape).astype(F32)).to(DEV).requires_grad_(True)
    z = torch.from_numpy(c["z"]).to(DEV).requires_grad_(True)
    tp = torch.from_numpy(rng.uniform(0.05, 0.95, c["p"].shape).astype(F32)).to(DEV)
    tz = torch.from_numpy((c["z"] + rng.normal(0, 0.5, c["z"].shape)).astype(F32)).to(DEV)
    cw = cases.cw_case(42, [(20, 20), (10, 10), (5, 5)], N=B, C=4)
    sf = [torch.from_numpy(x).to(DEV).requires_grad_(True) for x in cw["s"]]
    tf = [torch.from_numpy(x).to(DEV) for x in cw["t"]]
    targets = torch.from_numpy(acases.targets(42, [4, 0, 6], nc, lo=0.2, hi=0.7))
    crit = dd.ComputeLossDistill(num_classes=nc, ori_img_size=S, distill_feat=distill_feat)
    loss, items = crit((feats, p, z), (feats, tp, tz), sf, tf, targets, epoch, max_epoch, T, 0, S, S)
    assert loss.is_cuda and items.is_cuda and tuple(items.shape) == (4,) and crit.last_status.tolist() == [0, 0, 0]
    (loss * 2.0).backward()
    # the parts, called one by one
    anc, stride = (torch.from_numpy(v).to(DEV) for v in da.anchor_points(S))
    _, boxes_px = dl.decode_boxes(z, anc, stride)
    labels, tb, ts, fg, _ = da.assign_batch(p, boxes_px, anc, targets, (S, S), nc)
    assert fg.any().item() and not fg[1].any().item()
    p2, z2 = p.detach().clone().requires_grad_(True), z.detach().clone().requires_grad_(True)
    loss2, items2 = dd.distill_batch(p2, z2, tp, tz, anc, stride, labels, tb, ts, fg, nc, T, epoch, max_epoch)
    if distill_feat:
        sf2 = [x.detach().clone().requires_grad_(True) for x in sf]
        k = dd.decay(epoch, max_epoch) * 10.0
        cwl = dd.distill_cw(sf2, tf) * k
        loss2 = loss2 + cwl
        assert items[3].item() == cwl.item() > 0
    else:
        assert items[3].item() == 0 and all(x.grad is None for x in sf)
    loss2.backward()
    assert torch.equal(loss.detach(), loss2.detach()) and torch.equal(items[:3], items2)
    assert torch.equal(p.grad, p2.grad * 2) and torch.equal(z.grad, z2.grad * 2)
    if distill_feat:
        for a, b in zip(sf, sf2):
            assert torch.equal(a.grad, b.grad * 2)
    # the host route on the same tensors: the same loss to the last places, the same gradients to a float32 rounding
    crit_h = dd.ComputeLossDistill(num_classes=nc, ori_img_size=S, distill_feat=distill_feat)
    ph, zh = p.detach().cpu().requires_grad_(True), z.detach().cpu().requires_grad_(True)
    sfh = [x.detach().cpu().requires_grad_(True) for x in sf]
    loss_h, items_h = crit_h(([f.cpu() for f in feats], ph, zh), (None, tp.cpu(), tz.cpu()), sfh, [x.cpu() for x in tf], targets, epoch,
                             max_epoch, T, 0, S, S)
    loss_h.backward()
    assert loss.item() == pytest.approx(loss_h.item(), rel=1e-12)
    assert np.abs(p.grad.cpu().numpy() - 2 * ph.grad.numpy()).max() <= 2.0 ** -22 * np.abs(ph.grad.numpy()).max()
    assert np.abs(z.grad.cpu().numpy() - 2 * zh.grad.numpy()).max() <= 2.0 ** -22 * np.abs(zh.grad.numpy()).max()
    with torch.no_grad():
        quiet, _ = crit((feats, p, z), (feats, tp, tz), sf, tf, targets, epoch, max_epoch, T, 0, S, S)
    assert not quiet.requires_grad and quiet.item() == loss.item()


def test_capture_and_replay():
    dd = _dd()
    c1 = cases.with_teacher(lcases.base(51, S=64, B=3, nc=2, n_fg=7), 251)
    c2 = cases.with_teacher(lcases.base(52, S=64, B=3, nc=2, n_fg=4), 252)
    cw1, cw2 = cases.cw_case(53, [(8, 8), (4, 4), (2, 2)]), cases.cw_case(54, [(8, 8), (4, 4), (2, 2)])
    t = on_device(c1)
    s = [torch.from_numpy(x).to(DEV) for x in cw1["s"]]
    tt = [torch.from_numpy(x).to(DEV) for x in cw1["t"]]
    eager, eager_cw = entry(c1, t), cw_entry(cw1)
    kc, kd = cases.k_of(c1)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = dd._distill_device(t["p"], t["z"], t["tp"], t["tz"], t["anc"], t["stride"], t["labels"], t["tb"], t["ts"], t["fg"], 16, 17, True,
                                 c1["weights"], c1["T"], kc, kd, True)
        out_cw = dd._cw_device(s, tt, 1.0, True)
    for k in ("p", "z", "tp", "tz", "labels", "tb", "ts", "fg"):
        t[k].copy_(torch.from_numpy(c2[k]))
    for l in range(3):
        s[l].copy_(torch.from_numpy(cw2["s"][l]))
        tt[l].copy_(torch.from_numpy(cw2["t"][l]))
    graph.replay()
    torch.cuda.synchronize()
    d = {}
    want = cases.host(c2, d)
    got = [o.cpu().numpy() for o in out]
    check_against_bounds("replay on new contents", got[0], got[1], got[2], want[0], d["gs"], d["gz"], cases.bounds(c2, want[0], d),
                         extra_rel=F32_ROUND)
    d = {}
    want_cw, _ = cases.cw_host(cw2, d)
    check_cw_against_bounds("replay on new maps", cw2, out_cw[0].cpu().numpy(), [g.cpu().numpy() for g in out_cw[1]],
                            dict(loss=want_cw[0], levels=list(want_cw[1:]), grads=d["g"]), d, extra_rel=F32_ROUND)
    for k in ("p", "z", "tp", "tz", "labels", "tb", "ts", "fg"):
        t[k].copy_(torch.from_numpy(c1[k]))
    for l in range(3):
        s[l].copy_(torch.from_numpy(cw1["s"][l]))
        tt[l].copy_(torch.from_numpy(cw1["t"][l]))
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(out, eager):
        assert_bit_equal(a.cpu().numpy(), b, "the same bytes as the eager call")
    assert_bit_equal(out_cw[0].cpu().numpy(), eager_cw[0])
    for a, b in zip(out_cw[1], eager_cw[1]):
        assert_bit_equal(a.cpu().numpy(), b)


@pytest.mark.parametrize("f32_targets", [False, True], ids=["f64", "f32"])
def test_scratch_and_outputs_are_as_long_as_stated_and_wholly_written(f32_targets):
    """Inputs, scratch and outputs exactly as long as the header says, each between guard bands, the inputs registered
    read-only; scratch and outputs poisoned with each of FILLS give the same bytes (the scratch needs no initialisation, every
    output byte is written), no band and no input byte changes.  A = 525, nc = 80: 21 tiles of 25 rows per image, the last
    box workgroup of an image holds 13 anchors."""
    from event_representation_study_amd import _lib
    lib = _lib.load()
    c = cases.with_teacher(lcases.base(61, S=160, B=3, nc=80, n_fg=20), 261)
    if f32_targets:
        c["tb"], c["ts"] = c["tb"].astype(F32), c["ts"].astype(F32)
    B, A, nc, R, K = 3, 525, 80, 16, 17
    nbytes = int(lib.evrep_detloss_distill_workspace_bytes(B, A, nc))
    assert nbytes == 12800 + 3 * 256 + 2 * 512 + 4 * 256
    flags = _lib.DETLOSS_USE_DFL | (_lib.DETLOSS_F32_TARGETS if f32_targets else 0)
    kc, kd = cases.k_of(c)
    P = ctypes.c_void_p
    first = None

    def call(arena, fill, flags, with_grads=True):
        ins = {}
        for k in cases.KEYS:
            v = np.asarray(c[k])
            arena.carve_like(torch.from_numpy(v.view(np.uint8) if v.dtype == bool else v), name=k)
            ins[k] = arena.ptr()
        outs, ptrs = {}, {}
        shapes = (("losses", (8,), torch.float64), ("status", (B,), torch.int32))
        if with_grads:
            shapes += (("gs", (B, A, nc), torch.float32), ("gz", (B, A, 4 * K), torch.float32))
        for name, shape, dtype in shapes:
            outs[name] = arena.carve_shape(shape, dtype, fill=fill, name=name)
            ptrs[name] = arena.ptr()
        arena.carve(nbytes, fill=fill, name="scratch")
        _lib.check(lib.evrep_detloss_distill(P(ins["p"]), P(ins["z"]), P(ins["tp"]), P(ins["tz"]), P(ins["anc"]), P(ins["stride"]),
                                             P(ins["labels"]), P(ins["tb"]), P(ins["ts"]), P(ins["fg"]), B, A, nc, R, 1.0, 2.5, 0.5, c["T"], kc, kd,
                                             flags, P(ptrs["losses"]), P(ptrs["gs"]) if with_grads else None,
                                             P(ptrs["gz"]) if with_grads else None, P(ptrs["status"]), P(arena.ptr()),
                                             P(torch.cuda.current_stream().cuda_stream)), "evrep_detloss_distill")
        torch.cuda.synchronize()
        arena.check()
        arena.check_inputs()
        return {k: v.cpu().numpy() for k, v in outs.items()}
    for seed, fill in enumerate(FILLS):
        got = call(Arena(DEV, seed + 1), fill, flags)
        if first is None:
            first = got
            d = {}
            want = cases.host(c, d)
            check_against_bounds("guarded", got["losses"], got["gs"], got["gz"], want[0], d["gs"], d["gz"], cases.bounds(c, want[0], d),
                                 extra_rel=F32_ROUND)
            assert not got["status"].any()
        for k in got:
            assert_bit_equal(got[k], first[k], "fill %s %s" % (fill, k))
    quiet = call(Arena(DEV, 9), "ones", flags | _lib.DETLOSS_NO_GRAD, with_grads=False)   # NULL gradient pointers
    assert_bit_equal(quiet["losses"], first["losses"])


def test_channel_wise_scratch_and_outputs_are_as_long_as_stated_and_wholly_written():
    """Rows of 4096 (staged), 4097 (re-read) and 255 values, the maps, their gradients, out and the scratch between bands."""
    from event_representation_study_amd import _lib
    lib = _lib.load()
    c = cases.cw_case(62, [(64, 64), (1, 4097), (15, 17)], N=1, C=2)
    P = ctypes.c_void_p
    first = None
    for seed, fill in enumerate(FILLS):
        arena = Arena(DEV, seed + 1)
        lv = (_lib.CwdLevel * 3)()
        grads = []
        for l in range(3):
            arena.carve_like(torch.from_numpy(c["s"][l]), name="s%d" % l)
            lv[l].s = arena.ptr()
            arena.carve_like(torch.from_numpy(c["t"][l]), name="t%d" % l)
            lv[l].t = arena.ptr()
            grads.append(arena.carve_shape(c["s"][l].shape, torch.float32, fill=fill, name="g%d" % l))
            lv[l].grad_s = arena.ptr()
            lv[l].n, lv[l].c, lv[l].h, lv[l].w = c["s"][l].shape
        L = ctypes.cast(lv, ctypes.c_void_p)
        nbytes = int(lib.evrep_detloss_cwd_workspace_bytes(L, 3))
        assert nbytes == 256                                           # six rows
        out = arena.carve_shape((4,), torch.float64, fill=fill, name="out")
        op = arena.ptr()
        arena.carve(nbytes, fill=fill, name="scratch")
        _lib.check(lib.evrep_detloss_cwd(L, 3, 1.0, 0, P(op), P(arena.ptr()), P(torch.cuda.current_stream().cuda_stream)), "evrep_detloss_cwd")
        torch.cuda.synchronize()
        arena.check()
        arena.check_inputs()
        got = [out.cpu().numpy()] + [g.cpu().numpy() for g in grads]
        if first is None:
            first = got
            d = {}
            want, _ = cases.cw_host(c, d)
            check_cw_against_bounds("guarded", c, got[0], got[1:], dict(loss=want[0], levels=list(want[1:]), grads=d["g"]), d, extra_rel=F32_ROUND)
        for a, b in zip(got, first):
            assert_bit_equal(a, b, "fill %s" % fill)


def test_smoke_at_8400_anchors():
    c = cases.with_teacher(lcases.base(71, S=640, B=2, nc=80, n_fg=200), 271)
    d = {}
    want = cases.host(c, d)
    t = on_device(c)
    losses, gs, gz, status = entry(c, t)
    check_against_bounds("8400", losses, gs, gz, want[0], d["gs"], d["gz"], cases.bounds(c, want[0], d), extra_rel=F32_ROUND)
    assert losses[6] == 400 and not status.any() and c["p"].shape == (2, 8400, 80)
