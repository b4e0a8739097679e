"""GPU: the loss terms and their gradients (csrc/evrep_detloss.hip through the C entry, detector_loss.loss_batch,
decode_boxes and ComputeLoss) against the host restatement loss_host within the DERIVED bound of tests/detector_loss_cases.py
plus one float32 rounding for the stored gradients, and against the golden recorded from the reference's own VarifocalLoss /
BboxLoss / bbox_decode within four times its MEASURED float32 rounding.

Shapes: A = 84 (S = 64: less than one workgroup, three levels) and A = 525 (S = 160: three workgroups per image, the last one
of 13 anchors); B in {1, 3}; nc in {1, 2, 80}; R = 16, and R = 0 without DFL; one smoke case at 8400 anchors."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import assert_bit_equal, load_golden
import detector_assign_cases as acases
import detector_loss_cases as cases
from guarded import FILLS, Arena
from test_detector_loss_cpu import check_against_bounds, check_against_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, F64 = np.float32, np.float64
KEYS = ("p", "z", "anc", "stride", "labels", "tb", "ts", "fg")
F32_ROUND = 2.0 ** -24


def _dl():
    from event_representation_study_amd import detector_loss
    return detector_loss


def on_device(c):
    return {k: torch.from_numpy(np.asarray(c[k])).to(DEV) for k in KEYS}


def entry(c, t, grad=True):
    """The C entry through the package's thin wrapper: (losses (5,), grad_scores, grad_distri, status) as numpy."""
    K = c["R"] + 1 if c["use_dfl"] else 1
    out = _dl()._loss_device(t["p"], t["z"], t["anc"], t["stride"], t["labels"], t["tb"], t["ts"], t["fg"], c["R"], K, c["use_dfl"],
                             c["weights"], grad)
    torch.cuda.synchronize()
    return tuple(None if o is None else o.cpu().numpy() for o in out)


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_every_case_on_the_device(name):
    dl = _dl()
    c = cases.CASES[name]()
    d = {}
    want, gs_h, gz_h, st_h = cases.host(c, d)
    bd = cases.bounds(c, want, d)
    t = on_device(c)
    # the C entry
    losses, gs, gz, status = entry(c, t)
    assert gs.dtype == F32 and gz.dtype == F32 and losses.dtype == F64
    check_against_bounds(name + " [entry]", c, losses, gs, gz, want, d["gs"], d["gz"], bd, extra_rel=F32_ROUND)
    assert losses[3] == pytest.approx(want[3], rel=286 * cases.U, abs=0) and losses[4] == want[4]
    assert_bit_equal(status.view(np.uint32), st_h, name + " status")
    if not c["fg"].any():
        assert losses[1] == 0 and losses[2] == 0 and not gz.any()
    assert not gz[~c["fg"]].any(), "background rows of grad_distri are zeros"
    again = entry(c, t)
    for a, b in zip((losses, gs, gz, status), again):
        assert_bit_equal(a, b, name + ": two calls give equal bits")
    quiet = entry(c, t, grad=False)
    assert quiet[1] is None and quiet[2] is None
    assert_bit_equal(quiet[0], losses, name + ": NO_GRAD gives the same losses")
    # loss_batch, autograd
    p, z = t["p"].clone().requires_grad_(True), t["z"].clone().requires_grad_(True)
    loss, items, st = dl.loss_batch(p, z, t["anc"], t["stride"], t["labels"], t["tb"], t["ts"], t["fg"], c["nc"], c["R"], c["use_dfl"],
                                    return_status=True)
    assert loss.is_cuda and loss.dtype == torch.float64 and loss.dim() == 0 and items.dtype == torch.float64
    wc, wi, wd = c["weights"]
    assert loss.item() == (losses[0] * wc + losses[1] * wi) + losses[2] * wd
    assert items.tolist() == [losses[1] * wi, losses[2] * wd, losses[0] * wc]
    loss.backward()
    assert_bit_equal(p.grad.cpu().numpy(), gs, name + ": loss_batch's grad_scores are the entry's")
    assert_bit_equal(z.grad.cpu().numpy(), gz, name + ": loss_batch's grad_distri are the entry's")
    assert_bit_equal(st.cpu().numpy().view(np.uint32), st_h)
    with torch.no_grad():
        quiet_loss, _ = dl.loss_batch(p, z, t["anc"], t["stride"], t["labels"], t["tb"], t["ts"], t["fg"], c["nc"], c["R"], c["use_dfl"])
    assert not quiet_loss.requires_grad and quiet_loss.item() == loss.item()
    # decode_boxes: the float64 box rounded once
    K = c["R"] + 1 if c["use_dfl"] else 1
    boxes_s, boxes_px = (o.cpu().numpy() for o in dl.decode_boxes(t["z"], t["anc"], t["stride"], c["R"], c["use_dfl"]))
    box = d["box"]
    slack = 12 * K * cases.U * np.abs(box).max(-1, keepdims=True)      # the expectation's last places (detector_loss_cases.py)
    assert (np.abs(boxes_s.astype(F64) - box) <= F32_ROUND * np.abs(box) + slack).all()
    px = box * c["stride"].astype(F64)[None, :, None]
    assert (np.abs(boxes_px.astype(F64) - px) <= F32_ROUND * np.abs(px) + slack * 32).all()
    # the reference's own results
    if name in cases.GOLDEN:
        check_against_golden(name, c, load_golden("detector_loss"), losses, gs, gz, boxes_s)


def test_backward_scales_by_the_upstream_gradient():
    dl = _dl()
    c = cases.plain_nc2()
    t = on_device(c)
    _, gs, gz, _ = entry(c, t)
    p, z = t["p"].clone().requires_grad_(True), t["z"].clone().requires_grad_(True)
    loss, _ = dl.loss_batch(p, z, t["anc"], t["stride"], t["labels"], t["tb"], t["ts"], t["fg"], 2)
    (loss * 3.0).backward()
    assert_bit_equal(p.grad.cpu().numpy(), gs * F32(3))
    assert_bit_equal(z.grad.cpu().numpy(), gz * F32(3))
    # only one prediction needs a gradient
    p2 = t["p"].clone().requires_grad_(True)
    loss2, _ = dl.loss_batch(p2, t["z"], t["anc"], t["stride"], t["labels"], t["tb"], t["ts"], t["fg"], 2)
    loss2.backward()
    assert_bit_equal(p2.grad.cpu().numpy(), gs)


def _head(seed, B, S, nc):
    c = cases.base(seed, S=S, B=B, nc=nc)
    rng = np.random.default_rng(seed)
    feats = [torch.zeros((B, 1, S // s, S // s), device=DEV) for s in (8, 16, 32)]
    p = torch.from_numpy(rng.uniform(0.05, 0.95, c["p"].shape).astype(F32)).to(DEV)
    return feats, p, torch.from_numpy(c["z"]).to(DEV), c


def test_loss_batch_after_assign_batch_is_compute_loss():
    from event_representation_study_amd import detector_assign as da
    dl = _dl()
    B, S, nc = 3, 160, 2
    feats, p, z, c = _head(41, B, S, nc)
    targets = torch.from_numpy(acases.targets(42, [4, 0, 6], nc, lo=0.2, hi=0.7))
    crit = dl.ComputeLoss(num_classes=nc, ori_img_size=S)
    p.requires_grad_(True)
    z.requires_grad_(True)
    loss, items = crit((feats, p, z), targets, 4, 0, S, S)
    loss.backward()
    anc, stride = (torch.from_numpy(v).to(DEV) for v in da.anchor_points(S))
    boxes_s, boxes_px = dl.decode_boxes(z, anc, stride)
    labels, tb, ts, fg, st = da.assign_batch(p, boxes_px, anc, targets, (S, S), nc)
    assert fg.any().item() and not fg[1].any().item()
    p2, z2 = p.detach().clone().requires_grad_(True), z.detach().clone().requires_grad_(True)
    loss2, items2 = dl.loss_batch(p2, z2, anc, stride, labels, tb, ts, fg, nc)
    loss2.backward()
    assert torch.equal(loss.detach(), loss2.detach()) and torch.equal(items, items2)
    assert torch.equal(p.grad, p2.grad) and torch.equal(z.grad, z2.grad) and crit.last_status.tolist() == [0, 0, 0]
    # against the host routes on the same inputs
    gt = da.preprocess_host(targets.numpy(), B, S, S)[0]
    hl, hb, hs, hf, _ = da.tal_host(p.detach().cpu().numpy(), boxes_px.cpu().numpy(), anc.cpu().numpy(), gt)
    assert_bit_equal(fg.cpu().numpy(), hf)
    d = {}
    want = dl.loss_host(p.detach().cpu().numpy(), z.detach().cpu().numpy(), anc.cpu().numpy(), stride.cpu().numpy(), hl, hb, hs, hf, details=d)[0]
    host_loss = (want[0] * 1.0 + want[1] * 2.5) + want[2] * 0.5
    assert loss.item() == pytest.approx(host_loss, rel=1e-12, abs=0)
    # empty targets through ComputeLoss: M = 0
    empty, items0 = crit((feats, p, z), torch.zeros((0, 6)), 4, 0, S, S)
    assert items0[0].item() == 0 and items0[1].item() == 0 and empty.item() == items0[2].item() > 0
    p.grad = z.grad = None
    empty.backward()
    assert not z.grad.any().item() and p.grad.any().item()
    # CUDA targets need max_labels, as in assign_batch
    dev_targets = targets.to(DEV)
    with pytest.raises(ValueError, match="max_labels"):
        crit((feats, p, z), dev_targets, 4, 0, S, S)
    loss3, _ = dl.ComputeLoss(num_classes=nc, max_labels=6)((feats, p, z), dev_targets, 4, 0, S, S)
    assert torch.equal(loss3.detach(), loss.detach())
    with pytest.raises(NotImplementedError, match="ATSSAssigner"):
        crit((feats, p, z), targets, 0, 0, S, S)
    with pytest.raises(ValueError, match=r"\.float\(\)"):
        crit((feats, p.double(), z), targets, 4, 0, S, S)


def test_capture_and_replay():
    dl = _dl()
    c1, c2 = cases.base(51, S=64, B=3, nc=2, n_fg=7), cases.base(52, S=64, B=3, nc=2, n_fg=4)
    t = on_device(c1)
    eager = entry(c1, t)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with torch.no_grad():
            boxes = dl.decode_boxes(t["z"], t["anc"], t["stride"])
        out = dl._loss_device(t["p"], t["z"], t["anc"], t["stride"], t["labels"], t["tb"], t["ts"], t["fg"], 16, 17, True, cases.WEIGHTS, True)
    for k in ("p", "z", "labels", "tb", "ts", "fg"):
        t[k].copy_(torch.from_numpy(c2[k]))
    graph.replay()
    torch.cuda.synchronize()
    d = {}
    want = cases.host(c2, d)
    bd = cases.bounds(c2, want[0], d)
    got = [o.cpu().numpy() for o in out]
    check_against_bounds("replay on new contents", c2, got[0], got[1], got[2], want[0], d["gs"], d["gz"], bd, extra_rel=F32_ROUND)
    assert np.abs(boxes[0].cpu().numpy() - d["box"]).max() < 1e-5
    for k in ("p", "z", "labels", "tb", "ts", "fg"):
        t[k].copy_(torch.from_numpy(c1[k]))
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(out, eager):
        assert_bit_equal(a.cpu().numpy(), b, "the same bytes as the eager call")


@pytest.mark.parametrize("f32_targets", [False, True], ids=["f64", "f32"])
def test_scratch_and_outputs_are_as_long_as_stated_and_wholly_written(f32_targets):
    """Inputs, scratch and outputs exactly as long as the header says, each between guard bands, the inputs registered
    read-only; scratch and outputs poisoned with zeros, 0xFF and random bytes give the same bytes (the scratch needs no
    initialisation, every output byte is written), no band and no input byte changes.  A = 525: the last workgroup of an image
    holds 13 anchors; B * A = 1575 fills no 256-byte slot of the scratch."""
    from event_representation_study_amd import _lib
    lib = _lib.load()
    c = cases.base(61, S=160, B=3, nc=2, n_fg=20)
    if f32_targets:
        c["tb"], c["ts"] = c["tb"].astype(F32), c["ts"].astype(F32)
    B, A, nc, R, K = 3, 525, 2, 16, 17
    nbytes = int(lib.evrep_detloss_workspace_bytes(B, A, nc))
    assert nbytes == 12800 + 256 + 256 + 3 * 256
    flags = _lib.DETLOSS_USE_DFL | (_lib.DETLOSS_F32_TARGETS if f32_targets else 0)
    P = ctypes.c_void_p
    first = None
    for seed, fill in tuple((1, f) for f in FILLS) + ((2, "random"),):
        arena = Arena(DEV, seed)
        ins = {}
        for k in KEYS:
            v = np.asarray(c[k])
            arena.carve_like(torch.from_numpy(v.view(np.uint8) if v.dtype == bool else v), name=k)
            ins[k] = arena.ptr()
        outs, ptrs = {}, {}
        for name, shape, dtype in (("losses", (5,), torch.float64), ("gs", (B, A, nc), torch.float32), ("gz", (B, A, 4 * K), torch.float32),
                                   ("status", (B,), torch.int32), ("boxes_s", (B, A, 4), torch.float32), ("boxes_px", (B, A, 4), torch.float32)):
            outs[name] = arena.carve_shape(shape, dtype, fill=fill, name=name)
            ptrs[name] = arena.ptr()
        arena.carve(nbytes, fill=fill, name="scratch")
        scratch = arena.ptr()
        stream = P(torch.cuda.current_stream().cuda_stream)
        _lib.check(lib.evrep_detloss_decode(P(ins["z"]), P(ins["anc"]), P(ins["stride"]), B, A, R, _lib.DETLOSS_USE_DFL, P(ptrs["boxes_s"]),
                                            P(ptrs["boxes_px"]), stream), "evrep_detloss_decode")
        _lib.check(lib.evrep_detloss(P(ins["p"]), P(ins["z"]), P(ins["anc"]), P(ins["stride"]), P(ins["labels"]), P(ins["tb"]), P(ins["ts"]),
                                     P(ins["fg"]), B, A, nc, R, 1.0, 2.5, 0.5, flags, P(ptrs["losses"]), P(ptrs["gs"]), P(ptrs["gz"]),
                                     P(ptrs["status"]), P(scratch), stream), "evrep_detloss")
        torch.cuda.synchronize()
        arena.check()
        arena.check_inputs()
        got = {k: v.cpu().numpy() for k, v in outs.items()}
        if first is None:
            first = got
            d = {}
            want = cases.host(c, d)
            bd = cases.bounds(c, want[0], d)
            check_against_bounds("guarded", c, got["losses"], got["gs"], got["gz"], want[0], d["gs"], d["gz"], bd, extra_rel=F32_ROUND)
            assert not got["status"].any() and np.abs(got["boxes_s"] - d["box"]).max() < 1e-5
        for k in got:
            assert_bit_equal(got[k], first[k], "seed %d fill %s %s" % (seed, fill, k))
    # NO_GRAD with NULL gradient pointers: the same losses
    arena = Arena(DEV, 3)
    ins = {}
    for k in KEYS:
        v = np.asarray(c[k])
        arena.carve_like(torch.from_numpy(v.view(np.uint8) if v.dtype == bool else v), name=k)
        ins[k] = arena.ptr()
    losses = arena.carve_shape((5,), torch.float64, fill="ones", name="losses")
    lp = arena.ptr()
    status = arena.carve_shape((B,), torch.int32, fill="ones", name="status")
    sp = arena.ptr()
    arena.carve(nbytes, fill="ones", name="scratch")
    _lib.check(lib.evrep_detloss(P(ins["p"]), P(ins["z"]), P(ins["anc"]), P(ins["stride"]), P(ins["labels"]), P(ins["tb"]), P(ins["ts"]),
                                 P(ins["fg"]), B, A, nc, R, 1.0, 2.5, 0.5, flags | _lib.DETLOSS_NO_GRAD, P(lp), None, None, P(sp),
                                 P(arena.ptr()), P(torch.cuda.current_stream().cuda_stream)), "evrep_detloss")
    torch.cuda.synchronize()
    arena.check()
    arena.check_inputs()
    assert_bit_equal(losses.cpu().numpy(), first["losses"])
    assert not status.any().item()


def test_smoke_at_8400_anchors():
    c = cases.base(71, S=640, B=2, nc=80, n_fg=200)
    d = {}
    want = cases.host(c, d)
    bd = cases.bounds(c, want[0], d)
    t = on_device(c)
    losses, gs, gz, status = entry(c, t)
    check_against_bounds("8400", c, losses, gs, gz, want[0], d["gs"], d["gz"], bd, extra_rel=F32_ROUND)
    assert losses[4] == 400 and not status.any() and c["p"].shape == (2, 8400, 80)
