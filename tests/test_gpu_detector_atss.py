"""GPU: the ATSS assigner of the warm-up epochs (csrc/evrep_atss.hip through detector_assign._atss_device / atss_assign_batch /
ATSSAssigner and ComputeLoss(warmup_assigner="atss")) against the host restatement atss_host BIT FOR BIT -- labels, boxes,
scores, fg, status, in both storage widths of boxes and scores -- and against the golden recorded from the reference's own
ATSSAssigner.forward.  No tolerance anywhere: device and host perform the same float64 statements.

Shapes: the select launch streams a level's anchors in chunks of 256 and merges into a list of topk <= 32; levels of 9 (exactly
topk), 256, 257 and 289 anchors; one level and five; topk 1, 9, 32; M on both sides of 1 and up to 101; B 1..3; 8400 anchors
once, in the golden."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

from conftest import assert_bit_equal
import detector_assign_cases as tal_cases
from guarded import FILLS, Arena
from test_detector_atss_cpu import HAND, _case, _loss_inputs, golden_case, golden_names, host

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, F64 = np.float32, np.float64
WIDTHS = ((torch.float64, torch.float32), (torch.float32, torch.float64), (torch.float64, torch.float64), (torch.float32, torch.float32))
NP = {torch.float64: F64, torch.float32: F32}
NAMES = ("labels", "boxes", "scores", "fg", "status")


def _da():
    from event_representation_study_amd import detector_assign
    return detector_assign


def device(c, boxes_dtype=torch.float64, scores_dtype=torch.float32):
    t = lambda v: None if v is None else torch.from_numpy(v).to(DEV)
    out = _da()._atss_device(t(c["anchors"]), c["counts"], t(c["gt"]), t(c["pd"]), c["nc"], c["topk"], boxes_dtype, scores_dtype)
    torch.cuda.synchronize()
    labels, tb, ts, fg, status = (o.cpu().numpy() for o in out)
    return labels, tb, ts, fg.astype(bool), status.view(np.uint32)


def check(c, what=""):
    """Device == atss_host on all five, in the four pairs of storage widths, the first pair twice; returns the host results in
    the reference's widths."""
    first = None
    for i, (bd, sd) in enumerate(WIDTHS):
        want = host(c, boxes_dtype=NP[bd], scores_dtype=NP[sd])
        for rep in range(2 if i == 0 else 1):
            got = device(c, bd, sd)
            for g, w, name in zip(got, want, NAMES):
                assert_bit_equal(g, w, "%s %s/%s %s call %d" % (what, NP[bd].__name__, NP[sd].__name__, name, rep))
        first = first or want
    return first


@pytest.mark.parametrize("name", golden_names())
def test_device_equals_the_reference_and_the_host(name):
    g, pd, (H, W), B, nc = golden_case(name)
    c = dict(anchors=g[name + "/anchors"], counts=g[name + "/levels"].tolist(), gt=g[name + "/gt"], pd=pd, nc=nc, topk=9)
    labels, boxes, scores, fg, status = check(c, name)
    for got, key in zip((labels, boxes, scores, fg), NAMES):
        assert_bit_equal(got, g[name + "/" + key], name + " " + key)
    assert not status.any()


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_built_cases_on_the_device(name):
    check(HAND[name](), name)


@pytest.mark.parametrize("M", [1, 2, 17])
def test_padded_rows_and_label_counts(M):
    """Rows of padding behind, and between, the labels; the image without labels has none but padding."""
    da = _da()
    anchors, counts = da.anchor_boxes(96)
    t = tal_cases.targets(900 + M, [M, 0, min(M, 2)], 2, lo=0.15, hi=0.7)
    gt = da.preprocess_host(t, 3, 96, 96, max_labels=M + 3)[0]
    gt[0, [0, M]] = gt[0, [M, 0]]                                        # row 0 is padding: background carries ITS box
    out = check(_case(anchors, counts, gt, pd_seed=900 + M), "M %d" % M)
    assert out[3][0].any() and not out[3][1].any() and out[3][2].any() and not out[1][0][~out[3][0]].any()


# ------------------------------------------------------------------------------------------------------------ the public routes
def test_both_python_entries_agree_with_the_host():
    da = _da()
    name = "rect_96x160"
    g, pd, (H, W), B, nc = golden_case(name)
    targets = g[name + "/targets"]
    anchors, counts = da.anchor_boxes((H, W))
    a, p = torch.from_numpy(anchors).to(DEV), torch.from_numpy(pd).to(DEV)
    M = g[name + "/gt"].shape[1]
    for t, kw, m in ((torch.from_numpy(targets), {}, M), (torch.from_numpy(targets).to(DEV), dict(max_labels=M + 2), M + 2)):
        gt_h = da.preprocess_host(targets, B, W, H, max_labels=m)[0]
        for dt in (torch.float64, torch.float32):
            want = da.atss_host(anchors, counts, gt_h, pd, 9, nc, boxes_dtype=NP[dt], scores_dtype=NP[dt])
            labels, tb, ts, fg, status = da.atss_assign_batch(a, counts, p, t, (H, W), nc, out_dtype=dt, check=True, **kw)
            assert labels.is_cuda and labels.dtype == torch.int64 and fg.dtype == torch.bool and tb.dtype == ts.dtype == dt
            assert status.tolist() == [0] * B
            for got, w in zip((labels, tb, ts, fg), want):
                assert_bit_equal(got.cpu().numpy(), w)
    assert_bit_equal(labels.cpu().numpy(), g[name + "/labels"])
    # the drop-in class on CUDA tensors
    gt = torch.from_numpy(g[name + "/gt"]).to(DEV)
    atss = da.ATSSAssigner(9, num_classes=nc)
    out = atss(a, counts, gt[:, :, :1], gt[:, :, 1:], (gt[:, :, 1:].sum(-1, keepdim=True) > 0).float(), p)
    assert [o.dtype for o in out] == [torch.int64, torch.float64, torch.float32, torch.bool] and all(o.is_cuda for o in out)
    assert atss.last_status.tolist() == [0] * B
    for o, key in zip(out, NAMES):
        assert_bit_equal(o.cpu().numpy(), g[name + "/" + key], key)
    none = atss(a, counts, gt[:, :, :1], gt[:, :, 1:], None, None)
    assert set(none[2].unique().tolist()) == {0.0, 1.0} and torch.equal(none[3], out[3])
    # the refusals of the device route
    with pytest.raises(ValueError, match="max_labels"):
        da.atss_assign_batch(a, counts, p, torch.from_numpy(targets).to(DEV), (H, W), nc)
    with pytest.raises(ValueError, match="image 1: more labels than max_labels"):
        da.atss_assign_batch(a, counts, p, torch.from_numpy(targets), (H, W), nc, max_labels=M - 1, check=True)
    with pytest.raises(ValueError, match="add up"):
        da.atss_assign_batch(a, [240, 60, 14], p, torch.from_numpy(targets), (H, W), nc)
    with pytest.raises(ValueError, match="below topk"):
        da.atss_assign_batch(a, counts, p, torch.from_numpy(targets), (H, W), nc, topk=16)
    with pytest.raises(ValueError, match=r"\.float\(\)"):
        da.atss_assign_batch(a, counts, p.double(), torch.from_numpy(targets), (H, W), nc)


def test_capture_and_replay():
    da = _da()
    B, S, nc = 3, 96, 2
    import detector_atss_cases as cases
    anchors, counts = da.anchor_boxes(S)
    pd1, pd2 = cases.pred_boxes(1100, B, S), cases.pred_boxes(1101, B, S)
    t1, t2 = tal_cases.targets(1102, [4, 0, 5], nc, lo=0.2, hi=0.7), tal_cases.targets(1103, [2, 5, 2], nc, lo=0.2, hi=0.7)
    assert t1.shape == t2.shape
    a, p, t = (torch.from_numpy(v).to(DEV) for v in (anchors, pd1, t1))
    eager = da.atss_assign_batch(a, counts, p, t, (S, S), nc, max_labels=5)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = da.atss_assign_batch(a, counts, p, t, (S, S), nc, max_labels=5)
    p.copy_(torch.from_numpy(pd2)); t.copy_(torch.from_numpy(t2))
    graph.replay()
    torch.cuda.synchronize()
    want = da.atss_host(anchors, counts, da.preprocess_host(t2, B, S, S, max_labels=5)[0], pd2, 9, nc, scores_dtype=F64)
    assert want[3].any(1).all()
    for g, w, name in zip(out[:4], want, NAMES):
        assert_bit_equal(g.cpu().numpy(), w, "replay on new contents: " + name)
    p.copy_(torch.from_numpy(pd1)); t.copy_(torch.from_numpy(t1))
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(out, eager)), "the same bytes as the eager call"


# ------------------------------------------------------------------------------------------------------ the size contracts
@pytest.mark.parametrize("widths", [0, 1, 2, 3], ids=["f64_f64", "f32_boxes", "f32_scores", "f32_f32"])
def test_scratch_and_outputs_are_as_long_as_stated_and_wholly_written(widths):
    """Inputs, scratch and outputs exactly as long as the header says, each between guard bands, the inputs registered
    read-only; scratch and outputs poisoned with zeros, 0xFF and random bytes give the same bytes (the scratch needs no
    initialisation, every output byte is written), no band and no input byte changes.  B * A = 567: no array of the scratch
    fills its last 256-byte slot."""
    from event_representation_study_amd import _lib
    da = _da()
    lib = _lib.load()
    B, S, nc, M = 3, 96, 3, 6
    import detector_atss_cases as cases
    anchors, counts = da.anchor_boxes(S)
    pd = cases.pred_boxes(1200, B, S)
    gt = da.preprocess_host(tal_cases.targets(1201, [6, 0, 3], nc, lo=0.2, hi=0.8), B, S, S, max_labels=M)[0]
    A = len(anchors)
    bdt, sdt = (torch.float32 if widths & 1 else torch.float64), (torch.float32 if widths & 2 else torch.float64)
    want = da.atss_host(anchors, counts, gt, pd, 9, nc, boxes_dtype=NP[bdt], scores_dtype=NP[sdt])
    assert want[3].any()
    nbytes = int(lib.evrep_atss_workspace_bytes(B, M, A))
    assert A == 189 and nbytes == 3 * 2304 + 4608
    P = ctypes.c_void_p
    level_counts = (ctypes.c_int32 * 3)(*counts)
    for seed, fill in tuple((1, f) for f in FILLS) + ((2, "random"),):
        arena = Arena(DEV, seed)
        ins = {}
        for name, v in (("anchors", anchors), ("gt", gt), ("pd", pd)):
            arena.carve_like(torch.from_numpy(v), name=name)
            ins[name] = arena.ptr()
        outs, ptrs = {}, {}
        for name, shape, dtype in (("labels", (B, A), torch.int64), ("tb", (B, A, 4), bdt), ("ts", (B, A, nc), sdt),
                                   ("fg", (B, A), torch.uint8), ("status", (B,), torch.int32)):
            outs[name] = arena.carve_shape(shape, dtype, fill=fill, name=name)
            ptrs[name] = arena.ptr()
        arena.carve(nbytes, fill=fill, name="scratch")
        scratch = arena.ptr()
        stream = P(torch.cuda.current_stream().cuda_stream)
        _lib.check(lib.evrep_atss_assign(P(ins["anchors"]), level_counts, 3, P(ins["gt"]), P(ins["pd"]), B, M, A, nc, 9, widths,
                                         P(ptrs["labels"]), P(ptrs["tb"]), P(ptrs["ts"]), P(ptrs["fg"]), P(ptrs["status"]), P(scratch),
                                         stream), "evrep_atss_assign")
        torch.cuda.synchronize()
        arena.check()
        arena.check_inputs()
        what = "seed %d fill %s " % (seed, fill)
        for name, w in zip(("labels", "tb", "ts"), want):
            assert_bit_equal(outs[name].cpu().numpy(), w, what + name)
        assert_bit_equal(outs["fg"].cpu().numpy().astype(bool), want[3], what + "fg")
        assert outs["fg"].max().item() == 1, "fg is 0 or 1"
        assert_bit_equal(outs["status"].cpu().numpy().view(np.uint32), want[4], what + "status")


# --------------------------------------------------------------------------------------------------------------- ComputeLoss
def test_compute_loss_warms_up_with_atss_on_the_device():
    from event_representation_study_amd import detector_loss as dl
    da = _da()
    B, S, nc = 3, 160, 2
    feats, p, z = _loss_inputs(81, B, S, nc)
    feats, p, z = [f.to(DEV) for f in feats], p.to(DEV), z.to(DEV)
    targets_h = tal_cases.targets(82, [4, 0, 6], nc, lo=0.2, hi=0.7)
    targets = torch.from_numpy(targets_h).to(DEV)
    crit = dl.ComputeLoss(num_classes=nc, ori_img_size=S, warmup_assigner="atss", max_labels=6)
    p.requires_grad_(True)
    z.requires_grad_(True)
    crit((feats, p, z), targets, 4, 0, S, S)                             # (the anchors are cached, the scratch is allocated)
    crit((feats, p, z), targets, 0, 0, S, S)
    torch.cuda.synchronize()
    # no read of device data on the host: what epoch 4 passes under the sync check, epoch 0 passes too
    mode = torch.cuda.get_sync_debug_mode()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                 # (torch calls the mode a prototype)
        torch.cuda.set_sync_debug_mode("error")
    try:
        late, _ = crit((feats, p, z), targets, 4, 0, S, S)
        loss, items = crit((feats, p, z), targets, 0, 0, S, S)
        status = crit.last_status
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    loss.backward()
    assert status.tolist() == [0, 0, 0] and late.item() != loss.item()
    anchors, anc, n_list, stride = crit.anchors(feats, p.device)
    assert_bit_equal(anchors.cpu().numpy(), da.anchor_boxes(S)[0])
    assert n_list == [400, 100, 25]
    _, boxes_px = dl.decode_boxes(z, anc, stride)
    labels, tb, ts, fg, st = da.atss_assign_batch(anchors, n_list, boxes_px, targets, (S, S), nc, max_labels=6)
    assert fg[0].any().item() and not fg[1].any().item() and fg[2].any().item() and tb.dtype == ts.dtype == torch.float64
    p2, z2 = p.detach().clone().requires_grad_(True), z.detach().clone().requires_grad_(True)
    loss2, items2 = dl.loss_batch(p2, z2, anc, stride, labels, tb, ts, fg, nc)
    loss2.backward()
    assert torch.equal(loss.detach(), loss2.detach()) and torch.equal(items, items2)
    assert torch.equal(p.grad, p2.grad) and torch.equal(z.grad, z2.grad)
    # the targets are the host's
    gt = da.preprocess_host(targets_h, B, S, S, max_labels=6)[0]
    want = da.atss_host(anchors.cpu().numpy(), n_list, gt, boxes_px.cpu().numpy(), 9, nc, scores_dtype=F64)
    for got, w in zip((labels, tb, ts, fg), want):
        assert_bit_equal(got.cpu().numpy(), w)
    # an instance of the class takes the same route; CPU targets count their labels on the host
    crit2 = dl.ComputeLoss(num_classes=nc, ori_img_size=S, warmup_assigner=da.ATSSAssigner(9, num_classes=nc))
    loss3, items3 = crit2((feats, p, z), torch.from_numpy(targets_h), 0, 0, S, S)
    assert torch.equal(loss3.detach(), loss.detach()) and torch.equal(items3, items)
    # the default still says what is missing
    with pytest.raises(NotImplementedError, match="ATSSAssigner"):
        dl.ComputeLoss(num_classes=nc)((feats, p, z), targets, 0, 0, S, S)
