"""-m gpu: the EST layer's backward (k_est_bwd / evrep_est_voxel_backward / EventBatch.est_voxel_backward) against the float64
restatement of tests/test_est_train_cpu.py -- bit for bit where the inputs make every product and sum exact, under the derived
summation bound elsewhere -- and est.TrainableQuantizationLayer end to end against the reference's own gradients
(tests/golden/est_grad.npz).  Every input is built and checked for exactness / selectivity on the CPU in test_est_train_cpu.py."""
import ctypes

import numpy as np
import pytest

from test_est_train_cpu import (EXACT_COUNTS, GENERAL, GOLDEN_GRAD, KEYS, assert_within_backward_bound, backward_selective_share,
                                err32_of, exact_case, general_case, loss_weights, rel_err, restate, state_of)

pytestmark = pytest.mark.gpu


def _backward(case):
    import torch
    from event_representation_study_amd import engine as eng
    eb = eng.EventBatch(torch.from_numpy(case.rows).cuda(), torch.from_numpy(case.offsets), case.H, case.W)
    seg = torch.from_numpy(case.table.seg).cuda()
    bucket = torch.from_numpy(np.ascontiguousarray(case.table.bucket, dtype=np.int32)).cuda()
    args = (torch.from_numpy(case.tn).cuda(), case.C, seg, bucket, case.table.lo, case.table.hi, torch.from_numpy(case.G).cuda())
    return eb, args, eb.est_voxel_backward(*args).cpu().numpy()


@pytest.mark.parametrize("layout", ["one_pixel", "own_piece"])
@pytest.mark.parametrize("n", EXACT_COUNTS)
def test_backward_is_bit_equal_on_exact_inputs(n, layout):
    """frame 5x7, B = 3 with an empty middle window, tn multiples of 2^-10, dyadic shifts, integer G: grad_seg equals the
    restatement bit for bit, untouched pieces hold +0.0.  1 .. three slices + 1 events; tables of 1, 2 and 300 pieces."""
    for C in (2, 3, 5):
        for nseg in (1, 2, 300):
            case = exact_case(n, C, nseg, layout)
            want = restate(case)
            got = _backward(case)[2]
            assert got.shape == (nseg, 2) and got.dtype == np.float64
            assert np.array_equal(got.view(np.uint64), (want.grad + 0.0).view(np.uint64)), (n, layout, C, nseg)
            assert not got[want.count == 0].any()


@pytest.mark.parametrize("kind,C", GENERAL)
def test_backward_within_the_summation_bound_and_deterministic(kind, C):
    """the 300-piece table, uniform / tied / descending times, C in {2, 8}: every piece within gamma(n_k + 2) * sum |terms| of the
    restatement, and a second call returns the same bits."""
    case = general_case(kind, C)
    r = restate(case)
    assert backward_selective_share(r) >= 0.99
    eb, args, got = _backward(case)
    print("backward bound used, %s C=%d: %.4f" % (kind, C, assert_within_backward_bound(got, r, "%s C=%d" % (kind, C))))
    again = eb.est_voxel_backward(*args).cpu().numpy()
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64))


def test_backward_refuses_bad_arguments_before_any_launch():
    import torch
    from event_representation_study_amd import _lib
    case = exact_case(65, 3, 2, "own_piece")
    lib = _lib.load()
    t = [torch.from_numpy(v).cuda() for v in (case.rows, case.offsets, case.tn, case.table.seg,
                                              np.ascontiguousarray(case.table.bucket, dtype=np.int32), case.G)]
    ev, off, tn, seg, bucket, G = t
    grad = torch.full((2, 2), 7.0, dtype=torch.float64, device="cuda")
    scratch = torch.zeros(lib.evrep_est_backward_scratch_bytes(65, 2), dtype=torch.uint8, device="cuda")
    p = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731

    def call(nseg=2, C=3, grad_out=p(G)):
        return lib.evrep_est_voxel_backward(p(ev), p(off), 3, case.H, case.W, p(tn), C, p(seg), nseg, p(bucket), bucket.numel(),
                                            -1.0, 1.0, grad_out, p(grad), p(scratch), None)
    assert call(nseg=_lib.EST_BWD_MAX_SEG + 1) == _lib.EVREP_EINVAL
    assert call(C=9) == _lib.EVREP_EINVAL
    assert call(grad_out=None) == _lib.EVREP_EINVAL
    torch.cuda.synchronize()
    assert bool((grad == 7.0).all())                       # nothing was launched: grad_seg is overwritten by every launch
    assert call() == _lib.EVREP_OK
    torch.cuda.synchronize()
    assert np.array_equal(grad.cpu().numpy(), restate(case).grad)


@pytest.fixture(scope="module")
def grad_golden():
    return np.load(GOLDEN_GRAD)


@pytest.mark.parametrize("size", [96, None])
def test_trainable_layer_end_to_end(grad_golden, size):
    """est.TrainableQuantizationLayer on the fixture: the output equals est.QuantizationLayer's bit for bit; after backward every
    weight gradient lies within 2 * err32 of the reference's float64 run (err32 = the reference's own float32 run against it;
    factor 2: both share the float32 rounding of u that the kernel mirrors, all it adds is float64 work); the events get no
    gradient and are left alone."""
    import torch
    from event_representation_study_amd import est
    g = grad_golden
    C, H, W = (int(v) for v in g["dim"])
    state = state_of(g)
    ev = g["events"].copy()
    events = torch.from_numpy(ev).requires_grad_(False)
    layer = est.TrainableQuantizationLayer((C, H, W), est.ValueLayer(state), image_size=size)
    out = layer(events)
    want = est.QuantizationLayer((C, H, W), est.ValueLayer(state), image_size=size)(torch.from_numpy(ev.copy()))
    assert out.dtype == torch.float32 and out.is_cuda and torch.equal(out, want)
    wt = torch.from_numpy(loss_weights(out.shape, g["seed"])).cuda()
    (wt * out).sum().backward()
    assert events.grad is None and np.array_equal(events.numpy(), g["events"])
    got = {k: p.grad.detach().cpu().numpy() for k, p in layer.value_layer.named_parameters()}
    assert all(got[k].shape == state[k].shape for k in KEYS)
    err = rel_err(got, {k: g["grad_f64_%d_%s" % (size or 0, k)] for k in KEYS})
    e32 = err32_of(g, size or 0)
    print("image_size %s: " % size + ", ".join("%s %.2e (err32 %.2e)" % (k, err[k], e32[k]) for k in KEYS))
    for k in KEYS:
        assert err[k] <= 2 * e32[k], (k, err[k], e32[k])
    # a second backward is not supported and says so: a gradient of the gradient needs an upstream gradient that is itself a variable
    wt2 = wt.clone().requires_grad_(True)
    (gr,) = torch.autograd.grad((wt2 * layer(events)).sum(), layer.value_layer.mlp[2].bias, create_graph=True)
    with pytest.raises(RuntimeError, match="differentiate twice"):
        gr.sum().backward()


def test_one_optimiser_step_lowers_the_loss(grad_golden):
    """One SGD step on the fixture loss (Wt * forward(events)).sum(), image_size 96: the weights change, the next forward uses a
    rebuilt table, the loss falls.  The step moves no weight by more than 1e-3 of the largest weight, so the first-order
    decrease lr * |grad|^2 governs; the loss is summed in float64 so that its own rounding stays far below that decrease."""
    import torch
    from event_representation_study_amd import est
    g = grad_golden
    C, H, W = (int(v) for v in g["dim"])
    events = torch.from_numpy(g["events"].copy())
    layer = est.TrainableQuantizationLayer((C, H, W), est.ValueLayer(state_of(g)), image_size=96)
    before = [p.detach().clone() for p in layer.parameters()]
    out = layer(events)
    wt = torch.from_numpy(loss_weights(out.shape, g["seed"])).cuda().double()
    loss0 = (wt * out.double()).sum()
    table0 = (layer.kernel.edges.copy(), layer.kernel.a.copy(), layer.kernel.c.copy())
    loss0.backward()
    gmax = max(float(p.grad.abs().max()) for p in layer.parameters())
    gsq = sum(float((p.grad.double() ** 2).sum()) for p in layer.parameters())
    lr = 1e-3 * max(float(p.abs().max()) for p in before) / gmax
    torch.optim.SGD(layer.parameters(), lr=lr).step()
    assert all(not torch.equal(b, p.detach()) for b, p in zip(before, layer.parameters()))
    with torch.no_grad():
        loss1 = (wt * layer(events).double()).sum()
    assert layer.kernel.edges.shape != table0[0].shape or not np.array_equal(layer.kernel.edges, table0[0])
    assert layer.kernel.a.shape != table0[1].shape or not np.array_equal(layer.kernel.a, table0[1])
    print("loss %.9e -> %.9e, first-order estimate of the decrease %.3e" % (float(loss0.detach()), float(loss1), lr * gsq))
    assert float(loss1) < float(loss0.detach())
