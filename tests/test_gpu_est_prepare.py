"""-m gpu: the EST layer's event preparation on the device (k_est_prep_scan / k_est_prep_write / evrep_est_prepare /
engine.est_prepare / est.prepare_events_device) against the restatement of tests/test_est_cpu.py, bit for bit, and the two layers
with a CUDA input against the same layers with the host input.  Every stream is built and checked on the CPU in
test_est_prepare_cpu.py."""
import ctypes

import numpy as np
import pytest

from conftest import assert_bit_equal
from test_est_cpu import GOLDEN_EST, WRAPPER_KINDS, _weights, wrapper_events
from test_est_prepare_cpu import BAD, GOOD, H, W, bad_stream, good_stream, nan_equal_bits, restated
from test_est_train_cpu import GOLDEN_GRAD, KEYS, loss_weights, state_of

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _prepare(ev, bs):
    import torch
    from event_representation_study_amd import est
    batch, tn = est.prepare_events_device(torch.from_numpy(ev).to(DEV), H, W, DEV, batch_size=bs)
    assert batch.events.is_cuda and tn.is_cuda and batch.offsets.is_cuda
    return batch.events.cpu().numpy(), batch.offsets_host.numpy(), tn.cpu().numpy(), batch.offsets.cpu().numpy()


def _assert_restated(ev, bs, what):
    with np.errstate(all="ignore"):
        rows, offs, tn = restated(ev, bs)
    grows, goffs, gtn, goffs_dev = _prepare(ev, bs)
    assert_bit_equal(grows, rows, what + " rows")
    assert_bit_equal(goffs, offs, what + " offsets")
    assert_bit_equal(goffs_dev, offs, what + " offsets (device)")
    nan_equal_bits(gtn, tn, what + " tnorm")


@pytest.mark.parametrize("name", GOOD)
def test_prepare_is_bit_equal_to_the_restatement(name):
    ev, bs = good_stream(name)
    _assert_restated(ev, bs, name)


@pytest.mark.parametrize("name", BAD)
def test_prepare_refuses_and_the_status_is_not_sticky(name):
    import torch
    from event_representation_study_amd import est
    ev, bs, exc = bad_stream(name)
    with pytest.raises(exc):
        est.prepare_events_device(torch.from_numpy(ev).to(DEV), H, W, DEV, batch_size=bs)
    good, gbs = good_stream("edge_lengths_on_edges")
    _assert_restated(good, gbs, "after " + name)


def test_prepare_refuses_shapes_and_other_devices():
    import torch
    from event_representation_study_amd import est
    for t in (torch.zeros((0, 5)), torch.zeros((7, 4)), torch.zeros(5)):
        with pytest.raises(ValueError):
            est.prepare_events_device(t.to(DEV), H, W, DEV)
    with pytest.raises(ValueError):
        est.prepare_events_device(torch.zeros((3, 5)), H, W, DEV)               # a host tensor is the dispatcher's business


def test_prepare_converts_other_dtypes_and_strides_without_touching_them():
    import torch
    from event_representation_study_amd import est
    ev, _ = good_stream("single_event")
    with np.errstate(all="ignore"):
        rows, offs, tn = restated(ev)
    wide = torch.zeros((len(ev), 7), dtype=torch.float64, device=DEV)
    wide[:, 1:6] = torch.from_numpy(ev).to(DEV)
    view, keep = wide[:, 1:6], wide.clone()
    batch, gtn = est.prepare_events_device(view, H, W, DEV)
    assert torch.equal(wide, keep)
    assert_bit_equal(batch.events.cpu().numpy(), rows, "rows")
    assert_bit_equal(batch.offsets_host.numpy(), offs, "offsets")
    nan_equal_bits(gtn.cpu().numpy(), tn, "tnorm")


@pytest.mark.parametrize("kind", WRAPPER_KINDS)
def test_quantization_layer_cuda_input_equals_host_input(kind):
    import torch
    from event_representation_study_amd import est
    C = 5
    ev = wrapper_events(kind, H, W)
    layer = est.QuantizationLayer((C, H, W), est.PiecewiseLinearKernel(_weights(np.load(GOLDEN_EST))), image_size=None, device=DEV)
    dev_in = torch.from_numpy(ev).to(DEV)
    keep = dev_in.clone()
    got = layer.voxel(dev_in)
    want = layer.voxel(torch.from_numpy(ev.copy()))
    assert torch.equal(dev_in, keep)                                             # the CUDA input is left alone
    assert got.shape == (3, 2 * C, H, W)
    nan_equal_bits(got.cpu().numpy(), want.cpu().numpy(), kind)
    assert bool(torch.isnan(got).any()) == (kind == "zero_times")


@pytest.mark.parametrize("size", [96, None])
def test_trainable_layer_cuda_input_equals_host_input(size):
    import torch
    from event_representation_study_amd import est
    g = np.load(GOLDEN_GRAD)
    C, H_, W_ = (int(v) for v in g["dim"])
    state = state_of(g)
    res = {}
    for route in ("host", "cuda"):
        events = torch.from_numpy(g["events"].copy())
        events = events.to(DEV) if route == "cuda" else events
        layer = est.TrainableQuantizationLayer((C, H_, W_), est.ValueLayer(state), image_size=size, device=DEV)
        out = layer(events)
        wt = torch.from_numpy(loss_weights(out.shape, g["seed"])).to(DEV)
        (wt * out).sum().backward()
        assert np.array_equal(events.cpu().numpy(), g["events"]) and events.grad is None
        grads = {k: p.grad.detach().cpu().numpy() for k, p in layer.value_layer.named_parameters()}
        res[route] = (out.detach().cpu().numpy(), grads)
    assert_bit_equal(res["cuda"][0], res["host"][0], "output")
    assert set(res["cuda"][1]) == set(KEYS) and len(KEYS) == 6
    for k in KEYS:
        assert_bit_equal(res["cuda"][1][k], res["host"][1][k], "grad " + k)
        assert np.abs(res["cuda"][1][k]).max() > 0


def test_cuda_input_makes_no_host_round_trip(monkeypatch):
    import torch
    from event_representation_study_amd import est

    def refuse(*a, **k):
        raise AssertionError("the host route was taken")
    ev = wrapper_events("skipped_index", H, W)
    layer = est.QuantizationLayer((5, H, W), est.PiecewiseLinearKernel(_weights(np.load(GOLDEN_EST))), image_size=None, device=DEV)
    want = layer.voxel(torch.from_numpy(ev.copy()))
    monkeypatch.setattr(est, "_prepare_events_host", refuse)
    got = layer.voxel(torch.from_numpy(ev).to(DEV))
    assert torch.equal(got, want)
    with pytest.raises(AssertionError, match="host route"):
        layer.voxel(torch.from_numpy(ev.copy()))                                 # the dispatcher sends a host tensor to the host route
    with pytest.raises(AssertionError, match="host route"):
        layer.voxel(ev.copy())                                                   # and a numpy array


def test_prepare_is_deterministic():
    for name in ("tiny_items", "unsorted_max_in_first_wave", "edge_lengths"):
        ev, bs = good_stream(name)
        a, b = _prepare(ev, bs), _prepare(ev, bs)
        for x, y in zip(a, b):
            assert_bit_equal(x, y, name)


@pytest.mark.parametrize("name", ["jump_0_7", "trailing_empty", "b_beyond_batch_size", "b_negative_and_nan"])
def test_offsets_and_status_stay_inside_their_words(name):
    """the entry point itself, with guard words on both sides of offsets and status -- also for streams whose batch indices
    are refused: they are clamped before they index anything"""
    import torch
    from event_representation_study_amd import _lib
    lib = _lib.load()
    if name in GOOD:
        ev, bs = good_stream(name)
        want_status = 0
    elif name == "b_beyond_batch_size":
        ev, bs, _ = bad_stream(name)
        want_status = _lib.EST_PREP_BAD_INDEX
    else:
        ev, bs, _ = bad_stream("p_2")
        ev[:, 3] = (ev[:, 3] > 0)
        ev[:5, 4], ev[5:9, 4], ev[-3:, 4] = -4.0, np.nan, 1e9
        bs, want_status = 2, _lib.EST_PREP_BAD_INDEX
    B = bs if bs is not None else int(1 + ev[-1, 4])
    n, G, MARK = len(ev), 8, -0x5A5A5A5A5A5A5A5B
    d = torch.from_numpy(ev).to(DEV)
    offs = torch.full((G + B + 1 + G,), MARK, dtype=torch.int64, device=DEV)
    stat = torch.full((2 * G + 1,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    rows = torch.empty((n, 4), dtype=torch.int32, device=DEV)
    tn = torch.empty(n, dtype=torch.float32, device=DEV)
    scratch = torch.empty(int(lib.evrep_est_prepare_scratch_bytes(n, B)), dtype=torch.uint8, device=DEV)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)  # noqa: E731
    rc = lib.evrep_est_prepare(p(d), n, B, H, W, p(rows), p(offs, 8 * G), p(tn), p(stat, 4 * G), p(scratch),
                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == _lib.EVREP_OK
    torch.cuda.synchronize()
    offs, stat = offs.cpu().numpy(), stat.cpu().numpy()
    assert (offs[:G] == MARK).all() and (offs[-G:] == MARK).all()
    assert (stat[:G] == 0x5A5A5A5A).all() and (stat[-G:] == 0x5A5A5A5A).all()
    inner = offs[G:G + B + 1]
    assert (inner != MARK).all() and inner.min() >= 0 and inner.max() <= n        # every entry written
    assert int(stat[G]) == want_status
    if want_status == 0:
        assert_bit_equal(inner, restated(ev, bs)[1], name)
