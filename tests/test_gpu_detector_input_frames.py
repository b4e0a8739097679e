"""GPU: the detector input for frames of different sizes (DetectorFrontEnd.prepare_frames: evrep_resize_tap_tables +
evrep_detector_input_frames, csrc/evrep_detin_frames.hip).  The device tap tables against gwd_pipeline.resize_taps bit for
bit; the images against the tests' numpy restatement (tests/detector_input_ref.py) per sample, against the per-window route
and the 4-D route, bit for bit; and against the golden recorded from the reference's Gen1H5.__getitem__ with TORE's
bounding-box frames (cv2 behind a stand-in there: parity unpinned).  S = 48; frames 31x47 and 47x31 (letterbox resizes once
more), 48x20 (r == 1), 70x96 (shrinks; INTER_AREA in validation), 1x1, 5x7, 47x47; C in {12, 5}; float64 and float32."""
import os
import random

import numpy as np
import pytest
import torch

from conftest import ROOT
import detector_input_ref as ref
import test_detector_input_frames_cpu as host
import test_gpu_detector_input as dense

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "detector_input_frames.npz")
DEV = "cuda:0"
S = 48
SIZES = [(31, 47), (47, 31), (48, 20), (70, 96), (1, 1), (5, 7), (47, 47)]
DTYPES = [np.float64, np.float32]
_assert_bits, _params, _front = dense._assert_bits, dense._params, dense._front


def _di():
    from event_representation_study_amd import detector_input
    return detector_input


def _frames(C, dtype, seed=0, sizes=SIZES):
    rng = np.random.default_rng(100 + seed + 31 * C)
    return [rng.uniform(0, 255, (h, w, C)).astype(dtype) for h, w in sizes]


def _dev(frames):
    return [torch.from_numpy(f).to(DEV) for f in frames]


def _train_mix():
    """Per sample of SIZES: (matrix, (flipud, fliplr)) -- warping, flipping and untouched samples, both kinds on frames that
    need the second resize."""
    Ms = dense._matrices(S)
    mats = [Ms[3], np.eye(3), Ms[7], Ms[12], Ms[2], np.eye(3), Ms[9]]
    flips = [(0, 1), (1, 0), (0, 0), (1, 1), (0, 0), (0, 0), (1, 0)]
    return mats, flips


def _want(frames, augment, mats=None, flips=None, pad=114.0, scale=None):
    outs = []
    for b, f in enumerate(frames):
        M = None if mats is None else [mats[b]]
        ud, lr = (None, None) if flips is None else ([flips[b][0]], [flips[b][1]])
        outs.append(ref.detector_input_ref(f[None], S, augment, M, ud, lr, pad=pad, scale=scale)[0])
    return np.stack(outs)


# ------------------------------------------------------------------------------------------------ 1
def test_device_tap_tables_equal_the_host_tables():
    di = _di()
    axes = []
    for src in range(1, 97):
        for dst in range(1, 97):
            axes.append((src, dst, "linear", 2 + (src + dst) % 3 // 2))                     # every third one padded to T = 3
            if dst <= src:
                axes.append((src, dst, "area", di.area_taps_bound(src, dst) + (src * dst) % 4 // 3 * 2))
    axes.append((48, 48, "identity", 1))
    axes.append((7, 7, "identity", 3))
    got = di.resize_tap_tables(axes, DEV)
    torch.cuda.synchronize()
    start = torch.cat([g[0] for g in got]).cpu().numpy()
    count = torch.cat([g[1] for g in got]).cpu().numpy()
    whole = torch.cat([g[2].reshape(-1) for g in got]).cpu().numpy()
    want_start, want_count, want_w = [], [], []
    for src, dst, interp, T in axes:
        if interp == "identity":
            s, c, w = np.arange(dst, dtype=np.int32), np.ones(dst, dtype=np.int32), np.ones((dst, 1))
        else:
            s, c, w, _ = (t.numpy() if torch.is_tensor(t) else t for t in di.resize_taps(src, dst, interp, "cpu"))
        assert w.shape[1] <= T, (src, dst, interp, T)
        padded = np.zeros((dst, T))
        padded[:, :w.shape[1]] = w
        want_start.append(s)
        want_count.append(c)
        want_w.append(padded.reshape(-1))
    want_start, want_count, want_w = np.concatenate(want_start), np.concatenate(want_count), np.concatenate(want_w)
    assert start.dtype == np.int32 and count.dtype == np.int32 and whole.dtype == np.float64
    assert np.array_equal(start, want_start)
    assert np.array_equal(count, want_count) and count.min() >= 0
    bad = whole.view(np.int64) != want_w.view(np.int64)                                      # +0.0 padding included
    assert not bad.any(), "%d of %d weights differ" % (bad.sum(), bad.size)
    assert (count > 2).any() and (count == 1).any()


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("C", [12, 5])
def test_frames_launch_is_bit_equal_to_the_restatement_per_sample(C, dtype):
    frames = _frames(C, dtype)
    d_frames = _dev(frames)
    mats, flips = _train_mix()
    fe = _front(S, True)
    assert [fe.geometry(h, w).fused for h, w in SIZES].count(False) >= 3
    got = fe.prepare_frames(d_frames, params=_params(mats, flips), scale=None)[0]
    _assert_bits(got, _want(frames, True, mats, flips), "train")
    pad = np.arange(C, dtype=np.float64) + 100
    got = fe.prepare_frames(d_frames, params=_params(mats, flips), pad=pad)[0]
    _assert_bits(got, _want(frames, True, mats, flips, pad=pad, scale=1.0 / 255), "train, pad table, / 255")
    val = _front(S, False)
    state = random.getstate()
    got, targets, shapes = val.prepare_frames(d_frames, labels=[np.zeros((0, 5), np.float32)] * len(frames), scale=None)
    assert random.getstate() == state and targets.shape == (0, 6) and [s[0] for s in shapes] == SIZES
    _assert_bits(got, _want(frames, False), "validation")
    got = val.prepare_frames(d_frames, pad=pad)[0]
    _assert_bits(got, _want(frames, False, pad=pad, scale=1.0 / 255), "validation, pad table, / 255")


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_three_routes_agree(dtype):
    d_frames = _dev(_frames(12, dtype, seed=1))
    mats, flips = _train_mix()
    for augment in (True, False):
        fe = _front(S, augment)
        params = _params(mats, flips) if augment else fe.draw(len(SIZES))
        ragged = fe.prepare_frames(d_frames, params=params)[0]
        for b, f in enumerate(d_frames):
            one = fe.prepare(f[None], params=[params[b]])[0]
            assert torch.equal(ragged[b].view(torch.int32), one[0].view(torch.int32)), (augment, SIZES[b])
    # frames of one size: the 4-D route
    fe = _front(S, True)
    same = _dev(_frames(12, dtype, seed=2, sizes=[(20, 30)] * 3))
    params = _params(mats[:3], flips[:3])
    labels = [np.array([[0, 0.5, 0.5, 0.4, 0.4], [1, 0.3, 0.6, 0.2, 0.3]], dtype=np.float32)] * 3
    a = fe.prepare_frames(same, labels=labels, params=params)
    b = fe.prepare(torch.stack(same), labels=labels, params=params)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1]) and a[2] == b[2]
    # a non-contiguous frame is made contiguous, not misread
    wide = torch.from_numpy(_frames(12, dtype, seed=3, sizes=[(20, 60)])[0]).to(DEV)
    cut = wide[:, 10:40]
    assert not cut.is_contiguous()
    c = fe.prepare_frames([cut], params=params[:1])[0]
    d = fe.prepare(cut.contiguous()[None], params=params[:1])[0]
    assert torch.equal(c.view(torch.int32), d.view(torch.int32))


def test_prepare_frames_draws_as_draw_does():
    d_frames = _dev(_frames(5, np.float32, seed=4, sizes=SIZES[:3]))
    fe = _front(S, True)
    random.seed(31)
    params = fe.draw(3)
    state = random.getstate()
    random.seed(31)
    got = fe.prepare_frames(d_frames)[0]
    assert random.getstate() == state
    assert torch.equal(got.view(torch.int32), fe.prepare_frames(d_frames, params=params)[0].view(torch.int32))


# ------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_guard_words_around_the_output_survive(dtype):
    sizes = [(31, 47), (70, 96), (5, 7)]
    C, B, guard = 5, 3, 4096
    frames = _frames(C, dtype, seed=5, sizes=sizes)
    n = B * C * S * S
    buf = torch.full((n + 2 * guard,), float("nan"), dtype=torch.float32, device=DEV)
    buf.view(torch.int32).fill_(0x7FC0DEAD)
    out = buf[guard:guard + n].view(B, C, S, S)
    Ms = dense._matrices(S)
    mats, flips = [Ms[3], Ms[8], np.eye(3)], [(0, 0), (1, 0), (0, 1)]
    got = _front(S, True).prepare_frames(_dev(frames), params=_params(mats, flips), scale=None, out=out)[0]
    assert got.data_ptr() == out.data_ptr()
    words = buf.view(torch.int32)
    assert (words[:guard] == 0x7FC0DEAD).all() and (words[guard + n:] == 0x7FC0DEAD).all()
    assert not (words[guard:guard + n] == 0x7FC0DEAD).any()          # every element was written
    _assert_bits(out, _want(frames, True, mats, flips), "guarded output")


# ------------------------------------------------------------------------------------------------ 5
def test_golden_images_targets_and_shapes_through_prepare_frames():
    di = _di()
    cases = ref.load_golden(GOLDEN)
    for group in host.golden_batches(cases):
        c0 = group[0]
        fe = di.DetectorFrontEnd(int(c0["img_size"]), host._hyp(c0), augment=bool(c0["augment"]))
        params = host.golden_params(fe, group)
        frames = [torch.from_numpy(c["rep"]).to(DEV) for c in group]
        images, targets, shapes = fe.prepare_frames(frames, labels=[c["boxes"] for c in group], params=params, scale=None)
        t = targets.numpy()
        assert targets.dtype == torch.float32
        for b, c in enumerate(group):
            _assert_bits(images[b], c["image"], "golden seed %d" % int(c["seed"]))
            assert np.array_equal(t[t[:, 0] == b][:, 1:], c["labels_out"][:, 1:])
            (h0, w0), ((rh, rw), pad) = shapes[b]
            assert [h0, w0, rh, rw, pad[0], pad[1]] == list(c["shapes"])


# ------------------------------------------------------------------------------------------------ 6, 7
class _Spy:
    """Counts the two launches of a batch and keeps the frame addresses the second one was given."""

    def __init__(self, monkeypatch):
        from event_representation_study_amd import _lib
        self.lib, self.taps, self.frames, self.src = _lib.api(), 0, 0, []      # the handle the package calls through
        real_taps, real_frames = self.lib.evrep_resize_tap_tables, self.lib.evrep_detector_input_frames

        def taps(*a):
            self.taps += 1
            return real_taps(*a)

        def frames(table, B, *a):
            self.frames += 1
            self.src = [f.src for f in (_lib.DetinFrame * B).from_address(table.value)]
            return real_frames(table, B, *a)

        monkeypatch.setattr(self.lib, "evrep_resize_tap_tables", taps)
        monkeypatch.setattr(self.lib, "evrep_detector_input_frames", frames)


def _windows():
    from event_representation_study_amd.synthetic import make_events, make_events_moving_circle
    W, H = 40, 30
    one = np.array([[17, 11, 500, 1]], dtype=np.int32)
    return [make_events_moving_circle(400, W, H, seed=1), one,
            make_events_moving_circle(300, W, H, seed=2, circle_radius=3.0, starting_point=(8.0, 12.0), flow=(4.0, 2.0)),
            make_events(500, W, H, seed=3)], H, W


def test_windows_to_detector_batch_in_two_launches_without_a_frame_copy(monkeypatch):
    from event_representation_study_amd.engine import EventBatch
    windows, H, W = _windows()
    frames = EventBatch.from_numpy(windows, H, W, device=DEV).tore(scale=255.0)
    sizes = [tuple(f.shape[:2]) for f in frames]
    assert sizes[1] == (1, 1) and len(set(sizes)) == 4 and all(f.shape[2] == 12 and f.is_cuda for f in frames)
    fe = _front(S, True)
    random.seed(9)
    params = fe.draw(4)
    labels = [np.array([[0, 0.5, 0.5, 0.4, 0.4]], dtype=np.float32)] * 4
    spy = _Spy(monkeypatch)
    images, targets, shapes = fe.prepare_frames(frames, labels=labels, params=params)
    assert (spy.taps, spy.frames) == (1, 1)
    assert spy.src == [f.data_ptr() for f in frames]                    # the views are read where they lie
    assert images.shape == (4, 12, S, S) and [s[0] for s in shapes] == sizes
    rows = []
    for b, f in enumerate(frames):
        im, t, sh = fe.prepare(f[None], labels=[labels[b]], params=[params[b]])
        assert torch.equal(images[b].view(torch.int32), im[0].view(torch.int32)), sizes[b]
        assert sh[0] == shapes[b]
        t[:, 0] = b
        rows.append(t)
    assert torch.equal(targets, torch.cat(rows))


def test_refusals_on_the_device_launch_nothing(monkeypatch):
    from event_representation_study_amd.engine import EventBatch
    windows, H, W = _windows()
    windows[2] = np.zeros((0, 4), dtype=np.int32)                        # an empty window: no bounding box
    frames = EventBatch.from_numpy(windows, H, W, device=DEV).tore(scale=255.0)
    assert tuple(frames[2].shape) == (0, 0, 12)
    fe = _front(S, True)
    spy = _Spy(monkeypatch)
    state = random.getstate()
    with pytest.raises(ValueError, match="sample 2 is an empty"):
        fe.prepare_frames(frames)
    with pytest.raises(TypeError, match="sample 1"):
        fe.prepare_frames([frames[0], frames[1].double()])
    with pytest.raises(ValueError, match="int32"):                      # warp_tables' refusal, as in prepare
        fe.prepare_frames([frames[0], frames[1]], params=_params([np.eye(3), dense._translation(3e6, 0)]))
    assert (spy.taps, spy.frames) == (0, 0) and random.getstate() == state
