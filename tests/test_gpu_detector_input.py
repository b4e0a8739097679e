"""GPU: the one-launch detector input (csrc/evrep_detin.hip through detector_input.DetectorFrontEnd) against the tests' numpy
restatement of stages R-F (tests/detector_input_ref.py) bit for bit, against the staged route, against torch's own grid_sample
and `.float() / 255`, and against the golden recorded from the reference's Gen1H5.__getitem__ (cv2 behind a stand-in there:
parity unpinned).  Shapes: B = 3, S in {32, 33, 48}; sources 20x30 and 30x20 (linear: pad rows / pad columns, top != bottom),
96x70 (area), 48x48 (r == 1); C in {1, 2, 5, 12}; float64 and float32."""
import math
import os
import random

import numpy as np
import pytest
import torch

from conftest import ROOT
import detector_input_ref as ref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "detector_input.npz")
DEV = "cuda:0"
# (H, W, S, C, augment): augment picks INTER_LINEAR / scale-up; False is the validation geometry (INTER_AREA when shrinking)
CONFIGS = [(20, 30, 32, 5, True), (30, 20, 33, 12, True), (96, 70, 48, 2, False), (48, 48, 48, 1, True)]
DTYPES = [np.float64, np.float32]


def _di():
    from event_representation_study_amd import detector_input
    return detector_input


def _rep(H, W, C, dtype, B=3, seed=0):
    rng = np.random.default_rng(seed + 7 * H + W + 31 * C)
    return rng.uniform(0, 255, (B, H, W, C)).astype(dtype)


def _translation(tx, ty):
    return np.array([[1.0, 0, tx], [0, 1.0, ty], [0, 0, 1]])


def _matrices(S):
    di = _di()
    c, s = math.cos(math.pi / 4), math.sin(math.pi / 4)
    rot_shear = _translation(S / 2, S / 2) @ np.array([[1, 0.8, 0], [0.6, 1, 0], [0, 0, 1.0]]) @ np.array([[c, s, 0], [-s, c, 0], [0, 0, 1.0]]) \
        @ _translation(-S / 2, -S / 2)
    small = _translation(S / 2, S / 2) @ np.diag([0.1, 0.1, 1.0]) @ _translation(-S / 2, -S / 2)
    Ms = [np.eye(3), _translation(3, -2), small, rot_shear, np.array([[1.0, 2.0, 0], [0.5, 1.0, 0], [0, 0, 1]]), _translation(1e6, 0)]
    random.seed(2024)
    h = ref.REF_HYP
    Ms += [di.get_transform_matrix((S, S), (S, S), h["degrees"], h["scale"], h["shear"], h["translate"])[0] for _ in range(20)]
    return Ms + [np.eye(3)]          # 27: nine batches of three


def _params(Ms, flips=None):
    di = _di()
    flips = flips or [(False, False)] * len(Ms)
    return [di.SampleParams(M, 1.0, bool(f[0]), bool(f[1])) for M, f in zip(Ms, flips)]


def _front(S, augment):
    return _di().DetectorFrontEnd(S, ref.REF_HYP, augment=augment)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_bits(got, want, what=""):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape, what
    bad = _bits(got) != _bits(want)
    assert not bad.any(), "%s: %d of %d elements differ, first at %s" % (what, bad.sum(), bad.size, np.argwhere(bad)[:3].tolist())


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "%dx%d_S%d_C%d" % c[:4])
def test_kernel_is_bit_equal_to_the_restatement(cfg, dtype):
    H, W, S, C, aug = cfg
    rep = _rep(H, W, C, dtype)
    fe, Ms = _front(S, aug), _matrices(S)
    I = ref.letterbox_ref(rep, S, aug)
    d_rep = torch.from_numpy(rep).to(DEV)
    for k in range(0, len(Ms), 3):
        got, _, _ = fe.prepare(d_rep, params=_params(Ms[k:k + 3]), scale=None)
        _assert_bits(got, ref.finish_ref(I, Ms[k:k + 3], None, None), "matrices %d..%d" % (k, k + 2))


def test_integer_translation_is_a_shifted_copy_with_border_fill():
    H, W, S, C, aug = CONFIGS[0]
    rep = _rep(H, W, C, np.float64)
    I = ref.letterbox_ref(rep, S, aug)
    got, _, _ = _front(S, aug).prepare(torch.from_numpy(rep).to(DEV), params=_params([_translation(3, -2)] * 3), scale=None)
    want = np.full_like(I, 114.0)
    want[:, :S - 2, 3:] = I[:, 2:, :S - 3]                 # out(y, x) = I(y + 2, x - 3)
    _assert_bits(got, want.transpose(0, 3, 1, 2)[:, ::-1].astype(np.float32), "translation (3, -2)")
    far, _, _ = _front(S, aug).prepare(torch.from_numpy(rep).to(DEV), params=_params([_translation(1e6, 0)] * 3), scale=None)
    assert (far == 114.0).all()                            # the int16 clamp: everything is border


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "%dx%d_S%d_C%d" % c[:4])
def test_fused_launch_equals_the_staged_route(cfg, dtype):
    H, W, S, C, aug = cfg
    d_rep = torch.from_numpy(_rep(H, W, C, dtype, seed=1)).to(DEV)
    fe, Ms = _front(S, aug), _matrices(S)
    assert fe.geometry(H, W).fused
    params = _params([Ms[3], Ms[7], Ms[0]], [(1, 0), (0, 1), (1, 1)])
    fused, _, _ = fe.prepare(d_rep, params=params)
    staged, _, _ = fe.prepare(d_rep, params=params, staged=True)
    assert torch.equal(fused.view(torch.int32), staged.view(torch.int32))
    # the intermediate of the staged route is what the existing functions write
    im, g = fe.letterboxed(d_rep)
    want = ref.letterbox_ref(d_rep.cpu().numpy(), S, aug)
    assert np.array_equal(fe._pad_square(im, g, 114.0).cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_flips_and_channel_reversal_are_index_permutations(dtype):
    H, W, S, C, aug = CONFIGS[1]
    rep = _rep(H, W, C, dtype, seed=2)
    d_rep = torch.from_numpy(rep).to(DEV)
    fe, Ms = _front(S, aug), _matrices(S)
    three = [Ms[3], Ms[0], Ms[9]]
    plain = fe.prepare(d_rep, params=_params(three))[0]
    for ud in (0, 1):
        for lr in (0, 1):
            got = fe.prepare(d_rep, params=_params(three, [(ud, lr)] * 3))[0]
            want = plain.flip(2) if ud else plain
            want = want.flip(3) if lr else want
            assert torch.equal(got.view(torch.int32), want.contiguous().view(torch.int32)), (ud, lr)
    swapped = fe.prepare(torch.from_numpy(np.ascontiguousarray(rep[..., ::-1])).to(DEV), params=_params(three))[0]
    assert torch.equal(swapped.view(torch.int32), plain.flip(1).contiguous().view(torch.int32))
    # [::-1]: output channel c is source channel C-1-c
    ident = fe.prepare(d_rep, params=_params([np.eye(3)] * 3), scale=None)[0].cpu().numpy()
    I = ref.letterbox_ref(rep, S, aug)
    for c in range(C):
        assert np.array_equal(ident[:, c], I[..., C - 1 - c].astype(np.float32))


# ------------------------------------------------------------------------------------------------ 4
def test_against_torch_grid_sample_in_float64():
    """An independent reference: torch's CPU grid_sample in float64 at the EXACT inverse coordinates.  Where the four taps lie
    inside, the kernel's fixed-point walk differs by at most 2 (1/64 + 1/1024) g, g the largest difference between neighbouring
    pixels of I: the coordinate is rounded to 1/32 pixel (1/64) after two roundings of 1/1024 (adelta / bdelta and X0 / Y0, 1/2048
    each), and bilinear interpolation is g-Lipschitz per axis.  (The issue's CPU prototype measured 0.024 g over twenty drawn
    matrices at S = 48.)"""
    H, W, S, C, aug = 48, 48, 48, 5, True
    rep = _rep(H, W, C, np.float64, seed=3)
    I = ref.letterbox_ref(rep, S, aug)
    g = max(np.abs(np.diff(I, axis=1)).max(), np.abs(np.diff(I, axis=2)).max())
    bound = 2 * (1 / 64 + 1 / 1024) * g
    Ms = _matrices(S)[6:26] + _matrices(S)[6:7]          # the twenty drawn matrices, in seven batches of three
    fe, d_rep = _front(S, aug), torch.from_numpy(rep).to(DEV)
    worst, checked = 0.0, 0
    for k in range(0, 21, 3):
        got = fe.prepare(d_rep, params=_params(Ms[k:k + 3]), scale=None)[0].cpu().numpy().astype(np.float64)
        for j in range(3):
            Minv = np.linalg.inv(Ms[k + j])
            yy, xx = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64), indexing="ij")
            sx = Minv[0, 0] * xx + Minv[0, 1] * yy + Minv[0, 2]
            sy = Minv[1, 0] * xx + Minv[1, 1] * yy + Minv[1, 2]
            grid = torch.from_numpy(np.stack([2 * sx / (S - 1) - 1, 2 * sy / (S - 1) - 1], -1))[None]
            img = torch.from_numpy(np.ascontiguousarray(I[j].transpose(2, 0, 1)))[None]
            want = torch.nn.functional.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0].numpy()
            inside = (sx >= 1) & (sx <= S - 2) & (sy >= 1) & (sy <= S - 2)      # the four taps of both walks lie inside
            err = np.abs(got[j][::-1] - want)[:, inside]
            print("matrix %d: %d outputs inside, max error %.5f g" % (k + j, inside.sum(), err.max() / g if err.size else 0.0))
            worst, checked = max(worst, err.max() if err.size else 0.0), checked + int(inside.sum())
    assert checked > 5 * S * S
    assert worst <= bound, (worst / g, bound / g)


# ------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_scaled_output_is_torchs_float_div_255(dtype):
    H, W, S, C, aug = CONFIGS[1]
    d_rep = torch.from_numpy(_rep(H, W, C, dtype, seed=4)).to(DEV)
    fe = _front(S, aug)
    params = _params(_matrices(S)[6:9], [(1, 0), (0, 0), (0, 1)])
    staged = fe.prepare(d_rep, params=params, scale=None)[0]
    scaled = fe.prepare(d_rep, params=params)[0]
    assert torch.equal(scaled.view(torch.int32), (staged.float() / 255).view(torch.int32))


# ------------------------------------------------------------------------------------------------ 6
def test_golden_images_and_targets_through_prepare():
    di = _di()
    for c in ref.load_golden(GOLDEN):
        S = int(c["img_size"])
        hyp = dict(ref.REF_HYP)
        if int(c["return_int"]) >= 0:
            hyp["letterbox_return_int"] = bool(c["return_int"])
        fe = di.DetectorFrontEnd(S, hyp, augment=bool(c["augment"]))
        random.seed(int(c["seed"]))
        images, targets, shapes = fe.prepare(torch.from_numpy(c["rep"][None]).to(DEV), labels=[c["boxes"]], scale=None)
        _assert_bits(images[0], c["image"], "golden seed %d" % int(c["seed"]))
        assert targets.dtype == torch.float32 and np.array_equal(targets.numpy()[:, 1:], c["labels_out"][:, 1:])
        (h0, w0), ((rh, rw), pad) = shapes[0]
        assert [h0, w0, rh, rw, pad[0], pad[1]] == list(c["shapes"])


# ------------------------------------------------------------------------------------------------ 7
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_guard_words_around_the_output_survive(dtype):
    di = _di()
    H, W, S, C, aug = CONFIGS[0]
    B, guard = 3, 4096
    d_rep = torch.from_numpy(_rep(H, W, C, dtype, seed=5)).to(DEV)
    fe = _front(S, aug)
    g = fe.geometry(H, W)
    n = B * C * S * S
    buf = torch.full((n + 2 * guard,), float("nan"), dtype=torch.float32, device=DEV)
    buf.view(torch.int32).fill_(0x7FC0DEAD)
    out = buf[guard:guard + n].view(B, C, S, S)
    Ms = _matrices(S)
    flags = np.array([1, 1 | 2, 4], dtype=np.uint32)
    warp = np.stack([np.stack(di.warp_tables(M, S)) for M in (Ms[3], Ms[8], Ms[0])]).astype(np.int32)
    rows, cols = di.resize_taps(H, g.rh, g.interp, d_rep.device), di.resize_taps(W, g.rw, g.interp, d_rep.device)
    got = di.detector_input(d_rep, S, rows, cols, g.nh, g.nw, g.top, g.left, 114.0, flags, warp, None, out=out)
    assert got.data_ptr() == out.data_ptr()
    words = buf.view(torch.int32)
    assert (words[:guard] == 0x7FC0DEAD).all() and (words[guard + n:] == 0x7FC0DEAD).all()
    assert not (words[guard:guard + n] == 0x7FC0DEAD).any()          # every element was written
    want = ref.finish_ref(ref.letterbox_ref(d_rep.cpu().numpy(), S, aug), [Ms[3], Ms[8], None], [0, 1, 0], [0, 0, 1])
    _assert_bits(out, want, "guarded output")


# ------------------------------------------------------------------------------------------------ 8
def test_batch_where_only_some_samples_warp_or_flip():
    H, W, S, C, aug = CONFIGS[1]
    rep = _rep(H, W, C, np.float32, seed=6)
    Ms = _matrices(S)
    mats, flips = [Ms[10], np.eye(3), np.eye(3)], [(0, 0), (1, 1), (0, 0)]
    got = _front(S, aug).prepare(torch.from_numpy(rep).to(DEV), params=_params(mats, flips))[0]
    want = ref.detector_input_ref(rep, S, aug, mats, [f[0] for f in flips], [f[1] for f in flips], scale=1.0 / 255)
    _assert_bits(got, want, "mixed batch")
    # per-channel pad table
    pad = np.arange(C, dtype=np.float64) + 100
    got = _front(S, aug).prepare(torch.from_numpy(rep).to(DEV), params=_params(mats, flips), pad=pad, scale=None)[0]
    _assert_bits(got, ref.detector_input_ref(rep, S, aug, mats, [f[0] for f in flips], [f[1] for f in flips], pad=pad), "pad table")


def test_validation_route_has_no_warp_no_flip_no_scale_up():
    for (H, W, S, C, _) in CONFIGS:
        rep = _rep(H, W, C, np.float32, seed=8)
        fe = _front(S, False)
        state = random.getstate()
        got, targets, shapes = fe.prepare(torch.from_numpy(rep).to(DEV), labels=[np.zeros((0, 5), np.float32)] * 3)
        assert random.getstate() == state and targets.shape == (0, 6) and len(shapes) == 3
        _assert_bits(got, ref.detector_input_ref(rep, S, False, scale=1.0 / 255), "validation %dx%d" % (H, W))


# ------------------------------------------------------------------------------------------------ 9
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_fallback_when_letterbox_needs_its_own_resize(dtype):
    H, W, S, C = 31, 47, 48, 5
    rep = _rep(H, W, C, dtype, seed=9)
    fe = _front(S, True)
    g = fe.geometry(H, W)
    assert not g.fused and (g.nh, g.nw) != (g.rh, g.rw)
    Ms = _matrices(S)
    mats, flips = [Ms[12], np.eye(3), Ms[3]], [(0, 1), (1, 0), (0, 0)]
    got = fe.prepare(torch.from_numpy(rep).to(DEV), params=_params(mats, flips), scale=None)[0]
    want = ref.detector_input_ref(rep, S, True, mats, [f[0] for f in flips], [f[1] for f in flips])
    _assert_bits(got, want, "fallback")


# ------------------------------------------------------------------------------------------------ 10
def test_matrix_whose_tables_leave_int32_raises_before_any_launch(monkeypatch):
    di = _di()
    H, W, S, C, aug = CONFIGS[0]
    d_rep = torch.from_numpy(_rep(H, W, C, np.float32)).to(DEV)
    launched = []
    monkeypatch.setattr(di, "detector_input", lambda *a, **k: launched.append(1))
    for bad in (_translation(3e6, 0), np.diag([1e-7, 1.0, 1.0])):
        with pytest.raises(ValueError):
            _front(S, aug).prepare(d_rep, params=_params([np.eye(3), bad, np.eye(3)]))
    assert not launched


def test_cpu_tensor_is_refused():
    di = _di()
    from event_representation_study_amd._lib import EvrepError
    with pytest.raises(EvrepError):
        _front(32, True).prepare(torch.zeros((1, 20, 30, 2), dtype=torch.float32), params=_params([np.eye(3)]))
    assert di.DetectorFrontEnd(32).prepare(torch.zeros((1, 20, 30, 2), device=DEV))[0].shape == (1, 2, 32, 32)


# ------------------------------------------------------------------------------------------------ the whole route
def test_recording_to_detector_batch_without_a_host_copy():
    """DeviceRecording.windows_before -> builder -> DetectorFrontEnd.prepare: events and images stay on the device."""
    from event_representation_study_amd.recording import DeviceRecording
    from event_representation_study_amd.synthetic import make_events
    H, W, S = 30, 40, 48
    ev = make_events(3000, W, H, seed=5, polarity="01")
    rec = DeviceRecording(ev[:, 0], ev[:, 1], np.sort(ev[:, 2]), ev[:, 3], H, W, device=DEV)
    batch = rec.windows_before([1000, 2000, 3000], 800)
    rep = batch.event_stack()
    assert rep.is_cuda and rep.shape[:3] == (3, H, W)
    fe = _front(S, True)
    random.seed(1)
    params = fe.draw(3)
    labels = [np.array([[0, 0.5, 0.5, 0.4, 0.4]], dtype=np.float32)] * 3
    images, targets, shapes = fe.prepare(rep, labels=labels, params=params)
    assert images.is_cuda and images.shape == (3, int(rep.shape[3]), S, S) and images.dtype == torch.float32
    want = ref.detector_input_ref(rep.cpu().numpy(), S, True, [p.M for p in params], [p.flipud for p in params],
                                  [p.fliplr for p in params], scale=1.0 / 255)
    _assert_bits(images, want, "whole route")
    assert targets.shape[1] == 6 and set(targets[:, 0].tolist()) <= {0.0, 1.0, 2.0}
