"""CPU: the host side of N-ImageNet's event front end (event_representation_study_amd/n_imagenet_front.py) against
tests/golden/nimg_front.npz, which the reference's own load_event / parse_event / base_augment wrote
(tests/golden/make_golden_nimg_front.py).

The host mirrors run on temporary .npz samples in both layouts load_event reads, under the recorded seeds: their output is
bit-equal to the reference's (float64, no tolerance), and they leave both random generators in the recorded state.
``draw_slice`` / ``draw_augment`` return the recorded parameters, and ``host_rows`` with those parameters -- the restatement
the device path is tested against -- gives the same rows again.  The new C entry point is checked for its EVREP_EINVAL cases;
nothing is launched.
"""
import ctypes
import hashlib
import json
import random
import types

import numpy as np
import pytest
import torch

from conftest import assert_bit_equal, load_golden

_G = load_golden("nimg_front")
CASES = json.loads(str(_G["manifest"]))
IDS = [c["name"] for c in CASES]


def columns(case):
    return tuple(_G["stream%d.%s" % (case["stream"], k)] for k in "xytp")


def write_sample(path, cols, layout):
    x, y, t, p = cols
    if layout == "compressed":
        rec = np.zeros(len(x), dtype=[("x", "<u2"), ("y", "<u2"), ("t", "<i8"), ("p", "i1")])
        rec["x"], rec["y"], rec["t"], rec["p"] = x, y, t, p
        np.savez(path, event_data=rec)
    else:
        np.savez(path, x_pos=x, y_pos=y, timestamp=t, polarity=p)


def state_digests():
    a = np.random.get_state()
    return (hashlib.sha1(np.asarray(a[1], np.uint32).tobytes() + repr(tuple(a[2:])).encode()).hexdigest(),
            hashlib.sha1(repr(random.getstate()).encode()).hexdigest())


def seed_both(seed):
    np.random.seed(seed)
    random.seed(seed)


def assert_rows_equal(got, want, what):
    """Bit-equal float64 rows; NaNs compare as NaN, all else through assert_bit_equal."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    assert_bit_equal(np.where(nan, 0.0, got), np.where(nan, 0.0, want), what)


def test_the_golden_holds_the_cases_it_must():
    draws = {c["name"]: _G[c["name"] + ".draw"] for c in CASES}
    assert {(int(d[0]), int(d[1])) for n, d in draws.items() if n.startswith("flip_")} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert any(c["mode"] == "eval" for c in CASES)
    pols = {tuple(np.unique(_G["stream%d.p" % c["stream"]]).tolist()) for c in CASES}
    assert {(0, 1), (-1, 1), (1,), (0,)} <= pols
    t = columns(next(c for c in CASES if c["name"] == "dup_times"))[2]
    assert t[0] == t[1] and t[-1] == t[-2]
    c = next(c for c in CASES if c["name"] == "time_slice")
    t = columns(c)[2]
    assert c["cfg"]["slice_start"] in (t / 1e6) and c["cfg"]["slice_end"] in (t / 1e6)
    assert any(c["cfg"].get("slice_start") is None for c in CASES if c["cfg"].get("slice_method") == "idx")
    assert any((c["cfg"].get("slice_start") or 0) < 0 for c in CASES if c["cfg"].get("slice_method") == "idx")
    n = len(t)
    assert any(c["cfg"].get("slice_method") == "random" and c["cfg"]["slice_length"] >= n for c in CASES)
    assert any(c["cfg"].get("slice_method") == "random" and c["cfg"].get("slice_augment") for c in CASES)
    big = columns(next(c for c in CASES if c["name"] == "abs_1p6e15"))[2]
    # t / 1e6 rounds there: the absolute route differs from dividing the rebased times, which is why the device takes t_base
    assert big[0] >= 1_600_000_000_000_000 and np.any(big / 1e6 - big[0] / 1e6 != (big - big[0]) / 1e6)
    assert {c["layout"] for c in CASES} == {"compressed", "columns"}


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_host_mirrors_equal_the_reference(case, tmp_path):
    from event_representation_study_amd import n_imagenet_front as nf
    path = str(tmp_path / "sample.npz")
    write_sample(path, columns(case), case["layout"])
    cfg = types.SimpleNamespace(**case["cfg"])
    seed_both(case["seed"])
    event = nf.parse_event(path, cfg)
    assert isinstance(event, torch.Tensor) and event.dtype == torch.float64
    aug = nf.base_augment(case["mode"])
    out = event if aug is None else aug(event)
    assert_rows_equal(out.numpy(), _G[case["name"] + ".out"], case["name"])
    assert state_digests() == (case["np_state"], case["py_state"]), "the generators are not where the reference leaves them"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_drawn_parameters_equal_the_reference(case):
    from event_representation_study_amd import _lib, n_imagenet_front as nf
    x, y, t, p = columns(case)
    cfg = types.SimpleNamespace(**case["cfg"])
    seed_both(case["seed"])
    sl = nf.draw_slice([len(x)], cfg)
    au = nf.draw_augment(1, case["mode"])
    assert state_digests() == (case["np_state"], case["py_state"])
    tf, xf, xs, ys, s0, s1 = (int(v) for v in _G[case["name"] + ".draw"])
    assert (int(au["time_flip"][0]), int(au["x_flip"][0]), int(au["x_shift"][0]), int(au["y_shift"][0])) == (tf, xf, xs, ys)
    assert (int(sl["s0"][0]), int(sl["s1"][0])) == (s0, s1)
    if case["cfg"].get("slice_method") == "time" and case["cfg"].get("slice_events"):
        assert (sl["t_lo"][0], sl["t_hi"][0]) == (case["cfg"]["slice_start"], case["cfg"]["slice_end"])
    else:
        assert sl["t_lo"][0] == -np.inf and sl["t_hi"][0] == np.inf
    par = nf.pack_params(sl, au)
    assert par.dtype == nf.PARAMS_DTYPE and par.shape == (1,)
    assert int(par["flags"][0]) == (_lib.AUG_TIME_FLIP if tf else 0) | (_lib.AUG_X_FLIP if xf else 0)
    # the restatement with the parameters handed in: the rows the reference left
    scale = (224 / 640, 224 / 480) if case["cfg"].get("reshape") else (1.0, 1.0)
    rows = nf.host_rows(x, y, t, p, par[0], sx=scale[0], sy=scale[1], train=case["mode"] == "train")
    assert_rows_equal(rows.numpy(), _G[case["name"] + ".out"], case["name"])


def test_a_batch_is_drawn_as_sequential_reference_calls_draw():
    """B windows: the draws of window b are those of the b-th of B sequential calls -- np.random per window in the order
    random(), random(), randint(size=2); Python's random per window randint (slice_augment, train) then choice (n > length)."""
    from event_representation_study_amd import n_imagenet_front as nf
    cfg = types.SimpleNamespace(slice_events=True, slice_method="random", slice_length=300, slice_augment=True,
                                slice_augment_width=50, mode="train")
    lengths = [1000, 200, 351, 349, 5000]
    seed_both(77)
    sl, au = nf.draw_slice(lengths, cfg), nf.draw_augment(len(lengths), "train")
    after = state_digests()
    seed_both(77)
    for b, n in enumerate(lengths):
        length = random.randint(250, 350)
        s0, s1 = (0, n)
        if n > length:
            s0 = random.choice(range(n - length + 1))
            s1 = s0 + length
        assert (int(sl["s0"][b]), int(sl["s1"][b])) == (s0, s1)
    for b in range(len(lengths)):
        assert bool(au["time_flip"][b]) == (np.random.random() < 0.5)
        assert bool(au["x_flip"][b]) == (np.random.random() < 0.5)
        assert [int(au["x_shift"][b]), int(au["y_shift"][b])] == np.random.randint(-20, 21, size=(2,)).tolist()
    assert state_digests() == after
    seed_both(3)
    before = state_digests()
    au = nf.draw_augment(4, "eval")
    assert state_digests() == before and not au["time_flip"].any() and not au["x_shift"].any()     # eval draws nothing


def test_in_place_side_effects_are_the_references():
    """The no-flip path works on the caller's tensor (the x flip and the shift are written into it); the time flip returns a
    copy and leaves the caller's tensor alone.  The time slice copies, the index slice is a view."""
    from event_representation_study_amd import n_imagenet_front as nf
    ev0 = torch.tensor([[10.0, 10.0, 0.1, 1.0], [50.0, 60.0, 0.2, -1.0], [223.0, 5.0, 0.4, 1.0]], dtype=torch.float64)
    ev = ev0.clone()
    out = nf.apply_augment(ev, False, True, 3, -6)
    assert torch.equal(ev[:, 0], 223 - ev0[:, 0] + 3) and torch.equal(ev[:, 1], ev0[:, 1] - 6)
    assert out.shape[0] == 2 and out.data_ptr() != ev.data_ptr()
    ev = ev0.clone()
    out = nf.apply_augment(ev, True, False, 0, 0)
    assert torch.equal(ev, ev0)
    assert out[:, 2].tolist() == [0.0, 0.4 - 0.2, 0.4 - 0.1] and out[:, 3].tolist() == [-1.0, 1.0, -1.0]
    view = nf.slice_event(ev, types.SimpleNamespace(slice_method="idx", slice_start=1, slice_end=None))
    assert view.data_ptr() == ev[1:].data_ptr()
    copy = nf.slice_event(ev, types.SimpleNamespace(slice_method="time", slice_start=0.0, slice_end=1.0))
    assert copy.data_ptr() != ev.data_ptr() and torch.equal(copy, ev)
    rs = nf.reshape_event_no_sample(ev, 480, 640, 224, 224)
    assert rs is ev and ev[1, 0].item() == 50.0 * (224 / 640)
    with pytest.raises(IndexError):
        nf.time_flipped(ev[:0])                      # event_tensor[0, 2] of an empty slice, imagenet.py:1169


def test_what_is_not_built_says_so():
    from event_representation_study_amd import n_imagenet_front as nf
    ev = torch.zeros((4, 4), dtype=torch.float64)
    for fn in (nf.reshape_event_with_sample, nf.reshape_event_unique):
        with pytest.raises(NotImplementedError):
            fn(ev, 480, 640, 224, 224)
    for method in ("sample", "unique"):
        with pytest.raises(NotImplementedError):
            nf.NImageNetFrontEnd(types.SimpleNamespace(reshape=True, reshape_method=method), "train")
    with pytest.raises(AssertionError):
        nf.base_augment("test")
    with pytest.raises(TypeError):
        nf.draw_slice([10], types.SimpleNamespace(slice_events=True, slice_method="time", slice_start=None, slice_end=1.0))


def test_no_cpu_fallback():
    from event_representation_study_amd import _lib, n_imagenet_front as nf
    if torch.cuda.is_available():
        return                      # a HIP device is visible: test_gpu_nimg_front.py covers the path
    with pytest.raises(_lib.EvrepError):
        nf.NImageNetFrontEnd(types.SimpleNamespace(reshape=True), "train")


@pytest.fixture(scope="module")
def lib():
    from event_representation_study_amd import build, _lib
    build.build()
    return _lib.load()


def _p(v):
    return ctypes.c_void_p(v)


def test_nimg_prepare_refuses_bad_arguments_before_any_launch(lib):
    from event_representation_study_amd import n_imagenet_front as nf
    from event_representation_study_amd._lib import EVREP_EINVAL, EVREP_OK, NIMG_P_UINT8, NIMG_TRAIN
    f = lib.evrep_nimg_prepare
    #     events   offsets  B  t_base    params    sx   sy   h    w    mode                       ev_out     t_out      tnorm      xy         off_out    status     scratch    stream
    ok = (_p(256), _p(512), 4, _p(1024), _p(2048), 0.35, 0.5, 224, 224, NIMG_TRAIN | NIMG_P_UINT8, _p(4096), _p(8192), _p(16384), _p(32768), _p(65536), _p(1 << 17), _p(1 << 18), None)
    bad = [(0, None), (0, _p(264)), (1, None), (1, _p(516)), (2, -1), (2, (1 << 24) + 1), (3, _p(1028)), (4, None), (4, _p(2052)),
           (5, 0.0), (5, -1.0), (5, float("nan")), (5, float("inf")), (6, 0.0), (6, float("nan")), (7, 0), (7, 4097), (8, 0), (8, 4097),
           (9, 4), (9, 0xFFFFFFFF), (10, None), (10, _p(4104)), (11, None), (11, _p(8196)), (12, None), (12, _p(16388)),
           (13, _p(32776)), (14, None), (14, _p(65540)), (15, None), (15, _p((1 << 17) + 2)), (16, None), (16, _p((1 << 18) + 8))]
    for i, v in bad:
        args = list(ok)
        args[i] = v
        assert f(*args) == EVREP_EINVAL, (i, v)
    for i, v in ((2, 0), ):                                          # no window: nothing to launch
        args = list(ok)
        args[i] = v
        assert f(*args) == EVREP_OK
    args = list(ok)
    args[2], args[3], args[13] = 0, None, None                       # t_base and xy_out are optional
    assert f(*args) == EVREP_OK
    sb = lib.evrep_nimg_prepare_scratch_bytes
    assert sb(0, 10) == 0 and sb(-1, 10) == 0 and sb(4, -1) == 0 and sb((1 << 24) + 1, 0) == 0
    assert sb(1, 0) >= 4 * 1025 + 44 and sb(1, 0) % 256 == 0 and sb(1000, 5) >= 4 * 1025 + 1000 * 44
    assert sb(7, 0) == sb(7, 1 << 40)                                # sized by the windows, not by the rows
    assert nf.PARAMS_DTYPE.itemsize == 48 and nf.PARAMS_DTYPE.fields["flags"][1] == 40      # struct evrep_nimg_params
