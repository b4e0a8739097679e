"""GPU: the batched sorted timestamp image on the device (evrep_time_index / evrep_sort_image, csrc/evrep_sort.hip).

Everything is BIT-EQUAL: sort_batch to the images the reference's reshape_then_acc_sort wrote (tests/golden/nimg_sort.npz),
sort_device to sort_batch on the host-augmented rows, evrep_time_index to numpy, evrep_sort_image on synthetic (B, H, W, 2K) tensors
to the numpy restatement that tests/test_sort_cpu.py pins against those same images.  The torch route reshape_then_acc_sort
is the second comparator, exact on the golden windows whose indices stay below 2^24 (its quantisation divides as the reference's
does since this test showed its q = 255 images one ulp off; the route is otherwise unchanged).

Shapes: windows around the wave (64) and the 1 024-event tile of a time-index slice, one window of several tiles per slice; frames
of one pixel, less than a wave, ragged, and the workload's 224x224 with 0 to all 50 176 pixels hot.
"""
import ctypes
import json
import random
import types

import numpy as np
import pytest
import torch

from conftest import assert_bit_equal, load_golden
from test_sort_cpu import (CASES, DECREASING, EMPTY, IDS, NO_INDEX, _G, case_events, sort_from_prim, sort_image, time_index,
                           time_status, time_values)

pytestmark = pytest.mark.gpu
F32 = np.float32
TILE = 1024          # kTiThreads: the events one workgroup takes per round of its slice
SLICES = 256         # kTiSlices


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _sp():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def kw_key(c):
    return (c["H"], c["W"], json.dumps(c["kw"], sort_keys=True))


# ------------------------------------------------------------------------------------------------ the reference's images
@pytest.fixture(scope="module")
def golden_batches():
    """sort_batch once per frame size and keyword set, over every stream that has such a case: {name: image}."""
    from event_representation_study_amd import n_imagenet_acc as ni
    groups, got = {}, {}
    for c in CASES:
        groups.setdefault(kw_key(c), []).append(c)
    for cs in groups.values():
        H, W, kw = cs[0]["H"], cs[0]["W"], cs[0]["kw"]
        tensors = [torch.from_numpy(case_events(c).copy()) for c in cs]
        res = ni.sort_batch(tensors, height=H, width=W, **kw)
        assert res.dtype == torch.float32 and res.is_cuda and res.is_contiguous() and tuple(res.shape[2:]) == (H, W) and len(res) == len(cs)
        for c, t in zip(cs, tensors):
            assert np.array_equal(t.numpy(), case_events(c)), "sort_batch wrote into the caller's tensor"
        for c, img in zip(cs, res.cpu().numpy()):
            got[c["name"]] = img
    assert any(len(cs) >= 5 for cs in groups.values())          # real batches, not one window per call
    return got


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_sort_batch_equals_the_reference_image(golden_batches, case):
    assert_bit_equal(golden_batches[case["name"]], _G[case["name"] + ".image"], case["name"])


def test_late_window_case_bites(golden_batches):
    """global_time=False, strict=True, 20 s in: two pixels' latest indices differ by 1 us and agree in float32; the image keeps
    them apart as the reference's does."""
    c = next(c for c in CASES if c["stream"] == "late" and c["kw"]["strict"] and not c["kw"]["global_time"] and c["kw"]["neglect_polarity"])
    ev = case_events(c)
    a, b = (int(v) for v in _G["late.pixels"])
    idx, pix = time_index(ev[:, 2]), ev[:, 0].astype(np.int64) + ev[:, 1].astype(np.int64) * c["W"]
    la, lb = int(idx[pix == a].max()), int(idx[pix == b].max())
    assert lb - la == 1 and F32(la) == F32(lb) and la > 1 << 24
    img = golden_batches[c["name"]][-1].reshape(-1)
    assert img[a] < img[b]
    assert_bit_equal(golden_batches[c["name"]], _G[c["name"] + ".image"], c["name"])


def test_sort_batch_agrees_with_the_unchanged_torch_route(golden_batches):
    """Exact on every golden window whose indices stay below 2^24 (all streams but ``epoch`` and ``late``)."""
    from event_representation_study_amd import n_imagenet_acc as ni
    bad, seen = [], 0
    for c in CASES:
        ev = case_events(c)
        if time_index(ev[:, 2]).max() >= 1 << 24:
            continue
        seen += 1
        old = ni.reshape_then_acc_sort(torch.from_numpy(ev.copy()), height=c["H"], width=c["W"], denoise_image=False, denoise_sort=False,
                                       **c["kw"]).numpy()
        new = golden_batches[c["name"]]
        if old.shape != new.shape or not np.array_equal(old, new):
            n = int((old != new).sum()) if old.shape == new.shape else -1
            worst = float(np.abs(old - new).max()) if old.shape == new.shape else float("nan")
            print("torch route differs: %s, %d values, max |diff| %g" % (c["name"], n, worst))
            bad.append(c["name"])
    assert seen >= 40 and {c["stream"] for c in CASES if c["name"] not in bad} >= {"base", "ties", "trunc", "index0", "flipped"}
    assert not bad, bad


def test_accumulate_device_still_has_no_acc_sort():
    from event_representation_study_amd import n_imagenet_acc as ni, n_imagenet_front as nf
    assert "acc_sort" not in ni.SPECS
    with pytest.raises(KeyError):
        nf.accumulate_device("acc_sort", None)
    with pytest.raises(KeyError):
        ni.accumulate_batch("acc_sort", [np.zeros((1, 4))])


def big_stream(n, H, W, seed, base=3_000_000, span=50_000):
    rng = np.random.default_rng(seed)
    ev = np.zeros((n, 4))
    ev[:, 0], ev[:, 1] = rng.integers(0, W, n), rng.integers(0, H, n)
    ev[:, 2] = (np.sort(rng.integers(0, span, n)) + base) / 1e6
    ev[:, 3] = rng.choice((-1, 1), n)
    return ev


@pytest.mark.parametrize("kw", [dict(global_time=True, neglect_polarity=False, use_image=True, strict=True, quantize_sort=[2, 8, 255]),
                                dict(global_time=False, neglect_polarity=True, use_image=False, strict=True, quantize_sort=None),
                                dict(global_time=False, neglect_polarity=False, use_image=True, strict=False, quantize_sort=4),
                                dict(global_time=True, neglect_polarity=True, use_image=True, strict=False, quantize_sort=None)],
                         ids=["strict_list", "strict_raw", "loose_raw", "loose_rank"])
def test_sort_batch_224_equals_the_restatement(kw):
    """The workload's frame: three windows of different lengths, the second 25 s into its recording."""
    from event_representation_study_amd import n_imagenet_acc as ni
    wins = [big_stream(10_000, 224, 224, 31), big_stream(30_000, 224, 224, 32, base=25_000_000), big_stream(700, 224, 224, 33)]
    got = ni.sort_batch(wins, **kw).cpu().numpy()
    for b, ev in enumerate(wins):
        want, status = sort_image(ev, 224, 224, **kw)
        assert status == 0
        assert_bit_equal(got[b], want, "window %d" % b)
    assert len(np.unique(got[1])) > 100


# ------------------------------------------------------------------------------------------------ the time index alone
def device_time_index(windows, mode):
    """evrep_time_index on a list of float64 time arrays -> (list of float64 arrays, status)."""
    from event_representation_study_amd import _lib
    lib = _lib.load()
    B = len(windows)
    off = np.zeros(B + 1, np.int64)
    np.cumsum([len(w) for w in windows], out=off[1:])
    total = int(off[-1])
    t = torch.from_numpy(np.concatenate(windows).astype(np.float64)).cuda()
    d_off = torch.from_numpy(off).cuda()
    out = torch.full((total,), -7.0, dtype=torch.float64, device="cuda")
    status = torch.full((B,), 0xFFFF, dtype=torch.int32, device="cuda")
    nbytes = int(lib.evrep_time_index_scratch_bytes(B, total))
    assert nbytes > 0
    scratch = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda")          # no initialisation needed
    _lib.check(lib.evrep_time_index(_p(t), _p(d_off), B, mode, _p(out), _p(status), _p(scratch), _sp()), "evrep_time_index")
    res = out.cpu().numpy()
    return [res[off[b]:off[b + 1]] for b in range(B)], status.cpu().numpy().astype(np.uint32)


def check_time_index(windows, what, decreasing=()):
    for mode in (1, 0):
        got, status = device_time_index(windows, mode)
        for b, w in enumerate(windows):
            assert int(status[b]) == time_status(w), (what, mode, b)
            if b not in decreasing:
                assert_bit_equal(got[b], time_values(w, rank=bool(mode)), "%s mode %d window %d (%d events)" % (what, mode, b, len(w)))


def stamps(rng, n, lo=3_000_000, step=3):
    """n sorted stamps k / 1e6 with ties (a third of the steps are 0)."""
    return (lo + np.cumsum(rng.integers(0, step, n))) / 1e6


def test_time_index_window_lengths_in_one_call():
    rng = np.random.default_rng(41)
    lengths = [1, 63, 64, 65, 0, TILE - 1, TILE, TILE + 1, 3, 0, 0, 200]
    wins = [stamps(rng, n) for n in lengths]
    assert time_status(wins[4]) == EMPTY
    check_time_index(wins, "lengths")


def test_time_index_restarts_at_equal_window_boundaries():
    """The last index of a window equals the first of the next (twice, once across an empty window); a window on one index; a
    decreasing window, whose status bit alone is checked, between two good ones."""
    rng = np.random.default_rng(42)
    a = stamps(rng, 700)
    b = np.concatenate([[a[-1]] * 3, stamps(rng, 500, lo=int(round(a[-1] * 1e6)))])
    c = np.full(300, b[-1])
    d = np.concatenate([[c[-1]], stamps(rng, 90, lo=int(round(c[-1] * 1e6)) + 5)])
    bad = stamps(rng, 400)[::-1].copy()
    e = stamps(rng, 130)
    wins = [a, b, np.zeros(0), c, d, bad, e]
    assert time_index(a)[-1] == time_index(b)[0] and time_index(c)[-1] == time_index(d)[0] == time_index(b)[-1]
    assert time_status(bad) == DECREASING and time_values(c, True).max() == 0
    check_time_index(wins, "boundaries", decreasing=(5,))


def test_time_index_several_tiles_per_slice():
    """700 001 + 5 000 + 1 events over 256 slices: 2 758 per slice, two tiles and a remainder each; a slice straddles the windows."""
    rng = np.random.default_rng(43)
    wins = [stamps(rng, 700_001, step=2), stamps(rng, 5_000), stamps(rng, 1)]
    assert sum(map(len, wins)) // SLICES > 2 * TILE
    check_time_index(wins, "tiles")


def test_time_index_truncates_the_float64_product():
    ks = np.array([k for k in range(1, 200_000) if int(np.float64(k) / 1e6 * 1e6) == k - 1][:200], np.int64)
    w = np.sort(np.concatenate([ks, ks - 1])) / 1e6
    assert (time_index(w) != np.rint(w * 1e6)).sum() >= 100
    check_time_index([w, stamps(np.random.default_rng(44), 50, lo=1_600_000_000_000_000)], "truncation")


# ------------------------------------------------------------------------------------------------ synthetic prim tensors
def device_sort_image(prim, strict, use_image, qs):
    """evrep_sort_image on a host (B, H, W, 2K) array -> host ((B, C, H, W), status)."""
    from event_representation_study_amd import _lib
    lib = _lib.load()
    B, H, W, C2 = prim.shape
    K = C2 // 2
    d_prim = torch.from_numpy(np.ascontiguousarray(prim, F32)).cuda()
    out = torch.full((B, K * (int(use_image) + max(len(qs), 1)), H, W), -1.0, dtype=torch.float32, device="cuda")
    status = torch.zeros(B, dtype=torch.int32, device="cuda")
    nbytes = int(lib.evrep_sort_image_scratch_bytes(B, H, W, K))
    assert nbytes > 0
    scratch = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda")
    flags = (_lib.SORT_STRICT if strict else 0) | (_lib.SORT_USE_IMAGE if use_image else 0)
    _lib.check(lib.evrep_sort_image(_p(d_prim), B, H, W, K, flags, _lib.int32_array(qs) if qs else None, len(qs), _p(out), _p(status),
                                    _p(scratch), _sp()), "evrep_sort_image")
    return out.cpu().numpy(), status.cpu().numpy().astype(np.uint32)


def synth_class(rng, H, W, nhot, U):
    """One class's (H, W, 2) [FLAG, TMAX]: nhot hot pixels holding U distinct integer ranks (each at least once), the smallest
    of them 0 when U > 1 is odd-seeded -- a hot pixel whose TMAX is 0 is not a pixel without an event."""
    flag, tmax = np.zeros(H * W, F32), np.zeros(H * W, F32)
    hot = rng.permutation(H * W)[:nhot]
    if nhot:
        values = np.sort(rng.choice(np.arange(0 if U % 2 else 1, 4 * U + 1), U, replace=False))
        pick = np.concatenate([np.arange(U), rng.integers(0, U, nhot - U)])
        flag[hot], tmax[hot] = 1.0, values[rng.permutation(pick)].astype(F32)
    return np.stack([flag, tmax], axis=1).reshape(H, W, 2)


# frame, hot pixels, distinct latest indices
PRIM_CASES = [(1, 1, 0, 0), (1, 1, 1, 1), (5, 7, 2, 2), (5, 7, 35, 9), (17, 70, 64, 64), (17, 70, 1024, 9), (17, 70, 1190, 1),
              (224, 224, 4096, 4096), (224, 224, 1024, 300), (224, 224, 50176, 50176), (224, 224, 50176, 17), (224, 224, 0, 0)]
# strict, use_image, quantisations, classes: U - 1 = 8 or 16 with q = 4 and 2 puts rank * q / (U - 1) on .5 ties
CONFIGS = [(True, True, [2, 8, 255], 2), (True, False, [], 1), (True, True, [4], 1), (False, True, [2, 8], 2), (False, False, [], 1)]


@pytest.mark.parametrize("H,W,nhot,U", PRIM_CASES)
def test_evrep_sort_image_equals_the_restatement(H, W, nhot, U):
    rng = np.random.default_rng(100 * H + nhot + U)
    other = synth_class(rng, H, W, min(H * W, 40), min(H * W, 17))
    for strict, use_image, qs, K in CONFIGS:
        main = synth_class(rng, H, W, nhot, U)
        # three windows: the case in the first class, in the second class, and in both
        wins = [np.concatenate([main] + [other] * (K - 1), axis=2), np.concatenate([other] * (K - 1) + [main], axis=2),
                np.concatenate([main] * K, axis=2)]
        got, status = device_sort_image(np.stack(wins), strict, use_image, qs)
        for b, prim in enumerate(wins):
            want, st = sort_from_prim(prim, strict, use_image, qs)
            assert int(status[b]) == st, (strict, K, b)
            assert_bit_equal(got[b], want, "%dx%d hot %d U %d strict %d K %d window %d" % (H, W, nhot, U, strict, K, b))
        if strict and U in (9, 17) and qs and qs[0] in (2, 4):
            m = sort_from_prim(wins[-1], True, False, [])[0][0] * F32(qs[0])
            assert (np.abs(m - np.floor(m) - 0.5) == 0).any()                       # a quantisation did land on a tie


def test_evrep_sort_image_status_bits_are_ored_per_class():
    """strict=False: a class none of whose pixels holds a positive index sets its own bit, on top of what the word holds."""
    rng = np.random.default_rng(7)
    live = synth_class(rng, 6, 9, 20, 5)
    flat = live.copy()
    flat[..., 1] = 0                                                                # events, but every latest index is 0
    dead = np.zeros_like(live)
    wins = [np.concatenate(p, axis=2) for p in ((live, live), (live, flat), (dead, live), (flat, dead))]
    _, status = device_sort_image(np.stack(wins), False, True, [])
    assert status.tolist() == [0, NO_INDEX << 1, NO_INDEX, NO_INDEX | NO_INDEX << 1]
    got, status = device_sort_image(np.stack(wins), True, True, [])
    assert not status.any()
    assert got[2, 0, 0, 0] == 1.0 and got[2, 0].sum() == 1.0 and not got[2, 1].any()     # the stand-in event of the empty class


# ------------------------------------------------------------------------------------------------ device-made rows
_F = load_golden("nimg_front")
FRONT_CASES = json.loads(str(_F["manifest"]))


def columns(case):
    return tuple(_F["stream%d.%s" % (case["stream"], k)] for k in "xytp")


def packed(x, y, t, p):
    base = int(t[0]) if len(t) else 0
    return np.stack([x.astype(np.int32), y.astype(np.int32), (t - base).astype(np.int32), p.astype(np.int32)], axis=1).reshape(-1, 4), base


def make_batch(windows, H, W):
    from event_representation_study_amd.engine import EventBatch
    rows, bases = zip(*(packed(*w) for w in windows))
    return EventBatch.from_numpy(list(rows), H, W), np.asarray(bases, np.int64)


@pytest.fixture(scope="module")
def front_batch():
    """The flip_00 / flip_11 / flip_10 windows of nimg_front.npz as one AugmentedBatch, and their host-mirror rows."""
    from event_representation_study_amd import n_imagenet_front as nf
    sel = [c for c in FRONT_CASES if c["name"] in ("flip_00", "flip_11", "flip_10")]
    assert len(sel) == 3
    pars = []
    for c in sel:
        np.random.seed(c["seed"])
        random.seed(c["seed"])
        front = nf.NImageNetFrontEnd(types.SimpleNamespace(**c["cfg"]), "train")
        pars.append(front.draw([len(columns(c)[0])]))
    wins = [columns(c) for c in sel]
    par = np.concatenate(pars)
    batch, base = make_batch(wins, 480, 640)
    aug = front.prepare(batch, t_base=base, params=par)
    rows = [nf.host_rows(*w, par[b], sx=front.sx, sy=front.sy, train=True) for b, w in enumerate(wins)]
    return aug, rows


@pytest.mark.parametrize("kw", [dict(global_time=True, neglect_polarity=False, use_image=True, strict=True, quantize_sort=[2, 8, 255]),
                                dict(global_time=False, neglect_polarity=True, use_image=True, strict=True, quantize_sort=None),
                                dict(global_time=False, neglect_polarity=False, use_image=False, strict=False, quantize_sort=None),
                                dict(global_time=True, neglect_polarity=True, use_image=True, strict=False, quantize_sort=4)],
                         ids=["strict_list", "strict_raw", "loose_raw", "loose_rank"])
def test_sort_device_equals_sort_batch_on_the_host_mirror_rows(front_batch, kw):
    from event_representation_study_amd import n_imagenet_acc as ni, n_imagenet_front as nf
    aug, rows = front_batch
    got = nf.sort_device(aug, **kw)
    want = ni.sort_batch([r.clone() for r in rows], **kw)
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == tuple(want.shape) and got.shape[0] == 3
    assert_bit_equal(got.cpu().numpy(), want.cpu().numpy(), "sort_device")
    assert len(np.unique(got.cpu().numpy())) > 100
    images, status = nf.sort_device(aug, check=False, **kw)
    assert status.is_cuda and status.cpu().numpy().tolist() == [0, 0, 0]
    assert_bit_equal(images.cpu().numpy(), want.cpu().numpy(), "check=False")


def test_sort_device_refusals():
    from event_representation_study_amd import _lib, n_imagenet_front as nf
    rng = np.random.default_rng(3)

    def win(n, pol=(0, 1)):
        t = (np.sort(rng.integers(0, 40_000, n)) + 3_000_000_000).astype(np.int64)
        return rng.integers(0, 224, n).astype(np.uint16), rng.integers(0, 224, n).astype(np.uint16), t, rng.choice(pol, n).astype(np.int8)

    kw = dict(global_time=True, neglect_polarity=False, use_image=True)
    front = nf.NImageNetFrontEnd(types.SimpleNamespace(mode="val"), "eval")
    good = win(50)
    batch, base = make_batch([good, win(0), good], 224, 224)
    aug = front.prepare(batch, t_base=base)
    assert aug.status.tolist() == [0, _lib.AUG_EMPTY, 0]
    for strict in (False, True):
        with pytest.raises(RuntimeError, match=r"max\(\).*sample 1"):
            nf.sort_device(aug, strict=strict, **kw)
    # a window of positive events only: strict=False has no negative index to take the maximum of
    batch, base = make_batch([good, good, win(40, pol=(1,))], 224, 224)
    aug = front.prepare(batch, t_base=base)
    assert not aug.status.any()
    with pytest.raises(RuntimeError, match=r"max\(\).*sample 2"):
        nf.sort_device(aug, strict=False, **kw)
    images, status = nf.sort_device(aug, strict=False, check=False, **kw)
    assert status.cpu().numpy().tolist() == [0, 0, NO_INDEX << 1] and tuple(images.shape) == (3, 4, 224, 224)
    assert tuple(nf.sort_device(aug, strict=True, **kw).shape) == (3, 4, 224, 224)          # the stand-in event: no refusal
    assert tuple(nf.sort_device(aug, strict=False, **dict(kw, neglect_polarity=True)).shape) == (3, 2, 224, 224)
    with pytest.raises(NameError):
        nf.sort_device(aug, strict=True, denoise_sort=True, **kw)
