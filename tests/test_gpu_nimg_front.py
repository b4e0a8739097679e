"""GPU: N-ImageNet's event front end on the device (evrep_nimg_prepare, csrc/evrep_augment.hip) against
tests/golden/nimg_front.npz -- outputs of the reference's own parse_event + base_augment -- and against the host mirrors of
event_representation_study_amd/n_imagenet_front.py on synthetic batches whose sizes sit at the edges of the kernel's partition
(1024 slices of the concatenated rows, 1024 lanes per round, 64 lanes per wave).  Everything is bit-equal: int32 rows, float64
t / tnorm / xy (NaN where the reference has NaN), offsets and status words.  The eleven accumulators built from the device
rows are bit-equal to accumulate_batch on the host-augmented tensors, and equal to the reference's recorded images within the
tolerance test_nimagenet_acc_against_reference_goldens uses (bit-exact; rtol 1e-5 for acc_exp).
"""
import json
import random
import types

import numpy as np
import pytest
import torch

from conftest import assert_bit_equal, load_golden

pytestmark = pytest.mark.gpu

_G = load_golden("nimg_front")
CASES = json.loads(str(_G["manifest"]))
IDS = [c["name"] for c in CASES]
NOSHAPE = types.SimpleNamespace(mode="train")                       # coordinates already on the 224x224 frame
RESHAPE = types.SimpleNamespace(reshape=True, mode="train")


def columns(case):
    return tuple(_G["stream%d.%s" % (case["stream"], k)] for k in "xytp")


def packed(x, y, t, p):
    """The int32 rows evrep_windows_gather writes (rebased to the first event) and their base."""
    base = int(t[0]) if len(t) else 0
    return np.stack([x.astype(np.int32), y.astype(np.int32), (t - base).astype(np.int32), p.astype(np.int32)], axis=1).reshape(-1, 4), base


def same(got, want, what):
    """Bit-equal; NaNs compare as NaN."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype.kind == "f":
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), what + ": NaN pattern"
        got, want = np.where(nan, 0, got), np.where(nan, 0, want)
    assert_bit_equal(got, want, what)


def expected(rows_list):
    """What evrep_nimg_prepare leaves for windows whose augmented float64 rows are rows_list."""
    from event_representation_study_amd import _lib
    ev, t, tn, xy, st = [], [], [], [], []
    for r in rows_list:
        r = np.asarray(r, dtype=np.float64).reshape(-1, 4)
        e = np.zeros((len(r), 4), np.int32)
        e[:, 0], e[:, 1], e[:, 3] = r[:, 0].astype(np.int64), r[:, 1].astype(np.int64), np.sign(r[:, 3])
        ev.append(e)
        t.append(r[:, 2])
        xy.append(r[:, :2])
        with np.errstate(divide="ignore", invalid="ignore"):
            tn.append((r[:, 2] - r[0, 2]) / (r[-1, 2] - r[0, 2]) if len(r) else np.zeros(0))          # imagenet.py:198-199
        st.append(_lib.AUG_EMPTY if len(r) == 0 else (_lib.AUG_FLAT_TIME if r[-1, 2] == r[0, 2] else 0))
    off = np.zeros(len(rows_list) + 1, np.int64)
    np.cumsum([len(e) for e in ev], out=off[1:])
    return dict(events=np.concatenate(ev), t=np.concatenate(t), tnorm=np.concatenate(tn), xy=np.ascontiguousarray(np.concatenate(xy)),
                offsets=off, status=np.asarray(st, np.uint32))


def check(aug, want, what):
    same(aug.batch.offsets_host, want["offsets"], what + " offsets")
    same(aug.status, want["status"], what + " status")
    same(aug.counts, np.diff(want["offsets"]), what + " counts")
    same(aug.batch.events, want["events"], what + " events")
    same(aug.t, want["t"], what + " t")
    same(aug.xy, want["xy"], what + " xy")
    same(aug.tnorm, want["tnorm"], what + " tnorm")


def make_batch(windows, H, W):
    """[(x, y, t, p)] -> EventBatch of the packed rows, t_base."""
    from event_representation_study_amd.engine import EventBatch
    rows, bases = zip(*(packed(*w) for w in windows))
    return EventBatch.from_numpy(list(rows), H, W), np.asarray(bases, np.int64)


def host(front, windows, par):
    """The host mirrors, window by window.  A time flip of an EMPTY slice raises IndexError in the reference (event_tensor[0, 2],
    imagenet.py:1169) and in the mirror; the device reports such a window as EVREP_AUG_EMPTY, on which accumulate_device raises
    the IndexError: its expected rows are none."""
    from event_representation_study_amd import _lib, n_imagenet_front as nf
    out = []
    for b, w in enumerate(windows):
        if len(w[0]) == 0:
            out.append(np.zeros((0, 4)))
            continue
        try:
            out.append(nf.host_rows(*w, par[b], sx=front.sx, sy=front.sy, train=front.mode == "train").numpy())
        except IndexError:
            assert int(par["flags"][b]) & _lib.AUG_TIME_FLIP
            out.append(np.zeros((0, 4)))
    return out


# ------------------------------------------------------------------------------------------ the reference's recorded outputs
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_device_path_equals_the_reference(case):
    """Seeded as the reference was: prepare() draws the parameters itself."""
    from event_representation_study_amd import n_imagenet_front as nf
    cols = columns(case)
    batch, base = make_batch([cols], 480, 640)
    front = nf.NImageNetFrontEnd(types.SimpleNamespace(**case["cfg"]), case["mode"])
    np.random.seed(case["seed"])
    random.seed(case["seed"])
    aug = front.prepare(batch, t_base=base)
    check(aug, expected([_G[case["name"] + ".out"]]), case["name"])
    assert (aug.batch.H, aug.batch.W, aug.batch.B) == (224, 224, 1)


def test_all_recorded_cases_in_one_batch():
    """The train-mode, reshaped cases as ONE batch with the recorded parameters: windows side by side, flipped and not."""
    from event_representation_study_amd import n_imagenet_front as nf
    sel = [c for c in CASES if c["mode"] == "train" and c["cfg"].get("reshape")]
    assert len(sel) >= 20
    pars = []
    for c in sel:
        np.random.seed(c["seed"])
        random.seed(c["seed"])
        front = nf.NImageNetFrontEnd(types.SimpleNamespace(**c["cfg"]), "train")
        pars.append(front.draw([len(columns(c)[0])]))
    batch, base = make_batch([columns(c) for c in sel], 480, 640)
    aug = front.prepare(batch, t_base=base, params=np.concatenate(pars))
    check(aug, expected([_G[c["name"] + ".out"] for c in sel]), "recorded batch")


# ------------------------------------------------------------------------------------------ the edges of the partition
def synthetic(n, rng, W=224, H=224, t0=3_000_000_000, pol=(0, 1)):
    x, y = rng.integers(0, W, n).astype(np.uint16), rng.integers(0, H, n).astype(np.uint16)
    t = (np.sort(rng.integers(0, 40_000, n)) + t0).astype(np.int64)
    return x, y, t, rng.choice(pol, n).astype(np.int8)


def params(nf, lengths, rng, time_flip=None, x_flip=None, shifts=None):
    B = len(lengths)
    sl = nf.draw_slice(lengths, types.SimpleNamespace())
    au = dict(time_flip=rng.integers(0, 2, B).astype(bool) if time_flip is None else np.asarray(time_flip, bool),
              x_flip=rng.integers(0, 2, B).astype(bool) if x_flip is None else np.asarray(x_flip, bool),
              x_shift=rng.integers(-20, 21, B).astype(np.int32), y_shift=rng.integers(-20, 21, B).astype(np.int32))
    if shifts is not None:
        au["x_shift"][:], au["y_shift"][:] = np.asarray(shifts, np.int32).T
    return nf.pack_params(sl, au)


def test_mixed_batch_at_the_partition_edges():
    from event_representation_study_amd import _lib, n_imagenet_front as nf
    rng = np.random.default_rng(5)
    lengths = [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 3000]
    wins = [synthetic(n, rng) for n in lengths]
    shifts = [(0, 0), (0, 0), (20, -20), (-20, 20), (0, 0), (20, 20), (-20, -20), (0, 20), (-20, 0), (20, 0)]
    flips = [0, 1, 1, 0, 1, 0, 1, 0, 1, 1]
    # a window cropped away entirely: every x below 20, shift -20
    gone = synthetic(500, rng)
    gone[0][:] = rng.integers(0, 20, 500)
    # one kept row, landing exactly on x'' == 0
    one = synthetic(300, rng)
    one[0][:] = rng.integers(0, 20, 300)
    one[0][137] = 20
    # rows landing exactly on x'' == 0 and just below res_w: x = 20, 223 (shift -20 -> 0, 203), x = 203, 204 (shift +20 -> 223, 224)
    edge_lo, edge_hi = synthetic(200, rng), synthetic(200, rng)
    edge_lo[0][:] = rng.choice([19, 20, 21, 223], 200)
    edge_hi[0][:] = rng.choice([0, 202, 203, 204], 200)
    edge_hi[1][:] = rng.choice([0, 203, 204, 223], 200)
    wins += [gone, wins[9], one, edge_lo, edge_hi, synthetic(0, rng), synthetic(70, rng)]
    shifts += [(-20, 3), (0, 0), (-20, 0), (-20, 0), (20, 20), (1, 1), (5, -5)]
    flips += [1, 0, 1, 0, 1, 0, 0]
    lengths = [len(w[0]) for w in wins]
    par = params(nf, lengths, rng, time_flip=flips, shifts=shifts)
    front = nf.NImageNetFrontEnd(NOSHAPE, "train")
    batch, base = make_batch(wins, 224, 224)
    aug = front.prepare(batch, t_base=base, params=par)
    want = expected(host(front, wins, par))
    check(aug, want, "mixed batch")
    E, F = _lib.AUG_EMPTY, _lib.AUG_FLAT_TIME
    assert aug.status[0] == E and aug.status[10] == E and aug.status[15] == E
    assert aug.batch.offsets_host[10] == aug.batch.offsets_host[11]                       # equal neighbouring offsets
    assert aug.counts[12] == 1 and aug.status[12] == F and bool(torch.isnan(aug.tnorm[aug.batch.offsets_host[12]]))
    assert aug.xy[int(aug.batch.offsets_host[12]), 0].item() == 0.0
    xs = aug.xy[:, 0].cpu().numpy()
    assert xs.min() == 0.0 and xs.max() == 223.0
    # the same call again: identical bytes
    again = front.prepare(batch, t_base=base, params=par)
    for a, b in ((aug.batch.events, again.batch.events), (aug.t, again.t), (aug.tnorm, again.tnorm), (aug.xy, again.xy)):
        assert np.array_equal(a.cpu().numpy().view(np.uint8), b.cpu().numpy().view(np.uint8))
    # without xy_out
    lean = front.prepare(batch, t_base=base, params=par, want_xy=False)
    assert lean.xy is None and torch.equal(lean.batch.events, aug.batch.events) and torch.equal(lean.t, aug.t)
    with pytest.raises(IndexError, match="sample 0"):
        nf.accumulate_device("acc_all", aug)


def test_slices_and_absolute_times_on_a_reshaped_batch():
    """640x480 -> 224x224 with index slices, strict time slices on timestamps that occur, flips, and bases near 1.6e15 us."""
    from event_representation_study_amd import _lib, n_imagenet_front as nf
    rng = np.random.default_rng(6)
    lengths = [700, 64, 2049, 1, 1500, 128, 900]
    wins = [synthetic(n, rng, 640, 480, t0=t0, pol=pol) for n, t0, pol in
            zip(lengths, [3_000_000_000, 0, 1_600_000_000_000_000, 5, 1_600_000_000_000_000, 77, 10 ** 12],
                [(0, 1), (-1, 1), (0, 1), (1,), (-1, 1), (0,), (0, 1)])]
    par = params(nf, lengths, rng)
    par["s0"][0], par["s1"][0] = 100, 650
    par["s0"][2], par["s1"][2] = 2049, 2049                                    # an empty slice at the window's end
    par["t_lo"][4], par["t_hi"][4] = float(wins[4][2][200]) / 1e6, float(wins[4][2][1200]) / 1e6
    par["t_lo"][6] = float(wins[6][2][450]) / 1e6
    par["s1"][6] = 800
    par["s0"][5], par["s1"][5] = 64, 128                                       # a slice that starts on a wave boundary
    front = nf.NImageNetFrontEnd(RESHAPE, "train")
    batch, base = make_batch(wins, 480, 640)
    aug = front.prepare(batch, t_base=base, params=par)
    check(aug, expected(host(front, wins, par)), "sliced batch")
    assert aug.status[2] == _lib.AUG_EMPTY
    # eval mode: no shift, no crop; the flips the parameters ask for are still applied
    ev_front = nf.NImageNetFrontEnd(types.SimpleNamespace(reshape=True, mode="val"), "eval")
    aug = ev_front.prepare(batch, t_base=base, params=par)
    check(aug, expected(host(ev_front, wins, par)), "sliced batch, eval")
    # a slice outside its window is refused for that window alone
    bad = par.copy()
    bad["s1"][1] = 65
    bad["s0"][3], bad["s1"][3] = 1, 0
    aug = front.prepare(batch, t_base=base, params=bad)
    rows = host(front, wins, par)
    rows[1] = rows[3] = np.zeros((0, 4))
    want = expected(rows)
    want["status"][[1, 3]] = _lib.AUG_EMPTY | _lib.AUG_BAD_SLICE
    check(aug, want, "bad slices")


def test_more_rows_than_one_round_of_every_slice():
    """Above 1024 * 1024 rows every slice is walked in more than one round of 1024 lanes."""
    from event_representation_study_amd import n_imagenet_front as nf
    rng = np.random.default_rng(7)
    lengths = [600_000, 3, 0, 500_000, 1025]
    wins = [synthetic(n, rng) for n in lengths]
    par = params(nf, lengths, rng, time_flip=[1, 0, 0, 0, 1])
    par["s0"][3], par["s1"][3] = 1234, 450_001
    front = nf.NImageNetFrontEnd(NOSHAPE, "train")
    batch, base = make_batch(wins, 224, 224)
    aug = front.prepare(batch, t_base=base, params=par)
    check(aug, expected(host(front, wins, par)), "two rounds")


def test_polarity_rule_reads_the_whole_window_not_the_slice():
    """Rows whose p is already what load_event's cast leaves (p_as_uint8=False).  Window 0 holds -1 outside its slice and
    {0, 1} inside: the minimum over the WINDOW is below -0.5, so the zeros stay zero.  Window 1 holds {0, 1} and its slice only
    ones next to a single zero: the zeros of the whole window's rule become -1."""
    from event_representation_study_amd import n_imagenet_front as nf
    rng = np.random.default_rng(8)
    wins = [synthetic(400, rng), synthetic(400, rng)]
    wins[0][3][:200], wins[0][3][200:] = -1, rng.integers(0, 2, 200)
    wins[1][3][:], wins[1][3][:200], wins[1][3][300] = 1, rng.integers(0, 2, 200), 0
    par = params(nf, [400, 400], rng, time_flip=[0, 0], x_flip=[0, 0], shifts=[(0, 0), (0, 0)])
    par["s0"][:] = 200
    front = nf.NImageNetFrontEnd(NOSHAPE, "train")
    batch, base = make_batch(wins, 224, 224)
    aug = front.prepare(batch, t_base=base, params=par, p_as_uint8=False)
    assert aug.counts.tolist() == [200, 200]
    pol = aug.batch.events[:, 3].cpu().numpy()
    assert np.array_equal(pol[:200], wins[0][3][200:]) and (pol[:200] == 0).any()
    want1 = np.where(wins[1][3][200:] > 0, 1, -1)
    assert np.array_equal(pol[200:], want1) and (want1 == -1).sum() == 1
    # read as load_event reads it, the stored -1 is 255: both windows follow the zero rule
    aug = front.prepare(batch, t_base=base, params=par)
    check(aug, expected(host(front, wins, par)), "p through uint8")
    assert set(aug.batch.events[:200, 3].cpu().numpy().tolist()) == {-1, 1}


# ------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def image_batch():
    from event_representation_study_amd import n_imagenet_front as nf
    sel = [c for c in CASES if c["name"] in ("flip_00", "flip_11", "flip_10")]
    pars = []
    for c in sel:
        np.random.seed(c["seed"])
        random.seed(c["seed"])
        front = nf.NImageNetFrontEnd(types.SimpleNamespace(**c["cfg"]), "train")
        pars.append(front.draw([len(columns(c)[0])]))
    wins = [columns(c) for c in sel]
    par = np.concatenate(pars)
    batch, base = make_batch(wins, 480, 640)
    return sel, front, front.prepare(batch, t_base=base, params=par), host(front, wins, par)


def test_accumulators_from_device_rows_equal_the_host_route(image_batch):
    from event_representation_study_amd import n_imagenet_acc as ni, n_imagenet_front as nf
    sel, front, aug, rows = image_batch
    for name in ni.SPECS:
        got = nf.accumulate_device(name, aug)
        want = ni.accumulate_batch(name, [torch.from_numpy(r) for r in rows])
        assert got.dtype == torch.float32 and tuple(got.shape) == (3, len(ni.SPECS[name][0]), 224, 224)
        same(got.contiguous(), want.contiguous().cpu().numpy(), name)
    with pytest.raises(KeyError):
        nf.accumulate_device("acc_sort", aug)


def test_accumulators_equal_the_reference_images(image_batch):
    from event_representation_study_amd import n_imagenet_front as nf
    sel, front, aug, rows = image_batch
    for name in ("acc_all", "acc_exp", "acc_intensity"):
        got = nf.accumulate_device(name, aug).cpu().numpy()
        for b, c in enumerate(sel):
            key = "%s.%s" % (c["name"], name)
            if key not in _G:
                continue
            if name == "acc_exp":
                np.testing.assert_allclose(got[b], _G[key], rtol=1e-5, atol=0, err_msg=key)
            else:
                np.testing.assert_array_equal(got[b], _G[key], err_msg=key)
    # eval mode
    c = next(c for c in CASES if c["name"] == "eval")
    batch, base = make_batch([columns(c)], 480, 640)
    aug = nf.NImageNetFrontEnd(types.SimpleNamespace(**c["cfg"]), "eval").prepare(batch, t_base=base)
    np.testing.assert_array_equal(nf.accumulate_device("acc_all", aug).cpu().numpy()[0], _G["eval.acc_all"])
    np.testing.assert_allclose(nf.accumulate_device("acc_exp", aug).cpu().numpy()[0], _G["eval.acc_exp"], rtol=1e-5, atol=0)
    np.testing.assert_array_equal(nf.accumulate_device("acc_intensity", aug).cpu().numpy()[0], _G["eval.acc_intensity"])


def test_prepare_recording_equals_prepare_on_host_cut_windows():
    from event_representation_study_amd import n_imagenet_front as nf
    from event_representation_study_amd.recording import DeviceRecording
    rng = np.random.default_rng(9)
    x, y, t, p = synthetic(20_000, rng, 640, 480, t0=1_600_000_000_000_000)
    rec = DeviceRecording(x, y, t, p, 480, 640)
    i0 = np.array([0, 5000, 5000, 19_000, 777], np.int64)
    i1 = np.array([3000, 8000, 5000, 20_000, 778], np.int64)
    front = nf.NImageNetFrontEnd(RESHAPE, "train")
    par = params(nf, (i1 - i0).tolist(), rng)
    aug = front.prepare_recording(rec, i0, i1, params=par)
    wins = [(x[a:e], y[a:e], t[a:e], p[a:e]) for a, e in zip(i0, i1)]
    batch, base = make_batch(wins, 480, 640)
    ref = front.prepare(batch, t_base=base, params=par)
    for a, b in ((aug.batch.events, ref.batch.events), (aug.t, ref.t), (aug.tnorm, ref.tnorm), (aug.xy, ref.xy)):
        same(a, b.cpu().numpy(), "recording")
    same(aug.status, ref.status, "recording status")
    check(aug, expected(host(front, wins, par)), "recording vs host")
    # drawn on the spot: the seeded generators give the batch B sequential reference calls would
    np.random.seed(4)
    random.seed(4)
    drawn = front.prepare_recording(rec, i0[:2], i1[:2])
    np.random.seed(4)
    random.seed(4)
    check(drawn, expected(host(front, wins[:2], front.draw([3000, 3000]))), "recording, drawn")
