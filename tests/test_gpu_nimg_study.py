"""GPU: the study's representations (ERGO-12, EventStack, TORE) for N-ImageNet batches on the device.

evrep_nimg_study_rows (csrc/evrep_study.hip) against n_imagenet_front.study_rows_host, bit for bit, on B = 8 windows of 1, 2, 63,
64, 65, 257, 1000 and 4099 rows -- lengths on both sides of a wave (64) and of a workgroup's slice (256), the longest spread
over seventeen slices; study_device / study_batch against the reference's own reshape_then_optimized / _event_stack / _tore
images in tests/golden/nimg_study.npz (ERGO-12 and EventStack bit-equal, TORE within the rtol = atol = 1e-6 of
test_nimagenet_builder_wrappers) and against a loop of this package's per-sample wrappers, bit for bit.  The frame is 24 x 32.
"""
import ctypes
import json
import types

import numpy as np
import pytest
import torch

from conftest import assert_bit_equal, load_golden

pytestmark = pytest.mark.gpu

_G = load_golden("nimg_study")
CASES = json.loads(str(_G["manifest"]))
H, W = 24, 32
LENGTHS = [1, 2, 63, 64, 65, 257, 1000, 4099]
NAMES = ("optimized", "event_stack", "tore")
T0 = 1.6e9
PATTERN = 0x5A5A5A5A
TORE_FLOOR = np.float32(np.log(np.float32(500e6) + 1) - np.log(151))      # an empty FIFO slot (tore.py:69-79)


def same(got, want, what):
    """Bit-equal; NaNs compare as NaN."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = want.cpu().numpy() if isinstance(want, torch.Tensor) else np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype.kind == "f":
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), what + ": NaN pattern"
        got, want = np.where(nan, 0, got), np.where(nan, 0, want)
    assert_bit_equal(got, want, what)


def same_floor_pattern(got, want, what):
    """The empty FIFO slots -- the largest value a slot can hold -- lie where the reference has them."""
    assert abs(float(want.max()) - float(TORE_FLOOR)) <= 1e-6 and abs(float(got.max()) - float(TORE_FLOOR)) <= 1e-6, what
    assert np.array_equal(got == got.max(), want == want.max()), what + ": floor pattern"


def compare(name, got, want, what):
    """ERGO-12 and EventStack bit for bit; TORE within 1e-6 with the same pattern of floor values."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape)
    if name != "tore":
        return same(got, want, what)
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-6, err_msg=what)
    same_floor_pattern(got, want, what)


# ------------------------------------------------------------------------------------------ windows of float64 rows
def window(n, seed, times=None, flip=False):
    """(n, 4) float64 rows [x, y, t, p] as the front end leaves them: fractional coordinates on the frame, seconds, p = -1 / +1."""
    rng = np.random.default_rng(seed)
    ev = np.zeros((n, 4))
    ev[:, 0], ev[:, 1] = rng.random(n) * W, rng.random(n) * H
    ev[:, 2] = T0 + 0.98 + np.sort(rng.integers(0, 50_000, n)) / 1e6 if times is None else times     # straddles a whole second
    ev[:, 3] = rng.choice([-1.0, 1.0], n)
    if flip and n:
        ev = ev[::-1].copy()
        ev[:, 2], ev[:, 3] = ev[0, 2] - ev[:, 2], -ev[:, 3]
    return ev


def int_rows(ev):
    r = np.zeros((len(ev), 4), np.int32)
    r[:, 0], r[:, 1], r[:, 3] = ev[:, 0].astype(np.int64), ev[:, 1].astype(np.int64), np.sign(ev[:, 3])
    return r


def as_aug(wins):
    """The AugmentedBatch evrep_nimg_prepare would leave for windows whose augmented rows are `wins`."""
    from event_representation_study_amd import _lib, n_imagenet_front as nf
    from event_representation_study_amd.engine import EventBatch
    batch = EventBatch.from_numpy([int_rows(w) for w in wins], H, W)
    cat = np.concatenate(wins) if len(wins) else np.zeros((0, 4))
    t = torch.from_numpy(np.ascontiguousarray(cat[:, 2])).to(batch.device)
    xy = torch.from_numpy(np.ascontiguousarray(cat[:, :2])).to(batch.device)
    counts = np.array([len(w) for w in wins], np.int64)
    return nf.AugmentedBatch(batch, t, None, xy, np.where(counts == 0, _lib.AUG_EMPTY, 0).astype(np.uint32), counts)


def raw_call(wins, want, pad=5):
    """evrep_nimg_study_rows on buffers filled with a pattern, pad rows / windows longer than needed -> numpy outputs."""
    from event_representation_study_amd import _lib
    aug = as_aug(wins)
    b, lib = aug.batch, _lib.load()
    B, total = b.B, b.total
    outs = {k: torch.full((total + pad, 4), PATTERN, dtype=torch.int32, device=b.device) for k in ("mdes", "stack", "tore")}
    st = torch.full((B + pad,), float(PATTERN), dtype=torch.float64, device=b.device)
    status = torch.full((B + pad,), PATTERN, dtype=torch.int64, device=b.device).to(torch.int32)
    scratch = torch.empty(int(lib.evrep_nimg_study_rows_scratch_bytes(B, total)), dtype=torch.uint8, device=b.device)
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    rows_in, t_in, xy_in = b.events, aug.t, aug.xy
    if total == 0:                                   # an empty tensor has no address: one row nothing reads
        rows_in, t_in, xy_in = (torch.zeros(shape, dtype=d, device=b.device)
                                for shape, d in (((1, 4), torch.int32), (1, torch.float64), ((1, 2), torch.float64)))
    with torch.cuda.device(b.device):
        rc = lib.evrep_nimg_study_rows(p(rows_in), p(t_in), p(xy_in), p(b.offsets), B, H, W, want, p(outs["mdes"]), p(outs["stack"]),
                                       p(outs["tore"]), p(st), p(status), p(scratch), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in outs.items()}
    res["sample_times"], res["status"] = st.cpu().numpy(), status.cpu().numpy().view(np.uint32)
    return res


def check_raw(wins, want, what):
    from event_representation_study_amd import _lib, n_imagenet_front as nf
    res = raw_call(wins, want)
    B, total = len(wins), sum(len(w) for w in wins)
    host = [nf.study_rows_host(int_rows(w), np.ascontiguousarray(w[:, 2]), np.ascontiguousarray(w[:, :2])) for w in wins]
    for j, (key, bit) in enumerate((("mdes", _lib.STUDY_MDES), ("stack", _lib.STUDY_STACK), ("tore", _lib.STUDY_TORE))):
        if want & bit:
            assert_bit_equal(res[key][:total], np.concatenate([h[j] for h in host]), "%s: rows_%s" % (what, key))
            assert (res[key][total:] == PATTERN).all(), "%s: rows_%s beyond offsets[B]" % (what, key)
        else:
            assert (res[key] == PATTERN).all(), "%s: rows_%s is not wanted" % (what, key)
    assert_bit_equal(res["status"][:B], np.array([h[4] for h in host], np.uint32), what + ": status")
    assert (res["status"][B:] == PATTERN).all()
    if want & _lib.STUDY_TORE:
        same(res["sample_times"][:B], np.array([h[3] for h in host]), what + ": sample times")
        assert (res["sample_times"][B:] == float(PATTERN)).all()
    else:
        assert (res["sample_times"] == float(PATTERN)).all(), what + ": the sample times go with TORE"
    return res, host


def ordinary_windows():
    wins = [window(n, 100 + k, flip=k in (2, 5)) for k, n in enumerate(LENGTHS)]
    # the coordinate minima of the longest window lie only in its last row, the last row of its seventeenth slice
    wins[7][:-1, :2] += 1.5
    wins[7][:, :2] = np.minimum(wins[7][:, :2], [W - 0.01, H - 0.01])
    wins[7][-1, :2] = (0.35, 0.2)
    # ... and those of the 1000-row window in one row of its middle
    wins[6][:, :2] = np.maximum(wins[6][:, :2], 2.0)
    wins[6][768, :2] = (1.85, 0.05)
    return wins


def flagged_windows():
    """-> windows, what each is: FLAT, FUTURE, T_RANGE and an empty one in the middle, between ordinary ones."""
    wins = ordinary_windows()
    wins[2] = window(63, 202, times=T0 + 0.1 + np.sort(np.random.default_rng(1).random(63)) * 0.05)          # inside one second
    wins[3] = window(64, 203, times=T0 + np.linspace(2.9, 0.1, 64))                                        # descending
    wins[5][200, 2] = 1e19                                                                                # cannot be cast
    wins.insert(4, np.zeros((0, 4)))                                                                       # empty, in the middle
    t = wins[8][:, 2].copy()                           # the smallest whole second only in the last row of the last slice
    wins[8][:, 2] = t + 2.0
    wins[8][-1, 2] = t[0]
    return wins


# ------------------------------------------------------------------------------------------ the kernel's raw outputs
@pytest.mark.parametrize("want", [7, 1, 2, 4, 5], ids=["all", "mdes", "stack", "tore", "mdes+tore"])
def test_kernel_outputs_equal_the_host_restatement(want):
    res, host = check_raw(ordinary_windows(), want, "ordinary")
    assert [int(h[4]) for h in host] == [8, 0, 8, 0, 0, 8, 0, 0]            # one row, and the time-flipped windows, are FLAT
    if want & 4:
        off = np.cumsum([0] + LENGTHS)
        assert res["tore"][off[8] - 1, :2].tolist() == [0, 0] and res["tore"][off[6] + 768, :2].tolist() == [0, 0]


def test_kernel_flags_and_an_empty_window_in_the_middle():
    from event_representation_study_amd import _lib
    E, F, R, L, U = _lib.STUDY_EMPTY, _lib.STUDY_FUTURE, _lib.STUDY_T_RANGE, _lib.STUDY_FLAT, _lib.STUDY_UNORDERED
    res, host = check_raw(flagged_windows(), 7, "flagged")
    assert [int(h[4]) for h in host] == [L, 0, L, F | U, E, 0, R | U, 0, F | U]
    off = np.cumsum([0] + [len(w) for w in flagged_windows()])
    assert off[4] == off[5] and res["sample_times"][4] == 0.0
    assert res["mdes"][off[9] - 1, 2] == 0 and res["mdes"][off[8], 2] >= 2          # rebased to the minimum in the last row
    assert res["tore"][off[3] + 5, 2] == -5 and res["tore"][off[2] + 5, 2] == 5     # the order marker counts down where t does not ascend
    # a batch of one empty window, and the call twice: the same bytes
    check_raw([np.zeros((0, 4))], 7, "one empty window")
    again, _ = check_raw(flagged_windows(), 7, "flagged, again")
    for k in res:
        same(again[k], res[k], "two calls: " + k)


@pytest.mark.parametrize("B", [4, 5, 1])
def test_scratch_and_outputs_are_held_to_their_sizes(B):
    """evrep_nimg_study_rows_scratch_bytes(B, total) = up256(64 B), one 64-byte record per window: B = 4 -> 256 with no slack in
    front of the tail guard, B = 5 -> 512, B = 1.  Every pointer from the guarded arena of test_gpu_scratch_contracts: the scratch
    as long as the size function says, the row sets exactly offsets[B] rows, the per-window outputs B entries, the inputs read-only;
    under three fills and two arena seeds the results are bit-equal and no guard band changes."""
    from event_representation_study_amd import _lib, n_imagenet_front as nf
    from test_gpu_scratch_contracts import _sp, drive, up256
    lib = _lib.load()
    wins = [window(n, 300 + k, flip=k == 2) for k, n in enumerate([65, 0, 257, 1, 300][:B] if B > 1 else [130])]
    off = np.zeros(B + 1, np.int64)
    np.cumsum([len(w) for w in wins], out=off[1:])
    total = int(off[-1])
    cat = np.concatenate(wins)
    nbytes = int(lib.evrep_nimg_study_rows_scratch_bytes(B, total))
    assert nbytes == up256(64 * B) and (B != 4 or nbytes == 64 * B)
    assert nbytes == int(lib.evrep_nimg_study_rows_scratch_bytes(B, 0)) == int(lib.evrep_nimg_study_rows_scratch_bytes(B, 1 << 40))

    def call(g):
        rows, t = g.inp(int_rows(cat), "rows"), g.inp(np.ascontiguousarray(cat[:, 2]), "t")
        xy, d_off = g.inp(np.ascontiguousarray(cat[:, :2]), "xy"), g.inp(off, "offsets")
        outs = [g.out((total, 4), torch.int32, "rows_" + k) for k in ("mdes", "stack", "tore")]
        st, status = g.out((B,), torch.float64, "sample_times"), g.out((B,), torch.int32, "status")
        sc = g.scratch(nbytes)
        _lib.check(lib.evrep_nimg_study_rows(g.p(rows), g.p(t), g.p(xy), g.p(d_off), B, H, W, 7, g.p(outs[0]), g.p(outs[1]), g.p(outs[2]),
                                             g.p(st), g.p(status), g.p(sc), _sp()), "evrep_nimg_study_rows")
        return {"mdes": outs[0], "stack": outs[1], "tore": outs[2], "sample_times": st, "status": status}

    got = drive(call, "nimg_study_rows")
    host = [nf.study_rows_host(int_rows(w), np.ascontiguousarray(w[:, 2]), np.ascontiguousarray(w[:, :2])) for w in wins]
    for j, k in enumerate(("mdes", "stack", "tore")):
        assert_bit_equal(got[k], np.concatenate([h[j] for h in host]), k)
    assert_bit_equal(got["status"].view(np.uint32), np.array([h[4] for h in host], np.uint32), "status")
    assert_bit_equal(got["sample_times"], np.array([h[3] for h in host]), "sample times")


# ------------------------------------------------------------------------------------------ against the reference's images
def recorded_params(nf, cases):
    from event_representation_study_amd import _lib
    par = np.zeros(len(cases), nf.PARAMS_DTYPE)
    for b, c in enumerate(cases):
        tf, xf, xs, ys, s0, s1 = (int(v) for v in _G[c["name"] + ".draw"])
        par["s0"][b], par["s1"][b], par["t_lo"][b], par["t_hi"][b] = s0, s1, -np.inf, np.inf
        par["x_shift"][b], par["y_shift"][b] = xs, ys
        par["flags"][b] = (_lib.AUG_TIME_FLIP if tf else 0) | (_lib.AUG_X_FLIP if xf else 0)
    return par


def golden_aug(nf, cases, mode):
    from event_representation_study_amd.engine import EventBatch
    rows, bases = [], []
    for c in cases:
        x, y, t, p = (_G["stream%d.%s" % (c["stream"], k)] for k in "xytp")
        bases.append(int(t[0]))
        rows.append(np.stack([x.astype(np.int32), y.astype(np.int32), (t - t[0]).astype(np.int32), p.astype(np.int32)], axis=1))
    (sh, sw), (ih, iw) = cases[0]["sensor"], cases[0]["image"]
    assert (ih, iw) == (H, W)
    front = nf.NImageNetFrontEnd(types.SimpleNamespace(reshape=True, mode="train" if mode == "train" else "val"), mode,
                                 sensor=(sh, sw), image=(ih, iw))
    return front.prepare(EventBatch.from_numpy(rows, sh, sw), t_base=np.asarray(bases, np.int64), params=recorded_params(nf, cases))


@pytest.fixture(scope="module")
def golden_batches():
    from event_representation_study_amd import n_imagenet_front as nf
    train = [c for c in CASES if c["mode"] == "train"]
    ev = [c for c in CASES if c["mode"] == "eval"]
    assert len(train) >= 6 and len(ev) == 1
    return [(train, golden_aug(nf, train, "train")), (ev, golden_aug(nf, ev, "eval"))]


@pytest.mark.parametrize("name", NAMES)
def test_study_device_equals_the_reference(golden_batches, name):
    from event_representation_study_amd import n_imagenet_acc as ni, n_imagenet_front as nf
    for cases, aug in golden_batches:
        for b, c in enumerate(cases):          # the front end left the reference's tensors
            o = int(aug.batch.offsets_host[b])
            same(aug.t[o:o + int(aug.counts[b])], _G[c["name"] + ".out"][:, 2], c["name"] + ": t")
        want = np.stack([_G["%s.%s" % (c["name"], name)] for c in cases])
        got = nf.study_device(name, aug)
        assert got.is_contiguous() and tuple(got.shape) == (len(cases), 12, H, W)
        compare(name, got, want, "study_device(%s)" % name)
        host = ni.study_batch(name, [torch.from_numpy(_G[c["name"] + ".out"].copy()) for c in cases], height=H, width=W)
        compare(name, host, want, "study_batch(%s)" % name)
        same(host, got, "study_batch against study_device (%s)" % name)
    if name == "optimized":
        assert np.isnan(_G["inside_00.optimized"]).any()      # a window inside one whole second: the reference's 0 / 0


@pytest.mark.parametrize("name", NAMES)
def test_study_batch_on_the_integral_streams_of_the_wrapper_golden(name):
    """The w1 / w2 streams test_nimagenet_builder_wrappers reads: integral coordinates and integral times."""
    from event_representation_study_amd import n_imagenet_acc as ni
    g = load_golden("nimagenet_acc")
    for tag in ("w1", "w2"):
        ev, h, w = g[tag + "_events"], int(g[tag + "_H"]), int(g[tag + "_W"])
        got = ni.study_batch(name, [torch.from_numpy(ev.copy()), torch.from_numpy(ev[:500].copy())], height=h, width=w)
        assert tuple(got.shape) == (2, 12, h, w)
        want = g["%s_%s" % (tag, name)]
        got = got.cpu().numpy()
        assert got.dtype == np.float32
        if name != "tore":
            same(got[0], want, tag + " " + name)
        else:
            np.testing.assert_allclose(got[0], want, rtol=1e-6, atol=1e-6)
            same_floor_pattern(got[0], want, tag)


# ------------------------------------------------------------------------------------------ batched equals per-sample
def sensor_windows(rng, lengths):
    out = []
    for n in lengths:
        x, y = rng.integers(0, W, n).astype(np.uint16), rng.integers(0, H, n).astype(np.uint16)
        t = (np.sort(rng.integers(0, 50_000, n)) + 1_600_000_000_980_000).astype(np.int64)
        out.append((x, y, t, rng.integers(0, 2, n).astype(np.int8)))
    return out


def front_batch(nf, wins, mode, flips):
    from event_representation_study_amd.engine import EventBatch
    B = len(wins)
    lengths = [len(w[0]) for w in wins]
    au = dict(time_flip=np.array([f & 1 for f in flips], bool), x_flip=np.array([f & 2 for f in flips], bool),
              x_shift=np.array([(b % 5) - 2 for b in range(B)], np.int32), y_shift=np.array([(b % 3) - 1 for b in range(B)], np.int32))
    par = nf.pack_params(nf.draw_slice(lengths, types.SimpleNamespace()), au)
    front = nf.NImageNetFrontEnd(types.SimpleNamespace(mode="train"), mode, sensor=(H, W), image=(H, W))
    rows = [np.stack([x.astype(np.int32), y.astype(np.int32), (t - t[0]).astype(np.int32), p.astype(np.int32)], axis=1) for x, y, t, p in wins]
    aug = front.prepare(EventBatch.from_numpy(rows, H, W), t_base=np.array([int(w[2][0]) for w in wins], np.int64), params=par)
    host = [nf.host_rows(*w, par[b], train=mode == "train", resolution=(H, W)) for b, w in enumerate(wins)]
    return aug, host


@pytest.fixture(scope="module")
def per_sample_batches():
    """Train mode with all four flip combinations over the eight lengths (centre pixels for the shortest, so the crop keeps
    them), and eval mode; the per-sample images are computed once."""
    from event_representation_study_amd import n_imagenet_acc as ni, n_imagenet_front as nf
    rng = np.random.default_rng(31)
    wins = sensor_windows(rng, LENGTHS)
    for w in wins[:2]:
        w[0][:], w[1][:] = W // 2, H // 2
    out = []
    for mode, flips in (("train", [0, 1, 2, 3, 0, 1, 2, 3]), ("eval", [3, 0, 0, 1, 2, 0, 0, 0])):
        aug, host = front_batch(nf, wins, mode, flips)
        assert all(len(h) for h in host) and aug.counts.tolist() == [len(h) for h in host]
        per = {name: torch.stack([getattr(ni, "reshape_then_" + name)(h.clone(), height=H, width=W) for h in host]) for name in NAMES}
        out.append((mode, aug, host, per))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_batched_equals_a_loop_of_the_per_sample_wrappers(per_sample_batches, name):
    from event_representation_study_amd import n_imagenet_front as nf
    for mode, aug, host, per in per_sample_batches:
        got = nf.study_device(name, aug)
        same(got, per[name].numpy(), "%s, %s mode" % (name, mode))


def test_output_contract_and_the_callers_columns(per_sample_batches):
    from event_representation_study_amd import n_imagenet_front as nf
    mode, aug, host, per = per_sample_batches[0]
    before = [v.clone() for v in (aug.batch.events, aug.batch.offsets, aug.t, aug.tnorm, aug.xy)]
    for name in NAMES:
        img = nf.study_device(name, aug)
        assert img.dtype == torch.float32 and tuple(img.shape) == (8, 12, H, W) and img.is_contiguous() and img.device == aug.t.device
        img2, status = nf.study_device(name, aug, check=False)
        assert status.dtype == torch.uint32 and tuple(status.shape) == (8,) and status.device == aug.t.device
        same(img2, img, name + ": two calls")
    for a, b in zip(before, (aug.batch.events, aug.batch.offsets, aug.t, aug.tnorm, aug.xy)):
        same(b, a, "the caller's columns")
    lean = nf.AugmentedBatch(aug.batch, aug.t, aug.tnorm, None, aug.status, aug.counts)         # prepare(want_xy=False)
    same(nf.study_device("optimized", lean), per["optimized"].numpy(), "without xy")
    with pytest.raises(ValueError):
        nf.study_device("tore", lean)


# ------------------------------------------------------------------------------------------ placement
def test_a_window_gives_the_same_bits_wherever_it_stands():
    from event_representation_study_amd import n_imagenet_front as nf
    probe, others = window(257, 41), [window(n, 50 + n) for n in (65, 1000, 64)]
    alone = {name: nf.study_device(name, as_aug([probe]), check=False)[0][0] for name in NAMES}
    for pos, wins in ((0, [probe] + others), (3, others + [probe]), (1, others[:1] + [probe] + others[1:])):
        aug = as_aug(wins)
        for name in NAMES:
            got, status = nf.study_device(name, aug, check=False)
            same(got[pos], alone[name], "%s at %d" % (name, pos))
            assert not status.cpu().numpy().any()
            same(nf.study_device(name, aug, check=False)[0], got, name + ": two calls")


# ------------------------------------------------------------------------------------------ refusals
def test_flagged_windows_are_refused_by_name_and_reported_without_check():
    from event_representation_study_amd import _lib, n_imagenet_acc as ni, n_imagenet_front as nf
    E, F, R, L, U = _lib.STUDY_EMPTY, _lib.STUDY_FUTURE, _lib.STUDY_T_RANGE, _lib.STUDY_FLAT, _lib.STUDY_UNORDERED
    good = [window(65, 61), window(257, 62), window(63, 63)]
    empty, future = np.zeros((0, 4)), window(64, 64, times=T0 + np.linspace(2.9, 0.1, 64))
    nan = window(65, 65)
    nan[7, 2] = np.nan
    clean = {name: nf.study_device(name, as_aug(good)) for name in NAMES}
    for name in NAMES:
        empty_error = IndexError if name == "event_stack" else ValueError
        with pytest.raises(empty_error, match="sample 1"):
            nf.study_device(name, as_aug([good[0], empty, good[1], empty]))
        with pytest.raises(ValueError, match="sample 2"):
            nf.study_device(name, as_aug([good[0], good[1], nan]))
        with pytest.raises(empty_error, match="sample 0"):
            ni.study_batch(name, [torch.from_numpy(empty), torch.from_numpy(good[0])], height=H, width=W)
        # without check: the words come back, the other windows are built as they are without the flagged ones
        wins = [good[0], empty, future, good[1], nan, good[2]]
        img, status = nf.study_device(name, as_aug(wins), check=False)
        assert status.cpu().numpy().tolist() == [0, E, F | U, 0, R | U, 0]
        same(img[[0, 3, 5]], clean[name], name + ": the windows beside flagged ones")
    with pytest.raises(ValueError, match="sample 2.*reshape_then_event_stack"):
        nf.study_device("event_stack", as_aug([good[0], good[1], future]))
    for name in ("optimized", "tore"):           # ERGO-12 and TORE take rows in any order, as their wrappers do
        img = nf.study_device(name, as_aug([good[0], future]))
        want = getattr(ni, "reshape_then_" + name)(torch.from_numpy(future.copy()), height=H, width=W)
        same(img[1], want.numpy(), name + " of a descending window")
    with pytest.raises(ValueError, match="sample 1"):
        ni.study_batch("optimized", [torch.from_numpy(good[0]), torch.from_numpy(np.array([[1.0, 1.0, 0.5, 2.0]]))], height=H, width=W)
    with pytest.raises(KeyError):
        nf.study_device("acc_all", as_aug(good))
    with pytest.raises(IndexError):
        nf.study_device("time_surface", as_aug(good))
