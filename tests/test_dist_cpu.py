"""CPU-only: the oracle of the DiST kernels and their C-ABI surface.

``dist_image`` / ``dist_from_prim`` are a numpy float32 restatement of the three image-space stages of N-ImageNet's DiST
(n_imagenet/real_cnn_model/data/imagenet.py:897-990: count clip, 5x5 temporal discount, dense rank), every statement one IEEE
float32 operation.  It must reproduce every image the reference itself wrote -- tests/golden/nimg_dist.npz and the ``a``, ``b``,
``pos`` DiST images of tests/golden/nimagenet_acc.npz -- BIT FOR BIT; tests/test_gpu_dist.py then uses it as the expected value
for synthetic frames the reference never saw.  ``prim_from_events`` is the host form of the per-polarity count / latest / earliest
statistics (what the polstats builder leaves, :883-924).

The C-ABI checks need the library but no device: symbols, signatures, scratch sizes, argument errors.
"""
import ctypes
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, assert_bit_equal, load_golden

CLIP_RATE, ALPHA = 0.99, 3.0
F32 = np.float32


# ------------------------------------------------------------------------------------------------ the numpy restatement
def prim_from_events(ev, H, W):
    """(N, 4) float64 rows [x, y, t, p] -> (H, W, 6) float32 [pos count, pos latest, pos earliest, neg count, neg latest,
    neg earliest]; times normalised in float64 as (t - t[0]) / (t[-1] - t[0]) and rounded to float32 once (:908-924)."""
    ev = np.asarray(ev, np.float64).reshape(-1, 4)
    prim = np.zeros((H * W, 6), F32)
    tn = (ev[:, 2] - ev[0, 2]) / (ev[-1, 2] - ev[0, 2])
    pix = ev[:, 0].astype(np.int64) + ev[:, 1].astype(np.int64) * W
    for k, sel in ((0, ev[:, 3] > 0), (3, ev[:, 3] < 0)):
        prim[:, k] = np.bincount(pix[sel], minlength=H * W).astype(F32)
        hi, lo = np.full(H * W, -np.inf), np.full(H * W, np.inf)
        np.maximum.at(hi, pix[sel], tn[sel])
        np.minimum.at(lo, pix[sel], tn[sel])
        hit = prim[:, k] > 0
        prim[:, k + 1] = np.where(hit, hi, 0.0).astype(F32)          # scatter_max / scatter_min leave 0 where nothing landed
        prim[:, k + 2] = np.where(hit, lo, 0.0).astype(F32)
    return prim.reshape(H, W, 6)


def clip_threshold(count, clip_rate=CLIP_RATE):
    """th = #{ j : S_j < H*W*clip_rate } over the distinct count values in ascending order (:898-900).  `int64 tensor < Python
    float` is a float32 comparison in torch (its type promotion): the float64 product is rounded to float32, and so is S_j."""
    _, n = np.unique(count, return_counts=True)
    return int((np.cumsum(n).astype(F32) < F32(count.size * clip_rate)).sum())


def _pool5(a, pad, op):
    H, W = a.shape
    p = np.full((H + 4, W + 4), pad, F32)
    p[2:-2, 2:-2] = a
    out = p[0:H, 0:W].copy()
    for dy in range(5):
        for dx in range(5):
            if dy or dx:
                out = op(out, p[dy:dy + H, dx:dx + W])
    return out.astype(F32)


def dist_image(count, latest, earliest, clip_rate=CLIP_RATE, alpha=ALPHA, nb_exact=False):
    """One (H, W) polarity image.  nb_exact=True replaces nb = 25 * (s / 25) by s: NOT the reference (the golden generator uses
    it to find a case that tells the two apart)."""
    count, out, mn = (np.array(a, F32) for a in (count, latest, earliest))
    count = np.minimum(count, F32(clip_threshold(count, clip_rate)))
    mn[count == 0] = 1.0
    s = _pool5(count, 0.0, np.add)                                   # small integers: exact in any order
    nb = s if nb_exact else F32(25.0) * (s / F32(25.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        disc = (_pool5(out, -np.inf, np.maximum) + _pool5(-mn, -np.inf, np.maximum)) / nb
        hit = count > 0
        out[hit] = out[hit] - F32(alpha) * disc[hit]
    out[out < 0] = 0
    out[nb == 1.0] = 0
    uniq, inv = np.unique(out.reshape(-1), return_inverse=True)      # (-0.0 == +0.0 there as well)
    return (inv.reshape(out.shape).astype(F32) / F32(uniq.size)).astype(F32)


def dist_from_prim(prim, clip_rate=CLIP_RATE, alpha=ALPHA, nb_exact=False):
    """(B, H, W, 6) -> (B, 2, H, W) float32."""
    prim = np.asarray(prim, F32)
    return np.stack([np.stack([dist_image(p[..., k], p[..., k + 1], p[..., k + 2], clip_rate, alpha, nb_exact) for k in (0, 3)])
                     for p in prim])


# ------------------------------------------------------------------------------------------------ against the reference's images
def golden_cases():
    if not os.path.exists(os.path.join(GOLDEN, "nimg_dist.npz")):     # only while make_golden_dist.py writes it the first time
        return {}, []
    g = load_golden("nimg_dist")
    return g, json.loads(str(g["manifest"]))


_G, _NAMES = golden_cases()


@pytest.mark.parametrize("name", _NAMES)
def test_restatement_equals_the_reference_images(name):
    ev, H, W = _G[name + ".events"], int(_G[name + ".H"]), int(_G[name + ".W"])
    got = dist_from_prim(prim_from_events(ev, H, W)[None])[0]
    assert_bit_equal(got, _G[name + ".dist"], name)


@pytest.mark.parametrize("tag", ["a", "b", "pos"])
def test_restatement_equals_the_accumulator_goldens(tag):
    g = load_golden("nimagenet_acc")
    ev, H, W = g[tag + "_events"], int(g[tag + "_H"]), int(g[tag + "_W"])
    assert_bit_equal(dist_from_prim(prim_from_events(ev, H, W)[None])[0], g[tag + "_acc_adj_sort"], tag)


def test_goldens_hold_the_cases_they_are_there_for():
    assert len(_NAMES) >= 8
    frames = {(int(_G[n + ".H"]), int(_G[n + ".W"])) for n in _NAMES}
    assert {(3, 7), (5, 5), (24, 32), (224, 224)} <= frames
    assert sum(1 for n in _NAMES if (int(_G[n + ".H"]), int(_G[n + ".W"])) == (224, 224)) <= 2
    hot = prim_from_events(_G["hot_pixel.events"], int(_G["hot_pixel.H"]), int(_G["hot_pixel.W"]))
    assert sorted(np.unique(hot[..., 0]).tolist()) == [0, 1, 2, 7, 5000]
    assert not (_G["single_pol.events"][:, 3] < 0).any() and not _G["single_pol.dist"][1].any()
    assert np.unique(_G["ties.events"][:, 2]).size <= 24
    assert _G["flip_11.draw"][:2].tolist() == [1, 1]
    if "nb_rounding" in _NAMES:           # the image changes when nb is taken as the plain sum
        ev, H, W = _G["nb_rounding.events"], int(_G["nb_rounding.H"]), int(_G["nb_rounding.W"])
        prim = prim_from_events(ev, H, W)[None]
        assert not np.array_equal(dist_from_prim(prim, nb_exact=True)[0], _G["nb_rounding.dist"])


def test_clip_threshold_counts_distinct_values_below_the_quantile():
    c = np.zeros((8, 8), F32)
    assert clip_threshold(c) == 0                         # one value, S = 64 >= 63.36
    c[0, :2] = 5000                                       # S = 62, 64 -> th = 1
    assert clip_threshold(c) == 1
    c[1, 0], c[1, 1], c[1, 2] = 1, 2, 7                   # S = 59, 60, 61, 62, 64 -> th = 4
    assert clip_threshold(c) == 4


QUANTILE_FRAME = (463, 573)      # H*W*0.99 = 262646.01 in float64 and 262646.0 in float32


def quantile_edge_counts():
    """Exactly 262 646 pixels without an event, one event in each of the others: S_0 equals the float32 limit and is below the
    float64 one, so the reference's float32 comparison gives th = 0 where a float64 comparison gives 1."""
    H, W = QUANTILE_FRAME
    c = np.ones(H * W, F32)
    c[np.random.default_rng(21).permutation(H * W)[:262646]] = 0
    return c.reshape(H, W)


def test_clip_threshold_compares_as_torch_does():
    import torch
    H, W = QUANTILE_FRAME
    assert H * W * CLIP_RATE > 262646 and F32(H * W * CLIP_RATE) == 262646
    cases = [quantile_edge_counts(), np.random.default_rng(22).poisson(0.3, (24, 32)).astype(F32)]
    for count in cases:
        t = torch.from_numpy(count)
        sums = torch.cumsum(torch.unique(t, return_counts=True)[1], dim=0)                  # the reference's statements (:898-900)
        want = sums[sums < count.size * CLIP_RATE].shape[0]
        assert clip_threshold(count) == want
    assert clip_threshold(cases[0]) == 0


# ------------------------------------------------------------------------------------------------ the C ABI, without a device
@pytest.fixture(scope="module")
def lib():
    from event_representation_study_amd import build, _lib
    build.build()
    return _lib.load()


def test_dist_symbols_and_signatures(lib):
    from event_representation_study_amd import _lib
    i32, i64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    want = {"evrep_dist_scratch_bytes": (ctypes.c_size_t, [i32, i32, i32]),
            "evrep_dist": (ctypes.c_int, [vp, i32, i32, i32, ctypes.c_double, ctypes.c_float, vp, vp, vp]),
            "evrep_dense_rank_scratch_bytes": (ctypes.c_size_t, [i32, i64]),
            "evrep_dense_rank_f32": (ctypes.c_int, [vp, vp, i32, vp, vp, vp, vp])}
    for name, (res, args) in want.items():
        assert _lib.SYMBOLS[name] == (res, args), name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    assert lib.evrep_abi_version() == 3 == _lib.ABI_VERSION
    header = open(_lib._PKG + "/../include/evrep.h").read()
    for name in want:
        assert name + "(" in header


def test_scratch_sizes_are_monotone(lib):
    sizes = [lib.evrep_dist_scratch_bytes(B, 224, 224) for B in (1, 2, 3, 32, 33, 256)]
    assert all(a < b for a, b in zip(sizes, sizes[1:]))
    # per image: the discounted times and two (key, index) pair arrays
    assert sizes[0] >= 2 * 224 * 224 * (4 + 16)
    assert lib.evrep_dist_scratch_bytes(1, 1, 1) > 0
    ranks = [lib.evrep_dense_rank_scratch_bytes(S, S * 1000) for S in (1, 2, 65)]
    assert all(a < b for a, b in zip(ranks, ranks[1:])) and ranks[0] >= 16 * 1000
    for bad in ((0, 8, 8), (-1, 8, 8), (1, 0, 8), (1, 8, -3), (1, 5000, 8), (1 << 21, 8, 8)):
        assert lib.evrep_dist_scratch_bytes(*bad) == 0
    assert lib.evrep_dense_rank_scratch_bytes(0, 10) == 0 and lib.evrep_dense_rank_scratch_bytes(1, -1) == 0


def test_argument_errors_come_back_before_any_launch(lib):
    from event_representation_study_amd._lib import EVREP_EINVAL
    p = ctypes.c_void_p(4096)            # never dereferenced on the host
    assert lib.evrep_dist(None, 1, 8, 8, CLIP_RATE, ALPHA, p, p, None) == EVREP_EINVAL
    assert lib.evrep_dist(p, 1, 8, 8, CLIP_RATE, ALPHA, None, p, None) == EVREP_EINVAL
    assert lib.evrep_dist(p, 1, 8, 8, CLIP_RATE, ALPHA, p, None, None) == EVREP_EINVAL
    assert lib.evrep_dist(p, 1, 8, 8, CLIP_RATE, ALPHA, p, ctypes.c_void_p(4100), None) == EVREP_EINVAL      # scratch alignment
    for B, H, W in ((0, 8, 8), (-2, 8, 8), (1, 0, 8), (1, 8, 0), (1, 8, 4097), (1 << 21, 8, 8)):
        assert lib.evrep_dist(p, B, H, W, CLIP_RATE, ALPHA, p, p, None) == EVREP_EINVAL
    assert lib.evrep_dist(p, 1, 8, 8, float("nan"), ALPHA, p, p, None) == EVREP_EINVAL
    assert lib.evrep_dist(p, 1, 8, 8, -0.5, ALPHA, p, p, None) == EVREP_EINVAL
    assert lib.evrep_dense_rank_f32(None, p, 1, p, None, p, None) == EVREP_EINVAL
    assert lib.evrep_dense_rank_f32(p, None, 1, p, None, p, None) == EVREP_EINVAL
    assert lib.evrep_dense_rank_f32(p, p, 1, None, None, p, None) == EVREP_EINVAL
    assert lib.evrep_dense_rank_f32(p, p, 1, p, None, None, None) == EVREP_EINVAL
    assert lib.evrep_dense_rank_f32(p, p, 0, p, None, p, None) == EVREP_EINVAL
    assert lib.evrep_dense_rank_f32(p, p, -1, p, None, p, None) == EVREP_EINVAL
    assert lib.evrep_dense_rank_f32(p, ctypes.c_void_p(4100), 1, p, None, p, None) == EVREP_EINVAL           # offsets alignment


def test_python_entry_points_exist_and_refuse_unrankable_windows():
    """dist_batch checks its windows on the host, before anything is uploaded."""
    from event_representation_study_amd import n_imagenet_acc as ni, n_imagenet_front as nf
    assert callable(nf.dist_device)
    with pytest.raises(IndexError):
        ni.dist_batch([np.zeros((0, 4))], 8, 8)
    flat = np.array([[1, 1, 0.5, 1], [2, 2, 0.5, -1]], np.float64)
    with pytest.raises(ValueError, match="sample 1"):
        ni.dist_batch([np.array([[0, 0, 0.0, 1], [1, 1, 1.0, 1]]), flat], 8, 8)
