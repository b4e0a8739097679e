"""GPU: batched DiST on the device (evrep_dist / evrep_dense_rank_f32, csrc/evrep_dist.hip).

Everything is BIT-EQUAL: dist_batch to the images the reference's reshape_then_acc_adj_sort wrote (tests/golden/nimg_dist.npz),
dist_device to dist_batch on the host-augmented rows, evrep_dist on synthetic (B, H, W, 6) tensors to the numpy float32
restatement that tests/test_dist_cpu.py pins against those same images, evrep_dense_rank_f32 to np.unique.  The torch route
reshape_then_acc_adj_sort (unchanged) is the second comparator, within the atol=1e-6 its own test uses.

Shapes: frames no larger than the 5x5 stencil, one and several 16x64 stencil tiles with ragged edges, the workload's 224x224;
rank segments around the wave (64), the round (1 024) and the chunk (4 096) of the pair sort, and one beyond 2^16.
"""
import ctypes
import json
import random
import types

import numpy as np
import pytest
import torch

from conftest import assert_bit_equal, load_golden
from test_dist_cpu import ALPHA, CLIP_RATE, clip_threshold, dist_from_prim

pytestmark = pytest.mark.gpu
F32 = np.float32

_G = load_golden("nimg_dist")
NAMES = json.loads(str(_G["manifest"]))


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _sp():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def device_dist(prim, clip_rate=CLIP_RATE, alpha=ALPHA):
    """evrep_dist on a host (B, H, W, 6) array -> host (B, 2, H, W)."""
    from event_representation_study_amd import _lib
    lib = _lib.load()
    B, H, W, _ = prim.shape
    d_prim = torch.from_numpy(np.ascontiguousarray(prim, F32)).cuda()
    out = torch.full((B, 2, H, W), -1.0, dtype=torch.float32, device="cuda")
    scratch = torch.empty(int(lib.evrep_dist_scratch_bytes(B, H, W)), dtype=torch.uint8, device="cuda")
    _lib.check(lib.evrep_dist(_p(d_prim), B, H, W, clip_rate, alpha, _p(out), _p(scratch), _sp()), "evrep_dist")
    return out.cpu().numpy()


def device_rank(segments):
    """evrep_dense_rank_f32 on a list of float32 arrays -> (list of rank arrays, n_distinct)."""
    from event_representation_study_amd import _lib
    lib = _lib.load()
    S = len(segments)
    off = np.zeros(S + 1, np.int64)
    np.cumsum([len(s) for s in segments], out=off[1:])
    total = int(off[-1])
    keys = torch.from_numpy(np.concatenate(segments).astype(F32)).cuda()
    d_off = torch.from_numpy(off).cuda()
    out = torch.full((total,), -1.0, dtype=torch.float32, device="cuda")
    nd = torch.full((S,), -1, dtype=torch.int32, device="cuda")
    scratch = torch.empty(max(int(lib.evrep_dense_rank_scratch_bytes(S, total)), 256), dtype=torch.uint8, device="cuda")
    _lib.check(lib.evrep_dense_rank_f32(_p(keys), _p(d_off), S, _p(out), _p(nd), _p(scratch), _sp()), "evrep_dense_rank_f32")
    res = out.cpu().numpy()
    return [res[off[s]:off[s + 1]] for s in range(S)], nd.cpu().numpy()


def check_rank(segments, what):
    got, nd = device_rank(segments)
    for s, k in enumerate(segments):
        uniq, inv = np.unique(k, return_inverse=True)
        assert int(nd[s]) == uniq.size, (what, s)
        if k.size:
            assert_bit_equal(got[s], inv.reshape(-1).astype(F32) / F32(uniq.size), "%s segment %d (%d keys)" % (what, s, k.size))


# ------------------------------------------------------------------------------------------------ the reference's images
@pytest.fixture(scope="module")
def golden_batches():
    """dist_batch once per frame: {name: image}."""
    from event_representation_study_amd import n_imagenet_acc as ni
    frames, got = {}, {}
    for n in NAMES:
        frames.setdefault((int(_G[n + ".H"]), int(_G[n + ".W"])), []).append(n)
    for (H, W), names in frames.items():
        res = ni.dist_batch([torch.from_numpy(_G[n + ".events"].copy()) for n in names], H, W)
        assert res.dtype == torch.float32 and tuple(res.shape) == (len(names), 2, H, W) and res.is_cuda and res.is_contiguous()
        for n, img in zip(names, res.cpu().numpy()):
            got[n] = img
    return got


@pytest.mark.parametrize("name", NAMES)
def test_dist_batch_equals_the_reference_image(golden_batches, name):
    assert_bit_equal(golden_batches[name], _G[name + ".dist"], name)


@pytest.mark.parametrize("name", NAMES)
def test_dist_batch_agrees_with_the_torch_route(golden_batches, name):
    from event_representation_study_amd import n_imagenet_acc as ni
    H, W = int(_G[name + ".H"]), int(_G[name + ".W"])
    old = ni.reshape_then_acc_adj_sort(torch.from_numpy(_G[name + ".events"].copy()), height=H, width=W).numpy()
    np.testing.assert_allclose(golden_batches[name], old, rtol=0, atol=1e-6)


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


def test_dist_device_equals_dist_batch_on_the_host_mirror_rows():
    """The flip_00 / flip_11 / flip_10 windows of nimg_front.npz as one AugmentedBatch (the image_batch recipe of
    test_gpu_nimg_front.py)."""
    from event_representation_study_amd import n_imagenet_acc as ni, n_imagenet_front as nf
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
    got = nf.dist_device(aug)
    want = ni.dist_batch(rows)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 2, 224, 224) and got.is_cuda
    assert_bit_equal(got.cpu().numpy(), want.cpu().numpy(), "dist_device")
    assert len(np.unique(got.cpu().numpy())) > 100
    with pytest.raises(KeyError):
        nf.accumulate_device("acc_sort", aug)


def test_dist_device_refuses_empty_and_flat_time_windows():
    from event_representation_study_amd import _lib, n_imagenet_front as nf
    rng = np.random.default_rng(3)

    def win(n, flat=False):
        t = np.full(n, 3_000_000_123, np.int64) if flat else (np.sort(rng.integers(0, 40_000, n)) + 3_000_000_000).astype(np.int64)
        return rng.integers(0, 224, n).astype(np.uint16), rng.integers(0, 224, n).astype(np.uint16), t, rng.integers(0, 2, n).astype(np.int8)

    front = nf.NImageNetFrontEnd(types.SimpleNamespace(mode="val"), "eval")
    good = win(50)
    batch, base = make_batch([good, win(0), good], 224, 224)
    aug = front.prepare(batch, t_base=base)
    assert aug.status.tolist() == [0, _lib.AUG_EMPTY, 0]
    with pytest.raises(IndexError, match="sample 1"):
        nf.dist_device(aug)
    batch, base = make_batch([good, good, win(7, flat=True)], 224, 224)
    aug = front.prepare(batch, t_base=base)
    assert aug.status.tolist() == [0, 0, _lib.AUG_FLAT_TIME]
    with pytest.raises(ValueError, match="sample 2"):
        nf.dist_device(aug)
    batch, base = make_batch([good, good], 224, 224)
    assert tuple(nf.dist_device(front.prepare(batch, t_base=base)).shape) == (2, 2, 224, 224)


# ------------------------------------------------------------------------------------------------ the dense rank alone
def _keys(rng, n, kind):
    if kind == "equal":
        return np.full(n, 0.375, F32)
    if kind == "distinct":
        return (rng.permutation(n).astype(F32) - F32(n // 2)) * F32(0.25)            # negative ones too, exact in float32
    if kind == "mantissa":                                                          # neighbours in the lowest mantissa bit
        return (np.uint32(0x3F000000) + rng.integers(0, 3, n).astype(np.uint32)).view(F32)
    if kind == "zeros":
        return rng.choice(np.array([0.0, -0.0, 1.0, -1.0, 1e-45, -1e-45], F32), n)
    return rng.integers(0, max(2, n // 3), n).astype(F32) / F32(7.0)                 # ties


def test_dense_rank_segment_lengths_in_one_call():
    rng = np.random.default_rng(11)
    lengths = [1, 63, 0, 64, 65, 1023, 1025, 50176, 65537]
    kinds = ["equal", "ties", "ties", "distinct", "zeros", "mantissa", "ties", "ties", "distinct"]
    check_rank([_keys(rng, n, k) for n, k in zip(lengths, kinds)], "lengths")


@pytest.mark.parametrize("kind", ["equal", "distinct", "mantissa", "zeros"])
def test_dense_rank_key_patterns(kind):
    rng = np.random.default_rng(12)
    check_rank([_keys(rng, n, kind) for n in (5, 4097, 300)], kind)


@pytest.mark.parametrize("S", [1, 65])
def test_dense_rank_segment_counts(S):
    rng = np.random.default_rng(13 + S)
    check_rank([_keys(rng, int(n), "ties") for n in rng.integers(0 if S > 1 else 200, 400, S)], "S=%d" % S)


def test_dense_rank_signed_zero_is_one_value():
    got, nd = device_rank([np.array([0.0, -0.0, 0.5, -0.0], F32)])
    assert nd.tolist() == [2]
    assert_bit_equal(got[0], np.array([0.0, 0.0, 0.5, 0.0], F32), "signed zero")


# ------------------------------------------------------------------------------------------------ synthetic prim tensors
def synth_prim(rng, H, W, density=0.6, pols=(0, 3)):
    """One (H, W, 6) window: Poisson counts, earliest <= latest in [0, 1], both 0 where nothing landed."""
    prim = np.zeros((H, W, 6), F32)
    for k in pols:
        c = rng.poisson(density, (H, W)).astype(F32)
        lo = rng.random((H, W)).astype(F32)
        hi = np.where(c > 1, lo + (F32(1.0) - lo) * rng.random((H, W)).astype(F32), lo).astype(F32)
        prim[..., k], prim[..., k + 1], prim[..., k + 2] = c, np.where(c > 0, hi, 0), np.where(c > 0, lo, 0)
    return prim


FRAMES = [(1, 1), (3, 7), (5, 5), (6, 64), (17, 65), (224, 224)]


@pytest.mark.parametrize("H,W", FRAMES)
@pytest.mark.parametrize("B", [1, 3, 33])
def test_evrep_dist_equals_the_restatement(H, W, B):
    """Three distinct windows (dense; sparse; one polarity without events), repeated round-robin up to B: the expected images are
    computed once per distinct window."""
    rng = np.random.default_rng(1000 * H + W)
    distinct = [synth_prim(rng, H, W, 1.5), synth_prim(rng, H, W, 0.2), synth_prim(rng, H, W, 0.6, pols=(3,))][:min(B, 3)]
    want = dist_from_prim(np.stack(distinct))
    pick = [b % len(distinct) for b in range(B)]
    got = device_dist(np.stack([distinct[i] for i in pick]))
    assert_bit_equal(got, want[pick], "%dx%d B=%d" % (H, W, B))
    if B >= 3:
        assert not got[2, 0].any()                        # the polarity without events


def test_evrep_dist_lone_events_and_hot_pixel():
    """Every event pixel alone in its 5x5 neighbourhood (nb == 1 -> 0 everywhere); the hot-pixel frame of the goldens."""
    lone = np.zeros((20, 70, 6), F32)
    rng = np.random.default_rng(5)
    for k in (0, 3):
        lone[::3, ::3, k] = 1
        t = rng.random((20, 70)).astype(F32)
        lone[..., k + 1] = lone[..., k + 2] = np.where(lone[..., k] > 0, t, 0)
    got = device_dist(lone[None])
    assert not got.any()
    assert_bit_equal(got, dist_from_prim(lone[None]), "lone events")
    from test_dist_cpu import prim_from_events
    hot = prim_from_events(_G["hot_pixel.events"], 10, 12)[None]
    assert hot[..., 0].max() == 5000 and clip_threshold(hot[0, ..., 0]) < 5
    assert_bit_equal(device_dist(hot), dist_from_prim(hot), "hot pixel")
    assert_bit_equal(device_dist(hot)[0], _G["hot_pixel.dist"], "hot pixel golden")


def test_evrep_dist_clip_beyond_the_histogram_window():
    """8x8: the count at which 99 % of the pixels are reached lies far beyond the 4 096 values one sweep of the clip resolves, and
    the distinct counts are sparse, so the sweep window has to move several times."""
    rng = np.random.default_rng(6)
    prim = synth_prim(rng, 8, 8, 0.0)
    counts = np.concatenate([np.zeros(10), np.full(4, 3), 4096 + np.arange(20) * 7001, 300_000 + np.arange(30) * 4096]).astype(F32)
    for k, shift in ((0, 0), (3, 5)):
        c = np.roll(counts, shift).reshape(8, 8)
        lo = rng.random((8, 8)).astype(F32)
        prim[..., k], prim[..., k + 1], prim[..., k + 2] = c, np.where(c > 0, lo + (F32(1) - lo) * F32(0.5), 0), np.where(c > 0, lo, 0)
    assert clip_threshold(prim[..., 0]) == 51             # {0, 3} and 49 of the 50 large values lie below the quantile
    assert_bit_equal(device_dist(prim[None]), dist_from_prim(prim[None]), "clip beyond the window")
    # other clip rates and discounts move the threshold through the windows
    for rate, alpha in ((0.5, 3.0), (1.0, 1.0), (0.2, 0.5)):
        assert_bit_equal(device_dist(prim[None], rate, alpha), dist_from_prim(prim[None], rate, alpha), "rate %g" % rate)


def test_evrep_dist_clip_compares_in_float32():
    """463x573: H*W*0.99 rounds to an integer in float32, and exactly that many pixels are empty (th = 0, not 1)."""
    from test_dist_cpu import quantile_edge_counts
    rng = np.random.default_rng(9)
    c = quantile_edge_counts()
    c2 = c.copy()
    c2.reshape(-1)[np.flatnonzero(c.reshape(-1) == 0)[:100]] = 1       # the other polarity: a hundred pixels off the edge
    prim = np.zeros(c.shape + (6,), F32)
    t = rng.random(c.shape).astype(F32)
    for k, cnt in ((0, c), (3, c2)):
        prim[..., k], prim[..., k + 1], prim[..., k + 2] = cnt, np.where(cnt > 0, t, 0), np.where(cnt > 0, t, 0)
    assert clip_threshold(prim[..., 0]) == 0 and clip_threshold(prim[..., 3]) == 1
    assert_bit_equal(device_dist(prim[None]), dist_from_prim(prim[None]), "float32 quantile")


# ------------------------------------------------------------------------------------------------ graph capture
def test_evrep_dist_in_a_captured_graph():
    from event_representation_study_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(8)
    B, H, W = 3, 40, 70
    prim = np.stack([synth_prim(rng, H, W, d) for d in (1.0, 0.3, 2.0)])
    eager = device_dist(prim)
    d_prim = torch.from_numpy(prim).cuda()
    out = torch.zeros((B, 2, H, W), dtype=torch.float32, device="cuda")
    scratch = torch.empty(int(lib.evrep_dist_scratch_bytes(B, H, W)), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc = lib.evrep_dist(_p(d_prim), B, H, W, CLIP_RATE, ALPHA, _p(out), _p(scratch), _sp())
    assert rc == 0
    for k in range(2):
        out.fill_(-1.0)
        scratch.zero_()
        graph.replay()
        assert_bit_equal(out.cpu().numpy(), eager, "replay %d" % k)
