"""-m gpu: every *_bytes function of include/evrep.h held to what its kernels read and write.

One small driver per entry, through _lib.load().  Every device pointer of a call comes from tests/guarded.py: the scratch region
exactly as long as the size function says, the outputs exactly as long as the header documents, the inputs registered read-only
and ending where their tail guard begins.  Each driver runs its call under the three interior fills (zeros, 0xFF, random) and
under a second arena seed, and asserts
  * the result equals the reference the entry's own test uses (imported from it, with its tolerance),
  * the results of the four runs are bit-equal -- scratch and outputs need no initialisation, and the bytes behind an input
    (which differ between the seeds) never reach a result,
  * no guard band and no input changed.
The arguments sit at the edges of each formula: a payload that is an exact multiple of 256 bytes (no slack in front of the tail
guard), one element over, and the smallest legal; the arithmetic stands in a comment at each driver.

The size functions of include/evrep.h and their drivers (a new one without a line here has no driver):
  evrep_workspace_bytes                       test_gpu_workspace_contract.py (the whole module); test_workspace_bytes_is_the_plan_field
  evrep_filter_compact_scratch_bytes          test_filter_compact
  evrep_nimg_prepare_scratch_bytes            test_nimg_prepare
  evrep_dist_scratch_bytes                    test_dist
  evrep_dense_rank_scratch_bytes              test_dense_rank
  evrep_time_index_scratch_bytes              test_time_index
  evrep_sort_image_scratch_bytes              test_sort_image
  evrep_voxel_normalize_scratch_bytes         test_voxel_normalize
  evrep_est_backward_scratch_bytes            test_est_voxel_backward
  evrep_est_prepare_scratch_bytes             test_est_prepare, test_an_understated_scratch_is_seen
  evrep_decode_scratch_bytes                  test_decode_drop_oob
  evrep_otmi_scratch_bytes                    test_otmi_clouds
  evrep_gwd_scratch_bytes                     test_gwd_padded_l1
  evrep_gwd_batch_scratch_bytes               test_gwd_padded_l1_batch
  evrep_gw_scratch_bytes                      test_entropic_gw
  evrep_detector_input_frames_scratch_bytes   test_detector_input_frames_table
Outputs of calls without scratch: test_windows_gather_and_time_to_index, test_resize_taps.
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import assert_bit_equal
from guarded import FILLS, Arena, GuardError

from event_representation_study_amd import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = np.float32
RUNS = tuple((1, f) for f in FILLS) + ((2, "random"),)      # (arena seed, interior fill)


def up256(n):
    return (int(n) + 255) // 256 * 256


def _sp():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class G:
    """One run's arena: inputs, outputs and scratch of a call, and their addresses (a zero-size view has no data_ptr())."""

    def __init__(self, seed, fill):
        self.arena, self.fill, self._ptr = Arena(DEV, seed), fill, {}

    def _reg(self, t):
        self._ptr[id(t)] = self.arena.ptr()
        return t

    def inp(self, array, name, align=256):
        t = array if isinstance(array, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(array))
        return self._reg(self.arena.carve_like(t, name=name, align=align))

    def out(self, shape, dtype, name):
        return self._reg(self.arena.carve_shape(shape, dtype, fill=self.fill, name=name))

    def scratch(self, nbytes, name="scratch"):
        assert nbytes > 0, name
        return self._reg(self.arena.carve(nbytes, fill=self.fill, name=name))

    def p(self, t):
        return ctypes.c_void_p(self._ptr[id(t)])

    def finish(self):
        torch.cuda.synchronize()
        self.arena.check()
        self.arena.check_inputs()


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8)), what


def drive(call, what):
    """call(g) -> {name: host array}; run under RUNS, guards and inputs checked, results bit-equal.  Returns the first run's."""
    first = None
    for seed, fill in RUNS:
        g = G(seed, fill)
        res = call(g)
        g.finish()
        res = {k: v.cpu().numpy() if isinstance(v, torch.Tensor) else v for k, v in res.items()}
        if first is None:
            first = res
        for k in res:
            _same(res[k], first[k], "%s: %s under seed %d, fill %s vs seed %d, fill %s" % (what, k, seed, fill, RUNS[0][0], RUNS[0][1]))
    return first


def test_workspace_bytes_is_the_plan_field():
    """evrep_workspace_bytes(plan) is the end of the last region; a refused plan has none.  (test_gpu_workspace_contract.py holds
    every kernel to it.)"""
    lib = _lib.load()
    plan = _lib.Plan()
    assert lib.evrep_plan_init_ex(ctypes.byref(plan), 1, 63, 300, 2207, 2207, 0) == _lib.EVREP_OK
    assert lib.evrep_workspace_bytes(ctypes.byref(plan)) == plan.workspace_bytes > plan.off_scratch
    assert lib.evrep_workspace_bytes(None) == 0


# ---------------------------------------------------------------------------------------------------------------- EST prepare
def _est_stream(B):
    """A grouped stream of B items (some batch indices never occur: empty items), the generator of test_est_prepare_cpu."""
    from test_est_prepare_cpu import item
    rng = np.random.default_rng(B)
    lengths = [(1, 5, 0, 64, 65, 3, 0, 17)[b % 8] for b in range(B)]
    lengths[0] = max(lengths[0], 1)
    return np.concatenate([item(n, b, rng) for b, n in enumerate(lengths) if n])


def _est_prepare(g, ev, B, scratch_bytes):
    from test_est_prepare_cpu import H, W
    lib, n = _lib.load(), len(ev)
    d = g.inp(ev, "events5")
    rows, offs = g.out((n, 4), torch.int32, "rows"), g.out((B + 1,), torch.int64, "offsets")
    tn, status = g.out((n,), torch.float32, "tnorm"), g.out((1,), torch.int32, "status")
    sc = g.scratch(scratch_bytes)
    rc = lib.evrep_est_prepare(g.p(d), n, B, H, W, g.p(rows), g.p(offs), g.p(tn), g.p(status), g.p(sc), _sp())
    assert rc == _lib.EVREP_OK
    return {"rows": rows, "offsets": offs, "tnorm": tn, "status": status}


@pytest.mark.parametrize("B", [63, 127, 1])
def test_est_prepare(B):
    """evrep_est_prepare_scratch_bytes(n, B) = up256((B + 1) * 4): B = 63 -> 256 and B = 127 -> 512 with no slack (the call clears
    exactly these bytes itself); B = 1 -> 8 bytes in 256."""
    from test_est_prepare_cpu import nan_equal_bits, restated
    lib = _lib.load()
    ev = _est_stream(B)
    nbytes = int(lib.evrep_est_prepare_scratch_bytes(len(ev), B))
    assert nbytes == up256((B + 1) * 4) and (B == 1 or nbytes == (B + 1) * 4)
    got = drive(lambda g: _est_prepare(g, ev, B, nbytes), "est_prepare B=%d" % B)
    with np.errstate(all="ignore"):
        rows, offs, tn = restated(ev, B)
    assert_bit_equal(got["rows"], rows, "rows")
    assert_bit_equal(got["offsets"], offs, "offsets")
    nan_equal_bits(got["tnorm"], tn, "tnorm")
    assert int(got["status"][0]) == 0


def test_an_understated_scratch_is_seen():
    """The control: B = 127 with a scratch region of 256 bytes where 512 are stated.  The call clears (B + 1) * 4 = 512 bytes
    itself and keeps its keys there, so the 256 bytes behind the region -- the start of its tail guard, inside the same torch
    allocation -- change, and arena.check() must report the tail guard touched at offsets 0 to 255.  The changed bytes are known
    exactly: where the upper half of a rightly sized scratch after the same call differs from the guard's pristine bytes (a key
    byte can coincide with a pseudo-random one; with this seed neither the first nor the last does).  The only place in the suite
    where a buffer is understated."""
    B = 127
    ev = _est_stream(B)
    assert int(_lib.load().evrep_est_prepare_scratch_bytes(len(ev), B)) == 512
    whole = G(2, "ones")
    _est_prepare(whole, ev, B, 512)
    whole.finish()
    keys = whole.arena.regions[-1].buf[whole.arena.regions[-1].start + 256:][:256].cpu().numpy()      # bytes 256 .. 511 of the scratch
    g = G(1, "random")
    _est_prepare(g, ev, B, 256)
    torch.cuda.synchronize()
    r = g.arena.regions[-1]
    assert r.name == "scratch" and r.nbytes == 256
    changed = np.flatnonzero(keys != r.pristine[r.start + 256:][:256].cpu().numpy())
    with pytest.raises(GuardError) as e:
        g.arena.check()
    e = e.value
    assert (e.region, e.side) == ("scratch", "tail"), str(e)
    assert (e.first, e.last, e.count) == (int(changed[0]), int(changed[-1]), changed.size), (str(e), changed)
    assert (e.first, e.last) == (0, 255) and e.count >= 248, str(e)
    g.arena.check_inputs()


# ---------------------------------------------------------------------------------------------------------------- DiST, dense rank
@pytest.mark.parametrize("B,H,W", [(1, 4, 8), (1, 5, 7), (3, 5, 7)])
def test_dist(B, H, W):
    """evrep_dist_scratch_bytes = up256(2B * 4) [thresholds] + up256(2B * HW * 4) [keys] + 4 * up256(2B * HW * 4) [rank arrays].
    B = 1, 4 x 8: 2 * 32 * 4 = 256: the key array and the four rank arrays end on their region's last byte; 5 x 7 and B = 3: odd."""
    from test_dist_cpu import ALPHA, CLIP_RATE, dist_from_prim
    from test_gpu_dist import synth_prim
    lib = _lib.load()
    rng = np.random.default_rng(100 * H + B)
    prim = np.stack([synth_prim(rng, H, W, d) for d in (1.5, 0.2, 0.6)[:B]])
    nbytes = int(lib.evrep_dist_scratch_bytes(B, H, W))
    assert nbytes == up256(2 * B * 4) + 5 * up256(2 * B * H * W * 4)
    if (B, H, W) == (1, 4, 8):
        assert nbytes == 256 + 5 * 2 * B * H * W * 4

    def call(g):
        d, out, sc = g.inp(prim, "prim"), g.out((B, 2, H, W), torch.float32, "out"), g.scratch(nbytes)
        _lib.check(lib.evrep_dist(g.p(d), B, H, W, CLIP_RATE, ALPHA, g.p(out), g.p(sc), _sp()), "evrep_dist")
        return {"out": out}

    assert_bit_equal(drive(call, "dist")["out"], dist_from_prim(prim), "dist %dx%d B=%d" % (H, W, B))


@pytest.mark.parametrize("lengths", [(64,), (30, 0, 35), (1,)], ids=["total64", "S3_empty_total65", "one_key"])
def test_dense_rank(lengths):
    """evrep_dense_rank_scratch_bytes(S, total) = 4 * up256(total * 4): total = 64 -> four arrays of exactly 256 bytes; 65: one
    element over; S = 3 with an empty segment."""
    from test_gpu_dist import _keys
    lib = _lib.load()
    rng = np.random.default_rng(sum(lengths))
    segs = [_keys(rng, n, "ties") for n in lengths]
    S, total = len(segs), sum(lengths)
    off = np.zeros(S + 1, np.int64)
    np.cumsum(lengths, out=off[1:])
    nbytes = int(lib.evrep_dense_rank_scratch_bytes(S, total))
    assert nbytes == 4 * up256(total * 4) and (total != 64 or nbytes == 4 * total * 4)

    def call(g):
        keys, d_off = g.inp(np.concatenate(segs).astype(F32), "keys"), g.inp(off, "seg_offsets")
        out, nd, sc = g.out((total,), torch.float32, "out"), g.out((S,), torch.int32, "n_distinct"), g.scratch(nbytes)
        _lib.check(lib.evrep_dense_rank_f32(g.p(keys), g.p(d_off), S, g.p(out), g.p(nd), g.p(sc), _sp()), "evrep_dense_rank_f32")
        return {"out": out, "nd": nd}

    got = drive(call, "dense_rank")
    for s, k in enumerate(segs):                                   # (test_gpu_dist.check_rank)
        uniq, inv = np.unique(k, return_inverse=True)
        assert int(got["nd"][s]) == uniq.size, s
        if k.size:
            assert_bit_equal(got["out"][off[s]:off[s + 1]], inv.reshape(-1).astype(F32) / F32(uniq.size), "segment %d" % s)


# ---------------------------------------------------------------------------------------------------------------- sorted timestamp image
@pytest.mark.parametrize("B", [64, 1, 65])
def test_time_index(B):
    """evrep_time_index_scratch_bytes(B, total) = up256(257 * 4) + 2 * up256(B * 4): B = 64 -> 1280 + 256 + 256, both per-window
    arrays end on their region's last byte; B = 65: one element over; B = 1."""
    from test_gpu_sort import stamps
    from test_sort_cpu import time_status, time_values
    lib = _lib.load()
    rng = np.random.default_rng(B)
    wins = [stamps(rng, (40, 0, 1, 65, 7)[b % 5] if B > 1 else 300) for b in range(B)]
    off = np.zeros(B + 1, np.int64)
    np.cumsum([len(w) for w in wins], out=off[1:])
    total = int(off[-1])
    nbytes = int(lib.evrep_time_index_scratch_bytes(B, total))
    assert nbytes == 1280 + 2 * up256(B * 4) and (B != 64 or nbytes == 1280 + 2 * B * 4)
    for mode in (_lib.TIME_INDEX_RANK, _lib.TIME_INDEX_RAW):
        def call(g):
            t, d_off = g.inp(np.concatenate(wins).astype(np.float64), "t"), g.inp(off, "offsets")
            out, status, sc = g.out((total,), torch.float64, "out"), g.out((B,), torch.int32, "status"), g.scratch(nbytes)
            _lib.check(lib.evrep_time_index(g.p(t), g.p(d_off), B, mode, g.p(out), g.p(status), g.p(sc), _sp()), "evrep_time_index")
            return {"out": out, "status": status}

        got = drive(call, "time_index mode %d" % mode)
        for b, w in enumerate(wins):                               # (test_gpu_sort.check_time_index)
            assert int(got["status"][b]) & 0xFFFFFFFF == time_status(w), (mode, b)
            assert_bit_equal(got["out"][off[b]:off[b + 1]], time_values(w, rank=bool(mode)), "mode %d window %d" % (mode, b))


@pytest.mark.parametrize("B,K,H,W", [(1, 1, 8, 8), (2, 2, 4, 4), (1, 2, 5, 7)])
def test_sort_image(B, K, H, W):
    """evrep_sort_image_scratch_bytes(B, H, W, K) = 4 * up256(B * K * H * W * 4): B * K * H * W = 64 -> four arrays of exactly 256
    bytes (K = 1 and K = 2); 5 x 7, K = 2: 70 elements."""
    from test_gpu_sort import synth_class
    from test_sort_cpu import sort_from_prim
    lib = _lib.load()
    rng = np.random.default_rng(B + 10 * K + H)
    prim = np.stack([np.concatenate([synth_class(rng, H, W, H * W // 2, 5) for _ in range(K)], axis=2) for _ in range(B)])
    nbytes = int(lib.evrep_sort_image_scratch_bytes(B, H, W, K))
    assert nbytes == 4 * up256(B * K * H * W * 4) and (B * K * H * W != 64 or nbytes == 1024)
    qs = [2, 8]
    C = K * (1 + len(qs))

    def call(g):
        d, out, sc = g.inp(prim.astype(F32), "prim"), g.out((B, C, H, W), torch.float32, "out"), g.scratch(nbytes)
        status = g.out((B,), torch.int32, "status")
        status.zero_()                                             # (OR-ed into: the caller's to zero)
        _lib.check(lib.evrep_sort_image(g.p(d), B, H, W, K, _lib.SORT_STRICT | _lib.SORT_USE_IMAGE, _lib.int32_array(qs), len(qs),
                                        g.p(out), g.p(status), g.p(sc), _sp()), "evrep_sort_image")
        return {"out": out, "status": status}

    got = drive(call, "sort_image")
    for b in range(B):
        want, st = sort_from_prim(prim[b], True, True, qs)
        assert int(got["status"][b]) == st, b
        assert_bit_equal(got["out"][b], want, "window %d" % b)


# ---------------------------------------------------------------------------------------------------------------- voxel normalise
@pytest.mark.parametrize("B,H,W,bins", [(16, 5, 7, 3), (1, 5, 7, 1), (3, 4, 4, 16)])
def test_voxel_normalize(B, H, W, bins):
    """evrep_voxel_normalize_scratch_bytes = 3 * up256(B * 128 * 8) [partials, always whole] + up256(B * 2 * 8) [mean, std]:
    B = 16 -> 256 with no slack; B = 1; bins = 1."""
    from evl_voxel_ref import assert_matches_restatement
    from test_gpu_evl_voxel_batch import synthetic_grids
    lib = _lib.load()
    grid = synthetic_grids(max(B, 3), H, W, bins, np.float64, seed=B + bins)
    grid = np.ascontiguousarray(grid[1:2] if B == 1 else grid)       # (alone: the dense window, where a one-pass variance cancels)
    assert grid.shape == (B, H, W, bins)
    nbytes = int(lib.evrep_voxel_normalize_scratch_bytes(B, H, W, bins))
    assert nbytes == 3 * B * 1024 + up256(B * 16) and (B != 16 or nbytes == 3 * B * 1024 + B * 16)

    def call(g):
        d, out = g.inp(grid, "grid"), g.out((B, bins, H, W), torch.float32, "out")
        stats, sc = g.out((B, 4), torch.float64, "stats"), g.scratch(nbytes)
        _lib.check(lib.evrep_voxel_normalize(g.p(d), _lib.F64, B, H, W, bins, _lib.VOXNORM_NORMALIZE, g.p(out), g.p(stats), g.p(sc),
                                             _sp()), "evrep_voxel_normalize")
        return {"out": out, "stats": stats}

    got = drive(call, "voxel_normalize")
    for b in range(B):
        assert_matches_restatement(got["out"][b], got["stats"][b], np.ascontiguousarray(grid[b].transpose(2, 0, 1)), "window %d" % b)


# ---------------------------------------------------------------------------------------------------------------- filter compaction
@pytest.mark.parametrize("total", [0, 1, 1023, 1024, 1025, 1024 * 1024 + 1])
def test_filter_compact(total):
    """evrep_filter_compact_scratch_bytes is a constant (one count and one offset per slice).  events_out holds exactly the kept
    rows; three windows, one of them empty, that start inside a slice; 1024 * 1024 + 1 rows: a second round of every slice."""
    lib = _lib.load()
    rng = np.random.default_rng(total)
    B = 3
    off = np.array([0, total // 3, total // 3, total], np.int64)
    ev = rng.integers(-2 ** 31, 2 ** 31 - 1, size=(total, 4)).astype(np.int32)
    keep = (rng.random(total) < 0.4).astype(np.uint8)
    kept = int(keep.sum())
    nbytes = int(lib.evrep_filter_compact_scratch_bytes(B, total))
    assert nbytes == int(lib.evrep_filter_compact_scratch_bytes(1, 0)) == int(lib.evrep_filter_compact_scratch_bytes(65535, 1 << 30))

    def call(g):
        d_ev, d_off, d_keep = g.inp(ev, "events"), g.inp(off, "offsets"), g.inp(keep, "keep")
        out, off_out, sc = g.out((kept, 4), torch.int32, "events_out"), g.out((B + 1,), torch.int64, "offsets_out"), g.scratch(nbytes)
        _lib.check(lib.evrep_filter_compact(g.p(d_ev), g.p(d_off), B, g.p(d_keep), g.p(out), g.p(off_out), g.p(sc), _sp()),
                   "evrep_filter_compact")
        return {"events_out": out, "offsets_out": off_out}

    got = drive(call, "filter_compact total %d" % total)
    assert_bit_equal(got["events_out"], ev[keep.astype(bool)], "kept rows")
    want_off = np.concatenate([[0], np.cumsum([int(keep[off[b]:off[b + 1]].sum()) for b in range(B)])]).astype(np.int64)
    assert_bit_equal(got["offsets_out"], want_off, "offsets_out")


# ---------------------------------------------------------------------------------------------------------------- EST backward
@pytest.mark.parametrize("n,nseg", [(1024, 16), (1025, 8), (65, 1), (1, 16)])
def test_est_voxel_backward(n, nseg):
    """evrep_est_backward_scratch_bytes(total, nseg) = up256(4096 + rows * 2 * nseg * 8), rows = ceil(total / 1024) (at most 512):
    total = 1024, nseg = 16 -> 4096 + 256; total = 1025, nseg = 8 -> two rows of 128 bytes = 256: no slack; nseg = 1: 16 bytes.
    The exact inputs of test_est_train_cpu (every product and sum exact): grad_seg equals the restatement bit for bit."""
    from test_est_train_cpu import exact_case, restate
    lib = _lib.load()
    case = exact_case(n, 3, nseg, "own_piece")
    want = restate(case)
    nbytes = int(lib.evrep_est_backward_scratch_bytes(n, nseg))
    rows = (n + 1023) // 1024
    assert nbytes == up256(4096 + rows * 2 * nseg * 8) and (nseg == 1 or n == 1 or nbytes == 4096 + rows * 2 * nseg * 8)
    bucket = np.ascontiguousarray(case.table.bucket, dtype=np.int32)

    def call(g):
        ev, off, tn = g.inp(case.rows, "events"), g.inp(case.offsets, "offsets"), g.inp(case.tn, "tnorm")
        seg, bk, G_ = g.inp(case.table.seg, "segments"), g.inp(bucket, "buckets"), g.inp(case.G, "grad_out")
        grad, sc = g.out((nseg, 2), torch.float64, "grad_seg"), g.scratch(nbytes)
        rc = lib.evrep_est_voxel_backward(g.p(ev), g.p(off), 3, case.H, case.W, g.p(tn), case.C, g.p(seg), nseg, g.p(bk), bucket.size,
                                          float(case.table.lo), float(case.table.hi), g.p(G_), g.p(grad), g.p(sc), _sp())
        assert rc == _lib.EVREP_OK
        return {"grad": grad}

    got = drive(call, "est_voxel_backward")["grad"]
    assert np.array_equal(got.view(np.uint64), (want.grad + 0.0).view(np.uint64)), (n, nseg)
    assert not got[want.count == 0].any()


# ---------------------------------------------------------------------------------------------------------------- N-ImageNet front end
@pytest.mark.parametrize("B", [64, 1])
def test_nimg_prepare(B):
    """evrep_nimg_prepare_scratch_bytes(B, total) = up256(up256(1025 * 4) + B * 40 + B * 4) = up256(4352 + 44 B): B = 64 ->
    4352 + 2816 = 7168 = 28 * 256, the kept counts end on the scratch's last byte; B = 1.  Flipped and unflipped windows, empty
    ones, a window of one row; every output carved at `total` rows, the kept rows compared."""
    import types
    from event_representation_study_amd import n_imagenet_front as nf
    from test_gpu_nimg_front import expected, host, packed, params, same, synthetic
    lib = _lib.load()
    rng = np.random.default_rng(B)
    lengths = [(300, 0, 1, 65, 1024, 17)[b % 6] for b in range(B)] if B > 1 else [500]
    wins = [synthetic(n, rng) for n in lengths]
    par = params(nf, lengths, rng, time_flip=[(b + 1) % 2 for b in range(B)])
    front = types.SimpleNamespace(sx=1.0, sy=1.0, mode="train")
    want = expected(host(front, wins, par))
    rows, bases = zip(*(packed(*w) for w in wins))
    ev, off = np.concatenate(rows), np.zeros(B + 1, np.int64)
    np.cumsum(lengths, out=off[1:])
    total = int(off[-1])
    nbytes = int(lib.evrep_nimg_prepare_scratch_bytes(B, total))
    assert nbytes == up256(4352 + 44 * B) and (B != 64 or nbytes == 4352 + 44 * B)

    def call(g):
        d_ev, d_off = g.inp(ev, "events"), g.inp(off, "offsets")
        d_tb, d_par = g.inp(np.asarray(bases, np.int64), "t_base"), g.inp(par.view(np.uint8), "params")
        ev_out, t_out, tn_out = g.out((total, 4), torch.int32, "events_out"), g.out((total,), torch.float64, "t_out"), g.out((total,), torch.float64, "tnorm_out")
        xy_out, off_out, st_out = g.out((total, 2), torch.float64, "xy_out"), g.out((B + 1,), torch.int64, "offsets_out"), g.out((B,), torch.int32, "status_out")
        sc = g.scratch(nbytes)
        _lib.check(lib.evrep_nimg_prepare(g.p(d_ev), g.p(d_off), B, g.p(d_tb), g.p(d_par), 1.0, 1.0, 224, 224, _lib.NIMG_P_UINT8 | _lib.NIMG_TRAIN,
                                          g.p(ev_out), g.p(t_out), g.p(tn_out), g.p(xy_out), g.p(off_out), g.p(st_out), g.p(sc), _sp()),
                   "evrep_nimg_prepare")
        torch.cuda.synchronize()
        kept = int(off_out[-1])         # (the rows behind the kept ones are not written: they keep the fill)
        return {"events": ev_out[:kept], "t": t_out[:kept], "tnorm": tn_out[:kept], "xy": xy_out[:kept], "offsets": off_out, "status": st_out}

    got = drive(call, "nimg_prepare")
    same(got["offsets"], want["offsets"], "offsets")
    same(got["status"].view(np.uint32), want["status"], "status")
    for k in ("events", "t", "tnorm", "xy"):
        same(got[k], want[k], k)
    assert 0 < int(want["offsets"][-1]) and (B == 1 or (want["status"] & _lib.AUG_EMPTY).any())


# ---------------------------------------------------------------------------------------------------------------- raw event files
@pytest.mark.parametrize("fmt,name,H,W", [("dat", "oob", None, None), ("bin", "n1025", 200, 180)])
def test_decode_drop_oob(fmt, name, H, W):
    """evrep_decode_scratch_bytes is a constant (a header and one count and one offset per slice).  DROP_OOB, the chunk lengths of
    test_gpu_decode.py: the columns carved at `capacity` entries, every raw chunk read-only and padded to 16 bytes as the header
    asks, the state carved."""
    from test_gpu_decode import CHUNKS, DTYPES, SENSOR_H, SENSOR_W, _G, expected_state, golden_columns, oob_mask
    lib = _lib.load()
    H, W = (SENSOR_H, SENSOR_W) if H is None else (H, W)
    want = golden_columns(fmt, name)
    keep = ~oob_mask(want, H, W)
    kept, n = int(keep.sum()), len(keep)
    assert 0 < kept < n
    raw = np.frombuffer(bytes(_G["%s.%s.payload" % (fmt, name)]), np.uint8)
    rec_bytes = 8 if fmt == "dat" else 5
    nbytes = int(lib.evrep_decode_scratch_bytes(1))
    assert nbytes == int(lib.evrep_decode_scratch_bytes(n)) == int(lib.evrep_decode_scratch_bytes(1 << 30)) and nbytes % 256 == 0
    tdt = {"x": torch.int16, "y": torch.int16, "t": torch.int64, "p": torch.int8}
    for chunk in (n,) + tuple(CHUNKS):
        def call(g):
            cols = {f: g.out((n,), tdt[f], f) for f in "xytp"}
            state, sc = g.out((8,), torch.int64, "state"), g.scratch(nbytes)
            _lib.check(lib.evrep_decode_state_init(g.p(state), _sp()))
            for first in range(0, n, chunk):
                m = min(chunk, n - first)
                piece = np.zeros((m * rec_bytes + 15) // 16 * 16, np.uint8)
                piece[:m * rec_bytes] = raw[first * rec_bytes:(first + m) * rec_bytes]
                d = g.inp(piece, "raw%d" % first)
                args = (first, H, W, _lib.DECODE_DROP_OOB, g.p(cols["x"]), g.p(cols["y"]), g.p(cols["t"]), g.p(cols["p"]), n, g.p(state),
                        g.p(sc), _sp())
                if fmt == "dat":
                    _lib.check(lib.evrep_decode_dat(g.p(d), m, 8, *args), "evrep_decode_dat")
                else:
                    _lib.check(lib.evrep_decode_bin5(g.p(d), m, *args), "evrep_decode_bin5")
            return dict({f: cols[f][:kept] for f in "xytp"}, state=state)

        got = drive(call, "decode %s chunk %d" % (fmt, chunk))
        st = dict(zip(_lib.DECODE_STATE_FIELDS, (int(v) for v in got["state"])))
        assert st == expected_state(want, H, W, kept=kept), (chunk, st)
        for f in "xytp":
            assert np.array_equal(got[f].view(DTYPES[f]), want[f][keep]), (chunk, f)


# ---------------------------------------------------------------------------------------------------------------- outputs of calls without scratch
def test_windows_gather_and_time_to_index():
    """evrep_time_to_index and evrep_windows_gather take no scratch: their outputs carved at the documented sizes -- out_idx [nq],
    events_out exactly dst_offsets[B] rows, base_out and status_out [B] -- the recording's columns read-only.  Overlapping, equal,
    empty and one-event ranges (test_gpu_evl_windows)."""
    from test_gpu_evl_windows import expected_rows, first_bases
    lib = _lib.load()
    rng = np.random.default_rng(21)
    n = 5000
    x, y = rng.integers(0, 304, n).astype(np.uint16), rng.integers(0, 240, n).astype(np.uint16)
    t = np.sort(rng.integers(0, 2_000_000, n)).astype(np.int64) + 5_000_000_000
    p = rng.choice([-1, 1], n).astype(np.int8)
    q = np.concatenate([rng.integers(t[0] - 10, t[-1] + 10, 77), t[::500], [t[0] - 1, t[-1], t[-1] + 1]]).astype(np.int64)
    i0 = np.array([0, 0, 10, 10, 500, 500, 4000, n - 1, n, 3], np.int64)
    i1 = np.array([1000, 1000, 10, 11, 500, 1524, 4063, n, n, 1028], np.int64)
    B = len(i0)
    dst = np.zeros(B + 1, np.int64)
    np.cumsum(i1 - i0, out=dst[1:])
    total = int(dst[-1])

    def call(g):
        dx, dy, dt_, dp = g.inp(x.view(np.int16), "x"), g.inp(y.view(np.int16), "y"), g.inp(t, "t"), g.inp(p, "p")
        dq, idx = g.inp(q, "queries"), g.out((len(q),), torch.int64, "out_idx")
        assert lib.evrep_time_to_index(g.p(dt_), n, g.p(dq), len(q), g.p(idx), _sp()) == _lib.EVREP_OK
        d0, d1, dd = g.inp(i0, "i0"), g.inp(i1, "i1"), g.inp(dst, "dst_offsets")
        rows, base, st = g.out((total, 4), torch.int32, "events_out"), g.out((B,), torch.int64, "base_out"), g.out((B,), torch.int32, "status_out")
        rc = lib.evrep_windows_gather(g.p(dx), g.p(dy), g.p(dt_), g.p(dp), n, g.p(d0), g.p(d1), g.p(dd), B, _lib.REBASE_FIRST, None,
                                      g.p(rows), g.p(base), g.p(st), _sp())
        assert rc == _lib.EVREP_OK
        return {"idx": idx, "rows": rows, "base": base, "status": st}

    got = drive(call, "windows")
    assert_bit_equal(got["idx"], np.searchsorted(t, q, side="right").astype(np.int64), "time_to_index")
    bases = first_bases(t, i0, i1)
    rows, offs = expected_rows((x, y, t, p), i0, i1, bases)
    assert_bit_equal(got["rows"], rows, "gathered rows")
    assert_bit_equal(got["base"], bases, "base_out")
    assert not got["status"].any()


@pytest.mark.parametrize("H,W,C,nh,nw,mode", [(9, 16, 12, 8, 8, "area"), (37, 53, 5, 64, 71, "linear")])
def test_resize_taps(H, W, C, nh, nw, mode):
    """evrep_resize_taps takes no scratch: out carved at exactly B * Ho * Wo * C elements, the representation and the six tap
    tables read-only; against the dense weight matrices, as test_resize_taps_kernel_equals_dense_weight_matrices."""
    from event_representation_study_amd import gwd_pipeline as gp
    lib = _lib.load()
    rng = np.random.default_rng(H + W)
    rep = rng.random((2, H, W, C)) * 255.0
    fn = gp.area_weights if mode == "area" else gp.linear_weights
    want = np.einsum("yi,bijc,xj->byxc", fn(H, nh), rep, fn(W, nw))
    ys, yc, yw, Ty = gp.resize_taps(H, nh, mode, DEV)
    xs, xc, xw, Tx = gp.resize_taps(W, nw, mode, DEV)
    T = max(Ty, Tx)
    yw, xw = torch.nn.functional.pad(yw, (0, T - Ty)).contiguous(), torch.nn.functional.pad(xw, (0, T - Tx)).contiguous()

    def call(g):
        d = g.inp(rep, "rep")
        tabs = [g.inp(v, k) for k, v in (("ystart", ys), ("ycount", yc), ("ywt", yw), ("xstart", xs), ("xcount", xc), ("xwt", xw))]
        out = g.out((2, nh, nw, C), torch.float64, "out")
        _lib.check(lib.evrep_resize_taps(g.p(d), _lib.F64, 2, H, W, C, nh, nw, T, *(g.p(v) for v in tabs), 1.0, _lib.F64, g.p(out), _sp()),
                   "evrep_resize_taps")
        return {"out": out}

    np.testing.assert_allclose(drive(call, "resize_taps")["out"], want, rtol=1e-13, atol=1e-12)


# ---------------------------------------------------------------------------------------------------------------- GWD / OTMI
def _gwd_call(lib, Xs, Xt, nbytes):
    def call(g):
        a, b = g.inp(Xs, "Xs"), g.inp(Xt, "Xt")
        cost, sc = g.out((1,), torch.float64, "cost"), g.scratch(nbytes)
        _lib.check(lib.evrep_gwd_padded_l1(g.p(a), Xs.shape[0], Xs.shape[1], g.p(b), Xt.shape[0], Xt.shape[1], 0.7, g.p(sc), g.p(cost),
                                           _sp()), "evrep_gwd_padded_l1")
        return {"cost": cost}
    return call


@pytest.mark.parametrize("n,m", [(128, 128), (129, 5), (1, 2), (1921, 77)])
def test_gwd_padded_l1(oracle, n, m):
    """evrep_gwd_scratch_bytes(n, m), with L = max(n, m), T = ceil(L / 128) tiles per side:
        up256((2 * 64 * 2 * 32 + 2 * 33) * 8) [statistics: 66 064 -> 66 304, always 240 bytes of slack]
      + 2 * 192 * pad128(n) + 2 * 192 * pad128(m) [the scaled clouds: 192 * 128 = 96 * 256, never any slack]
      + up256(T (T + 1) / 2 * 4 * 8) [per-tile, per-wave sums: the LAST region].
    16 T (T + 1) is a multiple of 256 for T = 15, 16: n = 1921 -> T = 16, 4352 bytes = 17 * 256, the sums end on the scratch's
    last byte.  (128, 128): one tile, both clouds exactly one padded tile; (129, 5): one row over; (1, 2): the smallest."""
    lib = _lib.load()
    rng = np.random.default_rng(n + m)
    Xs, Xt = rng.random((n, 4)), rng.random((m, 14)) * 255.0
    pad = lambda v: (v + 127) // 128 * 128
    T = pad(max(n, m)) // 128
    nbytes = int(lib.evrep_gwd_scratch_bytes(n, m))
    assert nbytes == 66304 + 2 * 192 * (pad(n) + pad(m)) + up256(16 * T * (T + 1)) and (n != 1921 or 16 * T * (T + 1) % 256 == 0)
    got = float(drive(_gwd_call(lib, Xs, Xt, nbytes), "gwd %d x %d" % (n, m))["cost"][0])
    with np.errstate(all="ignore"):
        ref = oracle.gwd(Xs, Xt)
    if n == 1:      # a cloud of one point has no variance: the reference's kernel width is 0 / 0, its cost NaN -- and so is this one
        assert np.isnan(ref) and np.isnan(got), (got, ref)
    else:
        assert abs(got - ref) <= 1e-5 * ref, (got, ref)      # (test_gpu_gwd_batch: the reference's budget)


def _gwd_batch_parts(lib, P, ds, dt, n_cap, m_cap):
    """The regions of evrep_gwd_batch_scratch_bytes (gwd_batch_layout), with the sizes that are not public -- a pair's table entry,
    a point's bytes in the scaled clouds -- taken from the function itself by differences: (pair table, clouds, tile sums payload)."""
    f = lambda P_, n_, m_: int(lib.evrep_gwd_batch_scratch_bytes(P_, ds, dt, n_, m_))
    pad = lambda v: (v + 127) // 128 * 128
    tiles = lambda n_, m_: (pad(max(n_, m_)) // 128) * (pad(max(n_, m_)) // 128 + 1) // 2
    big = 128 * 64                                                   # (one side far larger: the tile count stays put)
    fs = (f(1, 256, big) - f(1, 128, big)) // (2 * 128)              # bytes per point and form of a source cloud
    ft = (f(1, big, 256) - f(1, big, 128)) // (2 * 128)
    assert fs > 0 and ft > 0 and fs * 128 % 256 == 0 and ft * 128 % 256 == 0      # whole padded tiles: these regions never have slack
    clouds = P * 2 * (fs * pad(n_cap) + ft * pad(m_cap))
    rest = lambda P_: f(P_, 128, 128) - 256 - P_ * 66304 - P_ * 2 * 128 * (fs + ft) - up256(P_ * 1 * 32)
    pair = rest(256) // 256                                          # sizeof(GwdPair): 256 of them are a multiple of 256 bytes
    assert pair * 256 == rest(256) and 0 < pair
    return up256(P * pair), clouds, P * tiles(n_cap, m_cap) * 4 * 8


@pytest.mark.parametrize("ns,ms,n_cap,m_cap", [([129, 2, 200], [128, 260, 77], 200, 260), ([300, 2, 129, 257], [384, 128, 260, 77], 300, 384)],
                         ids=["P3_ragged", "P4_no_slack"])
def test_gwd_padded_l1_batch(oracle, ns, ms, n_cap, m_cap):
    """evrep_gwd_batch_scratch_bytes(P, ds, dt, n_cap, m_cap) (gwd_batch_layout), with T = ceil(max(n_cap, m_cap) / 128):
        up256(P * sizeof(pair entry)) + 256 [a total] + P * 66 304 [statistics, 240 bytes of slack each, as in the single solve]
      + P * 2 * (bytes per point * pad128(n_cap) + bytes per point * pad128(m_cap)) [the scaled clouds: whole tiles, never any slack]
      + up256(P * T (T + 1) / 2 * 4 * 8) [per-pair, per-tile, per-wave sums: the LAST region].
    P = 4 with caps 300 / 384: T = 3, 4 * 6 * 32 = 768 = 3 * 256: the sums end on the scratch's last byte.  P = 3 with caps 200 / 260:
    T = 3, 576 bytes in 768.  Ragged pairs, one with n = n_cap (and, in the second case, one with m = m_cap), in slots of n_cap /
    m_cap rows; the costs equal the single solves bit for bit (test_gpu_gwd_batch) and the oracle within 1e-5."""
    from event_representation_study_amd import engine as eng
    lib = _lib.load()
    rng = np.random.default_rng(9)
    ds, dt = 4, 14
    Xs, Xt = [rng.random((k, ds)) for k in ns], [rng.random((k, dt)) * 255.0 for k in ms]
    P = len(ns)
    assert max(ns) == n_cap and max(ms) <= m_cap
    big_s, big_t = np.zeros((P * n_cap, ds)), np.zeros((P * m_cap, dt))
    for p, (a, b) in enumerate(zip(Xs, Xt)):
        big_s[p * n_cap: p * n_cap + len(a)], big_t[p * m_cap: p * m_cap + len(b)] = a, b
    nbytes = int(lib.evrep_gwd_batch_scratch_bytes(P, ds, dt, n_cap, m_cap))
    table, clouds, sums = _gwd_batch_parts(lib, P, ds, dt, n_cap, m_cap)
    assert nbytes == table + 256 + P * 66304 + clouds + up256(sums)
    if P == 4:
        assert sums == 768 and nbytes == table + 256 + P * 66304 + clouds + sums and max(ms) == m_cap

    def call(g):
        a, b = g.inp(big_s, "Xs"), g.inp(big_t, "Xt")
        dn, dm = g.inp(np.array(ns, np.int64), "n"), g.inp(np.array(ms, np.int64), "m")
        costs, sc = g.out((P,), torch.float64, "costs"), g.scratch(nbytes)
        _lib.check(lib.evrep_gwd_padded_l1_batch(P, g.p(a), None, g.p(dn), ds, g.p(b), None, g.p(dm), dt, n_cap, m_cap, 0.7, g.p(sc),
                                                 g.p(costs), _sp()), "evrep_gwd_padded_l1_batch")
        return {"costs": costs}

    got = drive(call, "gwd batch")["costs"]
    single = np.array([float(eng.gwd_padded_l1(a, b).item()) for a, b in zip(Xs, Xt)])
    assert np.array_equal(got, single), (got, single)
    for p in range(P):
        ref = oracle.gwd(Xs[p], Xt[p])
        assert abs(got[p] - ref) <= 1e-5 * ref, (p, got[p], ref)


def _otmi_no_slack_count(lib):
    """The per-window bytes of evrep_otmi_scratch_bytes from the function itself (256 windows: a whole number of them is a
    multiple of 256 bytes) -> the smallest count whose scratch has no slack."""
    per = int(lib.evrep_otmi_scratch_bytes(256)) // 256
    assert per * 256 == int(lib.evrep_otmi_scratch_bytes(256))
    return per, 256 // np.gcd(per, 256)


@pytest.mark.parametrize("B", [1, 3, "no_slack"])
def test_otmi_clouds(B):
    """evrep_otmi_scratch_bytes(count) = up256(count * max(per-window bytes of the event harness, 3 * 32 * 4 of the representation
    harness)); the count without slack is derived from the function's own per-window size.  Xs / Xt carved at cap / m_cap rows per
    slot, the written rows compared with compute_otmi.otmi_point_clouds bit for bit (test_gpu_gwd_batch)."""
    from event_representation_study_amd.representations.representation_search.compute_otmi import otmi_point_clouds
    from event_representation_study_amd.synthetic import make_events
    lib = _lib.load()
    per, nos = _otmi_no_slack_count(lib)
    if B == "no_slack":
        B = int(nos)
        assert B <= 64 and int(lib.evrep_otmi_scratch_bytes(B)) == per * B
    H, W, S, C = 24, 30, 17, 5
    rng = np.random.default_rng(B)
    sizes = [(500, 120, 333, 64, 65)[b % 5] for b in range(B)]
    wins = [make_events(k, W, H, seed=40 + b, polarity="pm1" if b % 2 else "01") for b, k in enumerate(sizes)]
    reps = np.stack([rng.random((S, S, C)) * (rng.random((S, S, 1)) < 0.3) for _ in range(B)])
    reps[:, :2] = 114.0
    off = np.zeros(B + 1, np.int64)
    np.cumsum(sizes, out=off[1:])
    cap, m_cap = max(sizes), (S - (S // 2 - 1)) ** 2
    nbytes = int(lib.evrep_otmi_scratch_bytes(B))
    assert nbytes == up256(per * B)

    def call(g):
        ev, d_off, rp = g.inp(np.concatenate(wins), "events"), g.inp(off, "offsets"), g.inp(reps, "rep")
        Xs, n, quad = g.out((B, 3, cap, 4), torch.float64, "Xs"), g.out((B, 3), torch.int64, "n_out"), g.out((B, 3), torch.int32, "quad_out")
        Xt, m = g.out((B, 3, m_cap, C + 2), torch.float64, "Xt"), g.out((B, 3), torch.int64, "m_out")
        sc1, sc2 = g.scratch(nbytes, "scratch (events)"), g.scratch(nbytes, "scratch (rep)")
        _lib.check(lib.evrep_otmi_event_clouds(g.p(ev), g.p(d_off), B, H, W, cap, g.p(Xs), g.p(n), g.p(quad), g.p(sc1), _sp()), "event clouds")
        _lib.check(lib.evrep_otmi_rep_clouds(g.p(rp), _lib.F64, B, B, S, C, g.p(quad), m_cap, g.p(Xt), g.p(m), g.p(sc2), _sp()), "rep clouds")
        torch.cuda.synchronize()
        nn, mm = n.cpu().numpy(), m.cpu().numpy()
        res = {"n": n, "m": m, "quad": quad}
        for b in range(B):
            for k in range(3):          # (the rows behind a cloud's own are not written)
                res["Xs%d_%d" % (b, k)], res["Xt%d_%d" % (b, k)] = Xs[b, k, :nn[b, k]], Xt[b, k, :mm[b, k]]
        return res

    got = drive(call, "otmi clouds")
    for b in range(B):
        host = otmi_point_clouds(torch.from_numpy(wins[b]), reps[b], H, W, S)
        assert len(host) == 3
        for k, (hs, ht) in enumerate(host):
            assert got["n"][b, k] == len(hs) and got["m"][b, k] == len(ht), (b, k)
            assert np.array_equal(got["Xs%d_%d" % (b, k)], hs.astype(np.float64)) and np.array_equal(got["Xt%d_%d" % (b, k)], ht), (b, k)


# ---------------------------------------------------------------------------------------------------------------- entropic GW
@pytest.mark.parametrize("n,m,precision,loss,eps", [(17, 129, "f64", "kl_loss", 0.1), (64, 64, "f64", "square_loss", 0.05),
                                                    (128, 128, "f32", "square_loss", 0.5)])
def test_entropic_gw(n, m, precision, loss, eps):
    """evrep_gw_scratch_bytes(n, m, precision): sizes off and on the tile edges (the padded pitch), both precisions, 2 outer and 5
    Sinkhorn iterations, T_out given and NULL; against oracle/gw_oracle.py with the tolerances of test_gpu_gw_solver."""
    from oracle import gw_oracle
    from test_gpu_gw_solver import _problem
    lib = _lib.load()
    C1, C2, p, q = _problem(n, m, seed=n + m)
    prec = {"f64": _lib.F64, "f32": _lib.F32}[precision]
    code = {"square_loss": 0, "kl_loss": 1}[loss]
    nbytes = int(lib.evrep_gw_scratch_bytes(n, m, prec))
    assert nbytes > 0 and nbytes % 256 == 0
    Tref, gref = gw_oracle.entropic_gromov_wasserstein(C1, C2, p, q, loss, epsilon=eps, outer_iters=2, sinkhorn_iters=5)
    res = {}
    for plan in (True, False):
        def call(g):
            a, b, dp, dq = g.inp(C1, "C1"), g.inp(C2, "C2"), g.inp(p, "p"), g.inp(q, "q")
            T = g.out((n, m), torch.float64, "T_out") if plan else None
            gw, sc = g.out((1,), torch.float64, "gw_out"), g.scratch(nbytes)
            _lib.check(lib.evrep_entropic_gw(g.p(a), n, g.p(b), m, g.p(dp), g.p(dq), code, eps, 2, 5, prec, g.p(sc), g.p(T) if plan else None,
                                             g.p(gw), _sp()), "evrep_entropic_gw")
            return {"T": T, "gw": gw} if plan else {"gw": gw}

        res[plan] = drive(call, "entropic gw %s plan %s" % (precision, plan))
    assert res[True]["gw"][0] == res[False]["gw"][0]
    gw, T = float(res[True]["gw"][0]), res[True]["T"]
    if precision == "f64":
        assert abs(gw - gref) <= 1e-9 * abs(gref), (gw, gref)
        np.testing.assert_allclose(T, Tref, rtol=1e-8, atol=1e-14)
    else:
        assert abs(gw - gref) <= 1e-5 * abs(gref), (gw, gref)
        np.testing.assert_allclose(T, Tref, rtol=2e-4, atol=1e-12)


# ---------------------------------------------------------------------------------------------------------------- detector input, frames
@pytest.mark.parametrize("B", [32, 1])
def test_detector_input_frames_table(B, monkeypatch):
    """evrep_detector_input_frames_scratch_bytes(B) = B * 88 sizes frames_dev, the device copy of the caller's table: B = 32 ->
    2816 = 11 * 256.  DetectorFrontEnd.prepare_frames builds the table; the C entry is driven with a carved frames_dev of exactly
    that size and a carved out.  The region is an INPUT of the kernel: after the launch it still equals the host table."""
    import test_gpu_detector_input_frames as F
    lib = _lib.load()
    nbytes = int(lib.evrep_detector_input_frames_scratch_bytes(B))
    assert nbytes == B * ctypes.sizeof(_lib.DetinFrame) == B * 88 and (B != 32 or nbytes % 256 == 0)
    sizes = [F.SIZES[b % len(F.SIZES)] for b in range(B)]
    frames = F._frames(5, np.float32, seed=B, sizes=sizes)
    mats0, flips0 = F._train_mix()
    mats, flips = [mats0[b % 7] for b in range(B)], [flips0[b % 7] for b in range(B)]
    want = F._want(frames, True, mats, flips)
    api = _lib.api()                                  # the handle prepare_frames calls through
    real = api.evrep_detector_input_frames
    state = {}

    def carved_call(table, B_, dt, C, S, start, count, wts, n_rows, n_wt, pad, warp, scale, frames_dev, out, stream):
        g = state["g"]
        state["table"] = ctypes.string_at(table, nbytes)
        state["dev"] = g.scratch(nbytes, "frames_dev")
        return real(table, B_, dt, C, S, start, count, wts, n_rows, n_wt, pad, warp, scale, g.p(state["dev"]), out, stream)

    monkeypatch.setattr(api, "evrep_detector_input_frames", carved_call)

    def call(g):
        state["g"] = g
        d_frames = [g.inp(f, "frame%d" % b) for b, f in enumerate(frames)]
        out = g.out((B, 5, F.S, F.S), torch.float32, "out")
        got = F._front(F.S, True).prepare_frames(d_frames, params=F._params(mats, flips), scale=None, out=out)[0]
        assert got.data_ptr() == out.data_ptr()
        torch.cuda.synchronize()
        assert state["dev"].cpu().numpy().tobytes() == state["table"], "the kernel's copy of the table changed"
        return {"out": out}

    F._assert_bits(torch.from_numpy(drive(call, "detector input frames")["out"]), want, "frames B=%d" % B)
