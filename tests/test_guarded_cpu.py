"""The guard helper of the size-contract tests (tests/guarded.py) bites, on host tensors: a change of one byte at either edge
of a region, at the far end of a band, a store of four zero bytes, and a changed byte of a read-only region are each reported with
the region, the side and the offset; a change inside a region is not."""
import numpy as np
import pytest
import torch

from guarded import FILLS, GUARD_MAX, GUARD_MIN, Arena, GuardError, guard_bytes


def _flip(buf, i):
    buf[i] = (int(buf[i]) + 1) & 0xFF


def _arena():
    a = Arena("cpu", seed=7)
    first = a.carve(1000, name="first")
    mid = a.carve(300, fill="zeros", name="mid")
    last = a.carve(4096, fill="ones", name="last")
    return a, first, mid, last


def _raises(a, fn=None):
    with pytest.raises(GuardError) as e:
        (fn or a.check)()
    return e.value


def test_guard_width():
    assert guard_bytes(0) == GUARD_MIN == 64 * 1024 and guard_bytes(GUARD_MIN + 1) == GUARD_MIN + 1
    assert guard_bytes(1 << 30) == GUARD_MAX == 4 * 1024 * 1024
    a = Arena("cpu", seed=1)
    a.carve(100000, name="r")
    r = a.regions[0]
    assert r.start == r.guard == 100000 and r.buf.numel() == 300000


def test_clean_arena_and_interior_writes_are_silent():
    a, first, mid, last = _arena()
    a.check()
    a.check_inputs()
    mid[:] = 0x5A
    first[0], first[-1] = 1, 2
    last.zero_()
    a.check()
    a.check_inputs()


def test_first_byte_behind_a_region():
    a, first, mid, last = _arena()
    r = a.regions[1]
    _flip(r.buf, r.start + r.nbytes)
    e = _raises(a)
    assert (e.region, e.side, e.first, e.last, e.count) == ("mid", "tail", 0, 0, 1)
    assert "mid" in str(e) and "tail" in str(e)


def test_last_byte_in_front_of_a_region():
    a, first, mid, last = _arena()
    r = a.regions[2]
    _flip(r.buf, r.start - 1)
    e = _raises(a)
    assert (e.region, e.side, e.first, e.last, e.count) == ("last", "head", -1, -1, 1)


def test_far_end_of_the_tail_guard():
    a, first, mid, last = _arena()
    r = a.regions[0]
    _flip(r.buf, r.buf.numel() - 1)
    e = _raises(a)
    assert (e.region, e.side, e.first, e.last) == ("first", "tail", r.guard - 1, r.guard - 1)
    assert r.guard == GUARD_MIN


def test_far_end_of_the_head_guard():
    a, first, mid, last = _arena()
    _flip(a.regions[1].buf, 0)
    e = _raises(a)
    assert (e.region, e.side, e.first, e.last) == ("mid", "head", -GUARD_MIN, -GUARD_MIN)


def test_four_byte_zero_store_into_a_guard():
    """The bands are pseudo-random: a stray 0.0f / memset of zeros differs from them (the seed is fixed, so this cannot flake)."""
    a, first, mid, last = _arena()
    r = a.regions[1]
    lo = r.start + r.nbytes + 40
    assert r.buf[lo: lo + 4].any()
    r.buf[lo: lo + 4] = 0
    e = _raises(a)
    assert (e.region, e.side) == ("mid", "tail") and 40 <= e.first <= e.last <= 43
    # the same with 0xFF bytes in front of the region
    a, first, mid, last = _arena()
    r = a.regions[2]
    r.buf[r.start - 8: r.start - 4] = 0xFF
    e = _raises(a)
    assert (e.region, e.side) == ("last", "head") and -8 <= e.first <= e.last <= -5


def test_the_guards_are_not_a_constant():
    a = Arena("cpu", seed=3)
    a.carve(16, name="r")
    r = a.regions[0]
    head = r.buf[: r.start].numpy()
    assert len(np.unique(head)) == 256 and abs(float(head.mean()) - 127.5) < 2.0
    b = Arena("cpu", seed=4)
    b.carve(16, name="r")
    assert not torch.equal(b.regions[0].buf[:64], r.buf[:64])        # another seed, other bytes
    c = Arena("cpu", seed=3)
    c.carve(16, name="r")
    assert torch.equal(c.regions[0].buf, r.buf)                      # the same seed, the same bytes


def test_read_only_region():
    a = Arena("cpu", seed=5)
    src = torch.arange(24, dtype=torch.int32).reshape(6, 4)
    ev = a.carve_like(src, name="events")
    out = a.carve_shape((3, 5), torch.float64, name="out")
    assert ev.dtype == torch.int32 and tuple(ev.shape) == (6, 4) and torch.equal(ev, src) and ev.is_contiguous()
    assert a.regions[0].nbytes == 96 and a.regions[0].readonly and not a.regions[1].readonly
    out.fill_(1.0)                  # an output may change ...
    a.check()
    a.check_inputs()
    ev[4, 1] += 1                   # ... an input may not: int32 element 17 = bytes 68 .. 71, the low byte changes
    a.check()                       # (no guard was touched)
    e = _raises(a, a.check_inputs)
    assert (e.region, e.side, e.first, e.last, e.count) == ("events", "contents", 68, 68, 1)


@pytest.mark.parametrize("fill,want", [("zeros", 0), ("ones", 0xFF)])
def test_interior_fill(fill, want):
    a = Arena("cpu", seed=2)
    v = a.carve(777, fill=fill, name="s")
    assert v.dtype == torch.uint8 and v.numel() == 777 and bool((v == want).all())
    r = a.regions[0]
    assert len(np.unique(r.buf[: r.start].numpy())) == 256         # the bands stay pseudo-random
    assert set(FILLS) == {"zeros", "ones", "random"}
    with pytest.raises(ValueError):
        a.carve(8, fill="nan")


def test_random_interior_comes_from_the_seed():
    v1 = Arena("cpu", seed=11).carve(4096, fill="random")
    v2 = Arena("cpu", seed=11).carve(4096, fill="random")
    v3 = Arena("cpu", seed=12).carve(4096, fill="random")
    assert torch.equal(v1, v2) and not torch.equal(v1, v3) and len(np.unique(v1.numpy())) == 256


@pytest.mark.parametrize("align", [1, 16, 256, 4096])
@pytest.mark.parametrize("nbytes", [0, 1, 255, 256, 257])
def test_carving_honours_align(nbytes, align):
    a = Arena("cpu", seed=nbytes)
    for i in range(3):
        v = a.carve(nbytes, align=align, name="r%d" % i)
        r = a.regions[-1]
        assert v.numel() == nbytes and a.ptr() % align == 0
        if nbytes:
            assert v.data_ptr() == a.ptr() and v.data_ptr() % align == 0
        # the tail guard begins at byte nbytes exactly: no rounding of the region
        assert r.buf.data_ptr() + r.start == a.ptr() and r.buf.numel() == r.start + nbytes + r.guard
        was = int(r.buf[r.start + nbytes])
        _flip(r.buf, r.start + nbytes)
        e = _raises(a)
        assert (e.region, e.side, e.first) == ("r%d" % i, "tail", 0)
        r.buf[r.start + nbytes] = was
        if nbytes:
            _flip(r.buf, r.start + nbytes - 1)      # the region's own last byte is not guarded
        a.check()


def test_typed_views():
    a = Arena("cpu", seed=9)
    for dtype, item in ((torch.uint8, 1), (torch.int32, 4), (torch.float32, 4), (torch.float64, 8), (torch.int64, 8)):
        v = a.carve_shape((3, 7), dtype, fill="ones", name=str(dtype))
        assert v.dtype == dtype and tuple(v.shape) == (3, 7) and v.is_contiguous() and v.data_ptr() % 256 == 0
        assert a.regions[-1].nbytes == 21 * item
    v = a.carve_shape((0, 4), torch.int32, name="empty")
    assert tuple(v.shape) == (0, 4) and a.regions[-1].nbytes == 0 and a.ptr() % 256 == 0
    a.check()
