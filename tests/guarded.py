"""Guarded buffers for the size contracts of include/evrep.h: every workspace, scratch, output and input region a test hands
to the library is cut out of a larger torch allocation, exactly as long as the header says, with a band of known pseudo-random
bytes in front of it and behind it.  Shared by test_guarded_cpu.py, test_gpu_workspace_contract.py and
test_gpu_scratch_contracts.py; nothing here needs a device (Arena("cpu", seed) works on host tensors).

Why: torch's caching allocator rounds every request up and gives a test of one shape the same block back, so a kernel that
writes a record past its region, or reads scratch it never wrote, goes unseen with torch.empty(nbytes).  No sanitizer runs on the
device, so the bands and a poisoned interior are the only way to see either.

    arena = Arena("cuda:0", seed=1)
    ws = arena.carve(nbytes, fill="ones", name="workspace")        # uint8 view, data_ptr() % 256 == 0, tail guard at byte nbytes
    out = arena.carve_shape((B, H, W, 12), torch.float64, name="out")
    ev = arena.carve_like(events, name="events")                   # a copy of `events`, registered read-only
    ...
    arena.check()            # every guard band still holds its bytes
    arena.check_inputs()     # every read-only region still holds its contents

Guard width on each side: min(max(nbytes, 64 KiB), 4 MiB).  The bands hold bytes of numpy.random.default_rng(seed), not a
constant: a stray memset of zeros or 0xFF, or a stray 0.0, differs from them (a store of 4 zero bytes matches the band with
probability 2^-32).  `fill` poisons the interior: "zeros", "ones" (0xFF bytes) or "random" (the same generator).

A GuardError names the region, the side and the first and last changed byte.  Offsets are relative to the region: for the
head band they are negative (-1 = the last byte in front of the region), for the tail band they count from the region's end
(0 = the first byte behind it, which is byte `nbytes` of the region), for a read-only region they are offsets into it.
"""
import numpy as np
import torch

GUARD_MIN = 64 * 1024
GUARD_MAX = 4 * 1024 * 1024
FILLS = ("zeros", "ones", "random")


def guard_bytes(nbytes):
    return min(max(int(nbytes), GUARD_MIN), GUARD_MAX)


class GuardError(AssertionError):
    def __init__(self, region, side, first, last, count):
        self.region, self.side, self.first, self.last, self.count = region, side, first, last, count
        what = "read-only contents changed" if side == "contents" else "%s guard touched" % side
        super().__init__("region %r: %s, %d byte(s) between offsets %d and %d" % (region, what, count, first, last))


class _Region:
    __slots__ = ("name", "buf", "pristine", "start", "nbytes", "guard", "ptr", "readonly")


class Arena:
    def __init__(self, device="cpu", seed=0):
        self.device = torch.device(device)
        self.rng = np.random.default_rng(seed)
        self.regions = []

    def _random(self, n):
        return torch.from_numpy(self.rng.integers(0, 256, size=int(n), dtype=np.uint8))

    def carve(self, nbytes, align=256, fill="random", name=None, readonly=False):
        """A uint8 view of exactly `nbytes` whose data_ptr() is a multiple of `align`; the tail guard begins at byte `nbytes`."""
        nbytes, align = int(nbytes), int(align)
        if nbytes < 0 or align < 1:
            raise ValueError("carve(%d, align=%d)" % (nbytes, align))
        if fill not in FILLS:
            raise ValueError("fill must be one of %r" % (FILLS,))
        g = guard_bytes(nbytes)
        raw = torch.empty(g + align - 1 + nbytes + g, dtype=torch.uint8, device=self.device)
        lo = (-(raw.data_ptr() + g)) % align          # the first offset >= g at which the address is a multiple of align
        r = _Region()
        r.name = name if name is not None else "region%d" % len(self.regions)
        r.buf = raw[lo: lo + g + nbytes + g]           # head band, region, tail band: nothing else is looked at
        r.start, r.nbytes, r.guard, r.readonly = g, nbytes, g, bool(readonly)
        r.ptr = raw.data_ptr() + lo + g
        if fill == "random":
            host = self._random(r.buf.numel())
        else:       # (the generator is only asked for what stays pseudo-random: a large zero-filled output is cheap to carve)
            host = torch.full((r.buf.numel(),), 0 if fill == "zeros" else 0xFF, dtype=torch.uint8)
            host[:g], host[g + nbytes:] = self._random(g), self._random(g)
        r.buf.copy_(host)
        r.pristine = r.buf.clone()
        self.regions.append(r)
        view = r.buf[g: g + nbytes]
        assert r.ptr % align == 0 and (nbytes == 0 or view.data_ptr() == r.ptr)
        return view

    def carve_shape(self, shape, dtype, fill="random", name=None, align=256):
        """A contiguous view of `shape` and `dtype`, exactly numel * itemsize bytes long."""
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        item = torch.empty(0, dtype=dtype).element_size()
        n = int(np.prod(shape, dtype=np.int64)) if shape else 1
        align = max(int(align), item)
        if align % item:
            raise ValueError("align %d is no multiple of the element size %d" % (align, item))
        return self.carve(n * item, align, fill, name).view(dtype).view(shape)

    def carve_like(self, tensor, name=None, readonly=True, align=256):
        """A guarded copy of `tensor` (any device), its last byte directly in front of the tail guard; read-only regions are
        compared whole by check_inputs()."""
        t = tensor.detach().contiguous()
        view = self.carve_shape(tuple(t.shape), t.dtype, "random", name, align)
        view.copy_(t)
        r = self.regions[-1]
        r.readonly = bool(readonly)
        r.pristine = r.buf.clone()
        return view

    def ptr(self, index=-1):
        """The address of a region (a zero-size view has no data_ptr() of its own)."""
        return self.regions[index].ptr

    @staticmethod
    def _diff(r, lo, hi, side, base):
        a, b = r.buf[lo:hi], r.pristine[lo:hi]
        if torch.equal(a, b):
            return
        bad = np.flatnonzero(a.cpu().numpy() != b.cpu().numpy())
        raise GuardError(r.name, side, int(bad[0]) + base, int(bad[-1]) + base, int(bad.size))

    def check(self):
        """Every guard band equals its pristine copy."""
        for r in self.regions:
            self._diff(r, 0, r.start, "head", -r.guard)
            self._diff(r, r.start + r.nbytes, r.buf.numel(), "tail", 0)

    def check_inputs(self):
        """Every read-only region equals what it was registered with."""
        for r in self.regions:
            if r.readonly:
                self._diff(r, r.start, r.start + r.nbytes, "contents", 0)
