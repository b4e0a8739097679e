"""The cases of the head's decode and tail (event_representation_study_amd/detector_head.py), shared by the golden maker
(tests/golden/make_golden_detector_head.py) and the tests: a seeded builder of the per-level maps as the head's last
convolutions leave them.  The smallest shapes at which the tile, the level offsets and the row stores can go wrong.

    name     B  nc  R / DFL  level maps (h x w)                   strides        stands on
    default  2   2  16 yes   8x8, 4x4, 2x2 (N = 84)               8, 16, 32      the default
    odd      3   3  16 yes   5x7, 3x4, 2x2 (N = 51)               8, 16, 32      odd, non-square; offsets that are multiples of nothing
    four     3   2  16 yes   8x12, 4x6, 2x3, 1x2 (N = 128)        8, 16, 32, 64  the four-level head; a two-anchor level
    single   1   1  16 yes   as default                           8, 16, 32      one image, one class (row of 6)
    coco     2  80  16 yes   as default                           8, 16, 32      row of 85 floats: every fourth row starts 16-byte aligned
    no_dfl   2   2   0 no    as odd                               8, 16, 32      4 regression channels, d = z
    k8       2   5   7 yes   3x3, 1x1                             8, 16          K = 8
    k33      2   5  32 yes   3x3, 1x1                             8, 16          the greatest K = 33
    extreme  2   4  16 yes   as odd                               8, 16, 32      extreme finite logits (see _extreme)

HOST_ONLY (held to the host mirror, not in the fixture): single-level maps 1 x (T - 1), 1 x T, 1 x (T + 1) and 2 x T with T the
kernel's tile, at nc = 3 and nc = 80, and an L = 8 head of 1 x 1 maps.
"""
import numpy as np

F32 = np.float32
TILE = 64       # _lib.DETHEAD_TILE (tests/test_detector_head_cpu.py holds the two equal)

_DEFAULT = ((8, 8), (4, 4), (2, 2))
_ODD = ((5, 7), (3, 4), (2, 2))
#        name: (seed, B, nc, R, use_dfl, shapes, strides)
GOLDEN = {
    "default": (11, 2, 2, 16, True, _DEFAULT, (8, 16, 32)),
    "odd": (12, 3, 3, 16, True, _ODD, (8, 16, 32)),
    "four": (13, 3, 2, 16, True, ((8, 12), (4, 6), (2, 3), (1, 2)), (8, 16, 32, 64)),
    "single": (14, 1, 1, 16, True, _DEFAULT, (8, 16, 32)),
    "coco": (15, 2, 80, 16, True, _DEFAULT, (8, 16, 32)),
    "no_dfl": (16, 2, 2, 0, False, _ODD, (8, 16, 32)),
    "k8": (17, 2, 5, 7, True, ((3, 3), (1, 1)), (8, 16)),
    "k33": (18, 2, 5, 32, True, ((3, 3), (1, 1)), (8, 16)),
    "extreme": (19, 2, 4, 16, True, _ODD, (8, 16, 32)),
}
HOST_ONLY = {}
for _nc in (3, 80):
    for _h, _w in ((1, TILE - 1), (1, TILE), (1, TILE + 1), (2, TILE)):
        HOST_ONLY["tile_%dx%d_nc%d" % (_h, _w, _nc)] = (100 + _nc + _h * _w, 2, _nc, 16, True, ((_h, _w),), (8,))
HOST_ONLY["eight_levels"] = (99, 2, 3, 16, True, ((1, 1),) * 8, (2, 4, 8, 16, 32, 64, 128, 256))


def _extreme(rng, cls, reg, K):
    """Large finite logits, inside the contract.  Per (image, anchor, side), in turn: a one-hot row at +-1e4 (the softmax is
    exactly one-hot, d an exact integer); an all-equal row (d = R / 2); logits near +-88 (exp at the edge of float32's range);
    logits of +-3e38; two rows left as they are.  Class logits in turn: +-1e4 (p = 0 and 1 exactly), near +-17 and +-104 (where
    float32's sigmoid saturates and underflows), 0, and one left as it is."""
    turn = 0
    for c, r in zip(cls, reg):
        B, _, h, w = r.shape
        rows = r.reshape(B, 4, K, h * w)
        for b in range(B):
            for a in range(h * w):
                for s in range(4):
                    kind = turn % 6
                    turn += 1
                    if kind == 0:
                        rows[b, s, :, a] = -1e4
                        rows[b, s, rng.integers(K), a] = 1e4
                    elif kind == 1:
                        rows[b, s, :, a] = F32(rng.normal() * 50)
                    elif kind == 2:
                        rows[b, s, :, a] = (rng.choice([-1.0, 1.0], K) * (88.0 + rng.uniform(-1, 1, K))).astype(F32)
                    elif kind == 3:
                        rows[b, s, :, a] = (rng.choice([-1.0, 1.0], K) * 3e38).astype(F32)
        flat = c.reshape(-1)
        special = np.array([1e4, -1e4, 17.0, -17.0, 104.0, -104.0, 0.0, 16.6, -103.3, 3e38, -3e38], F32)
        for i in range(flat.size):
            if i % 12 < len(special):
                flat[i] = special[i % 12] + (F32(rng.uniform(-0.5, 0.5)) if 2 <= i % 12 <= 5 else F32(0))


def build(name):
    """The case as a dict: B, nc, R, use_dfl, K, shapes, strides, N, cls / reg (lists of float32 NCHW arrays), and the seeded
    weights Wc (B, N, nc), Wr (B, N, 4K) of the training branch's scalar."""
    seed, B, nc, R, use_dfl, shapes, strides = (GOLDEN.get(name) or HOST_ONLY[name])
    rng = np.random.default_rng(seed)
    K = R + 1 if use_dfl else 1
    cls = [(rng.normal(size=(B, nc, h, w)) * 3.0).astype(F32) for h, w in shapes]
    if use_dfl:
        reg = [(rng.normal(size=(B, 4 * K, h, w)) * 2.0).astype(F32) for h, w in shapes]
    else:
        reg = [rng.uniform(0.0, 6.0, size=(B, 4, h, w)).astype(F32) for h, w in shapes]
    if name == "extreme":
        _extreme(rng, cls, reg, K)
    N = sum(h * w for h, w in shapes)
    Wc = rng.normal(size=(B, N, nc)).astype(F32)
    Wr = rng.normal(size=(B, N, 4 * K)).astype(F32)
    return dict(name=name, B=B, nc=nc, R=R, use_dfl=use_dfl, K=K, shapes=tuple(shapes), strides=tuple(strides), N=N, cls=cls, reg=reg,
                Wc=Wc, Wr=Wr)


def anchors(shapes, strides):
    """Per anchor: ax, ay (float64, grid units) and the stride (float64)."""
    ax, ay, s = [], [], []
    for (h, w), st in zip(shapes, strides):
        a = np.arange(h * w)
        ax.append((a % w) + 0.5)
        ay.append((a // w) + 0.5)
        s.append(np.full(h * w, float(st)))
    return np.concatenate(ax), np.concatenate(ay), np.concatenate(s)
