"""Seeded cases for the loss tests (test_detector_loss_cpu.py, test_gpu_detector_loss.py) and for
tests/golden/make_golden_detector_loss.py, built by hand: the four target arrays are WRITTEN, not assigned, so that edges can be
placed.  A case is a dict: p (B, A, nc) float32, z (B, A, 4K) float32, anc (A, 2), stride (A,) float32, labels int64 (B, A),
tb (B, A, 4) pixels, ts (B, A, nc), fg bool (B, A), nc, R, use_dfl, weights.

No case contains an exact tie of a min / max pair or a clamp argument of exactly 0 (check_decided asserts it on loss_host's
intermediates): there torch's autograd and the kernel agree by rule (halves), but a rounding apart on either side would move a
whole gradient term, which no tolerance covers.

bounds(): the DERIVED error bound between two evaluations of the stated rules that differ in the order of their sums, in the
last place of every exp / log, and (the torch restatement) in the order of a few products.  With u = 2^-53:

* class term: an element's bce * wt takes 10 roundings (1 - p, two logs, 1 - q, two products, their sum, two products for wt, the
  product); its terms have one sign, so its relative error is at most 10 u per side, 20 u.  A sum of n same-signed terms in any
  order has relative error (depth) u, depth the longest chain of additions: below 64 on either side for the n here (numpy and
  torch add pairwise in blocks, the kernel per lane, by butterfly, per wave, per slice): 128 u.  norm: a row of nc values left to
  right or pairwise, nc - 1 <= 79 u per side, and the 128 u of the sum over the rows: 286 u.  The division: 2 u.  C_CLS = 436.
* a gradient element of pred_scores: the same chain (bce, wt), four more roundings for (p - q) / max((1 - p) * p, 1e-12), the
  factor wc / norm (288 u), two products and a sum per side, on the sum of the absolute values of its two terms:
  C_GS = 20 + 8 + 288 + 6 = 322.
* box terms: a side's expectation d adds K positive products: K exps of 1 ulp, K subtractions, K - 1 + K - 1 additions, K
  divisions and products, relative 5 K + 2 <= 6 K u per side, 12 K u.  A coordinate ax -/+ d therefore carries an ABSOLUTE error
  of 12 K u * extent (extent: the greatest coordinate or distance of the anchor), and a length (a difference of coordinates) a
  relative error of 2 * 12 K u * extent / length + u.  With cond = extent / (the smallest length that enters a product or a
  quotient: w1, h1, w2, h2, cw, ch and the positive ones of iw, ih), every length is within e = (24 K * cond + 1) u.  Every term of
  giou and of its backward pass is a product or quotient of at most 8 lengths and 12 roundings: relative (8 e + 12 u) per side;
  doubled, on the sum of the absolute values of the terms: E_a = 2 * (8 e + 12 u).
  loss_iou: sum_a E_a * iou_scale_a + (128 + 286 + 2) u * loss_iou.
* DFL: ce = (m + log Z) - z_k: Z relative (K + 1) u, log 1 ulp, two roundings: (K + 4) u on |m| + |log Z| + |z_k| + 1 per side;
  the side and the mean add 6: C_DFL = 2 * (K + 10) on dfl_scale, + 416 u * loss_dfl as above.
* a gradient element of pred_distri: pr_k and d (12 K u), the GIoU part E_a, the factor 1 / norm (288 u), 8 roundings:
  (E_a + (12 K + 296) u) on the sum of the absolute values of its terms (gz_abs).
A stored float32 gradient adds one float32 rounding, 2^-24 relative."""
import numpy as np

from event_representation_study_amd.detector_assign import anchor_points

F32, F64 = np.float32, np.float64
U = 2.0 ** -53
WEIGHTS = (1.0, 2.5, 0.5)


def base(seed, S=64, B=1, nc=2, R=16, use_dfl=True, n_fg=6):
    """Scores in (0.02, 0.98); logits peaked about a distance of 0.5 .. 6 strides; n_fg foreground anchors per image with a target
    box of 0.6 .. 7 strides to each side of the anchor's centre and one score in (0.05, 1) at the label."""
    rng = np.random.default_rng(seed)
    anc, stride = anchor_points(S)
    stride = stride.reshape(-1)
    A, K = len(anc), (R + 1 if use_dfl else 1)
    p = rng.uniform(0.02, 0.98, (B, A, nc)).astype(F32)
    dist = rng.uniform(0.5, 6.0, (B, A, 4))
    if use_dfl:
        k = np.arange(K)[None, None, None, :]
        z = (rng.normal(0, 1, (B, A, 4, K)) + 4.0 * np.exp(-0.5 * (k - dist[..., None]) ** 2)).astype(F32).reshape(B, A, 4 * K)
    else:
        z = dist.astype(F32)
    labels = rng.integers(0, nc, (B, A)).astype(np.int64)
    fg = np.zeros((B, A), bool)
    tb = np.zeros((B, A, 4), F64)
    ts = np.zeros((B, A, nc), F64)
    for b in range(B):
        fg[b, rng.choice(A, min(n_fg, A), replace=False)] = True
    ext = rng.uniform(0.6, 7.0, (B, A, 4)) * stride[None, :, None]
    tb[..., 0], tb[..., 1] = anc[None, :, 0] - ext[..., 0], anc[None, :, 1] - ext[..., 1]
    tb[..., 2], tb[..., 3] = anc[None, :, 0] + ext[..., 2], anc[None, :, 1] + ext[..., 3]
    bb, aa = np.nonzero(fg)
    ts[bb, aa, labels[bb, aa]] = rng.uniform(0.05, 1.0, len(bb))
    return dict(p=p, z=z, anc=anc, stride=stride.astype(F32), labels=labels, tb=tb, ts=ts, fg=fg, nc=nc, R=R, use_dfl=use_dfl,
                weights=WEIGHTS)


def _first_fg(c, n):
    bb, aa = np.nonzero(c["fg"])
    return list(zip(bb[:n].tolist(), aa[:n].tolist()))


def plain():
    return base(11, S=160, B=1, nc=2, n_fg=40)


def plain_nc80():
    return base(24, S=64, B=1, nc=80, n_fg=12)


def large():
    """The shape with several slices per image and several images: not recorded (the fixture stays small)."""
    return base(25, S=160, B=3, nc=80, n_fg=40)


def large_no_dfl_f32():
    c = base(26, S=160, B=3, nc=1, R=0, use_dfl=False, n_fg=30)
    c["tb"], c["ts"] = c["tb"].astype(F32), c["ts"].astype(F32)
    return c


def plain_small():
    return base(12, S=64, B=1, nc=1, n_fg=5)


def plain_nc2():
    return base(13, S=64, B=3, nc=2, n_fg=9)


def no_dfl():
    return base(14, S=160, B=3, nc=2, R=0, use_dfl=False, n_fg=30)


def no_positives():
    c = base(15, S=64, B=1, nc=2)
    c["fg"][:] = False
    c["ts"][:] = 0.0
    return c


def tss_below_one():
    c = base(16, S=64, B=1, nc=2, n_fg=2)
    for (b, a), v in zip(_first_fg(c, 2), (0.4, 0.3)):
        c["ts"][b, a, c["labels"][b, a]] = v
    return c


def tss_just_above_one():
    c = tss_below_one()
    (b, a), _ = _first_fg(c, 2)
    c["ts"][b, a, c["labels"][b, a]] = 0.7 + 2.0 ** -20
    return c


def saturated():
    """p exactly 0 and exactly 1 on non-label and on label elements whose q lies inside (0, 1): the -100 clamp of either log and
    the 1e-12 denominator; gradients of 1e11 .. 1e12."""
    c = base(17, S=64, B=1, nc=2, n_fg=8)
    fgs = _first_fg(c, 4)
    for i, (b, a) in enumerate(fgs):
        l = c["labels"][b, a]
        c["p"][b, a, l] = (0.0, 1.0, 0.0, 1.0)[i]
        c["p"][b, a, 1 - l] = (1.0, 0.0, 0.5, 0.5)[i]
        c["ts"][b, a, 1 - l] = (0.25, 0.5, 0.0, 0.0)[i]
    bg = np.argwhere(~c["fg"])[:6]
    for i, (b, a) in enumerate(bg):
        c["p"][b, a, 0] = (0.0, 1.0)[i % 2]
        c["p"][b, a, 1] = (1.0, 0.0)[i % 2]
        c["ts"][b, a, i % 2] = (0.0, 0.5, 0.75)[i % 3]
    return c


def _set_box(c, b, a, l, t, r, bt):
    """A target of l, t, r, bt strides to the sides of the anchor's centre (negative: beyond it)."""
    s, (x, y) = F64(c["stride"][a]), c["anc"][a].astype(F64)
    c["tb"][b, a] = [x - l * s, y - t * s, x + r * s, y + bt * s]


def disjoint():
    """Targets that the predicted box misses (inter = 0: the gradient flows through the convex term only) in x, in y and in both;
    a target that contains the predicted box and one that lies inside it."""
    c = base(18, S=64, B=1, nc=2, n_fg=10)
    f = _first_fg(c, 5)
    _set_box(c, *f[0], -9.0, 1.0, 12.0, 1.0)
    _set_box(c, *f[1], 1.0, -8.5, 1.0, 11.0)
    _set_box(c, *f[2], 13.0, 12.5, -9.5, -8.0)
    _set_box(c, *f[3], 14.0, 14.5, 15.0, 13.5)
    _set_box(c, *f[4], 0.3, 0.25, 0.35, 0.3)
    return c


def clipped():
    """Target distances below 0, above R - 0.01 and exactly integral (wr = 0)."""
    c = base(19, S=64, B=1, nc=2, n_fg=8)
    f = _first_fg(c, 4)
    _set_box(c, *f[0], -2.0, 3.0, 20.0, 16.0)
    _set_box(c, *f[1], 3.0, 5.0, 1.0, 15.0)
    _set_box(c, *f[2], 15.99, 15.995, 0.0, 2.5)
    _set_box(c, *f[3], 17.0, -1.5, 4.0, 25.0)
    return c


def big_logits():
    """|z| up to 80: exp(80) * 17 overflows nothing in float64 but a softmax that does not subtract its maximum is far off in
    float32; the gradients' pr_k underflow towards 0."""
    c = base(20, S=64, B=1, nc=2, n_fg=6)
    rng = np.random.default_rng(21)
    z = c["z"].reshape(1, -1, 4, 17)
    z *= F32(4.0)
    for b, a in _first_fg(c, 6):
        z[b, a, :, :] = rng.uniform(-80, 80, (4, 17)).astype(F32)
        z[b, a, 0, 3] = 80.0
        z[b, a, 1, 16] = -80.0
    np.clip(z, -80, 80, out=z)
    return c


def bad_label():
    c = base(22, S=64, B=3, nc=2, n_fg=5)
    f = _first_fg(c, 15)
    (b0, a0), (b1, a1) = f[0], f[-1]                                   # images 0 and 2
    c["labels"][b0, a0] = 2
    c["labels"][b1, a1] = -1
    c["ts"][b0, a0] = [0.3, 0.0]
    c["ts"][b1, a1] = [0.0, 0.6]
    return c


def f32_targets():
    c = base(23, S=64, B=1, nc=80, n_fg=10)
    c["tb"], c["ts"] = c["tb"].astype(F32), c["ts"].astype(F32)
    return c


CASES = {f.__name__: f for f in (plain, plain_small, plain_nc2, plain_nc80, large, large_no_dfl_f32, no_dfl, no_positives, tss_below_one, tss_just_above_one, saturated,
                                 disjoint, clipped, big_logits, bad_label, f32_targets)}
# recorded from the reference: all but bad_label (its one_hot raises there) and the two large shapes (the fixture's size)
GOLDEN = [n for n in CASES if n not in ("bad_label", "large", "large_no_dfl_f32")]


def host(c, details=None):
    from event_representation_study_amd import detector_loss as dl
    return dl.loss_host(c["p"], c["z"], c["anc"], c["stride"], c["labels"], c["tb"], c["ts"], c["fg"], c["R"], c["use_dfl"],
                        dict(zip(("class", "iou", "dfl"), c["weights"])), details=details)


def restated(c, dtype=None):
    """The torch restatement (detector_loss_ref.loss_terms) on the case; float32 targets are widened first, as the rules say."""
    import torch
    import detector_loss_ref as ref
    t = {k: torch.from_numpy(np.asarray(c[k])) for k in ("p", "z", "anc", "stride", "labels", "tb", "ts", "fg")}
    return ref.loss_terms(t["p"], t["z"], t["anc"], t["stride"], t["labels"], t["tb"].double(), t["ts"].double(), t["fg"], c["nc"],
                          c["R"], c["use_dfl"], c["weights"], **({} if dtype is None else dict(dtype=dtype)))


def check_decided(name, c, d):
    """No tie of a min / max pair, no clamp argument of exactly 0, on loss_host's intermediates ``d``."""
    for k, pr in enumerate(d["pairs"]):
        assert not (pr[:, 0] == pr[:, 1]).any(), (name, "a tie of min / max pair %d" % k)
    for k, v in enumerate(d["clamps"]):
        assert not (v == 0).any(), (name, "clamp argument %d is exactly 0" % k)


def bounds(c, losses, d):
    """The bounds of the module docstring from loss_host's ``losses`` and details ``d``: a dict with cls, iou, dfl (absolute, on
    the normalised terms), gs and gz (arrays, absolute, per gradient element in float64)."""
    K = c["R"] + 1 if c["use_dfl"] else 1
    e = (24.0 * K * d["cond"] + 1.0) * U
    E = 2.0 * (8.0 * e + 12.0 * U)                                      # (B, A)
    out = dict(cls=436 * U * d["cls_abs"],
               iou=float((E * d["iou_scale"]).sum()) + 416 * U * d["iou_abs"],
               dfl=2 * (K + 10) * U * float(d["dfl_scale"].sum()) + 416 * U * d["dfl_abs"],
               gs=322 * U * d["gs_abs"],
               gz=(E + (12 * K + 296) * U)[..., None] * d["gz_abs"])
    return out
