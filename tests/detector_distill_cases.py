"""Seeded cases for the distillation tests (test_detector_distill_cpu.py, test_gpu_detector_distill.py) and for
tests/golden/make_golden_detector_distill.py.  A case is a dict of detector_loss_cases.base (p, z, anc, stride, labels, tb, ts,
fg, nc, R, use_dfl, weights) with the teacher's tp (B, A, nc) and tz (B, A, 4K) float32, the temperature T, epoch, max_epoch
and the distillation weights dw.  Channel-wise cases are dicts with s, t (lists of (N, C, H, W) float32) and tau.

bounds() / cw_bounds(): the DERIVED error bound between two evaluations of the stated rules that differ in the order of their
sums, in the last place of every exp / log and in the order of a few products.  u = 2^-53.  What both sides share exactly: the
widened inputs, x / T (one correctly rounded division) and m (a selection).

* a probability of a softmax over n values: x / T - m is one rounding, relative u of an argument of size at most a (a: the
  greatest |x / T - m| of the tensor), so exp's value moves by a u relatively, and by 1 u for its last place; Z adds n
  positive terms, n - 1 more; the quotient 1 more: e_p = (2 a + n + 2) u per side, relative.
* a KL term pt log pt - pt log ps: a logarithm of a value with relative error e_p is off by e_p ABSOLUTELY, plus its last
  place; times pt; both products carry pt's error and a rounding; the difference one more.  Per side
  2 e_p pt + (e_p + 3 u) (|pt log pt| + |pt log ps|).  The terms of a row CANCEL (the sum is 0 when teacher and student agree),
  so the row's bound stands on the sum of the absolute values of its products (rows_abs) and on spt = sum pt: per side
  2 e_p spt + (e_p + (n + 2) u) rows_abs, n - 1 of it for the additions.  Doubled for the two sides.
* d_loss_cls = T^2 * sum over B * A rows: the rows' bounds, the additions in any order (depth below 64 per side, 128 u on the
  sum of absolute values), T * T and the product (2 per side): 4 e_p * dcls_spt + (2 e_p + (2 n + 4 + 132) u) * dcls_abs.
* d_loss_dfl = (((T^2 * (sum / (4 n_fg))) * W) / norm: the same with n = K on the foreground rows (ddfl_spt, ddfl_abs carry the
  factors), plus W (rows of nc values, nc - 1 per side, and 128 u for the sum over the anchors), norm (286 u,
  detector_loss_cases) and five more operations per side: 4 e_K * ddfl_spt + (2 e_K + (2 K + 4 + 128 + 2 (nc - 1) + 128 + 286 +
  10) u) * ddfl_abs.
* the three terms of loss.py and their gradients: detector_loss_cases.bounds on loss_host's intermediates at this norm.
* the distillation part of a gradient, c * (ps * spt - pt): ps and pt e_p each, spt e_p + (n - 1) u, two products and the
  difference, c two or six operations (with W and norm for the DFL part): per side 2 e_p + (n + 4) u, doubled, on
  |c| (|ps spt| + |pt|) (gs_abs_kd, gz_abs_kd); the DFL part adds (2 (nc - 1) + 128 + 286 + 12) u.  The one addition of the two
  parts: 2 u on the sum of all absolute values.
* channel-wise, a row of n = H * W values: Z adds n positive terms in an order of depth D = ceil(n / 256) + 64 at most; with
  a = the greatest |ls| or |lt| (it bounds |log Z| and |x - m| too) a log-probability is off by d = (2 + D + 2 a) u absolutely
  per side.  pt = exp(lt): relative d + u.  A term pt (lt - ls): pt (2 d + u |lt - ls|) + |term| (d + 2 u); the additions D u.
  A level: 2 * (2 d * spt_l) + (2 (d + (3 + D) u) + 134 u) * abs_l, with spt_l and abs_l the scaled sums of spt and of
  pt (|lt| + |ls|) (cw_host's details).  A gradient element: 2 (2 d + (D + 6) u) on (tau / (N C)) (|exp(ls) spt| + pt).
A stored float32 gradient adds one float32 rounding, 2^-24 relative."""
import numpy as np

import detector_loss_cases as lcases

F32, F64 = np.float32, np.float64
U = lcases.U
DW = (1.0, 1.0)


def with_teacher(c, seed, T=20.0, epoch=3, max_epoch=10, dw=DW):
    """A teacher near the student: scores in (0.02, 0.98), logits the student's plus N(0, 0.5)."""
    rng = np.random.default_rng(seed)
    c["tp"] = rng.uniform(0.02, 0.98, c["p"].shape).astype(F32)
    c["tz"] = (c["z"] + rng.normal(0, 0.5, c["z"].shape)).astype(F32)
    c.update(T=float(T), epoch=epoch, max_epoch=max_epoch, dw=dw)
    return c


def plain():
    return with_teacher(lcases.base(111, S=160, B=1, nc=2, n_fg=40), 211)


def large():
    """Several tiles of the class launch per image, several images, nc = 80: not recorded (the fixture stays small)."""
    return with_teacher(lcases.base(112, S=160, B=3, nc=80, n_fg=40), 212)


def t_one():
    return with_teacher(lcases.base(113, S=64, B=3, nc=2, n_fg=9), 213, T=1.0)


def t_three():
    return with_teacher(lcases.base(114, S=64, B=1, nc=80, n_fg=12), 214, T=3.0)


def nc_one():
    return with_teacher(lcases.base(115, S=64, B=1, nc=1, n_fg=5), 215)


def teacher_is_student():
    c = with_teacher(lcases.base(116, S=64, B=1, nc=2, n_fg=6), 216)
    c["tp"], c["tz"] = c["p"].copy(), c["z"].copy()
    return c


def no_positives():
    return with_teacher(lcases.no_positives(), 217)


def one_positive():
    return with_teacher(lcases.base(118, S=64, B=1, nc=2, n_fg=1), 218)


def tss_below_one():
    return with_teacher(lcases.tss_below_one(), 219)


def tss_zero_with_fg():
    c = lcases.base(120, S=64, B=1, nc=2, n_fg=4)
    c["ts"][:] = 0.0
    return with_teacher(c, 220)


def w_not_tss():
    """Background rows with scores: W != tss (the assigner never writes such rows; the kernel must not assume it)."""
    c = lcases.base(121, S=64, B=1, nc=2, n_fg=6)
    bg = np.argwhere(~c["fg"])[:10]
    for i, (b, a) in enumerate(bg):
        c["ts"][b, a, i % 2] = 0.1 + 0.05 * i
    return with_teacher(c, 221)


def no_dfl():
    return with_teacher(lcases.base(122, S=160, B=3, nc=2, R=0, use_dfl=False, n_fg=30), 222)


def big_logits():
    """|z| and |tz| up to 80 at T = 20: arguments of exp down to -8."""
    c = lcases.big_logits()
    rng = np.random.default_rng(223)
    c = with_teacher(c, 223)
    tz = (c["z"] * F32(0.5) + rng.uniform(-40, 40, c["z"].shape).astype(F32)).astype(F32)
    np.clip(tz, -80, 80, out=tz)
    bb, aa = np.nonzero(c["fg"])
    tz.reshape(1, -1, 4, 17)[bb[0], aa[0], 0, 5] = 80.0
    tz.reshape(1, -1, 4, 17)[bb[0], aa[0], 1, 2] = -80.0
    c["tz"] = tz
    return c


def r8():
    return with_teacher(lcases.base(124, S=64, B=1, nc=2, R=8, n_fg=6), 224)


def f32_targets():
    return with_teacher(lcases.f32_targets(), 225)


def decay_start():
    return with_teacher(lcases.base(126, S=64, B=1, nc=2, n_fg=6), 226, epoch=0, max_epoch=10)


def decay_mid():
    return with_teacher(lcases.base(126, S=64, B=1, nc=2, n_fg=6), 226, epoch=5, max_epoch=10)


def decay_end():
    return with_teacher(lcases.base(126, S=64, B=1, nc=2, n_fg=6), 226, epoch=10, max_epoch=10)


CASES = {f.__name__: f for f in (plain, large, t_one, t_three, nc_one, teacher_is_student, no_positives, one_positive, tss_below_one,
                                 tss_zero_with_fg, w_not_tss, no_dfl, big_logits, r8, f32_targets, decay_start, decay_mid, decay_end)}
# recorded from the reference: not r8 (its view(-1, 17)), not the exact-zero cases (its float32 need not be exactly zero), not
# the large shape (the fixture's size)
GOLDEN = [n for n in CASES if n not in ("r8", "nc_one", "teacher_is_student", "large")]
KEYS = ("p", "z", "tp", "tz", "anc", "stride", "labels", "tb", "ts", "fg")


def k_of(c):
    """(k_class, k_dfl) of rule 8."""
    from event_representation_study_amd import detector_distill as dd
    dec = dd.decay(c["epoch"], c["max_epoch"])
    return dec * c["dw"][0], dec * c["dw"][1]


def host(c, details=None):
    from event_representation_study_amd import detector_distill as dd
    kc, kd = k_of(c)
    return dd.distill_host(c["p"], c["z"], c["tp"], c["tz"], c["anc"], c["stride"], c["labels"], c["tb"], c["ts"], c["fg"], c["T"], kc, kd,
                           c["R"], c["use_dfl"], dict(zip(("class", "iou", "dfl"), c["weights"])), details=details)


def total(c, losses):
    """Rule 8's loss from the eight entries, in Python floats."""
    kc, kd = k_of(c)
    wc, wi, wd = c["weights"]
    cls_all, dfl_all = losses[0] + losses[3] * kc, losses[2] + losses[4] * kd
    return float((cls_all * wc + losses[1] * wi) + dfl_all * wd), [float(losses[1] * wi), float(dfl_all * wd), float(cls_all * wc)]


def restated(c, dtype=None):
    import torch
    import detector_distill_ref as ref
    t = {k: torch.from_numpy(np.asarray(c[k])) for k in KEYS}
    return ref.distill_terms(t["p"], t["z"], t["tp"], t["tz"], t["anc"], t["stride"], t["labels"], t["tb"].double(), t["ts"].double(),
                             t["fg"], c["nc"], c["R"], c["use_dfl"], c["weights"], c["T"], c["epoch"], c["max_epoch"], c["dw"],
                             **({} if dtype is None else dict(dtype=dtype)))


def _spread(x, n, T):
    """The greatest |x / T - m| over rows of n values."""
    r = x.astype(F64).reshape(-1, n)
    return float((r.max(1) - r.min(1)).max() / T)


def bounds(c, losses, d):
    """The bounds of the module docstring from distill_host's ``losses`` and details ``d``: cls, iou, dfl, dcls, ddfl (absolute) and
    gs, gz (arrays, absolute, per gradient element in float64)."""
    nc, T = c["nc"], c["T"]
    K = c["R"] + 1 if c["use_dfl"] else 1
    base = lcases.bounds(c, losses, dict(d, gs_abs=d["gs_abs_base"], gz_abs=d["gz_abs_base"]))
    e_p = (2 * max(_spread(c["p"], nc, T), _spread(c["tp"], nc, T)) + nc + 2) * U
    out = dict(cls=base["cls"], iou=base["iou"], dfl=base["dfl"])
    out["dcls"] = 4 * e_p * d["dcls_spt"] + (2 * e_p + (2 * nc + 4 + 132) * U) * d["dcls_abs"]
    out["gs"] = base["gs"] + 2 * (2 * e_p + (nc + 4) * U) * d["gs_abs_kd"] + 2 * U * d["gs_abs"]
    if c["use_dfl"]:
        e_k = (2 * max(_spread(c["z"], K, T), _spread(c["tz"], K, T)) + K + 2) * U
        out["ddfl"] = 4 * e_k * d["ddfl_spt"] + (2 * e_k + (2 * K + 4 + 128 + 2 * (nc - 1) + 128 + 286 + 10) * U) * d["ddfl_abs"]
        out["gz"] = base["gz"] + (2 * (2 * e_k + (K + 4) * U) + (2 * (nc - 1) + 128 + 286 + 12) * U) * d["gz_abs_kd"] + 2 * U * d["gz_abs"]
    else:
        out["ddfl"], out["gz"] = 0.0, base["gz"]
    return out


# ------------------------------------------------------------------------------------------------------ channel-wise cases
def cw_case(seed, shapes, tau=1.0, N=2, C=3):
    """Maps of N(0, 1.5) for the student, the student's plus N(0, 0.7) for the teacher."""
    rng = np.random.default_rng(seed)
    s = [rng.normal(0, 1.5, (N, C, h, w)).astype(F32) for h, w in shapes]
    t = [(x + rng.normal(0, 0.7, x.shape)).astype(F32) for x in s]
    return dict(s=s, t=t, tau=float(tau))


CW_CASES = {
    "plain": lambda: cw_case(301, [(8, 8), (4, 4), (2, 2)]),
    "one_value": lambda: cw_case(302, [(1, 1), (1, 1), (1, 1)]),                       # exactly 0
    "wave": lambda: cw_case(303, [(8, 8), (5, 13), (7, 9)]),                           # 64, 65, 63 values
    "workgroup": lambda: cw_case(304, [(16, 16), (257, 1), (15, 17)]),                 # 256, 257, 255
    "staging": lambda: cw_case(305, [(64, 64), (1, 4097), (4095, 1)], N=1, C=2),       # 4096 staged, 4097 re-read, 4095
    "longest": lambda: cw_case(306, [(80, 80), (40, 40), (20, 20)], N=1, C=2),         # the reference's largest
    "four_levels": lambda: cw_case(307, [(8, 8), (4, 4), (2, 2), (3, 3)]),             # the fourth is ignored
    "tau_two": lambda: cw_case(308, [(8, 8), (4, 4), (2, 2)], tau=2.0),
    "uneven": lambda: dict(s=[np.random.default_rng(309).normal(0, 2, sh).astype(F32) for sh in ((2, 3, 6, 5), (1, 7, 3, 3), (3, 1, 2, 9))],
                           t=[np.random.default_rng(310).normal(0, 2, sh).astype(F32) for sh in ((2, 3, 6, 5), (1, 7, 3, 3), (3, 1, 2, 9))],
                           tau=1.0),                                                    # (N, C) differ per level
}
CW_GOLDEN = [n for n in CW_CASES if n != "one_value"]


def cw_host(c, details=None):
    from event_representation_study_amd import detector_distill as dd
    return dd.cw_host(c["s"], c["t"], c["tau"], details=details)


def cw_restated(c, dtype=None):
    import torch
    import detector_distill_ref as ref
    return ref.cw_terms([torch.from_numpy(x) for x in c["s"]], [torch.from_numpy(x) for x in c["t"]], c["tau"],
                        **({} if dtype is None else dict(dtype=dtype)))


def cw_bounds(c, d):
    """Per level: (loss bound, gradient bound array); then the bound of the sum."""
    levels, grads = [], []
    for l in range(3):
        n = int(np.prod(c["s"][l].shape[2:]))
        D = (n + 255) // 256 + 64
        dl = (2 + D + 2 * d["amax"][l]) * U
        levels.append(2 * (2 * dl * d["spt"][l]) + (2 * (dl + (3 + D) * U) + 134 * U) * d["abs"][l])
        grads.append(2 * (2 * dl + (D + 6) * U) * d["g_abs"][l])
    return levels, grads, sum(levels) + 2 * U * sum(d["abs"])
