"""A numpy restatement of ev-licious' ``Events.render`` for integer coordinates, written from the per-pixel formulas the device
kernels implement (include/evrep.h, evrep_render_state / evrep_render_compose) -- not from the reference's statements: every
type is a function of a small per-pixel state, ``cast=False`` a 2 x 2 stencil over it.  tests/test_evl_render_cpu.py holds it to
the images the reference itself drew (tests/golden/evl_render.npz); the GPU tests then use it on inputs that have no golden.

"positive" is p > 0; every other p counts as negative (``Events`` forces p into {-1, +1})."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OVERLAP, RB_NO_OVERLAP, BW_NO_OVERLAP, TIME_SURFACE, EVENT_FRAME = 1, 2, 3, 4, 5
TYPE_NAMES = {1: "RED_BLUE_OVERLAP", 2: "RED_BLUE_NO_OVERLAP", 3: "BLACK_WHITE_NO_OVERLAP", 4: "TIME_SURFACE", 5: "EVENT_FRAME"}
TAU = 3e4


def load_golden():
    z = np.load(os.path.join(HERE, "golden", "evl_render.npz"))
    return z, json.loads(str(z["manifest"]))


def golden_case(z, name):
    H, W = (int(v) for v in z[name + ".size"])
    return tuple(z["%s.%s" % (name, k)] for k in "xytp") + (H, W)


def golden_image(z, manifest, name, rtype, cast, with_canvas):
    return z[manifest["cases"][name]["%s.%s.cast%d.canvas%d" % (name, TYPE_NAMES[int(rtype)], bool(cast), bool(with_canvas))]]


def in_frame(x, y, H, W):
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    return (x >= 0) & (y >= 0) & (x < W) & (y < H)


def pixel_state(x, y, p, H, W):
    """-> (any_pos, any_neg, last_pos, net): (H, W) bool, bool, bool, int64.  last_pos: the polarity of the pixel's last event in
    array order.  Rows outside the frame are left out."""
    x, y, p = np.asarray(x, np.int64), np.asarray(y, np.int64), np.asarray(p, np.int64)
    keep = in_frame(x, y, H, W)
    x, y, pos = x[keep], y[keep], p[keep] > 0
    any_pos, any_neg = np.zeros((H, W), bool), np.zeros((H, W), bool)
    any_pos[y[pos], x[pos]] = True
    any_neg[y[~pos], x[~pos]] = True
    last = np.zeros((H, W), np.int64)
    np.maximum.at(last, (y, x), np.arange(1, len(x) + 1))
    last_pos = np.zeros((H, W), bool)
    hit = last > 0
    last_pos[hit] = pos[last[hit] - 1]
    net = np.zeros((H, W), np.int64)
    np.add.at(net, (y, x), np.where(pos, 1, -1))
    return any_pos, any_neg, last_pos, net


def _shift(a, dy, dx):
    """out[y, x] = a[y - dy, x - dx], False outside."""
    out = np.zeros_like(a)
    H, W = a.shape
    out[dy:, dx:] = a[:H - dy, :W - dx]
    return out


def jitter_state(any_pos, any_neg, last_pos):
    """The state cast=False draws from: every event also at (x, y+1), (x+1, y), (x+1, y+1), the four copies concatenated.  The
    union of the flags; the last event of an output pixel is the last one of the first source, latest copy first -- (y-1, x-1),
    (y, x-1), (y-1, x), (y, x) -- that has any event."""
    jp, jn = np.zeros_like(any_pos), np.zeros_like(any_neg)
    done, jl = np.zeros_like(any_pos), np.zeros_like(last_pos)
    for dy, dx in ((1, 1), (0, 1), (1, 0), (0, 0)):
        sp, sn, sl = _shift(any_pos, dy, dx), _shift(any_neg, dy, dx), _shift(last_pos, dy, dx)
        jp |= sp
        jn |= sn
        take = ~done & (sp | sn)
        jl[take] = sl[take]
        done |= sp | sn
    return jp, jn, jl


def surface(x, y, t, H, W, tau=TAU):
    """The time surface's image before the colour map, float32 (H, W): v = exp(-(t[-1] - t) / tau) in float64, one float32
    rounding per event in array order, img = fl32(float64(img) + v) (what np.add.at does)."""
    x, y, t = np.asarray(x, np.int64), np.asarray(y, np.int64), np.asarray(t, np.int64)
    if len(x) == 0:
        return np.zeros((H, W), np.float32)
    v = np.exp(-(t[-1] - t) / float(tau))
    keep = in_frame(x, y, H, W)
    x, y, v = x[keep], y[keep], v[keep]
    img = np.zeros((H, W), np.float32)
    for xi, yi, vi in zip(x, y, v):
        img[yi, xi] = np.float32(np.float64(img[yi, xi]) + vi)
    return img


def lut_index(img):
    """min(int(img * 256), 255), the product in float32; everything from 1 up (inf included) is the last row."""
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.asarray(img, np.float32) * np.float32(256)
        return np.where(f >= 255, 255, np.where(f >= 0, f, 0).astype(np.int64)).astype(np.int64)


def render(x, y, t, p, H, W, rtype, cast=True, canvas=None, lut=None, surface_image=None):
    """The image ``Events(x, y, t, p, width=W, height=H).render(canvas, rtype, cast)`` returns."""
    rtype = int(rtype)
    if rtype == TIME_SURFACE:
        if len(x) <= 2:
            return np.zeros((H, W), np.uint8)
        img = surface(x, y, t, H, W) if surface_image is None else surface_image
        return np.asarray(lut, np.float64)[lut_index(img)]
    any_pos, any_neg, last_pos, net = pixel_state(x, y, p, H, W)
    if rtype == EVENT_FRAME:
        gray = np.clip(20 * net + 128, 0, 255).astype(np.uint8)
        return np.stack([gray, gray, gray], axis=-1)
    if not cast:
        any_pos, any_neg, last_pos = jitter_state(any_pos, any_neg, last_pos)
    out = np.full((H, W, 3), 255, np.uint8) if canvas is None else np.array(canvas, dtype=np.uint8, copy=True)
    hit = any_pos | any_neg
    if rtype == OVERLAP:
        colour = np.stack([np.where(any_neg, 255, 0), np.zeros((H, W), np.int64), np.where(any_pos, 255, 0)], axis=-1)
    elif rtype == RB_NO_OVERLAP:
        colour = np.stack([np.where(last_pos, 0, 255), np.zeros((H, W), np.int64), np.where(last_pos, 255, 0)], axis=-1)
    else:
        colour = np.repeat(np.where(last_pos, 255, 0)[..., None], 3, axis=-1)
    out[hit] = colour[hit].astype(np.uint8)
    return out


def surface_bound(x, y, t, H, W, tau=TAU):
    """Per pixel with k events and (float64) sum s of its terms: (k + 1) * 2^-23 * s -- every term's exp held to 1e-12 relative
    (far below 2^-24), each of the k stores rounds once (relative 2^-24 of a partial sum <= s), on either side of the comparison."""
    x, y, t = np.asarray(x, np.int64), np.asarray(y, np.int64), np.asarray(t, np.int64)
    k, s = np.zeros((H, W), np.float64), np.zeros((H, W), np.float64)
    if len(x):
        keep = in_frame(x, y, H, W)
        v = np.exp(-(t[-1] - t) / float(tau))[keep]
        np.add.at(k, (y[keep], x[keep]), 1.0)
        np.add.at(s, (y[keep], x[keep]), v)
    return (k + 1.0) * 2.0 ** -23 * s, k


def check_surface(got, want, x, y, t, H, W, what=""):
    """`got` against the recorded / restated float32 surface `want`: within surface_bound everywhere, the LUT index off by at
    most 1, and at most 1 % of the touched pixels different at all.  Returns (pixels that differ, touched pixels)."""
    bound, k = surface_bound(x, y, t, H, W)
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin]), what
    err = np.abs(got[fin].astype(np.float64) - want[fin].astype(np.float64))
    assert np.all(err <= bound[fin]), (what, float(err.max()))
    assert np.all(got[k == 0] == 0), what
    step = np.abs(lut_index(got) - lut_index(want))
    assert step.max() <= 1, (what, int(step.max()))
    differ, touched = int(np.count_nonzero(got != want)), int(np.count_nonzero(k))
    assert differ <= 0.01 * touched, (what, differ, touched)
    return differ, touched
