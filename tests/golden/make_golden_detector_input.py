#!/usr/bin/env python3
"""Golden vectors for the detector's input batch (tests/golden/detector_input.npz).

Run where the reference lies (the fixture travels, the reference does not):

    python tests/golden/make_golden_detector_input.py

The reference's own ``yolov6.data.data_augment`` and ``yolov6.data.gen1_2yolo.Gen1H5`` are IMPORTED (never copied) and
``Gen1H5.__getitem__`` runs on a bare instance whose three loader methods (convert_idx_to_rel_idx, _load_bbox, _load_events)
return synthetic windows and boxes; the representation is the reference's EventStack through its get_item_transform.  What
the reference's own statements decide is thereby pinned: the order of the stages, the label arithmetic, the draws from
``random`` and ``shapes``.

Packages the reference imports but this image lacks are replaced by in-process stand-ins, as make_golden.py does: empty
``h5py``, ``hdf5plugin``, ``matplotlib``, ``wandb``, ``tonic``; a ``torch_geometric.data`` with an attribute bag ``Data`` and
an empty ``Dataset``; and a ``cv2`` with ``resize``, ``split``, ``merge``, ``copyMakeBorder``, ``warpAffine`` and
``getRotationMatrix2D`` written here in numpy from OpenCV's published algorithms (INTER_AREA / INTER_LINEAR tables; the
10-bit fixed-point walk of warpAffine; float64 sums, the four warp taps in the image's dtype), independently of the kernel
and of the package's own host mirrors.  What sits behind that ``cv2`` boundary is therefore NOT pinned against OpenCV:
PARITY UNPINNED (cv2 absent).

Per case the file holds: the ``random.seed``, the events, the boxes _load_bbox returned, the representation, M (identity
without augment), the image, ``labels_out`` and ``shapes``.
"""
import math
import os
import random
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

REF = mg.REF
OUT = os.path.join(HERE, "detector_input.npz")
HYP = {"degrees": 0.373, "translate": 0.245, "scale": 0.898, "shear": 0.602, "flipud": 0.5, "fliplr": 0.5}


# --------------------------------------------------------------------------- the cv2 stand-in
def _area_matrix(src, dst):
    scale = src / dst
    Wm = np.zeros((dst, src))
    for d in range(dst):
        f1 = d * scale
        f2 = f1 + scale
        cell = min(scale, src - f1)
        s1 = math.ceil(f1)
        s2 = min(math.floor(f2), src - 1)
        s1 = min(s1, s2)
        if s1 - f1 > 1e-3:
            Wm[d, s1 - 1] += (s1 - f1) / cell
        for k in range(s1, s2):
            Wm[d, k] += 1.0 / cell
        if f2 - s2 > 1e-3:
            Wm[d, s2] += min(min(f2 - s2, 1.0), cell) / cell
    return Wm


def _linear_matrix(src, dst):
    scale = src / dst
    Wm = np.zeros((dst, src))
    for d in range(dst):
        f = (d + 0.5) * scale - 0.5
        k = math.floor(f)
        f -= k
        if k < 0:
            k, f = 0, 0.0
        if k >= src - 1:
            k, f = src - 1, 0.0
        Wm[d, k] += 1.0 - f
        if f:
            Wm[d, k + 1] += f
    return Wm


def _taps_apply(img, Wy, Wx):
    """x taps first, then y taps, each a float64 sum over the non-zero run in index order; one cast to the image's dtype."""
    H, W = img.shape
    src = img.astype(np.float64)
    tmp = np.zeros((H, Wx.shape[0]))
    for ox in range(Wx.shape[0]):
        nz = np.nonzero(Wx[ox])[0]
        for k in range(nz[0], nz[-1] + 1):
            tmp[:, ox] += src[:, k] * Wx[ox, k]
    out = np.zeros((Wy.shape[0], Wx.shape[0]))
    for oy in range(Wy.shape[0]):
        nz = np.nonzero(Wy[oy])[0]
        for k in range(nz[0], nz[-1] + 1):
            out[oy] += tmp[k] * Wy[oy, k]
    return out.astype(img.dtype)


def _make_cv2():
    cv2 = types.ModuleType("cv2")
    cv2.INTER_LINEAR, cv2.INTER_AREA, cv2.BORDER_CONSTANT = 1, 3, 0

    def resize(im, dsize, interpolation=1):
        w, h = dsize
        make = _area_matrix if interpolation == cv2.INTER_AREA else _linear_matrix
        if im.ndim == 2:
            return _taps_apply(im, make(im.shape[0], h), make(im.shape[1], w))
        if im.shape[2] > 4:
            raise ValueError("cv2.resize: more than 4 channels")      # why the reference splits the channels
        return np.stack([_taps_apply(im[..., c], make(im.shape[0], h), make(im.shape[1], w)) for c in range(im.shape[2])], -1)

    def split(im):
        return [np.ascontiguousarray(im[..., c]) for c in range(im.shape[2])]

    def merge(chs):
        return np.stack(list(chs), -1)

    def copyMakeBorder(im, top, bottom, left, right, borderType, value=0):
        if im.ndim == 3 and im.shape[2] > 4:
            raise ValueError("cv2.copyMakeBorder: more than 4 channels")   # the reference's except branch goes per channel
        v = value[0] if isinstance(value, (tuple, list)) else value
        pads = ((top, bottom), (left, right)) + (((0, 0),) if im.ndim == 3 else ())
        return np.pad(im, pads, mode="constant", constant_values=im.dtype.type(v))

    def getRotationMatrix2D(angle, center, scale):
        assert tuple(center) == (0, 0)
        alpha, beta = scale * math.cos(angle * math.pi / 180), scale * math.sin(angle * math.pi / 180)
        return np.array([[alpha, beta, 0.0], [-beta, alpha, 0.0]])

    def warpAffine(img, M, dsize, borderValue=0):
        width, height = dsize
        h, w = img.shape[:2]
        M = np.asarray(M, dtype=np.float64)
        D = M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]
        D = 1.0 / D if D != 0 else 0.0
        m00, m11 = M[1, 1] * D, M[0, 0] * D
        m01, m10 = M[0, 1] * (-D), M[1, 0] * (-D)
        m02 = -m00 * M[0, 2] - m01 * M[1, 2]
        m12 = -m10 * M[0, 2] - m11 * M[1, 2]
        T = img.dtype.type
        border = borderValue[0] if isinstance(borderValue, (tuple, list)) else borderValue   # 114 on every channel here
        out = np.empty((height, width) + img.shape[2:], dtype=img.dtype)

        def rint(v):
            return int(np.rint(v))

        def tap(yy, xx):
            if 0 <= yy < h and 0 <= xx < w:
                return img[yy, xx]
            return np.full(img.shape[2:], border, dtype=img.dtype)

        for y in range(height):
            X0 = rint((m01 * y + m02) * 1024) + 16
            Y0 = rint((m11 * y + m12) * 1024) + 16
            for x in range(width):
                X = (X0 + rint(m00 * x * 1024)) >> 5
                Y = (Y0 + rint(m10 * x * 1024)) >> 5
                sx, sy = min(max(X >> 5, -32768), 32767), min(max(Y >> 5, -32768), 32767)
                ax, ay = T(X & 31) / T(32), T(Y & 31) / T(32)
                one = T(1)
                out[y, x] = ((tap(sy, sx) * ((one - ay) * (one - ax)) + tap(sy, sx + 1) * ((one - ay) * ax))
                             + tap(sy + 1, sx) * (ay * (one - ax))) + tap(sy + 1, sx + 1) * (ay * ax)
        return out

    for f in (resize, split, merge, copyMakeBorder, getRotationMatrix2D, warpAffine):
        setattr(cv2, f.__name__, f)
    return cv2


def _install():
    mg._install_standins()
    for name in ("h5py", "hdf5plugin", "wandb", "matplotlib", "matplotlib.pyplot"):
        if name not in sys.modules:
            try:
                __import__(name)
            except ImportError:
                sys.modules[name] = types.ModuleType(name)
    tg = types.ModuleType("torch_geometric")
    tg.data = types.ModuleType("torch_geometric.data")

    class Data:
        def __init__(self, **kw):
            self.__dict__.update(kw)

        def clone(self):
            return Data(**{k: (v.clone() if torch.is_tensor(v) else v) for k, v in self.__dict__.items()})

    class Dataset:
        def __init__(self, *a, **k):
            pass

    tg.data.Data, tg.data.Dataset = Data, Dataset
    sys.modules["torch_geometric"], sys.modules["torch_geometric.data"] = tg, tg.data
    sys.modules["cv2"] = _make_cv2()
    os.chdir(REF)
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(REF, "representations"))
    sys.path.insert(0, os.path.join(REF, "ev-YOLOv6"))
    from yolov6.data import data_augment, gen1_2yolo
    from representations.event_stack import EventStack
    return data_augment, gen1_2yolo, EventStack


# --------------------------------------------------------------------------- synthetic windows
def _window(rng, n, height, width):
    x = rng.integers(0, width, n)
    y = rng.integers(0, height, n)
    t = np.sort(rng.integers(0, 100000, n)) + 1000
    p = rng.integers(0, 2, n) * 2 - 1
    return np.stack([x, y, t], -1).astype(np.int64), p.astype(np.int64)


def _boxes(rng, n):
    """[class, x, y, w, h] with (x, y) the top-left corner, normalised: what _load_bbox stacks before _adjust_bbox."""
    xy = rng.uniform(0.05, 0.6, (n, 2))
    wh = rng.uniform(0.15, 0.35, (n, 2))
    b = np.concatenate([rng.integers(0, 2, (n, 1)).astype(np.float64), xy, wh], 1).astype(np.float32)
    return b


def run_case(mods, seed, augment, return_int, height, width, img_size, n_events=600, n_boxes=3):
    data_augment, gen1_2yolo, EventStack = mods
    Gen1H5 = gen1_2yolo.Gen1H5
    rng = np.random.default_rng(1000 + seed)
    xyt, pol = _window(rng, n_events, height, width)
    raw_boxes = _boxes(rng, n_boxes)
    ds = Gen1H5.__new__(Gen1H5)
    hyp = dict(HYP)
    if return_int is not None:
        hyp["letterbox_return_int"] = bool(return_int)
    ds.augment, ds.hyp, ds.rect, ds.img_size = augment, hyp, False, img_size
    ds.height, ds.width, ds.num_events, ds.time_window = height, width, n_events, 100000
    ds.transform, ds.vis_paths_to_indexes = EventStack, {}
    handle = {"bbox": None, "events": None}
    ds.convert_idx_to_rel_idx = lambda item: (0, handle, "synthetic")
    seen = {}

    def load_bbox(h, idx):
        bbox = Gen1H5._adjust_bbox(ds, raw_boxes, 0, 1)          # the reference's own clipping and centring
        bbox[:, 1:3] += 0.5 * bbox[:, 3:5]
        seen["boxes"] = bbox.copy()
        return bbox, 0

    ds._load_bbox = load_bbox
    ds._load_events = lambda h, event_idx: (xyt.copy(), pol.copy())
    # listeners on the reference's own functions: what they returned, not what they do
    real_gtm, real_git = data_augment.get_transform_matrix, gen1_2yolo.get_item_transform

    def gtm(*a, **k):
        M, s = real_gtm(*a, **k)
        seen["M"], seen["s"] = M.copy(), s
        return M, s

    def git(*a, **k):
        rep = real_git(*a, **k)
        seen["rep"] = np.array(rep, copy=True)
        return rep

    data_augment.get_transform_matrix, gen1_2yolo.get_item_transform = gtm, git
    try:
        random.seed(seed)
        img, labels_out, _, shapes = ds[0]
    finally:
        data_augment.get_transform_matrix, gen1_2yolo.get_item_transform = real_gtm, real_git
    (h0, w0), ((rh, rw), pad) = shapes
    return {"seed": np.int64(seed), "augment": np.bool_(augment), "return_int": np.int64(-1 if return_int is None else int(return_int)),
            "img_size": np.int64(img_size), "events": np.concatenate([xyt, pol[:, None]], 1).astype(np.int32),
            "boxes": seen["boxes"], "rep": seen["rep"], "M": seen.get("M", np.eye(3)), "s": np.float64(seen.get("s", 1.0)),
            "image": img.numpy(), "labels_out": labels_out.numpy(),
            "shapes": np.array([h0, w0, rh, rw, pad[0], pad[1]], dtype=np.float64),
            "flips": np.array(_flips_of(seed, hyp) if augment else [0, 0], dtype=np.int64)}


def _flips_of(seed, hyp):
    random.seed(seed)
    for _ in range(6):
        random.random()           # random.uniform(a, b) is a + (b - a) * random(): one draw each
    return [int(random.random() < hyp["flipud"]), int(random.random() < hyp["fliplr"])]


def main():
    mods = _install()
    want, seeds = {(0, 0), (0, 1), (1, 0), (1, 1)}, {}
    seed = 0
    while want:
        f = tuple(_flips_of(seed, HYP))
        if f in want:
            want.discard(f)
            seeds[f] = seed
        seed += 1
    cases = []
    geo = [(20, 30, 32), (30, 20, 33), (20, 30, 32), (30, 20, 33)]      # (height, width, S): pad rows / pad columns
    for k, (f, sd) in enumerate(sorted(seeds.items())):
        h, w, S = geo[k]
        cases.append(run_case(mods, sd, True, k % 2, h, w, S))
    cases.append(run_case(mods, 3, True, None, 48, 48, 48))              # r == 1, hyp without letterbox_return_int
    cases.append(run_case(mods, 1, False, 0, 20, 30, 32))                # validation: INTER_LINEAR up-size
    cases.append(run_case(mods, 2, False, 1, 70, 96, 48))                # validation: INTER_AREA
    cases.append(run_case(mods, 4, False, None, 48, 48, 48))             # validation: r == 1
    flat = {"n_cases": np.int64(len(cases)), "hyp": np.array([HYP[k] for k in ("degrees", "translate", "scale", "shear", "flipud", "fliplr")])}
    for i, c in enumerate(cases):
        for k, v in c.items():
            flat["c%d_%s" % (i, k)] = v
        print("case %d seed %d augment %d S %d rep %s %s image %s labels %s flips %s" % (
            i, c["seed"], c["augment"], c["img_size"], c["rep"].shape, c["rep"].dtype, c["image"].shape, c["labels_out"].shape, c["flips"]))
    np.savez_compressed(OUT, **flat)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
