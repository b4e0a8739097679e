"""The last mile of the detector route: a batch of representations on the GPU -> the tensor, targets and shapes the detector
is trained on, as ``Gen1H5.__getitem__`` does after ``get_item_transform``, plus ``collate_fn`` and ``Trainer.prepro_data``
(ev-YOLOv6/yolov6/data/gen1_2yolo.py:210-228,230-265,320-398,427-447; the same statements in gen4/gen4_2yolo_raw.py:368-445;
data_augment.py:31-85,95-184; yolov6/core/engine.py:629-635): keep-ratio resize, ``letterbox(114)``, ``random_affine``,
``general_augment`` (up-down / left-right flips), HWC -> CHW with ``[::-1]``, ``.float() / 255``.

The images are ONE launch of ``evrep_detector_input`` (csrc/evrep_detin.hip): the (B, H, W, C) float64/float32 representation is
read through the caches and the (B, C, S, S) float32 tensor is written once; no intermediate image exists in memory.  The boxes
are a few numbers per sample and stay on the host, in numpy, statement for statement.

OpenCV is absent here.  ``cv2.resize`` is restated in gwd_pipeline; ``cv2.warpAffine`` (INTER_LINEAR, BORDER_CONSTANT) and
``cv2.getRotationMatrix2D`` are RESTATED here from OpenCV's published algorithm -- PARITY UNPINNED against cv2 itself.  The warp
is OpenCV's fixed-point walk of the inverse map (10 fractional bits, coordinates rounded to 1/32 pixel, the integer part
stored as int16), see ``warp_tables``; ``borderValue`` is a per-channel table because what cv2's four-entry Scalar does for a
fifth channel is not known here.

Frames of DIFFERENT sizes -- TORE's per-window bounding boxes, ``EventBatch.tore(frame_mode=0)`` -- go through
``DetectorFrontEnd.prepare_frames``: every sample through its own geometry, the resize tap tables made on the device
(``evrep_resize_tap_tables``), then ONE launch of ``evrep_detector_input_frames`` (csrc/evrep_detin_frames.hip); a sample whose
letterbox needs a resize of its own takes both resizes inside that launch.  ``targets_frames`` is its host side (targets and
shapes from the B frame sizes), usable without a device.  ``prepare`` itself keeps refusing a list.

Out of scope (NotImplementedError): ``rect`` / ``batch_shapes``.
"""
import collections
import ctypes
import math
import random

import numpy as np
import torch

from . import _lib
from ._lib import ptr, stream_ptr, want
from .gwd_pipeline import letterbox, resize_batch, resize_taps  # noqa: F401  (letterbox: re-exported under the reference's name)

AB_BITS = 10                      # OpenCV's fixed point of the inverse map
_AB_SCALE = 1 << AB_BITS
_ROUND_DELTA = 1 << (AB_BITS - 5 - 1)   # 16: rounds the shift that leaves 5 fractional bits
_I32 = (-(1 << 31), (1 << 31) - 1)

SampleParams = collections.namedtuple("SampleParams", "M s flipud fliplr")


# ------------------------------------------------------------------------------------------------ host mirrors
def rotation_matrix_2d(angle, scale):
    """cv2.getRotationMatrix2D(angle, (0, 0), scale) in closed form: [[alpha, beta, 0], [-beta, alpha, 0]]."""
    alpha = scale * math.cos(angle * math.pi / 180)
    beta = scale * math.sin(angle * math.pi / 180)
    return np.array([[alpha, beta, 0.0], [-beta, alpha, 0.0]], dtype=np.float64)


def get_transform_matrix(img_shape, new_shape, degrees, scale, shear, translate):
    """data_augment.py:153-184: M = T @ S @ R @ C and the scale draw; six ``random.uniform`` draws in the reference's order
    (angle, scale, x shear, y shear, x translation, y translation)."""
    new_height, new_width = new_shape
    centre = np.eye(3)
    centre[0, 2] = -img_shape[1] / 2
    centre[1, 2] = -img_shape[0] / 2
    rot = np.eye(3)
    a = random.uniform(-degrees, degrees)
    s = random.uniform(1 - scale, 1 + scale)
    rot[:2] = rotation_matrix_2d(a, s)
    sh = np.eye(3)
    sh[0, 1] = math.tan(random.uniform(-shear, shear) * math.pi / 180)
    sh[1, 0] = math.tan(random.uniform(-shear, shear) * math.pi / 180)
    tr = np.eye(3)
    tr[0, 2] = random.uniform(0.5 - translate, 0.5 + translate) * new_width
    tr[1, 2] = random.uniform(0.5 - translate, 0.5 + translate) * new_height
    return tr @ sh @ rot @ centre, s


def box_candidates(box1, box2, wh_thr=2, ar_thr=20, area_thr=0.1, eps=1e-16):
    """data_augment.py:95-107: which warped boxes (box2, (4, n)) are kept, given the boxes before the warp (box1)."""
    w1, h1 = box1[2] - box1[0], box1[3] - box1[1]
    w2, h2 = box2[2] - box2[0], box2[3] - box2[1]
    ar = np.maximum(w2 / (h2 + eps), h2 / (w2 + eps))
    return (w2 > wh_thr) & (h2 > wh_thr) & (w2 * h2 / (w1 * h1 + eps) > area_thr) & (ar < ar_thr)


def inverse_affine(M):
    """The six float64 coefficients of the inverse map, as cv2.warpAffine inverts M[:2] (a singular M inverts to D = 0)."""
    M = np.asarray(M, dtype=np.float64)
    D = M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]
    D = 1.0 / D if D != 0 else 0.0
    m00, m11 = M[1, 1] * D, M[0, 0] * D
    m01, m10 = M[0, 1] * (-D), M[1, 0] * (-D)
    m02 = -m00 * M[0, 2] - m01 * M[1, 2]
    m12 = -m10 * M[0, 2] - m11 * M[1, 2]
    return m00, m01, m02, m10, m11, m12


def warp_tables(M, width, height=None):
    """(adelta[width], bdelta[width], X0[height], Y0[height]) int64: OpenCV's fixed-point inverse map of ``M`` for a
    ``width x height`` output.  adelta[x] = rint(m00 x 1024), bdelta[x] = rint(m10 x 1024), X0[y] = rint((m01 y + m02) 1024) + 16,
    Y0[y] = rint((m11 y + m12) 1024) + 16, rint rounding half to even.  An entry or a sum X0 + adelta / Y0 + bdelta outside
    int32 -- where OpenCV's own int arithmetic overflows -- is a ValueError."""
    height = width if height is None else height
    x = np.arange(width, dtype=np.float64)
    y = np.arange(height, dtype=np.float64)
    with np.errstate(all="ignore"):
        m00, m01, m02, m10, m11, m12 = inverse_affine(M)
        real = (m00 * x * _AB_SCALE, m10 * x * _AB_SCALE, (m01 * y + m02) * _AB_SCALE, (m11 * y + m12) * _AB_SCALE)
    tabs = []
    for k, r in enumerate(real):
        r = np.rint(r)
        if not np.isfinite(r).all() or (np.abs(r) >= 2.0 ** 62).any():
            raise ValueError("warp_tables: the inverse map of M leaves int32 (fixed point, %d bits)" % AB_BITS)
        tabs.append(r.astype(np.int64) + (_ROUND_DELTA if k >= 2 else 0))
    ad, bd, X0, Y0 = tabs
    for lo, hi in ((ad.min(), ad.max()), (bd.min(), bd.max()), (X0.min(), X0.max()), (Y0.min(), Y0.max()),
                   (X0.min() + ad.min(), X0.max() + ad.max()), (Y0.min() + bd.min(), Y0.max() + bd.max())):
        if lo < _I32[0] or hi > _I32[1]:
            raise ValueError("warp_tables: the inverse map of M leaves int32 (fixed point, %d bits)" % AB_BITS)
    return ad, bd, X0, Y0


def warp_affine(img, M, dsize, borderValue=114.0):
    """cv2.warpAffine(img, M, dsize=(width, height), borderValue=...) with its defaults, restated in numpy for an (h, w[, C])
    float image; the arithmetic of the four taps is done in the image's dtype.  ``borderValue``: a scalar or one per channel."""
    img = np.asarray(img)
    squeeze = img.ndim == 2
    src = img[..., None] if squeeze else img
    h, w, C = src.shape
    width, height = int(dsize[0]), int(dsize[1])
    T = src.dtype if src.dtype in (np.float32, np.float64) else np.dtype(np.float64)
    src = src.astype(T, copy=False)
    ad, bd, X0, Y0 = warp_tables(np.asarray(M, dtype=np.float64), width, height)
    X = (X0[:, None] + ad[None, :]) >> 5
    Y = (Y0[:, None] + bd[None, :]) >> 5
    sx, sy = np.clip(X >> 5, -32768, 32767), np.clip(Y >> 5, -32768, 32767)
    ax, ay = ((X & 31).astype(T) / T.type(32))[..., None], ((Y & 31).astype(T) / T.type(32))[..., None]
    one = T.type(1)
    pad = np.broadcast_to(np.asarray(borderValue, dtype=T), (C,))

    def tap(yy, xx):
        inside = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        v = src[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)]
        return np.where(inside[..., None], v, pad)

    out = ((tap(sy, sx) * ((one - ay) * (one - ax)) + tap(sy, sx + 1) * ((one - ay) * ax)) + tap(sy + 1, sx) * (ay * (one - ax))) \
        + tap(sy + 1, sx + 1) * (ay * ax)
    out = out.astype(img.dtype, copy=False)
    return out[..., 0] if squeeze else out


def _affine_labels(labels, M, s, width, height):
    """random_affine's label branch (data_augment.py:125-148): the four corners of every box through M, the enclosing box,
    clipped; boxes that shrank too much are dropped."""
    n = len(labels)
    if not n:
        return labels
    corners = np.ones((n * 4, 3))
    corners[:, :2] = labels[:, [1, 2, 3, 4, 1, 4, 3, 2]].reshape(n * 4, 2)
    corners = corners @ M.T
    corners = corners[:, :2].reshape(n, 8)
    xs, ys = corners[:, [0, 2, 4, 6]], corners[:, [1, 3, 5, 7]]
    new = np.concatenate((xs.min(1), ys.min(1), xs.max(1), ys.max(1))).reshape(4, n).T
    new[:, [0, 2]] = new[:, [0, 2]].clip(0, width)
    new[:, [1, 3]] = new[:, [1, 3]].clip(0, height)
    keep = box_candidates(box1=labels[:, 1:5].T * s, box2=new.T, area_thr=0.1)
    labels = labels[keep]
    labels[:, 1:5] = new[keep]
    return labels


def random_affine(img, labels=(), degrees=10, translate=0.1, scale=0.1, shear=10, new_shape=(640, 640)):
    """data_augment.py:110-150 on the host: the draws of get_transform_matrix, the warp (border 114) unless M is the identity,
    and the label branch.  Returns (img, labels)."""
    height, width = new_shape
    M, s = get_transform_matrix(img.shape[:2], (height, width), degrees, scale, shear, translate)
    if (M != np.eye(3)).any():
        img = warp_affine(img, M[:2], dsize=(width, height), borderValue=114.0)
    if len(labels):
        labels = _affine_labels(labels, M, s, width, height)
    return img, labels


def general_augment(img, labels, hyp):
    """Gen1H5.general_augment (gen1_2yolo.py:210-228): up-down, then left-right flip, one ``random.random()`` draw each; the
    labels (normalised xywh) are changed in place."""
    nl = len(labels)
    if random.random() < hyp["flipud"]:
        img = np.flipud(img)
        if nl:
            labels[:, 2] = 1 - labels[:, 2]
    if random.random() < hyp["fliplr"]:
        img = np.fliplr(img)
        if nl:
            labels[:, 1] = 1 - labels[:, 1]
    return img, labels


# ------------------------------------------------------------------------------------------------ the device path
_IDENTITY_TAPS = {}


def identity_taps(n, device):
    """The tap tables that copy: one tap of weight 1 per output sample."""
    key = (int(n), str(device))
    if key not in _IDENTITY_TAPS:
        _IDENTITY_TAPS[key] = (torch.arange(int(n), dtype=torch.int32, device=device),
                               torch.ones(int(n), dtype=torch.int32, device=device),
                               torch.ones((int(n), 1), dtype=torch.float64, device=device), 1)
    return _IDENTITY_TAPS[key]


def _pad_taps(wt, T_have, T):
    return wt if T_have == T else torch.nn.functional.pad(wt, (0, T - T_have)).contiguous()


_PAD_TABLES = {}


def _pad_table(pad, C, device):
    """The (C,) float64 device table of a scalar or per-channel pad; kept, so that a call uploads nothing for it."""
    padv = np.broadcast_to(np.asarray(pad, dtype=np.float64), (C,)).copy()
    key = (padv.tobytes(), str(device))
    if key not in _PAD_TABLES:
        _PAD_TABLES[key] = torch.from_numpy(padv).to(device)
    return _PAD_TABLES[key]


def device_tables(flags, warp, B, S, device):
    """(B,) flags and (B, 4, S) warp tables as the int32 device tensors the launch reads; device tensors pass through."""
    if torch.is_tensor(flags) and torch.is_tensor(warp):
        flags, warp = flags.to(device).contiguous(), warp.to(device).contiguous()
        return want(flags, "detector_input: flags", torch.int32, numel=B), want(warp, "detector_input: warp", torch.int32, numel=B * 4 * S)
    flags_d = torch.from_numpy(np.ascontiguousarray(np.asarray(flags, dtype=np.uint32).reshape(B)).view(np.int32)).to(device)
    warp_d = torch.from_numpy(np.ascontiguousarray(np.asarray(warp, dtype=np.int32).reshape(B, 4, S))).to(device)
    return flags_d, warp_d


def detector_input(rep, img_size, row_taps, col_taps, nh, nw, top, left, pad=114.0, flags=None, warp=None, scale=1.0 / 255,
                   out=None):
    """One launch of evrep_detector_input.  rep: (B, H, W, C) float64/float32 CUDA tensor; row_taps / col_taps: (start, count,
    weights, T) device tables for the ``nh`` rows and ``nw`` columns of the resized rectangle; flags: (B,) uint32 values
    (_lib.DETIN_*) with warp: (B, 4, S) int32 tables (numpy, or int32 device tensors that are used as they are), or both None.  Returns the (B, C, S, S) float32 tensor."""
    api = _lib.api()
    if not rep.is_cuda:
        raise _lib.EvrepError("detector_input needs a CUDA tensor; there is no CPU fallback")
    if rep.dtype not in (torch.float64, torch.float32):
        raise TypeError("detector_input: float64 or float32 representation, not %s" % rep.dtype)
    rep = rep.contiguous()
    B, H, W, C = (int(v) for v in rep.shape)
    S = int(img_size)
    dev = rep.device
    ys, yc, yw, Ty = row_taps
    xs, xc, xw, Tx = col_taps
    T = max(Ty, Tx)
    yw, xw = _pad_taps(yw, Ty, T), _pad_taps(xw, Tx, T)
    pad_d = _pad_table(pad, C, dev)
    flags_d = warp_d = None
    if flags is not None:
        flags_d, warp_d = device_tables(flags, warp, B, S, dev)
    if out is None:
        out = torch.empty((B, C, S, S), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        api.evrep_detector_input(ptr(rep), _lib.F64 if rep.dtype == torch.float64 else _lib.F32, B, H, W, C, int(nh), int(nw), T, ptr(ys),
                                 ptr(yc), ptr(yw), ptr(xs), ptr(xc), ptr(xw), S, int(top), int(left), ptr(pad_d), ptr(flags_d),
                                 ptr(warp_d), 1.0 if scale is None else float(scale), ptr(out), stream_ptr())
    return out


Geometry = collections.namedtuple("Geometry", "r interp rh rw ratio nh nw dw dh top left fused")


class DetectorFrontEnd:
    """``Gen1H5.__getitem__`` after ``get_item_transform`` + ``collate_fn`` + ``prepro_data`` for a batch on the device.

    ``hyp``: the reference's dictionary (degrees, translate, scale, shear, flipud, fliplr, optionally letterbox_return_int).
    ``augment=False`` is the validation route: no warp, no flip, no scale-up, INTER_AREA when shrinking."""

    def __init__(self, img_size=640, hyp=None, augment=False, rect=False):
        if rect:
            raise NotImplementedError("rect / batch_shapes: the letterboxed shape is the img_size square")
        if augment and not hyp:
            raise ValueError("augment=True needs hyp (degrees, translate, scale, shear, flipud, fliplr)")
        self.img_size = int(img_size)
        self.hyp = hyp
        self.augment = bool(augment)

    def draw(self, B):
        """The per-sample parameters of a batch: for sample 0, 1, ... in turn the six ``random.uniform`` draws of
        get_transform_matrix, then the two ``random.random()`` draws of general_augment, call for call."""
        S, out = self.img_size, []
        for _ in range(int(B)):
            if not self.augment:
                out.append(SampleParams(np.eye(3), 1.0, False, False))
                continue
            M, s = get_transform_matrix((S, S), (S, S), self.hyp["degrees"], self.hyp["scale"], self.hyp["shear"], self.hyp["translate"])
            ud = random.random() < self.hyp["flipud"]
            lr = random.random() < self.hyp["fliplr"]
            out.append(SampleParams(M, s, ud, lr))
        return out

    def geometry(self, h0, w0):
        """The sizes resize_image and letterbox(auto=False, scaleup=augment) arrive at for an (h0, w0) source."""
        S = self.img_size
        r = S / max(h0, w0)
        rh, rw = (int(h0 * r), int(w0 * r)) if r != 1 else (int(h0), int(w0))
        interp = "area" if (r < 1 and not self.augment) else "linear"
        ratio = min(S / rh, S / rw)
        if not self.augment:
            ratio = min(ratio, 1.0)
        nw, nh = int(round(rw * ratio)), int(round(rh * ratio))
        dw, dh = (S - nw) / 2, (S - nh) / 2
        top, left = int(round(dh - 0.1)), int(round(dw - 0.1))
        return Geometry(r, interp, rh, rw, ratio, nh, nw, dw, dh, top, left, (rw, rh) == (nw, nh))

    def letterboxed(self, rep):
        """Stages R + L materialised by the existing functions: (B, H, W, C) -> (B, S, S, C) of the same dtype (the staged
        route; what ``prepare`` hands the kernel when letterbox needs a resize of its own)."""
        B, h0, w0, C = (int(v) for v in rep.shape)
        g, S = self.geometry(h0, w0), self.img_size
        im = rep if g.r == 1 else resize_batch(rep, g.rh, g.rw, g.interp, out_dtype=rep.dtype)
        if not g.fused:
            im = resize_batch(im, g.nh, g.nw, "linear", out_dtype=rep.dtype)
        return im, g

    def _pad_square(self, im, g, pad):
        B, _, _, C = (int(v) for v in im.shape)
        S = self.img_size
        padv = _pad_table(pad, C, im.device).to(im.dtype)
        sq = padv.expand(B, S, S, C).contiguous()
        sq[:, g.top:g.top + g.nh, g.left:g.left + g.nw] = im
        return sq

    def prepare(self, rep, labels=None, params=None, pad=114.0, scale=1.0 / 255, staged=False):
        """rep: (B, H, W, C) float64/float32 CUDA tensor.  Returns (images, targets, shapes): the (B, C, S, S) float32 tensor
        of one launch; the (n, 6) float32 targets of collate_fn (column 0 the sample index) from ``labels``, a list of B
        (n_b, 5) arrays [class, xc, yc, w, h], normalised (their dtype is kept: float32, as the reference loads them,
        reproduces its roundings); per sample ``((h0, w0), ((h * ratio / h0, w * ratio / w0), pad))``.  ``params``: what
        ``draw(B)`` returned (default: drawn now).  ``staged=True`` materialises resize + letterbox first (the same kernel then
        copies); it is what happens anyway when letterbox needs a resize of its own."""
        if isinstance(rep, (list, tuple)):
            raise NotImplementedError("per-window frames (TORE's bounding boxes) are not one batch: call prepare per window")
        if rep.dim() != 4:
            raise ValueError("prepare: a (B, H, W, C) representation")
        B, h0, w0, C = (int(v) for v in rep.shape)
        S = self.img_size
        if params is None:
            params = self.draw(B)
        if len(params) != B or (labels is not None and len(labels) != B):
            raise ValueError("prepare: one parameter set and one label array per sample")
        g = self.geometry(h0, w0)
        # every table is made (and may raise) before anything is launched
        flags = warp = None
        if any(p.flipud or p.fliplr or (np.asarray(p.M) != np.eye(3)).any() for p in params):
            flags = np.zeros(B, dtype=np.uint32)
            warp = np.zeros((B, 4, S), dtype=np.int32)
            for b, p in enumerate(params):
                if (np.asarray(p.M) != np.eye(3)).any():
                    flags[b] |= _lib.DETIN_WARP
                    warp[b] = np.stack(warp_tables(p.M, S))
                flags[b] |= (_lib.DETIN_FLIPUD if p.flipud else 0) | (_lib.DETIN_FLIPLR if p.fliplr else 0)
        if staged or not g.fused:
            im, _ = self.letterboxed(rep)
            sq = self._pad_square(im, g, pad)
            taps = identity_taps(S, rep.device)
            images = detector_input(sq, S, taps, taps, S, S, 0, 0, pad, flags, warp, scale)
        else:
            if g.r == 1:
                rows, cols = identity_taps(h0, rep.device), identity_taps(w0, rep.device)
            else:
                rows, cols = resize_taps(h0, g.rh, g.interp, rep.device), resize_taps(w0, g.rw, g.interp, rep.device)
            images = detector_input(rep, S, rows, cols, g.nh, g.nw, g.top, g.left, pad, flags, warp, scale)
        return_int = bool(self.hyp and self.hyp.get("letterbox_return_int"))
        lb_pad = (g.left, g.top) if return_int else (g.dw, g.dh)
        shapes = [((h0, w0), ((g.rh * g.ratio / h0, g.rw * g.ratio / w0), lb_pad)) for _ in range(B)]
        return images, self.targets(labels, params, g, lb_pad), shapes

    def targets(self, labels, params, g, lb_pad):
        """The box statements of __getitem__:348-394, random_affine's label branch and the flips, per sample, then collate_fn."""
        rows = [self._sample_targets(b, lab, params[b], g, lb_pad) for b, lab in enumerate(labels or [])]
        return torch.cat(rows, 0) if rows else torch.zeros((0, 6))

    def _sample_targets(self, b, lab, p, g, lb_pad):
        """Sample b's rows of ``targets``: its boxes through its own geometry ``g`` and letterbox pad."""
        S = self.img_size
        lab = np.array(lab, copy=True)
        lab = lab.reshape(-1, 5) if lab.size else np.zeros((0, 5), dtype=lab.dtype if lab.dtype.kind == "f" else np.float32)
        if lab.size:
            w, h = g.rw * g.ratio, g.rh * g.ratio
            boxes = np.copy(lab[:, 1:])
            boxes[:, 0] = w * (lab[:, 1] - lab[:, 3] / 2) + lb_pad[0]
            boxes[:, 1] = h * (lab[:, 2] - lab[:, 4] / 2) + lb_pad[1]
            boxes[:, 2] = w * (lab[:, 1] + lab[:, 3] / 2) + lb_pad[0]
            boxes[:, 3] = h * (lab[:, 2] + lab[:, 4] / 2) + lb_pad[1]
            lab[:, 1:] = boxes
        if self.augment:
            lab = _affine_labels(lab, np.asarray(p.M, dtype=np.float64), p.s, S, S)
        if len(lab):
            lab[:, [1, 3]] = lab[:, [1, 3]].clip(0, S - 1e-3)
            lab[:, [2, 4]] = lab[:, [2, 4]].clip(0, S - 1e-3)
            boxes = np.copy(lab[:, 1:])
            boxes[:, 0] = ((lab[:, 1] + lab[:, 3]) / 2) / S
            boxes[:, 1] = ((lab[:, 2] + lab[:, 4]) / 2) / S
            boxes[:, 2] = (lab[:, 3] - lab[:, 1]) / S
            boxes[:, 3] = (lab[:, 4] - lab[:, 2]) / S
            lab[:, 1:] = boxes
            if p.flipud:
                lab[:, 2] = 1 - lab[:, 2]
            if p.fliplr:
                lab[:, 1] = 1 - lab[:, 1]
        t = torch.zeros((len(lab), 6))
        if len(lab):
            t[:, 1:] = torch.from_numpy(np.ascontiguousarray(lab))
        t[:, 0] = b
        return t

    # -------------------------------------------------------------------------------------------- frames of different sizes
    def frame_geometries(self, sizes):
        """``geometry`` of every (h0, w0) of a ragged batch; an empty frame (an empty window has no bounding box) and a frame so
        thin that the keep-ratio resize leaves no row or column are ValueErrors naming the sample (the reference fails inside
        cv2.resize or divides by zero there)."""
        geos = []
        for b, (h0, w0) in enumerate(sizes):
            h0, w0 = int(h0), int(w0)
            if h0 < 1 or w0 < 1:
                raise ValueError("prepare_frames: sample %d is an empty %d x %d frame (an empty window)" % (b, h0, w0))
            r = self.img_size / max(h0, w0)
            if r != 1 and (int(h0 * r) < 1 or int(w0 * r) < 1):
                raise ValueError("prepare_frames: sample %d (%d x %d) resizes to %d x %d" % (b, h0, w0, int(h0 * r), int(w0 * r)))
            geos.append(self.geometry(h0, w0))
        return geos

    def _lb_pad(self, g):
        return (g.left, g.top) if bool(self.hyp and self.hyp.get("letterbox_return_int")) else (g.dw, g.dh)

    def targets_frames(self, sizes, labels=None, params=None):
        """The host side of ``prepare_frames``, no device needed: ``sizes`` are the B (h0, w0) pairs.  Returns (targets, shapes)
        as ``prepare`` does, sample b through its OWN geometry: the reference scales the sensor-normalised boxes by the resized
        bounding-box frame (gen1_2yolo.py:348-363 after gen1_transforms.py:61-66), and so does this."""
        geos = self.frame_geometries(sizes)
        B = len(geos)
        if labels is not None and len(labels) != B:
            raise ValueError("prepare_frames: %d label arrays for %d frames" % (len(labels), B))
        if params is None:
            params = self.draw(B)
        if len(params) != B:
            raise ValueError("prepare_frames: %d parameter sets for %d frames" % (len(params), B))
        rows = [self._sample_targets(b, lab, params[b], geos[b], self._lb_pad(geos[b])) for b, lab in enumerate(labels or [])]
        shapes = [((int(h0), int(w0)), ((g.rh * g.ratio / int(h0), g.rw * g.ratio / int(w0)), self._lb_pad(g)))
                  for (h0, w0), g in zip(sizes, geos)]
        return (torch.cat(rows, 0) if rows else torch.zeros((0, 6))), shapes

    def frame_tables(self, sizes, geos, params):
        """The host side of one ragged launch: (table, host, n_axes, max_dst, n_rows, n_wt).  ``table``: the B evrep_detin_frame
        descriptors (``src`` left 0); ``host``: the int32 buffer that is uploaded, the axis descriptors of
        evrep_resize_tap_tables -- one axis per distinct (src, dst, interpolation, T) of the batch -- followed, when a sample
        warps, by the (B, 4, S) warp tables.  T is known in closed form: 2 for INTER_LINEAR, ``area_taps_bound`` for INTER_AREA, 1
        for a copy; no (dst, src) matrix is made."""
        B, S = len(sizes), self.img_size
        axes, rows_total, wt_total = {}, 0, 0

        def axis(src, dst, code, T):
            nonlocal rows_total, wt_total
            key = (src, dst, code, T)
            if key not in axes:
                axes[key] = (rows_total, wt_total)
                rows_total, wt_total = rows_total + dst, wt_total + dst * T
            return axes[key]

        table = np.zeros(B, dtype=_FRAME_DTYPE)
        warp = None
        for b, (g, p) in enumerate(zip(geos, params)):
            h0, w0 = sizes[b]
            d = table[b]
            if g.r == 1:
                code, T1 = _lib.TAPS_IDENTITY, 1
            elif g.interp == "area":
                code, T1 = _lib.TAPS_AREA, max(area_taps_bound(h0, g.rh), area_taps_bound(w0, g.rw))
            else:
                code, T1 = _lib.TAPS_LINEAR, 2
            (d["row1"], d["wrow1"]), (d["col1"], d["wcol1"]) = axis(h0, g.rh, code, T1), axis(w0, g.rw, code, T1)
            d["H"], d["W"], d["rh"], d["rw"], d["T1"] = h0, w0, g.rh, g.rw, T1
            d["nh"], d["nw"], d["top"], d["left"] = g.nh, g.nw, g.top, g.left
            if not g.fused:
                d["T2"] = 2
                (d["row2"], d["wrow2"]), (d["col2"], d["wcol2"]) = axis(g.rh, g.nh, _lib.TAPS_LINEAR, 2), axis(g.rw, g.nw, _lib.TAPS_LINEAR, 2)
            flag = (_lib.DETIN_FLIPUD if p.flipud else 0) | (_lib.DETIN_FLIPLR if p.fliplr else 0)
            if (np.asarray(p.M) != np.eye(3)).any():
                flag |= _lib.DETIN_WARP
                if warp is None:
                    warp = np.zeros((B, 4, S), dtype=np.int32)
                warp[b] = np.stack(warp_tables(p.M, S))
            d["flags"] = flag
        n_axes = len(axes)
        host = np.empty(n_axes * _lib.TAPS_AXIS_FIELDS + (warp.size if warp is not None else 0), dtype=np.int32)
        host[:n_axes * _lib.TAPS_AXIS_FIELDS] = np.array([k + v for k, v in axes.items()], dtype=np.int32).reshape(-1)
        if warp is not None:
            host[n_axes * _lib.TAPS_AXIS_FIELDS:] = warp.reshape(-1)
        return table, host, n_axes, max(k[1] for k in axes), rows_total, wt_total

    def prepare_frames(self, frames, labels=None, params=None, pad=114.0, scale=1.0 / 255, out=None):
        """``prepare`` for B frames of DIFFERENT sizes -- ``EventBatch.tore(frame_mode=0)``'s per-window bounding boxes -- in one
        launch.  frames: a list / tuple of (H_b, W_b, C) CUDA tensors of one dtype (float64 / float32), C and device; views into
        one allocation are read where they lie, a non-contiguous frame is made contiguous.  Returns (images, targets, shapes)
        as ``prepare`` does, every sample through its own ``geometry``.  From the host go one upload (axis descriptors and the
        warp tables, one buffer) and the descriptor table that evrep_detector_input_frames checks and copies itself; then one
        launch makes the tap tables (evrep_resize_tap_tables) and one the images.  A sample whose letterbox needs a resize of
        its own takes both resizes inside that launch; no intermediate image is made.  Everything is checked, and every table
        is made, before anything is launched.  ``out``: a contiguous (B, C, S, S) float32 tensor to write into."""
        if not isinstance(frames, (list, tuple)) or not len(frames):
            raise ValueError("prepare_frames: a non-empty list of (H, W, C) frames")
        B, S = len(frames), self.img_size
        if (params is not None and len(params) != B) or (labels is not None and len(labels) != B):
            raise ValueError("prepare_frames: one parameter set and one label array per frame (%d frames)" % B)
        for b, f in enumerate(frames):
            if not torch.is_tensor(f) or f.dim() != 3:
                raise ValueError("prepare_frames: sample %d is not an (H, W, C) tensor" % b)
            if f.dtype not in (torch.float64, torch.float32):
                raise TypeError("prepare_frames: float64 or float32 frames, sample %d is %s" % (b, f.dtype))
            if f.dtype != frames[0].dtype or int(f.shape[2]) != int(frames[0].shape[2]):
                raise TypeError("prepare_frames: sample %d is %s with %d channels, sample 0 %s with %d"
                                % (b, f.dtype, int(f.shape[2]), frames[0].dtype, int(frames[0].shape[2])))
        C = int(frames[0].shape[2])
        if C < 1 or C > _lib.MAX_CHANNELS:
            raise ValueError("prepare_frames: 1..%d channels, not %d" % (_lib.MAX_CHANNELS, C))
        sizes = [(int(f.shape[0]), int(f.shape[1])) for f in frames]
        geos = self.frame_geometries(sizes)
        for b, f in enumerate(frames):
            if not f.is_cuda or f.device != frames[0].device:
                raise _lib.EvrepError("prepare_frames needs CUDA tensors on one device (sample %d is on %s); there is no CPU fallback"
                                      % (b, f.device))
        dev = frames[0].device
        if out is None:
            out = torch.empty((B, C, S, S), dtype=torch.float32, device=dev)
        else:
            want(out, "prepare_frames: out", torch.float32, (B, C, S, S), device=dev)
        if params is None:
            params = self.draw(B)
        table, host, n_axes, max_dst, rows_total, wt_total = self.frame_tables(sizes, geos, params)
        targets, shapes = self.targets_frames(sizes, labels, params)
        keep = [f if f.is_contiguous() else f.contiguous() for f in frames]
        table["src"] = [f.data_ptr() for f in keep]
        has_warp = host.size > n_axes * _lib.TAPS_AXIS_FIELDS
        api = _lib.api()
        up = torch.from_numpy(host).to(dev)                                    # the one upload
        axes_d = up[:n_axes * _lib.TAPS_AXIS_FIELDS]
        warp_d = up[n_axes * _lib.TAPS_AXIS_FIELDS:] if has_warp else None
        idx = torch.empty(2 * rows_total, dtype=torch.int32, device=dev)
        start_d, count_d = idx[:rows_total], idx[rows_total:]
        wt_d = torch.empty(wt_total, dtype=torch.float64, device=dev)
        frames_d = torch.empty(api.evrep_detector_input_frames_scratch_bytes(B) // 8, dtype=torch.int64, device=dev)
        pad_d = _pad_table(pad, C, dev)
        images = out
        with torch.cuda.device(dev):
            stream = stream_ptr()
            api.evrep_resize_tap_tables(ptr(axes_d), n_axes, max_dst, ptr(start_d), ptr(count_d), ptr(wt_d), rows_total, wt_total, stream)
            api.evrep_detector_input_frames(ctypes.c_void_p(table.ctypes.data), B, _lib.F64 if frames[0].dtype == torch.float64 else _lib.F32,
                                            C, S, ptr(start_d), ptr(count_d), ptr(wt_d), rows_total, wt_total, ptr(pad_d), ptr(warp_d),
                                            1.0 if scale is None else float(scale), ptr(frames_d), ptr(images), stream)
        return images, targets, shapes


_FRAME_DTYPE = np.dtype(_lib.DetinFrame)


def area_taps_bound(src, dst):
    """An upper bound, in closed form, on the taps of one output sample of an INTER_AREA axis: ceil(src / dst) + 1 (the cell
    [d scale, (d + 1) scale) touches at most that many source samples)."""
    return (int(src) + int(dst) - 1) // int(dst) + 1


def resize_tap_tables(axes, device):
    """One launch of evrep_resize_tap_tables for ``axes``, a list of (src, dst, interpolation, T) with interpolation "linear" /
    "area" / "identity".  Returns per axis the (start, count, weights, T) device tables, views into three tensors."""
    api = _lib.api()
    codes = {"linear": _lib.TAPS_LINEAR, "area": _lib.TAPS_AREA, "identity": _lib.TAPS_IDENTITY}
    desc, rows, wts = [], 0, 0
    for src, dst, interp, T in axes:
        desc.append((int(src), int(dst), codes[interp], int(T), rows, wts))
        rows, wts = rows + int(dst), wts + int(dst) * int(T)
    axes_d = torch.from_numpy(np.array(desc, dtype=np.int32).reshape(-1)).to(device)
    start = torch.empty(rows, dtype=torch.int32, device=device)
    count = torch.empty(rows, dtype=torch.int32, device=device)
    wt = torch.empty(wts, dtype=torch.float64, device=device)
    with torch.cuda.device(device):
        api.evrep_resize_tap_tables(ptr(axes_d), len(desc), max(d[1] for d in desc), ptr(start), ptr(count), ptr(wt), rows, wts, stream_ptr())
    return [(start[r:r + dst], count[r:r + dst], wt[w:w + dst * T].view(dst, T), T) for (_, dst, _, T, r, w) in desc]
