"""Scoring the detections: the statistics step of the reference's validation loop, on the device.

``ev-YOLOv6/yolov6/core/evaler.py:206-258`` takes, for every image of every batch, the detections to the host, rescales them
and the labels to the source frame, and calls ``yolov6/utils/metrics.py:process_batch`` (ten rounds of ``torch.where`` ->
``.cpu().numpy()`` -> ``argsort`` -> ``np.unique`` -> ``np.unique``) and optionally ``ConfusionMatrix.process_batch``.  Here
``match_batch`` does all of it for the padded batch ``nms_batch`` returned in ONE launch of ``evrep_det_match``
(csrc/evrep_deteval.hip: one workgroup per image), with no host read; ``DetectionEvaluator`` keeps the per-batch results on the
device.  ``compute()`` reads them back once and runs the reference's ``ap_per_class`` (its numpy statements, on the host: the
numpy route); ``compute_device()`` turns them into mAP where they lie (``evrep_det_ap_gather`` and ``evrep_det_ap``,
csrc/evrep_detap.hip: the device route, rules A1-A7 below) and reads back the small result.  ``match_host`` is the same rules
in numpy float32: what the tests hold the kernel to bit for bit, and the CPU route; ``ap_host`` is that for A1-A7.

The rules (include/evrep.h states them with the C entry point).  Per image b the detections are rows ``0 .. count[b]-1`` of
``det[b]``, ``[x1, y1, x2, y2, conf, cls]`` in NMS order; the labels are the rows of ``targets`` whose column 0 equals b, in
array order, ``[image, cls, cx, cy, w, h]``.  Every statement is one float32 operation.

1. Geometry, normalised mode (evaler.py:228-249).  Detections: ``scale_coords`` with ``ratio_pad`` given and ``scale_exact``
   false -- float32 pad and gain, subtract the pad, divide by ``gain[0]``, clamp to ``[0, w0]`` / ``[0, h0]``: what
   ``detector_output.scale_coords_batch`` does.  Labels: ``xywh2xyxy`` (``cx - w / 2``, ...), then ``x *= W``, ``y *= H`` of the
   letterboxed image, then the same ``scale_coords``.
2. Native mode: labels are ``[image, cls, x1, y1, x2, y2]`` and both sides are taken as they are: what
   ``process_batch(detections, labels, iouv)`` receives.
3. IoU (``general.box_iou(labels, detections)``): ``area = (x2 - x1) * (y2 - y1)``; ``w = clamp(min(x2l, x2d) - max(x1l, x1d), 0)``,
   ``h`` likewise; ``inter = w * h``; ``iou = inter / ((area_l + area_d) - inter)``.  ``0 / 0`` is NaN and matches nothing.
4. ``correct``: for detection j, ``k*(j)`` is the label of equal class (float equality) of greatest IoU, ``iou*(j)`` that
   value; ``correct[j, i]`` iff ``iou*(j) >= iouv[i]`` and no ``j' < j`` has ``k*(j') == k*(j)`` and ``iou*(j') >= iouv[i]``.
   This equals the reference's sort / unique / unique for every threshold.  TIE: among labels of equal greatest IoU the
   LOWEST label index wins.  The reference's ``argsort()[::-1]`` is numpy's unstable sort and leaves this open (the outcome depends on
   numpy's build and the CPU) -- the same kind of case as rule 4 of detector_output.py.
5. Confusion matrix (``ConfusionMatrix.process_batch``): only detections with ``conf > float32(conf)`` take part; for
   detection j the best label over ALL classes with ``iou > float32(iou_thres)`` (strict); for label k the detection of
   greatest IoU among those whose best label is k.  Ties: lowest label index, then lowest detection index (open in the
   reference, as in rule 4).  A matched label adds 1 at ``[int(cls_det), int(cls_label)]``, an unmatched one at
   ``[nc, int(cls_label)]``; detections that won no label add 1 at ``[int(cls_det), nc]``, but only if the image has at least one
   match.  A class outside ``[0, nc)`` sets ``ST_BAD_CLASS`` and that update is skipped (the reference raises or wraps).
   ``skip_empty`` is the evaler's guard (evaler.py:215-225): an image without detections adds nothing.

More than ``MAX_LABELS`` (1024) labels of one image: ``ST_LABEL_OVERFLOW``, all-false rows, nothing added to the matrix.  A count
outside ``[0, max_det]`` is clamped and sets ``ST_BAD_COUNT``.

The geometry is pinned to the reference's own ``Evaler.scale_coords`` and ``xywh2xyxy`` by tests/golden/detector_eval.npz, as
``process_batch``, ``ConfusionMatrix.process_batch`` and ``ap_per_class`` are (inputs without label ties).

Average precision, the device route and ``ap_host`` (include/evrep.h states the rules with evrep_det_ap).  Inputs: tp (n, T)
bool, conf (n,), pred_cls (n,), target_cls (m,) float32, nc.  Every float64 statement is one IEEE operation rounded on its own
(nothing fused, no float atomic, no reassociation): the same bits from run to run.

A1. Order: descending ``conf``; rows of equal confidence keep array order (stable; ``-0.0`` equals ``+0.0``), and array order is
    (batch, image, detection), the layout ``compute()`` builds.  The declared TIE rule: the reference's ``argsort(-conf)`` is
    numpy's unstable sort and leaves the curves open where two rows of a class tie.
A2. Classes: class c in ``[0, nc)`` owns the rows with ``pred_cls == c`` and ``n_l[c]`` targets.  A class outside ``[0, nc)`` or
    not integral sets ``AP_ST_BAD_CLASS`` and takes part in nothing; a NaN confidence sets ``AP_ST_NAN_CONF`` (its class's rows
    are then unspecified).
A3. Counts: at a class's k-th row (1-based) ``tpc[k, j]`` = the integer count of true ``tp[., j]`` among its first k rows,
    ``recall = double(tpc) / double(n_l)`` (``n_l + 1e-16`` is ``n_l`` in float64), ``precision = double(tpc) / double(k)``.  A
    class with ``n_p == 0`` or ``n_l == 0`` has all-zero rows in every output.
A4. Curves: ``px = np.linspace(0, 1, 1000)`` (uploaded, not recomputed); ``r[c] = interp(-px, -conf_c, recall[:, 0], left=0)``,
    ``p[c] = interp(-px, -conf_c, precision[:, 0], left=1)``, ``conf_c`` widened to float64.
A5. ``interp(x, xp, fp, left, right=fp[-1])``: ``x < xp[0]`` -> left; ``x > xp[-1]`` -> right; else j the LARGEST index with
    ``xp[j] <= x``: the last -> ``fp[-1]``; ``xp[j] == x`` -> ``fp[j]``; else
    ``((fp[j+1] - fp[j]) / (xp[j+1] - xp[j])) * (x - xp[j]) + fp[j]``.
A6. ``compute_ap`` per (class, threshold): ``mrec = [0, recall[:, j], recall[-1, j] + 0.01]``, ``mpre = [1, precision[:, j], 0]``
    replaced by its running maximum from the right, ``y = interp(linspace(0, 1, 101), mrec, mpre)``,
    ``ap = sum_i (d_i * (y_i + y_{i+1})) / 2.0`` with ``d = np.diff(linspace(0, 1, 101))``, added in ascending i one at a time
    (numpy's ``trapz`` adds pairwise: within 2.2e-14 of it).
A7. ``f1 = ((2 * p) * r) / ((p + r) + 1e-16)``.

Not mirrored: plots and ``print``; pycocotools' evaluation; ``scale_exact=True``; half-precision input.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .detector_output import xywh2xyxy  # noqa: F401  (the reference imports it beside process_batch)

F32 = np.float32
MAX_LABELS = _lib.DETEVAL_MAX_LABELS
MAX_T = _lib.DETEVAL_MAX_T
ST_LABEL_OVERFLOW, ST_BAD_CLASS, ST_BAD_COUNT = _lib.DETEVAL_ST_LABEL_OVERFLOW, _lib.DETEVAL_ST_BAD_CLASS, _lib.DETEVAL_ST_BAD_COUNT
_STATUS_TEXT = ((ST_LABEL_OVERFLOW, "more than %d labels" % MAX_LABELS), (ST_BAD_CLASS, "a class outside [0, nc)"),
                (ST_BAD_COUNT, "a count outside [0, max_det]"))


def default_iouv():
    """``torch.linspace(0.5, 0.95, 10)``: the evaler's thresholds, as float32 numpy."""
    return torch.linspace(0.5, 0.95, 10).numpy()


def _iouv_host(iouv):
    if iouv is None:
        return default_iouv()
    v = iouv.detach().cpu().numpy() if isinstance(iouv, torch.Tensor) else np.asarray(iouv)
    v = np.ascontiguousarray(v, dtype=F32).reshape(-1)
    if not 1 <= v.size <= MAX_T or np.isnan(v).any():
        raise ValueError("iouv must hold 1..%d thresholds, none of them NaN" % MAX_T)
    return v


def geometry_rows(shapes, B):
    """(B, 5) float32 ``[pad_x, pad_y, gain, w0, h0]`` from the list ``DetectorFrontEnd.prepare`` returned, one
    ``((h0, w0), ((gain_y, gain_x), (pad_x, pad_y)))`` per image -- the float32 values scale_coords computes with."""
    if len(shapes) != B:
        raise ValueError("%d shapes for %d images" % (len(shapes), B))
    return np.array([[ratio_pad[1][0], ratio_pad[1][1], ratio_pad[0][0], w0, h0] for (h0, w0), ratio_pad in shapes],
                    dtype=np.float64).astype(F32).reshape(B, 5)


def geometry_tensor(shapes, device):
    """``geometry_rows`` as a (B, 5) float32 tensor on ``device``: what ``match_batch`` uploads on every call when it is given
    the list.  Made once and passed as ``shapes``, the call uploads nothing -- which a graph capture requires."""
    return torch.from_numpy(geometry_rows(shapes, len(shapes))).to(device)


def box_iou(box1, box2):
    """``general.box_iou``: the (N, M) IoU of (N, 4) and (M, 4) xyxy boxes; the reference's torch statements, on the boxes' device."""
    def box_area(box):
        return (box[2] - box[0]) * (box[3] - box[1])

    area1, area2 = box_area(box1.T), box_area(box2.T)
    inter = (torch.min(box1[:, None, 2:], box2[:, 2:]) - torch.max(box1[:, None, :2], box2[:, :2])).clamp(0).prod(2)
    return inter / (area1[:, None] + area2 - inter)


# ------------------------------------------------------------------------------------------------------------ the host route
def _clamp(v, hi):
    """clamp_(0, hi) as two comparisons: a NaN stays."""
    return np.where(v < 0, F32(0), np.where(v > hi, hi, v)).astype(F32)


def _scale_coords_host(box, g):
    """Rule 1's scale_coords on (n, 4) float32 boxes; g = [pad_x, pad_y, gain, w0, h0] float32."""
    out = np.empty_like(box)
    out[:, 0] = _clamp((box[:, 0] - g[0]) / g[2], g[3])
    out[:, 1] = _clamp((box[:, 1] - g[1]) / g[2], g[4])
    out[:, 2] = _clamp((box[:, 2] - g[0]) / g[2], g[3])
    out[:, 3] = _clamp((box[:, 3] - g[1]) / g[2], g[4])
    return out


def _label_boxes_host(rows, g, H, W):
    """Rule 1 for the labels: (n, 4) [cx, cy, w, h] -> native-space xyxy."""
    hw, hh = rows[:, 2] * F32(0.5), rows[:, 3] * F32(0.5)
    box = np.stack([(rows[:, 0] - hw) * F32(W), (rows[:, 1] - hh) * F32(H), (rows[:, 0] + hw) * F32(W), (rows[:, 1] + hh) * F32(H)], axis=1)
    return _scale_coords_host(box.astype(F32), g)


def iou_host(lab, det):
    """Rule 3 in numpy float32: (M, 4) labels x (n, 4) detections -> (M, n)."""
    lab, det = np.asarray(lab, F32).reshape(-1, 4), np.asarray(det, F32).reshape(-1, 4)
    al = (lab[:, 2] - lab[:, 0]) * (lab[:, 3] - lab[:, 1])
    ad = (det[:, 2] - det[:, 0]) * (det[:, 3] - det[:, 1])
    dw = np.minimum(lab[:, None, 2], det[None, :, 2]) - np.maximum(lab[:, None, 0], det[None, :, 0])
    dh = np.minimum(lab[:, None, 3], det[None, :, 3]) - np.maximum(lab[:, None, 1], det[None, :, 1])
    w, h = np.where(dw < 0, F32(0), dw), np.where(dh < 0, F32(0), dh)
    inter = w * h
    return (inter / ((al[:, None] + ad[None, :]) - inter)).astype(F32)


def _best_label(iou, allowed):
    """Per detection (column): (found, k, value) of the greatest non-NaN IoU among the allowed labels, lowest label first."""
    M, n = iou.shape
    if M == 0 or n == 0:
        return np.zeros(n, bool), np.zeros(n, np.int64), np.zeros(n, F32)
    ok = allowed & ~np.isnan(iou)
    found = ok.any(axis=0)
    k = np.argmax(np.where(ok, iou, -np.inf), axis=0)                 # the first maximum
    first_ok = np.argmax(ok, axis=0)                                  # (every allowed value is -inf: the first allowed one)
    cols = np.arange(n)
    k = np.where(ok[k, cols], k, first_ok)
    return found, k, iou[k, cols]


def _class_index(c, nc):
    """int(c) when it lies in [0, nc), else None (c > -1 and c < nc in float32; a NaN fails)."""
    return int(c) if (c > F32(-1) and c < F32(nc)) else None


def _image_host(d, lab_cls, lab_box, iouv, correct, matrix, nc, conf, iou_thres, use_matrix):
    """Rules 3-5 for one image; writes correct (n, T) in place, adds to matrix, returns the status bits it sets."""
    n, M, status = d.shape[0], lab_box.shape[0], 0
    with np.errstate(all="ignore"):
        iou = iou_host(lab_box, d[:, :4])
        found, k, best = _best_label(iou, lab_cls[:, None] == d[None, :, 5])
        for i, thr in enumerate(iouv):
            js = np.flatnonzero(found & (best >= thr))
            if js.size:
                correct[js[np.unique(k[js], return_index=True)[1]], i] = 1       # the first claimant of every label
        if not use_matrix:
            return status
        part = d[:, 4] > F32(conf)
        cfound, ck, cbest = _best_label(iou, (iou > F32(iou_thres)) & part[None, :])
    winner = np.full(M, -1, np.int64)
    for j in np.flatnonzero(cfound):                                   # ascending j: a later one wins only with a greater IoU
        if winner[ck[j]] < 0 or cbest[j] > cbest[winner[ck[j]]]:
            winner[ck[j]] = j

    def add(row, col):
        nonlocal status
        if row is None or col is None:
            status |= ST_BAD_CLASS
        else:
            matrix[row * (nc + 1) + col] += 1

    for kk in range(M):
        gc = _class_index(lab_cls[kk], nc)
        add(_class_index(d[winner[kk], 5], nc) if winner[kk] >= 0 else nc, gc)
    if (winner >= 0).any():
        won = set(winner[winner >= 0].tolist())
        for j in np.flatnonzero(part):
            if j not in won:
                add(_class_index(d[j, 5], nc), nc)
    return status


def match_host(det, count, targets, img_shape=None, shapes=None, iouv=None, native=False, matrix=None, nc=0, conf=0.25,
               iou_thres=0.45, skip_empty=False):
    """The rules of this module in numpy float32 for a padded batch: det (B, max_det, 6), count (B,), targets (n_t, 6).
    Returns ``(correct uint8 (B, max_det, T), detn float32 (B, max_det, 6), tbox float32 (n_t, 4), n_labels int32 (B,),
    status uint32 (B,))``.  ``matrix``: an int64 array of (nc + 1) ** 2 elements that rule 5 adds to in place (None: no
    confusion matrix).  ``native``: rule 2, img_shape and shapes are not read."""
    det = np.ascontiguousarray(det, dtype=F32)
    count = np.asarray(count).astype(np.int64).reshape(-1)
    targets = np.ascontiguousarray(targets, dtype=F32).reshape(-1, 6)
    iouv = _iouv_host(iouv)
    B, max_det, T = det.shape[0], det.shape[1], iouv.size
    if det.ndim != 3 or det.shape[2] != 6 or count.size != B:
        raise ValueError("det must be (B, max_det, 6) and count (B,)")
    geom = None if native else geometry_rows(shapes, B)
    H, W = (0, 0) if native else (int(img_shape[0]), int(img_shape[1]))
    correct = np.zeros((B, max_det, T), np.uint8)
    detn = np.zeros((B, max_det, 6), F32)
    tbox = np.zeros((targets.shape[0], 4), F32)
    n_labels = np.zeros(B, np.int32)
    status = np.zeros(B, np.uint32)
    with np.errstate(all="ignore"):
        for b in range(B):
            n = int(min(max(count[b], 0), max_det))
            if n != count[b]:
                status[b] |= ST_BAD_COUNT
            rows = np.flatnonzero(targets[:, 0] == F32(b))
            n_labels[b] = rows.size
            lab_box = targets[rows, 2:6] if native else _label_boxes_host(targets[rows, 2:6], geom[b], H, W)
            tbox[rows] = lab_box
            d = det[b, :n].copy()
            if not native:
                d[:, :4] = _scale_coords_host(d[:, :4], geom[b])
            detn[b, :n] = d
            if rows.size > MAX_LABELS:
                status[b] |= ST_LABEL_OVERFLOW
                continue
            use_matrix = matrix is not None and not (skip_empty and n == 0)
            status[b] |= _image_host(d, targets[rows, 1], lab_box, iouv, correct[b], matrix, nc, conf, iou_thres, use_matrix)
    return correct, detn, tbox, n_labels, status


# ---------------------------------------------------------------------------------------------------------- the device route
def _launch(det, count, targets, geom, img_hw, iouv, native, matrix, nc, conf, iou_thres, skip_empty, want_detn, want_tbox):
    if not (isinstance(det, torch.Tensor) and det.is_cuda):
        raise ValueError("match_batch: det must be a CUDA tensor (CPU arrays go through match_host)")
    if det.dtype != torch.float32:
        raise ValueError("det is %s: the device route computes in float32, call .float() on it first" % det.dtype)
    if det.dim() != 3 or det.shape[2] != 6:
        raise ValueError("det must be (B, max_det, 6)")
    dev = det.device
    B, max_det, T = int(det.shape[0]), int(det.shape[1]), int(iouv.size)
    if not (1 <= B <= 65535 and 1 <= max_det <= _lib.NMS_MAX_DET):
        raise ValueError("match_batch: 1 <= B <= 65535 and 1 <= max_det <= %d" % _lib.NMS_MAX_DET)
    det = det.contiguous()
    count = _lib.want(count.to(dev).contiguous(), "count", torch.int32, shape=(B,), device=dev)
    targets = targets.to(dev)
    if targets.dtype != torch.float32 or targets.dim() != 2 or targets.shape[1] != 6:
        raise ValueError("targets must be a float32 (n_t, 6) tensor")
    targets = targets.contiguous()
    n_t = int(targets.shape[0])
    correct = torch.empty((B, max_det, T), dtype=torch.uint8, device=dev)
    detn = torch.empty((B, max_det, 6), dtype=torch.float32, device=dev) if want_detn else None
    tbox = torch.empty((n_t, 4), dtype=torch.float32, device=dev) if want_tbox else None
    n_labels = torch.empty((B,), dtype=torch.int32, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    geom_d = None
    if not native:
        geom_d = geom if isinstance(geom, torch.Tensor) else torch.from_numpy(geom).to(dev)
        _lib.want(geom_d, "the geometry rows", torch.float32, shape=(B, 5), device=dev)
    flags = (_lib.DETEVAL_NATIVE if native else 0) | (_lib.DETEVAL_SKIP_EMPTY if skip_empty else 0)
    iouv_arr = (ctypes.c_float * T)(*[float(v) for v in iouv])
    if matrix is not None:
        _lib.want(matrix, "matrix", torch.int64, numel=(nc + 1) * (nc + 1), device=dev)
    with torch.cuda.device(dev):
        _lib.api().evrep_det_match(_lib.ptr(det), _lib.ptr(count), B, max_det, _lib.ptr(targets) if n_t else None, n_t,
                                   _lib.ptr(geom_d), int(img_hw[0]), int(img_hw[1]), iouv_arr, T, flags, _lib.ptr(matrix), int(nc),
                                   float(F32(conf)), float(F32(iou_thres)), _lib.ptr(correct), _lib.ptr(detn), _lib.ptr(tbox),
                                   _lib.ptr(n_labels), _lib.ptr(status), _lib.stream_ptr())
    return correct, detn, tbox, n_labels, status


def match_batch(det, count, targets, img_shape, shapes, iouv=None, confusion=None, skip_empty=True, return_tbox=False):
    """evaler.py:209-258 for the padded batch of ``nms_batch``: det (B, max_det, 6) and count (B,) on the device, targets
    (n_t, 6) ``[image, cls, cx, cy, w, h]`` normalised to the letterboxed image of ``img_shape`` (H, W), ``shapes`` the list
    ``DetectorFrontEnd.prepare`` returned.  Returns ``(correct uint8 (B, max_det, T), detn (B, max_det, 6), n_labels int32 (B,),
    status int32 (B,))`` on the device; one launch, no host read, no wait.  ``shapes`` may also be the (B, 5) device tensor of
    ``geometry_tensor``; with it (and a confusion matrix whose device array exists) the call can be captured into a graph.  ``confusion``: a ``ConfusionMatrix`` whose
    device matrix the launch adds to, images without detections left out as the evaler does (``skip_empty``).  ``return_tbox``
    appends the (n_t, 4) native-space label boxes."""
    iouv = _iouv_host(iouv)
    B = int(det.shape[0])
    geom = shapes if isinstance(shapes, torch.Tensor) else geometry_rows(shapes, B)
    matrix = confusion.device_matrix(det.device) if confusion is not None else None
    correct, detn, tbox, n_labels, status = _launch(
        det, count, targets, geom, img_shape, iouv, False, matrix, confusion.nc if confusion is not None else 0,
        confusion.conf if confusion is not None else 0.25, confusion.iou_thres if confusion is not None else 0.45,
        bool(skip_empty), True, bool(return_tbox))
    return (correct, detn, n_labels, status, tbox) if return_tbox else (correct, detn, n_labels, status)


def _native_inputs(detections, labels):
    n, M = int(detections.shape[0]), int(labels.shape[0])
    if n > _lib.NMS_MAX_DET:
        raise ValueError("at most %d detections per image on the device" % _lib.NMS_MAX_DET)
    dev = detections.device
    det = torch.zeros((1, max(n, 1), 6), dtype=torch.float32, device=dev)
    det[0, :n] = detections.float()
    targets = torch.zeros((M, 6), dtype=torch.float32, device=dev)
    targets[:, 1:] = labels.to(dev).float()
    return det, torch.tensor([n], dtype=torch.int32).to(dev), targets


def process_batch(detections, labels, iouv):
    """``metrics.process_batch``: detections (n, 6) ``[x1, y1, x2, y2, conf, cls]``, labels (M, 5) ``[cls, x1, y1, x2, y2]`` ->
    the (n, T) bool matrix of correct predictions on ``iouv``'s device.  CUDA detections: one launch in native mode with B = 1;
    CPU tensors: ``match_host``.  Rule 4's tie rule holds where the reference leaves the outcome open."""
    v = _iouv_host(iouv)
    n = int(detections.shape[0])
    out_dev = iouv.device if isinstance(iouv, torch.Tensor) else detections.device
    if isinstance(detections, torch.Tensor) and detections.is_cuda:
        det, count, targets = _native_inputs(detections, labels)
        correct = _launch(det, count, targets, None, (0, 0), v, True, None, 0, 0.25, 0.45, False, False, False)[0]
        return correct[0, :n].bool().to(out_dev)
    det = detections.detach().float().numpy().reshape(1, n, 6) if n else np.zeros((1, 0, 6), F32)
    lab = labels.detach().float().numpy().reshape(-1, 5)
    targets = np.concatenate([np.zeros((lab.shape[0], 1), F32), lab], axis=1)
    correct = match_host(det, [n], targets, iouv=v, native=True)[0]
    return torch.from_numpy(correct[0].astype(bool)).to(out_dev)


class ConfusionMatrix:
    """``metrics.ConfusionMatrix``: ``process_batch(detections, labels)``, ``matrix`` ((nc + 1, nc + 1) float64, as the
    reference's attribute) and ``tp_fp()``.  The counts are integers: a host int64 array for CPU inputs and, once a CUDA
    input or ``match_batch`` has asked for it, a device int64 array that launches add to; ``matrix`` reads the device part back."""

    def __init__(self, nc, conf=0.25, iou_thres=0.45):
        if not 1 <= int(nc) <= _lib.NMS_MAX_CLASSES:
            raise ValueError("nc must be in 1..%d" % _lib.NMS_MAX_CLASSES)
        self.nc, self.conf, self.iou_thres = int(nc), conf, iou_thres
        self._host = np.zeros((self.nc + 1) * (self.nc + 1), np.int64)
        self._dev = None
        self.status = 0                     # the status bits of the CPU route (the device route's are in its status words)

    def device_matrix(self, device):
        """The device int64 array of (nc + 1) ** 2 counts (made and zeroed at the first call)."""
        if self._dev is None:
            self._dev = torch.zeros((self.nc + 1) * (self.nc + 1), dtype=torch.int64, device=device)
        elif self._dev.device != torch.device(device):
            raise ValueError("the confusion matrix lives on %s" % self._dev.device)
        return self._dev

    def process_batch(self, detections, labels):
        n = int(detections.shape[0])
        if isinstance(detections, torch.Tensor) and detections.is_cuda:
            det, count, targets = _native_inputs(detections, labels)
            _launch(det, count, targets, None, (0, 0), np.array([0.5], F32), True, self.device_matrix(det.device), self.nc,
                    self.conf, self.iou_thres, False, False, False)
            return
        det = detections.detach().float().numpy().reshape(1, n, 6) if n else np.zeros((1, 0, 6), F32)
        lab = labels.detach().float().numpy().reshape(-1, 5)
        targets = np.concatenate([np.zeros((lab.shape[0], 1), F32), lab], axis=1)
        st = match_host(det, [n], targets, iouv=np.array([0.5], F32), native=True, matrix=self._host, nc=self.nc, conf=self.conf,
                        iou_thres=self.iou_thres)[4]
        self.status |= int(st[0])

    def counts(self):
        """The (nc + 1, nc + 1) int64 counts, host and device parts together (one read-back when a device part exists)."""
        total = self._host.copy()
        if self._dev is not None:
            total += self._dev.cpu().numpy()
        return total.reshape(self.nc + 1, self.nc + 1)

    @property
    def matrix(self):
        return self.counts().astype(np.float64)

    def tp_fp(self):
        m = self.matrix
        tp = m.diagonal()
        fp = m.sum(1) - tp
        return tp[:-1], fp[:-1]


# ------------------------------------------------------------------------------------------------ AP: the reference's numpy
_trapezoid = getattr(np, "trapezoid", None) or np.trapz


def compute_ap(recall, precision):
    """``metrics.compute_ap`` (the 101-point interpolation): (ap, mpre, mrec)."""
    mrec = np.concatenate(([0.0], recall, [recall[-1] + 0.01]))
    mpre = np.concatenate(([1.0], precision, [0.0]))
    mpre = np.flip(np.maximum.accumulate(np.flip(mpre)))
    x = np.linspace(0, 1, 101)
    ap = _trapezoid(np.interp(x, mrec, mpre), x)
    return ap, mpre, mrec


def ap_per_class(tp, conf, pred_cls, target_cls, nc=None):
    """``metrics.ap_per_class`` without its plots: (p, r, ap, f1, unique_classes int32); p, r, f1 are (classes, 1000) curves
    over confidence, ap is (classes, T).  numpy arrays: the reference's numpy statements, on the host.  CUDA tensors: the device
    route (``ap_device``, rules A1-A7), the small result read back once and restricted to the classes present in
    ``target_cls``; ``nc`` (the number of classes) defaults to the largest target class + 1, which costs no read when
    ``target_cls`` lives on the host and one scalar read in front of the launches when it lives on the device.  On the device
    route a NaN confidence raises ValueError (the status word comes back in the same read); a predicted class outside
    ``[0, nc)`` is, as in the reference, a class without labels and takes part in nothing."""
    if any(isinstance(v, torch.Tensor) and v.is_cuda for v in (tp, conf, pred_cls)):
        return _ap_per_class_device(tp, conf, pred_cls, target_cls, nc)
    i = np.argsort(-conf)
    tp, conf, pred_cls = tp[i], conf[i], pred_cls[i]
    unique_classes = np.unique(target_cls)
    nc = unique_classes.shape[0]
    px = np.linspace(0, 1, 1000)
    ap, p, r = np.zeros((nc, tp.shape[1])), np.zeros((nc, 1000)), np.zeros((nc, 1000))
    for ci, c in enumerate(unique_classes):
        i = pred_cls == c
        n_l = (target_cls == c).sum()
        n_p = i.sum()
        if n_p == 0 or n_l == 0:
            continue
        fpc = (1 - tp[i]).cumsum(0)
        tpc = tp[i].cumsum(0)
        recall = tpc / (n_l + 1e-16)
        r[ci] = np.interp(-px, -conf[i], recall[:, 0], left=0)
        precision = tpc / (tpc + fpc)
        p[ci] = np.interp(-px, -conf[i], precision[:, 0], left=1)
        for j in range(tp.shape[1]):
            ap[ci, j], _, _ = compute_ap(recall[:, j], precision[:, j])
    f1 = 2 * p * r / (p + r + 1e-16)
    return p, r, ap, f1, unique_classes.astype("int32")


def summarize(stats, nc, seen):
    """evaler.py:260-283 on ``stats = (correct (n, T) bool, conf (n,), pred_cls (n,), target_cls (m,))``: a dict with ``p, r, ap,
    f1, ap_class, best_f1_index, mp, mr, map50, map, nt, seen`` -- or ``(0.0, 0.0)``, as the reference returns, when no
    prediction is correct."""
    if not (len(stats) and stats[0].any()):
        return 0.0, 0.0
    p, r, ap, f1, ap_class = ap_per_class(*stats)
    nt = np.bincount(stats[3].astype(np.int64), minlength=nc)
    return _summary(p, r, ap, f1, ap_class, nt, seen)


def _summary(p, r, ap, f1, ap_class, nt, seen):
    """evaler.py:266-283: the means at the best-F1 confidence, behind either route to ``p, r, ap, f1``."""
    best = len(f1.mean(0)) - f1.mean(0)[::-1].argmax() - 1
    ap50, ap_mean = ap[:, 0], ap.mean(1)
    return dict(p=p, r=r, ap=ap, f1=f1, ap_class=ap_class, best_f1_index=int(best), mp=p[:, best].mean(), mr=r[:, best].mean(),
                map50=ap50.mean(), map=ap_mean.mean(), nt=nt, seen=int(seen))


# ------------------------------------------------------------------------------------- AP: the declared rules, host and device
AP_ST_BAD_CLASS, AP_ST_NAN_CONF = _lib.AP_ST_BAD_CLASS, _lib.AP_ST_NAN_CONF
_AP_STATUS_TEXT = ((AP_ST_BAD_CLASS, "a prediction or target class outside [0, nc) or not integral"), (AP_ST_NAN_CONF, "a NaN confidence"))


def ap_tables():
    """float64 [1201]: ``linspace(0, 1, 1000)``, ``linspace(0, 1, 101)`` and the latter's ``diff`` -- numpy's own values, which
    the device route uploads and does not recompute (A4, A6)."""
    x = np.linspace(0, 1, _lib.AP_X)
    return np.concatenate([np.linspace(0, 1, _lib.AP_PX), x, np.diff(x)])


def _interp_host(x, xp, fp, left, right):
    """A5 for ascending ``xp``: numpy's interp restated, one float64 operation per statement."""
    last = xp.size - 1
    j = np.searchsorted(xp, x, side="right") - 1                      # the LARGEST j with xp[j] <= x; -1: x < xp[0]
    j0 = np.clip(j, 0, max(last - 1, 0))
    j1 = np.minimum(j0 + 1, last)
    with np.errstate(all="ignore"):
        slope = (fp[j1] - fp[j0]) / (xp[j1] - xp[j0])
        out = slope * (x - xp[j0]) + fp[j0]
    out = np.where(xp[j0] == x, fp[j0], out)
    out = np.where(j >= last, fp[last], out)
    out = np.where(x > xp[last], right, out)
    return np.where(x < xp[0], left, out)


def _class_bins(cls, nc):
    """A2: (the class of every element as int64, nc for one that takes part in nothing; whether any such element exists)."""
    cls = np.asarray(cls, F32).reshape(-1)
    with np.errstate(invalid="ignore"):
        ok = (cls >= 0) & (cls < nc) & (cls == np.floor(cls))
    return np.where(ok, cls, nc).astype(np.int64), bool((~ok).any())


def ap_host(tp, conf, pred_cls, target_cls, nc):
    """Rules A1-A7 (include/evrep.h, with evrep_det_ap) in numpy: the CPU route, and what the tests hold the kernels to bit for
    bit.  tp (n, T) bool / uint8, conf (n,), pred_cls (n,), target_cls (m,) -> ``(p, r, ap, f1, n_labels, n_pred, any_correct,
    status)``: p, r, f1 float64 (nc, 1000), ap float64 (nc, T), n_labels and n_pred int64 (nc,), two ints."""
    tp = np.asarray(tp)
    conf = np.ascontiguousarray(conf, dtype=F32).reshape(-1)
    n, nc = conf.size, int(nc)
    if tp.ndim != 2 or tp.shape[0] != n:
        raise ValueError("tp must be (n, T) with one row per confidence")
    tp = tp != 0
    T = tp.shape[1]
    if not (1 <= T <= MAX_T and 1 <= nc <= _lib.NMS_MAX_CLASSES):
        raise ValueError("ap_host: 1 <= T <= %d and 1 <= nc <= %d" % (MAX_T, _lib.NMS_MAX_CLASSES))
    pc, bad_p = _class_bins(pred_cls, nc)
    tc, bad_t = _class_bins(target_cls, nc)
    if pc.size != n:
        raise ValueError("tp, conf and pred_cls must have one row per prediction")
    status = (AP_ST_BAD_CLASS if bad_p or bad_t else 0) | (AP_ST_NAN_CONF if np.isnan(conf).any() else 0)
    n_pred = np.bincount(pc, minlength=nc + 1)[:nc].astype(np.int64)
    n_labels = np.bincount(tc, minlength=nc + 1)[:nc].astype(np.int64)
    tables = ap_tables()
    px, x101, d = tables[:_lib.AP_PX], tables[_lib.AP_PX:_lib.AP_PX + _lib.AP_X], tables[_lib.AP_PX + _lib.AP_X:]
    p, r, ap = np.zeros((nc, _lib.AP_PX)), np.zeros((nc, _lib.AP_PX)), np.zeros((nc, T))
    order = np.argsort(-conf, kind="stable")                          # A1: descending, equal confidences in array order
    pc_sorted = pc[order]
    for c in np.flatnonzero((n_pred > 0) & (n_labels > 0)):
        rows = order[pc_sorted == c]
        tpc = tp[rows].cumsum(0, dtype=np.int64)
        recall = tpc.astype(np.float64) / np.float64(n_labels[c])
        precision = tpc.astype(np.float64) / np.arange(1, rows.size + 1, dtype=np.float64)[:, None]
        xp = -conf[rows].astype(np.float64)
        r[c] = _interp_host(-px, xp, recall[:, 0], 0.0, recall[-1, 0])
        p[c] = _interp_host(-px, xp, precision[:, 0], 1.0, precision[-1, 0])
        for j in range(T):
            mrec = np.concatenate(([0.0], recall[:, j], [recall[-1, j] + 0.01]))
            mpre = np.concatenate(([1.0], precision[:, j], [0.0]))
            mpre = np.flip(np.maximum.accumulate(np.flip(mpre)))
            y = _interp_host(x101, mrec, mpre, mpre[0], mpre[-1])
            ap[c, j] = np.add.accumulate((d * (y[:-1] + y[1:])) / 2.0)[-1]      # ascending, one addition at a time
    f1 = ((2 * p) * r) / ((p + r) + 1e-16)
    return p, r, ap, f1, n_labels, n_pred, int(tp.any()), int(status)


_AP_TABLES = {}


def _ap_tables_device(dev):
    if dev not in _AP_TABLES:
        _AP_TABLES[dev] = torch.from_numpy(ap_tables()).to(dev)
    return _AP_TABLES[dev]


def ap_workspace_bytes(n, T, nc):
    """``evrep_det_ap_workspace_bytes``: the scratch of ``ap_device`` for up to n rows."""
    size = _lib.api().evrep_det_ap_workspace_bytes(int(n), int(T), int(nc))
    if size == 0:
        raise ValueError("ap_device: 0 <= n < 2**31, 1 <= T <= %d and 1 <= nc <= %d" % (MAX_T, _lib.NMS_MAX_CLASSES))
    return size


def ap_device(tp, conf, pred_cls, target_cls, nc, counts=None, out=None, workspace=None):
    """Rules A1-A7 on CUDA tensors: tp (n, T) bool / uint8, conf (n,), pred_cls (n,), target_cls (m,) float32 -> the device
    tensors ``(p, r, ap, f1, n_labels, n_pred, any_correct, status)`` of ``ap_host``'s shapes (the last two int32 of one
    element).  The launch sequence of evrep_det_ap; nothing is read back, nothing waits.  ``counts``: an int64 (2,) device
    tensor holding the true n and m, when only the device knows them (the tensors' sizes are then capacities).  ``out`` /
    ``workspace``: tensors to write into, as returned / of ``ap_workspace_bytes`` bytes."""
    if not (isinstance(conf, torch.Tensor) and conf.is_cuda):
        raise ValueError("ap_device: conf must be a CUDA tensor (CPU arrays go through ap_host)")
    dev, n, nc = conf.device, int(conf.shape[0]), int(nc)
    if tp.dtype == torch.bool:
        tp = tp.view(torch.uint8)
    _lib.want(tp, "tp", torch.uint8, shape=(n, None), device=dev)
    T = int(tp.shape[1])
    _lib.want(conf, "conf", torch.float32, shape=(n,), device=dev)
    _lib.want(pred_cls, "pred_cls", torch.float32, shape=(n,), device=dev)
    _lib.want(target_cls, "target_cls", torch.float32, shape=(None,), device=dev)
    m = int(target_cls.shape[0])
    if counts is not None:
        _lib.want(counts, "counts", torch.int64, shape=(2,), device=dev)
    size = ap_workspace_bytes(n, T, nc)
    if workspace is None:
        workspace = _lib.scratch(size, dev)
    _lib.want(workspace, "workspace", torch.uint8, device=dev)
    if out is None:
        f64 = dict(dtype=torch.float64, device=dev)
        out = (torch.empty((nc, _lib.AP_PX), **f64), torch.empty((nc, _lib.AP_PX), **f64), torch.empty((nc, T), **f64),
               torch.empty((nc, _lib.AP_PX), **f64), torch.empty(nc, dtype=torch.int64, device=dev),
               torch.empty(nc, dtype=torch.int64, device=dev), torch.empty(1, dtype=torch.int32, device=dev),
               torch.empty(1, dtype=torch.int32, device=dev))
    p, r, ap, f1, n_labels, n_pred, any_correct, status = out
    for t, what, dtype, shape in ((p, "p", torch.float64, (nc, _lib.AP_PX)), (r, "r", torch.float64, (nc, _lib.AP_PX)),
                                  (ap, "ap", torch.float64, (nc, T)), (f1, "f1", torch.float64, (nc, _lib.AP_PX)),
                                  (n_labels, "n_labels", torch.int64, (nc,)), (n_pred, "n_pred", torch.int64, (nc,)),
                                  (any_correct, "any_correct", torch.int32, (1,)), (status, "status", torch.int32, (1,))):
        _lib.want(t, what, dtype, shape=shape, device=dev)
    with torch.cuda.device(dev):
        _lib.api().evrep_det_ap(_lib.ptr(tp) if n else None, _lib.ptr(conf) if n else None, _lib.ptr(pred_cls) if n else None,
                                _lib.ptr(target_cls) if m else None, n, m, T, nc, _lib.ptr(counts), _lib.ptr(_ap_tables_device(dev)),
                                _lib.ptr(p), _lib.ptr(r), _lib.ptr(f1), _lib.ptr(ap), _lib.ptr(n_labels), _lib.ptr(n_pred),
                                _lib.ptr(any_correct), _lib.ptr(status), _lib.ptr(workspace), workspace.numel(), _lib.stream_ptr())
    return out


def _read_once(tensors):
    """The tensors as numpy arrays through ONE device-to-host copy."""
    if not tensors:
        return []
    flat = torch.cat([t.contiguous().reshape(-1).view(torch.uint8) for t in tensors]).cpu().numpy()
    host, at = [], 0
    for t in tensors:
        nbytes = t.numel() * t.element_size()
        host.append(flat[at:at + nbytes].view(torch.empty(0, dtype=t.dtype).numpy().dtype).reshape(tuple(t.shape)))
        at += nbytes
    return host


def _raise_ap_status(status):
    if status:
        raise ValueError("%s (AP status %d)" % (", ".join(text for bit, text in _AP_STATUS_TEXT if status & bit), status))


def _ap_per_class_device(tp, conf, pred_cls, target_cls, nc):
    dev = next(v.device for v in (tp, conf, pred_cls) if isinstance(v, torch.Tensor) and v.is_cuda)
    tp, conf, pred_cls = (torch.as_tensor(v).to(dev) for v in (tp, conf, pred_cls))
    if nc is None:
        t = target_cls.detach() if isinstance(target_cls, torch.Tensor) else np.asarray(target_cls)
        top = float(t.max()) if len(t) else 0.0                       # (a device target_cls: the one scalar read)
        if not 0 <= top < _lib.NMS_MAX_CLASSES:
            raise ValueError("ap_per_class: the largest target class must lie in [0, %d)" % _lib.NMS_MAX_CLASSES)
        nc = int(top) + 1
    target_cls = torch.as_tensor(target_cls, dtype=torch.float32).to(dev).contiguous().reshape(-1)
    out = ap_device(tp.contiguous(), conf.float().contiguous(), pred_cls.float().contiguous(), target_cls, nc)
    p, r, ap, f1, n_labels, status = _read_once(list(out[:5]) + [out[7]])
    # AP_ST_BAD_CLASS is not an error here: with nc taken from the targets a prediction of a class beyond them is a class
    # without labels, which takes part in nothing in the reference either.  A NaN confidence leaves its class unspecified.
    _raise_ap_status(int(status[0]) & AP_ST_NAN_CONF)
    present = n_labels > 0
    return p[present], r[present], ap[present], f1[present], np.flatnonzero(present).astype("int32")


def _gather_host(batches, T):
    """``compute()``'s compaction without its loop over images: the rows below each image's clamped count in (batch, image,
    detection) order, and the classes of the targets whose image lies in [0, B)."""
    tp, conf, pcls, tcls = [np.zeros((0, T), bool)], [np.zeros(0, F32)], [np.zeros(0, F32)], [np.zeros(0, F32)]
    for correct, conf_cls, count, tgt, _ in batches:
        B, max_det = correct.shape[0], correct.shape[1]
        keep = np.arange(max_det)[None, :] < np.clip(count.astype(np.int64), 0, max_det)[:, None]
        tp.append(correct[keep] != 0)
        conf.append(conf_cls[keep][:, 0])
        pcls.append(conf_cls[keep][:, 1])
        t0 = tgt[:, 0]
        tcls.append(tgt[(t0 >= 0) & (t0 < B) & (t0 == np.floor(t0)), 1])
    return np.concatenate(tp, 0), np.concatenate(conf, 0), np.concatenate(pcls, 0), np.concatenate(tcls, 0)


class DetectionEvaluator:
    """The evaler's statistics over a validation run.  ``update`` scores one batch on the device and keeps its padded
    ``correct`` / conf / class tensors and the target classes there, reading nothing back; ``compute`` reads everything back in
    ONE copy, compacts with ``count`` in image order and detection order (the layout of the reference's ``stats``) and returns
    ``summarize``'s result.  ``confusion=True`` adds a ``ConfusionMatrix(nc)`` (``self.confusion``) filled by the same launches.
    ``check=True``: ``compute`` raises ValueError naming the batch and image of any non-zero status word."""

    def __init__(self, nc, iouv=None, confusion=False, check=False):
        self.nc, self.iouv, self.check = int(nc), _iouv_host(iouv), bool(check)
        self.confusion = ConfusionMatrix(nc) if confusion else None
        self._batches = []

    def update(self, det, count, targets, img_shape, shapes):
        correct, _, n_labels, status = match_batch(det, count, targets, img_shape, shapes, self.iouv, self.confusion)
        targets = targets.to(det.device)
        self.add_batch(correct, det[:, :, 4:6], count.to(det.device), targets[:, 0:2], status)

    def compute(self):
        T = self.iouv.size
        if not self._batches:
            return summarize((np.zeros((0, T), bool), np.zeros(0, F32), np.zeros(0, F32), np.zeros(0, F32)), self.nc, 0)
        parts = [t for batch in self._batches for t in batch]
        flat = torch.cat([t.reshape(-1).view(torch.uint8) for t in parts]).cpu().numpy()       # the one read-back
        host, at = [], 0
        for t in parts:
            nbytes = t.numel() * t.element_size()
            host.append(flat[at:at + nbytes].view(torch.empty(0, dtype=t.dtype).numpy().dtype).reshape(tuple(t.shape)))
            at += nbytes
        tp, conf, pcls, tcls, seen = [], [], [], [], 0
        for i in range(0, len(host), 5):
            correct, conf_cls, count, tgt, status = host[i:i + 5]
            B, max_det = correct.shape[0], correct.shape[1]
            if self.check and status.any():
                b = int(np.flatnonzero(status)[0])
                what = ", ".join(text for bit, text in _STATUS_TEXT if int(status[b]) & bit)
                raise ValueError("batch %d, image %d: %s (status %d)" % (i // 5, b, what, int(status[b])))
            seen += B
            for b in range(B):
                n = int(min(max(count[b], 0), max_det))
                tp.append(correct[b, :n].astype(bool))
                conf.append(conf_cls[b, :n, 0])
                pcls.append(conf_cls[b, :n, 1])
                tcls.append(tgt[tgt[:, 0] == F32(b), 1])
        stats = (np.concatenate(tp, 0), np.concatenate(conf, 0), np.concatenate(pcls, 0), np.concatenate(tcls, 0))
        return summarize(stats, self.nc, seen)

    def add_batch(self, correct, conf_cls, count, targets, status):
        """Keeps one already scored batch: correct (B, max_det, T) uint8, conf_cls (B, max_det, 2) float32 (columns 4 and 5 of
        the detections), count (B,) int32, targets (n_t, 2) float32 (image, class), status (B,) int32 -- what ``update`` keeps
        of ``match_batch``'s launch, and the one place that says what a kept batch is (``update`` ends here).  All five on one
        device."""
        if not isinstance(correct, torch.Tensor) or correct.dim() != 3 or correct.shape[2] != self.iouv.size:
            raise ValueError("correct must be a (B, max_det, %d) tensor" % self.iouv.size)
        dev, B, max_det = correct.device, int(correct.shape[0]), int(correct.shape[1])
        conf_cls, targets = conf_cls.contiguous(), targets.contiguous()
        _lib.want(correct, "correct", torch.uint8, shape=(B, max_det, self.iouv.size), device=dev)
        _lib.want(conf_cls, "conf_cls", torch.float32, shape=(B, max_det, 2), device=dev)
        _lib.want(count, "count", torch.int32, shape=(B,), device=dev)
        _lib.want(targets, "targets", torch.float32, shape=(None, 2), device=dev)
        _lib.want(status, "status", torch.int32, shape=(B,), device=dev)
        if self._batches and self._batches[0][0].device != dev:
            raise ValueError("the evaluator's batches live on %s" % self._batches[0][0].device)
        self._batches.append((correct, conf_cls, count, targets, status))

    def compute_device(self):
        """``compute()`` with the compaction, the ordering and the AP on the batches' device (rules A1-A7): per batch two
        launches of evrep_det_ap_gather, then evrep_det_ap, then ONE read-back of the result arrays and the status words; the
        host works per batch, never per image or row.  Returns ``compute()``'s dict (tied confidences: in array order, the
        declared rule), or ``(0.0, 0.0)`` when no prediction is correct.  Batches on the CPU take the same route through
        ``ap_host``."""
        T = self.iouv.size
        if not self._batches:
            return 0.0, 0.0
        dev, seen = self._batches[0][0].device, sum(int(b[0].shape[0]) for b in self._batches)
        words = [b[4] for b in self._batches]
        if dev.type != "cuda":
            host = [[t.numpy() for t in b] for b in self._batches]
            result = ap_host(*_gather_host(host, T), self.nc)
            p, r, ap, f1, n_labels, _, any_correct, ap_status = result
            words = [b[4] for b in host]
        else:
            cap_n = sum(int(b[0].shape[0]) * int(b[0].shape[1]) for b in self._batches)
            cap_m = sum(int(b[3].shape[0]) for b in self._batches)
            tp = torch.empty((cap_n, T), dtype=torch.uint8, device=dev)
            conf, pcls = torch.empty(cap_n, dtype=torch.float32, device=dev), torch.empty(cap_n, dtype=torch.float32, device=dev)
            tcls = torch.empty(cap_m, dtype=torch.float32, device=dev)
            cursor = torch.zeros(2, dtype=torch.int64, device=dev)
            with torch.cuda.device(dev):
                for correct, conf_cls, count, tgt, _ in self._batches:
                    B, max_det, n_t = int(correct.shape[0]), int(correct.shape[1]), int(tgt.shape[0])
                    _lib.api().evrep_det_ap_gather(_lib.ptr(correct), _lib.ptr(conf_cls), _lib.ptr(count), B, max_det, T,
                                                   _lib.ptr(tgt) if n_t else None, n_t, _lib.ptr(tp), _lib.ptr(conf), _lib.ptr(pcls),
                                                   cap_n, _lib.ptr(tcls) if cap_m else None, cap_m, _lib.ptr(cursor), _lib.stream_ptr())
            out = ap_device(tp, conf, pcls, tcls, self.nc, counts=cursor)
            host = _read_once([out[0], out[1], out[2], out[3], out[4], out[6], out[7]] + words)     # the one read-back
            p, r, ap, f1, n_labels = host[:5]
            any_correct, ap_status, words = int(host[5][0]), int(host[6][0]), host[7:]
        if self.check:
            for i, status in enumerate(words):
                if status.any():
                    b = int(np.flatnonzero(status)[0])
                    what = ", ".join(text for bit, text in _STATUS_TEXT if int(status[b]) & bit)
                    raise ValueError("batch %d, image %d: %s (status %d)" % (i, b, what, int(status[b])))
            _raise_ap_status(ap_status)
        if not any_correct:
            return 0.0, 0.0
        present = n_labels > 0
        return _summary(p[present], r[present], ap[present], f1[present], np.flatnonzero(present).astype("int32"), n_labels, seen)
