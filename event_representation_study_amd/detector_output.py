"""The other end of the detector route: the head's ``(B, N, 5 + C)`` output -> detections, on the device.

``non_max_suppression`` has the name, the signature and the return value of the reference's
``ev-YOLOv6/yolov6/utils/nms.py:non_max_suppression`` (a list of B ``(n_b, 6)`` float32 tensors ``[x1, y1, x2, y2, conf, cls]``
on the input's device), which the reference calls once per batch from ``core/evaler.py`` and ``core/inferer.py``.  For a CUDA
tensor it is ONE launch of ``evrep_nms`` (csrc/evrep_nms.hip: one workgroup per image) and one read-back of the B counts;
``nms_batch`` is the same launch without the read-back, its padded results staying on the device.  A CPU tensor takes
``nms_host``, the same rules in numpy float32, which the tests hold the kernel to bit for bit.

The rules (include/evrep.h states them with the C entry point):

1. ``ct = float32(conf_thres)``; a box is a candidate iff ``obj > ct`` and ``max(cls) > ct`` (a NaN fails both).
2. ``conf_c = cls_c * obj``; corners ``cx -/+ w / 2``, ``cy -/+ h / 2``.
3. ``multi_label`` and C > 1: a row per (box, class) with ``conf_c > ct``, in (box, class) order; otherwise a row per candidate
   with the FIRST maximum of ``conf_c``, kept iff it is above ``ct``.  ``classes``: a row survives iff its class is listed.
4. More than ``max_nms`` rows (30000 in the reference, a parameter here): the ``max_nms`` of greatest ``conf``.  The reference's
   ``argsort(descending=True)`` is not stable and leaves ties at the cut (and the order of equal scores inside it) open; here
   the lower row goes first.
5. Order: ``conf`` descending, equal scores by row ascending -- torchvision's stable sort.
6. Boxes offset by ``cls * 4096`` (``cls * 0`` with ``agnostic``) IN FLOAT32 -- the addition rounds the corners, and the IoU is
   formed on the rounded ones -- then torchvision's greedy pass: a row is kept iff no earlier kept row has
   ``double(ovr) > iou_thres``.
7. The first ``max_det`` kept rows, un-offset.

Rules 1-5 and 7 are pinned to the reference's own torch statements by tests/golden/detector_output.npz.  Rule 6 is
torchvision's ``nms_kernel_impl`` RESTATED (``torchvision_nms_host``): torchvision is absent here, so that part is parity
unpinned, as the ``cv2`` functions behind detector_input.py are.

Not mirrored: the reference's 10 s ``time_limit`` break; half-precision input (the reference computes in half; a CUDA tensor
that is not float32 is refused here: call ``.float()``); the reference's empty entries all being ONE tensor object.
"""
import ctypes

import numpy as np
import torch

from . import _lib

MAX_WH = 4096          # the reference's max_wh: the class offset
MAX_NMS = 30000        # the reference's max_nms
F32 = np.float32


def xywh2xyxy(x):
    """[cx, cy, w, h] -> [x1, y1, x2, y2] for an (n, 4) tensor or array, in its dtype (the reference's function of this name)."""
    y = x.clone() if isinstance(x, torch.Tensor) else np.copy(x)
    half_w, half_h = x[:, 2] / 2, x[:, 3] / 2
    y[:, 0] = x[:, 0] - half_w
    y[:, 1] = x[:, 1] - half_h
    y[:, 2] = x[:, 0] + half_w
    y[:, 3] = x[:, 1] + half_h
    return y


def _check_thresholds(conf_thres, iou_thres):
    assert 0 <= conf_thres <= 1, f"conf_thresh must be in 0.0 to 1.0, however {conf_thres} is provided."
    assert 0 <= iou_thres <= 1, f"iou_thres must be in 0.0 to 1.0, however {iou_thres} is provided."


def torchvision_nms_host(boxes, scores, iou_threshold):
    """torchvision's CPU kernel ``nms_kernel_impl`` restated for float32 arrays: boxes (n, 4) [x1, y1, x2, y2], scores (n).
    Returns the kept indices (int64) in the order they were kept.  Every statement is its own float32 rounding; std::max /
    std::min are the comparisons they are; the test is ``double(ovr) > iou_threshold``, strict, and a NaN suppresses nothing."""
    boxes = np.ascontiguousarray(boxes, dtype=F32).reshape(-1, 4)
    scores = np.ascontiguousarray(scores, dtype=F32).reshape(-1)
    n = scores.shape[0]
    x1, y1, x2, y2 = (boxes[:, k] for k in range(4))
    areas = (x2 - x1) * (y2 - y1)
    order = np.argsort(-scores, kind="stable")          # scores.sort(stable=True, descending=True)
    suppressed = np.zeros(n, dtype=bool)
    thr = float(iou_threshold)
    zero = F32(0)
    keep = []
    with np.errstate(all="ignore"):
        for _i in range(n):
            i = order[_i]
            if suppressed[i]:
                continue
            keep.append(i)
            js = order[_i + 1:]
            xx1 = np.where(x1[i] < x1[js], x1[js], x1[i])           # std::max(ix1, x1[j])
            yy1 = np.where(y1[i] < y1[js], y1[js], y1[i])
            xx2 = np.where(x2[js] < x2[i], x2[js], x2[i])           # std::min(ix2, x2[j])
            yy2 = np.where(y2[js] < y2[i], y2[js], y2[i])
            dw, dh = xx2 - xx1, yy2 - yy1
            w = np.where(zero < dw, dw, zero)                       # std::max(0, d)
            h = np.where(zero < dh, dh, zero)
            inter = w * h
            ovr = inter / ((areas[i] + areas[js]) - inter)
            suppressed[js] |= ovr.astype(np.float64) > thr
    return np.asarray(keep, dtype=np.int64)


def _rows_host(x, ct, classes, multi_label):
    """Rules 1-3 for one image: (rows (n, 6) float32 [x1, y1, x2, y2, conf, cls], row numbers (n) int64 = i * C + c)."""
    C = x.shape[1] - 5
    with np.errstate(all="ignore"):
        cand = (x[:, 4] > ct) & (np.max(x[:, 5:], axis=1) > ct)       # (np.max propagates a NaN, as torch.max does)
        idx = np.flatnonzero(cand)
        x = x[idx]
        conf = x[:, 5:] * x[:, 4:5]
        box = xywh2xyxy(x[:, :4])
        if multi_label and C > 1:
            bi, ci = np.nonzero(conf > ct)
        else:
            ci = np.argmax(conf, axis=1) if idx.size else np.zeros(0, np.int64)     # the first maximum (a NaN first)
            bi = np.arange(idx.size)
            sel = conf[bi, ci] > ct
            bi, ci = bi[sel], ci[sel]
    if classes is not None:
        sel = np.isin(ci, np.asarray(list(classes), dtype=np.int64))
        bi, ci = bi[sel], ci[sel]
    rows = np.concatenate([box[bi], conf[bi, ci][:, None], ci.astype(F32)[:, None]], axis=1).astype(F32)
    return rows, idx[bi].astype(np.int64) * C + ci.astype(np.int64)


def nms_host(prediction, conf_thres=0.25, iou_thres=0.45, classes=None, agnostic=False, multi_label=False, max_det=300,
             max_nms=MAX_NMS, max_wh=MAX_WH):
    """The rules of this module in numpy float32: prediction (B, N, 5 + C) -> a list of B (n_b, 6) float32 arrays.  What the
    kernel is held to, and the CPU route of ``non_max_suppression``.  max_wh: the class offset (4096 in the reference)."""
    _check_thresholds(conf_thres, iou_thres)
    pred = np.ascontiguousarray(prediction, dtype=F32)
    if pred.ndim != 3 or pred.shape[2] < 6:
        raise ValueError("prediction must be (B, N, 5 + C) with C >= 1")
    ct = F32(conf_thres)
    out = []
    for x in pred:
        rows, number = _rows_host(x, ct, classes, multi_label)
        if rows.shape[0] > max_nms:
            # conf descending, the lower row first among equals: number ascends, so a stable sort says it
            rows = rows[np.argsort(-rows[:, 4], kind="stable")[:max_nms]]
        with np.errstate(all="ignore"):
            offset = rows[:, 5:6] * F32(0 if agnostic else max_wh)
            boxes = rows[:, :4] + offset
        keep = torchvision_nms_host(boxes, rows[:, 4], iou_thres)[:max_det]
        out.append(rows[keep])
    return out


def nms_scratch_total(B, N, C, multi_label):
    """The `total` of evrep_dense_rank_scratch_bytes(B, total) that sizes evrep_nms's scratch: five arrays of B * R uint32, R
    the rows an image has when every box is a candidate under every class it can be."""
    R = N * C if (multi_label and C > 1) else N
    return 5 * ((B * R + 3) // 4)


def _launch(prediction, conf_thres, iou_thres, classes, agnostic, multi_label, max_det, max_nms):
    _check_thresholds(conf_thres, iou_thres)
    if not (isinstance(prediction, torch.Tensor) and prediction.is_cuda):
        raise ValueError("nms_batch: prediction must be a CUDA tensor (a CPU tensor goes through non_max_suppression / nms_host)")
    if prediction.dtype != torch.float32:
        raise ValueError("prediction is %s: the device route computes in float32, call .float() on it first" % prediction.dtype)
    if prediction.dim() != 3 or prediction.shape[2] < 6:
        raise ValueError("prediction must be (B, N, 5 + C) with C >= 1")
    B, N, C = int(prediction.shape[0]), int(prediction.shape[1]), int(prediction.shape[2]) - 5
    max_det, max_nms = int(max_det), int(max_nms)
    if not 1 <= max_det <= _lib.NMS_MAX_DET:
        raise ValueError("max_det must be in 1..%d on the device" % _lib.NMS_MAX_DET)
    if max_nms < 1:
        raise ValueError("max_nms must be at least 1")
    if C > _lib.NMS_MAX_CLASSES or N * C > _lib.NMS_MAX_ROWS or B > 65535:
        raise ValueError("nms_batch: B <= 65535, C <= %d and N * C <= %d" % (_lib.NMS_MAX_CLASSES, _lib.NMS_MAX_ROWS))
    dev = prediction.device
    det = torch.empty((B, max_det, 6), dtype=torch.float32, device=dev)
    count = torch.empty((B,), dtype=torch.int32, device=dev)
    if B == 0 or N == 0:
        return det.zero_(), count.zero_()
    pred = prediction.contiguous()
    api = _lib.api()
    nbytes = int(api.evrep_dense_rank_scratch_bytes(B, nms_scratch_total(B, N, C, multi_label)))
    if nbytes == 0:
        raise ValueError("nms_batch: the batch is too large for one call")
    sc = _lib.scratch(nbytes, dev)
    if classes is None:
        cls_arr, n_cls = None, -1
    else:
        listed = [int(c) for c in classes if -2 ** 31 <= int(c) < 2 ** 31]
        cls_arr, n_cls = _lib.int32_array(listed or [0]), len(listed)
    flags = (_lib.NMS_MULTI_LABEL if multi_label else 0) | (_lib.NMS_AGNOSTIC if agnostic else 0)
    with torch.cuda.device(dev):
        api.evrep_nms(_lib.ptr(pred), B, N, C, float(F32(conf_thres)), float(iou_thres), flags, cls_arr, n_cls, max_nms, max_det,
                      _lib.ptr(det), _lib.ptr(count), _lib.ptr(sc), _lib.stream_ptr())
    return det, count


def nms_batch(prediction, conf_thres=0.25, iou_thres=0.45, classes=None, agnostic=False, multi_label=False, max_det=300,
              max_nms=MAX_NMS):
    """prediction (B, N, 5 + C) float32 CUDA -> (det (B, max_det, 6) float32, count (B,) int32), both on the device: det[b, :count[b]]
    are image b's detections, the rows behind them are zero.  One launch, no host read, no wait; max_det <= 1024.  May be
    captured into a graph (the scratch is then the capture's allocation)."""
    return _launch(prediction, conf_thres, iou_thres, classes, agnostic, multi_label, max_det, max_nms)


def non_max_suppression(prediction, conf_thres=0.25, iou_thres=0.45, classes=None, agnostic=False, multi_label=False, max_det=300):
    """The reference's non_max_suppression: a list of B (n_b, 6) float32 tensors [x1, y1, x2, y2, conf, cls] on the input's
    device.  CUDA float32 input: nms_batch and one read-back of the counts; CPU input: nms_host.  See the module's text for
    the rules and for what is not mirrored."""
    _check_thresholds(conf_thres, iou_thres)
    if isinstance(prediction, torch.Tensor) and prediction.is_cuda:
        det, count = _launch(prediction, conf_thres, iou_thres, classes, agnostic, multi_label, max_det, MAX_NMS)
        return [det[b, :n] for b, n in enumerate(count.tolist())]
    pred = prediction.detach().float().numpy() if isinstance(prediction, torch.Tensor) else np.asarray(prediction, dtype=F32)
    return [torch.from_numpy(np.ascontiguousarray(r)) for r in
            nms_host(pred, conf_thres, iou_thres, classes, agnostic, multi_label, max_det)]


def scale_coords_batch(det, count, img_shape, shapes):
    """The evaler's scale_coords (core/evaler.py:512-543, ratio_pad given, scale_exact=False) for the padded batch of
    nms_batch: det (B, max_det, 6), count (B,), shapes the list ``DetectorFrontEnd.prepare`` returned, one
    ``((h0, w0), ((gain_y, gain_x), (pad_x, pad_y)))`` per image.  Returns a new tensor whose first four columns are in the
    source frame -- subtract the pad, divide by gain[0], clamp to the frame, in the reference's order -- and whose rows at or
    beyond count[b] stay 0.  Plain torch statements, no host read.  img_shape (the letterboxed size) is not needed once the
    ratio and pad are given; it is taken for the reference's argument order."""
    B = det.shape[0]
    if len(shapes) != B:
        raise ValueError("scale_coords_batch: %d shapes for %d images" % (len(shapes), B))
    host = torch.tensor([[ratio_pad[1][0], ratio_pad[1][1], ratio_pad[0][0], w0, h0] for (h0, w0), ratio_pad in shapes],
                        dtype=torch.float64).to(torch.float32).reshape(B, 5, 1)
    t = host.to(det.device)
    pad_x, pad_y, gain, w0, h0 = (t[:, k] for k in range(5))
    out = det.clone()
    xs, ys = out[:, :, 0:4:2], out[:, :, 1:4:2]
    xs.sub_(pad_x[:, :, None]).div_(gain[:, :, None])
    ys.sub_(pad_y[:, :, None]).div_(gain[:, :, None])
    zero = torch.zeros((), dtype=out.dtype, device=out.device)
    xs.copy_(torch.minimum(torch.maximum(xs, zero), w0[:, :, None]))
    ys.copy_(torch.minimum(torch.maximum(ys, zero), h0[:, :, None]))
    live = torch.arange(det.shape[1], device=det.device)[None, :] < count.to(det.device)[:, None]
    return torch.where(live[:, :, None], out, torch.zeros_like(out))
