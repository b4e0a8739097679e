"""The training targets on the device: label padding and the task-aligned assigner of the reference's loss.

``ev-YOLOv6/yolov6/models/losses/loss.py:73-111`` turns, once per training step, the batch's labels into a padded tensor on the
host (``ComputeLoss.preprocess``: ``.cpu().numpy().tolist()``, a Python loop over every label, back to the device) and then runs
``TaskAlignedAssigner.forward`` (``yolov6/assigners/tal_assigner.py``), which materialises a dozen ``(B, M, A)`` tensors and an
int64 one-hot of ``(B, M, 13, A)``.  Here ``assign_batch`` does both with no host read and no ``(B, M, A)`` array:
``evrep_det_targets_pad`` and ``evrep_tal_assign`` (csrc/evrep_assign.hip).  ``tal_host`` and ``preprocess_host`` are the same
rules in numpy: what the tests hold the kernels to bit for bit, and the route of CPU tensors.

The rules (include/evrep.h states them with the C entry points).  The reference's route is float64 -- ``preprocess`` builds its
tensor from Python floats -- but for ONE float32 quantity, the predicted box's own area; every statement is one operation of
that type.  ``max(a, b)`` is ``a > b ? a : b``, ``min`` likewise.

1. Padding.  A label row ``[img, cls, cx, cy, w, h]`` (float32) and the float32 ``width``, ``height`` are widened exactly;
   ``bx = cx * W``, ``by = cy * H``, ``bw = w * W``, ``bh = h * H``, ``x1 = bx - bw * 0.5``, ``y1 = by - bh * 0.5``, ``x2 = x1 + bw``,
   ``y2 = y1 + bh``.  Row m of image b is its m-th label in array order; padding rows ``[-1, 0, 0, 0, 0]`` come last.
2. A row is valid iff ``((x1 + y1) + x2) + y2 > 0`` (``mask_gt``) and its class lies in ``[0, nc)``.  A valid box with a class
   outside sets ``ST_BAD_CLASS`` and counts as padding (the reference raises or wraps).
3. ``in_gt = min(ax - x1, ay - y1, x2 - ax, y2 - ay) > 1e-9``: a centre on an edge is outside.
4. ``iou = ov / (((a1 + a2) - ov) + 1e-9)`` with ``a2`` the float32 area of the predicted box (``assigner_utils.py:73-93``).
5. ``al = score^alpha * iou^beta`` with integer exponents in 0..16 as repeated multiplication; ``key = al`` if ``in_gt`` and
   ``al > 0``, else ``+0``.
6. Per valid row the first ``topk`` anchors of the TOTAL order (key descending, anchor index ascending); a selected anchor is a
   candidate iff it is ``in_gt``.  ZERO KEYS are therefore chosen by lowest index, inside the box or not: the reference's
   ``torch.topk`` leaves them open, and an in-box anchor of IoU 0 becomes a positive or not at torch's choosing.
7. Per anchor with c candidate rows: c = 0 background (row 0's label and box, as the reference returns), c = 1 that row, c > 1
   the FIRST row of greatest IoU over ALL M rows, padding and non-candidates included (``select_highest_overlaps``).
8. ``target_scores`` is zero but at a foreground anchor's label: ``(al * pos_ov) / (pos_al + 1e-9)`` with ``pos_al`` / ``pos_ov`` the
   greatest metric / IoU over the anchors assigned to the row.
9. M = 0 is the reference's early return (labels ``num_classes``, the rest zero).  A non-finite value among an image's
   predictions or labels sets ``ST_NONFINITE`` and the image is written as if it had no valid row.

THE WARM-UP ASSIGNER.  While ``epoch_num < warmup_epoch`` the reference assigns with ``ATSSAssigner(9, num_classes)``
(``yolov6/assigners/atss_assigner.py``, loss.py:84-97), which needs no class scores: ``atss_assign_batch`` / ``ATSSAssigner`` here,
``evrep_atss_assign`` (csrc/evrep_atss.hip) behind them, ``atss_host`` the same rules in numpy.  Float64 statements as above:

A1. The anchor BOX is float32; ``area_a = fl32(fl32(ax2 - ax1) * fl32(ay2 - ay1))`` and the centre ``fl32(fl32(ax1 + ax2) / 2f)`` are
    float32 quantities, then widened.  Rows are valid as in rule 2.
A2. ``o = ov / max((area_g + area_a) - ov, 1e-6)`` with ``ov = max(min(x2, ax2) - max(x1, ax1), 0) * (y likewise)`` and the
    unclamped ``area_g``; ``d = sqrt(dx * dx + dy * dy)`` between the centres, ``(x1 + x2) / 2.0`` the row's.
A3. Per valid row every level gives the first ``topk`` of its anchors in the TOTAL order (d ascending, anchor index ascending);
    ``torch.topk`` leaves equal distances open.  A level with fewer than ``topk`` anchors is refused, as the reference fails on it.
A4. Over the ``n = levels * topk`` candidate values in the order (level, place): ``mean`` = their left-to-right sum / n, ``ss`` the
    left-to-right sum of ``(v - mean) * (v - mean)``, ``thr = mean + sqrt(ss / (n - 1))`` (n = 1: NaN, no positives).  torch adds in
    another order: the outcome differs from the reference's only where a candidate's ``o`` lies within rounding of ``thr``.
A5. A candidate is positive iff ``o > thr`` and its centre is ``in_gt`` (rule 3).  Per anchor with c positive rows: c = 0 background
    (label ``nc``, row 0's box), c = 1 that row, c > 1 the FIRST row of greatest ``o`` over ALL M rows.
A6. ``target_scores`` is zero but at a foreground anchor's label: ``fl32(iou)`` (rule 4, against the predicted box), or 1 without
    predicted boxes.  M = 0 and non-finite images are written as in rule 9 (a non-finite image: every anchor background).

Half-precision predictions are not mirrored.  The loss terms behind the assigners are ``detector_loss`` (``decode_boxes`` in
front of ``assign_batch`` / ``atss_assign_batch``, ``loss_batch`` behind them, ``ComputeLoss`` for all of it).
"""
import numpy as np
import torch

from . import _lib

F32, F64 = np.float32, np.float64
MAX_TOPK, MAX_LABELS, MAX_CLASSES, MAX_POWER = _lib.TAL_MAX_TOPK, _lib.TAL_MAX_LABELS, _lib.TAL_MAX_CLASSES, _lib.TAL_MAX_POWER
ATSS_MAX_TOPK, ATSS_MAX_LEVELS, ATSS_MAX_CANDIDATES = _lib.ATSS_MAX_TOPK, _lib.ATSS_MAX_LEVELS, _lib.ATSS_MAX_CANDIDATES
ST_LABEL_OVERFLOW, ST_BAD_CLASS, ST_NONFINITE = _lib.TAL_ST_LABEL_OVERFLOW, _lib.TAL_ST_BAD_CLASS, _lib.TAL_ST_NONFINITE
_STATUS_TEXT = ((ST_LABEL_OVERFLOW, "more labels than max_labels"), (ST_BAD_CLASS, "a class outside [0, num_classes)"),
                (ST_NONFINITE, "a non-finite prediction or label"))
EPS = 1e-9


def anchor_points(img_size, strides=(8, 16, 32), offset=0.5):
    """``generate_anchors``' anchor points and strides for a square (or ``(H, W)``) input: ``((A, 2) float32 [x, y] in pixels,
    (A, 1) float32)``, level after level, rows first -- 8400 points at 640."""
    h, w = (img_size, img_size) if np.isscalar(img_size) else img_size
    points, stride_rows = [], []
    for s in strides:
        nh, nw = int(h) // s, int(w) // s
        x = ((np.arange(nw, dtype=F32) + F32(offset)) * F32(s)).astype(F32)
        y = ((np.arange(nh, dtype=F32) + F32(offset)) * F32(s)).astype(F32)
        yy, xx = np.meshgrid(y, x, indexing="ij")
        points.append(np.stack([xx, yy], axis=-1).reshape(-1, 2))
        stride_rows.append(np.full((nh * nw, 1), s, F32))
    return np.concatenate(points, 0), np.concatenate(stride_rows, 0)


def _power(alpha, what):
    if float(alpha) != int(alpha) or not 0 <= int(alpha) <= MAX_POWER:
        raise NotImplementedError("%s = %r: integer exponents in 0..%d only" % (what, alpha, MAX_POWER))
    return int(alpha)


def _pow(x, n):
    """x^n by n - 1 multiplications, left to right; x^0 = 1."""
    if n == 0:
        return np.ones_like(x)
    r = x
    for _ in range(n - 1):
        r = r * x
    return r


def _max(a, b):
    return np.where(a > b, a, b)


def _min(a, b):
    return np.where(a < b, a, b)


# ------------------------------------------------------------------------------------------------------------ the host route
def preprocess_host(targets, batch_size, width, height, max_labels=None):
    """Rule 1 in numpy: targets (n_t, 6) float32 -> ``(gt (B, M, 5) float64, n_labels int32 (B,), status uint32 (B,))``.
    ``max_labels=None`` gives the reference's M, the greatest number of labels of an image."""
    t = np.ascontiguousarray(targets, dtype=F32).reshape(-1, 6)
    B = int(batch_size)
    rows = [np.flatnonzero(t[:, 0] == F32(b)) for b in range(B)]
    n_labels = np.array([len(r) for r in rows], np.int32)
    M = int(n_labels.max()) if max_labels is None else int(max_labels)
    W, H = F64(F32(width)), F64(F32(height))
    gt = np.zeros((B, M, 5), F64)
    gt[:, :, 0] = -1.0
    status = np.zeros(B, np.uint32)
    for b, r in enumerate(rows):
        if len(r) > M:
            status[b] |= ST_LABEL_OVERFLOW
            r = r[:M]
        v = t[r].astype(F64)
        bx, by, bw, bh = v[:, 2] * W, v[:, 3] * H, v[:, 4] * W, v[:, 5] * H
        x1, y1 = bx - bw * 0.5, by - bh * 0.5
        gt[b, :len(r)] = np.stack([v[:, 1], x1, y1, x1 + bw, y1 + bh], axis=1)
    return gt, n_labels, status


def _iou_host(box, pd):
    """Rule 4: (M, 4) float64 rows x (A, 4) float32 predictions -> (M, A) float64."""
    p = pd.astype(F64)
    x1, y1, x2, y2 = (box[:, k, None] for k in range(4))
    ix1, iy1 = _max(x1, p[None, :, 0]), _max(y1, p[None, :, 1])
    ix2, iy2 = _min(x2, p[None, :, 2]), _min(y2, p[None, :, 3])
    ov = _max(ix2 - ix1, 0.0) * _max(iy2 - iy1, 0.0)
    a1 = _max(x2 - x1, 0.0) * _max(y2 - y1, 0.0)
    w, h = pd[:, 2] - pd[:, 0], pd[:, 3] - pd[:, 1]                     # float32
    a2 = (np.where(w > 0, w, F32(0)) * np.where(h > 0, h, F32(0))).astype(F32).astype(F64)
    return ov / (((a1 + a2[None, :]) - ov) + EPS)


def _in_gt_host(box, anc):
    a = anc.astype(F64)
    ax, ay = a[None, :, 0], a[None, :, 1]
    d = _min(_min(ax - box[:, 0, None], ay - box[:, 1, None]), _min(box[:, 2, None] - ax, box[:, 3, None] - ay))
    return d > EPS


def tal_image_host(scores, pd, anc, gt, topk, nc, alpha, beta, details=None):
    """Rules 2-9 for one image: scores (A, nc) float32, pd (A, 4) float32, anc (A, 2) float32, gt (M, 5) float64 with M > 0 ->
    ``(labels int64 (A,), boxes float64 (A, 4), target_scores float64 (A, nc), fg bool (A,), status)``.  ``details``: a dict that
    receives ``key``, ``iou``, ``in_gt``, ``valid``, ``count`` (what the golden script checks its cases with)."""
    A, M = scores.shape[0], gt.shape[0]
    status = 0
    with np.errstate(all="ignore"):
        finite = np.isfinite(scores).all() and np.isfinite(pd).all() and np.isfinite(gt).all()
        if not finite:
            status |= ST_NONFINITE
        cls, box = gt[:, 0], gt[:, 1:5]
        in_class = (cls >= 0) & (cls < nc)
        lab = np.where(in_class, cls, 0.0).astype(np.int64)
        box_ok = ((box[:, 0] + box[:, 1]) + box[:, 2]) + box[:, 3] > 0
        if finite and (box_ok & ~in_class).any():
            status |= ST_BAD_CLASS
        valid = box_ok & in_class & finite
        iou = _iou_host(box, pd)
        sc = scores[:, lab].T.astype(F64)                               # (M, A)
        al = np.where(in_class[:, None], _pow(sc, alpha) * _pow(iou, beta), 0.0)
        in_gt = _in_gt_host(box, anc)
        key = np.where(in_gt & (al > 0), al, 0.0)
        cand = np.zeros((M, A), bool)
        for m in np.flatnonzero(valid):
            sel = np.argsort(-key[m], kind="stable")[:topk]
            cand[m, sel] = in_gt[m, sel]
        count = cand.sum(0)
        g = np.where(count == 1, np.argmax(cand, axis=0), 0)
        multi = count > 1
        if multi.any():
            g = np.where(multi, np.argmax(np.where(np.isnan(iou), -np.inf, iou), axis=0), g)
        fg = count > 0
        cols = np.arange(A)
        al_a, iou_a = np.where(fg, al[g, cols], 0.0), np.where(fg, iou[g, cols], 0.0)
        pos_al, pos_ov = np.zeros(M), np.zeros(M)
        for a in np.flatnonzero(fg):
            if al_a[a] > pos_al[g[a]]:
                pos_al[g[a]] = al_a[a]
            if iou_a[a] > pos_ov[g[a]]:
                pos_ov[g[a]] = iou_a[a]
        out = np.zeros((A, nc), F64)
        f = np.flatnonzero(fg)
        out[f, lab[g[f]]] = (al_a[f] * pos_ov[g[f]]) / (pos_al[g[f]] + EPS)
    if details is not None:
        details.update(key=key, iou=iou, in_gt=in_gt, valid=valid, count=count, al=al)
    return lab[g], box[g].copy(), out, fg, status


def tal_host(pd_scores, pd_bboxes, anc_points, gt, topk=13, num_classes=None, alpha=1, beta=6, out_dtype=np.float64):
    """The assigner in numpy for a batch: pd_scores (B, A, nc), pd_bboxes (B, A, 4), anc_points (A, 2) float32, gt (B, M, 5)
    float64 ``[cls, x1, y1, x2, y2]`` -> ``(target_labels int64 (B, A), target_bboxes (B, A, 4), target_scores (B, A, nc), fg bool
    (B, A), status uint32 (B,))``.  ``out_dtype`` float32 rounds the float64 values once."""
    s = np.ascontiguousarray(pd_scores, dtype=F32)
    p = np.ascontiguousarray(pd_bboxes, dtype=F32)
    anc = np.ascontiguousarray(anc_points, dtype=F32)
    gt = np.ascontiguousarray(gt, dtype=F64)
    B, A, nc = s.shape
    if num_classes is not None and int(num_classes) != nc:
        raise ValueError("pd_scores has %d classes, num_classes is %d" % (nc, num_classes))
    alpha, beta = _power(alpha, "alpha"), _power(beta, "beta")
    if not 1 <= int(topk) <= MAX_TOPK:
        raise ValueError("topk must be in 1..%d" % MAX_TOPK)
    M = gt.shape[1]
    labels = np.full((B, A), nc, np.int64)
    boxes, out = np.zeros((B, A, 4), F64), np.zeros((B, A, nc), F64)
    fg, status = np.zeros((B, A), bool), np.zeros(B, np.uint32)
    if M > 0:
        for b in range(B):
            labels[b], boxes[b], out[b], fg[b], status[b] = tal_image_host(s[b], p[b], anc, gt[b], int(topk), nc, alpha, beta)
    return labels, boxes.astype(out_dtype), out.astype(out_dtype), fg, status


# ---------------------------------------------------------------------------------------------------------- the device route
def _np_dtype(dtype):
    if dtype not in (torch.float64, torch.float32):
        raise ValueError("out_dtype must be torch.float64 (the reference's) or torch.float32")
    return F64 if dtype == torch.float64 else F32


def _count_labels(targets, batch_size):
    """The reference's M for a CPU targets tensor: counted on the host."""
    img = targets[:, 0].numpy() if targets.numel() else np.zeros(0, F32)
    return max([int((img == F32(b)).sum()) for b in range(int(batch_size))] + [0])


def _pad_device(targets, B, M, width, height):
    dev = targets.device
    if targets.dtype != torch.float32 or targets.dim() != 2 or targets.shape[1] != 6:
        raise ValueError("targets must be a float32 (n_t, 6) tensor")
    if not (1 <= B <= 65535 and 0 <= M <= MAX_LABELS):
        raise ValueError("1 <= batch_size <= 65535 and 0 <= max_labels <= %d" % MAX_LABELS)
    targets = targets.contiguous()
    n_t = int(targets.shape[0])
    gt = torch.empty((B, M, 5), dtype=torch.float64, device=dev)
    n_labels = torch.empty((B,), dtype=torch.int32, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.api().evrep_det_targets_pad(_lib.ptr(targets) if n_t else None, n_t, B, M, float(F32(width)), float(F32(height)),
                                         _lib.ptr(gt) if M else None, _lib.ptr(n_labels), _lib.ptr(status), _lib.stream_ptr())
    return gt, n_labels, status


def preprocess(targets, batch_size, width, height, max_labels=None, return_status=False):
    """``ComputeLoss.preprocess``: targets (n_t, 6) float32 ``[img, cls, cx, cy, w, h]`` -> the padded (B, M, 5) float64
    ``[cls, x1, y1, x2, y2]`` in pixels of a ``width`` x ``height`` image.  A CPU ``targets`` -- what ``DetectorFrontEnd.prepare``
    returns -- gives the reference's ``M = max labels per image``, counted on the host, and the result on the CPU through
    ``preprocess_host``.  A CUDA ``targets`` is padded by the kernel and needs ``max_labels`` (M cannot be read from the device
    without a wait).  ``return_status`` appends ``(n_labels, status)``."""
    B = int(batch_size)
    if not isinstance(targets, torch.Tensor):
        raise ValueError("targets must be a torch tensor")
    if targets.is_cuda:
        if max_labels is None:
            raise ValueError("a CUDA targets tensor needs max_labels: M cannot be read from the device without a wait")
        gt, n_labels, status = _pad_device(targets, B, int(max_labels), width, height)
    else:
        g, n, s = preprocess_host(targets.detach().float().numpy(), B, width, height, max_labels)
        gt, n_labels, status = torch.from_numpy(g), torch.from_numpy(n), torch.from_numpy(s.view(np.int32))
    return (gt, n_labels, status) if return_status else gt


def _targets_on(targets, B, dev, max_labels):
    """``(M, targets on dev)`` for either assigner: a CPU ``targets`` gives the reference's M, counted on the host, unless
    ``max_labels`` states it; a CUDA one needs ``max_labels``."""
    if not targets.is_cuda:
        return (_count_labels(targets.detach().float(), B) if max_labels is None else int(max_labels)), targets.to(dev)
    if max_labels is None:
        raise ValueError("a CUDA targets tensor needs max_labels: M cannot be read from the device without a wait")
    return int(max_labels), targets


def _shape_limits(B, A, nc, M):
    """The limits of ``evrep_tal_assign`` and ``evrep_atss_assign`` (ValueError)."""
    if not (1 <= B <= 65535 and 1 <= A <= _lib.TAL_MAX_ANCHORS and 1 <= nc <= MAX_CLASSES and A * nc < 2 ** 31 and 0 <= M <= MAX_LABELS):
        raise ValueError("the assigner takes 1 <= B <= 65535, 1 <= nc <= %d, A * nc < 2^31 and M <= %d" % (MAX_CLASSES, MAX_LABELS))


def _outputs(B, A, nc, boxes_dtype, scores_dtype, dev):
    """What an assigner's C entry writes: ``(labels, boxes, scores, fg uint8, status int32)``, uninitialised."""
    labels = torch.empty((B, A), dtype=torch.int64, device=dev)
    boxes = torch.empty((B, A, 4), dtype=boxes_dtype, device=dev)
    out = torch.empty((B, A, nc), dtype=scores_dtype, device=dev)
    fg = torch.empty((B, A), dtype=torch.uint8, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    return labels, boxes, out, fg, status


def _finish(outputs, st_pad, check):
    """The tail of ``assign_batch`` / ``atss_assign_batch``: the padding's status into the assigner's, ``check``, fg as bool."""
    labels, boxes, out, fg, st = outputs
    status = torch.bitwise_or(st, st_pad)
    if check:
        check_status(status)
    return labels, boxes, out, fg.bool(), status


def _assign_device(pd_scores, pd_bboxes, anc_points, gt, topk, alpha, beta, out_dtype):
    dev = pd_scores.device
    if pd_scores.dtype != torch.float32 or pd_bboxes.dtype != torch.float32:
        raise ValueError("predictions are %s / %s: the assigner takes float32, call .float() on them first" % (pd_scores.dtype, pd_bboxes.dtype))
    if pd_scores.dim() != 3 or pd_bboxes.dim() != 3:
        raise ValueError("pd_scores must be (B, A, nc) and pd_bboxes (B, A, 4)")
    B, A, nc = (int(v) for v in pd_scores.shape)
    M = int(gt.shape[1])
    _shape_limits(B, A, nc, M)
    if not 1 <= int(topk) <= MAX_TOPK:
        raise ValueError("topk must be in 1..%d" % MAX_TOPK)
    _np_dtype(out_dtype)
    pd_scores = pd_scores.detach().contiguous()
    pd_bboxes = _lib.want(pd_bboxes.detach().contiguous(), "pd_bboxes", torch.float32, shape=(B, A, 4), device=dev)
    anc = _lib.want(anc_points.detach().to(dev).float().contiguous(), "anc_points", torch.float32, shape=(A, 2), device=dev)
    gt = _lib.want(gt.detach().contiguous(), "gt", torch.float64, shape=(B, M, 5), device=dev)
    labels, boxes, out, fg, status = _outputs(B, A, nc, out_dtype, out_dtype, dev)
    with torch.cuda.device(dev):
        api = _lib.api()
        scratch = _lib.scratch(api.evrep_tal_workspace_bytes(B, M, A), dev)
        api.evrep_tal_assign(_lib.ptr(pd_scores), _lib.ptr(pd_bboxes), _lib.ptr(anc), _lib.ptr(gt) if M else None, B, M, A, nc,
                             int(topk), alpha, beta, _lib.TAL_F32_OUT if out_dtype == torch.float32 else 0, _lib.ptr(labels),
                             _lib.ptr(boxes), _lib.ptr(out), _lib.ptr(fg), _lib.ptr(status), _lib.ptr(scratch), _lib.stream_ptr())
    return labels, boxes, out, fg, status


def check_status(status):
    """ValueError naming the first image whose status word is not zero (one read-back)."""
    st = status.detach().cpu().numpy().astype(np.int64)
    if st.any():
        b = int(np.flatnonzero(st)[0])
        raise ValueError("image %d: %s (status %d)" % (b, ", ".join(text for bit, text in _STATUS_TEXT if st[b] & bit), st[b]))


def assign_batch(pd_scores, pd_bboxes, anc_points, targets, img_hw, num_classes, max_labels=None, out_dtype=torch.float64,
                 check=False, topk=13, alpha=1.0, beta=6.0):
    """loss.py:73-111 up to the assigner's return: pads ``targets`` (n_t, 6) to ``img_hw = (height, width)`` pixels and assigns,
    with no host read.  pd_scores (B, A, nc) and pd_bboxes (B, A, 4, xyxy in pixels) float32 on the device, anc_points (A, 2).
    Returns ``(target_labels int64 (B, A), target_bboxes (B, A, 4), target_scores (B, A, nc), fg_mask bool (B, A), status int32
    (B,))`` on the device.  A CPU ``targets`` gives the reference's M (counted on the host, one upload); a CUDA one needs
    ``max_labels``.  ``check=True`` reads the status back and raises ValueError naming the image of a non-zero word."""
    if not (isinstance(pd_scores, torch.Tensor) and pd_scores.is_cuda):
        raise ValueError("assign_batch: the predictions must be CUDA tensors (CPU tensors go through TaskAlignedAssigner / tal_host)")
    if int(pd_scores.shape[-1]) != int(num_classes):
        raise ValueError("pd_scores has %d classes, num_classes is %d" % (pd_scores.shape[-1], num_classes))
    alpha, beta = _power(alpha, "alpha"), _power(beta, "beta")
    B = int(pd_scores.shape[0])
    M, targets = _targets_on(targets, B, pd_scores.device, max_labels)
    gt, _, st_pad = _pad_device(targets, B, M, img_hw[1], img_hw[0])
    return _finish(_assign_device(pd_scores, pd_bboxes, anc_points, gt, topk, alpha, beta, out_dtype), st_pad, check)


class TaskAlignedAssigner(torch.nn.Module):
    """``yolov6.assigners.tal_assigner.TaskAlignedAssigner`` with its name, call signature and return tuple:
    ``forward(pd_scores, pd_bboxes, anc_points, gt_labels (B, M, 1), gt_bboxes (B, M, 4), mask_gt) -> (target_labels int64,
    target_bboxes, target_scores, fg_mask bool)``, the two float tensors in gt_bboxes' dtype.  CUDA inputs take the kernel, CPU
    inputs ``tal_host``.  ``mask_gt`` is recomputed from the boxes, as ``ComputeLoss`` computes it (rule 2).  The arithmetic is the
    reference's float64 route: float32 gt tensors (the reference's CPU fall-back) are widened and the result rounded to float32,
    which agrees with the reference's float32 run within tolerance only, not bit for bit.  ``eps`` other than 1e-9, non-integer
    exponents and non-float32 predictions are refused.  ``last_status`` holds the (B,) status words of the last call."""

    def __init__(self, topk=13, num_classes=80, alpha=1.0, beta=6.0, eps=1e-9):
        super().__init__()
        if eps != EPS:
            raise ValueError("eps = %r: the kernel and the host route are written for the reference's 1e-9" % (eps,))
        if not 1 <= int(topk) <= MAX_TOPK:
            raise ValueError("topk must be in 1..%d" % MAX_TOPK)
        self.topk, self.num_classes, self.bg_idx = int(topk), int(num_classes), int(num_classes)
        self.alpha, self.beta, self.eps = alpha, beta, eps
        self._alpha, self._beta = _power(alpha, "alpha"), _power(beta, "beta")
        self.last_status = None

    @torch.no_grad()
    def forward(self, pd_scores, pd_bboxes, anc_points, gt_labels, gt_bboxes, mask_gt=None):
        if pd_scores.dtype != torch.float32 or pd_bboxes.dtype != torch.float32:
            raise ValueError("predictions are %s / %s: the assigner takes float32, call .float() on them first" % (pd_scores.dtype, pd_bboxes.dtype))
        if int(pd_scores.shape[-1]) != self.num_classes:
            raise ValueError("pd_scores has %d classes, num_classes is %d" % (pd_scores.shape[-1], self.num_classes))
        if gt_bboxes.dtype not in (torch.float64, torch.float32):
            raise ValueError("gt_bboxes must be float64 (what preprocess returns) or float32")
        out_dtype = gt_bboxes.dtype
        B, M = int(gt_bboxes.shape[0]), int(gt_bboxes.shape[1])
        gt = torch.cat([gt_labels.reshape(B, M, 1).to(torch.float64), gt_bboxes.to(torch.float64)], dim=2)
        if pd_scores.is_cuda:
            labels, boxes, out, fg, status = _assign_device(pd_scores, pd_bboxes, anc_points, gt.to(pd_scores.device), self.topk,
                                                            self._alpha, self._beta, out_dtype)
            self.last_status = status
            return labels, boxes, out, fg.bool()
        labels, boxes, out, fg, status = tal_host(pd_scores.numpy(), pd_bboxes.numpy(), anc_points.float().numpy(), gt.numpy(), self.topk,
                                                  self.num_classes, self._alpha, self._beta, _np_dtype(out_dtype))
        self.last_status = torch.from_numpy(status.view(np.int32))
        return torch.from_numpy(labels), torch.from_numpy(boxes), torch.from_numpy(out), torch.from_numpy(fg)


# ------------------------------------------------------------------------------------------- the assigner of the warm-up epochs
def anchor_boxes(img_size, strides=(8, 16, 32), cell_size=5.0, offset=0.5):
    """``generate_anchors``' anchor boxes in training mode for a square (or ``(H, W)``) input: ``((A, 4) float32 xyxy in pixels,
    [anchors per level])``, level after level, rows first: squares of ``cell_size * stride`` about the anchor points."""
    h, w = (img_size, img_size) if np.isscalar(img_size) else img_size
    boxes, counts = [], []
    for s in strides:
        nh, nw = int(h) // s, int(w) // s
        x = ((np.arange(nw, dtype=F32) + F32(offset)) * F32(s)).astype(F32)
        y = ((np.arange(nh, dtype=F32) + F32(offset)) * F32(s)).astype(F32)
        yy, xx = np.meshgrid(y, x, indexing="ij")
        half = F32(cell_size * s * 0.5)
        boxes.append(np.stack([xx - half, yy - half, xx + half, yy + half], axis=-1).reshape(-1, 4).astype(F32))
        counts.append(nh * nw)
    return np.concatenate(boxes, 0), counts


def _levels(level_counts, A, topk):
    """The level counts as a list of ints, held to the limits of ``evrep_atss_assign`` (ValueError)."""
    counts = [int(n) for n in level_counts]
    topk = int(topk)
    if not 1 <= topk <= ATSS_MAX_TOPK:
        raise ValueError("topk must be in 1..%d" % ATSS_MAX_TOPK)
    if not 1 <= len(counts) <= ATSS_MAX_LEVELS or len(counts) * topk > ATSS_MAX_CANDIDATES:
        raise ValueError("%d levels with topk %d: 1..%d levels and at most %d candidates per label" %
                         (len(counts), topk, ATSS_MAX_LEVELS, ATSS_MAX_CANDIDATES))
    if min(counts) < topk:
        raise ValueError("a level of %d anchors is below topk = %d: the reference fails on such an input too" % (min(counts), topk))
    if sum(counts) != int(A):
        raise ValueError("the level counts %s add up to %d, there are %d anchors" % (counts, sum(counts), A))
    return counts


def _anchor_terms_host(anchors):
    """ATSS rule 1: the float32 area and centre of every anchor box, widened."""
    x1, y1, x2, y2 = (anchors[:, k] for k in range(4))
    area = ((x2 - x1).astype(F32) * (y2 - y1).astype(F32)).astype(F32).astype(F64)
    centre = np.stack([((x1 + x2).astype(F32) / F32(2)).astype(F32), ((y1 + y2).astype(F32) / F32(2)).astype(F32)], axis=1)
    return area, centre


def _overlap_host(box, anchors, area):
    """ATSS rule 3: (M, 4) float64 rows x (A, 4) float32 anchor boxes -> (M, A) float64."""
    a = anchors.astype(F64)
    x1, y1, x2, y2 = (box[:, k, None] for k in range(4))
    w = _max(_min(x2, a[None, :, 2]) - _max(x1, a[None, :, 0]), 0.0)
    h = _max(_min(y2, a[None, :, 3]) - _max(y1, a[None, :, 1]), 0.0)
    ov = w * h
    area_g = (x2 - x1) * (y2 - y1)
    return ov / _max((area_g + area[None, :]) - ov, 1e-6)


def atss_image_host(anchors, level_counts, gt, pd, topk, nc, details=None):
    """ATSS rules 1-10 for one image: anchors (A, 4) float32, gt (M, 5) float64 with M > 0, pd (A, 4) float32 or None ->
    ``(labels int64 (A,), boxes float64 (A, 4), target_scores float64 (A, nc) holding float32 values, fg bool (A,), status)``.
    ``details``: a dict that receives ``overlap``, ``distance``, ``valid``, ``candidates`` (row -> anchor indices in the order of rule
    6), ``thr`` (per row, NaN where not valid), ``positive`` and ``count`` (what the golden script checks its cases with)."""
    A, M = anchors.shape[0], gt.shape[0]
    counts = _levels(level_counts, A, topk)
    status = 0
    with np.errstate(all="ignore"):
        finite = bool(np.isfinite(gt).all() and (pd is None or np.isfinite(pd).all()))
        if not finite:
            status |= ST_NONFINITE
        cls, box = gt[:, 0], gt[:, 1:5]
        in_class = (cls >= 0) & (cls < nc)
        lab = np.where(in_class, cls, 0.0).astype(np.int64)
        box_ok = ((box[:, 0] + box[:, 1]) + box[:, 2]) + box[:, 3] > 0
        if finite and (box_ok & ~in_class).any():
            status |= ST_BAD_CLASS
        valid = box_ok & in_class & finite
        area, centre = _anchor_terms_host(anchors)
        o = _overlap_host(box, anchors, area)
        c64 = centre.astype(F64)
        dx = (box[:, 0, None] + box[:, 2, None]) / 2.0 - c64[None, :, 0]
        dy = (box[:, 1, None] + box[:, 3, None]) / 2.0 - c64[None, :, 1]
        d = np.sqrt(dx * dx + dy * dy)
        in_gt = _in_gt_host(box, centre)
        pos = np.zeros((M, A), bool)
        cands, thrs = {}, np.full(M, np.nan)
        n = len(counts) * topk
        for m in np.flatnonzero(valid):
            sel, s0 = [], 0
            for n_l in counts:
                sel.append(np.argsort(d[m, s0:s0 + n_l], kind="stable")[:topk] + s0)
                s0 += n_l
            sel = np.concatenate(sel)
            v = o[m, sel]
            total = F64(0.0)
            for x in v:
                total = total + x
            mean = total / F64(n)
            ss = F64(0.0)
            for x in v:
                ss = ss + (x - mean) * (x - mean)
            thr = mean + np.sqrt(ss / F64(n - 1))
            pos[m, sel] = (v > thr) & in_gt[m, sel]
            cands[int(m)], thrs[m] = sel, thr
        count = pos.sum(0)
        g = np.where(count == 1, np.argmax(pos, axis=0), 0)
        multi = count > 1
        if multi.any():
            g = np.where(multi, np.argmax(o, axis=0), g)
        fg = count > 0
        cols = np.arange(A)
        val = np.ones(A) if pd is None else _iou_host(box, pd)[g, cols].astype(F32).astype(F64)
        out = np.zeros((A, nc), F64)
        f = np.flatnonzero(fg)
        out[f, lab[g[f]]] = val[f]
    if details is not None:
        details.update(overlap=o, distance=d, valid=valid, candidates=cands, thr=thrs, positive=pos, count=count, in_gt=in_gt)
    return np.where(fg, lab[g], nc), box[g].copy(), out, fg, status


def atss_host(anchors, level_counts, gt, pd_bboxes=None, topk=9, num_classes=80, boxes_dtype=np.float64, scores_dtype=np.float32):
    """The ATSS assigner in numpy for a batch: anchors (A, 4) float32, level_counts a list of anchors per level, gt (B, M, 5)
    float64 ``[cls, x1, y1, x2, y2]``, pd_bboxes (B, A, 4) float32 or None -> ``(target_labels int64 (B, A), target_bboxes (B, A, 4),
    target_scores (B, A, nc), fg bool (B, A), status uint32 (B,))``.  The defaults are the reference's dtypes: float64 boxes, float32
    scores (the score values are float32 ones: either width holds them exactly)."""
    anchors = np.ascontiguousarray(anchors, dtype=F32).reshape(-1, 4)
    gt = np.ascontiguousarray(gt, dtype=F64)
    pd = None if pd_bboxes is None else np.ascontiguousarray(pd_bboxes, dtype=F32)
    A, nc, B, M = anchors.shape[0], int(num_classes), gt.shape[0], gt.shape[1]
    counts = _levels(level_counts, A, topk)
    if pd is not None and pd.shape != (B, A, 4):
        raise ValueError("pd_bboxes must be (B, A, 4) = (%d, %d, 4)" % (B, A))
    labels = np.full((B, A), nc, np.int64)
    boxes, out = np.zeros((B, A, 4), F64), np.zeros((B, A, nc), F64)
    fg, status = np.zeros((B, A), bool), np.zeros(B, np.uint32)
    if M > 0:
        for b in range(B):
            labels[b], boxes[b], out[b], fg[b], status[b] = atss_image_host(anchors, counts, gt[b], None if pd is None else pd[b],
                                                                            int(topk), nc)
    return labels, boxes.astype(boxes_dtype), out.astype(scores_dtype), fg, status


def _atss_device(anchors, level_counts, gt, pd_bboxes, nc, topk, boxes_dtype, scores_dtype):
    """The C entry on CUDA tensors: ``(labels, boxes, scores, fg uint8, status int32)``."""
    dev = gt.device
    if anchors.dtype != torch.float32 or anchors.dim() != 2 or anchors.shape[1] != 4:
        raise ValueError("the anchor boxes must be a float32 (A, 4) tensor, got %s %s" % (anchors.dtype, tuple(anchors.shape)))
    if pd_bboxes is not None and pd_bboxes.dtype != torch.float32:
        raise ValueError("pd_bboxes is %s: the assigner takes float32, call .float() on it first" % (pd_bboxes.dtype,))
    A, nc, topk = int(anchors.shape[0]), int(nc), int(topk)
    B, M = int(gt.shape[0]), int(gt.shape[1])
    counts = _levels(level_counts, A, topk)
    _shape_limits(B, A, nc, M)
    _np_dtype(boxes_dtype)
    _np_dtype(scores_dtype)
    anc = _lib.want(anchors.detach().to(dev).contiguous(), "anchors", torch.float32, shape=(A, 4), device=dev)
    gt = _lib.want(gt.detach().contiguous(), "gt", torch.float64, shape=(B, M, 5), device=dev)
    if pd_bboxes is not None:
        pd_bboxes = _lib.want(pd_bboxes.detach().contiguous(), "pd_bboxes", torch.float32, shape=(B, A, 4), device=dev)
    labels, boxes, out, fg, status = _outputs(B, A, nc, boxes_dtype, scores_dtype, dev)
    flags = (_lib.ATSS_F32_BOXES if boxes_dtype == torch.float32 else 0) | (_lib.ATSS_F32_SCORES if scores_dtype == torch.float32 else 0)
    with torch.cuda.device(dev):
        api = _lib.api()
        scratch = _lib.scratch(api.evrep_atss_workspace_bytes(B, M, A), dev)
        api.evrep_atss_assign(_lib.ptr(anc), _lib.int32_array(counts), len(counts), _lib.ptr(gt) if M else None,
                              None if pd_bboxes is None else _lib.ptr(pd_bboxes), B, M, A, nc, topk, flags, _lib.ptr(labels),
                              _lib.ptr(boxes), _lib.ptr(out), _lib.ptr(fg), _lib.ptr(status), _lib.ptr(scratch), _lib.stream_ptr())
    return labels, boxes, out, fg, status


def atss_assign_batch(anchors, n_anchors_list, pred_bboxes_px, targets, img_hw, num_classes, max_labels=None,
                      out_dtype=torch.float64, check=False, topk=9):
    """loss.py:73-97 up to the warm-up assigner's return: pads ``targets`` (n_t, 6) to ``img_hw = (height, width)`` pixels and
    assigns with the ATSS rules, with no host read.  anchors (A, 4) float32 anchor boxes and n_anchors_list their numbers per level
    (what ``generate_anchors`` returns in training mode), pred_bboxes_px (B, A, 4, xyxy in pixels) float32 on the device.  Returns
    ``(target_labels int64 (B, A), target_bboxes (B, A, 4), target_scores (B, A, nc), fg_mask bool (B, A), status int32 (B,))`` on the
    device, both float tensors in ``out_dtype`` (what ``loss_batch`` takes).  ``targets``, ``max_labels`` and ``check`` are as in
    ``assign_batch``."""
    if not (isinstance(pred_bboxes_px, torch.Tensor) and pred_bboxes_px.is_cuda and pred_bboxes_px.dim() == 3):
        raise ValueError("atss_assign_batch: pred_bboxes_px must be a CUDA (B, A, 4) tensor (CPU tensors, or no predicted boxes, go "
                         "through ATSSAssigner / atss_host)")
    B = int(pred_bboxes_px.shape[0])
    M, targets = _targets_on(targets, B, pred_bboxes_px.device, max_labels)
    _levels(n_anchors_list, anchors.shape[0], topk)                     # (refused before the padding launch)
    gt, _, st_pad = _pad_device(targets, B, M, img_hw[1], img_hw[0])
    return _finish(_atss_device(anchors, n_anchors_list, gt, pred_bboxes_px, num_classes, topk, out_dtype, out_dtype), st_pad, check)


class ATSSAssigner(torch.nn.Module):
    """``yolov6.assigners.atss_assigner.ATSSAssigner`` with its name, call signature and return tuple:
    ``forward(anc_bboxes (A, 4), n_level_bboxes, gt_labels (B, M, 1), gt_bboxes (B, M, 4), mask_gt, pd_bboxes (B, A, 4) or None) ->
    (target_labels int64, target_bboxes in gt_bboxes' dtype, target_scores float32, fg_mask bool)``.  CUDA inputs take the kernel,
    CPU inputs ``atss_host``.  ``mask_gt`` is recomputed from the boxes, as ``ComputeLoss`` computes it.  The arithmetic is the
    reference's float64 route (float32 gt tensors are widened and the boxes rounded back).  A level with fewer than ``topk``
    anchors is refused (ValueError): the reference itself fails there.  ``last_status`` holds the (B,) status words of the last
    call."""

    def __init__(self, topk=9, num_classes=80):
        super().__init__()
        if not 1 <= int(topk) <= ATSS_MAX_TOPK:
            raise ValueError("topk must be in 1..%d" % ATSS_MAX_TOPK)
        self.topk, self.num_classes, self.bg_idx = int(topk), int(num_classes), int(num_classes)
        self.last_status = None

    @torch.no_grad()
    def forward(self, anc_bboxes, n_level_bboxes, gt_labels, gt_bboxes, mask_gt=None, pd_bboxes=None):
        if gt_bboxes.dtype not in (torch.float64, torch.float32):
            raise ValueError("gt_bboxes must be float64 (what preprocess returns) or float32")
        if anc_bboxes.dtype != torch.float32 or (pd_bboxes is not None and pd_bboxes.dtype != torch.float32):
            raise ValueError("anchor boxes are %s, predicted boxes %s: the assigner takes float32, call .float() on them first" %
                             (anc_bboxes.dtype, None if pd_bboxes is None else pd_bboxes.dtype))
        out_dtype = gt_bboxes.dtype
        B, M = int(gt_bboxes.shape[0]), int(gt_bboxes.shape[1])
        gt = torch.cat([gt_labels.reshape(B, M, 1).to(torch.float64), gt_bboxes.to(torch.float64)], dim=2)
        if gt_bboxes.is_cuda:
            dev = gt_bboxes.device
            labels, boxes, out, fg, status = _atss_device(anc_bboxes.to(dev), n_level_bboxes, gt, None if pd_bboxes is None else
                                                          pd_bboxes.to(dev), self.num_classes, self.topk, out_dtype, torch.float32)
            self.last_status = status
            return labels, boxes, out, fg.bool()
        labels, boxes, out, fg, status = atss_host(anc_bboxes.numpy(), n_level_bboxes, gt.numpy(), None if pd_bboxes is None else
                                                   pd_bboxes.detach().numpy(), self.topk, self.num_classes, _np_dtype(out_dtype), F32)
        self.last_status = torch.from_numpy(status.view(np.int32))
        return torch.from_numpy(labels), torch.from_numpy(boxes), torch.from_numpy(out), torch.from_numpy(fg)
