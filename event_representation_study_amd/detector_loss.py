"""The loss terms on the device: what the reference's ``ComputeLoss.__call__`` does behind the assigner, forward and backward.

``ev-YOLOv6/yolov6/models/losses/loss.py:176-217`` turns the assigner's targets into three scalars with ``F.one_hot`` (an int64
``(B, A, nc + 1)`` tensor), three ``masked_select`` compactions, two more softmaxes for the cross-entropies, ``IOUloss`` as some
forty elementwise launches and two reads of the device (``target_scores_sum > 1``, ``num_pos > 0``); autograd then replays all
of it backwards.  Here ``loss_batch`` computes the three terms AND their gradients with respect to ``pred_scores`` and
``pred_distri`` in four launches (``evrep_detloss``, csrc/evrep_detloss.hip) with no host read; ``decode_boxes`` is
``bbox_decode`` (loss.py:238-244) in one launch, in front of ``detector_assign.assign_batch``.  ``loss_host`` is the same rules
in numpy float64: the oracle of the kernel and the route of CPU tensors.  ``ComputeLoss`` strings them together behind the
reference's constructor and call signature.

The rules (include/evrep.h states them with ``evrep_detloss``).  Every statement is one float64 operation; float32 inputs are
widened exactly; ``max(a, b)`` is ``a > b ? a : b``.  R = ``reg_max``, K = R + 1, z = ``pred_distri``, p = ``pred_scores`` (after the
sigmoid, as the head returns them in training).

1. Decode.  ``aps = fl32(anc / stride)``; per side: ``m = max_k z``, ``e_k = exp(z_k - m)``, Z = the e_k added left to right,
   ``pr_k = e_k / Z``, d = the ``pr_k * k`` added left to right (without DFL, d = z); ``box = [ax - d_l, ay - d_t, ax + d_r, ay + d_b]``.
2. Sums.  ``w[b, a]`` = the row of ``target_scores`` added left to right; ``tss`` = all of them; ``norm = tss > 1 ? tss : 1``.
3. Class term (VarifocalLoss).  ``lab = fg && label == c``; ``wt = lab ? q : (0.75 * p) * p``;
   ``bce = -(q * max(log p, -100) + (1 - q) * max(log(1 - p), -100))``; ``loss_cls = sum(bce * wt) / norm``.
4. Box term (IOUloss xyxy, giou, eps = 1e-10) per foreground anchor against ``tb = target_bboxes / stride``;
   ``loss_iou = sum((1 - giou) * w) / norm``.
5. DFL term per foreground anchor and side: ``t = clip(distance, 0, R - 0.01)``, ``tl = long(t)``, ``wl = (tl + 1) - t``,
   ``wr = 1 - wl``, ``ce(k) = (m + log Z) - z_k``, ``side = ce(tl) * wl + ce(tl + 1) * wr``, ``dfl`` = the four sides added left to
   right, divided by 4; ``loss_dfl = sum(dfl * w) / norm``.
6. Gradients of ``L = wc * loss_cls + wi * loss_iou + wd * loss_dfl``: torch autograd's for those statements -- BCE's backward
   ``(p - q) / max((1 - p) * p, fl32(1e-12))`` also where the log was clamped, the weight not detached, ``clamp(0)`` passing at
   ``x >= 0``, equal ``min`` / ``max`` arguments splitting in halves -- formed in float64 and rounded once to float32.
7. A foreground anchor whose label lies outside ``[0, nc)`` sets ``ST_BAD_LABEL`` and is background for the class term.

The warm-up epochs (``epoch_num < warmup_epoch``) assign with the ATSS rules of ``detector_assign`` when ``ComputeLoss`` is
built with ``warmup_assigner="atss"``.  ``siou`` / ``ciou`` / ``diou`` and half-precision predictions are not mirrored.
The distillation losses of ``loss_distill.py`` are ``detector_distill``.
"""
import numpy as np
import torch

from . import _lib
from . import detector_assign as _da

F32, F64 = np.float32, np.float64
ST_BAD_LABEL = _lib.DETLOSS_ST_BAD_LABEL
MAX_REG = _lib.DETLOSS_MAX_REG
DEFAULT_WEIGHT = {"class": 1.0, "iou": 2.5, "dfl": 0.5}
IOU_EPS = 1e-10
BCE_EPS = F64(F32(1e-12))    # torch's EPSILON of binary_cross_entropy_backward is a float: 9.999999960041972e-13

_max, _min = _da._max, _da._min


def _weights(loss_weight):
    lw = DEFAULT_WEIGHT if loss_weight is None else loss_weight
    return float(lw["class"]), float(lw["iou"]), float(lw["dfl"])


def _reg(reg_max, use_dfl):
    R = int(reg_max)
    if not (1 if use_dfl else 0) <= R <= MAX_REG:
        raise ValueError("reg_max must be in %d..%d%s" % (1 if use_dfl else 0, MAX_REG, " with use_dfl" if use_dfl else ""))
    return R, (R + 1 if use_dfl else 1)


# ------------------------------------------------------------------------------------------------------------ the host route
def decode_host(pred_distri, anc_points, stride, reg_max=16, use_dfl=True, details=None):
    """Rule 1 in numpy: pred_distri (B, A, 4K) float32, anc_points (A, 2), stride (A,) or (A, 1) -> the float64 box (B, A, 4) in
    stride units.  ``details`` receives ``aps`` (A, 2), ``m``, ``Z``, ``d`` (B, A, 4) and ``pr`` (B, A, 4, K)."""
    R, K = _reg(reg_max, use_dfl)
    z = np.ascontiguousarray(pred_distri, dtype=F32)
    B, A = z.shape[:2]
    z = z.reshape(B, A, 4, K).astype(F64)
    anc = np.ascontiguousarray(anc_points, dtype=F32).reshape(A, 2)
    s = np.ascontiguousarray(stride, dtype=F32).reshape(A)
    aps = (anc / s[:, None]).astype(F32).astype(F64)
    with np.errstate(all="ignore"):
        if use_dfl:
            m = z[..., 0]
            for k in range(1, K):
                m = _max(m, z[..., k])
            e = np.exp(z - m[..., None])
            Z = np.zeros_like(m)
            for k in range(K):
                Z = Z + e[..., k]
            pr = e / Z[..., None]
            d = np.zeros_like(m)
            for k in range(K):
                d = d + pr[..., k] * F64(k)
        else:
            m, Z, d, pr = np.zeros((B, A, 4)), np.ones((B, A, 4)), z[..., 0], np.ones((B, A, 4, 1))
        ax, ay = aps[None, :, 0], aps[None, :, 1]
        box = np.stack([ax - d[..., 0], ay - d[..., 1], ax + d[..., 2], ay + d[..., 3]], axis=-1)
    if details is not None:
        details.update(aps=aps, m=m, Z=Z, d=d, pr=pr, z=z)
    return box


def _take(first, tie, g):
    """What a min / max hands to its first argument: all where it is the one taken, half at a tie."""
    return np.where(tie, 0.5 * g, np.where(first, g, 0.0))


def loss_host(pred_scores, pred_distri, anc_points, stride, target_labels, target_bboxes, target_scores, fg_mask, reg_max=16,
              use_dfl=True, loss_weight=None, details=None, norm_floor=1.0):
    """Rules 1-7 in numpy float64 (``norm_floor``: ``norm = tss > norm_floor ? tss : 1``; detector_distill passes 0): ``(losses float64 (5,) = [loss_cls, loss_iou, loss_dfl, tss, number of foreground anchors],
    grad_scores float32 (B, A, nc), grad_distri float32 (B, A, 4K), status uint32 (B,))``.  ``details``: a dict that receives the
    float64 gradients (``gs``, ``gz``), for each of their elements the sum of the absolute values of its terms (``gs_abs``,
    ``gz_abs``: what an error bound scales with), the same for the three sums (``cls_abs`` ...), ``box``, and the arguments of
    every min / max / clamp of the foreground anchors (``pairs``: arrays of (a, b), ``clamps``: the arguments of clamp(0))."""
    R, K = _reg(reg_max, use_dfl)
    wc, wi, wd = _weights(loss_weight)
    p32 = np.ascontiguousarray(pred_scores, dtype=F32)
    B, A, nc = p32.shape
    p = p32.astype(F64)
    q = np.asarray(target_scores).astype(F64).reshape(B, A, nc)
    tbp = np.asarray(target_bboxes).astype(F64).reshape(B, A, 4)
    labels = np.asarray(target_labels).astype(np.int64).reshape(B, A)
    fg = np.asarray(fg_mask).astype(bool).reshape(B, A)
    s = np.ascontiguousarray(stride, dtype=F32).reshape(A).astype(F64)
    dd = {}
    box = decode_host(pred_distri, anc_points, stride, reg_max, use_dfl, details=dd)
    aps, m, Z, d, pr, z = dd["aps"], dd["m"], dd["Z"], dd["d"], dd["pr"], dd["z"]
    with np.errstate(all="ignore"):
        w = np.zeros((B, A))
        for c in range(nc):
            w = w + q[..., c]
        tss = F64(w.sum())
        norm = tss if tss > norm_floor else F64(1.0)
        # the class term
        bad = fg & ((labels < 0) | (labels >= nc))
        status = np.where(bad.any(1), ST_BAD_LABEL, 0).astype(np.uint32)
        lab = fg[..., None] & (labels[..., None] == np.arange(nc)[None, None, :])
        wt = np.where(lab, q, (0.75 * p) * p)
        omp = 1.0 - p
        lp, lq = _max(np.log(p), -100.0), _max(np.log(omp), -100.0)
        t1, t2 = q * lp, (1.0 - q) * lq
        bce = -(t1 + t2)
        term = bce * wt
        cls = F64(term.sum())
        sc = wc / norm
        db = (p - q) / _max(omp * p, BCE_EPS)
        g1, g2 = db * wt, np.where(lab, 0.0, bce * (1.5 * p))
        gs = sc * (g1 + g2)
        gs_abs = np.abs(sc) * (np.abs(g1) + np.abs(g2))
        # the box term, on every anchor; background anchors are masked out of the sums
        tb = tbp / s[None, :, None]
        x1, y1, x2, y2 = (box[..., k] for k in range(4))
        tx1, ty1, tx2, ty2 = (tb[..., k] for k in range(4))
        iwr, ihr = _min(x2, tx2) - _max(x1, tx1), _min(y2, ty2) - _max(y1, ty1)
        iw, ih = _max(iwr, 0.0), _max(ihr, 0.0)
        inter = iw * ih
        w1, h1 = x2 - x1, (y2 - y1) + IOU_EPS
        w2, h2 = tx2 - tx1, (ty2 - ty1) + IOU_EPS
        uni = ((w1 * h1 + w2 * h2) - inter) + IOU_EPS
        iou = inter / uni
        cw, ch = _max(x2, tx2) - _min(x1, tx1), _max(y2, ty2) - _min(y1, ty1)
        ca = cw * ch + IOU_EPS
        num = ca - uni
        giou = iou - num / ca
        l_iou = np.where(fg, (1.0 - giou) * w, 0.0)
        s_iou = F64(l_iou.sum())
        ax, ay = aps[None, :, 0], aps[None, :, 1]
        gz = np.zeros((B, A, 4, K))
        gz_abs = np.zeros((B, A, 4, K))
        l_dfl = np.zeros((B, A))
        if use_dfl:
            hi = F64(R) - 0.01
            dist = np.stack([ax - tx1, ay - ty1, tx2 - ax, ty2 - ay], axis=-1)
            t = _min(_max(dist, 0.0), hi)
            tl = np.where((t >= 0) & (t < R), t, 0.0).astype(np.int64)
            tl = np.minimum(tl, R - 1)
            wl = (tl + 1).astype(F64) - t
            wr = 1.0 - wl
            lse = m + np.log(Z)
            cl = lse - np.take_along_axis(z, tl[..., None], -1)[..., 0]
            cr = lse - np.take_along_axis(z, tl[..., None] + 1, -1)[..., 0]
            side = cl * wl + cr * wr
            dfl = (((side[..., 0] + side[..., 1]) + side[..., 2]) + side[..., 3]) / 4.0
            l_dfl = np.where(fg, dfl * w, 0.0)
        s_dfl = F64(l_dfl.sum())
        # backwards through IOUloss
        g = (wi * w) / norm
        g_num = g / ca
        u1 = (g * num) / (ca * ca)
        g_ca, a_ca = g_num - u1, np.abs(g_num) + np.abs(u1)
        g_iou = -g
        u2 = (g_iou * inter) / (uni * uni)
        g_uni, a_uni = -g_num - u2, np.abs(g_num) + np.abs(u2)
        u3 = g_iou / uni
        g_int, a_int = u3 - g_uni, np.abs(u3) + a_uni
        g_w1, g_h1, a_w1, a_h1 = g_uni * h1, g_uni * w1, a_uni * np.abs(h1), a_uni * np.abs(w1)
        pass_w, pass_h = iwr >= 0, ihr >= 0
        g_iw, a_iw = np.where(pass_w, g_int * ih, 0.0), np.where(pass_w, a_int * ih, 0.0)
        g_ih, a_ih = np.where(pass_h, g_int * iw, 0.0), np.where(pass_h, a_int * iw, 0.0)
        g_cw, g_ch, a_cw, a_ch = g_ca * ch, g_ca * cw, a_ca * np.abs(ch), a_ca * np.abs(cw)
        g_x1 = (-_take(x1 > tx1, x1 == tx1, g_iw) - _take(x1 < tx1, x1 == tx1, g_cw)) - g_w1
        g_y1 = (-_take(y1 > ty1, y1 == ty1, g_ih) - _take(y1 < ty1, y1 == ty1, g_ch)) - g_h1
        g_x2 = (_take(x2 < tx2, x2 == tx2, g_iw) + _take(x2 > tx2, x2 == tx2, g_cw)) + g_w1
        g_y2 = (_take(y2 < ty2, y2 == ty2, g_ih) + _take(y2 > ty2, y2 == ty2, g_ch)) + g_h1
        a_x, a_y = a_iw + a_cw + a_w1, a_ih + a_ch + a_h1
        g_d = np.stack([-g_x1, -g_y1, g_x2, g_y2], axis=-1)
        a_d = np.stack([a_x, a_y, a_x, a_y], axis=-1)
        if use_dfl:
            cd = ((wd * w) / norm) / 4.0
            ks = np.arange(K, dtype=F64)[None, None, None, :]
            v1 = g_d[..., None] * (pr * (ks - d[..., None]))
            is_l, is_r = ks == tl[..., None], ks == tl[..., None] + 1
            v2 = np.where(is_r, np.where(is_l, pr - wl[..., None], pr) - wr[..., None], np.where(is_l, pr - wl[..., None], pr))
            gz = v1 + cd[..., None, None] * v2
            gz_abs = a_d[..., None] * (pr * (ks + np.abs(d[..., None]))) + np.abs(cd)[..., None, None] * (
                pr + np.where(is_l, np.abs(wl[..., None]), 0.0) + np.where(is_r, np.abs(wr[..., None]), 0.0))
        else:
            gz, gz_abs = g_d[..., None], a_d[..., None]
        gz = np.where(fg[..., None, None], gz, 0.0)
        gz_abs = np.where(fg[..., None, None], gz_abs, 0.0)
        losses = np.array([cls / norm, s_iou / norm, s_dfl / norm, tss, F64(fg.sum())], F64)
    if details is not None:
        sel = fg
        pairs = [np.stack([a_[sel], b_[sel]], -1) for a_, b_ in ((x1, tx1), (y1, ty1), (x2, tx2), (y2, ty2))]
        with np.errstate(all="ignore"):
            # what an error bound of the box terms scales with: the greatest coordinate over the smallest length that enters a
            # product or a quotient, and the sums of the absolute values of the terms of (1 - giou) * w and of dfl * w
            extent = np.max(np.abs(np.concatenate([box, tb, d, np.broadcast_to(aps[None], (B, A, 2))], axis=-1)), axis=-1)
            lengths = np.stack([w1, h1, w2, h2, cw, ch, np.where(iwr > 0, iwr, np.inf), np.where(ihr > 0, ihr, np.inf)], axis=-1)
            details["cond"] = np.where(fg, extent / np.min(np.abs(lengths), axis=-1), 0.0)
            details["iou_scale"] = np.where(fg, w * ((1.0 + np.abs(iou)) + np.abs(num / ca)), 0.0) / norm
            if use_dfl:
                zl = np.abs(np.take_along_axis(z, tl[..., None], -1)[..., 0])
                zr = np.abs(np.take_along_axis(z, tl[..., None] + 1, -1)[..., 0])
                big = np.abs(m) + np.abs(np.log(Z)) + 1.0
                details["dfl_scale"] = np.where(fg, w * ((big + zl) * np.abs(wl) + (big + zr) * np.abs(wr)).sum(-1) / 4.0, 0.0) / norm
            else:
                details["dfl_scale"] = np.zeros((B, A))
        details.update(gs=gs, gz=gz.reshape(B, A, 4 * K), gs_abs=gs_abs, gz_abs=gz_abs.reshape(B, A, 4 * K), box=box, norm=norm,
                       cls_abs=F64(np.abs(term).sum()) / norm, iou_abs=F64(np.abs(l_iou).sum()) / norm,
                       dfl_abs=F64(np.abs(l_dfl).sum()) / norm, pairs=pairs, clamps=[iwr[sel], ihr[sel]], w=w,
                       dist=dist[sel] if use_dfl else None)
    return losses, gs.astype(F32), gz.reshape(B, A, 4 * K).astype(F32), status


# ---------------------------------------------------------------------------------------------------------- the device route
def _want_f32(t, what):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
        raise ValueError("%s is %s: the loss takes float32 predictions, call .float() on them first"
                         % (what, getattr(t, "dtype", type(t).__name__)))


def _anchors_on(dev, anc_points, stride, A):
    anc = _lib.want(anc_points.detach().to(dev).float().contiguous(), "anc_points", torch.float32, shape=(A, 2), device=dev)
    st = _lib.want(stride.detach().to(dev).float().reshape(-1).contiguous(), "stride", torch.float32, shape=(A,), device=dev)
    return anc, st


def decode_boxes(pred_distri, anc_points, stride, reg_max=16, use_dfl=True):
    """``bbox_decode`` (loss.py:238-244), no gradient: pred_distri (B, A, 4 * (reg_max + 1)) float32, anc_points (A, 2) in pixels,
    stride (A,) or (A, 1) -> ``(pred_bboxes, pred_bboxes_px)`` float32 (B, A, 4): the float64 box in stride units rounded once, and
    ``fl32(box * stride)``, what the assigner takes.  CUDA tensors take the kernel (one launch), CPU tensors ``decode_host``."""
    _want_f32(pred_distri, "pred_distri")
    R, K = _reg(reg_max, use_dfl)
    if pred_distri.dim() != 3 or int(pred_distri.shape[2]) != 4 * K:
        raise ValueError("pred_distri must be (B, A, %d)" % (4 * K))
    B, A = int(pred_distri.shape[0]), int(pred_distri.shape[1])
    if not pred_distri.is_cuda:
        box = decode_host(pred_distri.detach().numpy(), anc_points.detach().float().numpy(), stride.detach().float().numpy(), R, use_dfl)
        s = stride.detach().float().numpy().reshape(A).astype(F64)
        return torch.from_numpy(box.astype(F32)), torch.from_numpy((box * s[None, :, None]).astype(F32))
    dev = pred_distri.device
    if not (1 <= B <= 65535 and 1 <= A <= _lib.TAL_MAX_ANCHORS):
        raise ValueError("decode_boxes takes 1 <= B <= 65535 and 1 <= A <= 2^24")
    z = pred_distri.detach().contiguous()
    anc, st = _anchors_on(dev, anc_points, stride, A)
    boxes_s = torch.empty((B, A, 4), dtype=torch.float32, device=dev)
    boxes_px = torch.empty((B, A, 4), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.api().evrep_detloss_decode(_lib.ptr(z), _lib.ptr(anc), _lib.ptr(st), B, A, R, _lib.DETLOSS_USE_DFL if use_dfl else 0,
                                        _lib.ptr(boxes_s), _lib.ptr(boxes_px), _lib.stream_ptr())
    return boxes_s, boxes_px


def _targets_on(dev, target_labels, target_bboxes, target_scores, fg_mask, B, A, nc, use_dfl, grad):
    """The four targets held to their dtypes and shapes on ``dev``, and the flags word ``evrep_detloss`` and
    ``evrep_detloss_distill`` take: ``(labels, tb, ts, fg uint8, flags)``."""
    tdt = target_scores.dtype
    if tdt not in (torch.float64, torch.float32) or target_bboxes.dtype != tdt:
        raise ValueError("target_bboxes and target_scores must both be float64 (what assign_batch returns) or both float32")
    labels = _lib.want(target_labels.detach().contiguous(), "target_labels", torch.int64, shape=(B, A), device=dev)
    tb = _lib.want(target_bboxes.detach().contiguous(), "target_bboxes", tdt, shape=(B, A, 4), device=dev)
    ts = _lib.want(target_scores.detach().contiguous(), "target_scores", tdt, shape=(B, A, nc), device=dev)
    fg = fg_mask.detach()
    fg = (fg.view(torch.uint8) if fg.dtype == torch.bool else fg.to(torch.uint8)).contiguous()
    fg = _lib.want(fg, "fg_mask", torch.uint8, shape=(B, A), device=dev)
    flags = (_lib.DETLOSS_USE_DFL if use_dfl else 0) | (0 if grad else _lib.DETLOSS_NO_GRAD) | \
        (_lib.DETLOSS_F32_TARGETS if tdt == torch.float32 else 0)
    return labels, tb, ts, fg, flags


def _outputs(dev, n_losses, B, A, nc, K, grad):
    """What the two C entries write: ``(losses float64 (n_losses,), grad_scores, grad_distri (None without grad), status)``."""
    losses = torch.empty((n_losses,), dtype=torch.float64, device=dev)
    gs = torch.empty((B, A, nc), dtype=torch.float32, device=dev) if grad else None
    gz = torch.empty((B, A, 4 * K), dtype=torch.float32, device=dev) if grad else None
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    return losses, gs, gz, status


def _loss_device(pred_scores, pred_distri, anc_points, stride, target_labels, target_bboxes, target_scores, fg_mask, R, K, use_dfl,
                 weights, grad):
    """The C entry on CUDA tensors: ``(losses float64 (5,), grad_scores, grad_distri (None without grad), status int32 (B,))``."""
    dev = pred_scores.device
    B, A, nc = (int(v) for v in pred_scores.shape)
    if not (1 <= B <= 65535 and 1 <= A <= _lib.TAL_MAX_ANCHORS and 1 <= nc <= _lib.TAL_MAX_CLASSES and A * nc < 2 ** 31):
        raise ValueError("the loss takes 1 <= B <= 65535, 1 <= A <= 2^24, 1 <= nc <= %d and A * nc < 2^31" % _lib.TAL_MAX_CLASSES)
    p = pred_scores.detach().contiguous()
    z = _lib.want(pred_distri.detach().contiguous(), "pred_distri", torch.float32, shape=(B, A, 4 * K), device=dev)
    anc, st = _anchors_on(dev, anc_points, stride, A)
    labels, tb, ts, fg, flags = _targets_on(dev, target_labels, target_bboxes, target_scores, fg_mask, B, A, nc, use_dfl, grad)
    losses, gs, gz, status = _outputs(dev, 5, B, A, nc, K, grad)
    with torch.cuda.device(dev):
        api = _lib.api()
        scratch = _lib.scratch(api.evrep_detloss_workspace_bytes(B, A, nc), dev)
        api.evrep_detloss(_lib.ptr(p), _lib.ptr(z), _lib.ptr(anc), _lib.ptr(st), _lib.ptr(labels), _lib.ptr(tb), _lib.ptr(ts), _lib.ptr(fg),
                          B, A, nc, R, weights[0], weights[1], weights[2], flags, _lib.ptr(losses), _lib.ptr(gs), _lib.ptr(gz),
                          _lib.ptr(status), _lib.ptr(scratch), _lib.stream_ptr())
    return losses, gs, gz, status


class _Weighted(torch.autograd.Function):
    """``wc * loss_cls + wi * loss_iou + wd * loss_dfl`` carrying the two gradient arrays."""

    @staticmethod
    def forward(ctx, pred_scores, pred_distri, loss, gs, gz):
        ctx.save_for_backward(gs, gz)
        return loss.clone()

    @staticmethod
    def backward(ctx, grad_output):
        gs, gz = ctx.saved_tensors
        g = grad_output.to(torch.float32)
        return (gs * g if ctx.needs_input_grad[0] else None), (gz * g if ctx.needs_input_grad[1] else None), None, None, None


def _combine(losses, weights):
    wc, wi, wd = weights
    loss = (losses[0] * wc + losses[1] * wi) + losses[2] * wd
    items = torch.stack((losses[1] * wi, losses[2] * wd, losses[0] * wc)).detach()
    return loss, items


def check_status(status):
    """ValueError naming the first image whose status word is not zero (one read-back)."""
    st = status.detach().cpu().numpy().astype(np.int64)
    if st.any():
        b = int(np.flatnonzero(st)[0])
        raise ValueError("image %d: a foreground anchor's label outside [0, num_classes) (status %d)" % (b, st[b]))


def _from_host(out, grad):
    """What ``loss_host`` / ``distill_host`` return, as the tensors the device route returns: ``(losses, gs, gz, status)``."""
    gs, gz = (torch.from_numpy(out[1]), torch.from_numpy(out[2])) if grad else (None, None)
    return torch.from_numpy(out[0]), gs, gz, torch.from_numpy(out[3].view(np.int32))


def _finish(pred_scores, pred_distri, loss, items, gs, gz, status, grad, check, return_status):
    """The tail of ``loss_batch`` / ``distill_batch``: the autograd node, ``check``, the return tuple."""
    if grad:
        loss = _Weighted.apply(pred_scores, pred_distri, loss, gs, gz)
    if check:
        check_status(status)
    return (loss, items, status) if return_status else (loss, items)


def loss_batch(pred_scores, pred_distri, anc_points, stride, target_labels, target_bboxes, target_scores, fg_mask, num_classes,
               reg_max=16, use_dfl=True, loss_weight=None, check=False, return_status=False):
    """loss.py:176-217: ``(loss, loss_items)``.  pred_scores (B, A, nc) and pred_distri (B, A, 4 * (reg_max + 1)) float32, anc_points
    (A, 2) in pixels, stride (A,) or (A, 1); the four targets as ``assign_batch`` returns them (``target_bboxes`` in pixels; float64,
    or both float32).  ``loss`` is a float64 scalar on the predictions' device; where a prediction requires grad it carries one
    autograd node whose gradients were made by the forward launches and are multiplied by ``grad_output`` in backward.  Under
    ``torch.no_grad()`` (or with predictions that need none) no gradient is computed.  ``loss_items`` is the reference's detached
    ``cat((wi * iou, wd * dfl, wc * cls))``.  CUDA tensors take the kernels, with no host read; CPU tensors ``loss_host``.
    ``check=True`` reads the status back and raises ValueError naming the image; ``return_status`` appends the (B,) status."""
    _want_f32(pred_scores, "pred_scores")
    _want_f32(pred_distri, "pred_distri")
    R, K = _reg(reg_max, use_dfl)
    if pred_scores.dim() != 3 or int(pred_scores.shape[2]) != int(num_classes):
        raise ValueError("pred_scores must be (B, A, num_classes = %d), got %s" % (num_classes, tuple(pred_scores.shape)))
    weights = _weights(loss_weight)
    grad = torch.is_grad_enabled() and (pred_scores.requires_grad or pred_distri.requires_grad)
    if pred_scores.is_cuda:
        losses, gs, gz, status = _loss_device(pred_scores, pred_distri, anc_points, stride, target_labels, target_bboxes, target_scores,
                                              fg_mask, R, K, use_dfl, weights, grad)
    else:
        out = loss_host(pred_scores.detach().numpy(), pred_distri.detach().numpy(), anc_points.detach().float().numpy(),
                        stride.detach().float().numpy(), target_labels.numpy(), target_bboxes.numpy(), target_scores.numpy(),
                        fg_mask.numpy(), R, use_dfl, dict(zip(("class", "iou", "dfl"), weights)))
        losses, gs, gz, status = _from_host(out, grad)
    loss, items = _combine(losses, weights)
    return _finish(pred_scores, pred_distri, loss, items, gs, gz, status, grad, check, return_status)


class ComputeLoss:
    """``yolov6.models.losses.loss.ComputeLoss`` with its constructor arguments and call signature:
    ``__call__(outputs, targets, epoch_num, step_num, batch_height, batch_width) -> (loss, loss_items)`` with
    ``outputs = (feats, pred_scores, pred_distri)``.  The sequence is ``decode_boxes`` -> ``assign_batch`` -> ``loss_batch``; the
    anchors come from the feature shapes and are cached per shape on the device.  ``epoch_num < warmup_epoch`` assigns with
    ``warmup_assigner``: ``"atss"`` (the reference's ``ATSSAssigner(9, num_classes)``) or a ``detector_assign.ATSSAssigner`` takes
    ``atss_assign_batch`` for CUDA predictions, with no host read, and the host route for CPU tensors; any other callable is called
    with the reference's argument list ``(anchors, n_anchors_list, gt_labels, gt_bboxes, mask_gt, pred_bboxes_px)`` and returns
    ``(target_labels, target_bboxes, target_scores, fg_mask)``; the default None raises NotImplementedError there.
    ``max_labels`` is as in ``assign_batch`` (needed for CUDA ``targets``).  CPU tensors
    take the host routes.  No ``empty_cache``, no CPU fall-back for device tensors.  ``last_status`` holds the (B,) status words of
    the last call (assigner | loss)."""

    def __init__(self, fpn_strides=(8, 16, 32), grid_cell_size=5.0, grid_cell_offset=0.5, num_classes=80, ori_img_size=640,
                 warmup_epoch=4, use_dfl=True, reg_max=16, iou_type="giou", loss_weight=None, warmup_assigner=None, max_labels=None):
        if str(iou_type).lower() != "giou":
            raise NotImplementedError("iou_type = %r: only 'giou', what every shipped config uses, is built" % (iou_type,))
        self.fpn_strides, self.grid_cell_size, self.grid_cell_offset = tuple(fpn_strides), float(grid_cell_size), float(grid_cell_offset)
        self.num_classes, self.ori_img_size, self.warmup_epoch = int(num_classes), ori_img_size, warmup_epoch
        self.use_dfl, self.reg_max, self.iou_type = bool(use_dfl), int(reg_max), "giou"
        _reg(self.reg_max, self.use_dfl)
        self.loss_weight = dict(DEFAULT_WEIGHT if loss_weight is None else loss_weight)
        if isinstance(warmup_assigner, str):
            if warmup_assigner.lower() != "atss":
                raise ValueError("warmup_assigner = %r: 'atss', an assigner object or None" % (warmup_assigner,))
            warmup_assigner = _da.ATSSAssigner(9, num_classes=self.num_classes)
        if isinstance(warmup_assigner, _da.ATSSAssigner) and warmup_assigner.num_classes != self.num_classes:
            raise ValueError("the warm-up assigner has %d classes, the loss %d" % (warmup_assigner.num_classes, self.num_classes))
        self.warmup_assigner, self.max_labels = warmup_assigner, max_labels
        self.formal_assigner = _da.TaskAlignedAssigner(topk=13, num_classes=self.num_classes, alpha=1.0, beta=6.0)
        self.last_status = None
        self._anchors = {}

    def anchors(self, feats, device):
        """``generate_anchors`` in training mode for the feature maps' shapes: ``(anchors (A, 4), anchor_points (A, 2), n_anchors_list,
        stride_tensor (A, 1))`` float32 on ``device``, cached per shapes and device."""
        key = (tuple((int(f.shape[-2]), int(f.shape[-1])) for f in feats), str(device))
        if key not in self._anchors:
            boxes, points, strides, counts = [], [], [], []
            for (h, w), s in zip(key[0], self.fpn_strides):
                x = ((np.arange(w, dtype=F32) + F32(self.grid_cell_offset)) * F32(s)).astype(F32)
                y = ((np.arange(h, dtype=F32) + F32(self.grid_cell_offset)) * F32(s)).astype(F32)
                yy, xx = np.meshgrid(y, x, indexing="ij")
                half = F32(self.grid_cell_size * s * 0.5)
                boxes.append(np.stack([xx - half, yy - half, xx + half, yy + half], axis=-1).reshape(-1, 4).astype(F32))
                points.append(np.stack([xx, yy], axis=-1).reshape(-1, 2))
                strides.append(np.full((h * w, 1), s, F32))
                counts.append(h * w)
            self._anchors[key] = (torch.from_numpy(np.concatenate(boxes, 0)).to(device), torch.from_numpy(np.concatenate(points, 0)).to(device),
                                  counts, torch.from_numpy(np.concatenate(strides, 0)).to(device))
        return self._anchors[key]

    def targets_of(self, feats, pred_scores, pred_distri, targets, epoch_num, batch_height, batch_width):
        """``decode_boxes`` and the assigner of the epoch: ``(anc, stride, labels, target_bboxes, target_scores, fg, status or None)``."""
        dev = pred_scores.device
        anchors, anc, n_anchors_list, stride = self.anchors(feats, dev)
        B = int(pred_scores.shape[0])
        _, boxes_px = decode_boxes(pred_distri, anc, stride, self.reg_max, self.use_dfl)
        if epoch_num < self.warmup_epoch:
            if self.warmup_assigner is None:
                raise NotImplementedError("epoch %d < warmup_epoch %d: the reference assigns with ATSSAssigner there; build ComputeLoss "
                                          "with warmup_assigner='atss' for it (or hand it a callable, or set warmup_epoch=0)"
                                          % (epoch_num, self.warmup_epoch))
            ours = isinstance(self.warmup_assigner, _da.ATSSAssigner)
            if ours and pred_scores.is_cuda:
                labels, tb, ts, fg, st_assign = _da.atss_assign_batch(anchors, n_anchors_list, boxes_px, targets, (batch_height, batch_width),
                                                                     self.num_classes, max_labels=self.max_labels,
                                                                     topk=self.warmup_assigner.topk)
            else:
                gt = _da.preprocess(targets, B, batch_width, batch_height, self.max_labels)
                if gt.device != dev:
                    gt = gt.to(dev)
                gt_labels, gt_bboxes = gt[:, :, :1], gt[:, :, 1:]
                mask_gt = (gt_bboxes.sum(-1, keepdim=True) > 0).float()
                labels, tb, ts, fg = self.warmup_assigner(anchors, n_anchors_list, gt_labels, gt_bboxes, mask_gt, boxes_px)
                st_assign = self.warmup_assigner.last_status if ours else None
        elif pred_scores.is_cuda:
            labels, tb, ts, fg, st_assign = _da.assign_batch(pred_scores, boxes_px, anc, targets, (batch_height, batch_width),
                                                            self.num_classes, max_labels=self.max_labels)
        else:
            gt = _da.preprocess(targets, B, batch_width, batch_height, self.max_labels)
            labels, tb, ts, fg = self.formal_assigner(pred_scores.detach(), boxes_px, anc, gt[:, :, :1], gt[:, :, 1:], None)
            st_assign = self.formal_assigner.last_status
        return anc, stride, labels, tb, ts, fg, st_assign

    def __call__(self, outputs, targets, epoch_num, step_num, batch_height, batch_width):
        feats, pred_scores, pred_distri = outputs
        _want_f32(pred_scores, "pred_scores")
        _want_f32(pred_distri, "pred_distri")
        anc, stride, labels, tb, ts, fg, st_assign = self.targets_of(feats, pred_scores, pred_distri, targets, epoch_num, batch_height,
                                                                    batch_width)
        loss, items, st = loss_batch(pred_scores, pred_distri, anc, stride, labels, tb, ts, fg, self.num_classes, self.reg_max,
                                     self.use_dfl, self.loss_weight, return_status=True)
        self.last_status = st if st_assign is None else torch.bitwise_or(st, st_assign.to(st.device))
        return loss, items
