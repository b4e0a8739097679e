"""The distillation losses on the device: what the reference's ``loss_distill.ComputeLoss.__call__`` does behind the assigner.

``ev-YOLOv6/yolov6/models/losses/loss_distill.py:62-340`` (``engine.py:226-242`` with ``--distill``) adds to the three terms of
``loss.py`` a KL term between the student's and the teacher's class scores over all ``B * A`` rows, a KL term between their DFL
bins on the foreground rows, and with ``distill_feat`` a channel-wise KL term over three feature maps.  Here ``distill_batch``
computes the five terms AND the gradients with respect to the student's ``pred_scores`` / ``pred_distri`` in four launches
(``evrep_detloss_distill``, csrc/evrep_detdistill.hip with the shared kernels of csrc/evrep_detloss.hip), ``distill_cw`` the
channel-wise term and the maps' gradients in two (``evrep_detloss_cwd``), with no host read.  ``distill_host`` and ``cw_host``
are the same rules in numpy float64: the oracle of the kernels and the route of CPU tensors.  ``ComputeLossDistill`` strings
them together behind the reference's constructor and call signature.

The rules (include/evrep.h states them with ``evrep_detloss_distill`` and ``evrep_detloss_cwd``); T = ``temperature``, tp / tz the
teacher's ``pred_scores`` / ``pred_distri``, everything else as in ``detector_loss``:

1. ``loss_cls``, ``loss_iou``, ``loss_dfl`` as in ``detector_loss`` but ``norm = tss > 0 ? tss : 1``.
2. Softmax at T: ``m = max_k (x_k / T)``, ``e_k = exp(x_k / T - m)``, Z = the e_k added left to right, ``pr_k = e_k / Z``.
3. KL terms: ``pt_k * log(pt_k) - pt_k * log(ps_k)`` (first product 0 at ``pt_k == 0``), added in an order that depends on the
   shape only; spt = the pt_k of a row added left to right.
4. ``d_loss_cls = (T * T) * (all rows of the scores)``, not normalised.
5. ``d_loss_dfl = (((T * T) * (sum over the 4 * n_fg foreground rows / (4 * n_fg))) * W) / norm``, W = the ``w[b, a]`` of the
   foreground anchors; 0 without DFL or without a foreground anchor.
6. Gradients of ``wc * (loss_cls + k_class * d_loss_cls) + wi * loss_iou + wd * (loss_dfl + k_dfl * d_loss_dfl)``:
   ``detector_loss``'s plus ``((wc * k_class) * T) * (ps * spt - pt)`` and, on foreground rows,
   ``((((wd * k_dfl) * T) * W) / norm / (4 * n_fg)) * (ps * spt - pt)``; one rounding to float32.
7. Channel-wise term per level and ``(n, c)`` row at ``tau``: ``ls = (s / tau - ms) - log(Zs)``, ``lt`` likewise, ``pt = exp(lt)``,
   row = ``sum pt * (lt - ls)``; the level = ``rows * (tau * tau / (N * C))``; the first three levels are added left to right;
   ``d / d s = (tau / (N * C)) * (exp(ls) * sum(pt) - pt)``.
8. ``decay = ((1 - cos(epoch * pi / max_epoch)) / 2) * (0.01 - 1) + 1`` in Python floats; ``k_class = decay * dw["class"]``,
   ``k_dfl = decay * dw["dfl"]``; ``loss = ((wc * cls_all + wi * loss_iou) + wd * dfl_all) + d_loss_cw * (decay * w_cwd)``,
   with ``cls_all = loss_cls + d_loss_cls * k_class`` and ``dfl_all = loss_dfl + d_loss_dfl * k_dfl``.

16-bit feature maps (training under ``torch.autocast``): ``distill_cw`` takes float16 or bfloat16 maps as they are -- the three
student maps of one dtype, the three teacher maps of one, and the two may differ (a teacher may run outside autocast).  An
element is widened exactly to float32 at its load, so the loss has the bits it has for ``map.float()`` and stays float64.  The
gradient arrays of rule 7 stay FLOAT32 whatever the maps' dtype: an element is ``tau / (N * C)`` times a difference of
probabilities, about 1e-8 at the reference's shapes, below float16's smallest subnormal before the loss scale multiplies it.
The autograd node returns ``(g32 * grad_output).to(student's dtype)``: the one rounding comes after the scale.

float64 maps, 16-bit ``pred_scores`` / ``pred_distri`` (with ``detector_head``'s tail they are float32 by construction),
``loss_distill_ns.py`` and ``fuse_ab`` are not mirrored."""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from . import detector_loss as _dl

F32, F64 = np.float32, np.float64
DEFAULT_WEIGHT = {"class": 1.0, "iou": 2.5, "dfl": 0.5, "cwd": 10.0}
DEFAULT_DISTILL_WEIGHT = {"class": 1.0, "dfl": 1.0}
CW_LEVELS = _lib.CWD_MAX_LEVELS

_max = _dl._max


def decay(epoch_num, max_epoch):
    """Rule 8's ``distill_weightdecay``, a Python float."""
    return ((1 - math.cos(epoch_num * math.pi / max_epoch)) / 2) * (0.01 - 1) + 1


def _temperature(T):
    T = float(T)
    if not (math.isfinite(T) and T > 0):
        raise ValueError("temperature must be finite and > 0, got %r" % (T,))
    return T


# ------------------------------------------------------------------------------------------------------------ the host route
def _softmax_at(x, T):
    """Rule 2 over the last axis of a float64 array."""
    x = x / T
    n = x.shape[-1]
    m = x[..., 0]
    for k in range(1, n):
        m = _max(m, x[..., k])
    e = np.exp(x - m[..., None])
    Z = np.zeros_like(m)
    for k in range(n):
        Z = Z + e[..., k]
    return e / Z[..., None]


def _kl_rows(ps, pt):
    """Rule 3: ``(rows, spt, rows_abs)``; rows_abs adds the absolute values of both products of every term."""
    a = np.where(pt == 0, 0.0, pt * np.log(np.where(pt == 0, 1.0, pt)))
    b = pt * np.log(ps)
    term = a - b
    rows, spt, rows_abs = np.zeros(ps.shape[:-1]), np.zeros(ps.shape[:-1]), np.zeros(ps.shape[:-1])
    for k in range(ps.shape[-1]):
        rows = rows + term[..., k]
        spt = spt + pt[..., k]
        rows_abs = rows_abs + (np.abs(a[..., k]) + np.abs(b[..., k]))
    return rows, spt, rows_abs


def distill_host(pred_scores, pred_distri, t_pred_scores, t_pred_distri, anc_points, stride, target_labels, target_bboxes,
                 target_scores, fg_mask, temperature, k_class=1.0, k_dfl=1.0, reg_max=16, use_dfl=True, loss_weight=None, details=None):
    """Rules 1-6 in numpy float64: ``(losses float64 (8,) = [loss_cls, loss_iou, loss_dfl, d_loss_cls, d_loss_dfl, tss, n_fg, W],
    grad_scores float32 (B, A, nc), grad_distri float32 (B, A, 4K), status uint32 (B,))``.  ``details`` receives ``loss_host``'s
    and the float64 gradients with the distillation parts (``gs``, ``gz``), the sums of the absolute values of their terms
    (``gs_abs``, ``gz_abs``; ``*_base`` and ``*_kd`` are their two parts), of the two distillation losses' terms (``dcls_abs``,
    ``ddfl_abs``) and the same scaled sums of the rows' ``spt`` (``dcls_spt``, ``ddfl_spt``: what a probability's error scales)."""
    T = _temperature(temperature)
    R, K = _dl._reg(reg_max, use_dfl)
    wc, wi, wd = _dl._weights(loss_weight)
    d = {}
    base, _, _, status = _dl.loss_host(pred_scores, pred_distri, anc_points, stride, target_labels, target_bboxes, target_scores, fg_mask,
                                       R, use_dfl, dict(zip(("class", "iou", "dfl"), (wc, wi, wd))), details=d, norm_floor=0.0)
    p = np.ascontiguousarray(pred_scores, dtype=F32).astype(F64)
    B, A, nc = p.shape
    tp = np.ascontiguousarray(t_pred_scores, dtype=F32).astype(F64).reshape(B, A, nc)
    fg = np.asarray(fg_mask).astype(bool).reshape(B, A)
    norm, w = d["norm"], d["w"]
    T2 = F64(T) * F64(T)
    with np.errstate(all="ignore"):
        ps, pt = _softmax_at(p, F64(T)), _softmax_at(tp, F64(T))
        rows, spt, rows_abs = _kl_rows(ps, pt)
        d_cls = T2 * F64(rows.sum())
        ck = (F64(wc) * F64(k_class)) * F64(T)
        u1 = ps * spt[..., None]
        gs = d["gs"] + ck * (u1 - pt)
        gs_kd = np.abs(ck) * (np.abs(u1) + np.abs(pt))
        n_fg = F64(fg.sum())
        W = F64(w[fg].sum())
        gz, gz_kd = d["gz"], np.zeros_like(d["gz"])
        d_dfl, ddfl_abs, ddfl_spt = F64(0.0), F64(0.0), F64(0.0)
        if use_dfl and n_fg > 0:
            z = np.ascontiguousarray(pred_distri, dtype=F32).astype(F64).reshape(B, A, 4, K)
            tz = np.ascontiguousarray(t_pred_distri, dtype=F32).astype(F64).reshape(B, A, 4, K)
            qs, qt = _softmax_at(z, F64(T)), _softmax_at(tz, F64(T))
            r4, s4, a4 = _kl_rows(qs, qt)
            tot = F64(r4[fg].sum())
            d_dfl = ((T2 * (tot / (4.0 * n_fg))) * W) / norm
            ddfl_abs = ((T2 * (F64(a4[fg].sum()) / (4.0 * n_fg))) * np.abs(W)) / norm
            ddfl_spt = ((T2 * (F64(s4[fg].sum()) / (4.0 * n_fg))) * np.abs(W)) / norm
            cdd = ((((F64(wd) * F64(k_dfl)) * F64(T)) * W) / norm) / (4.0 * n_fg)
            u2 = qs * s4[..., None]
            add = np.where(fg[..., None, None], cdd * (u2 - qt), 0.0)
            gz = gz + add.reshape(B, A, 4 * K)
            gz_kd = np.where(fg[..., None, None], np.abs(cdd) * (np.abs(u2) + np.abs(qt)), 0.0).reshape(B, A, 4 * K)
        losses = np.array([base[0], base[1], base[2], d_cls, d_dfl, base[3], n_fg, W], F64)
    if details is not None:
        details.update(d)
        details.update(gs=gs, gz=gz, gs_abs=d["gs_abs"] + gs_kd, gz_abs=d["gz_abs"] + gz_kd, gs_abs_base=d["gs_abs"],
                       gz_abs_base=d["gz_abs"], gs_abs_kd=gs_kd, gz_abs_kd=gz_kd, dcls_abs=T2 * F64(rows_abs.sum()),
                       dcls_spt=T2 * F64(spt.sum()), ddfl_abs=ddfl_abs, ddfl_spt=ddfl_spt, T=T)
    return losses, gs.astype(F32), gz.astype(F32), status


def cw_host(s_feats, t_feats, temperature=1.0, details=None):
    """Rule 7 in numpy float64 over the first three maps: ``(out float64 (4,) = [d_loss_cw, level 0, 1, 2], [grad_s float32 per
    level])``.  ``details`` receives the float64 gradients (``g``), their terms' absolute sums (``g_abs``) and per level the sum
    of the absolute values of the loss's terms (``abs``), the scaled sum of the rows' ``spt`` (``spt``) and the greatest
    ``|ls|`` or ``|lt|`` (``amax``)."""
    tau = F64(_temperature(temperature))
    out, grads, g64, g_abs, l_abs, l_spt, amax = np.zeros(4, F64), [], [], [], [], [], []
    with np.errstate(all="ignore"):
        for l in range(CW_LEVELS):
            s = np.ascontiguousarray(s_feats[l], dtype=F32)
            N, C, H, Wd = s.shape
            x = s.astype(F64).reshape(N, C, H * Wd) / tau
            y = np.ascontiguousarray(t_feats[l], dtype=F32).astype(F64).reshape(N, C, H * Wd) / tau
            xm, ym = x - x.max(-1, keepdims=True), y - y.max(-1, keepdims=True)
            ls = xm - np.log(np.exp(xm).sum(-1, keepdims=True))
            lt = ym - np.log(np.exp(ym).sum(-1, keepdims=True))
            pt = np.exp(lt)
            term = pt * (lt - ls)
            spt = pt.sum(-1, keepdims=True)
            nc = F64(N * C)
            out[1 + l] = F64(term.sum()) * ((tau * tau) / nc)
            u = np.exp(ls) * spt
            g = (tau / nc) * (u - pt)
            grads.append(g.reshape(N, C, H, Wd).astype(F32))
            g64.append(g.reshape(N, C, H, Wd))
            g_abs.append(((tau / nc) * (np.abs(u) + pt)).reshape(N, C, H, Wd))
            l_abs.append(F64((pt * (np.abs(lt) + np.abs(ls))).sum()) * ((tau * tau) / nc))
            l_spt.append(F64(spt.sum()) * ((tau * tau) / nc))
            amax.append(F64(max(np.abs(ls).max(), np.abs(lt).max())))
        out[0] = (out[1] + out[2]) + out[3]
    if details is not None:
        details.update(g=g64, g_abs=g_abs, abs=l_abs, spt=l_spt, amax=amax)
    return out, grads


# ---------------------------------------------------------------------------------------------------------- the device route
def _distill_device(pred_scores, pred_distri, t_pred_scores, t_pred_distri, anc_points, stride, target_labels, target_bboxes,
                    target_scores, fg_mask, R, K, use_dfl, weights, T, k_class, k_dfl, grad):
    """The C entry on CUDA tensors: ``(losses float64 (8,), grad_scores, grad_distri (None without grad), status int32 (B,))``."""
    dev = pred_scores.device
    B, A, nc = (int(v) for v in pred_scores.shape)
    if not (1 <= B <= 65535 and 1 <= A <= _lib.TAL_MAX_ANCHORS and 1 <= nc <= _lib.DISTILL_MAX_CLASSES and A * nc < 2 ** 31):
        raise ValueError("the loss takes 1 <= B <= 65535, 1 <= A <= 2^24, 1 <= nc <= %d and A * nc < 2^31" % _lib.DISTILL_MAX_CLASSES)
    p = pred_scores.detach().contiguous()
    z = _lib.want(pred_distri.detach().contiguous(), "pred_distri", torch.float32, shape=(B, A, 4 * K), device=dev)
    tp = _lib.want(t_pred_scores.detach().contiguous(), "t_pred_scores", torch.float32, shape=(B, A, nc), device=dev)
    tz = _lib.want(t_pred_distri.detach().contiguous(), "t_pred_distri", torch.float32, shape=(B, A, 4 * K), device=dev)
    anc, st = _dl._anchors_on(dev, anc_points, stride, A)
    labels, tb, ts, fg, flags = _dl._targets_on(dev, target_labels, target_bboxes, target_scores, fg_mask, B, A, nc, use_dfl, grad)
    losses, gs, gz, status = _dl._outputs(dev, 8, B, A, nc, K, grad)
    with torch.cuda.device(dev):
        api = _lib.api()
        scratch = _lib.scratch(api.evrep_detloss_distill_workspace_bytes(B, A, nc), dev)
        api.evrep_detloss_distill(_lib.ptr(p), _lib.ptr(z), _lib.ptr(tp), _lib.ptr(tz), _lib.ptr(anc), _lib.ptr(st), _lib.ptr(labels),
                                  _lib.ptr(tb), _lib.ptr(ts), _lib.ptr(fg), B, A, nc, R, weights[0], weights[1], weights[2], float(T),
                                  float(k_class), float(k_dfl), flags, _lib.ptr(losses), _lib.ptr(gs), _lib.ptr(gz), _lib.ptr(status),
                                  _lib.ptr(scratch), _lib.stream_ptr())
    return losses, gs, gz, status


def _combine(losses, weights, k_class, k_dfl):
    """Rule 8 without the channel-wise term: ``(loss, (wi * iou, wd * dfl_all, wc * cls_all))``."""
    wc, wi, wd = weights
    cls_all = losses[0] + losses[3] * k_class
    dfl_all = losses[2] + losses[4] * k_dfl
    loss = (cls_all * wc + losses[1] * wi) + dfl_all * wd
    return loss, torch.stack((losses[1] * wi, dfl_all * wd, cls_all * wc)).detach()


def _same_shape(a, b, what):
    if not isinstance(b, torch.Tensor) or tuple(a.shape) != tuple(b.shape):
        raise ValueError("%s must have the student's shape %s, got %s" % (what, tuple(a.shape), tuple(getattr(b, "shape", ()))))


def distill_batch(pred_scores, pred_distri, t_pred_scores, t_pred_distri, anc_points, stride, target_labels, target_bboxes,
                  target_scores, fg_mask, num_classes, temperature, epoch_num, max_epoch, reg_max=16, use_dfl=True, loss_weight=None,
                  distill_weight=None, check=False, return_status=False):
    """loss_distill.py:216-279 without the channel-wise term: ``(loss, loss_items)``, ``loss_batch``'s counterpart.  The student's
    and the teacher's pred_scores (B, A, nc) and pred_distri (B, A, 4 * (reg_max + 1)) float32; the targets as ``assign_batch``
    returns them.  ``loss`` is a float64 scalar on the predictions' device carrying ONE autograd node for the student's tensors;
    the teacher's tensors get no gradient (one that requires grad is detached).  ``loss_items`` is the detached
    ``(wi * iou, wd * dfl_all, wc * cls_all)``.  CUDA tensors take the kernels with no host read, CPU tensors ``distill_host``."""
    _dl._want_f32(pred_scores, "pred_scores")
    _dl._want_f32(pred_distri, "pred_distri")
    _dl._want_f32(t_pred_scores, "t_pred_scores")
    _dl._want_f32(t_pred_distri, "t_pred_distri")
    R, K = _dl._reg(reg_max, use_dfl)
    if pred_scores.dim() != 3 or int(pred_scores.shape[2]) != int(num_classes):
        raise ValueError("pred_scores must be (B, A, num_classes = %d), got %s" % (num_classes, tuple(pred_scores.shape)))
    _same_shape(pred_scores, t_pred_scores, "t_pred_scores")
    _same_shape(pred_distri, t_pred_distri, "t_pred_distri")
    T = _temperature(temperature)
    weights = _dl._weights(loss_weight)                                 # (the defaults of the three terms are detector_loss's)
    dw = DEFAULT_DISTILL_WEIGHT if distill_weight is None else distill_weight
    dec = decay(epoch_num, max_epoch)
    k_class, k_dfl = dec * float(dw["class"]), dec * float(dw["dfl"])
    grad = torch.is_grad_enabled() and (pred_scores.requires_grad or pred_distri.requires_grad)
    if pred_scores.is_cuda:
        losses, gs, gz, status = _distill_device(pred_scores, pred_distri, t_pred_scores, t_pred_distri, anc_points, stride, target_labels,
                                                 target_bboxes, target_scores, fg_mask, R, K, use_dfl, weights, T, k_class, k_dfl, grad)
    else:
        out = distill_host(pred_scores.detach().numpy(), pred_distri.detach().numpy(), t_pred_scores.detach().numpy(),
                           t_pred_distri.detach().numpy(), anc_points.detach().float().numpy(), stride.detach().float().numpy(),
                           target_labels.numpy(), target_bboxes.numpy(), target_scores.numpy(), fg_mask.numpy(), T, k_class, k_dfl, R,
                           use_dfl, dict(zip(("class", "iou", "dfl"), weights)))
        losses, gs, gz, status = _dl._from_host(out, grad)
    loss, items = _combine(losses, weights, k_class, k_dfl)
    return _dl._finish(pred_scores, pred_distri, loss, items, gs, gz, status, grad, check, return_status)


class _CwNode(torch.autograd.Function):
    """``d_loss_cw`` carrying the three maps' float32 gradient arrays.  The backward returns ``(g32 * grad_output).to(student's
    dtype)``: the one rounding of a 16-bit student's gradient comes after the loss scale.  ``custom_fwd`` without ``cast_inputs``
    and ``custom_bwd``: 16-bit maps stay as they are inside an autocast region, the backward runs under the forward's state."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda")
    def forward(ctx, loss, g0, g1, g2, s0, s1, s2):
        ctx.save_for_backward(g0, g1, g2)
        ctx.dtype = s0.dtype
        return loss.clone()

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_output):
        g = grad_output.to(torch.float32)
        return (None, None, None, None) + tuple((gi * g).to(ctx.dtype) if ctx.needs_input_grad[4 + i] else None
                                                for i, gi in enumerate(ctx.saved_tensors))


def _cw_device(s, t, tau, grad):
    """The C entry on three pairs of contiguous CUDA maps (the student's of one dtype, the teacher's of one):
    ``(out float64 (4,), [grad_s float32] or None)``."""
    dev = s[0].device
    lv = (_lib.CwdLevel * CW_LEVELS)()
    grads = [torch.empty(x.shape, dtype=torch.float32, device=dev) for x in s] if grad else None
    for l in range(CW_LEVELS):
        N, C, H, W = (int(v) for v in s[l].shape)
        lv[l].s, lv[l].t = s[l].data_ptr(), t[l].data_ptr()
        lv[l].grad_s = grads[l].data_ptr() if grad else None
        lv[l].n, lv[l].c, lv[l].h, lv[l].w = N, C, H, W
    out = torch.empty((4,), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        api = _lib.api()
        nbytes = api.evrep_detloss_cwd_typed_workspace_bytes(ctypes.cast(lv, ctypes.c_void_p), CW_LEVELS)
        if nbytes == 0:
            raise ValueError("distill_cw takes maps of at most 2^24 rows (N * C, all levels) of at most 2^24 values (H * W)")
        scratch = _lib.scratch(nbytes, dev)
        api.evrep_detloss_cwd_typed(ctypes.cast(lv, ctypes.c_void_p), CW_LEVELS, float(tau), 0 if grad else _lib.DETLOSS_NO_GRAD,
                                    _lib.MAP_DTYPES[s[0].dtype], _lib.MAP_DTYPES[t[0].dtype], _lib.ptr(out), _lib.ptr(scratch),
                                    _lib.stream_ptr())
    return out, grads


def _want_map(t, what, dtype, first):
    """A feature map of float32, float16 or bfloat16 (float64 keeps the loss's refusal), of the dtype of its side's first map."""
    if not isinstance(t, torch.Tensor) or t.dtype not in _lib.MAP_DTYPES:
        _dl._want_f32(t, what)
    if dtype is not None and t.dtype != dtype:
        raise ValueError("%s is %s, %s %s: the maps of one side share one dtype" % (what, t.dtype, first, dtype))
    return t.dtype


def distill_cw(s_feats, t_feats, temperature=1):
    """``distill_loss_cw`` (loss_distill.py:294-340) over the FIRST THREE maps of ``s_feats`` / ``t_feats`` ((N, C, H, W) float32,
    float16 or bfloat16, one dtype per side; further levels are ignored as the reference ignores them): a float64 scalar on the
    maps' device carrying ONE autograd node over the three student maps, whose gradients come in the student's dtype; the
    teacher's maps get no gradient.  CUDA maps take the kernel (two launches, no host read), CPU maps ``cw_host``."""
    tau = _temperature(temperature)
    if len(s_feats) < CW_LEVELS or len(t_feats) < CW_LEVELS:
        raise ValueError("distill_cw takes at least %d levels of student and teacher maps" % CW_LEVELS)
    s, t = list(s_feats[:CW_LEVELS]), list(t_feats[:CW_LEVELS])
    sdt = tdt = None
    for l in range(CW_LEVELS):
        sdt = _want_map(s[l], "s_feats[%d]" % l, sdt, "s_feats[0]")
        tdt = _want_map(t[l], "t_feats[%d]" % l, tdt, "t_feats[0]")
        if s[l].dim() != 4:
            raise ValueError("s_feats[%d] must be (N, C, H, W), got %s" % (l, tuple(s[l].shape)))
        _same_shape(s[l], t[l], "t_feats[%d]" % l)
        if t[l].device != s[l].device or s[l].device != s[0].device:
            raise ValueError("t_feats[%d] and s_feats[%d] must lie on s_feats[0]'s device" % (l, l))
    grad = torch.is_grad_enabled() and any(x.requires_grad for x in s)
    sc, tc = [x.detach().contiguous() for x in s], [x.detach().contiguous() for x in t]
    if s[0].is_cuda:
        out, grads = _cw_device(sc, tc, tau, grad)
    else:
        o, g = cw_host([x.float().numpy() for x in sc], [x.float().numpy() for x in tc], tau)      # .float(): the exact widening
        out, grads = torch.from_numpy(o), ([torch.from_numpy(x) for x in g] if grad else None)
    loss = out[0]
    if grad:
        loss = _CwNode.apply(loss, *grads, *s)
    return loss


class ComputeLossDistill(_dl.ComputeLoss):
    """``yolov6.models.losses.loss_distill.ComputeLoss`` with its constructor arguments and call signature:
    ``__call__(outputs, t_outputs, s_featmaps, t_featmaps, targets, epoch_num, max_epoch, temperature, step_num, batch_height,
    batch_width) -> (loss, loss_items)``; ``t_outputs[-2]`` and ``t_outputs[-1]`` are the teacher's pred_scores and pred_distri.
    The sequence is ``decode_boxes`` -> the assigner of the epoch (``ComputeLoss.targets_of``, with ``warmup_assigner`` and
    ``max_labels`` as there) -> ``distill_batch``, plus ``distill_cw`` when ``distill_feat``.  ``loss_items`` has four entries:
    ``wi * iou, wd * dfl_all, wc * cls_all, w_cwd * d_loss_cw``; without ``distill_feat`` the fourth is a zero on the device."""

    def __init__(self, fpn_strides=(8, 16, 32), grid_cell_size=5.0, grid_cell_offset=0.5, num_classes=80, ori_img_size=640,
                 warmup_epoch=0, use_dfl=True, reg_max=16, iou_type="giou", loss_weight=None, distill_feat=False, distill_weight=None,
                 warmup_assigner=None, max_labels=None):
        lw = dict(DEFAULT_WEIGHT if loss_weight is None else loss_weight)
        super().__init__(fpn_strides, grid_cell_size, grid_cell_offset, num_classes, ori_img_size, warmup_epoch, use_dfl, reg_max,
                         iou_type, lw, warmup_assigner, max_labels)
        self.distill_feat = bool(distill_feat)
        self.distill_weight = dict(DEFAULT_DISTILL_WEIGHT if distill_weight is None else distill_weight)
        if self.distill_feat and "cwd" not in self.loss_weight:
            raise ValueError("distill_feat needs loss_weight['cwd']")

    def __call__(self, outputs, t_outputs, s_featmaps, t_featmaps, targets, epoch_num, max_epoch, temperature, step_num, batch_height,
                 batch_width):
        feats, pred_scores, pred_distri = outputs
        t_pred_scores, t_pred_distri = t_outputs[-2], t_outputs[-1]
        _dl._want_f32(pred_scores, "pred_scores")
        _dl._want_f32(pred_distri, "pred_distri")
        _same_shape(pred_scores, t_pred_scores, "t_pred_scores")
        _same_shape(pred_distri, t_pred_distri, "t_pred_distri")
        anc, stride, labels, tb, ts, fg, st_assign = self.targets_of(feats, pred_scores, pred_distri, targets, epoch_num, batch_height,
                                                                    batch_width)
        loss, items, st = distill_batch(pred_scores, pred_distri, t_pred_scores, t_pred_distri, anc, stride, labels, tb, ts, fg,
                                        self.num_classes, temperature, epoch_num, max_epoch, self.reg_max, self.use_dfl, self.loss_weight,
                                        self.distill_weight, return_status=True)
        self.last_status = st if st_assign is None else torch.bitwise_or(st, st_assign.to(st.device))
        if self.distill_feat:
            cw = distill_cw(s_featmaps, t_featmaps) * (decay(epoch_num, max_epoch) * float(self.loss_weight["cwd"]))
            loss = loss + cw.to(loss.device)
            last = cw.detach().to(items.device).reshape(1)
        else:
            last = torch.zeros((1,), dtype=items.dtype, device=items.device)
        return loss, torch.cat((items, last))
