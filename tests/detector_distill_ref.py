"""A torch restatement of the reference's distillation losses (ev-YOLOv6/yolov6/models/losses/loss_distill.py:
ComputeLoss.__call__ :216-279, distill_loss_cls :281-292, distill_loss_cw :294-340, BboxLoss.forward :395-464 and
distill_loss_dfl :489-500), written from their statements as plain torch calls, independent of the package, run in float64
(or any dtype handed in) under torch.autograd for the gradients.  The statements loss_distill.py shares with loss.py (decode,
GIoU, _df_loss) are detector_loss_ref's.  Shared by test_detector_distill_cpu.py, test_gpu_detector_distill.py,
tools/bench_detector_distill.py and tests/golden/make_golden_detector_distill.py, which measures the reference's own float32
rounding against it.

Two departures: the reference's ``view(-1, 17)`` is ``view(-1, reg_max + 1)`` (the same at reg_max = 16, the only value the
reference is defined for), and a foreground anchor whose label lies outside [0, nc) is given the background label."""
import math

import torch
import torch.nn.functional as F

from detector_loss_ref import decode, df_loss, giou_loss


def decay(epoch_num, max_epoch):
    return ((1 - math.cos(epoch_num * math.pi / max_epoch)) / 2) * (0.01 - 1) + 1


def kd_cls(logits_student, logits_teacher, num_classes, temperature):
    s = logits_student.view(-1, num_classes)
    t = logits_teacher.view(-1, num_classes)
    ps = F.softmax(s / temperature, dim=1)
    pt = F.softmax(t / temperature, dim=1)
    return F.kl_div(torch.log(ps), pt, reduction="sum") * temperature ** 2


def kd_dfl(logits_student, logits_teacher, bins, temperature):
    s = logits_student.view(-1, bins)
    t = logits_teacher.view(-1, bins)
    ps = F.softmax(s / temperature, dim=1)
    pt = F.softmax(t / temperature, dim=1)
    return F.kl_div(torch.log(ps), pt, reduction="none").sum(1).mean() * temperature ** 2


def distill_terms(pred_scores, pred_distri, t_pred_scores, t_pred_distri, anc, stride, labels, target_bboxes, target_scores, fg, nc,
                  reg_max, use_dfl, weights, temperature, epoch_num, max_epoch, distill_weight=(1.0, 1.0), dtype=torch.float64,
                  scalars=True):
    """Tensors in; the student's predictions are cast to ``dtype`` and made leaves, the teacher's are cast.  Returns a dict:
    loss_cls, loss_iou, loss_dfl (normalised), d_loss_cls, d_loss_dfl (before the decay and the distillation weights), loss,
    tss, grad_scores, grad_distri.  ``scalars=False`` leaves the scalars as tensors."""
    wc, wi, wd = weights
    p = pred_scores.detach().to(dtype).requires_grad_(True)
    z = pred_distri.detach().to(dtype).requires_grad_(True)
    tp, tz = t_pred_scores.detach().to(dtype), t_pred_distri.detach().to(dtype)
    stride = stride.reshape(-1, 1).float()
    aps = (anc.float() / stride).to(dtype)
    pred_bboxes = decode(z, aps, reg_max, use_dfl)
    tb = target_bboxes.clone() / stride
    ts = target_scores
    fg = fg.bool()
    lab = torch.where(fg & (labels >= 0) & (labels < nc), labels, torch.full_like(labels, nc))
    one_hot = F.one_hot(lab.long(), nc + 1)[..., :-1]
    weight = 0.75 * p.pow(2.0) * (1 - one_hot) + ts * one_hot
    loss_cls = (F.binary_cross_entropy(p, ts.to(dtype), reduction="none") * weight).sum()
    tss = ts.sum()
    if tss > 0:
        loss_cls = loss_cls / tss
    if fg.sum() > 0:
        m4 = fg.unsqueeze(-1).repeat([1, 1, 4])
        pb = torch.masked_select(pred_bboxes, m4).reshape([-1, 4])
        tbp = torch.masked_select(tb, m4).reshape([-1, 4])
        bw = torch.masked_select(ts.sum(-1), fg).unsqueeze(-1)
        loss_iou = (giou_loss(pb, tbp) * bw).sum()
        if not tss == 0:
            loss_iou = loss_iou / tss
        if use_dfl:
            K = reg_max + 1
            mk = fg.unsqueeze(-1).repeat([1, 1, K * 4])
            zp = torch.masked_select(z, mk).reshape([-1, 4, K])
            tzp = torch.masked_select(tz, mk).reshape([-1, 4, K])
            x1y1, x2y2 = torch.split(tb, 2, -1)
            ltrb = torch.cat([aps - x1y1, x2y2 - aps], -1).clip(0, reg_max - 0.01)
            lp = torch.masked_select(ltrb, m4).reshape([-1, 4])
            loss_dfl = (df_loss(zp, lp, reg_max) * bw).sum()
            d_loss_dfl = (kd_dfl(zp, tzp, K, temperature) * bw).sum()
            if not tss == 0:
                loss_dfl = loss_dfl / tss
                d_loss_dfl = d_loss_dfl / tss
        else:
            loss_dfl = z.sum() * 0.0
            d_loss_dfl = z.sum() * 0.0
    else:
        loss_iou = z.sum() * 0.0
        loss_dfl = z.sum() * 0.0
        d_loss_dfl = z.sum() * 0.0
    d_loss_cls = kd_cls(p, tp, nc, temperature)
    raw_cls, raw_dfl = d_loss_cls.detach().clone(), d_loss_dfl.detach().clone()
    dec = decay(epoch_num, max_epoch)
    cls_all = loss_cls + (d_loss_cls * dec) * distill_weight[0]
    dfl_all = loss_dfl + (d_loss_dfl * dec) * distill_weight[1]
    loss = wc * cls_all + wi * loss_iou + wd * dfl_all
    loss.backward()
    out = dict(loss_cls=loss_cls.detach(), loss_iou=loss_iou.detach(), loss_dfl=loss_dfl.detach(), d_loss_cls=raw_cls, d_loss_dfl=raw_dfl,
               loss=loss.detach(), tss=tss)
    if scalars:
        out = {k: v.item() for k, v in out.items()}
    out.update(grad_scores=p.grad.detach(), grad_distri=z.grad.detach())
    return out


def cw_terms(s_feats, t_feats, temperature=1, dtype=torch.float64, scalars=True):
    """distill_loss_cw over the first three maps: a dict with loss, levels (list of three) and grads (the student maps')."""
    s = [x.detach().to(dtype).requires_grad_(True) for x in s_feats[:3]]
    t = [x.detach().to(dtype) for x in t_feats[:3]]
    levels = []
    for a, b in zip(s, t):
        N, C, H, W = a.shape
        levels.append(F.kl_div(F.log_softmax(a.view(N, C, H * W) / temperature, dim=2),
                               F.log_softmax(b.view(N, C, H * W) / temperature, dim=2), reduction="sum", log_target=True)
                      * (temperature * temperature) / (N * C))
    loss = levels[0] + levels[1] + levels[2]
    loss.backward()
    if scalars:
        return dict(loss=loss.item(), levels=[v.item() for v in levels], grads=[a.grad.detach() for a in s])
    return dict(loss=loss.detach(), levels=[v.detach() for v in levels], grads=[a.grad for a in s])
