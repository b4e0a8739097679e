"""A torch restatement of the reference's loss terms (ev-YOLOv6/yolov6/models/losses/loss.py:176-217 with VarifocalLoss,
BboxLoss, bbox_decode, general.py's dist2bbox / bbox2dist and figure_iou.py's IOUloss(xyxy, giou, eps=1e-10)), written from
their statements as plain torch calls, independent of the package, run in float64 (or any dtype handed in) under
torch.autograd for the gradients.  Shared by test_detector_loss_cpu.py, test_gpu_detector_loss.py and
tests/golden/make_golden_detector_loss.py, which measures the reference's own float32 rounding against it.

One departure, stated in include/evrep.h: a foreground anchor whose label lies outside [0, nc) is given the background label
nc before the one-hot (the reference's one_hot raises there)."""
import torch
import torch.nn.functional as F


def decode(pred_distri, aps, reg_max, use_dfl):
    """bbox_decode: softmax over the reg_max + 1 bins, the expectation by a matmul with linspace(0, reg_max), dist2bbox."""
    d = pred_distri
    if use_dfl:
        B, A, _ = d.shape
        proj = torch.linspace(0, reg_max, reg_max + 1).to(d.dtype).to(d.device)
        d = F.softmax(d.view(B, A, 4, reg_max + 1), dim=-1).matmul(proj)
    lt, rb = torch.split(d, 2, -1)
    return torch.cat([aps - lt, aps + rb], -1)


def giou_loss(b1, b2, eps=1e-10):
    x1, y1, x2, y2 = torch.split(b1, 1, dim=-1)
    tx1, ty1, tx2, ty2 = torch.split(b2, 1, dim=-1)
    inter = (torch.min(x2, tx2) - torch.max(x1, tx1)).clamp(0) * (torch.min(y2, ty2) - torch.max(y1, ty1)).clamp(0)
    w1, h1 = x2 - x1, y2 - y1 + eps
    w2, h2 = tx2 - tx1, ty2 - ty1 + eps
    union = w1 * h1 + w2 * h2 - inter + eps
    iou = inter / union
    cw = torch.max(x2, tx2) - torch.min(x1, tx1)
    ch = torch.max(y2, ty2) - torch.min(y1, ty1)
    c_area = cw * ch + eps
    return 1.0 - (iou - (c_area - union) / c_area)


def df_loss(pred_dist, target, reg_max):
    left = target.to(torch.long)
    right = left + 1
    wl = right.to(torch.float) - target
    wr = 1 - wl
    flat = pred_dist.view(-1, reg_max + 1)
    ll = F.cross_entropy(flat, left.view(-1), reduction="none").view(left.shape) * wl
    lr = F.cross_entropy(flat, right.view(-1), reduction="none").view(left.shape) * wr
    return (ll + lr).mean(-1, keepdim=True)


def loss_terms(pred_scores, pred_distri, anc, stride, labels, target_bboxes, target_scores, fg, nc, reg_max, use_dfl, weights,
               dtype=torch.float64, scalars=True):
    """Tensors in; predictions are cast to ``dtype`` and made leaves.  Returns a dict: loss_cls, loss_iou, loss_dfl (floats of
    the normalised, unweighted terms), loss, tss, pred_bboxes, grad_scores, grad_distri (tensors of ``dtype``).  ``scalars=False``
    leaves the five scalars as tensors: no read of the device beyond the reference's own two (``tss > 1``, ``num_pos > 0``)."""
    wc, wi, wd = weights
    p = pred_scores.detach().to(dtype).requires_grad_(True)
    z = pred_distri.detach().to(dtype).requires_grad_(True)
    stride = stride.reshape(-1, 1).float()
    aps = (anc.float() / stride).to(dtype)                             # the float32 quotient, widened
    pred_bboxes = decode(z, aps, reg_max, use_dfl)
    tb = target_bboxes.clone() / stride
    ts = target_scores
    fg = fg.bool()
    lab = torch.where(fg & (labels >= 0) & (labels < nc), labels, torch.full_like(labels, nc))
    one_hot = F.one_hot(lab.long(), nc + 1)[..., :-1]
    weight = 0.75 * p.pow(2.0) * (1 - one_hot) + ts * one_hot
    loss_cls = (F.binary_cross_entropy(p, ts.to(dtype), reduction="none") * weight).sum()
    tss = ts.sum()
    if tss > 1:
        loss_cls = loss_cls / tss
    if fg.sum() > 0:
        m4 = fg.unsqueeze(-1).repeat([1, 1, 4])
        pb = torch.masked_select(pred_bboxes, m4).reshape([-1, 4])
        tp = torch.masked_select(tb, m4).reshape([-1, 4])
        bw = torch.masked_select(ts.sum(-1), fg).unsqueeze(-1)
        loss_iou = (giou_loss(pb, tp) * bw).sum()
        if tss > 1:
            loss_iou = loss_iou / tss
        if use_dfl:
            mk = fg.unsqueeze(-1).repeat([1, 1, (reg_max + 1) * 4])
            zp = torch.masked_select(z, mk).reshape([-1, 4, reg_max + 1])
            x1y1, x2y2 = torch.split(tb, 2, -1)
            ltrb = torch.cat([aps - x1y1, x2y2 - aps], -1).clip(0, reg_max - 0.01)
            lp = torch.masked_select(ltrb, m4).reshape([-1, 4])
            loss_dfl = (df_loss(zp, lp, reg_max) * bw).sum()
            if tss > 1:
                loss_dfl = loss_dfl / tss
        else:
            loss_dfl = z.sum() * 0.0
    else:
        loss_iou = z.sum() * 0.0
        loss_dfl = z.sum() * 0.0
    loss = wc * loss_cls + wi * loss_iou + wd * loss_dfl
    loss.backward()
    if not scalars:
        return dict(loss_cls=loss_cls.detach(), loss_iou=loss_iou.detach(), loss_dfl=loss_dfl.detach(), loss=loss.detach(), tss=tss,
                    pred_bboxes=pred_bboxes.detach(), grad_scores=p.grad, grad_distri=z.grad)
    return dict(loss_cls=loss_cls.item(), loss_iou=loss_iou.item(), loss_dfl=loss_dfl.item(), loss=loss.item(), tss=tss.item(),
                pred_bboxes=pred_bboxes.detach(), grad_scores=p.grad.detach(), grad_distri=z.grad.detach())
