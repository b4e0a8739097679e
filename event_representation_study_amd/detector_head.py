"""The head's outputs on the device: what the reference's ``Detect.forward`` does behind its last convolutions.

``ev-YOLOv6/yolov6/models/effidehead.py:111-173`` turns the per-level maps of ``cls_preds`` / ``reg_preds`` into the prediction
tensor ``(B, N, 5 + nc)`` with, per level, a reshape, a permute, a softmax over the ``reg_max + 1`` bins, a 1 x 1 convolution with
the weights ``0 .. reg_max`` and a sigmoid, then two concatenations, two permutes, ``generate_anchors(is_eval=True)``,
``dist2bbox(..., "xywh")``, a multiply by the stride tensor, a ``torch.ones`` and a last ``torch.cat``; the training branch
(``:90-110``) is a sigmoid per level and four copies through ``flatten / permute / cat``, replayed by autograd backwards.  Here
``predict`` is one launch (``evrep_dethead_predict``, csrc/evrep_dethead.hip), ``train_outputs`` one launch forward and one
backward, and ``predict_batch`` hands the prediction tensor on to ``detector_output.nms_batch`` with no host read.  The
``*_host`` functions are the same rules in numpy: the oracle of the kernels and the route of CPU tensors.

The rules (include/evrep.h states them with ``evrep_dethead_predict``).  Level ``l`` has a map of ``h_l x w_l``, ``n_l = h_l * w_l``
anchors, offset ``off_l`` and stride ``s_l``; anchor ``a = off_l + i * w_l + j`` has the point ``ax = j + 0.5``, ``ay = i + 0.5``.
``cls_l`` is ``[B, nc, h_l, w_l]`` (raw logits), ``reg_l`` ``[B, 4K, h_l, w_l]`` with channel ``side * K + k``, float32 or 16-bit (below),
K = ``reg_max + 1`` with DFL and 1 without.  Every statement of E1-E4 is one float64 operation on exactly widened inputs.

E1. The side distance ``d`` is rule 1 of ``detector_loss`` (``m``, ``e_k``, ``Z``, ``pr_k``, ``d`` added left to right); without DFL ``d = z``.
E2. ``x1 = ax - d_0``, ``y1 = ay - d_1``, ``x2 = ax + d_2``, ``y2 = ay + d_3``; ``cx = (x1 + x2) / 2``, ``cy`` likewise, ``w = x2 - x1``,
    ``h = y2 - y1``; each times ``s_l``, rounded once to float32 into ``pred[b, a, 0:4]``.
E3. ``pred[b, a, 4] = 1``.
E4. ``pred[b, a, 5 + c] = fl32(1 / (1 + exp(-x)))``, ``x = cls_l[b, c, i, j]``.
T1. ``pred_scores[b, a, c]`` is the value of E4.   T2. ``pred_distri[b, a, ch] = reg_l[b, ch, i, j]``, a bit copy.
Backward, float32, one operation per statement (torch's ``sigmoid_backward`` on the stored output):
``gcls_l[b, c, i, j] = (g * (1 - p)) * p``; ``greg_l[b, ch, i, j] = grad_distri[b, a, ch]``.

16-bit maps (training under ``torch.autocast``, evaluation with ``model.half()``): the 2L maps of a call may be float16 or
bfloat16 instead of float32, all of one dtype, and go into the same launches as they are (``evrep_dethead_*_typed``).
W1. A 16-bit element is widened exactly to float32 at its load (float16 by IEEE conversion, bfloat16 by its 16 bits on top of
    16 zero bits; subnormals and -0.0 keep value and sign), and E1-E4 / T1 run on that; T2 is the exact widening.  So
    ``predict`` and ``train_outputs`` give the bits they give for ``map.float()``, and all outputs stay float32.
W2. The backward forms its float32 value as above and rounds it once, to nearest even, to the maps' dtype at the store
    (overflow to +-inf, which the scaler's ``found_inf`` exists for; a NaN stays a NaN): ``float32_gradient.to(dtype)`` bit for
    bit wherever it is no NaN.  The gradient maps are allocated in the maps' dtype and handed to autograd as they are.
CPU maps of a 16-bit dtype take the host mirrors on ``map.float()`` and return ``.to(dtype)`` gradients.

Inputs must be finite.  float64 maps, ``Detect.export``, the anchor-based and distillation heads and a ``proj`` other than
``linspace(0, reg_max, reg_max + 1)`` are not mirrored; ``pred_scores`` / ``pred_distri`` and everything behind them stay float32.
"""
import numpy as np
import torch

from . import _lib
from .detector_loss import _max, _reg

F32, F64 = np.float32, np.float64
TILE = _lib.DETHEAD_TILE
MAX_LEVELS = _lib.DETHEAD_MAX_LEVELS


# ---------------------------------------------------------------------------------------------------------------- the checks
def _levels(cls_maps, reg_maps, K, strides=None, nc=None):
    """The refusals of this module, each naming the level.  Returns (B, nc, [(h, w)], device)."""
    cls_maps, reg_maps = list(cls_maps), list(reg_maps)
    L = len(cls_maps)
    if not 1 <= L <= MAX_LEVELS or len(reg_maps) != L:
        raise ValueError("the head takes 1..%d levels and as many reg maps as cls maps, got %d and %d" % (MAX_LEVELS, L, len(reg_maps)))
    if strides is not None and len(strides) != L:
        raise ValueError("%d strides for %d levels" % (len(strides), L))
    dev, B, shapes, dtype = None, None, [], None
    for l, (c, r) in enumerate(zip(cls_maps, reg_maps)):
        for name, t in (("cls", c), ("reg", r)):
            what = "level %d: %s map" % (l, name)
            if not isinstance(t, torch.Tensor) or t.dtype not in _lib.MAP_DTYPES:
                raise ValueError("%s is %s: the head takes float32, float16 or bfloat16 maps (float64 is not mirrored), call .float() "
                                 "on it first" % (what, getattr(t, "dtype", type(t).__name__)))
            if dtype is None:
                dtype = t.dtype
            elif t.dtype != dtype:
                raise ValueError("%s is %s, level 0's cls map %s: all maps of a call share one dtype" % (what, t.dtype, dtype))
            if t.dim() != 4:
                raise ValueError("%s must be (B, C, h, w), got %s" % (what, tuple(t.shape)))
            if not t.is_contiguous():
                raise ValueError("%s is not contiguous in NCHW order (channels_last included): call .contiguous() on it first" % what)
            if dev is None:
                dev = t.device
            elif t.device != dev:
                raise ValueError("%s is on %s, level 0's cls map on %s: all maps must share a device" % (what, t.device, dev))
        if nc is None:
            nc = int(c.shape[1])
        if B is None:
            B = int(c.shape[0])
        h, w = int(c.shape[2]), int(c.shape[3])
        if tuple(c.shape) != (B, nc, h, w) or min(h, w) < 1:
            raise ValueError("level %d: cls map must be (%d, nc = %d, h, w), got %s" % (l, B, nc, tuple(c.shape)))
        if tuple(r.shape) != (B, 4 * K, h, w):
            raise ValueError("level %d: reg map must be (%d, 4K = %d, %d, %d) to go with its cls map, got %s"
                             % (l, B, 4 * K, h, w, tuple(r.shape)))
        shapes.append((h, w))
    N = sum(h * w for h, w in shapes)
    if not (1 <= B <= 65535 and 1 <= nc <= _lib.TAL_MAX_CLASSES and N <= _lib.TAL_MAX_ANCHORS):
        raise ValueError("the head takes 1 <= B <= 65535, 1 <= nc <= %d and N <= 2^24, got B = %d, nc = %d, N = %d"
                         % (_lib.TAL_MAX_CLASSES, B, nc, N))
    if strides is not None:
        for l, s in enumerate(strides):
            if not (np.isfinite(F32(s)) and F32(s) > 0):
                raise ValueError("level %d: stride %r must be finite and > 0" % (l, s))
    return B, nc, shapes, dev


# ------------------------------------------------------------------------------------------------------------ the host route
def _side_host(z):
    """E1 for z (..., K) float64: rule 1 of detector_loss.decode_host, the additions left to right."""
    K = z.shape[-1]
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
    return d


def _sigmoid_host(x32):
    with np.errstate(all="ignore"):
        return (1.0 / (1.0 + np.exp(-x32.astype(F64)))).astype(F32)


def _np_maps(maps):
    """float32 arrays of the maps; a 16-bit tensor is widened exactly by ``.float()`` (numpy has no bfloat16)."""
    return [np.ascontiguousarray(m.detach().cpu().float().numpy() if isinstance(m, torch.Tensor) else m, dtype=F32) for m in maps]


def predict_host(cls_maps, reg_maps, strides=(8, 16, 32), reg_max=16, use_dfl=True):
    """E1-E4 in numpy float64: lists of L arrays (B, nc, h, w) and (B, 4K, h, w) float32 -> pred (B, N, 5 + nc) float32."""
    R, K = _reg(reg_max, use_dfl)
    cls_maps, reg_maps = _np_maps(cls_maps), _np_maps(reg_maps)
    out = []
    with np.errstate(all="ignore"):
        for c, r, s in zip(cls_maps, reg_maps, strides):
            B, nc, h, w = c.shape
            n = h * w
            z = r.reshape(B, 4, K, n).astype(F64).transpose(0, 3, 1, 2)           # (B, n, 4, K)
            d = _side_host(z) if use_dfl else z[..., 0]
            a = np.arange(n)
            ax, ay = (a % w).astype(F64) + 0.5, (a // w).astype(F64) + 0.5
            x1, y1, x2, y2 = ax - d[..., 0], ay - d[..., 1], ax + d[..., 2], ay + d[..., 3]
            s64 = F64(F32(s))
            box = np.stack([((x1 + x2) / 2.0) * s64, ((y1 + y2) / 2.0) * s64, (x2 - x1) * s64, (y2 - y1) * s64], axis=-1).astype(F32)
            p = _sigmoid_host(c.reshape(B, nc, n)).transpose(0, 2, 1)
            out.append(np.concatenate([box, np.ones((B, n, 1), F32), p], axis=-1))
    return np.ascontiguousarray(np.concatenate(out, axis=1))


def train_outputs_host(cls_maps, reg_maps, reg_max=16, use_dfl=True):
    """T1, T2 in numpy: ``(pred_scores (B, A, nc), pred_distri (B, A, 4K))`` float32."""
    _reg(reg_max, use_dfl)
    cls_maps, reg_maps = _np_maps(cls_maps), _np_maps(reg_maps)
    ps = [_sigmoid_host(c.reshape(c.shape[0], c.shape[1], -1)).transpose(0, 2, 1) for c in cls_maps]
    pd = [r.reshape(r.shape[0], r.shape[1], -1).transpose(0, 2, 1) for r in reg_maps]
    return np.ascontiguousarray(np.concatenate(ps, axis=1)), np.ascontiguousarray(np.concatenate(pd, axis=1))


def train_backward_host(pred_scores, grad_scores, grad_distri, shapes):
    """The backward rules in numpy float32: the stored scores (B, A, nc), the two gradients (either may be None) and the levels'
    (h, w) -> ``(gcls list, greg list)`` of (B, nc, h, w) and (B, 4K, h, w) arrays (None for a half that was not given)."""
    gcls = greg = None
    if grad_scores is not None:
        p, g = np.asarray(pred_scores, dtype=F32), np.asarray(grad_scores, dtype=F32)
        with np.errstate(all="ignore"):
            v = ((g * (F32(1.0) - p)).astype(F32) * p).astype(F32)
        gcls, off = [], 0
        for h, w in shapes:
            gcls.append(np.ascontiguousarray(v[:, off:off + h * w].transpose(0, 2, 1)).reshape(v.shape[0], v.shape[2], h, w))
            off += h * w
    if grad_distri is not None:
        g = np.asarray(grad_distri, dtype=F32)
        greg, off = [], 0
        for h, w in shapes:
            greg.append(np.ascontiguousarray(g[:, off:off + h * w].transpose(0, 2, 1)).reshape(g.shape[0], g.shape[2], h, w))
            off += h * w
    return gcls, greg


# ---------------------------------------------------------------------------------------------------------- the device route
def _level_table(cls_maps, reg_maps, shapes, strides):
    table = (_lib.DetheadLevel * len(shapes))()
    for l, ((h, w), c, r) in enumerate(zip(shapes, cls_maps, reg_maps)):
        table[l] = _lib.DetheadLevel(c.data_ptr(), r.data_ptr(), h, w, float(strides[l]))
    return table


def _flags(use_dfl):
    return _lib.DETHEAD_USE_DFL if use_dfl else 0


def _dt(maps):
    """The dtype code of the call: that of its first map (``_levels`` has held the others to it)."""
    return _lib.MAP_DTYPES[maps[0].dtype]


def predict(cls_maps, reg_maps, strides=(8, 16, 32), reg_max=16, use_dfl=True, out=None):
    """``Detect.forward`` in evaluation, behind the convolutions: lists of L maps ``cls_l (B, nc, h_l, w_l)`` (raw logits) and
    ``reg_l (B, 4K, h_l, w_l)`` float32 -> ``pred (B, N, 5 + nc)`` float32 ``[cx, cy, w, h, 1, scores]`` in pixels.  CUDA maps take
    the kernel: one launch, no host read (``out``: a tensor to write into); CPU maps take ``predict_host``.  No gradient."""
    R, K = _reg(reg_max, use_dfl)
    B, nc, shapes, dev = _levels(cls_maps, reg_maps, K, strides)
    N = sum(h * w for h, w in shapes)
    if dev.type != "cuda":
        res = torch.from_numpy(predict_host(cls_maps, reg_maps, strides, R, use_dfl))
        return res if out is None else out.copy_(res)
    cls_maps, reg_maps = [c.detach() for c in cls_maps], [r.detach() for r in reg_maps]
    if out is None:
        out = torch.empty((B, N, 5 + nc), dtype=torch.float32, device=dev)
    else:
        _lib.want(out, "out", torch.float32, shape=(B, N, 5 + nc), device=dev)
    with torch.cuda.device(dev):
        _lib.api().evrep_dethead_predict_typed(_level_table(cls_maps, reg_maps, shapes, strides), len(shapes), B, nc, R, _flags(use_dfl),
                                               _dt(cls_maps), _lib.ptr(out), _lib.stream_ptr())
    return out


def _train_device(cls_maps, reg_maps, shapes, B, nc, R, K, use_dfl, dev, scores=None, distri=None):
    N = sum(h * w for h, w in shapes)
    scores = torch.empty((B, N, nc), dtype=torch.float32, device=dev) if scores is None else scores
    distri = torch.empty((B, N, 4 * K), dtype=torch.float32, device=dev) if distri is None else distri
    with torch.cuda.device(dev):
        _lib.api().evrep_dethead_train_typed(_level_table(cls_maps, reg_maps, shapes, [1.0] * len(shapes)), len(shapes), B, nc, R,
                                             _flags(use_dfl), _dt(cls_maps), _lib.ptr(scores), _lib.ptr(distri), _lib.stream_ptr())
    return scores, distri


def _backward_device(pred_scores, grad_scores, grad_distri, shapes, B, nc, R, K, use_dfl, dev, gcls=None, greg=None,
                     dtype=torch.float32):
    """The backward launch: new maps of ``dtype`` (or the given ones, whose dtype then counts) for the halves whose gradient is
    not None.  The float32 value is rounded once to the maps' dtype at the store."""
    given = [g for g in (gcls, greg) if g is not None]
    if given:
        dtype = given[0][0].dtype
        if any(m.dtype != dtype for g in given for m in g) or dtype not in _lib.MAP_DTYPES:
            raise ValueError("the gradient maps of a call share one dtype of float32, float16, bfloat16")
    if grad_scores is not None and gcls is None:
        gcls = [torch.empty((B, nc, h, w), dtype=dtype, device=dev) for h, w in shapes]
    if grad_distri is not None and greg is None:
        greg = [torch.empty((B, 4 * K, h, w), dtype=dtype, device=dev) for h, w in shapes]
    table = (_lib.DetheadGradLevel * len(shapes))()
    for l, (h, w) in enumerate(shapes):
        table[l] = _lib.DetheadGradLevel(gcls[l].data_ptr() if grad_scores is not None else None,
                                         greg[l].data_ptr() if grad_distri is not None else None, h, w)
    with torch.cuda.device(dev):
        _lib.api().evrep_dethead_train_backward_typed(table, len(shapes), B, nc, R, _flags(use_dfl), _lib.MAP_DTYPES[dtype],
                                                      _lib.ptr(pred_scores) if grad_scores is not None else None,
                                                      _lib.ptr(grad_scores), _lib.ptr(grad_distri), _lib.stream_ptr())
    return (gcls if grad_scores is not None else None), (greg if grad_distri is not None else None)


class _TrainOutputs(torch.autograd.Function):
    """(pred_scores, pred_distri) of the maps; the backward is the backward launch and returns a gradient per map, in the maps'
    dtype.  ``custom_fwd`` without ``cast_inputs`` leaves 16-bit maps as they are inside an autocast region (a cast to float32
    is the launch this node saves) and ``custom_bwd`` runs the backward under the forward's autocast state; neither launch is
    a torch operator, so autocast changes no bit of either."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda")
    def forward(ctx, meta, *maps):
        L, R, use_dfl = meta
        K = R + 1 if use_dfl else 1
        cls_maps, reg_maps = maps[:L], maps[L:]
        B, nc, shapes, dev = _levels(cls_maps, reg_maps, K)
        if dev.type == "cuda":
            scores, distri = _train_device(cls_maps, reg_maps, shapes, B, nc, R, K, use_dfl, dev)
        else:
            scores, distri = (torch.from_numpy(a) for a in train_outputs_host(cls_maps, reg_maps, R, use_dfl))
        ctx.save_for_backward(scores)
        ctx.set_materialize_grads(False)                                 # an output the loss does not use arrives as None
        ctx.meta = (L, R, K, use_dfl, B, nc, shapes, dev, maps[0].dtype)
        return scores, distri

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_scores, grad_distri):
        L, R, K, use_dfl, B, nc, shapes, dev, dtype = ctx.meta
        scores, = ctx.saved_tensors
        need_c, need_r = any(ctx.needs_input_grad[1:1 + L]), any(ctx.needs_input_grad[1 + L:])
        gs = grad_scores.to(torch.float32).contiguous() if (grad_scores is not None and need_c) else None
        gd = grad_distri.to(torch.float32).contiguous() if (grad_distri is not None and need_r) else None
        gcls = greg = None
        if gs is not None or gd is not None:
            if dev.type == "cuda":
                gcls, greg = _backward_device(scores, gs, gd, shapes, B, nc, R, K, use_dfl, dev, dtype=dtype)
            else:
                gcls, greg = train_backward_host(scores.numpy(), None if gs is None else gs.numpy(), None if gd is None else gd.numpy(),
                                                 shapes)
                gcls = None if gcls is None else [torch.from_numpy(g).to(dtype) for g in gcls]      # the one rounding
                greg = None if greg is None else [torch.from_numpy(g).to(dtype) for g in greg]
        none = [None] * L
        return (None,) + tuple(gcls or none) + tuple(greg or none)


def train_outputs(cls_maps, reg_maps, reg_max=16, use_dfl=True):
    """``Detect.forward`` in training, behind the convolutions: ``(pred_scores (B, A, nc), pred_distri (B, A, 4K))`` float32, what
    ``detector_loss.ComputeLoss`` takes in ``outputs``.  One autograd node: one launch forward, one backward, a gradient per map
    (an output that takes no part in the loss costs nothing).  CPU maps take the host functions."""
    R, K = _reg(reg_max, use_dfl)
    cls_maps, reg_maps = list(cls_maps), list(reg_maps)
    _levels(cls_maps, reg_maps, K)
    return _TrainOutputs.apply((len(cls_maps), R, bool(use_dfl)), *cls_maps, *reg_maps)


def predict_batch(cls_maps, reg_maps, conf_thres=0.25, iou_thres=0.45, classes=None, agnostic=False, multi_label=False, max_det=300,
                  strides=(8, 16, 32), reg_max=16, use_dfl=True):
    """``nms_batch(predict(...))``: the maps of the convolutions -> ``(det (B, max_det, 6), count (B,))`` on the device, two
    launches, no host read."""
    from .detector_output import nms_batch
    return nms_batch(predict(cls_maps, reg_maps, strides, reg_max, use_dfl), conf_thres, iou_thres, classes, agnostic, multi_label,
                     max_det)


class DetectTail(torch.nn.Module):
    """What ``Detect.forward`` returns behind its convolutions, without parameters: ``forward(cls_maps, reg_maps)`` gives
    ``(pred_scores, pred_distri)`` when ``self.training`` and ``pred`` otherwise.  The DFL projection ``linspace(0, reg_max,
    reg_max + 1)`` is built into the kernel; ``check_proj`` holds a checkpoint's ``proj_conv.weight`` to it."""

    def __init__(self, num_classes, strides=(8, 16, 32), use_dfl=True, reg_max=16):
        super().__init__()
        self.num_classes, self.strides = int(num_classes), tuple(float(s) for s in strides)
        self.use_dfl, self.reg_max = bool(use_dfl), int(reg_max)
        _reg(self.reg_max, self.use_dfl)

    def check_proj(self, weight):
        """ValueError unless ``weight`` (``proj`` or ``proj_conv.weight`` of a checkpoint) is ``linspace(0, R, R + 1)``."""
        R = self.reg_max
        w = torch.as_tensor(weight).detach().reshape(-1).double().cpu()
        if w.numel() != R + 1 or not torch.equal(w, torch.arange(R + 1, dtype=torch.float64)):
            raise ValueError("proj_conv.weight is not linspace(0, %d, %d): the kernel builds that projection in and mirrors no other"
                             % (R, R + 1))

    def forward(self, cls_maps, reg_maps):
        cls_maps = list(cls_maps)
        for l, c in enumerate(cls_maps):
            if isinstance(c, torch.Tensor) and c.dim() == 4 and int(c.shape[1]) != self.num_classes:
                raise ValueError("level %d: cls map has %d channels, the head %d classes" % (l, int(c.shape[1]), self.num_classes))
        if len(cls_maps) != len(self.strides):
            raise ValueError("%d levels for %d strides" % (len(cls_maps), len(self.strides)))
        if self.training:
            return train_outputs(cls_maps, reg_maps, self.reg_max, self.use_dfl)
        return predict(cls_maps, reg_maps, self.strides, self.reg_max, self.use_dfl)
