"""Row F4 (second half): the EST quantisation layer of ev-YOLOv6, forward and backward.

Mirror of ``QuantizationLayer.forward`` (ev-YOLOv6/yolov6/models/learned_repr.py:143-179): events
``(N, 5)`` rows ``[x, y, t, p, b]`` -> per batch item, polarity and time bin i the image
``sum_events t_n * f(t_n - i/(C-1))`` with ``t_n = t / t.max()`` (:159-160) and ``f`` the layer's value MLP
(1 -> 100 -> 100 -> 1, LeakyReLU(0.1), :9-43), channels ``[p*C + i]`` (:175-176), letterboxed to
``image_size`` with bilinear interpolation and the constant 114 (:93-136).

The MLP is a scalar function of a scalar with piecewise-linear activations, hence EXACTLY piecewise linear:
``PiecewiseLinearKernel`` derives its breakpoints in closed form from the weights (the kinks of the first
layer, then the zero crossings of every second-layer pre-activation inside each first-layer piece) and the
HIP builder (k_est) evaluates ``f`` by a bucketed breakpoint search + one fused multiply-add in float64 --
~10^4 multiply-adds per (event, bin) become a table lookup, and the layer is a per-pixel segmented
reduction on the binned stream like every other builder.

The layer is trainable here.  On piece k the MLP is ``f(u) = a_k u + c_k`` and (a_k, c_k) are smooth functions of the
six weight tensors while every piece keeps its activation pattern, so the backward on the device is a gather of
dL/dvox at each event's voxels plus a keyed float64 reduction into 2 * pieces numbers (k_est_bwd, bit-reproducible,
no floating-point atomics), and torch autograd carries (dL/da, dL/dc) on to the weights through ``piece_coefficients``.
``TrainableQuantizationLayer`` is the nn.Module (``ValueLayer`` holds the parameters under the reference's state-dict
keys); it rebuilds the table from the current weights on every forward.  The events get no gradient: t is data.

Differences, all on the safe side: pixel/voxel indices are exact integers (the reference forms them in
float32, :163, which loses bits beyond 2**24 voxels, i.e. for more than ~19 batch items of 6x240x304); p must
be in {0, 1} (a p of -1 makes the reference clamp negative indices onto voxel 0, :170); the caller's events
tensor is not modified (the reference normalises ``t`` in place through a view, :156-160).

A CUDA ``(N, 5)`` tensor on the layer's device is prepared on the device (``prepare_events_device``, evrep_est_prepare): the
int32 rows, the offsets and ``t / t.max()`` are formed there and only (B + 2) words come back, bit-equal to the host route
that every other input takes.  Two corners of the device route differ, both declared: non-finite coordinates raise
IndexError (the host route casts them with numpy, which is undefined for NaN), and an item whose maximum is a zero while it
also holds negative times is unspecified (torch does not define which zero ``max`` returns; the device takes +0).
"""
import numpy as np
import torch

from . import _lib
from .engine import EventBatch

NEG_SLOPE = 0.1


def mlp_weights(value_layer):
    """(w1, b1, W2, b2, w3, b3) float64 arrays of a ValueLayer-like module (``.mlp`` = three nn.Linear) or of a
    state dict with keys mlp.{0,1,2}.{weight,bias}."""
    sd = value_layer if isinstance(value_layer, dict) else value_layer.state_dict()
    g = lambda k: np.asarray(sd[k].detach().cpu().numpy() if hasattr(sd[k], "detach") else sd[k], dtype=np.float64)  # noqa: E731
    w1, b1 = g("mlp.0.weight").reshape(-1), g("mlp.0.bias").reshape(-1)
    W2, b2 = g("mlp.1.weight"), g("mlp.1.bias").reshape(-1)
    w3, b3 = g("mlp.2.weight").reshape(-1), float(g("mlp.2.bias").reshape(-1)[0])
    if W2.shape != (len(b2), len(w1)) or len(w3) != len(b2):
        raise ValueError("expected a 1 -> n -> m -> 1 MLP")
    return w1, b1, W2, b2, w3, b3


def _leaky(z, slope=NEG_SLOPE):
    return np.where(z > 0, z, slope * z)


def bucket_table(ends, lo, hi, nbucket):
    """The hint table of k_est: [lo, hi) in ``nbucket`` equal buckets, entry g = the first piece whose end
    (``ends[k]``, ascending; piece k covers u < ends[k]) lies beyond the bucket's left edge, at most the last piece.
    The kernel starts its forward walk there, so an entry may be too small but never too large."""
    ends = np.asarray(ends, dtype=np.float64)
    left = lo + (hi - lo) * np.arange(int(nbucket)) / int(nbucket)
    bucket = np.searchsorted(ends, left, side="right")          # first piece whose end > left edge
    return np.minimum(bucket, len(ends) - 1).astype(np.int32)


def _piece_forms(weights, mids, slope):
    """Slope and intercept of every piece from the activation pattern at its midpoint (exact: no kink inside), and the
    intermediates the gradient needs: (a, c, a1, a2, A2, B2)."""
    w1, b1, W2, b2, w3, b3 = weights
    a1 = np.where(np.outer(mids, w1) + b1 > 0, 1.0, slope)             # (pieces, n1)
    A2 = (a1 * w1) @ W2.T                                              # d z2 / du
    B2 = (a1 * b1) @ W2.T + b2
    a2 = np.where(A2 * mids[:, None] + B2 > 0, 1.0, slope)
    return (a2 * A2) @ w3, (a2 * B2) @ w3 + b3, a1, a2, A2, B2


class PiecewiseLinearKernel:
    """f(u) = w3 . leaky(W2 leaky(w1 u + b1) + b2) + b3 on [lo, hi] as sorted breakpoints + per-piece (a, c)."""

    def __init__(self, weights, lo=-1.0, hi=1.0, nbucket=4096, slope=NEG_SLOPE):
        w1, b1, W2, b2, w3, b3 = weights
        self.weights, self.lo, self.hi, self.slope = weights, float(lo), float(hi), float(slope)
        with np.errstate(divide="ignore", invalid="ignore"):
            k1 = -b1 / w1                                     # kinks of the first layer
        k1 = k1[np.isfinite(k1) & (k1 > lo) & (k1 < hi)]
        edges = np.concatenate([[lo], np.sort(k1), [hi]])
        kinks = [k1]
        for a, b in zip(edges[:-1], edges[1:]):                # inside (a, b) the first layer is linear in u
            if not b > a:
                continue
            mid = 0.5 * (a + b)
            alpha = np.where(w1 * mid + b1 > 0, 1.0, slope)    # which side of its kink each neuron is on
            A = W2 @ (alpha * w1)                              # z2_k(u) = A_k u + B_k on this piece
            Bc = W2 @ (alpha * b1) + b2
            with np.errstate(divide="ignore", invalid="ignore"):
                z = -Bc / A
            kinks.append(z[np.isfinite(z) & (z > a) & (z < b)])
        bp = np.unique(np.concatenate(kinks))
        self.edges = np.concatenate([[lo], bp, [hi]])          # piece k = [edges[k], edges[k+1])
        mids = 0.5 * (self.edges[:-1] + self.edges[1:])
        self.a, self.c = _piece_forms(weights, mids, slope)[:2]
        self.nbucket = int(nbucket)
        self.bucket = bucket_table(self.edges[1:], lo, hi, self.nbucket)
        self._dev = {}

    def __len__(self):
        return len(self.a)

    def __call__(self, u):
        """float64 evaluation through the table (host; what the HIP builder computes)."""
        u = np.asarray(u, dtype=np.float64)
        k = np.clip(np.searchsorted(self.edges[1:-1], u, side="right"), 0, len(self.a) - 1)
        return self.a[k] * u + self.c[k]

    def mlp(self, u):
        """The MLP itself in float64 (ground truth for the table)."""
        w1, b1, W2, b2, w3, b3 = self.weights
        u = np.asarray(u, dtype=np.float64).reshape(-1)
        h1 = _leaky(np.outer(u, w1) + b1, self.slope)
        h2 = _leaky(h1 @ W2.T + b2, self.slope)
        return h2 @ w3 + b3

    def device_table(self, device):
        key = str(device)
        if key not in self._dev:
            seg = np.stack([self.edges[1:], self.a, self.c], axis=1)       # {u_next, a, c}
            self._dev[key] = (torch.from_numpy(np.ascontiguousarray(seg)).to(device),
                              torch.from_numpy(self.bucket).to(device))
        return self._dev[key]


def letterbox_image_batch(image_batch, size, color=114):
    """learned_repr.py:93-136: bilinear resize with unchanged aspect ratio, centred on a `color` canvas."""
    bsz, c, orig_h, orig_w = image_batch.shape
    scale = min(size / orig_w, size / orig_h)
    new_w, new_h = int(orig_w * scale), int(orig_h * scale)
    resized = torch.nn.functional.interpolate(image_batch, size=(new_h, new_w), mode="bilinear", align_corners=False)
    canvas = torch.full((bsz, c, size, size), fill_value=color, dtype=image_batch.dtype, device=image_batch.device)
    top, left = (size - new_h) // 2, (size - new_w) // 2
    canvas[:, :, top:top + new_h, left:left + new_w] = resized
    return canvas


def _on_device(events, device):
    """True for a CUDA tensor that lives on ``device`` ("cuda" without an index is the current device)."""
    if not isinstance(events, torch.Tensor) or not events.is_cuda:
        return False
    device = torch.device(device)
    if device.type != "cuda":
        return False
    return events.device.index == (device.index if device.index is not None else torch.cuda.current_device())


def prepare_events(events, H, W, device):
    """(N, 5) [x, y, t, p, b] rows -> (EventBatch of the int32 rows, float32 t / t.max() per batch item on the device).
    The caller's tensor is not modified.  A CUDA tensor on ``device`` is prepared there (``prepare_events_device``: no
    event leaves the device); host tensors, numpy arrays and CUDA tensors of another device take the host route
    (``_prepare_events_host``).  Both give the same bits."""
    if _on_device(events, device):
        return prepare_events_device(events, H, W, device)
    return _prepare_events_host(events, H, W, device)


_EMPTY_OR_SHAPE = "events must be a non-empty (N, 5) tensor of [x, y, t, p, b] rows"
_NOT_GROUPED = "events must be grouped by batch index (ascending), as the collate function delivers them"
_BAD_POLARITY = "p must be in {0, 1} (learned_repr.py:163 indexes the polarity half with it)"


def prepare_events_device(events, H, W, device, batch_size=None):
    """``prepare_events`` for a CUDA tensor on ``device``, on the device (evrep_est_prepare: offsets from the boundaries of b,
    the per-item maximum of t by integer atomicMax, one float32 division, the int32 rows).  ``batch_size``: the number of
    items B; default 1 + events[-1, -1] (learned_repr.py:145, a 4-byte read).  A larger one gives trailing empty items.
    One read-back of (B + 2) words brings the offsets (``EventBatch`` sizes its plan from them) and the status word; the
    host route's exceptions are raised from it before any builder runs: NotImplementedError (b descending), ValueError
    (p not 0 or 1; b negative, non-integral, non-finite or >= B; empty or wrong shape), IndexError (out of the frame).

    Two corners differ from the host route.  Non-finite coordinates are an IndexError here (numpy's float-to-int cast of
    NaN, which the host route goes through, is undefined).  An item whose maximum is a zero while it also holds negative
    times divides by +0 here if both zeros occur; torch does not define which zero its max returns, so the sign of that
    item's infinities is unspecified on either route."""
    from .engine import est_prepare
    if not _on_device(events, device):
        raise ValueError("prepare_events_device takes a CUDA tensor on %s" % (device,))
    if events.dim() != 2 or events.shape[1] != 5 or events.shape[0] == 0:
        raise ValueError(_EMPTY_OR_SHAPE)
    ev = events.detach().to(torch.float32).contiguous()                 # a copy only where needed, never in place
    if batch_size is None:
        last = float(ev[-1, 4].item())                                   # B = 1 + events[-1, -1]  (:145)
        if not (last == last and -1.0 < last < _lib.EST_PREP_MAX_B):
            raise ValueError("the last batch index must be in 0 .. %d, got %r" % (_lib.EST_PREP_MAX_B - 1, last))
        nb = int(1 + last)
    else:
        nb = int(batch_size)
    if not 1 <= nb <= _lib.EST_PREP_MAX_B:
        raise ValueError("1 <= batch_size <= %d, got %d" % (_lib.EST_PREP_MAX_B, nb))
    rows, _, tn, _, packed = est_prepare(ev, nb, H, W)
    host = packed.cpu()                                                  # the one read-back: offsets and status
    status = int(host[nb + 1].item()) & 0xFFFFFFFF
    if status & _lib.EST_PREP_DESCENDING:
        raise NotImplementedError(_NOT_GROUPED)
    if status & _lib.EST_PREP_BAD_POLARITY:
        raise ValueError(_BAD_POLARITY)
    if status & _lib.EST_PREP_OUT_OF_FRAME:
        raise IndexError("event coordinates outside the %dx%d frame" % (W, H))
    if status & _lib.EST_PREP_BAD_INDEX:
        raise ValueError("batch indices must be integers in 0 .. %d" % (nb - 1))
    return EventBatch(rows, host[:nb + 1].clone(), H, W), tn


def _prepare_events_host(events, H, W, device):
    """The host route of ``prepare_events``: the rows are brought to the CPU, prepared with torch and numpy, and uploaded."""
    ev = events.detach().to("cpu", torch.float32) if isinstance(events, torch.Tensor) else \
        torch.as_tensor(np.asarray(events, dtype=np.float32))
    if ev.dim() != 2 or ev.shape[1] != 5 or ev.shape[0] == 0:
        raise ValueError(_EMPTY_OR_SHAPE)
    b = ev[:, 4].to(torch.int64)
    nb = int(1 + ev[-1, 4].item())                                   # B = 1 + events[-1, -1]  (:145)
    if bool((b[1:] < b[:-1]).any()):
        raise NotImplementedError(_NOT_GROUPED)
    p = ev[:, 3]
    if bool(((p != 0) & (p != 1)).any()):
        raise ValueError(_BAD_POLARITY)
    counts = torch.bincount(b, minlength=nb)[:nb]
    offs = np.zeros(nb + 1, dtype=np.int64)
    np.cumsum(counts.numpy(), out=offs[1:])
    tn = ev[:, 2].clone()
    for bi in range(nb):                                             # t[b == bi] /= t[b == bi].max()  (:159-160)
        s, e = int(offs[bi]), int(offs[bi + 1])
        if e > s:
            tn[s:e] /= tn[s:e].max()
    rows = np.zeros((ev.shape[0], 4), dtype=np.int32)
    rows[:, 0] = ev[:, 0].numpy().astype(np.int64)                   # idx.long() truncates  (:170)
    rows[:, 1] = ev[:, 1].numpy().astype(np.int64)
    rows[:, 3] = p.numpy().astype(np.int32)
    if rows[:, 0].min() < 0 or rows[:, 1].min() < 0 or rows[:, 0].max() >= W or rows[:, 1].max() >= H:
        raise IndexError("event coordinates outside the %dx%d frame" % (W, H))
    batch = EventBatch(torch.from_numpy(rows).to(device), torch.from_numpy(offs), H, W)
    return batch, tn.contiguous().to(device)


class QuantizationLayer:
    """Forward-only mirror of learned_repr.QuantizationLayer(dim=(C, H, W), image_size)."""

    def __init__(self, dim, value_layer, image_size=640, device="cuda:0"):
        self.dim = tuple(int(v) for v in dim)
        if not 2 <= self.dim[0] <= 8:
            raise ValueError("2 <= C <= 8 bins (2C channels <= 16)")
        self.image_size = image_size
        self.device = torch.device(device)
        self.kernel = value_layer if isinstance(value_layer, PiecewiseLinearKernel) else \
            PiecewiseLinearKernel(mlp_weights(value_layer))

    def voxel(self, events):
        """(N, 5) [x, y, t, p, b] -> (B, 2C, H, W) float32 on the device, before the letterbox (:143-176)."""
        C, H, W = self.dim
        batch, tn = prepare_events(events, H, W, self.device)
        seg, bucket = self.kernel.device_table(self.device)
        out = batch.est_voxel(tn, C, seg, bucket, self.kernel.lo, self.kernel.hi)
        return out.permute(0, 3, 1, 2)                                   # (B, 2C, H, W): [p*C + i]  (:175-176)

    def forward(self, events):
        vox = self.voxel(events)
        if self.image_size is None:
            return vox.contiguous()
        return letterbox_image_batch(vox.contiguous(), self.image_size).to(dtype=torch.float32)

    __call__ = forward


# ------------------------------------------------------------------------------------------------
# Training: the parameters, (a, c) as differentiable functions of them, the autograd bridge, the nn.Module
# ------------------------------------------------------------------------------------------------
class ValueLayer(torch.nn.Module):
    """The value MLP 1 -> hidden -> hidden -> 1 with LeakyReLU(0.1): ``.mlp`` is a ModuleList of three nn.Linear, so the
    state-dict keys are mlp.{0,1,2}.{weight,bias} as in the reference's checkpoints, and ``mlp_weights`` accepts it."""

    def __init__(self, state_dict=None, hidden=100):
        super().__init__()
        if state_dict is not None:
            hidden = int(np.asarray(state_dict["mlp.0.bias"]).shape[0])
        self.mlp = torch.nn.ModuleList([torch.nn.Linear(1, hidden), torch.nn.Linear(hidden, hidden), torch.nn.Linear(hidden, 1)])
        if state_dict is not None:
            self.load_state_dict({k: torch.as_tensor(np.asarray(v)) if not isinstance(v, torch.Tensor) else v
                                  for k, v in state_dict.items()})

    def forward(self, x):
        """f(x) elementwise, by the MLP's own statements (the device path never calls this: it uses the table)."""
        h = x.reshape(-1, 1)
        h = torch.nn.functional.leaky_relu(self.mlp[0](h), NEG_SLOPE)
        h = torch.nn.functional.leaky_relu(self.mlp[1](h), NEG_SLOPE)
        return self.mlp[2](h).reshape(x.shape)

    @classmethod
    def from_trilinear(cls, C, hidden=100):
        """The trilinear kernel max(0, 1 - (C-1)|u|) in closed form (the reference fits it with 1000 Adam steps).
        With l = LeakyReLU(0.1): relu(z) = (l(z) + 0.1 l(-z)) / 0.99 and z = (l(z) - l(-z)) / 1.1, so six first-layer
        units carry +-(s u + 1), +-(s u), +-(s u - 1) with s = C - 1, two second-layer units carry +-hat(u) =
        +-(relu(su+1) - 2 relu(su) + relu(su-1)), and the output layer undoes the second activation.  Every other
        unit is zero."""
        if hidden < 6:
            raise ValueError("the closed form needs 6 hidden units")
        s = float(int(C) - 1)
        layer = cls(hidden=hidden)
        with torch.no_grad():
            for lin in layer.mlp:
                lin.weight.zero_()
                lin.bias.zero_()
            for j, off in enumerate((1.0, 0.0, -1.0)):
                layer.mlp[0].weight[2 * j, 0], layer.mlp[0].bias[2 * j] = s, off
                layer.mlp[0].weight[2 * j + 1, 0], layer.mlp[0].bias[2 * j + 1] = -s, -off
            hat = torch.zeros(hidden, dtype=torch.float64)
            for j, coef in enumerate((1.0, -2.0, 1.0)):
                hat[2 * j], hat[2 * j + 1] = coef / 0.99, 0.1 * coef / 0.99
            layer.mlp[1].weight[0] = hat.to(torch.float32)
            layer.mlp[1].weight[1] = (-hat).to(torch.float32)
            layer.mlp[2].weight[0, 0], layer.mlp[2].weight[0, 1] = 1.0 / 1.1, -1.0 / 1.1
        return layer


def trilinear_kernel(u, C):
    """max(0, 1 - (C-1)|u|): what ``ValueLayer.from_trilinear`` represents."""
    u = np.asarray(u, dtype=np.float64)
    return np.maximum(0.0, 1.0 - (int(C) - 1) * np.abs(u))


class _PieceCoefficients(torch.autograd.Function):
    """(a, c) of every piece.  The values come from the very numpy statements ``PiecewiseLinearKernel`` uses, so the
    table of the training path equals the table of the inference path bit for bit whatever BLAS torch is linked
    to; the gradient is those statements' adjoint with the activation masks as constants."""

    @staticmethod
    def forward(ctx, w1, b1, W2, b2, w3, b3, mids, slope):
        wn = [t.detach().cpu().numpy().astype(np.float64, copy=False) for t in (w1, b1, W2, b2, w3)]
        a, c, a1, a2, A2, B2 = _piece_forms(wn + [float(b3.detach().reshape(-1)[0])], mids, slope)
        ctx.save_for_backward(w1, b1, W2, w3)
        ctx.masks = tuple(torch.from_numpy(np.ascontiguousarray(v)) for v in (a1, a2, A2, B2))
        return torch.from_numpy(a), torch.from_numpy(c)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, ga, gc):
        w1, b1, W2, w3 = ctx.saved_tensors
        a1, a2, A2, B2 = ctx.masks
        gA2 = a2 * torch.outer(ga, w3)                  # a = (a2 * A2) @ w3
        gB2 = a2 * torch.outer(gc, w3)                  # c = (a2 * B2) @ w3 + b3
        g_w3 = (a2 * A2).T @ ga + (a2 * B2).T @ gc
        g_b3 = gc.sum().reshape(1)
        g_W2 = gA2.T @ (a1 * w1) + gB2.T @ (a1 * b1)    # A2 = (a1 * w1) @ W2.T, B2 = (a1 * b1) @ W2.T + b2
        g_b2 = gB2.sum(0)
        g_w1 = ((gA2 @ W2) * a1).sum(0)
        g_b1 = ((gB2 @ W2) * a1).sum(0)
        return g_w1, g_b1, g_W2, g_b2, g_w3, g_b3, None, None


def piece_coefficients(weights, kernel):
    """(a, c) float64 tensors of the pieces of ``kernel`` as functions of the six weight tensors (w1, b1, W2, b2, w3,
    b3 in ``mlp_weights`` order, any float dtype, shapes as nn.Linear holds them or flat): the formulas of
    ``PiecewiseLinearKernel.__init__`` with the activation masks taken at the kernel's piece midpoints as constants.
    Differentiable in the weights (once); equal to ``kernel.a`` / ``kernel.c`` bit for bit when ``kernel`` was built from
    these weights."""
    w1, b1, W2, b2, w3, b3 = [t.to(device="cpu", dtype=torch.float64) for t in weights]
    n2, n1 = W2.shape
    mids = 0.5 * (kernel.edges[:-1] + kernel.edges[1:])
    return _PieceCoefficients.apply(w1.reshape(n1), b1.reshape(n1), W2, b2.reshape(n2), w3.reshape(n2), b3.reshape(1),
                                    mids, kernel.slope)


class EstVoxelFunction(torch.autograd.Function):
    """est_voxel as a function of the table's (a, c): forward k_est, backward k_est_bwd.  a, c: float64 (pieces,) on the
    batch's device; ends, bucket: the kernel's piece ends (float64) and hint table (int32) there."""

    @staticmethod
    def forward(ctx, a, c, ends, bucket, batch, tn, C, lo, hi):
        seg = torch.stack([ends, a.detach(), c.detach()], dim=1).contiguous()      # {u_next, a, c}
        ctx.table = (seg, bucket, batch, tn, int(C), float(lo), float(hi))
        return batch.est_voxel(tn, C, seg, bucket, lo, hi)

    @staticmethod
    @torch.autograd.function.once_differentiable   # a second backward raises: the keyed reduction has no derivative of its own here
    def backward(ctx, grad_out):
        seg, bucket, batch, tn, C, lo, hi = ctx.table
        g = batch.est_voxel_backward(tn, C, seg, bucket, lo, hi, grad_out.to(torch.float32).contiguous())
        return g[:, 0], g[:, 1], None, None, None, None, None, None, None


class TrainableQuantizationLayer(torch.nn.Module):
    """learned_repr.QuantizationLayer(dim=(C, H, W), image_size) with a trainable ``value_layer``: forward on k_est,
    backward on k_est_bwd.  Every forward rebuilds the breakpoints and the hint table from the current weights on the
    host (under no_grad); the output equals ``QuantizationLayer``'s for the same weights bit for bit."""

    def __init__(self, dim, value_layer=None, image_size=640, device="cuda:0"):
        super().__init__()
        self.dim = tuple(int(v) for v in dim)
        if not 2 <= self.dim[0] <= 8:
            raise ValueError("2 <= C <= 8 bins (2C channels <= 16)")
        self.image_size = image_size
        self.device = torch.device(device)
        self.value_layer = value_layer if isinstance(value_layer, torch.nn.Module) else \
            (ValueLayer(value_layer) if value_layer is not None else ValueLayer.from_trilinear(self.dim[0]))
        self.kernel = None               # the table of the last forward

    def table(self):
        """The piecewise-linear table of the current weights (host)."""
        with torch.no_grad():
            kernel = PiecewiseLinearKernel(mlp_weights(self.value_layer))
        if len(kernel) > _lib.EST_BWD_MAX_SEG:
            raise ValueError("the value MLP has %d linear pieces; the backward holds at most EVREP_EST_BWD_MAX_SEG = %d"
                             % (len(kernel), _lib.EST_BWD_MAX_SEG))
        return kernel

    def voxel(self, events):
        C, H, W = self.dim
        self.kernel = kernel = self.table()
        mlp = self.value_layer.mlp
        a, c = piece_coefficients([mlp[0].weight, mlp[0].bias, mlp[1].weight, mlp[1].bias, mlp[2].weight, mlp[2].bias], kernel)
        batch, tn = prepare_events(events, H, W, self.device)
        ends = torch.from_numpy(np.ascontiguousarray(kernel.edges[1:])).to(self.device)
        bucket = torch.from_numpy(kernel.bucket).to(self.device)
        out = EstVoxelFunction.apply(a.to(self.device), c.to(self.device), ends, bucket, batch, tn, C, kernel.lo, kernel.hi)
        return out.permute(0, 3, 1, 2)                                   # (B, 2C, H, W): [p*C + i]  (:175-176)

    def forward(self, events):
        vox = self.voxel(events)
        if self.image_size is None:
            return vox.contiguous()
        return letterbox_image_batch(vox.contiguous(), self.image_size).to(dtype=torch.float32)
