"""ev-licious' ``Events.render`` on the device: the five renderings for a whole batch of windows.

``Events.render`` (ev-licious/src/evlicious/io/utils/render.py:9-141) draws ONE window per Python call -- the ``*_NO_OVERLAP``
types through a numba loop over the events -- and ``Visualizer.update`` / ``convert_to_video`` (io/utils/visualization.py:37-46,
145-165) call it once per frame.  Here a batch of windows is rendered by the binning pass, one stream builder
(``evrep_render_state``: the per-pixel state every type is a function of) and one streaming launch (``evrep_render_compose``):
``EventBatch.render`` returns ``(B, H, W, 3)`` uint8 frames (``(B, H, W, 4)`` float64 for ``TIME_SURFACE``) and
``DeviceRecording.render_iterator`` turns a recording into frame batches with no event crossing PCIe.  The same call shows what a
filter keeps: ``f.insert_device(batch).render(...)`` beside ``batch.render(...)``.

What the reference computes, with integer coordinates (``divider == 1``; "positive" is ``p > 0``, ``Events`` forces p into
{-1, +1}), is a function of a small per-pixel state (include/evrep.h states the bits):

* ``RED_BLUE_OVERLAP``: a touched pixel is (255 if any negative, 0, 255 if any positive); order-free.
* ``RED_BLUE_NO_OVERLAP`` / ``BLACK_WHITE_NO_OVERLAP``: the reversed first-visit loop gives a pixel the colour of its LAST event
  in array order: positive (0, 0, 255) / white, negative (255, 0, 0) / black.
* ``cast=False`` (``_jitter_events``) draws every event at (x, y), (x, y+1), (x+1, y), (x+1, y+1), the four copies concatenated
  and clipped to the frame: a 2 x 2 stencil over the state.
* ``EVENT_FRAME``: ``uint8(clip(20 * (#pos - #neg) + 128, 0, 255))`` on three channels.
* ``TIME_SURFACE``: ``np.add.at`` of ``exp(-(t[-1] - t) / 3e4)`` (float64) into a float32 image, one rounding per event in array
  order, then matplotlib's jet colour map: float64 RGBA.  A window of <= 2 events is an all-zero image instead.
* ``rendering``: the canvas the three colour types draw onto (white by default); the other two ignore it, and ``cast``.

Not mirrored: sub-pixel coordinates (``divider > 1``: the bilinear ``_aggregate_float``; the reference's colour types fail on float
indices there), and the Visualizer's window, keys, text overlay, ``cv2.resize`` and video writer.  matplotlib is not imported:
``jet_lut`` restates its table.  There is no CPU fallback.
"""
import enum

import numpy as np
import torch

from . import _lib
from ._lib import ptr, want

TAU_US = 3e4        # render.py:128


class RenderingType(enum.IntEnum):
    """render.py:9-14 (``enum.auto()`` counts from 1)."""
    RED_BLUE_OVERLAP = 1
    RED_BLUE_NO_OVERLAP = 2
    BLACK_WHITE_NO_OVERLAP = 3
    TIME_SURFACE = 4
    EVENT_FRAME = 5


_COLOUR_TYPES = (RenderingType.RED_BLUE_OVERLAP, RenderingType.RED_BLUE_NO_OVERLAP, RenderingType.BLACK_WHITE_NO_OVERLAP)

# matplotlib's published segment data of "jet" (lib/matplotlib/_cm.py, _jet_data): rows (x, y0, y1) per channel
_JET_SEGMENTS = (
    ((0.00, 0, 0), (0.35, 0, 0), (0.66, 1, 1), (0.89, 1, 1), (1.00, 0.5, 0.5)),
    ((0.000, 0, 0), (0.125, 0, 0), (0.375, 1, 1), (0.640, 1, 1), (0.910, 0, 0), (1.000, 0, 0)),
    ((0.00, 0.5, 0.5), (0.11, 1, 1), (0.34, 1, 1), (0.65, 0, 0), (1.00, 0, 0)),
)


def jet_lut():
    """The (256, 4) float64 table ``plt.get_cmap("jet")`` looks colours up in: per channel matplotlib's linear-segment formula
    (``colors._create_lookup_table``, gamma 1) over the segment data above; alpha 1."""
    N = 256
    lut = np.ones((N, 4), np.float64)
    xind = (N - 1) * np.linspace(0, 1, N)
    for c, data in enumerate(_JET_SEGMENTS):
        adata = np.array(data, dtype=np.float64)
        x, y0, y1 = adata[:, 0] * (N - 1), adata[:, 1], adata[:, 2]
        ind = np.searchsorted(x, xind)[1:-1]
        distance = (xind[1:-1] - x[ind - 1]) / (x[ind] - x[ind - 1])
        col = np.concatenate([[y1[0]], distance * (y0[ind] - y1[ind - 1]) + y1[ind - 1], [y0[-1]]])
        lut[:, c] = np.clip(col, 0.0, 1.0)
    return lut


_LUT_DEVICE = {}


def _lut_on(device):
    key = (device.type, device.index)
    if key not in _LUT_DEVICE:
        _LUT_DEVICE[key] = torch.from_numpy(jet_lut()).to(device)
    return _LUT_DEVICE[key]


def check_canvas(rendering, height, width, batch=None):
    """The canvas of a call as it was given: None, or a uint8 array / tensor of shape (H, W, 3) -- or (B, H, W, 3) where
    ``batch`` says how many windows there are.  ``ValueError`` otherwise."""
    if rendering is None:
        return None
    shapes = [(height, width, 3)] + ([(batch, height, width, 3)] if batch is not None else [])
    dtype = rendering.dtype if isinstance(rendering, (np.ndarray, torch.Tensor)) else None
    if dtype not in (np.dtype(np.uint8), torch.uint8) or tuple(rendering.shape) not in shapes:
        raise ValueError("rendering must be a uint8 canvas of shape %s, not %s %s"
                         % (" or ".join(str(s) for s in shapes), dtype, tuple(getattr(rendering, "shape", ()))))
    return rendering


def render_state(batch, net=False, surface=False, tau=TAU_US, state=None):
    """``evrep_render_state`` for an EventBatch -> (state uint8, net int32 or None, surface float32 or None), (B, H, W) device
    tensors; include/evrep.h states their meaning.  net / surface: True allocates, a tensor is written.  Nothing is read back."""
    batch.bin()
    shape = (batch.B, batch.H, batch.W)

    def tensor(given, dtype, name):
        if given is None or given is False:
            return None
        if given is True:
            return torch.empty(shape, dtype=dtype, device=batch.device)
        return want(given, name, dtype, shape, device=batch.device)

    state = tensor(True if state is None else state, torch.uint8, "state")
    net_t, surf = tensor(net, torch.int32, "net"), tensor(surface, torch.float32, "surface")
    batch._launch(batch.api.evrep_render_state, ptr(state), ptr(net_t), ptr(surf), float(tau))
    return state, net_t, surf


def device_status(batch):
    """The windows' EVREP_ST_* words as a (B,) uint32 DEVICE tensor: the status field of the workspace's window statistics, which
    ``evrep_render_state`` leaves merged under every binning pass.  No read-back."""
    p = batch.plan
    meta = batch.workspace[p.off_meta:p.off_meta + batch.B * 64].view(torch.int32).view(batch.B, 16)
    return meta[:, 8].clone().view(torch.uint32)


def render_compose(state, rendering_type, cast=True, net=None, surface=None, rendering=None, out=None):
    """``evrep_render_compose`` on the current stream: the (B, H, W) state of ``render_state`` (+ net for EVENT_FRAME, surface
    for TIME_SURFACE, a device canvas for the colour types) -> frames, written to ``out`` where given.  Nothing is read back."""
    rt = RenderingType(int(rendering_type))
    B, H, W = (int(v) for v in state.shape)
    ts = rt == RenderingType.TIME_SURFACE
    shape, dtype = ((B, H, W, 4), torch.float64) if ts else ((B, H, W, 3), torch.uint8)
    out = torch.empty(shape, dtype=dtype, device=state.device) if out is None else want(out, "out", dtype, shape, device=state.device)
    colour = rt in _COLOUR_TYPES
    canvas = None
    if rendering is not None and colour:
        canvas = want(check_canvas(rendering, H, W, batch=B), "rendering", torch.uint8, device=state.device)
    flags = _lib.RENDER_JITTER if (not cast and colour) else 0       # the other two types ignore cast
    with torch.cuda.device(state.device):
        _lib.api().evrep_render_compose(ptr(state), ptr(net), ptr(surface), ptr(_lut_on(state.device)) if ts else None, ptr(canvas),
                                        int(canvas is not None and canvas.dim() == 4), B, H, W, int(rt), flags, ptr(out),
                                        _lib.stream_ptr())
    return out


def render_batch(batch, rendering_type=RenderingType.RED_BLUE_OVERLAP, cast=True, rendering=None, check=True, out=None):
    """``EventBatch.render``."""
    rt = RenderingType(int(rendering_type))
    B, H, W = batch.B, batch.H, batch.W
    canvas = check_canvas(rendering, H, W, batch=B)
    if canvas is not None and rt in _COLOUR_TYPES:
        if isinstance(canvas, np.ndarray):
            canvas = torch.from_numpy(np.ascontiguousarray(canvas))
        canvas = canvas.to(batch.device).contiguous()      # (a canvas that overlaps `out` is refused by the library)
    ts = rt == RenderingType.TIME_SURFACE
    state, net, surf = render_state(batch, net=rt == RenderingType.EVENT_FRAME, surface=ts)
    out = render_compose(state, rt, cast=cast, net=net, surface=surf, rendering=canvas, out=out)
    status = device_status(batch)
    if not check:
        return out, status
    st = status.cpu().numpy()
    bad = np.flatnonzero(st & _lib.ST_OOB)
    if bad.size:
        raise ValueError("window %d holds rows outside the %d x %d (height x width) frame, which Events refuses (EVREP_ST_OOB; %d "
                         "such windows)" % (int(bad[0]), H, W, bad.size))
    return out


def render(events, rendering=None, rendering_type=RenderingType.RED_BLUE_OVERLAP, cast=True, device="cuda:0"):
    """The per-sample drop-in for ``Events.render``: anything with x, y, t, p, width, height -> a numpy image with the reference's
    shape and dtype: (H, W, 3) uint8; TIME_SURFACE (H, W, 4) float64, or (H, W) uint8 zeros for <= 2 events."""
    from .engine import EventBatch
    rt = RenderingType(int(rendering_type))
    if int(getattr(events, "divider", 1)) > 1:
        raise NotImplementedError("divider > 1: sub-pixel coordinates go through the reference's bilinear draw _aggregate_float, "
                                  "which is not mirrored (and its colour types fail on float indices)")
    H, W = int(events.height), int(events.width)
    canvas = check_canvas(rendering, H, W)
    x, y, t, p = (np.asarray(getattr(events, k)) for k in "xytp")
    n = len(x)
    if n and (int(x.max()) >= W or int(y.max()) >= H or int(x.min()) < 0 or int(y.min()) < 0):
        raise ValueError("events outside the %d x %d (height x width) frame, which Events refuses" % (H, W))
    if rt == RenderingType.TIME_SURFACE and n <= 2:
        return np.zeros((H, W), np.uint8)
    rows = np.empty((n, 4), np.int32)
    rows[:, 0], rows[:, 1] = x, y
    if n:
        # t[-1] - t is all the time surface reads; beyond +-2^31 us exp() is 0 or inf either way, so the clip changes no value
        rows[:, 2] = np.clip(t.astype(np.int64) - np.int64(t[-1]), -(1 << 31) + 1, (1 << 31) - 1)
    rows[:, 3] = np.where(p > 0, 1, -1)
    batch = EventBatch.from_numpy([rows], H, W, device=device)
    return render_batch(batch, rt, cast=cast, rendering=canvas, check=True)[0].cpu().numpy()


def video_frames(images):
    """What ``convert_to_video`` hands its writer (visualization.py:149-150): ``clip(rgba[..., :3] * 255, 0, 255)`` as uint8 for
    a TIME_SURFACE batch, the images themselves otherwise."""
    if images.dtype == torch.float64:
        return (images[..., :3] * 255).clamp(0, 255).to(torch.uint8)
    return images
