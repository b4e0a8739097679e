"""Row F4: n_imagenet's per-polarity accumulators on the binned stream.

Host-side mirror of the `reshape_then_*` accumulator family of
n_imagenet/real_cnn_model/data/imagenet.py (same names, same `(event_tensor, augment=None, **kwargs)`
signature, same (C, H, W) float32 result, same empty-input behaviour):

    reshape_then_acc            :169-210   [pos count / max, pos latest time, neg count / max, neg latest time]
    reshape_then_acc_time       :213-247   [pos earliest, pos latest, neg earliest, neg latest]
    reshape_then_acc_count      :250-293   [pos count, pos latest, neg count, neg latest]
    reshape_then_acc_count_pol  :296-321   [pos count, neg count]
    reshape_then_acc_count_only :324-343   [count]
    reshape_then_acc_all        :346-394   [pos count, neg count, pos latest, neg latest, pos earliest, neg earliest]
    reshape_then_flat           :397-413   [any event]
    reshape_then_flat_pol       :416-438   [any pos event, any neg event]
    reshape_then_acc_exp        :441-472   exp(-(1 - latest)/0.3) per polarity, over the whole frame
    reshape_then_acc_time_pol   :475-510   [pos latest, neg latest]
    reshape_then_acc_intensity  :841-870   min-max normalised (pos count - neg count)

`event_tensor` is what parse_event hands over (:128-164): a float64 (N, 4) tensor of rows
[x, y, t_seconds, p], p in {-1, +1}, coordinates possibly fractional (they are truncated by `.long()`,
:187).  All of them are ONE HIP builder (evrep_polstats, csrc/evrep_builders.hip k_polstats) with a
per-channel (polarity class, statistic) descriptor; the two window-level normalisations (count / count.max(),
min-max of the intensity) are strided float32 tensor ops on the builder's output, as in the reference.

The three n_imagenet wrappers of the path's own builders that run in the reference -- reshape_then_optimized
(:1025-1039), reshape_then_event_stack (:1042-1060), reshape_then_tore (:1080-1107) -- are mirrored here too
(float64 event tensors with integral values, as load_event produces them without `reshape`).  study_batch is their batched
form: one upload, evrep_nimg_study_rows (csrc/evrep_study.hip: the rows each wrapper hands its builder, formed on the device), the
batched builder, one cast-and-transpose launch; n_imagenet_front.study_device is the same on device-made rows.
reshape_then_time_surface (:1110-1137) raises IndexError in the reference itself (a float `p` field indexes
the surface memory, time_surface.py:67) and does so here; reshape_then_voxel_grid / _to_image go through tonic
(absent; see representations/tonic_compat.py).

reshape_then_acc_adj_sort (DiST, :873-999) = the same builder (per-polarity count, latest and earliest time)
followed by the reference's own image-space statements (count clipping, 5x5 pooling, temporal discount, dense
rank of the discounted timestamps) as torch ops on the GPU, one window per call.  dist_batch is its batched form: the same
builder for B windows, then ONE evrep_dist call (csrc/evrep_dist.hip: clip, 5x5 discount and dense rank as HIP kernels), bit-equal
to the reference's image; n_imagenet_front.dist_device is the same on device-made rows.

reshape_then_acc_sort (:513-838) is mirrored for strict=False (the "sorted timestamp image": latest time INDEX per
pixel, from the same builder with the dense time rank as the per-event value) and for strict=True (followed by the dense
rank of the per-pixel maxima; bit-exact on goldens that the generator checks not to depend on which of several tied events
torch_scatter's arg-max names); the quantisation runs in the reference's precision (float32 when strict, float64 otherwise) with a
true division -- torch's GPU `tensor / python_int` multiplies by the reciprocal, which is off by one ulp for q = 255; the denoise options raise the NameError they raise in the reference
(density_filter_event_image is never defined there).
sort_batch is its batched form for every switch (strict, global_time, use_image, neglect_polarity, quantize_sort): ONE
evrep_time_index call (csrc/evrep_sort.hip: idx = (int64)(t * 1e6) and its consecutive rank per window, a segmented scan over several
workgroups per window), the same builder for B windows, then ONE evrep_sort_image call (the masked dense rank of the per-pixel
maxima with the reference's own normalisation and quantisation), bit-equal to the reference's image; strict=True ranks the
consecutive rank whatever global_time is, so latest indices one microsecond apart stay apart beyond 2^24 us, where the float32
index reshape_then_acc_sort ranks has merged them.  n_imagenet_front.sort_device is the same on device-made rows.
The EST quantisation layer is in est.py.
The product path needs the HIP library and an MI355X; there is no CPU fallback.
"""
import numpy as np
import torch

from . import _lib
from ._lib import ptr, stream_ptr
from .engine import EventBatch

IMAGE_H = 224    # imagenet.py:17-18
IMAGE_W = 224
EXP_TAU = 0.3    # imagenet.py:20

ANY, POS, NEG = 0, 1, 2                                  # EVREP_PS_* of include/evrep.h
COUNT, TMAX, TMIN, FLAG, EXP, SIGNED = 0, 1, 2, 3, 4, 5

# name -> (polarity class per channel, statistic per channel)
SPECS = {
    "acc": ([POS, POS, NEG, NEG], [COUNT, TMAX, COUNT, TMAX]),
    "acc_time": ([POS, POS, NEG, NEG], [TMIN, TMAX, TMIN, TMAX]),
    "acc_count": ([POS, POS, NEG, NEG], [COUNT, TMAX, COUNT, TMAX]),
    "acc_count_pol": ([POS, NEG], [COUNT, COUNT]),
    "acc_count_only": ([ANY], [COUNT]),
    "acc_all": ([POS, NEG, POS, NEG, POS, NEG], [COUNT, COUNT, TMAX, TMAX, TMIN, TMIN]),
    "flat": ([ANY], [FLAG]),
    "flat_pol": ([POS, NEG], [FLAG, FLAG]),
    "acc_exp": ([POS, NEG], [EXP, EXP]),
    "acc_time_pol": ([POS, NEG], [TMAX, TMAX]),
    "acc_intensity": ([ANY], [SIGNED]),
}


def _as_f64(event_tensor):
    a = event_tensor.detach().cpu().numpy() if isinstance(event_tensor, torch.Tensor) else np.asarray(event_tensor)
    return np.asarray(a, dtype=np.float64).reshape(-1, 4)


def _window(ev, H, W):
    """(N,4) float64 -> int32 rows [x.long(), y.long(), 0, sign(p)] and the normalised float64 times
    (t - t[0]) / (t[-1] - t[0])  (imagenet.py:178-181,198-199)."""
    xi, yi = ev[:, 0].astype(np.int64), ev[:, 1].astype(np.int64)   # .long() truncates toward zero
    if len(ev) and (xi.min() < 0 or yi.min() < 0 or xi.max() >= W or yi.max() >= H):
        # the reference fails here as well (bincount grows past H*W and the reshape raises, :187-189)
        raise RuntimeError("event coordinates outside the %dx%d frame" % (W, H))
    rows = np.zeros((len(ev), 4), dtype=np.int32)
    rows[:, 0], rows[:, 1] = xi, yi
    rows[:, 3] = (ev[:, 3] > 0).astype(np.int32) - (ev[:, 3] < 0).astype(np.int32)
    with np.errstate(divide="ignore", invalid="ignore"):
        tn = (ev[:, 2] - ev[0, 2]) / (ev[-1, 2] - ev[0, 2]) if len(ev) else np.zeros(0)
    return rows, tn


def accumulate_batch(name, event_tensors, height=IMAGE_H, width=IMAGE_W, device="cuda:0"):
    """Batched form: a list of (N_b, 4) float64 event tensors -> (B, C, H, W) float32 CUDA tensor (a
    channel-first VIEW of the builder's (B, H, W, C) output, like the reference's permute(2, 0, 1))."""
    if name not in SPECS:
        raise KeyError(name)
    wins = [_as_f64(e) for e in event_tensors]
    for w in wins:
        if len(w) == 0:
            raise IndexError("empty event tensor")   # event_tensor[0, 2], imagenet.py:178
    packed = [_window(w, height, width) for w in wins]
    batch = EventBatch.from_numpy([r for r, _ in packed], height, width, device=device)
    tnorm = torch.from_numpy(np.concatenate([t for _, t in packed]) if packed else np.zeros(0)).to(batch.device)
    return _accumulate(name, batch, tnorm)


def _accumulate(name, batch, tnorm):
    """The part of accumulate_batch behind the upload (n_imagenet_front.accumulate_device enters here with device-made rows):
    the polstats builder and the two window-level normalisations."""
    pol, stat = SPECS[name]
    out = batch.polstats(tnorm, pol, stat, tau=EXP_TAU)            # (B, H, W, C) float32
    if name == "acc":          # pos_count / pos_count.max().float()  (:190-191,196-197): float32 / float32
        for c in (0, 2):
            out[..., c] /= out[..., c].amax(dim=(1, 2), keepdim=True)
    elif name == "acc_intensity":   # (i - i.min()) / (i.max() - i.min())  (:867)
        lo = out.amin(dim=(1, 2, 3), keepdim=True)
        hi = out.amax(dim=(1, 2, 3), keepdim=True)
        out = (out - lo) / (hi - lo)
    return out.permute(0, 3, 1, 2)


def _single(name, event_tensor, augment, kwargs):
    if augment is not None:
        event_tensor = augment(event_tensor)
    H = kwargs.get("height", IMAGE_H)
    W = kwargs.get("width", IMAGE_W)
    ev = _as_f64(event_tensor)
    if len(ev) == 0:
        if name in ("acc_count", "acc_time_pol"):   # ten synthetic events at the origin (:258-261,483-486)
            ev = np.zeros((10, 4))
            ev[:, 2] = (np.arange(10, dtype=np.float32) / np.float32(10.0)).astype(np.float64)
            ev[:, 3] = 1
        elif name == "acc_all":                     # :353-354 (IMAGE_H x IMAGE_W whatever height/width say)
            return torch.zeros([6, IMAGE_H, IMAGE_W])
    res = accumulate_batch(name, [ev], H, W, device=kwargs.get("device", "cuda:0"))[0]
    return res if kwargs.get("keep_on_device", False) else res.cpu()


def reshape_then_acc(event_tensor, augment=None, **kwargs):
    return _single("acc", event_tensor, augment, kwargs)


def reshape_then_acc_time(event_tensor, augment=None, **kwargs):
    return _single("acc_time", event_tensor, augment, kwargs)


def reshape_then_acc_count(event_tensor, augment=None, **kwargs):
    return _single("acc_count", event_tensor, augment, kwargs)


def reshape_then_acc_count_pol(event_tensor, augment=None, **kwargs):
    return _single("acc_count_pol", event_tensor, augment, kwargs)


def reshape_then_acc_count_only(event_tensor, augment=None, **kwargs):
    return _single("acc_count_only", event_tensor, augment, kwargs)


def reshape_then_acc_all(event_tensor, augment=None, **kwargs):
    return _single("acc_all", event_tensor, augment, kwargs)


def reshape_then_flat(event_tensor, augment=None, **kwargs):
    return _single("flat", event_tensor, augment, kwargs)


def reshape_then_flat_pol(event_tensor, augment=None, **kwargs):
    return _single("flat_pol", event_tensor, augment, kwargs)


def reshape_then_acc_exp(event_tensor, augment=None, **kwargs):
    return _single("acc_exp", event_tensor, augment, kwargs)


def reshape_then_acc_time_pol(event_tensor, augment=None, **kwargs):
    return _single("acc_time_pol", event_tensor, augment, kwargs)


def reshape_then_acc_intensity(event_tensor, augment=None, **kwargs):
    return _single("acc_intensity", event_tensor, augment, kwargs)


CLIP_COUNT_RATE = 0.99   # imagenet.py:23
DISC_ALPHA = 3.0         # imagenet.py:24


def reshape_then_acc_adj_sort(event_tensor, augment=None, **kwargs):
    """DiST (imagenet.py:873-999): discounted, sorted timestamp image, (2, H, W) float32."""
    F = torch.nn.functional
    if augment is not None:
        event_tensor = augment(event_tensor)
    H = kwargs.get("height", IMAGE_H)
    W = kwargs.get("width", IMAGE_W)
    # [pos count, pos latest, pos earliest, neg count, neg latest, neg earliest] from the HIP builder
    pol, stat = [POS, POS, POS, NEG, NEG, NEG], [COUNT, TMAX, TMIN, COUNT, TMAX, TMIN]
    ev = _as_f64(event_tensor)
    if len(ev) == 0:
        raise IndexError("empty event tensor")
    rows, tn = _window(ev, H, W)
    batch = EventBatch.from_numpy([rows], H, W, device=kwargs.get("device", "cuda:0"))
    prim = batch.polstats(torch.from_numpy(tn).to(batch.device), pol, stat)[0]          # (H, W, 6)
    halves = []
    for k in (0, 3):
        count, out, min_out = prim[..., k].clone(), prim[..., k + 1].clone(), prim[..., k + 2].clone()
        # clip count (:893-901)
        unique_count = torch.unique(count, return_counts=True)[1]
        sum_subset = torch.cumsum(unique_count, dim=0)
        th_clip = sum_subset[sum_subset < H * W * CLIP_COUNT_RATE].shape[0]
        count[count > th_clip] = th_clip
        min_out[count == 0] = 1.0                                                        # (:924-925)
        patch = 5
        neighbor = patch ** 2 * F.avg_pool2d(count.unsqueeze(0), patch, stride=1, padding=patch // 2)
        disc = (F.max_pool2d(out.unsqueeze(0), patch, stride=1, padding=patch // 2)
                + F.max_pool2d(-min_out.unsqueeze(0), patch, stride=1, padding=patch // 2)) / neighbor
        out[count > 0] = out[count > 0] - DISC_ALPHA * disc.squeeze()[count > 0]         # (:957-961)
        out[out < 0] = 0
        out[neighbor.squeeze() == 1.0] = 0
        flat = out.reshape(H * W)
        val, idx = torch.sort(flat)                                                      # (:973-990)
        unq, cnt = torch.unique_consecutive(val, return_counts=True)
        srt = torch.zeros_like(flat)
        srt[idx] = torch.repeat_interleave(torch.arange(unq.shape[0], device=flat.device), cnt).float() / unq.shape[0]
        halves.append(srt.reshape(H, W))
    res = torch.stack(halves, dim=2).permute(2, 0, 1).float()
    return res if kwargs.get("keep_on_device", False) else res.cpu()


DIST_POL, DIST_STAT = [POS, POS, POS, NEG, NEG, NEG], [COUNT, TMAX, TMIN, COUNT, TMAX, TMIN]


def _dist(batch, tnorm, clip_rate=CLIP_COUNT_RATE, alpha=DISC_ALPHA):
    """The part of dist_batch behind the upload (n_imagenet_front.dist_device enters here with device-made rows): the polstats
    builder, then evrep_dist (csrc/evrep_dist.hip: clip, 5x5 discount, dense rank) on its output.  Nothing waits for the device."""
    prim = batch.polstats(tnorm, DIST_POL, DIST_STAT)                                   # (B, H, W, 6) float32
    B, H, W = batch.B, batch.H, batch.W
    out = torch.empty((B, 2, H, W), dtype=torch.float32, device=batch.device)
    if B == 0:
        return out
    api = batch.api
    nbytes = api.evrep_dist_scratch_bytes(B, H, W)
    if nbytes == 0:
        raise ValueError("evrep_dist does not take %d windows of %dx%d" % (B, H, W))
    scratch = _lib.scratch(nbytes, batch.device)
    with torch.cuda.device(batch.device):
        api.evrep_dist(ptr(prim), B, H, W, float(clip_rate), float(alpha), ptr(out), ptr(scratch), stream_ptr())
    return out


def dist_batch(event_tensors, height=IMAGE_H, width=IMAGE_W, device="cuda:0"):
    """DiST for a batch: a list of (N_b, 4) float64 event tensors -> (B, 2, H, W) float32 device tensor, channel 0 positive,
    channel 1 negative; window b is bit-equal to the reference's reshape_then_acc_adj_sort(event_tensors[b]) (imagenet.py:873-999).
    The batched sibling of accumulate_batch: one upload, one polstats launch, one evrep_dist call of three launches.

    Windows the reference cannot rank meaningfully are refused on the host, before anything is uploaded: an empty tensor raises
    IndexError (event_tensor[0, 2], as accumulate_batch does); a tensor whose first and last timestamp agree raises ValueError
    naming the sample -- its normalised times are NaN, and the order the reference's sort gives NaNs is not a parity target."""
    wins = [_as_f64(e) for e in event_tensors]
    for b, w in enumerate(wins):
        if len(w) == 0:
            raise IndexError("empty event tensor (sample %d)" % b)
        if w[-1, 2] == w[0, 2]:
            raise ValueError("DiST of a window whose first and last timestamp agree (sample %d): its normalised times are NaN" % b)
    packed = [_window(w, height, width) for w in wins]
    batch = EventBatch.from_numpy([r for r, _ in packed], height, width, device=device)
    tnorm = torch.from_numpy(np.concatenate([t for _, t in packed]) if packed else np.zeros(0)).to(batch.device)
    return _dist(batch, tnorm)


TIME_SCALE = 1000000     # imagenet.py:21


def reshape_then_acc_sort(event_tensor, augment=None, **kwargs):
    """Sorted timestamp image (imagenet.py:513-838): per pixel (and polarity) the LATEST time index (strict=False) or
    the dense rank of it among the pixels' latest indices (strict=True), optionally with the binary event image and
    quantised copies; (C, H, W) float32."""
    if augment is not None:
        event_tensor = augment(event_tensor)
    global_time, neglect, use_image, strict = (kwargs[k] for k in ("global_time", "neglect_polarity", "use_image", "strict"))
    H = kwargs.get("height", IMAGE_H)
    W = kwargs.get("width", IMAGE_W)
    ev_t = event_tensor if isinstance(event_tensor, torch.Tensor) else torch.as_tensor(np.asarray(event_tensor))
    time_idx = (ev_t[:, 2] * TIME_SCALE).long()
    if global_time:   # dense rank of the microsecond timestamps (:521-525)
        mem, cnt = torch.unique_consecutive(time_idx, return_counts=True)
        time_idx = torch.repeat_interleave(torch.arange(mem.shape[0]), cnt)
    ev_t[:, 2] = time_idx                      # the reference overwrites the caller's time column as well (:525,539)
    if use_image and kwargs["denoise_image"]:
        raise NameError("name 'density_filter_event_image' is not defined")   # what the reference raises (:556,679)
    if kwargs["denoise_sort"]:
        raise NameError("name 'density_filter_event_image' is not defined")   # (:609,777)
    ev = _as_f64(ev_t)
    if len(ev) == 0:
        raise RuntimeError("max(): Expected reduction dim to be specified for input.numel() == 0")
    rows, _ = _window(ev, H, W)
    batch = EventBatch.from_numpy([rows], H, W, device=kwargs.get("device", "cuda:0"))
    tval = torch.from_numpy(np.ascontiguousarray(ev[:, 2])).to(batch.device)       # float64 time index per event
    classes = [ANY] if neglect else [POS, NEG]
    pol = [c for c in classes for _ in (0, 1)]
    stat = [FLAG, TMAX] * len(classes)
    prim = batch.polstats(tval, pol, stat)[0]                                      # (H, W, 2 * len(classes))
    q = kwargs["quantize_sort"]
    chans = []
    for k in range(len(classes)):
        image, srt = prim[..., 2 * k], prim[..., 2 * k + 1]
        if strict:
            # :563-590,685-748: per pixel the event of the latest time index (scatter_max's arg; which of several
            # events sharing pixel AND index it names does not matter, they carry the same value and the stream is
            # time-ordered), then the DENSE RANK of those per-pixel maxima (+1), min-max normalised in float32
            hot = image > 0
            if not bool(hot.any()):
                # a polarity without events is replaced by ONE event at pixel (0, 0), t = 0 (:647-652): its rank
                # image is all zero (max == min -> fill_(0)), its event image has that one pixel set
                image = torch.zeros_like(image)
                image[0, 0] = 1.0
                srt = torch.zeros_like(srt)
            else:
                vals = srt[hot]
                uniq, inv = torch.unique(vals, sorted=True, return_inverse=True)
                fs = inv.to(torch.float32) + 1
                if int(uniq.numel()) > 1:
                    fs = (fs - fs.min()) / (fs.max() - fs.min())
                else:
                    fs = torch.zeros_like(fs)
                srt = torch.zeros_like(srt)
                srt[hot] = fs
        elif not bool((srt > 0.0).any()):      # hot_event_sort.max() on an empty selection (:592-594,744-746)
            raise RuntimeError("max(): Expected reduction dim to be specified for input.numel() == 0")
        if q is not None:
            # the reference quantises a float32 tensor when strict (:588-591) and the float64 output of scatter_max otherwise
            # (:596), with a true division; torch's GPU `tensor / python_int` multiplies by the reciprocal, a device tensor divides
            # (the float32 quotient is taken in float64 and rounded once more: 53 bits make that the correctly rounded float32 one)
            def quant(s, qs, dt=torch.float32 if strict else torch.float64):
                return (torch.round(s.to(dt) * qs).double() / torch.tensor(qs, dtype=torch.float64, device=s.device)).float()
            if type(q) == int:
                srt = quant(srt, q)
            elif type(q) == list:
                srt = torch.stack([quant(srt, qs) for qs in q], dim=2)
        parts = ([image.unsqueeze(-1)] if use_image else []) + [srt if srt.dim() == 3 else srt.unsqueeze(-1)]
        chans.append(torch.cat(parts, dim=2))
    res = torch.cat(chans, dim=2).permute(2, 0, 1).float()
    return res if kwargs.get("keep_on_device", False) else res.cpu()


SORT_MAX_WINDOW = 1 << 24   # strict=True ranks float32 TMAX of the consecutive time rank: exact below 2^24 events per window
_SORT_EMPTY_TEXT = "max(): Expected reduction dim to be specified for input.numel() == 0"


def _sort_options(neglect_polarity, use_image, quantize_sort, denoise_image, denoise_sort):
    """The option checks sort_batch and n_imagenet_front.sort_device share -> (polarity classes, quantisation list)."""
    if use_image and denoise_image:
        raise NameError("name 'density_filter_event_image' is not defined")   # what the reference raises (:556,679)
    if denoise_sort:
        raise NameError("name 'density_filter_event_image' is not defined")   # (:609,777)
    q = quantize_sort
    if q is not None and type(q) not in (int, list):
        raise TypeError("quantize_sort is None, an int or a list of ints, not %s" % type(q).__name__)
    qs = [] if q is None else ([q] if type(q) == int else list(q))
    if q is not None and not qs:
        raise ValueError("quantize_sort is an empty list")
    if any(type(v) != int or v <= 0 or v >= 1 << 31 for v in qs):
        raise ValueError("quantize_sort holds positive ints")
    from ._lib import SORT_MAX_Q
    if len(qs) > SORT_MAX_Q:
        raise ValueError("quantize_sort holds at most %d sizes" % SORT_MAX_Q)
    return ([ANY] if neglect_polarity else [POS, NEG]), qs


def sort_status_error(status, strict):
    """The exception the status words of _sort stand for (None: no window is refused), naming the first such sample."""
    from ._lib import SORT_DECREASING, SORT_EMPTY, SORT_NO_INDEX
    status = np.asarray(status)
    for bit, make in ((SORT_EMPTY, lambda b: RuntimeError("%s (sample %d)" % (_SORT_EMPTY_TEXT, b))),
                      (SORT_DECREASING, lambda b: ValueError("time indices decrease inside the window (sample %d): the sorted "
                                                             "timestamp image ranks consecutive indices" % b))):
        hit = np.flatnonzero(status & bit)
        if hit.size:
            return make(int(hit[0]))
    hit = np.flatnonzero(status & (SORT_NO_INDEX | SORT_NO_INDEX << 1)) if not strict else np.zeros(0, np.int64)
    if hit.size:      # hot_event_sort.max() on an empty selection (:597-599,755-757,766-768)
        return RuntimeError("%s (sample %d: a polarity class without a positive time index)" % (_SORT_EMPTY_TEXT, int(hit[0])))
    return None


def _sort(batch, t, global_time, strict, classes, qs, use_image):
    """The part of sort_batch behind the upload (n_imagenet_front.sort_device enters here with device-made rows): one
    evrep_time_index, one polstats launch, one evrep_sort_image (csrc/evrep_sort.hip) -> ((B, C, H, W) float32, (B,) uint32 status
    words, both on the device).  Nothing waits for the device.

    strict=True feeds polstats the consecutive rank whatever global_time is: the dense rank of the per-pixel maxima does not change
    under a strictly increasing map of the indices, and the rank, unlike a raw microsecond index beyond 2^24, is exact in float32."""
    B, H, W, K = batch.B, batch.H, batch.W, len(classes)
    if B == 0:
        raise ValueError("no window")
    lengths = batch.offsets_host[1:] - batch.offsets_host[:-1]
    if strict and int(lengths.max()) >= SORT_MAX_WINDOW:
        raise ValueError("strict=True takes windows below %d events (sample %d holds %d)"
                         % (SORT_MAX_WINDOW, int(lengths.argmax()), int(lengths.max())))
    batch._per_event(t, "t")
    api, dev = batch.api, batch.device
    rows = max(batch.total, 1)
    tval = torch.empty(rows, dtype=torch.float64, device=dev)
    status = torch.empty(B, dtype=torch.uint32, device=dev)
    nsort = max(len(qs), 1)
    out = torch.empty((B, K * (int(bool(use_image)) + nsort), H, W), dtype=torch.float32, device=dev)
    n_ti, n_img = api.evrep_time_index_scratch_bytes(B, batch.total), api.evrep_sort_image_scratch_bytes(B, H, W, K)
    if n_ti == 0 or n_img == 0:
        raise ValueError("the sorted timestamp image does not take %d windows of %dx%d with %d events" % (B, H, W, batch.total))
    scratch = _lib.scratch(max(n_ti, n_img), dev)
    mode = _lib.TIME_INDEX_RANK if (global_time or strict) else _lib.TIME_INDEX_RAW
    with torch.cuda.device(dev):
        api.evrep_time_index(ptr(t) if batch.total else ptr(tval), ptr(batch.offsets), B, mode, ptr(tval), ptr(status), ptr(scratch),
                             stream_ptr())
    prim = batch.polstats(tval[:batch.total], [c for c in classes for _ in (0, 1)], [FLAG, TMAX] * K)      # (B, H, W, 2K) float32
    flags = (_lib.SORT_STRICT if strict else 0) | (_lib.SORT_USE_IMAGE if use_image else 0)
    with torch.cuda.device(dev):
        api.evrep_sort_image(ptr(prim), B, H, W, K, flags, _lib.int32_array(qs) if qs else None, len(qs), ptr(out), ptr(status),
                             ptr(scratch), stream_ptr())
    return out, status


def sort_batch(event_tensors, global_time, neglect_polarity, use_image, strict, quantize_sort=None, denoise_image=False,
               denoise_sort=False, height=IMAGE_H, width=IMAGE_W, device="cuda:0"):
    """The sorted timestamp image for a batch: a list of (N_b, 4) float64 event tensors -> (B, C, H, W) float32 device tensor;
    window b is bit-equal to the reference's reshape_then_acc_sort(event_tensors[b], **kwargs) (imagenet.py:513-838), channels in
    its order: with neglect_polarity [image?] + sort channels, otherwise [pos image?, pos sort..., neg image?, neg sort...]; one
    sort channel, or len(quantize_sort) of them for a list.  The batched sibling of dist_batch: one upload, one evrep_time_index,
    one polstats launch, one evrep_sort_image.  Unlike the reference (and reshape_then_acc_sort here), the caller's time column is
    NOT overwritten with the time indices.

    Refused on the host, before anything is uploaded: denoise_image with use_image, or denoise_sort, raise the NameError the
    reference raises; an empty window, and with strict=False a polarity class without a positive time index, raise RuntimeError
    with the text of the reference's max() of an empty selection; a window whose microsecond indices decrease raises ValueError
    naming the sample (the reference's consecutive ranks are dense ranks only where they never do); strict=True refuses windows of
    2^24 events and more."""
    classes, qs = _sort_options(neglect_polarity, use_image, quantize_sort, denoise_image, denoise_sort)
    wins = [_as_f64(e) for e in event_tensors]
    status = np.zeros(len(wins), np.uint32)
    for b, w in enumerate(wins):
        if len(w) == 0:
            status[b] |= _lib.SORT_EMPTY
            continue
        idx = (w[:, 2] * TIME_SCALE).astype(np.int64)
        if (idx[1:] < idx[:-1]).any():
            status[b] |= _lib.SORT_DECREASING
        val = (idx != idx[0]) if global_time else (idx > 0)       # the event's value (rank or index) is positive
        for k, c in enumerate(classes):
            sel = np.ones(len(w), bool) if c == ANY else (w[:, 3] > 0 if c == POS else w[:, 3] < 0)
            if not (val & sel).any():
                status[b] |= _lib.SORT_NO_INDEX << k
    err = sort_status_error(status, strict)
    if err is not None:
        raise err
    rows = [_window(w, height, width)[0] for w in wins]
    batch = EventBatch.from_numpy(rows, height, width, device=device)
    t = torch.from_numpy(np.ascontiguousarray(np.concatenate([w[:, 2] for w in wins]))).to(batch.device)
    return _sort(batch, t, global_time, strict, classes, qs, use_image)[0]


# ---------------------------------------------------------------------------------------------
# n_imagenet's wrappers of the path's own builders (imagenet.py:1002-1137)
# ---------------------------------------------------------------------------------------------
def fix_events_training(events):
    """(N, 4) float array -> structured array with '<f8' fields x, y, t, p (imagenet.py:1002-1006)."""
    ev = np.ascontiguousarray(np.asarray(events, dtype=np.float64).reshape(-1, 4))
    return ev.view([("x", "<f8"), ("y", "<f8"), ("t", "<f8"), ("p", "<f8")]).reshape(-1)


def _prep(event_tensor, augment, kwargs):
    if augment is not None:
        event_tensor = augment(event_tensor)
    return fix_events_training(_as_f64(event_tensor)), kwargs.get("height", IMAGE_H), kwargs.get("width", IMAGE_W)


def reshape_then_optimized(event_tensor, augment=None, **kwargs):
    from .representations.optimized_representation import get_optimized_representation
    data, H, W = _prep(event_tensor, augment, kwargs)
    rep = get_optimized_representation(data, data.shape[0], H, W)
    return torch.tensor(rep.transpose(2, 0, 1)).float()


def reshape_then_event_stack(event_tensor, augment=None, **kwargs):
    from .representations.event_stack import EventStack
    data, H, W = _prep(event_tensor, augment, kwargs)
    data["p"] = (data["p"] + 1) // 2
    transformation = EventStack(12, data.shape[0], H, W)
    post = transformation.post_stack(transformation.pre_stack(data, data[-1]["t"]))
    return torch.tensor(post.transpose(3, 0, 1, 2)[..., 0]).float()


def reshape_then_tore(event_tensor, augment=None, **kwargs):
    from .representations.tore import events2ToreFeature
    data, H, W = _prep(event_tensor, augment, kwargs)
    x, y, ts, pol = data["x"], data["y"], data["t"], data["p"]
    x = x - min(x) + 1          # the reference's shift to 1-based coordinates (:1095-1096)
    y = y - min(y) + 1
    rep = events2ToreFeature(x, y, ts, pol, ts[-1], 6, (H, W))
    return torch.tensor(rep.transpose(2, 0, 1)).float()


def reshape_then_time_surface(event_tensor, augment=None, **kwargs):
    # the reference stores int8 polarities back into a '<f8' field and then indexes memory[p, y, x] with it
    raise IndexError("only integers, slices (`:`), ellipsis (`...`), numpy.newaxis (`None`) and integer or boolean "
                     "arrays are valid indices")


# ---------------------------------------------------------------------------------------------
# the same three wrappers for a batch: the rows formed on the device (csrc/evrep_study.hip), then the batched builders
# ---------------------------------------------------------------------------------------------
STUDY_NAMES = ("optimized", "event_stack", "tore")
_STUDY_EMPTY_ERRORS = {      # what reshape_then_<name> raises for an empty tensor, and where
    "optimized": (ValueError, "zero-size array to reduction operation minimum which has no identity"),   # t.min() on no events
    "event_stack": (IndexError, "index -1 is out of bounds for axis 0 with size 0"),                     # data[-1]["t"]
    "tore": (ValueError, "min() arg is an empty sequence"),                                              # min(x)
}


def _study_name(name):
    if name == "time_surface":
        reshape_then_time_surface(None)           # the reference cannot run it: its IndexError
    if name not in STUDY_NAMES:
        raise KeyError(name)
    return {"optimized": _lib.STUDY_MDES, "event_stack": _lib.STUDY_STACK, "tore": _lib.STUDY_TORE}[name]


def study_status_error(name, status):
    """The exception the status words of evrep_nimg_study_rows stand for under reshape_then_<name> (None: no window is refused),
    naming the first such sample: the wrapper's own exception for an empty tensor, ValueError for times that cannot be cast or
    rebased into int32, and for EventStack ValueError for a window with rows behind its last time."""
    from ._lib import STUDY_EMPTY, STUDY_FUTURE, STUDY_T_RANGE
    status = np.asarray(status)
    hit = np.flatnonzero(status & STUDY_EMPTY)
    if hit.size:
        cls, text = _STUDY_EMPTY_ERRORS[name]
        return cls("%s (sample %d: empty event tensor)" % (text, int(hit[0])))
    hit = np.flatnonzero(status & STUDY_T_RANGE)
    if hit.size:
        return ValueError("sample %d: a time that is NaN or not below 2^63, or whole seconds that span more than int32 holds"
                          % int(hit[0]))
    hit = np.flatnonzero(status & STUDY_FUTURE) if name == "event_stack" else np.zeros(0, np.int64)
    if hit.size:
        return ValueError("sample %d: rows later than the window's last time (descending or negative times); the batched form "
                          "builds the past half only, reshape_then_event_stack builds such a window" % int(hit[0]))
    return None


def _study_rows(batch, t, xy, want):
    """evrep_nimg_study_rows on the rows of `batch` ([x.long(), y.long(), 0, sign p]), their float64 times and untruncated
    coordinates -> dict of device tensors: "mdes" / "stack" / "tore" ((total, 4) int32, the wanted sets only), "sample_times"
    ((B,) float64, with "tore"), "status" ((B,) uint32).  Nothing waits for the device."""
    B, total, dev, api = batch.B, batch.total, batch.device, batch.api
    if B == 0:
        raise ValueError("no window")
    batch._per_event(t, "t")
    if int(batch.offsets_host[0]) != 0 or int(batch.offsets_host[-1]) != total:
        raise ValueError("the batch's offsets must run from 0 to its %d rows: the row sets are written at the offsets" % total)
    tore = bool(want & _lib.STUDY_TORE)
    if tore:
        _lib.want(xy, "xy (TORE needs the untruncated coordinates)", torch.float64, (total, 2), device=dev)
    nbytes = api.evrep_nimg_study_rows_scratch_bytes(B, total)
    if nbytes == 0:
        raise ValueError("evrep_nimg_study_rows does not take %d windows" % B)
    n = max(total, 1)
    sets = [k for k, bit in (("mdes", _lib.STUDY_MDES), ("stack", _lib.STUDY_STACK), ("tore", _lib.STUDY_TORE)) if want & bit]
    out = torch.empty((len(sets) * n, 4), dtype=torch.int32, device=dev)
    res = {k: out[j * n:j * n + n] for j, k in enumerate(sets)}
    meta = torch.empty(nbytes + B * 16, dtype=torch.uint8, device=dev)         # scratch, sample times, status words
    res["sample_times"] = meta[nbytes:nbytes + B * 8].view(torch.float64)
    res["status"] = meta[nbytes + B * 8:nbytes + B * 12].view(torch.uint32)
    if total == 0:       # an empty tensor has no address: one row nothing reads
        rows_in, t_in, xy_in = out.new_zeros((1, 4)), meta.new_zeros(8).view(torch.float64), meta.new_zeros(16).view(torch.float64)
    else:
        rows_in, t_in, xy_in = batch.events, t, xy
    with torch.cuda.device(dev):
        api.evrep_nimg_study_rows(ptr(rows_in), ptr(t_in), ptr(xy_in) if tore else None, ptr(batch.offsets), B, batch.H, batch.W,
                                  int(want), *[ptr(res.get(k)) for k in ("mdes", "stack", "tore")],
                                  ptr(res["sample_times"]) if tore else None, ptr(res["status"]), ptr(meta), stream_ptr())
    for k in sets:
        res[k] = res[k][:total]
    return res


def _study(name, batch, t, xy):
    """The part of study_batch behind the upload (n_imagenet_front.study_device enters here with device-made rows): the rows of
    reshape_then_<name> from evrep_nimg_study_rows, the batched builder on an EventBatch over them, the cast and the channel-first
    transpose (evrep_voxel_normalize without its normalisation) -> ((B, 12, H, W) float32, (B,) uint32 status words, both on the
    device).  Nothing waits for the device."""
    from .engine import voxel_normalize
    want = _study_name(name)
    r = _study_rows(batch, t, xy, want)
    rows = r[{"optimized": "mdes", "event_stack": "stack", "tore": "tore"}[name]]
    nb = EventBatch(rows, batch.offsets_host, batch.H, batch.W, max_events_per_window=int(batch.plan.max_events_per_window),
                    plan_flags=int(batch.plan.flags))
    if name == "optimized":
        rep = nb.optimized(scale=1.0, dtype=torch.float64)
    elif name == "event_stack":
        rep = nb.event_stack(12, premap=2, scale=1.0)            # the rows hold the final -1 / +1 (EventStack.pre_stack's 2p - 1)
    else:
        rep = nb.tore(k=6, frame_mode=2, scale=1.0, times_f64=t, sample_times_f64=r["sample_times"])
    return voxel_normalize(rep, normalize=False), r["status"]


def study_batch(name, event_tensors, height=IMAGE_H, width=IMAGE_W, device="cuda:0"):
    """reshape_then_optimized / reshape_then_event_stack / reshape_then_tore (name "optimized", "event_stack", "tore") for a batch:
    a list of (N_b, 4) float64 event tensors [x, y, t_seconds, p], p in {-1, 0, +1}, coordinates inside the frame -> (B, 12, H, W)
    float32 device tensor; window b is what reshape_then_<name>(event_tensors[b], height=height, width=width) returns (ERGO-12 and
    EventStack bit for bit).  The batched sibling of accumulate_batch, dist_batch and sort_batch: one upload of the rows, their
    times and coordinates; evrep_nimg_study_rows; the binning pass and the builder for B windows; one cast-and-transpose launch.

    Refused, naming the sample: an empty tensor (the exception reshape_then_<name> raises for one), times that are NaN, not below
    2^63 or whose whole seconds span more than int32 holds (ValueError), for "event_stack" a window with rows later than its last
    time (ValueError: the batched form builds the past half only), coordinates outside the frame (RuntimeError) and a polarity
    outside {-1, 0, +1} (ValueError).  "time_surface" raises the IndexError of reshape_then_time_surface, any other name KeyError."""
    _study_name(name)
    wins = [_as_f64(e) for e in event_tensors]
    for b, w in enumerate(wins):
        if len(w) and not np.isin(w[:, 3], (-1.0, 0.0, 1.0)).all():
            raise ValueError("sample %d: the batched form takes polarities -1, 0 and +1" % b)
    batch = EventBatch.from_numpy([_window(w, height, width)[0] for w in wins], height, width, device=device)
    cat = np.concatenate(wins) if wins else np.zeros((0, 4))
    tx = torch.from_numpy(np.ascontiguousarray(cat[:, [2, 0, 1]].T)).to(batch.device)          # one upload: t, x, y
    t, xy = tx[0].contiguous(), tx[1:].t().contiguous()
    images, status = _study(name, batch, t, xy)
    err = study_status_error(name, status.cpu().numpy())
    if err is not None:
        raise err
    return images
