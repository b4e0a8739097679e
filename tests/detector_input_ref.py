"""The tests' own numpy restatement of the detector input's stages R (resize), L (letterbox), W (affine warp), F (flips) and
the conversion, written from the stage definitions of include/evrep.h / DESIGN.md 3.10 and shared by
test_detector_input_cpu.py and test_gpu_detector_input.py.  Nothing of event_representation_study_amd.detector_input is used;
the per-axis resize weights are gwd_pipeline's host matrices, which is where the definition takes them from."""
import numpy as np

from event_representation_study_amd.gwd_pipeline import area_weights, linear_weights

REF_HYP = {"degrees": 0.373, "translate": 0.245, "scale": 0.898, "shear": 0.602, "flipud": 0.5, "fliplr": 0.5}


def _taps(src, dst, interpolation):
    Wm = (area_weights if interpolation == "area" else linear_weights)(src, dst)
    rows = []
    for d in range(dst):
        nz = np.nonzero(Wm[d])[0]
        rows.append((int(nz[0]), Wm[d, nz[0]:nz[-1] + 1]))
    return rows


def resize_ref(img, new_h, new_w, interpolation):
    """(..., H, W, C) of dtype T -> (..., new_h, new_w, C) of T: x taps, then y taps, float64 sums in tap order, one cast."""
    src = img.astype(np.float64)
    xt, yt = _taps(img.shape[-2], new_w, interpolation), _taps(img.shape[-3], new_h, interpolation)
    tmp = np.zeros(img.shape[:-2] + (new_w, img.shape[-1]))
    for ox, (s, w) in enumerate(xt):
        for k, wk in enumerate(w):
            tmp[..., ox, :] += src[..., s + k, :] * wk
    out = np.zeros(img.shape[:-3] + (new_h, new_w, img.shape[-1]))
    for oy, (s, w) in enumerate(yt):
        acc = np.zeros_like(out[..., oy, :, :])
        for k, wk in enumerate(w):
            acc += tmp[..., s + k, :, :] * wk
        out[..., oy, :, :] = acc
    return out.astype(img.dtype)


def geometry_ref(h0, w0, S, augment):
    r = S / max(h0, w0)
    rh, rw = (int(h0 * r), int(w0 * r)) if r != 1 else (h0, w0)
    interp = "area" if (r < 1 and not augment) else "linear"
    r2 = min(S / rh, S / rw)
    if not augment:
        r2 = min(r2, 1.0)
    nw, nh = int(round(rw * r2)), int(round(rh * r2))
    dw, dh = (S - nw) / 2, (S - nh) / 2
    return dict(r=r, rh=rh, rw=rw, interp=interp, ratio=r2, nh=nh, nw=nw, dw=dw, dh=dh, top=int(round(dh - 0.1)),
                bottom=int(round(dh + 0.1)), left=int(round(dw - 0.1)), right=int(round(dw + 0.1)))


def letterbox_ref(rep, S, augment, pad=114.0):
    """Stages R + L: (B, H, W, C) of T -> (B, S, S, C) of T."""
    B, h0, w0, C = rep.shape
    g = geometry_ref(h0, w0, S, augment)
    im = rep if g["r"] == 1 else resize_ref(rep, g["rh"], g["rw"], g["interp"])
    if (g["rw"], g["rh"]) != (g["nw"], g["nh"]):
        im = resize_ref(im, g["nh"], g["nw"], "linear")
    out = np.empty((B, S, S, C), dtype=rep.dtype)
    out[...] = np.broadcast_to(np.asarray(pad, dtype=rep.dtype), (C,))
    out[:, g["top"]:g["top"] + g["nh"], g["left"]:g["left"] + g["nw"]] = im
    return out


def inverse_ref(M):
    M = np.asarray(M, dtype=np.float64)
    D = M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]
    D = 1.0 / D if D != 0 else 0.0
    m00, m11 = M[1, 1] * D, M[0, 0] * D
    m01, m10 = M[0, 1] * (-D), M[1, 0] * (-D)
    return m00, m01, -m00 * M[0, 2] - m01 * M[1, 2], m10, m11, -m10 * M[0, 2] - m11 * M[1, 2]


def warp_ref(I, M, pad=114.0):
    """Stage W on one (S, S, C) image of T: the fixed-point walk in int64 (the tables asked of it stay far inside)."""
    S, _, C = I.shape
    T = I.dtype.type
    m00, m01, m02, m10, m11, m12 = inverse_ref(M)
    padv = np.broadcast_to(np.asarray(pad, dtype=I.dtype), (C,))
    i = np.arange(S, dtype=np.float64)
    ad, bd = np.rint(m00 * i * 1024).astype(np.int64), np.rint(m10 * i * 1024).astype(np.int64)
    X0, Y0 = np.rint((m01 * i + m02) * 1024).astype(np.int64) + 16, np.rint((m11 * i + m12) * 1024).astype(np.int64) + 16
    X, Y = (X0[:, None] + ad[None, :]) >> 5, (Y0[:, None] + bd[None, :]) >> 5
    sx, sy = np.clip(X >> 5, -32768, 32767), np.clip(Y >> 5, -32768, 32767)
    ax, ay = ((X & 31).astype(I.dtype) / T(32))[..., None], ((Y & 31).astype(I.dtype) / T(32))[..., None]
    framed = np.empty((S + 2, S + 2, C), dtype=I.dtype)          # one ring of border around I: every outside tap lands on it
    framed[...] = padv
    framed[1:-1, 1:-1] = I

    def tap(yy, xx):
        return framed[np.clip(yy, -1, S) + 1, np.clip(xx, -1, S) + 1]

    w00, w01, w10, w11 = (T(1) - ay) * (T(1) - ax), (T(1) - ay) * ax, ay * (T(1) - ax), ay * ax
    return ((tap(sy, sx) * w00 + tap(sy, sx + 1) * w01) + tap(sy + 1, sx) * w10) + tap(sy + 1, sx + 1) * w11


def finish_ref(I, Ms, flipud, fliplr, pad=114.0, scale=None):
    """Stages W, F and the conversion on letterboxed (B, S, S, C) images: -> (B, C, S, S) float32."""
    outs = []
    for b in range(I.shape[0]):
        im = I[b]
        if Ms is not None and Ms[b] is not None and (np.asarray(Ms[b]) != np.eye(3)).any():
            im = warp_ref(im, Ms[b], pad)
        if flipud is not None and flipud[b]:
            im = im[::-1]
        if fliplr is not None and fliplr[b]:
            im = im[:, ::-1]
        chw = im.transpose(2, 0, 1)[::-1].astype(np.float32)
        outs.append(chw if scale is None else chw * np.float32(scale))
    return np.ascontiguousarray(np.stack(outs))


def detector_input_ref(rep, S, augment, Ms=None, flipud=None, fliplr=None, pad=114.0, scale=None):
    return finish_ref(letterbox_ref(rep, S, augment, pad), Ms, flipud, fliplr, pad, scale)


def load_golden(path):
    z = np.load(path)
    cases = []
    for i in range(int(z["n_cases"])):
        cases.append({k[len("c%d_" % i):]: z[k] for k in z.files if k.startswith("c%d_" % i)})
    return cases
