"""The 16-bit cases of the head's decode and tail: the cases of tests/detector_head_cases.py with their maps rounded to float16
or bfloat16, and two cases of their own that hold every bit pattern of the dtype and every rounding boundary in front of it.

    build(name, dtype)   detector_head_cases.build(name), the maps clamped to the dtype's largest finite value (`extreme` holds
                         +-3e38, which float16 would turn into infinities: inputs must be finite) and rounded to the dtype.
                         cls / reg are lists of torch CPU tensors of the dtype; cls32 / reg32 their exact widenings as float32
                         arrays, what the float32 entries and the host mirrors are given.
    bits16(dtype)        B = 1, nc = 68, R = 16 (68 regression channels), levels 31 x 31 and 1 x 3: 964 anchors x 68 channels =
                         65552 elements per kind.  The reg maps hold ALL 65536 bit patterns of the dtype in order (then zeros), the
                         cls maps the finite ones in order (then zeros).  31 x 31 = 961 is odd, so every second plane starts at an
                         address that is only 2-byte aligned; the level is 15 whole tiles and one anchor.
    rounding(dtype)      B = 1, nc = 68, R = 16, one level of 1 x 3855 anchors: grad_distri and grad_scores (1, 3855, 68) float32
                         hold, for every finite 16-bit value h of the dtype, h itself, the float32 midpoint between h and its
                         successor in magnitude (a tie: it goes to the even neighbour; behind the largest finite value it is the
                         first float32 that rounds to infinity) and the float32 neighbours of that midpoint on both sides; then
                         float32 subnormals, +-0, +-inf, the largest float32 and a NaN.  grad_scores holds them in reverse order.
"""
import numpy as np
import torch

import detector_head_cases as base

F32, F64 = np.float32, np.float64
DTYPES = {"float16": torch.float16, "bfloat16": torch.bfloat16}
#              mantissa bits, smallest normal exponent
_FORMAT = {torch.float16: (10, -14), torch.bfloat16: (7, -126)}


def patterns(dtype):
    """All 65536 bit patterns of the dtype, in order, as a tensor of the dtype."""
    return torch.from_numpy(np.arange(65536, dtype=np.uint16).view(np.int16).copy()).view(dtype)


def bits(t):
    """The 16 bits of every element of a 16-bit tensor, as an int16 tensor."""
    return t.contiguous().view(torch.int16)


def build(name, dtype):
    c = dict(base.build(name))
    top = float(torch.finfo(dtype).max)
    for kind in ("cls", "reg"):
        maps = [torch.from_numpy(np.clip(a, -top, top)).to(dtype) for a in c[kind]]
        assert all(bool(torch.isfinite(m.float()).all()) for m in maps)
        c[kind] = maps
        c[kind + "32"] = [m.float().numpy() for m in maps]
    c["dtype"] = dtype
    return c


def _fill(values, shapes, chans, dtype):
    """`values` (1-D, of the dtype) laid through the levels' (1, chans, h, w) maps in memory order, zeros behind them."""
    maps, at = [], 0
    for h, w in shapes:
        n = chans * h * w
        m = torch.zeros(n, dtype=dtype)
        k = max(0, min(n, values.numel() - at))
        m[:k] = values[at:at + k]
        at += k
        maps.append(m.view(1, chans, h, w))
    assert at >= values.numel()
    return maps


def bits16(dtype):
    shapes, nc, R = ((31, 31), (1, 3)), 68, 16
    pats = patterns(dtype)
    finite = pats[torch.isfinite(pats.float())]
    assert finite.numel() == {torch.float16: 63488, torch.bfloat16: 65280}[dtype]
    reg, cls = _fill(pats, shapes, 4 * (R + 1), dtype), _fill(finite, shapes, nc, dtype)
    return dict(name="bits16", B=1, nc=nc, R=R, use_dfl=True, K=R + 1, shapes=shapes, strides=(8, 16), N=964, cls=cls, reg=reg,
                cls32=[m.float().numpy() for m in cls], reg32=[m.float().numpy() for m in reg], dtype=dtype)


def boundaries(dtype):
    """The float32 values of `rounding`, 1-D."""
    p, emin = _FORMAT[dtype]
    pats = patterns(dtype).float().numpy()
    h = pats[np.isfinite(pats)].astype(F64)
    mag = np.abs(h)
    with np.errstate(divide="ignore"):
        e = np.where(mag > 0, np.floor(np.log2(np.where(mag > 0, mag, 1.0))), emin)
    ulp = np.exp2(np.maximum(e, emin) - p)
    sign = np.where(np.signbit(h), -1.0, 1.0)
    mid64 = sign * (mag + ulp / 2)
    mid = mid64.astype(F32)
    assert (mid.astype(F64) == mid64).all()                               # every midpoint is a float32
    inward, outward = np.nextafter(mid, F32(0)), np.nextafter(mid, (sign * np.inf).astype(F32))
    special = np.array([2.0 ** -149, -2.0 ** -149, 2.0 ** -127, -2.0 ** -127, 0.0, -0.0, np.inf, -np.inf, np.nan], F64).astype(F32)
    tiny = np.array([0x007FFFFF, 0x807FFFFF, 0x00400000, 0x80400001, 0x7F7FFFFF, 0xFF7FFFFF], np.uint32).view(F32)
    return np.concatenate([h.astype(F32), mid, inward, outward, special, tiny])


def rounding(dtype):
    shapes, nc, R, n = ((1, 3855),), 68, 16, 3855
    v = boundaries(dtype)
    assert v.size <= n * 68
    gd = np.zeros(n * 68, F32)
    gd[:v.size] = v
    gs = gd[::-1].copy()
    rng = np.random.default_rng(77)
    cls = [torch.from_numpy((rng.normal(size=(1, nc, 1, n)) * 3.0).astype(F32)).to(dtype)]
    reg = [torch.from_numpy((rng.normal(size=(1, 68, 1, n)) * 2.0).astype(F32)).to(dtype)]
    return dict(name="rounding", B=1, nc=nc, R=R, use_dfl=True, K=R + 1, shapes=shapes, strides=(8,), N=n, cls=cls, reg=reg,
                cls32=[m.float().numpy() for m in cls], reg32=[m.float().numpy() for m in reg], dtype=dtype,
                grad_distri=gd.reshape(1, n, 68), grad_scores=gs.reshape(1, n, nc))
