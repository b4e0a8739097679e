"""CPU-only: the batched ev-licious voxel grid (evrep_voxel_normalize, EventBatch.evl_voxel_grid).  The numpy restatement of
its semantics (evl_voxel_ref.py) reproduces the reference's own normalised grids from its raw ones; the C entry point refuses
bad arguments before any launch; without a device the Python entries raise.  No kernel is launched."""
import ctypes
import types

import numpy as np
import pytest

from conftest import load_golden
from evl_voxel_ref import gamma, restate


@pytest.fixture(scope="module")
def lib():
    from event_representation_study_amd import build, _lib
    build.build()
    return _lib.load()


@pytest.mark.parametrize("golden,raw,norm", [("evlicious_voxel", "a_raw5", "a_norm5"), ("evlicious_voxel", "b_raw5", "b_norm5"),
                                             ("boundary", "sp_a_raw5", "sp_a_norm5"), ("boundary", "sp_b_raw5", "sp_b_norm5"),
                                             ("boundary", "evl_raw5_0", "evl_norm5_0")])
def test_restatement_reproduces_the_reference(golden, raw, norm):
    """The reference normalises in float32 (numpy's pairwise mean / std of a float32 array); the float64 restatement stays
    within the tolerance the per-sample route is held to (test_gpu_reference_api.py), with the same zero pattern."""
    g = load_golden(golden)
    out, st, _ = restate(g[raw], True)
    assert st["applied"] == 1 and st["n"] == int(np.count_nonzero(g[raw]))
    print("%s: max |diff| %.3g, bit-equal %.4f" % (raw, float(np.abs(out - g[norm]).max()),
                                                   float((out.view(np.uint32) == g[norm].view(np.uint32)).mean())))
    np.testing.assert_allclose(out, g[norm], rtol=1e-5, atol=1e-6)
    assert np.array_equal(out == 0, g[norm] == 0)


def test_restatement_degenerate_windows_and_bound():
    z = np.zeros((3, 4, 5), np.float64)
    out, st, tol = restate(z)
    assert st == dict(n=0, mean=0.0, std=0.0, applied=0, e_mean=0.0, e_std=0.0) and not out.any() and not tol.any()
    one = z.copy()
    one[1, 2, 3] = -3.0
    out, st, tol = restate(one)
    assert (st["n"], st["mean"], st["std"], st["applied"]) == (1, -3.0, 0.0, 0) and np.array_equal(out, one.astype(np.float32))
    ones = z.copy()
    ones[0] = 1.0
    out, st, _ = restate(ones)
    assert (st["n"], st["mean"], st["std"], st["applied"]) == (20, 1.0, 0.0, 0) and np.array_equal(out, ones.astype(np.float32))
    pm = z.copy()
    pm[0], pm[1] = 1.0, -1.0
    out, st, tol = restate(pm)
    assert (st["mean"], st["std"], st["applied"]) == (0.0, 1.0, 1)
    assert np.array_equal(out[0], np.full((4, 5), np.float32(1.0 / (1e-5 + 1.0)))) and not out[2].any()
    # the bound is a few float32 roundings wide at most, and exactly zero where no arithmetic happens
    assert not tol[2].any() and 0 < tol[0].max() < 4 * 2.0 ** -24
    assert not restate(pm, False)[2].any() and np.array_equal(restate(pm, False)[0], pm.astype(np.float32))
    assert gamma(1) > 2.0 ** -53 and abs(gamma(1000) / (1000 * 2.0 ** -53) - 1) < 1e-12


P = ctypes.c_void_p
GOOD = dict(grid=P(4096), dtype=0, B=2, H=60, W=80, bins=5, flags=1, out=P(8192), stats=P(256), scratch=P(512))


def _call(lib, **kw):
    a = dict(GOOD, **kw)
    return lib.evrep_voxel_normalize(a["grid"], a["dtype"], a["B"], a["H"], a["W"], a["bins"], a["flags"], a["out"], a["stats"],
                                     a["scratch"], None)


@pytest.mark.parametrize("bad", [dict(grid=None), dict(out=None), dict(scratch=None),
                                 dict(grid=P(4104)), dict(out=P(8196)), dict(out=P(8200)), dict(scratch=P(520)), dict(stats=P(264)),
                                 dict(bins=0), dict(bins=17), dict(bins=-1),
                                 dict(B=0), dict(B=65536), dict(H=0), dict(W=0), dict(H=-4),
                                 dict(H=32768, W=32768, bins=2),        # H * W * bins == 2^31
                                 dict(H=65536, W=32768, bins=1),        # H * W == 2^31
                                 dict(H=65536, W=65536, bins=16),       # wraps a 32-bit product to 0
                                 dict(dtype=2), dict(dtype=-1),
                                 dict(flags=2), dict(flags=3), dict(flags=0x80000001),
                                 dict(flags=0, scratch=None)],          # statistics without the normalisation
                         ids=lambda d: ",".join("%s=%s" % (k, getattr(v, "value", v)) for k, v in d.items()))
def test_entry_refuses_bad_arguments_before_any_launch(lib, bad):
    from event_representation_study_amd._lib import EVREP_EINVAL
    assert _call(lib, **bad) == EVREP_EINVAL


def test_scratch_size(lib):
    f = lib.evrep_voxel_normalize_scratch_bytes
    assert f(1, 1, 1, 1) > 0 and f(32, 480, 640, 5) >= 32 * (2 * 8 + 4)
    assert f(32, 480, 640, 5) % 256 == 0 and f(32, 480, 640, 5) <= 1 << 20      # partial sums only: never a copy of the batch
    assert f(0, 480, 640, 5) == 0 and f(1, 480, 640, 17) == 0 and f(1, 32768, 32768, 2) == 0 and f(65536, 8, 8, 1) == 0
    assert f(1, 32768, 32767, 2) > 0                                             # the largest window: 2^31 - 65536 values


def test_binding_and_header_agree():
    import os
    import re
    from conftest import ROOT
    from event_representation_study_amd import _lib
    text = open(os.path.join(ROOT, "include", "evrep.h")).read()
    assert int(re.search(r"^#define\s+EVREP_VOXNORM_NORMALIZE\s+(\d+)u", text, flags=re.M).group(1)) == _lib.VOXNORM_NORMALIZE
    assert len(_lib.SYMBOLS["evrep_voxel_normalize"][1]) == 11 and len(_lib.SYMBOLS["evrep_voxel_normalize_scratch_bytes"][1]) == 4


def test_no_cpu_fallback():
    """Without a HIP device the batched grid raises; nothing is computed on the host."""
    import torch
    if torch.cuda.is_available():
        return                       # (with a device there is nothing to refuse; test_gpu_evl_voxel_batch.py runs these entries)
    from event_representation_study_amd import _lib
    from event_representation_study_amd.engine import EventBatch, voxel_normalize
    from event_representation_study_amd.evlicious_tools import events_to_voxel_grid_batch
    e = types.SimpleNamespace(x=np.arange(4, dtype=np.uint16), y=np.zeros(4, np.uint16), t=np.arange(4), p=np.ones(4, np.int8),
                              width=8, height=8)
    with pytest.raises(_lib.EvrepError):
        events_to_voxel_grid_batch([e, e], 5)
    with pytest.raises(_lib.EvrepError):
        EventBatch.evl_voxel_grid(EventBatch.__new__(EventBatch), 5)
    with pytest.raises(_lib.EvrepError):
        voxel_normalize(torch.zeros((1, 2, 2, 5), dtype=torch.float64))
