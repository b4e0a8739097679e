"""CPU-only: the C-ABI library loads, exports every symbol include/evrep.h declares, and its
host-side entry points (plan / workspace sizing, argument checks) behave.  No kernel is launched."""
import ctypes
import os
import re

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    from event_representation_study_amd import build, _lib
    build.build()
    return _lib.load()


def _declared_functions():
    text = open(os.path.join(ROOT, "include", "evrep.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(evrep_[a-z0-9_]+)\s*\(", text)))


def test_every_declared_symbol_is_exported_and_bound(lib):
    from event_representation_study_amd import _lib
    declared = _declared_functions()
    assert len(declared) >= 14
    assert set(declared) == set(_lib.SYMBOLS), (set(declared) ^ set(_lib.SYMBOLS))
    for name in declared:
        assert getattr(lib, name) is not None
    assert lib.evrep_abi_version() == _lib.ABI_VERSION


def _declared_plan_flags():
    text = open(os.path.join(ROOT, "include", "evrep.h")).read()
    return {name: int(value) for name, value in re.findall(r"^#define\s+EVREP_(PLAN_[A-Z0-9_]+)\s+(\d+)u\b", text, flags=re.M)}


def test_plan_flags_match_header():
    """A bit renumbered on one side would send a "force the stream / force the ordered path" switch to the wrong path, whose
    results are bit-equal: only this comparison of the two tables notices."""
    from event_representation_study_amd import _lib
    header = _declared_plan_flags()
    python = {name: value for name, value in vars(_lib).items() if name.startswith("PLAN_")}
    assert len(header) >= 22
    assert header == python, (set(header.items()) ^ set(python.items()))
    assert all(v > 0 and v & (v - 1) == 0 for v in header.values())
    assert len(set(header.values())) == len(header)
    assert {bit for _, bit in _lib._ENV_FLAGS} <= set(header.values())


def test_plan_struct_layout_matches_header(lib):
    from event_representation_study_amd._lib import Plan
    p = Plan()
    assert lib.evrep_plan_init(ctypes.byref(p), 32, 480, 640, 32 * 50000, 50000) == 0
    assert (p.B, p.H, p.W, p.total_events, p.max_events_per_window) == (32, 480, 640, 1600000, 50000)
    assert p.nchunk == 5 and p.chunk >= 256 and p.nblk * p.chunk >= 50000
    offs = [p.off_meta, p.off_table, p.off_stats, p.off_rowoff, p.off_chunkoff, p.off_sorted1, p.off_sorted2,
            p.off_cuts, p.off_scratch]
    assert offs == sorted(offs) and all(o % 256 == 0 for o in offs)
    assert lib.evrep_workspace_bytes(ctypes.byref(p)) == p.workspace_bytes > p.off_scratch
    # 2 x 16 B per event for the two partition levels dominate the workspace
    assert p.workspace_bytes >= 2 * 16 * 1600000


@pytest.mark.parametrize("args", [(0, 480, 640, 10, 10), (1, 0, 640, 10, 10), (1, 480, 5000, 10, 10),
                                  (1, 480, 640, 10, 11), (1, 480, 640, -1, 0), (1, 480, 640, 1 << 31, 1),
                                  (65536, 8, 8, 10, 10),            # windows ride gridDim.z
                                  (60000, 4096, 4096, 10, 10)])     # > 2^31 work units
def test_plan_init_rejects_bad_arguments(lib, args):
    from event_representation_study_amd._lib import Plan, EVREP_EINVAL
    assert lib.evrep_plan_init(ctypes.byref(Plan()), *args) == EVREP_EINVAL


def test_large_window_partition_geometry(lib):
    from event_representation_study_amd._lib import Plan
    p = Plan()
    assert lib.evrep_plan_init(ctypes.byref(p), 1, 720, 1280, 1000000, 1000000) == 0
    assert p.nblk <= 128 and p.nblk * p.chunk >= 1000000 and p.chunk % 256 == 0 and p.nchunk == 10


def test_null_and_misaligned_pointers_are_refused_before_any_launch(lib):
    from event_representation_study_amd._lib import Plan, EVREP_EINVAL
    p = Plan()
    assert lib.evrep_plan_init(ctypes.byref(p), 1, 8, 8, 4, 4) == 0
    assert lib.evrep_bin_events(ctypes.byref(p), None, None, None, None) == EVREP_EINVAL
    assert lib.evrep_bin_events(ctypes.byref(p), ctypes.c_void_p(8), ctypes.c_void_p(256), ctypes.c_void_p(256),
                                None) == EVREP_EINVAL   # events not 16-byte aligned
    assert lib.evrep_gwd_padded_l1(None, 1, 4, None, 1, 4, 0.7, None, None, None) == EVREP_EINVAL
    i32 = (ctypes.c_int32 * 2)(0, 0)
    assert lib.evrep_polstats(ctypes.byref(p), ctypes.c_void_p(256), ctypes.c_void_p(256), ctypes.c_void_p(256),
                              ctypes.c_void_p(256), 17, i32, i32, 0.3, ctypes.c_void_p(256), None) == EVREP_EINVAL
    bad = (ctypes.c_int32 * 2)(0, 9)   # unknown statistic
    assert lib.evrep_polstats(ctypes.byref(p), ctypes.c_void_p(256), ctypes.c_void_p(256), ctypes.c_void_p(256),
                              ctypes.c_void_p(256), 2, i32, bad, 0.3, ctypes.c_void_p(256), None) == EVREP_EINVAL
    assert lib.evrep_gwd_scratch_bytes(12500, 14400) > 14 * 14400 * 4


def test_scratch_sizes_are_the_published_ones(lib):
    """Scratch sizes are a contract: callers size allocations they keep across library versions with them.  The table was
    recorded by tests/golden/make_golden_scratch_sizes.py, a handful of argument tuples per function, one per edge of its
    formula."""
    import json
    from event_representation_study_amd import _lib
    with open(os.path.join(ROOT, "tests", "golden", "scratch_sizes.json")) as f:
        table = json.load(f)
    assert sorted(table) == sorted(name for name in _lib.SYMBOLS if name.endswith("_scratch_bytes"))
    for name, rows in table.items():
        assert len(rows) >= 4, name
        for args, size in rows:
            assert getattr(lib, name)(*args) == size, (name, args)


# The pointer arguments of every entry point whose checks are written with the shared helpers of evrep_capi_shared.h, in
# call order: _p(a) a required pointer aligned to a bytes (1: no alignment stated), _opt(a) an optional one (NULL allowed,
# a misaligned one refused), _PLAN a real plan (B 1, 8 x 8, 4 events), _host(...) an int32 array the entry reads on the host,
# _FRAME one frame descriptor read on the host; everything else is a scalar inside its stated range.  Each call is valid but
# for its addresses, which are made up: the test runs only where there is no device.
def _p(align=1):
    return ("ptr", align)


def _opt(align):
    return ("opt", align)


def _host(*values):
    return ("host", values)


_PLAN, _FRAME = ("plan",), ("frame",)
_COMMON = [_PLAN, _p(16), _p(), _p(256)]
_POINTER_TABLE = {
    "evrep_bin_events": _COMMON + [None],
    "evrep_probe_store": [_p(16), 12288, None],
    "evrep_mdes": _COMMON + [2, _host(0, 0), _host(0, 0), _host(0, 0), 1.0, 0, _p(), None],
    "evrep_mdes_ex": _COMMON + [2, _host(0, 0), _host(0, 0), _host(0, 0), 1.0, 0, _p(), _opt(1), _opt(1), None],
    "evrep_optimized": _COMMON + [1.0, 0, _p(), None],
    "evrep_mdes_sbt_windows": [_p(16), _p(), 1, 8, 8, _p(), _p(), None],
    "evrep_event_stack": _COMMON + [4, 0, 1.0, _p(), None],
    "evrep_time_surface": _COMMON + [2, _opt(1), 1.0, 0, 1.0, 0, _p(), None],
    "evrep_time_surface_ftime": _COMMON + [2, _opt(1), _opt(1), 1.0, 0, 1.0, 0, _p(), None],
    "evrep_tore": _COMMON + [2, 0, _opt(1), 1.0, _p(), None],
    "evrep_tore_ftime": _COMMON + [2, 0, _opt(1), _opt(1), _opt(1), 1.0, _p(), None],
    "evrep_voxel": _COMMON + [2, 0, 1.0, _p(), None],
    "evrep_voxel_range": _COMMON + [2, 0, 1.0, _opt(1), _p(), None],
    "evrep_voxel_tnorm": _COMMON + [_p(), 2, 1.0, _p(), None],
    "evrep_voxel_subpixel": _COMMON + [_p(), 2, _opt(1), _p(), None],
    "evrep_polstats": _COMMON + [_p(), 2, _host(0, 0), _host(0, 0), 0.3, _p(), None],
    "evrep_est_voxel": _COMMON + [_p(), 2, _p(), 1, _p(), 1, 0.0, 1.0, _p(), None],
    "evrep_est_voxel_backward": [_p(16), _p(), 1, 8, 8, _p(), 2, _p(), 1, _p(), 1, 0.0, 1.0, _p(), _p(8), _p(16), None],
    "evrep_est_prepare": [_p(4), 10, 1, 8, 8, _p(16), _p(8), _p(4), _p(4), _p(4), None],
    "evrep_gwd_padded_l1": [_p(), 10, 4, _p(), 10, 4, 0.7, _p(256), _p(), None],
    "evrep_gwd_padded_l1_batch": [2, _p(), _opt(1), _p(), 4, _p(), _opt(1), _p(), 4, 10, 10, 0.7, _p(256), _p(), None],
    "evrep_otmi_event_clouds": [_p(16), _p(), 1, 8, 8, 10, _p(), _p(), _p(), _p(16), None],
    "evrep_otmi_rep_clouds": [_p(), 0, 1, 1, 4, 2, _p(), 10, _p(), _p(), _p(16), None],
    "evrep_otmi_rep_clouds_bank": [_p(), _p(), 0, 1, 4, 2, 3, 0, _host(0, 1), 2, _p(), 10, _p(), _p(), _p(16), None],
    "evrep_resize_taps": [_p(), 0, 1, 8, 8, 1, 4, 4, 1, _p(), _p(), _p(), _p(), _p(), _p(), 1.0, 0, _p(), None],
    "evrep_entropic_gw": [_p(), 4, _p(), 4, _p(), _p(), 0, 0.1, 1, 1, 0, _p(256), _opt(1), _p(), None],
    "evrep_filter_pixel_fsm": _COMMON + [0, 1.0, None, _p(8), _p(), None],
    "evrep_filter_background": _COMMON + [1.0, 1, None, _p(8), _p(), None],
    "evrep_filter_mask_gather": [_p(16), _p(), 1, 8, 8, 4, _p(), _p(), None],
    "evrep_filter_cell_map": [_p(16), 4, 8, 8, 1, 1, _p(16), None],
    "evrep_filter_compact": [_p(16), _p(), 1, _p(), _p(16), _p(8), _p(16), None],
    "evrep_time_to_index": [_p(8), 4, _p(8), 2, _p(8), None],
    "evrep_windows_gather": [_p(2), _p(2), _p(8), _p(), 4, _p(8), _p(8), _p(8), 1, 0, _opt(8), _p(16), _p(8), _p(4), None],
    "evrep_nimg_prepare": [_p(16), _p(8), 1, _opt(8), _p(8), 1.0, 1.0, 8, 8, 0, _p(16), _p(8), _p(8), _opt(16), _p(8), _p(4), _p(16), None],
    "evrep_dist": [_p(4), 1, 8, 8, 0.99, 3.0, _p(4), _p(16), None],
    "evrep_dense_rank_f32": [_p(4), _p(8), 1, _p(4), _opt(4), _p(16), None],
    "evrep_time_index": [_p(8), _p(8), 1, 0, _p(8), _p(4), _p(16), None],
    "evrep_sort_image": [_p(4), 1, 8, 8, 1, 0, _host(1, 2), 2, _p(4), _p(4), _p(16), None],
    "evrep_nimg_study_rows": [_p(16), _p(8), _p(16), _p(8), 1, 8, 8, 7, _p(16), _p(16), _p(16), _p(8), _p(4), _p(16), None],
    "evrep_detector_input": [_p(8), 0, 1, 8, 8, 1, 4, 4, 1, _p(4), _p(4), _p(8), _p(4), _p(4), _p(8), 8, 0, 0, _p(8), _opt(4), _opt(4),
                             1.0, _p(4), None],
    "evrep_resize_tap_tables": [_p(4), 1, 8, _p(4), _p(4), _p(8), 16, 16, None],
    "evrep_detector_input_frames": [_FRAME, 1, 0, 1, 8, _p(4), _p(4), _p(8), 64, 64, _p(8), _opt(4), 1.0, _p(8), _p(4), None],
    "evrep_voxel_normalize": [_p(16), 0, 1, 8, 8, 2, 1, _p(16), _opt(16), _p(16), None],
    "evrep_decode_state_init": [_p(8), None],
    "evrep_decode_dat": [_p(16), 4, 8, 0, 8, 8, 0, _p(16), _p(16), _p(16), _p(16), 10, _p(8), _opt(256), None],
    "evrep_decode_bin5": [_p(16), 4, 0, 8, 8, 0, _p(16), _p(16), _p(16), _p(16), 10, _p(8), _opt(256), None],
    "evrep_dat_seek_time": [_p(8), 4, _p(8), 2, 1, _p(8), None],
}


def _pointer_cases():
    cases = [(name, -1, "valid") for name in _POINTER_TABLE]
    for name, spec in _POINTER_TABLE.items():
        for i, a in enumerate(spec):
            if not isinstance(a, tuple):
                continue
            if a[0] != "opt":
                cases.append((name, i, "null"))
            if a[0] in ("ptr", "opt") and a[1] > 1:
                cases.append((name, i, "misaligned"))
    return cases


@pytest.mark.parametrize("name,index,fault", _pointer_cases(), ids=lambda v: str(v))
def test_every_pointer_check_refuses_before_any_launch(lib, name, index, fault):
    """One call per pointer argument and fault: a required pointer NULL, a pointer with a stated alignment off by half of it.
    Each is EVREP_EINVAL; the call with no fault gets past the argument checks (and fails in HIP: there is no device)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: made-up addresses must never be able to reach a launch")
    from event_representation_study_amd._lib import DetinFrame, Plan, EVREP_EINVAL
    fn = getattr(lib, name)
    keep, args = [], []
    for i, (a, ctype) in enumerate(zip(_POINTER_TABLE[name], fn.argtypes)):
        if not isinstance(a, tuple):
            args.append(a)
            continue
        if i == index and fault == "null":
            args.append(None)
            continue
        if a[0] == "plan":
            keep.append(Plan())
            assert lib.evrep_plan_init(ctypes.byref(keep[-1]), 1, 8, 8, 4, 4) == 0
            address = ctypes.addressof(keep[-1])
        elif a[0] == "host":
            keep.append((ctypes.c_int32 * len(a[1]))(*a[1]))
            address = ctypes.addressof(keep[-1])
        elif a[0] == "frame":
            keep.append(DetinFrame(src=0x7000000, H=8, W=8, rh=4, rw=4, T1=1, nh=4, nw=4))
            address = ctypes.addressof(keep[-1])
        elif a[0] == "opt" and i != index:
            address = None
        else:
            address = 0x10000000 + 0x100000 * i + (a[1] // 2 if i == index else 0)
        args.append(None if address is None else ctypes.cast(ctypes.c_void_p(address), ctype))
    assert len(args) == len(fn.argtypes)
    rc = fn(*args)
    if fault == "valid":
        assert rc != EVREP_EINVAL
    else:
        assert rc == EVREP_EINVAL


def test_no_cpu_fallback():
    """Without a GPU the product path must fail loudly (never route through the oracle)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import numpy as np
    from event_representation_study_amd import _lib
    from event_representation_study_amd.engine import EventBatch
    from event_representation_study_amd.representations.optimized_representation import get_optimized_representation
    from event_representation_study_amd.synthetic import make_events, to_structured
    with pytest.raises(_lib.EvrepError):
        EventBatch.from_numpy(np.zeros((4, 4), np.int32), 8, 8)
    with pytest.raises(_lib.EvrepError):
        get_optimized_representation(to_structured(make_events(10, 8, 8)), 10, 8, 8)


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "event_representation_study_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f
                assert "libevrep_oracle" not in src and "evrep_oracle.c" not in src, f
