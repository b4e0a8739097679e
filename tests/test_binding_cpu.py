"""CPU-only: the two handles on libevrep.so (_lib.load: the raw C ABI; _lib.api: the checked one the package calls), the one
status message, the one tensor check, and the dependencies build.py derives from the sources.  No kernel is launched."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT


@pytest.fixture(scope="module")
def handles():
    from event_representation_study_amd import build, _lib
    build.build()
    return _lib.load(), _lib.api()


def _status_functions_of_the_header():
    text = open(os.path.join(ROOT, "include", "evrep.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\bint\s+(evrep_[a-z0-9_]+)\s*\(", text)) - {"evrep_abi_version"}


def test_every_status_function_is_checked_and_nothing_else(handles):
    from event_representation_study_amd import _lib
    raw, api = handles
    status = _status_functions_of_the_header()
    assert len(status) >= 40 and "evrep_bin_events" in status and "evrep_gwd_scratch_bytes" not in status
    assert {name for name in _lib.SYMBOLS if getattr(api, name).errcheck is not None} == status
    assert {name for name, entry in _lib.SYMBOLS.items() if isinstance(entry, _lib.Status)} == status
    for name, (res, args) in _lib.SYMBOLS.items():
        a, r = getattr(api, name), getattr(raw, name)
        assert a is not r and a.__name__ == name
        assert a.restype is r.restype is res and list(a.argtypes) == list(r.argtypes) == args, name
        assert getattr(r, "errcheck", None) is None, name
    assert _lib.api() is api and _lib.load() is raw


def test_same_call_on_both_handles(handles):
    from event_representation_study_amd._lib import EVREP_EINVAL, EvrepError, Plan
    raw, api = handles
    p = Plan()
    assert raw.evrep_plan_init(ctypes.byref(p), 1, 8, 8, 4, 4) == 0
    assert api.evrep_plan_init(ctypes.byref(p), 1, 8, 8, 4, 4) == 0
    assert raw.evrep_bin_events(ctypes.byref(p), None, None, None, None) == EVREP_EINVAL
    with pytest.raises(EvrepError) as e:
        api.evrep_bin_events(ctypes.byref(p), None, None, None, None)
    assert "evrep_bin_events" in str(e.value) and "EVREP_EINVAL" in str(e.value)
    assert str(e.value) == "evrep_bin_events failed: EVREP_EINVAL (bad argument)"
    assert raw.evrep_bin_events(ctypes.byref(p), None, None, None, None) == EVREP_EINVAL      # the raw handle still returns the code
    assert raw.evrep_bin_events is not api.evrep_bin_events


def test_size_functions_are_unchecked_and_agree(handles):
    raw, api = handles
    n = raw.evrep_gwd_scratch_bytes(12500, 14400)
    assert isinstance(n, int) and n > 14 * 14400 * 4 and api.evrep_gwd_scratch_bytes(12500, 14400) == n
    assert api.evrep_gwd_scratch_bytes.errcheck is None
    assert api.evrep_abi_version() == raw.evrep_abi_version()


def test_the_one_message():
    from event_representation_study_amd import _lib
    want = {_lib.EVREP_EINVAL: "evrep_x failed: EVREP_EINVAL (bad argument)",
            _lib.EVREP_EWORKSPACE: "evrep_x failed: EVREP_EWORKSPACE",
            _lib.EVREP_ENOTBINNED: "evrep_x failed: EVREP_ENOTBINNED",
            17: "evrep_x failed: rc=17"}
    for rc, text in want.items():
        assert _lib.failure(rc, "evrep_x") == text
        with pytest.raises(_lib.EvrepError) as e:
            _lib.check(rc, "evrep_x")
        assert str(e.value) == text
    with pytest.raises(_lib.EvrepError) as e:
        _lib.check(_lib.EVREP_EINVAL)
    assert str(e.value) == "libevrep call failed: EVREP_EINVAL (bad argument)"
    assert _lib.check(0) is None and _lib.check(0, "evrep_x") is None


def test_want_is_the_one_tensor_check():
    from event_representation_study_amd._lib import ptr, want
    cpu = torch.device("cpu")
    t = torch.zeros((6, 4), dtype=torch.int32)
    assert want(t, "rows", torch.int32) is t
    assert want(t, "rows", torch.int32, (6, 4), device=cpu) is t
    assert want(t, "rows", torch.int32, (None, 4)) is t
    assert want(t, "rows", torch.int32, numel=24, device=cpu) is t
    assert want(t, "rows", (torch.float32, torch.int32), (6, 4)) is t
    refused = {"not a tensor": lambda: want(t.numpy(), "rows", torch.int32),
               "dtype": lambda: want(t, "rows", torch.int64),
               "shape": lambda: want(t, "rows", torch.int32, (4, 6)),
               "rank": lambda: want(t, "rows", torch.int32, (24,)),
               "free dimension": lambda: want(t, "rows", torch.int32, (None, 3)),
               "element count": lambda: want(t, "rows", torch.int32, numel=23),
               "strided view": lambda: want(torch.zeros((12, 4), dtype=torch.int32)[::2], "rows", torch.int32, (6, 4)),
               "transposed view": lambda: want(torch.zeros((4, 6), dtype=torch.int32).t(), "rows", torch.int32, (6, 4)),
               "other device": lambda: want(torch.zeros((6, 4), dtype=torch.int32, device="meta"), "rows", torch.int32, (6, 4), device=cpu),
               "not on a GPU": lambda: want(t, "rows", torch.int32, device="cuda")}
    for case, call in refused.items():
        with pytest.raises(ValueError, match="^rows must be a contiguous torch.int(32|64) tensor"):
            call()
    with pytest.raises(ValueError) as e:
        want(t, "rows", torch.float64, (None, 2), device=cpu)
    assert str(e.value) == "rows must be a contiguous torch.float64 tensor of shape (*, 2) on cpu"
    assert ptr(None) is None
    z = torch.zeros(4)
    assert isinstance(ptr(z), ctypes.c_void_p) and ptr(z).value == z.data_ptr()


def test_engine_keeps_its_helper_names():
    from event_representation_study_amd import _lib, engine
    assert engine._ptr is _lib.ptr and engine._stream_ptr is _lib.stream_ptr and engine._require_gpu is _lib.require_gpu


def test_dependencies_are_derived_from_the_sources():
    from event_representation_study_amd import build
    deps = {src: [os.path.relpath(p, ROOT) for p in build.unit_deps(src)] for src in build.SOURCES}
    names = {src: {os.path.basename(p) for p in paths} for src, paths in deps.items()}
    assert len(build.SOURCES) == 15
    for src, paths in deps.items():
        assert paths[0] == os.path.join("event_representation_study_amd", "csrc", src) and len(set(paths)) == len(paths)
        assert os.path.join("include", "evrep.h") in paths, src
        assert "evrep_common.h" in names[src], src
    for src in ("evrep_capi_mdes.hip", "evrep_capi_builders.hip"):
        assert {"evrep_builders.hip", "evrep_bin.hip", "evrep_capi_builders.h", "evrep_est_table.h"} <= names[src], src
    for src in ("evrep_capi_decode.hip", "evrep_capi_study.hip", "evrep_capi_windows.hip"):
        assert "evrep_wave_search.h" in names[src], src
    on_disk = {f for f in os.listdir(build.CSRC) if f.endswith((".hip", ".h"))}
    assert on_disk == set().union(*names.values()) - {"evrep.h"}, "a file of csrc/ that no translation unit includes"
    assert not hasattr(build, "UNIT_DEPS")
