"""CPU-only: the renderings of ev-licious' Events.render (event_representation_study_amd/evlicious_render.py) as far as they can
be held without a device -- the enum, the jet table, the numpy restatement the GPU tests compare with (tests/evl_render_ref.py)
against the images the reference itself drew (tests/golden/evl_render.npz, make_golden_evl_render.py), the two new entry points
in the header and the binding, and their argument checks.  No kernel is launched."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from conftest import ROOT, assert_bit_equal
import evl_render_ref as ref


@pytest.fixture(scope="module")
def golden():
    return ref.load_golden()


@pytest.fixture(scope="module")
def lib():
    from event_representation_study_amd import build, _lib
    build.build()
    return _lib.load()


_Z, _MANIFEST = ref.load_golden()
CASES = sorted(_MANIFEST["cases"])


def test_rendering_type_is_the_references(golden):
    from event_representation_study_amd.evlicious_render import RenderingType
    _, manifest = golden
    assert {m.name: int(m.value) for m in RenderingType} == manifest["reference_types"]
    assert [int(m) for m in RenderingType] == [1, 2, 3, 4, 5]


def test_jet_lut_is_matplotlibs(golden):
    from event_representation_study_amd.evlicious_render import jet_lut
    z, _ = golden
    assert_bit_equal(jet_lut(), z["jet_lut"], "jet_lut")


def test_the_package_does_not_import_matplotlib():
    import subprocess
    import sys
    code = "import sys; import event_representation_study_amd.evlicious_render; assert 'matplotlib' not in sys.modules"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


def test_golden_covers_what_it_should(golden):
    z, manifest = golden
    sizes = {tuple(int(v) for v in z[name + ".size"]) for name in CASES}
    assert sizes == {(1, 1), (1, 5), (5, 1), (3, 7), (9, 130), (240, 304)}
    counts = {name: len(z[name + ".x"]) for name in CASES}
    assert {counts["3x7_n%d" % n] for n in range(4)} == {0, 1, 2, 3}
    t = z["3x7_unsorted.t"]
    assert np.any(np.diff(t) < 0) and z["3x7_big_t.t"].min() > 1.5e15
    for name in CASES:
        assert len(manifest["cases"][name]) == 5 * 2 * 2


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(golden, name):
    """Bit-equal for the four uint8 types, cast and canvas both ways; exact LUT rows of the recorded float32 surface for
    TIME_SURFACE (shape and dtype of the <= 2-event quirk included)."""
    z, manifest = golden
    x, y, t, p, H, W = ref.golden_case(z, name)
    canvas = z[name + ".canvas"]
    for rtype in (1, 2, 3, 5):
        for cast in (True, False):
            for with_canvas in (False, True):
                want = ref.golden_image(z, manifest, name, rtype, cast, with_canvas)
                got = ref.render(x, y, t, p, H, W, rtype, cast=cast, canvas=canvas if with_canvas else None)
                assert_bit_equal(got, want, "%s type %d cast %d canvas %d" % (name, rtype, cast, with_canvas))
    want = ref.golden_image(z, manifest, name, 4, True, False)
    got = ref.render(x, y, t, p, H, W, 4, lut=z["jet_lut"], surface_image=z[name + ".surface"])
    assert_bit_equal(got, want, name + " TIME_SURFACE")


@pytest.mark.parametrize("name", CASES)
def test_restated_surfaces_stay_within_the_bound(golden, name):
    """The helper's own surface (float64 terms, one float32 rounding per event) against numpy's np.add.at image: within
    (k + 1) * 2^-23 * s per pixel, LUT index off by at most 1, at most 1 % of the touched pixels different."""
    z, _ = golden
    x, y, t, p, H, W = ref.golden_case(z, name)
    want = z[name + ".surface"]
    differ, touched = ref.check_surface(ref.surface(x, y, t, H, W), want, x, y, t, H, W, name)
    print(name, "differ", differ, "of", touched)


def test_symbols_are_declared_bound_and_checked(lib):
    from event_representation_study_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "evrep.h")).read(), flags=re.S)
    for name, arity in (("evrep_render_state", 9), ("evrep_render_compose", 13)):
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text)
        assert m and len(m.group(1).split(",")) == arity, name
        entry = _lib.SYMBOLS[name]
        assert isinstance(entry, _lib.Status) and len(entry[1]) == arity
        assert getattr(_lib.api(), name).errcheck is not None
    assert _lib.ABI_VERSION == 3 and lib.evrep_abi_version() == 3 and "#define EVREP_ABI_VERSION 3" in text
    defines = dict(re.findall(r"#define (EVREP_RENDER_[A-Z_]+) (\d+)u?", text))
    assert {k[len("EVREP_"):]: int(v) for k, v in defines.items()} == {
        "RENDER_RED_BLUE_OVERLAP": 1, "RENDER_RED_BLUE_NO_OVERLAP": 2, "RENDER_BLACK_WHITE_NO_OVERLAP": 3, "RENDER_TIME_SURFACE": 4,
        "RENDER_EVENT_FRAME": 5, "RENDER_JITTER": 1}
    for k, v in defines.items():
        assert getattr(_lib, k[len("EVREP_"):]) == int(v)


# The pointer arguments of the two entries, in call order, in the notation of tests/test_capi_cpu.py's _POINTER_TABLE: ("ptr", a) a
# required pointer aligned to a bytes, ("opt", a) an optional one, ("plan",) a real plan; everything else a valid scalar.
_COMMON = [("plan",), ("ptr", 16), ("ptr", 1), ("ptr", 256)]
_POINTER_TABLE = {
    "evrep_render_state": _COMMON + [("ptr", 4), ("opt", 4), ("opt", 4), 3e4, None],
    "evrep_render_compose colour": [("ptr", 4), ("opt", 4), ("opt", 4), ("opt", 8), ("opt", 1), 0, 1, 8, 8, 1, 1, ("ptr", 16), None],
    "evrep_render_compose EVENT_FRAME": [("ptr", 4), ("ptr", 4), ("opt", 4), ("opt", 8), ("opt", 1), 0, 1, 8, 8, 5, 0, ("ptr", 16), None],
    "evrep_render_compose TIME_SURFACE": [("ptr", 4), ("opt", 4), ("ptr", 4), ("ptr", 8), ("opt", 1), 0, 1, 8, 8, 4, 0, ("ptr", 16), None],
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


def _call(lib, name, index, fault, replace=None):
    from event_representation_study_amd._lib import Plan
    fn = getattr(lib, name.split()[0])
    keep, args = [], []
    for i, (a, ctype) in enumerate(zip(_POINTER_TABLE[name], fn.argtypes)):
        if replace and i in replace:
            a = replace[i]
        if not isinstance(a, tuple):
            args.append(a)
        elif i == index and fault == "null":
            args.append(None)
        elif a[0] == "plan":
            keep.append(Plan())
            assert lib.evrep_plan_init(ctypes.byref(keep[-1]), 1, 8, 8, 4, 4) == 0
            args.append(ctypes.cast(ctypes.c_void_p(ctypes.addressof(keep[-1])), ctype))
        elif a[0] == "opt" and i != index:
            args.append(None)
        else:
            args.append(ctypes.cast(ctypes.c_void_p(0x10000000 + 0x100000 * i + (a[1] // 2 if i == index else 0)), ctype))
    assert len(args) == len(fn.argtypes)
    return fn(*args)


@pytest.mark.parametrize("name,index,fault", _pointer_cases(), ids=lambda v: str(v))
def test_every_pointer_rule_refuses_before_any_launch(lib, name, index, fault):
    """One call per pointer argument and fault, as tests/test_capi_cpu.py holds the older entries: a required pointer NULL (net
    for EVENT_FRAME, surface and lut for TIME_SURFACE among them), a pointer with a stated alignment off by half of it.  Each is
    EVREP_EINVAL; the call with no fault gets past the checks (and fails in HIP: there is no device)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: made-up addresses must never be able to reach a launch")
    from event_representation_study_amd._lib import EVREP_EINVAL
    rc = _call(lib, name, index, fault)
    assert (rc != EVREP_EINVAL) if fault == "valid" else (rc == EVREP_EINVAL)


@pytest.mark.parametrize("what,replace", [
    ("jitter with EVENT_FRAME", {9: 5, 10: 1, 1: ("ptr", 4)}), ("jitter with TIME_SURFACE", {9: 4, 10: 1, 2: ("ptr", 4), 3: ("ptr", 8)}),
    ("unknown flag", {10: 2}), ("type 0", {9: 0}), ("type 6", {9: 6}), ("B 0", {6: 0}), ("B 65536", {6: 65536}), ("H 0", {7: 0}),
    ("H * W * 4 = 2^31", {7: 1 << 15, 8: 1 << 14}), ("canvas_is_batched 2", {4: ("ptr", 1), 5: 2}),
    ("out is the canvas", {4: ("fixed", 0x10000000 + 0x100000 * 11)}), ("canvas overlaps out", {4: ("fixed", 0x10000000 + 0x100000 * 11 + 100)}),
])
def test_compose_scalar_rules_refuse_before_any_launch(lib, what, replace):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: made-up addresses must never be able to reach a launch")
    from event_representation_study_amd._lib import EVREP_EINVAL
    fn = lib.evrep_render_compose
    args = []
    for i, (a, ctype) in enumerate(zip(_POINTER_TABLE["evrep_render_compose colour"], fn.argtypes)):
        a = replace.get(i, a)
        if not isinstance(a, tuple):
            args.append(a)
        elif a[0] == "opt":
            args.append(None)
        else:
            args.append(ctypes.cast(ctypes.c_void_p(a[1] if a[0] == "fixed" else 0x10000000 + 0x100000 * i), ctype))
    assert fn(*args) == EVREP_EINVAL, what


def test_state_refuses_tau_and_size_before_any_launch(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: made-up addresses must never be able to reach a launch")
    from event_representation_study_amd._lib import EVREP_EINVAL
    for tau in (0.0, -1.0, float("nan")):
        assert _call(lib, "evrep_render_state", -1, "valid", replace={6: ("ptr", 4), 7: tau}) == EVREP_EINVAL
    assert _call(lib, "evrep_render_state", -1, "valid", replace={7: 0.0}) != EVREP_EINVAL      # tau is only read with surface


def _events(n=5, H=4, W=6, divider=1):
    return types.SimpleNamespace(x=np.zeros(n, np.uint16), y=np.zeros(n, np.uint16), t=np.arange(n, dtype=np.int64),
                                 p=np.ones(n, np.int8), width=W, height=H, divider=divider)


def test_render_refuses_what_it_does_not_mirror():
    from event_representation_study_amd.evlicious_render import RenderingType, render
    with pytest.raises(NotImplementedError, match="_aggregate_float"):
        render(_events(divider=4))
    for bad in (np.zeros((4, 6), np.uint8), np.zeros((6, 4, 3), np.uint8), np.zeros((4, 6, 3), np.float32), np.zeros((1, 4, 6, 3), np.uint8),
                [[0]]):
        with pytest.raises(ValueError, match="rendering must be a uint8 canvas"):
            render(_events(), rendering=bad)
    outside = _events()
    outside.x[2] = 6      # x == width: the Events constructor refuses it
    with pytest.raises(ValueError, match="outside the 4 x 6"):
        render(outside)
    # the <= 2-event quirk needs no device: (H, W) uint8 zeros
    for n in (0, 1, 2):
        img = render(_events(n), rendering_type=RenderingType.TIME_SURFACE)
        assert img.shape == (4, 6) and img.dtype == np.uint8 and not img.any()


def test_video_frames():
    import torch
    from event_representation_study_amd.evlicious_render import video_frames
    rgba = torch.tensor([[[[0.0, 0.5, 1.0, 1.0], [0.999, 0.002, 2.0, 1.0]]]], dtype=torch.float64)
    want = np.clip(rgba.numpy()[..., :3] * 255, 0, 255).astype("uint8")
    assert np.array_equal(video_frames(rgba).numpy(), want)
    u8 = torch.zeros((1, 2, 2, 3), dtype=torch.uint8)
    assert video_frames(u8) is u8
