"""CPU-only: float16 and bfloat16 feature maps into the channel-wise distillation term (detector_distill.distill_cw with rules W1
and W3 of include/evrep.h).  Exact: the loss is cw_host's on the exactly widened maps, and a student map's gradient is the
float32 gradient array times grad_output, rounded once to the student's dtype -- (g32 * grad_output).to(dtype), torch's own
rounding.  The student's three maps share a dtype, the teacher's three share one, the two may differ.  Then the refusals of the
Python module and of the typed C entry, none of which reaches a launch."""
import ctypes

import numpy as np
import pytest
import torch

import detector_distill_cases as cases

F32, F64 = np.float32, np.float64
PAIRS = [(torch.float16, torch.float16), (torch.bfloat16, torch.bfloat16), (torch.float16, torch.float32), (torch.float32, torch.bfloat16)]
PAIR_IDS = ["f16-f16", "bf16-bf16", "f16-f32", "f32-bf16"]


def _dd():
    from event_representation_study_amd import detector_distill
    return detector_distill


@pytest.fixture(scope="module")
def lib():
    from event_representation_study_amd import build, _lib
    build.build()
    return _lib.load()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("name", sorted(cases.CW_CASES))
def test_distill_cw_on_cpu_tensors(name, pair):
    dd = _dd()
    c = cases.CW_CASES[name]()
    sdt, tdt = pair
    s16 = [torch.from_numpy(x).to(sdt) for x in c["s"]]
    t16 = [torch.from_numpy(x).to(tdt) for x in c["t"]]
    out, g32 = dd.cw_host([x.float().numpy() for x in s16[:3]], [x.float().numpy() for x in t16[:3]], c["tau"])
    for scale in (1.0, 65536.0):
        s = [x.clone().requires_grad_(True) for x in s16]
        loss = dd.distill_cw(s, t16, c["tau"])
        assert loss.dtype == torch.float64 and loss.dim() == 0 and loss.item() == out[0]
        loss.backward(torch.tensor(scale, dtype=torch.float64))
        for l in range(3):
            want = (torch.from_numpy(g32[l]) * torch.tensor(scale, dtype=torch.float32)).to(sdt)
            assert s[l].grad.dtype == sdt and torch.equal(_bits(s[l].grad), _bits(want)), (name, l, scale)
        assert all(x.grad is None for x in s[3:])
    with torch.no_grad():
        assert dd.distill_cw(s16, t16, c["tau"]).item() == out[0]


def test_autocast_changes_no_bit_on_cpu_tensors():
    dd = _dd()
    c = cases.CW_CASES["wave"]()
    got = []
    for inside in (False, True):
        s = [torch.from_numpy(x).to(torch.bfloat16).requires_grad_(True) for x in c["s"]]
        t = [torch.from_numpy(x).to(torch.bfloat16) for x in c["t"]]
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=inside):
            loss = dd.distill_cw(s, t, c["tau"])
        (loss * 65536.0).backward()
        got.append([loss.detach().reshape(1).view(torch.int64)] + [_bits(x.grad) for x in s])
    assert all(torch.equal(a, b) for a, b in zip(*got))


def test_python_refusals():
    dd = _dd()
    c = cases.CW_CASES["plain"]()
    s, t = [torch.from_numpy(x) for x in c["s"]], [torch.from_numpy(x) for x in c["t"]]
    for dtype in (torch.float16, torch.bfloat16):
        with pytest.raises(ValueError, match=r"s_feats\[1\].*share one dtype"):
            dd.distill_cw([s[0], s[1].to(dtype), s[2]], t)
        with pytest.raises(ValueError, match=r"t_feats\[2\].*share one dtype"):
            dd.distill_cw(s, [t[0], t[1], t[2].to(dtype)])
        with pytest.raises(ValueError, match=r"s_feats\[2\].*share one dtype"):
            dd.distill_cw([x.to(dtype) for x in s[:2]] + [s[2]], t)
        with pytest.raises(ValueError, match=r"t_feats\[1\] is torch.float64.*\.float\(\)"):
            dd.distill_cw([x.to(dtype) for x in s], [t[0], t[1].double(), t[2]])
    with pytest.raises(ValueError, match=r"s_feats\[0\] is torch.float64.*\.float\(\)"):
        dd.distill_cw([s[0].double(), s[1], s[2]], t)
    with pytest.raises(ValueError, match=r"s_feats\[1\]"):
        dd.distill_cw([s[0], s[1].to(torch.int32), s[2]], t)


def _levels(base_s=0x10000000, base_t=0x20000000, base_g=0x30000000, n=2, c=3, h=4, w=5, L=3):
    from event_representation_study_amd import _lib
    lv = (_lib.CwdLevel * max(L, 1))()
    for l in range(max(L, 1)):
        lv[l].s, lv[l].t, lv[l].grad_s = (base_s + 0x100000 * l) or None, (base_t + 0x100000 * l) or None, (base_g + 0x100000 * l) or None
        lv[l].n, lv[l].c, lv[l].h, lv[l].w = n, c, h, w
    return lv


def test_typed_c_entry_refuses_before_any_launch(lib):
    """Made-up addresses, as tests/test_detector_distill_cpu.py: skipped where a device could be reached."""
    if torch.cuda.is_available():
        pytest.skip("GPU present: made-up addresses must never be able to reach a launch")
    from event_representation_study_amd._lib import EVREP_EINVAL, DT_F32, DT_F16, DT_BF16
    vp = ctypes.c_void_p

    def call(lv, L=3, tau=1.0, flags=0, sdt=DT_F16, tdt=DT_F16, out=0x40000000, scratch=0x50000000):
        return lib.evrep_detloss_cwd_typed(ctypes.cast(lv, vp) if lv is not None else None, L, tau, flags, sdt, tdt, vp(out), vp(scratch), None)
    for sdt, tdt in ((DT_F32, DT_F32), (DT_F16, DT_F16), (DT_BF16, DT_BF16), (DT_F16, DT_F32), (DT_F32, DT_BF16)):
        assert call(_levels(), sdt=sdt, tdt=tdt) != EVREP_EINVAL         # past the checks (and fails in HIP: there is no device)
    assert call(_levels(base_s=0x10000002, base_t=0x20000002)) != EVREP_EINVAL      # 2-byte aligned 16-bit maps
    assert call(_levels(base_s=0x10000002), sdt=DT_F16, tdt=DT_F32) != EVREP_EINVAL
    refused = {
        "unknown student code": dict(sdt=3), "unknown teacher code": dict(tdt=-1), "odd student address": dict(lv=_levels(base_s=0x10000001)),
        "odd teacher address": dict(lv=_levels(base_t=0x20000001)),
        "student % 4 == 2 with F32": dict(lv=_levels(base_s=0x10000002), sdt=DT_F32), "teacher % 4 == 2 with F32": dict(lv=_levels(base_t=0x20000002), tdt=DT_F32),
        "gradient % 4 == 2": dict(lv=_levels(base_g=0x30000002)), "NULL student": dict(lv=_levels(base_s=0)), "NULL teacher": dict(lv=_levels(base_t=0)),
        "NULL gradient": dict(lv=_levels(base_g=0)), "NULL table": dict(lv=None), "L = 0": dict(L=0), "L = 4": dict(lv=_levels(L=4), L=4),
        "tau = 0": dict(tau=0.0), "tau NaN": dict(tau=float("nan")), "unknown flag": dict(flags=1), "NULL out": dict(out=0), "scratch % 256": dict(scratch=0x50000010),
        "h = 0": dict(lv=_levels(h=0)), "rows > 2^24": dict(lv=_levels(n=4096, c=4097)),
    }
    for what, kw in refused.items():
        kw = dict(kw)
        lv = kw.pop("lv", _levels())
        assert call(lv, **kw) == EVREP_EINVAL, what
    from event_representation_study_amd._lib import DETLOSS_NO_GRAD
    assert call(_levels(base_g=0), flags=DETLOSS_NO_GRAD) != EVREP_EINVAL          # no gradient asked for: grad_s may be NULL


def test_typed_entry_is_declared_and_bound_and_sized_as_the_float32_one(lib):
    import os
    import re
    from conftest import ROOT
    from event_representation_study_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "evrep.h")).read(), flags=re.S)
    for name, nargs in (("evrep_detloss_cwd_typed_workspace_bytes", 2), ("evrep_detloss_cwd_typed", 9)):
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, text)
        assert decl and len(decl.group(1).split(",")) == nargs == len(_lib.SYMBOLS[name][1]), name
    assert isinstance(_lib.SYMBOLS["evrep_detloss_cwd_typed"], _lib.Status)
    assert _lib.SYMBOLS["evrep_detloss_cwd_typed_workspace_bytes"][0] is ctypes.c_size_t
    P = ctypes.cast(_levels(n=2, c=3), ctypes.c_void_p)
    for L in (0, 1, 2, 3, 4):
        assert lib.evrep_detloss_cwd_typed_workspace_bytes(P, L) == lib.evrep_detloss_cwd_workspace_bytes(P, L)
    assert lib.evrep_detloss_cwd_typed_workspace_bytes(P, 3) == 256 and lib.evrep_detloss_cwd_typed_workspace_bytes(None, 3) == 0   # 18 rows
