"""CPU-only: the host side of the detector input for frames of different sizes (DetectorFrontEnd.targets_frames /
prepare_frames) against the golden recorded from the reference's Gen1H5.__getitem__ with TORE's bounding-box frames
(tests/golden/make_golden_detector_input_frames.py; what sits behind cv2 is a stand-in there, parity unpinned), its refusals,
and the argument checks of evrep_resize_tap_tables / evrep_detector_input_frames without a launch."""
import ctypes
import os
import random
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import detector_input_ref as ref

GOLDEN = os.path.join(ROOT, "tests", "golden", "detector_input_frames.npz")


@pytest.fixture(scope="module")
def cases():
    return ref.load_golden(GOLDEN)


def _hyp(c):
    hyp = dict(ref.REF_HYP)
    if int(c["return_int"]) >= 0:
        hyp["letterbox_return_int"] = bool(c["return_int"])
    return hyp


def golden_batches(cases):
    """The cases that share (augment, hyp, S), in file order: one ragged batch each."""
    groups = {}
    for c in cases:
        groups.setdefault((bool(c["augment"]), int(c["return_int"]), int(c["img_size"])), []).append(c)
    return list(groups.values())


def golden_params(fe, group):
    """What B consecutive __getitem__ calls drew, each after its own random.seed."""
    params = []
    for c in group:
        random.seed(int(c["seed"]))
        params += fe.draw(1)
    return params


def test_golden_covers_what_it_should(cases):
    from event_representation_study_amd.detector_input import DetectorFrontEnd
    assert all(int(c["img_size"]) == 48 for c in cases) and os.path.getsize(GOLDEN) < 512 * 1024
    assert all(c["rep"].shape[2] == 12 and c["rep"].shape[:2] != tuple(c["sensor"]) for c in cases)      # bounding boxes
    train = [c for c in cases if c["augment"]]
    val = [c for c in cases if not c["augment"]]
    assert {tuple(c["flips"]) for c in train} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    longs = [max(c["rep"].shape[:2]) for c in train]
    assert 47 in longs and 48 in longs and max(longs) > 48 and min(longs) <= 8
    c47 = train[longs.index(47)]
    assert not DetectorFrontEnd(48, _hyp(c47), augment=True).geometry(*c47["rep"].shape[:2]).fused
    vlongs = [max(c["rep"].shape[:2]) for c in val]
    assert max(vlongs) > 48 and min(vlongs) < 48 and 48 in vlongs
    assert {int(c["return_int"]) for c in cases} == {-1, 0, 1}
    assert any(len(c["labels_out"]) for c in train) and any(len(c["labels_out"]) for c in val)
    for c in cases:                                                     # the frame is the events' bounding box
        x, y = c["events"][:, 0], c["events"][:, 1]
        assert c["rep"].shape[:2] == (y.max() - y.min() + 1, x.max() - x.min() + 1)


def test_targets_and_shapes_match_the_reference_in_mixed_batches(cases):
    from event_representation_study_amd import detector_input as di
    batches = golden_batches(cases)
    assert sum(len(g) for g in batches) == len(cases) and max(len(g) for g in batches) >= 2
    for group in batches:
        c0 = group[0]
        fe = di.DetectorFrontEnd(int(c0["img_size"]), _hyp(c0), augment=bool(c0["augment"]))
        params = golden_params(fe, group)
        for c, p in zip(group, params):
            assert np.array_equal(p.M, c["M"]) and p.s == float(c["s"]) and [int(p.flipud), int(p.fliplr)] == list(c["flips"])
        sizes = [c["rep"].shape[:2] for c in group]
        targets, shapes = fe.targets_frames(sizes, [c["boxes"] for c in group], params)
        t = targets.numpy()
        assert t.dtype == np.float32 and t.shape[1] == 6
        for b, c in enumerate(group):
            mine = t[t[:, 0] == b]
            assert mine.shape == c["labels_out"].shape and np.array_equal(mine[:, 1:], c["labels_out"][:, 1:]), int(c["seed"])
            (h0, w0), ((rh, rw), pad) = shapes[b]
            assert [h0, w0, rh, rw, pad[0], pad[1]] == list(c["shapes"]), int(c["seed"])
            if int(c["return_int"]) == 1:
                assert isinstance(pad[0], int) and isinstance(pad[1], int)
        assert (np.diff(t[:, 0]) >= 0).all()                            # collate_fn's order: sample by sample


def test_a_ragged_batch_consumes_random_as_draw_does():
    from event_representation_study_amd import detector_input as di
    sizes = [(31, 47), (5, 7), (70, 96), (48, 20)]
    fe = di.DetectorFrontEnd(48, ref.REF_HYP, augment=True)
    random.seed(77)
    want = fe.draw(4)
    state = random.getstate()
    random.seed(77)
    labels = [np.array([[0, 0.5, 0.5, 0.4, 0.4]], dtype=np.float32)] * 4
    got, _ = fe.targets_frames(sizes, labels)
    assert random.getstate() == state
    random.seed(77)
    same, _ = fe.targets_frames(sizes, labels, want)
    assert random.getstate() != state and torch.equal(got, same)       # given parameters draw nothing
    random.seed(5)
    state = random.getstate()
    di.DetectorFrontEnd(48, ref.REF_HYP, augment=False).targets_frames(sizes, labels)
    assert random.getstate() == state


def test_geometry_is_per_sample_and_uses_the_existing_one():
    from event_representation_study_amd import detector_input as di
    fe = di.DetectorFrontEnd(48, ref.REF_HYP, augment=True)
    sizes = [(31, 47), (47, 31), (48, 20), (70, 96), (1, 1), (5, 7), (47, 47)]
    geos = fe.frame_geometries(sizes)
    assert geos == [fe.geometry(h, w) for h, w in sizes]
    want = [ref.geometry_ref(h, w, 48, True) for h, w in sizes]
    assert [g.fused for g in geos] == [(r["rw"], r["rh"]) == (r["nw"], r["nh"]) for r in want]
    assert not geos[0].fused and not geos[1].fused and geos[2].fused and geos[3].fused      # both kinds in one batch
    assert di.area_taps_bound(96, 48) == 3 and di.area_taps_bound(70, 35) == 3 and di.area_taps_bound(48, 48) == 2


def test_refusals_before_anything_is_launched():
    from event_representation_study_amd import detector_input as di
    from event_representation_study_amd._lib import EvrepError
    fe = di.DetectorFrontEnd(48, ref.REF_HYP, augment=True)
    f32 = lambda h, w, c=12: torch.zeros((h, w, c), dtype=torch.float32)  # noqa: E731
    state = random.getstate()
    with pytest.raises(ValueError, match="sample 1 is an empty 0 x 0"):
        fe.prepare_frames([f32(5, 7), f32(0, 0)])
    with pytest.raises(ValueError, match="sample 2 .*resizes to 0 x 48"):
        fe.prepare_frames([f32(5, 7), f32(5, 7), f32(1, 100)])
    with pytest.raises(ValueError, match="sample 0 .*resizes to 48 x 0"):
        fe.targets_frames([(100, 1)])
    with pytest.raises(ValueError, match="one parameter set and one label array"):
        fe.prepare_frames([f32(5, 7), f32(6, 7)], labels=[np.zeros((0, 5), np.float32)])
    with pytest.raises(ValueError, match="one parameter set and one label array"):
        fe.prepare_frames([f32(5, 7), f32(6, 7)], params=fe.draw(3))
    with pytest.raises(ValueError):
        fe.targets_frames([(5, 7)], [np.zeros((0, 5), np.float32)] * 2, fe.draw(1))
    with pytest.raises(ValueError):
        fe.prepare_frames([])
    with pytest.raises(ValueError, match="sample 1 is not"):
        fe.prepare_frames([f32(5, 7), torch.zeros((1, 5, 7, 12))])
    state = random.getstate()
    with pytest.raises(TypeError, match="sample 1"):
        fe.prepare_frames([f32(5, 7), torch.zeros((5, 7, 12), dtype=torch.float64)])
    with pytest.raises(TypeError, match="sample 1"):
        fe.prepare_frames([f32(5, 7), f32(5, 7, 5)])
    with pytest.raises(TypeError, match="sample 0"):
        fe.prepare_frames([torch.zeros((5, 7, 12), dtype=torch.float16)])
    with pytest.raises(EvrepError, match="sample 0"):
        fe.prepare_frames([f32(5, 7), f32(9, 3)])
    assert random.getstate() == state                                   # a refused batch draws nothing
    with pytest.raises(NotImplementedError):                            # the 4-D entry keeps refusing lists
        fe.prepare([f32(5, 7)])


# ------------------------------------------------------------------------------------------------ the C ABI, no launch
@pytest.fixture(scope="module")
def lib():
    from event_representation_study_amd import build, _lib
    build.build()
    return _lib.load()


def test_symbols_struct_and_constants_match_the_header(lib):
    from event_representation_study_amd import _lib
    header = open(os.path.join(ROOT, "include", "evrep.h")).read()
    for name, nargs in (("evrep_resize_tap_tables", 9), ("evrep_detector_input_frames", 16), ("evrep_detector_input_frames_scratch_bytes", 1)):
        assert re.search(r"\b%s\s*\(" % name, header) and len(_lib.SYMBOLS[name][1]) == nargs and getattr(lib, name) is not None
    assert _lib.ABI_VERSION == 3 and lib.evrep_abi_version() == 3       # symbols were added, none changed
    for name in ("LINEAR", "AREA", "IDENTITY"):
        assert int(re.search(r"#define EVREP_TAPS_%s (\d+)" % name, header).group(1)) == getattr(_lib, "TAPS_" + name)
    body = re.search(r"typedef struct evrep_detin_frame \{(.*?)\} evrep_detin_frame;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [n for decl in body.split(";") for n in re.findall(r"\*?(\w+)\s*(?:,|$)", decl.strip())]
    assert declared == [n for n, _ in _lib.DetinFrame._fields_]
    assert ctypes.sizeof(_lib.DetinFrame) == 88 == lib.evrep_detector_input_frames_scratch_bytes(1)
    assert lib.evrep_detector_input_frames_scratch_bytes(0) == 0 == lib.evrep_detector_input_frames_scratch_bytes(65536)
    assert lib.evrep_detector_input_frames_scratch_bytes(65535) == 65535 * 88


def test_tap_table_arguments_are_checked_before_any_launch(lib):
    from event_representation_study_amd._lib import EVREP_EINVAL
    p = ctypes.c_void_p(256)
    good = dict(axes=p, n_axes=3, max_dst=48, start=p, count=p, wt=p, n_rows=100, n_wt=200, stream=None)
    bad = [dict(axes=None), dict(start=None), dict(count=None), dict(wt=None), dict(axes=ctypes.c_void_p(258)),
           dict(start=ctypes.c_void_p(258)), dict(wt=ctypes.c_void_p(260)), dict(n_axes=0), dict(max_dst=0), dict(max_dst=4097),
           dict(n_rows=0), dict(n_wt=0), dict(n_rows=1 << 31), dict(n_wt=1 << 31)]
    for kw in bad:
        a = dict(good, **kw)
        assert lib.evrep_resize_tap_tables(*[a[k] for k in good]) == EVREP_EINVAL, kw


def test_frames_arguments_are_checked_before_any_launch(lib):
    from event_representation_study_amd._lib import EVREP_EINVAL, F64, F32, DetinFrame, DETIN_WARP
    p = ctypes.c_void_p(256)
    # two frames at S = 48: 31 x 47 (stage 2: 31 x 47 -> 32 x 48) and 70 x 96 (35 x 48, no stage 2); tables of 400 rows, 900 weights
    f0 = dict(src=256, H=31, W=47, rh=31, rw=47, T1=2, row1=0, col1=31, wrow1=0, wcol1=62, nh=32, nw=48, T2=2, row2=78, col2=110,
              wrow2=156, wcol2=220, top=8, left=0, flags=0, reserved=0)
    f1 = dict(src=512, H=70, W=96, rh=35, rw=48, T1=3, row1=158, col1=193, wrow1=316, wcol1=421, nh=35, nw=48, T2=0, row2=0, col2=0,
              wrow2=0, wcol2=0, top=6, left=0, flags=DETIN_WARP, reserved=0)
    good = dict(B=2, dt=F64, C=12, S=48, start=p, count=p, wt=p, n_rows=400, n_wt=900, pad=p, warp=p, scale=1.0, frames_dev=p, out=p,
                stream=None)

    def call(frame=None, table=True, **kw):
        frames = (DetinFrame * 2)(DetinFrame(**f0), DetinFrame(**dict(f1, **(frame or {}))))
        a = dict(good, **kw)
        return lib.evrep_detector_input_frames(frames if table else None, *[a[k] for k in good])

    assert call(table=False) == EVREP_EINVAL
    bad = [dict(B=0), dict(B=65536), dict(dt=2), dict(C=0), dict(C=17), dict(S=0), dict(S=4097), dict(start=None), dict(count=None),
           dict(wt=None), dict(pad=None), dict(out=None), dict(frames_dev=None), dict(warp=None), dict(n_rows=0), dict(n_wt=0),
           dict(n_rows=1 << 31), dict(scale=float("nan")), dict(wt=ctypes.c_void_p(260)), dict(out=ctypes.c_void_p(258)),
           dict(frames_dev=ctypes.c_void_p(260)), dict(warp=ctypes.c_void_p(258)), dict(n_rows=240), dict(n_wt=564)]
    for kw in bad:
        assert call(**kw) == EVREP_EINVAL, kw
    bad_frames = [dict(src=None), dict(src=260), dict(H=0), dict(W=0), dict(H=0, W=0), dict(H=4097), dict(rh=0), dict(rw=4097),
                  dict(T1=0), dict(T1=4097), dict(T2=-1), dict(T2=4097), dict(nh=0), dict(nw=0), dict(nh=36), dict(nw=47),
                  dict(top=-1), dict(left=-1), dict(top=14), dict(left=1), dict(row1=-1), dict(row1=366), dict(col1=353),
                  dict(wrow1=-4), dict(wrow1=796), dict(wcol1=757), dict(T2=2, row2=366), dict(T2=2, col2=353),
                  dict(T2=2, wrow2=831), dict(T2=2, wcol2=805), dict(T2=2, wcol2=-1), dict(flags=8), dict(flags=0)]
    for kw in bad_frames:
        assert call(frame=kw) == EVREP_EINVAL, kw
    assert call(frame=dict(src=516), dt=F64) == EVREP_EINVAL            # aligned to 4, not to 8
    # flags and warp tables come together: no sample warps, yet a table is given
    assert call(frame=dict(flags=0)) == EVREP_EINVAL and call(warp=None) == EVREP_EINVAL
    assert F32 == 1
