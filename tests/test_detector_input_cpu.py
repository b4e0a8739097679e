"""CPU-only: the host side of the detector input (event_representation_study_amd/detector_input.py) against the golden
recorded from the reference's Gen1H5.__getitem__ (tests/golden/make_golden_detector_input.py: what the reference's own
statements decide is pinned -- stage order, label arithmetic, draws, shapes; what sits behind cv2 is a stand-in, parity
unpinned), the C ABI's argument checks without a launch, and the tests' own numpy restatement of stages R-F
(tests/detector_input_ref.py) against the golden images."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

from conftest import ROOT
import detector_input_ref as ref

GOLDEN = os.path.join(ROOT, "tests", "golden", "detector_input.npz")


@pytest.fixture(scope="module")
def cases():
    return ref.load_golden(GOLDEN)


def _hyp(c):
    hyp = dict(ref.REF_HYP)
    if int(c["return_int"]) >= 0:
        hyp["letterbox_return_int"] = bool(c["return_int"])
    return hyp


def test_golden_covers_what_it_should(cases):
    aug = [c for c in cases if c["augment"]]
    assert {tuple(c["flips"]) for c in aug} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert any(not c["augment"] for c in cases)
    assert {int(c["return_int"]) for c in cases} == {-1, 0, 1}
    assert all(int(c["img_size"]) <= 48 for c in cases) and os.path.getsize(GOLDEN) < 512 * 1024
    assert any(len(c["labels_out"]) for c in aug)


def test_draws_and_matrix_match_the_reference(cases):
    from event_representation_study_amd import detector_input as di
    for c in cases:
        S, hyp = int(c["img_size"]), _hyp(c)
        fe = di.DetectorFrontEnd(S, hyp, augment=bool(c["augment"]))
        random.seed(int(c["seed"]))
        (p,) = fe.draw(1)
        assert np.array_equal(p.M, c["M"]) and p.s == float(c["s"])
        assert [int(p.flipud), int(p.fliplr)] == list(c["flips"])
        if c["augment"]:
            random.seed(int(c["seed"]))
            M, s = di.get_transform_matrix((S, S), (S, S), hyp["degrees"], hyp["scale"], hyp["shear"], hyp["translate"])
            assert np.array_equal(M, c["M"]) and s == float(c["s"])


def test_draw_order_over_a_batch():
    """Sample by sample: six uniform draws, then the two flip draws -- what B consecutive __getitem__ calls consume."""
    from event_representation_study_amd import detector_input as di
    fe = di.DetectorFrontEnd(32, ref.REF_HYP, augment=True)
    random.seed(11)
    params = fe.draw(3)
    random.seed(11)
    for p in params:
        M, s = di.get_transform_matrix((32, 32), (32, 32), 0.373, 0.898, 0.602, 0.245)
        ud, lr = random.random() < 0.5, random.random() < 0.5
        assert np.array_equal(M, p.M) and s == p.s and (ud, lr) == (p.flipud, p.fliplr)
    random.seed(5)
    state = random.getstate()
    assert di.DetectorFrontEnd(32, ref.REF_HYP, augment=False).draw(4)[0].flipud is False and random.getstate() == state


def test_rotation_matrix_closed_form():
    from event_representation_study_amd.detector_input import rotation_matrix_2d
    R = rotation_matrix_2d(90.0, 2.0)
    assert np.allclose(R, [[0, 2, 0], [-2, 0, 0]], atol=1e-15)
    assert np.array_equal(rotation_matrix_2d(0.0, 1.0), [[1, 0, 0], [0, 1, 0]])


def test_targets_and_shapes_match_the_reference(cases):
    from event_representation_study_amd import detector_input as di
    for c in cases:
        S = int(c["img_size"])
        fe = di.DetectorFrontEnd(S, _hyp(c), augment=bool(c["augment"]))
        random.seed(int(c["seed"]))
        params = fe.draw(1)
        h0, w0 = c["rep"].shape[:2]
        g = fe.geometry(h0, w0)
        lb_pad = (g.left, g.top) if int(c["return_int"]) == 1 else (g.dw, g.dh)
        t = fe.targets([c["boxes"]], params, g, lb_pad).numpy()
        assert t.dtype == np.float32 and t.shape == c["labels_out"].shape
        assert np.array_equal(t[:, 1:], c["labels_out"][:, 1:]) and (t[:, 0] == 0).all()
        want = c["shapes"]
        assert [h0, w0, g.rh * g.ratio / h0, g.rw * g.ratio / w0, lb_pad[0], lb_pad[1]] == list(want)
        if int(c["return_int"]) == 1:
            assert isinstance(lb_pad[0], int)


def test_host_mirrors_step_by_step(cases):
    """random_affine and general_augment under the reference's names: same draws, same image, same labels as the recorded
    __getitem__ (the image stages before them come from the tests' restatement)."""
    from event_representation_study_amd import detector_input as di
    for c in [c for c in cases if c["augment"]]:
        S, hyp = int(c["img_size"]), _hyp(c)
        I = ref.letterbox_ref(c["rep"][None], S, True)[0]
        fe = di.DetectorFrontEnd(S, hyp, augment=True)
        g = fe.geometry(*c["rep"].shape[:2])
        pad = (g.left, g.top) if int(c["return_int"]) == 1 else (g.dw, g.dh)
        lab = c["boxes"].copy()
        w, h = g.rw * g.ratio, g.rh * g.ratio
        boxes = lab[:, 1:].copy()
        boxes[:, 0], boxes[:, 1] = w * (lab[:, 1] - lab[:, 3] / 2) + pad[0], h * (lab[:, 2] - lab[:, 4] / 2) + pad[1]
        boxes[:, 2], boxes[:, 3] = w * (lab[:, 1] + lab[:, 3] / 2) + pad[0], h * (lab[:, 2] + lab[:, 4] / 2) + pad[1]
        lab[:, 1:] = boxes
        random.seed(int(c["seed"]))
        img, lab = di.random_affine(I, lab, hyp["degrees"], hyp["translate"], hyp["scale"], hyp["shear"], (S, S))
        if len(lab):
            lab[:, [1, 3]] = lab[:, [1, 3]].clip(0, S - 1e-3)
            lab[:, [2, 4]] = lab[:, [2, 4]].clip(0, S - 1e-3)
            lab[:, 1:] = np.stack([(lab[:, 1] + lab[:, 3]) / 2 / S, (lab[:, 2] + lab[:, 4]) / 2 / S,
                                   (lab[:, 3] - lab[:, 1]) / S, (lab[:, 4] - lab[:, 2]) / S], 1)
        before = lab
        img, lab = di.general_augment(img, lab, hyp)
        assert lab is before                                          # flipped in place, like the reference
        assert np.array_equal(img.transpose(2, 0, 1)[::-1], c["image"])
        assert np.array_equal(lab, c["labels_out"][:, 1:])


def test_box_candidates_and_letterbox_names():
    from event_representation_study_amd import detector_input as di, gwd_pipeline
    assert di.letterbox is gwd_pipeline.letterbox
    b1 = np.array([[0, 0, 10, 10], [0, 0, 10, 10], [0, 0, 10, 10]], dtype=np.float64).T
    b2 = np.array([[0, 0, 10, 10], [0, 0, 1, 10], [0, 0, 3, 3]], dtype=np.float64).T
    assert di.box_candidates(b1, b2).tolist() == [True, False, False]


def test_restatement_reproduces_the_golden_images(cases):
    for c in cases:
        S = int(c["img_size"])
        Ms = [c["M"]] if c["augment"] else None
        got = ref.detector_input_ref(c["rep"][None], S, bool(c["augment"]), Ms, [c["flips"][0]], [c["flips"][1]])[0]
        assert got.dtype == np.float32 and np.array_equal(got, c["image"]), int(c["seed"])


def test_host_warp_equals_the_restatement():
    from event_representation_study_amd import detector_input as di
    rng = np.random.default_rng(3)
    for dt in (np.float64, np.float32):
        I = rng.uniform(0, 255, (17, 17, 5)).astype(dt)
        for M in (np.array([[0.9, 0.3, 1.5], [-0.2, 1.1, -2.25], [0, 0, 1]]), np.array([[1.0, 0, 3], [0, 1.0, -2], [0, 0, 1]]),
                  np.array([[1.0, 2.0, 0], [0.5, 1.0, 0], [0, 0, 1]])):
            assert np.array_equal(di.warp_affine(I, M[:2], (17, 17), 114.0), ref.warp_ref(I, M))


def test_warp_tables_refuse_what_leaves_int32():
    from event_representation_study_amd import detector_input as di
    ok = np.array([[1.0, 0, 1e6], [0, 1.0, 0], [0, 0, 1]])
    ad, bd, X0, Y0 = di.warp_tables(ok, 48)
    assert X0[0] == -1024000000 + 16 and ad[3] == 3072 and bd.max() == 0
    for bad in (np.array([[1.0, 0, 3e6], [0, 1.0, 0], [0, 0, 1]]), np.array([[1e-7, 0, 0], [0, 1.0, 0], [0, 0, 1]]),
                np.array([[1.0, 0, np.inf], [0, 1.0, 0], [0, 0, 1]]), np.array([[1.0, 0, 0], [0, 1e-300, 5], [0, 0, 1]])):
        with pytest.raises(ValueError):
            di.warp_tables(bad, 48)


def test_out_of_scope_raises():
    from event_representation_study_amd import detector_input as di
    with pytest.raises(NotImplementedError):
        di.DetectorFrontEnd(32, rect=True)
    with pytest.raises(NotImplementedError):
        di.DetectorFrontEnd(32).prepare([np.zeros((4, 4, 2))])


def test_reference_shapes_need_no_second_resize():
    from event_representation_study_amd.detector_input import DetectorFrontEnd
    for (h, w, S) in ((240, 304, 640), (720, 1280, 640), (480, 640, 640), (260, 346, 640), (180, 240, 640), (240, 304, 240)):
        for aug in (False, True):
            assert DetectorFrontEnd(S, ref.REF_HYP, augment=aug).geometry(h, w).fused
    assert not DetectorFrontEnd(48, ref.REF_HYP, augment=True).geometry(31, 47).fused


# ------------------------------------------------------------------------------------------------ the C ABI, no launch
@pytest.fixture(scope="module")
def lib():
    from event_representation_study_amd import build, _lib
    build.build()
    return _lib.load()


def test_symbol_is_declared_and_bound(lib):
    from event_representation_study_amd import _lib
    header = open(os.path.join(ROOT, "include", "evrep.h")).read()
    assert re.search(r"\bint evrep_detector_input\s*\(", header) and "evrep_detector_input" in _lib.SYMBOLS
    assert len(_lib.SYMBOLS["evrep_detector_input"][1]) == 24 and lib.evrep_detector_input is not None
    assert _lib.ABI_VERSION == 3 and lib.evrep_abi_version() == 3
    for name in ("WARP", "FLIPUD", "FLIPLR"):
        assert int(re.search(r"#define EVREP_DETIN_%s (\d+)u" % name, header).group(1)) == getattr(_lib, "DETIN_" + name)


def test_arguments_are_checked_before_any_launch(lib):
    from event_representation_study_amd._lib import EVREP_EINVAL, F64, F32
    p = ctypes.c_void_p(256)
    good = dict(rep=p, dt=F64, B=2, H=20, W=30, C=12, nh=21, nw=32, T=2, ys=p, yc=p, yw=p, xs=p, xc=p, xw=p, S=32, top=5, left=0,
                pad=p, flags=p, warp=p, scale=1.0, out=p, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return lib.evrep_detector_input(*[a[k] for k in good])

    bad = [dict(rep=None), dict(out=None), dict(pad=None), dict(ys=None), dict(yc=None), dict(yw=None), dict(xs=None), dict(xc=None),
           dict(xw=None), dict(dt=2), dict(B=0), dict(B=65536), dict(C=0), dict(C=17), dict(H=0), dict(W=4097), dict(S=0), dict(S=4097),
           dict(nh=0), dict(nw=0), dict(nw=33), dict(top=12), dict(top=-1), dict(left=1), dict(T=0), dict(scale=float("nan")),
           dict(flags=None), dict(warp=None), dict(rep=ctypes.c_void_p(260)), dict(rep=ctypes.c_void_p(258), dt=F32),
           dict(yw=ctypes.c_void_p(260)), dict(out=ctypes.c_void_p(258)), dict(warp=ctypes.c_void_p(258))]
    for kw in bad:
        assert call(**kw) == EVREP_EINVAL, kw
