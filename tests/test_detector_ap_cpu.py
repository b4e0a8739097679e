"""CPU: the declared rules A1-A7 of the average precision (detector_eval.ap_host, the CPU route and the oracle of
csrc/evrep_detap.hip) against the reference's own ap_per_class recorded in tests/golden/detector_ap.npz, against the package's
numpy ap_per_class, and through DetectionEvaluator.compute_device on CPU tensors.

Bounds.  On inputs whose confidences are pairwise distinct within every class the order is the reference's, and p, r, f1 and
the class list are the same float64 statements: BIT-EQUAL.  ap: A6 adds its 100 non-negative terms, whose sum is at most 1, in
ascending order, numpy's trapz adds the same terms pairwise; each order is within 99 * 2^-53 * sum of the exact sum, so the two
differ by at most 2 * 99 * 2^-53 = 2.2e-14."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, assert_bit_equal, load_golden
import detector_ap_cases as cases

AP_TOL = 2.2e-14
assert 2 * 99 * 2.0 ** -53 <= AP_TOL


def _de():
    from event_representation_study_amd import detector_eval
    return detector_eval


def against_reference(got, want, what):
    """got: ap_host's tuple; want: (p, r, ap, f1, classes) of an ap_per_class on the same, tie-free input."""
    p, r, ap, f1, n_labels = got[:5]
    wp, wr, wap, wf1, classes = want
    present = np.flatnonzero(n_labels > 0)
    assert np.array_equal(present, classes) and classes.dtype == np.int32, what
    assert_bit_equal(p[present], wp, what + " p")
    assert_bit_equal(r[present], wr, what + " r")
    assert_bit_equal(f1[present], wf1, what + " f1")
    err = np.abs(ap[present] - wap).max() if present.size else 0.0
    print("%s: ap differs by at most %.3g" % (what, err))
    assert err <= AP_TOL, (what, err)


def golden_inputs(g, name):
    return g[name + "/tp"], g[name + "/conf"], g[name + "/pred_cls"], g[name + "/target_cls"], int(g[name + "/nc"])


def golden_outputs(g, name):
    return tuple(g[name + "/" + k] for k in ("p", "r", "ap", "f1", "classes"))


def test_the_fixture_is_the_case_builder():
    g = load_golden("detector_ap")
    built = cases.golden_cases()
    assert list(g["names"]) == list(built) == list(cases.GOLDEN_NAMES)
    for name, case in built.items():
        assert cases.tie_free(case), name
        for got, want in zip(golden_inputs(g, name), case):
            assert_bit_equal(np.asarray(got), np.asarray(want), name)


@pytest.mark.parametrize("name", cases.GOLDEN_NAMES)
def test_ap_host_equals_the_reference(name):
    g = load_golden("detector_ap")
    got = _de().ap_host(*golden_inputs(g, name))
    assert got[7] == 0
    against_reference(got, golden_outputs(g, name), name)


@pytest.mark.parametrize("name", [n for n, c in cases.all_cases().items() if cases.tie_free(c) and c[1].size <= 3000])
def test_ap_host_equals_ap_per_class_without_ties(name):
    de = _de()
    tp, conf, pcls, tcls, nc = cases.all_cases()[name]
    if conf.size == 0:
        got = de.ap_host(tp, conf, pcls, tcls, nc)
        assert not got[0].any() and not got[2].any() and got[6] == 0 and got[5].sum() == 0
        return
    against_reference(de.ap_host(tp, conf, pcls, tcls, nc), de.ap_per_class(tp, conf, pcls, tcls), name)


@pytest.mark.parametrize("name", ["n20000_ties", "T16_nc80_ties", "all_equal", "signed_zeros"])
def test_ties_keep_array_order(name):
    """The declared rule: ap_host equals ap_per_class on the rows put in stable descending order and made tie-free by that
    order's rank (a strictly decreasing confidence per row, which any argsort orders alike)."""
    de = _de()
    tp, conf, pcls, tcls, nc = cases.all_cases()[name]
    assert not cases.tie_free((tp, conf, pcls, tcls, nc))
    got = de.ap_host(tp, conf, pcls, tcls, nc)
    order = np.argsort(-conf, kind="stable")
    want = de.ap_host(tp[order], conf[order], pcls[order], tcls, nc)            # pre-ordered rows: the same result
    for a, b in zip(got, want):
        assert_bit_equal(np.asarray(a), np.asarray(b), name)
    # ap (which does not read the confidences' values, only their order) against the numpy statements on ranked confidences
    rank = np.linspace(1.0, 0.0, conf.size).astype(np.float64)
    assert np.unique(rank).size == conf.size
    wp, wr, wap, wf1, classes = de.ap_per_class(tp[order], rank, pcls[order], tcls)
    present = np.flatnonzero(got[4] > 0)
    assert np.array_equal(present, classes)
    assert np.abs(got[2][present] - wap).max() <= AP_TOL


def test_interp_is_numpys_with_repeated_abscissae():
    de = _de()
    rng = np.random.default_rng(5)
    for trial in range(50):
        xp = np.sort(rng.integers(0, 12, int(rng.integers(1, 30))).astype(np.float64) / 8)
        fp = rng.random(xp.size)
        x = np.concatenate([rng.random(40) * 2 - 0.25, xp])
        assert_bit_equal(de._interp_host(x, xp, fp, -1.0, fp[-1]), np.interp(x, xp, fp, left=-1.0), "trial %d" % trial)


@pytest.mark.parametrize("name", list(cases.status_cases()))
def test_status_bits_and_ignored_rows(name):
    de = _de()
    (tp, conf, pcls, tcls, nc), bits = cases.status_cases()[name]
    got = de.ap_host(tp, conf, pcls, tcls, nc)
    assert got[7] == bits
    okp = (pcls >= 0) & (pcls < nc) & (pcls == np.floor(pcls))
    okt = (tcls >= 0) & (tcls < nc) & (tcls == np.floor(tcls))
    want = de.ap_host(tp[okp], conf[okp], pcls[okp], tcls[okt], nc)
    assert want[7] == 0
    for a, b in zip(got[:6], want[:6]):
        assert_bit_equal(a, b, name)


def test_nan_confidence_sets_its_bit():
    de = _de()
    got = de.ap_host(*cases.nan_conf_case())
    assert got[7] == de.AP_ST_NAN_CONF


def _evaluator(batches, nc=3, T=10, check=False):
    de = _de()
    ev = de.DetectionEvaluator(nc, iouv=np.linspace(0.5, 0.95, T).astype(np.float32), check=check)
    for b in batches:
        ev.add_batch(*(torch.from_numpy(t) for t in b))
    return ev


def against_compute(got, want, what=""):
    assert set(got) == set(want)
    for k in ("p", "r", "f1", "ap_class", "nt"):
        assert_bit_equal(got[k], want[k], what + k)
    for k in ("best_f1_index", "seen"):
        assert got[k] == want[k], k
    assert got["mp"] == want["mp"] and got["mr"] == want["mr"]
    assert np.abs(got["ap"] - want["ap"]).max() <= AP_TOL
    assert abs(got["map"] - want["map"]) <= AP_TOL and abs(got["map50"] - want["map50"]) <= AP_TOL


def test_compute_device_on_cpu_tensors_equals_compute():
    ev = _evaluator(cases.padded_batches(3))
    against_compute(ev.compute_device(), ev.compute())
    ev = _evaluator(cases.padded_batches(4, fill="false"))
    assert ev.compute_device() == (0.0, 0.0) == ev.compute()
    assert _evaluator([]).compute_device() == (0.0, 0.0)


def test_compute_device_on_cpu_tensors_at_the_gather_rounds():
    batches = cases.gather_edge_batches(6)
    kept = [int(((t[:, 0] >= 0) & (t[:, 0] < b[0].shape[0]) & (t[:, 0] == np.floor(t[:, 0]))).sum()) for b in batches for t in [b[3]]]
    assert all(k < b[3].shape[0] for k, b in zip(kept, batches)) and max(kept) > 1024
    ev = _evaluator(batches)
    got, want = ev.compute_device(), ev.compute()
    against_compute(got, want)
    assert int(got["nt"].sum()) == sum(kept)


def test_add_batch_says_what_a_kept_batch_is():
    de = _de()
    correct, conf_cls, count, targets, status = (torch.from_numpy(t) for t in cases.padded_batches(3)[0])
    ev = de.DetectionEvaluator(3, iouv=np.linspace(0.5, 0.95, 10).astype(np.float32))
    for bad in ((correct[:, :, :9], conf_cls, count, targets, status), (correct.int(), conf_cls, count, targets, status),
                (correct, conf_cls[:, :5], count, targets, status), (correct, conf_cls.double(), count, targets, status),
                (correct, conf_cls, count.long(), targets, status), (correct, conf_cls, count[:0], targets, status),
                (correct, conf_cls, count, targets[:, :1], status), (correct, conf_cls, count, targets, status.long()),
                (correct, conf_cls, count, targets, torch.zeros(9, dtype=torch.int32))):
        with pytest.raises(ValueError):
            ev.add_batch(*bad)
    assert not ev._batches
    ev.add_batch(correct, conf_cls, count, targets, status)
    assert len(ev._batches) == 1


def test_compute_device_check_raises_on_both_kinds_of_status():
    batches = cases.padded_batches(5)
    batches[1][4][0] = 4
    with pytest.raises(ValueError, match="batch 1, image 0"):
        _evaluator(batches, check=True).compute_device()
    batches = cases.padded_batches(5)
    batches[0][1][0, 0, 1] = 7.0                                      # a class outside [0, nc) in a counted row
    batches[0][2][0] = 3
    with pytest.raises(ValueError, match="AP status 1"):
        _evaluator(batches, check=True).compute_device()
    assert isinstance(_evaluator(batches).compute_device(), dict)


def test_summarize_is_unchanged_by_the_shared_tail():
    g = load_golden("detector_eval")
    stats = tuple(g["eval/stats_" + k] for k in ("tp", "conf", "pred_cls", "target_cls"))
    out = _de().summarize(stats, 3, int(g["eval/seen"]))
    assert_bit_equal(np.array([out["mp"], out["mr"], out["map50"], out["map"]]), g["eval/summary"])
    assert out["best_f1_index"] == int(g["eval/best_f1_index"]) and np.array_equal(out["nt"], g["eval/nt"])


def test_header_binding_and_constants_agree():
    from event_representation_study_amd import _lib
    text = open(os.path.join(ROOT, "include", "evrep.h")).read()
    for name in ("AP_SORT_TILE", "AP_SCAN_TILE", "AP_GATHER_CHUNK", "AP_GATHER_IMAGES", "AP_ST_BAD_CLASS", "AP_ST_NAN_CONF"):
        m = re.search(r"^#define\s+EVREP_%s\s+(\d+)u?\b" % name, text, flags=re.M)
        assert m and int(m.group(1)) == getattr(_lib, name), name
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("evrep_det_ap", "evrep_det_ap_gather", "evrep_det_ap_workspace_bytes"):
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, code)
        assert decl and len(decl.group(1).split(",")) == len(_lib.SYMBOLS[name][1]), name
    assert isinstance(_lib.SYMBOLS["evrep_det_ap"], _lib.Status) and _lib.SYMBOLS["evrep_det_ap_workspace_bytes"][0] is ctypes.c_size_t
    for rule in ("A1 order", "A2 classes", "A3 counts", "A4 curves", "A5 interp", "A6 ap", "A7 f1"):
        assert rule in text, rule


def test_argument_checks_refuse_before_any_launch():
    from event_representation_study_amd import build, _lib
    build.build()
    lib = _lib.load()
    size = lib.evrep_det_ap_workspace_bytes
    assert size(-1, 10, 3) == 0 and size(1 << 31, 10, 3) == 0 and size(10, 0, 3) == 0 and size(10, 17, 3) == 0
    assert size(10, 10, 0) == 0 and size(10, 10, _lib.NMS_MAX_CLASSES + 1) == 0
    assert size(0, 1, 1) > 0 and size(0, 1, 1) % 256 == 0
    # per row: two 8-byte keys, two 4-byte indices, the confidence, and per threshold a 4-byte count and an 8-byte maximum
    assert size(_lib.AP_SORT_TILE + 1, 10, 3) > size(_lib.AP_SORT_TILE, 10, 3) >= (28 + 12 * 10) * _lib.AP_SORT_TILE
    # The addresses of the arguments a call does not test.  Every call below must be refused before a launch; should a check
    # ever regress, nothing made up may reach a kernel: where a device is present they point into a real allocation, 64 kB
    # apart (more than any array of these shapes), and without one there is no launch to reach.
    P = ctypes.c_void_p
    step, base, keep = 0x100, 0x1000, None
    if torch.cuda.is_available():
        step = 64 * 1024
        keep = torch.zeros(17 * step + 256, dtype=torch.uint8, device="cuda:0")
        base = (keep.data_ptr() + 255) & ~255
    a = [P(base + step * i) for i in range(16)]
    off = lambda i, by: P(a[i].value + by)          # noqa: E731  (argument i, misaligned by `by` bytes)

    def call(n=8, m=4, T=10, nc=3, ws=None, ws_bytes=None, **ptrs):
        v = dict(tp=a[0], conf=a[1], pcls=a[2], tcls=a[3], counts=None, tables=a[4], p=a[5], r=a[6], f1=a[7], ap=a[8], nl=a[9],
                 np_=a[10], anyc=a[11], st=a[12])
        v.update(ptrs)
        return lib.evrep_det_ap(v["tp"], v["conf"], v["pcls"], v["tcls"], n, m, T, nc, v["counts"], v["tables"], v["p"], v["r"],
                                v["f1"], v["ap"], v["nl"], v["np_"], v["anyc"], v["st"], a[13] if ws is None else ws,
                                size(n, T, nc) if ws_bytes is None else ws_bytes, None)

    for kw in (dict(n=-1), dict(n=1 << 31), dict(m=-1), dict(T=0), dict(T=17), dict(nc=0), dict(nc=4097), dict(tp=None), dict(conf=None),
               dict(conf=off(1, 2)), dict(tcls=None), dict(tables=None), dict(tables=off(4, 4)), dict(p=None), dict(ap=off(8, 4)),
               dict(nl=None), dict(anyc=None), dict(st=off(12, 2)), dict(counts=off(14, 4)), dict(ws=off(13, 128))):
        assert call(**kw) == _lib.EVREP_EINVAL, kw
    assert call(ws_bytes=size(8, 10, 3) - 1) == _lib.EVREP_EWORKSPACE
    assert call(ws_bytes=0) == _lib.EVREP_EWORKSPACE
    g = [a[0], a[1], a[2], 2, 8, 10, a[3], 4, a[4], a[5], a[6], 16, a[7], 4, a[8], None]
    for i, bad in ((0, None), (1, off(1, 2)), (2, None), (3, 0), (4, 0), (4, 1025), (5, 17), (7, -1), (11, 15), (14, off(8, 4)), (14, None)):
        args = list(g)
        args[i] = bad
        assert lib.evrep_det_ap_gather(*args) == _lib.EVREP_EINVAL, (i, bad)
    del keep
