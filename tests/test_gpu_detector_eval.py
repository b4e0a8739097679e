"""GPU: the detection scoring (csrc/evrep_deteval.hip through detector_eval.match_batch / process_batch / ConfusionMatrix /
DetectionEvaluator) against the host restatement match_host and against the golden recorded from the reference's own
metrics.py and evaler.py, bit for bit: correct, detn, tbox, n_labels, status and the matrix.  No tolerance anywhere -- the
device and match_host perform the same float32 statements.

Shapes: the kernel lists labels in rounds of 1024 target rows with a scan over sixteen waves of 64, keeps at most 1024 labels
and has a lane per detection: label counts sit on both sides of 64, 256 and 1024, target arrays cross a listing round,
detection counts are 0, 1, 300 and 1024, T is 1, 10 and 16."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import assert_bit_equal, load_golden
import detector_eval_cases as cases
from guarded import FILLS, Arena
from test_detector_eval_cpu import IOUV_KEYS, eval_batch, golden_names

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = np.float32


def _de():
    from event_representation_study_amd import detector_eval
    return detector_eval


def device(det, count, targets, img_shape=None, shapes=None, iouv=None, native=False, nc=0, conf=0.25, iou_thres=0.45,
           skip_empty=False, matrix=None):
    """One launch with every output asked for: (correct, detn, tbox, n_labels, status, matrix) as numpy."""
    de = _de()
    v = de._iouv_host(iouv)
    geom = None if native else de.geometry_rows(shapes, det.shape[0])
    m = None
    if nc:
        m = torch.zeros((nc + 1) * (nc + 1), dtype=torch.int64, device=DEV) if matrix is None else matrix
    out = de._launch(torch.from_numpy(det).to(DEV), torch.from_numpy(np.asarray(count, np.int32)).to(DEV), torch.from_numpy(targets).to(DEV),
                     geom, img_shape or (0, 0), v, native, m, nc, conf, iou_thres, skip_empty, True, True)
    torch.cuda.synchronize()
    correct, detn, tbox, n_labels, status = (t.cpu().numpy() for t in out)
    return correct, detn, tbox, n_labels, status.view(np.uint32), (m.cpu().numpy() if m is not None else None)


def check(det, count, targets, what="", **kw):
    """The device == match_host on all six; returns the host results."""
    de = _de()
    nc = kw.get("nc", 0)
    want_m = np.zeros((nc + 1) * (nc + 1), np.int64) if nc else None
    host_kw = {k: v for k, v in kw.items() if k != "nc"}
    want = de.match_host(det, count, targets, matrix=want_m, nc=nc, **host_kw)
    got = device(det, count, targets, **kw)
    for g, w, name in zip(got, want + (want_m,), ("correct", "detn", "tbox", "n_labels", "status", "matrix")):
        if w is not None:
            assert_bit_equal(g, w, "%s %s" % (what, name))
    return want + (want_m,)


# ------------------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("key", IOUV_KEYS)
@pytest.mark.parametrize("name", golden_names())
def test_device_equals_process_batch_and_the_confusion_matrix(name, key):
    g = load_golden("detector_eval")
    det, lab, nc = g[name + "/det"], g[name + "/labels"], int(g[name + "/nc"])
    d, count, targets = cases.native_batch([det], [lab])
    correct, detn, tbox, n_labels, status, matrix = device(d, count, targets, iouv=g[name + "/iouv_" + key], native=True, nc=nc)
    assert_bit_equal(correct[0], g[name + "/correct_" + key], name)
    assert np.array_equal(matrix.reshape(nc + 1, nc + 1), g[name + "/matrix"]), name
    assert_bit_equal(detn, d)
    assert_bit_equal(tbox, lab[:, 1:])
    assert status.tolist() == [0] and n_labels.tolist() == [len(lab)]


def test_device_equals_the_evaler_over_two_batches():
    g = load_golden("detector_eval")
    matrix = torch.zeros(16, dtype=torch.int64, device=DEV)
    for bi in (0, 1):
        det, count, targets, shapes = eval_batch(g, bi)
        correct, detn, tbox, n_labels, status, _ = device(det, count, targets, cases.IMG, shapes, nc=3, skip_empty=True, matrix=matrix)
        pre = "eval%d/" % bi
        assert_bit_equal(correct, g[pre + "correct"], "correct")
        assert_bit_equal(detn, g[pre + "detn"], "detn")
        held = ~np.isnan(g[pre + "tbox"][:, 0])
        assert_bit_equal(tbox[held], g[pre + "tbox"][held], "tbox")
        assert not status.any()
    assert np.array_equal(matrix.cpu().numpy().reshape(4, 4), g["eval/matrix"]), "two calls accumulate the evaler's matrix"


# ------------------------------------------------------------------------------------------------------------------ the shapes
@pytest.mark.parametrize("T", [1, 10, 16])
@pytest.mark.parametrize("native", [False, True], ids=["normalised", "native"])
def test_counts_0_1_300(native, T):
    det, count, targets, shapes = cases.batch(7, [4, 3, 30], [0, 1, 300], nc=3, max_det=300)
    iouv = np.linspace(0.3, 0.975, T).astype(F32) if T != 10 else None
    kw = dict(native=True) if native else dict(img_shape=cases.IMG, shapes=shapes)
    out = check(det, count, targets, "counts", iouv=iouv, nc=3, **kw)
    assert out[0].shape == (3, 300, T) and (native or out[0][2].any()) and out[5].sum() > 0


def test_label_counts_around_a_wavefront_interleaved():
    n_labs = [0, 1, 63, 64, 65, 257]
    det, count, targets, shapes = cases.batch(8, n_labs, [10, 5, 70, 64, 65, 100], nc=4, max_det=100)
    assert (np.diff(targets[:, 0]) != 0).sum() > 100, "the rows of the images are interleaved"
    out = check(det, count, targets, "labels", img_shape=cases.IMG, shapes=shapes, nc=4)
    assert out[3].tolist() == n_labs and out[0][2:, :, 0].any(axis=1).all()
    check(det, count, targets, "labels, guarded", img_shape=cases.IMG, shapes=shapes, nc=4, skip_empty=True)


def test_targets_cross_a_listing_round_and_rows_of_no_image():
    det, count, targets, shapes = cases.batch(9, [257, 600, 300], [40, 50, 60], nc=3, max_det=64)
    assert len(targets) == 1157
    targets[5, 0], targets[1030, 0], targets[1100, 0], targets[7, 0] = 3.0, -1.0, 0.5, np.nan      # rows of no image
    out = check(det, count, targets, "rounds", img_shape=cases.IMG, shapes=shapes, nc=3)
    assert not out[2][[5, 7, 1030, 1100]].any() and out[3].sum() == 1153


def test_1024_labels_and_1025_labels():
    de = _de()
    dd = cases.grid_detections(200, 1024)
    det, count, targets = cases.native_batch([dd, dd], [cases.grid_labels(1024), cases.grid_labels(1025)])
    targets = targets[np.random.default_rng(3).permutation(len(targets))]
    out = check(det, count, targets, "cap", native=True, nc=3)
    assert out[4].tolist() == [0, de.ST_LABEL_OVERFLOW] and out[3].tolist() == [1024, 1025]
    assert out[0][0, :, 0].sum() > 100 and not out[0][1].any()
    assert len(targets) == 2049


def test_max_det_1024_with_count_1024():
    dd = cases.grid_detections(1024, 300, seed=5)
    det, count, targets = cases.native_batch([dd], [cases.grid_labels(300)], max_det=1024)
    out = check(det, count, targets, "1024", native=True, nc=3)
    assert count.tolist() == [1024] and out[0][0, :, 0].sum() == 300, "every label is claimed once, by its first detection"


@pytest.mark.parametrize("nc", [31, 32])
def test_matrix_of_1024_cells_and_of_more(nc):
    """A matrix of up to 1024 cells (nc <= 31) is counted in LDS and flushed with one atomic per cell; a larger one takes a
    global atomic per update.  Two launches accumulate on either path."""
    det, count, targets, shapes = cases.batch(50 + nc, [20, 0, 33], [60, 9, 0], nc=nc, max_det=64)
    want_m = np.zeros((nc + 1) * (nc + 1), np.int64)
    matrix = torch.zeros((nc + 1) * (nc + 1), dtype=torch.int64, device=DEV)
    for _ in range(2):
        _de().match_host(det, count, targets, cases.IMG, shapes, matrix=want_m, nc=nc)
        device(det, count, targets, cases.IMG, shapes, nc=nc, matrix=matrix)
    assert np.array_equal(matrix.cpu().numpy(), want_m) and want_m.sum() > 100 and want_m.sum() % 2 == 0


def test_bad_class_and_bad_count_set_their_bits():
    de = _de()
    lab = np.array([[5, 0, 0, 10, 10], [0, 20, 20, 30, 30], [np.nan, 40, 40, 50, 50]], F32)
    dd = np.array([[0, 0, 10, 10, 0.9, 0], [20, 20, 30, 30, 0.9, -3], [100, 100, 110, 110, 0.9, 1e9]], F32)
    det, count, targets = cases.native_batch([dd, dd], [lab, lab[:0]])
    count[1] = 9
    out = check(det, count, targets, "bits", native=True, nc=2)
    assert out[4].tolist() == [de.ST_BAD_CLASS, de.ST_BAD_COUNT]
    count[1] = -2
    out = check(det, count, targets, "negative count", native=True, nc=2)
    assert out[4].tolist() == [de.ST_BAD_CLASS, de.ST_BAD_COUNT] and not out[1][1].any()


def test_edges_of_the_rules_on_the_device():
    """The tie rule, IoU exactly at the thresholds, conf exactly at the threshold, NaN and zero-area boxes, 2.0 against 2.5."""
    lab = np.array([[1, 10, 10, 50, 50], [1, 10, 10, 50, 50], [2, 0, 0, 2, 1], [2, np.nan, 0, 10, 10], [2, 240, 240, 240, 240],
                    [2.5, 160, 160, 170, 170]], F32)
    dd = np.array([[10, 10, 50, 48, 0.9, 1], [10, 10, 50, 49, 0.8, 1], [0, 0, 1, 1, 0.7, 2], [0, 0, 10, np.nan, 0.6, 2],
                   [240, 240, 240, 240, 0.5, 2], [160, 160, 170, 170, 0.4, 2], [160, 160, 170, 170, 0.25, 2.5]], F32)
    det, count, targets = cases.native_batch([dd], [lab])
    iouv = np.array([0.5, np.nextafter(F32(0.5), F32(1))], F32)
    out = check(det, count, targets, "edges", iouv=iouv, native=True, nc=3, iou_thres=0.5)
    assert out[0][0].tolist() == [[1, 1], [0, 0], [1, 0], [0, 0], [0, 0], [0, 0], [1, 1]]
    check(det, count, targets, "edges, default thresholds", native=True, nc=3)


def test_two_different_labels_of_equal_iou_give_the_lowest_index():
    det, lab = cases.label_tie()
    d, count, targets = cases.native_batch([det], [lab])
    out = check(d, count, targets, "tie", iouv=np.array([0.5, 0.75], F32), native=True, nc=2)
    assert out[0][0].tolist() == [[1, 0], [0, 1]]
    assert out[5].reshape(3, 3).tolist() == [[0, 0, 0], [0, 1, 1], [0, 1, 0]]
    gpu = _de().process_batch(torch.from_numpy(det).to(DEV), torch.from_numpy(lab).to(DEV), torch.tensor([0.5], device=DEV))
    assert gpu[:, 0].tolist() == [True, False]


def test_shapes_from_the_front_end():
    """Fractional pads and gains as DetectorFrontEnd.prepare returns them for a 30 x 37 source in a 64 square."""
    from event_representation_study_amd.detector_input import DetectorFrontEnd
    from event_representation_study_amd import detector_output
    rng = np.random.default_rng(17)
    front = DetectorFrontEnd(64)
    labels = [np.concatenate([rng.integers(0, 3, (n, 1)), rng.uniform(0.2, 0.8, (n, 2)), rng.uniform(0.1, 0.3, (n, 2))], 1).astype(F32)
              for n in (6, 9)]
    rep = torch.from_numpy(rng.random((2, 30, 37, 2))).to(DEV)
    _, targets, shapes = front.prepare(rep, labels)
    targets = targets.cpu()
    (h0, w0), ((gy, gx), (px, py)) = shapes[0]
    assert (h0, w0) == (30, 37) and py != int(py) and gy != int(gy)
    tg, rows = targets.numpy(), []
    for b in range(2):                                                 # detections: the labels' letterboxed boxes, jittered
        t = tg[tg[:, 0] == b]
        xyxy = np.stack([t[:, 2] - t[:, 4] / 2, t[:, 3] - t[:, 5] / 2, t[:, 2] + t[:, 4] / 2, t[:, 3] + t[:, 5] / 2], 1) * 64
        rows.append(np.concatenate([xyxy + rng.normal(0, 0.4, xyxy.shape), np.linspace(0.9, 0.3, len(t))[:, None], t[:, 1:2]], 1).astype(F32))
    det, count = cases.pad_rows(rows, 16)
    out = check(det, count, targets.numpy(), "front end", img_shape=(64, 64), shapes=shapes, nc=3)
    assert out[0][:, :, 0].any()
    scb = detector_output.scale_coords_batch(torch.from_numpy(det).to(DEV), torch.from_numpy(count).to(DEV), (64, 64), shapes)
    assert_bit_equal(scb.cpu().numpy(), out[1], "detn == scale_coords_batch on the device")


# ------------------------------------------------------------------------------------------------------------ the public routes
def test_process_batch_and_confusion_matrix_on_cuda_equal_the_cpu_route():
    de = _de()
    det, lab = cases.native(21, 60, 20, nc=4, dup=5)
    iouv = torch.linspace(0.5, 0.95, 10)
    cpu = de.process_batch(torch.from_numpy(det), torch.from_numpy(lab), iouv)
    gpu = de.process_batch(torch.from_numpy(det).to(DEV), torch.from_numpy(lab).to(DEV), iouv.to(DEV))
    assert gpu.is_cuda and gpu.dtype == torch.bool and torch.equal(gpu.cpu(), cpu) and cpu.any()
    none = de.process_batch(torch.zeros((0, 6), device=DEV), torch.from_numpy(lab).to(DEV), iouv.to(DEV))
    assert tuple(none.shape) == (0, 10)
    a, b = de.ConfusionMatrix(4), de.ConfusionMatrix(4)
    for _ in range(2):                                                 # two calls accumulate
        a.process_batch(torch.from_numpy(det), torch.from_numpy(lab))
        b.process_batch(torch.from_numpy(det).to(DEV), torch.from_numpy(lab).to(DEV))
    assert np.array_equal(a.counts(), b.counts()) and a.counts().sum() > 0 and a.counts().sum() % 2 == 0
    assert np.array_equal(a.matrix, b.matrix) and all(np.array_equal(x, y) for x, y in zip(a.tp_fp(), b.tp_fp()))


def test_match_batch_returns_what_it_says_and_refuses_the_rest():
    de = _de()
    det, count, targets, shapes = cases.batch(23, [5, 7], [12, 20], nc=3, max_det=20)
    d, c, t = torch.from_numpy(det).to(DEV), torch.from_numpy(count).to(DEV), torch.from_numpy(targets).to(DEV)
    correct, detn, n_labels, status = de.match_batch(d, c, t, cases.IMG, shapes)
    want = de.match_host(det, count, targets, cases.IMG, shapes)
    assert correct.dtype == torch.uint8 and tuple(correct.shape) == (2, 20, 10) and correct.is_cuda
    assert_bit_equal(correct.cpu().numpy(), want[0])
    assert_bit_equal(detn.cpu().numpy(), want[1])
    assert n_labels.tolist() == [5, 7] and status.tolist() == [0, 0]
    tb = de.match_batch(d, c, targets=torch.from_numpy(targets), img_shape=cases.IMG, shapes=shapes, return_tbox=True)[4]
    assert_bit_equal(tb.cpu().numpy(), want[2], "CPU targets are taken to the device")
    assert_bit_equal(d.cpu().numpy(), det, "the input is left as it was")
    with pytest.raises(ValueError, match=r"\.float\(\)"):
        de.match_batch(d.double(), c, t, cases.IMG, shapes)
    with pytest.raises(ValueError, match="CUDA"):
        de.match_batch(torch.from_numpy(det), c, t, cases.IMG, shapes)
    with pytest.raises(ValueError, match="shapes"):
        de.match_batch(d, c, t, cases.IMG, shapes[:1])
    with pytest.raises(ValueError, match="iouv"):
        de.match_batch(d, c, t, cases.IMG, shapes, iouv=np.linspace(0, 1, 17))


def test_capture_and_replay():
    de = _de()
    det, count, targets, shapes = cases.batch(25, [9, 0, 14], [30, 12, 40], nc=3, max_det=40)
    other = cases.batch(26, [9, 0, 14], [25, 40, 1], nc=3, max_det=40)
    assert other[2].shape == targets.shape
    d, c, t = torch.from_numpy(det).to(DEV), torch.from_numpy(count).to(DEV), torch.from_numpy(targets).to(DEV)
    cm = de.ConfusionMatrix(3)
    cm.device_matrix(DEV)
    geom = de.geometry_tensor(shapes, DEV)                             # made before the capture: the call then uploads nothing
    eager = de.match_batch(d, c, t, cases.IMG, shapes)
    assert all(torch.equal(x, y) for x, y in zip(eager, de.match_batch(d, c, t, cases.IMG, geom)))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = de.match_batch(d, c, t, cases.IMG, geom, confusion=cm)
    d.copy_(torch.from_numpy(other[0])); c.copy_(torch.from_numpy(other[1])); t.copy_(torch.from_numpy(other[2]))
    graph.replay()
    torch.cuda.synchronize()
    want_m = np.zeros(16, np.int64)
    want = de.match_host(other[0], other[1], other[2], cases.IMG, shapes, matrix=want_m, nc=3, skip_empty=True)
    assert_bit_equal(out[0].cpu().numpy(), want[0], "replay on new contents")
    assert_bit_equal(out[1].cpu().numpy(), want[1])
    assert np.array_equal(cm.counts().reshape(-1), want_m)
    d.copy_(torch.from_numpy(det)); c.copy_(torch.from_numpy(count)); t.copy_(torch.from_numpy(targets))
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(out, eager)), "the same bytes as the eager call"


def test_end_to_end_nms_to_map():
    """nms_batch -> DetectionEvaluator.update x 2 -> compute() equals the host route's numbers."""
    from event_representation_study_amd import detector_output
    import detector_output_cases as nms_cases
    de = _de()
    ev = de.DetectionEvaluator(3, confusion=True, check=True)
    stats, want_m, seen = [[], [], [], []], np.zeros(16, np.int64), 0
    for seed in (31, 32):
        pred = nms_cases.head_output(seed, 3, 300, 3)
        rows = detector_output.nms_host(pred, 0.25, 0.45, max_det=50)
        shapes = cases.shapes_for(3)
        rng = np.random.default_rng(seed)
        tg = []
        for b in range(3):                                             # labels: some of the image's own detections, as xywh / 640
            pick = rows[b][rng.permutation(len(rows[b]))[:6]]
            xywh = np.stack([(pick[:, 0] + pick[:, 2]) / 2, (pick[:, 1] + pick[:, 3]) / 2, pick[:, 2] - pick[:, 0] + 3, pick[:, 3] - pick[:, 1]], 1) / 640
            tg.append(np.concatenate([np.full((len(pick), 1), b), pick[:, 5:6], xywh], 1).astype(F32))
        targets = np.concatenate(tg, 0)
        det, count = detector_output.nms_batch(torch.from_numpy(pred).to(DEV), 0.25, 0.45, max_det=50)
        ev.update(det, count, torch.from_numpy(targets).to(DEV), cases.IMG, shapes)
        h_det, h_count = nms_cases.pad(rows, 50)
        correct = de.match_host(h_det, h_count, targets, cases.IMG, shapes, matrix=want_m, nc=3, skip_empty=True)[0]
        for b in range(3):
            stats[0].append(correct[b, :h_count[b]].astype(bool)); stats[1].append(h_det[b, :h_count[b], 4])
            stats[2].append(h_det[b, :h_count[b], 5]); stats[3].append(targets[targets[:, 0] == b, 1])
            seen += 1
    got = ev.compute()
    want = de.summarize([np.concatenate(s, 0) for s in stats], 3, seen)
    assert isinstance(got, dict) and want["map50"] > 0
    for k in ("p", "r", "ap", "f1", "ap_class", "nt"):
        assert np.array_equal(got[k], want[k]), k
    for k in ("mp", "mr", "map50", "map", "best_f1_index", "seen"):
        assert got[k] == want[k], k
    assert np.array_equal(ev.confusion.counts().reshape(-1), want_m)


def test_check_names_the_image():
    de = _de()
    dd = cases.grid_detections(5, 5)
    det, count, targets = cases.native_batch([dd, dd], [cases.grid_labels(5), cases.grid_labels(1025)])
    targets[:, 2:] = targets[:, 2:] / 640                              # (any boxes: the count is what matters)
    ev = de.DetectionEvaluator(3, check=True)
    ev.update(torch.from_numpy(det).to(DEV), torch.from_numpy(count).to(DEV), torch.from_numpy(targets).to(DEV), cases.IMG, cases.shapes_for(2))
    with pytest.raises(ValueError, match="batch 0, image 1: more than 1024 labels"):
        ev.compute()


# ------------------------------------------------------------------------------------------------------ the output contract
@pytest.mark.parametrize("native", [False, True], ids=["normalised", "native"])
def test_outputs_are_as_long_as_stated_and_wholly_written(native):
    """correct / detn / tbox / n_labels / status / matrix exactly as long as the header says, each between guard bands, the
    inputs registered read-only; interior fills zeros, 0xFF and random give the same bytes (every output byte is written,
    the zero tails included), no band and no input byte changes.  The matrix is an accumulator: it starts from zeros."""
    from event_representation_study_amd import _lib
    de = _de()
    lib = _lib.load()
    det, count, targets, shapes = cases.batch(41, [3, 0, 65], [0, 7, 19], nc=3, max_det=19)
    targets[4, 0] = 7.0                                                # a row of no image: its tbox row is zero-filled
    B, T, n_t = 3, 10, len(targets)
    want_m = np.zeros(16, np.int64)
    kw = dict(native=True) if native else dict(img_shape=cases.IMG, shapes=shapes)
    want = de.match_host(det, count, targets, matrix=want_m, nc=3, **kw)
    geom = de.geometry_rows(shapes, B)
    iouv = (ctypes.c_float * T)(*[float(v) for v in de.default_iouv()])
    P = ctypes.c_void_p
    for seed, fill in tuple((1, f) for f in FILLS) + ((2, "random"),):
        arena = Arena(DEV, seed)
        ptrs = {}
        for name, t in (("det", det), ("count", count), ("targets", targets), ("geom", geom)):
            arena.carve_like(torch.from_numpy(t), name=name)
            ptrs[name] = arena.ptr()
        outs = {}
        for name, shape, dtype in (("correct", (B, 19, T), torch.uint8), ("detn", (B, 19, 6), torch.float32), ("tbox", (n_t, 4), torch.float32),
                                   ("n_labels", (B,), torch.int32), ("status", (B,), torch.int32)):
            outs[name] = arena.carve_shape(shape, dtype, fill=fill, name=name)
            ptrs[name] = arena.ptr()
        matrix = arena.carve_shape((16,), torch.int64, fill="zeros", name="matrix")
        ptrs["matrix"] = arena.ptr()
        rc = lib.evrep_det_match(P(ptrs["det"]), P(ptrs["count"]), B, 19, P(ptrs["targets"]), n_t, None if native else P(ptrs["geom"]),
                                 640, 640, iouv, T, _lib.DETEVAL_NATIVE if native else 0, P(ptrs["matrix"]), 3, 0.25, 0.45,
                                 P(ptrs["correct"]), P(ptrs["detn"]), P(ptrs["tbox"]), P(ptrs["n_labels"]), P(ptrs["status"]),
                                 P(torch.cuda.current_stream().cuda_stream))
        _lib.check(rc, "evrep_det_match")
        torch.cuda.synchronize()
        arena.check()
        arena.check_inputs()
        what = "seed %d fill %s" % (seed, fill)
        for name, w in zip(("correct", "detn", "tbox", "n_labels"), want):
            assert_bit_equal(outs[name].cpu().numpy(), w, what + " " + name)
        assert_bit_equal(outs["status"].cpu().numpy().view(np.uint32), want[4], what)
        assert np.array_equal(matrix.cpu().numpy(), want_m), what
    # the optional outputs left out: the same correct, nothing else touched
    arena = Arena(DEV, 3)
    d_in = [arena.carve_like(torch.from_numpy(t)) for t in (det, count, targets, geom)]
    correct = arena.carve_shape((B, 19, T), torch.uint8, name="correct")
    n_labels = arena.carve_shape((B,), torch.int32, name="n_labels")
    status = arena.carve_shape((B,), torch.int32, name="status")
    rc = lib.evrep_det_match(P(d_in[0].data_ptr()), P(d_in[1].data_ptr()), B, 19, P(d_in[2].data_ptr()), n_t, P(d_in[3].data_ptr()), 640, 640,
                             iouv, T, _lib.DETEVAL_NATIVE if native else 0, None, 0, 0.25, 0.45, P(correct.data_ptr()), None, None,
                             P(n_labels.data_ptr()), P(status.data_ptr()), P(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, "evrep_det_match")
    torch.cuda.synchronize()
    arena.check()
    arena.check_inputs()
    assert_bit_equal(correct.cpu().numpy(), want[0], "no optional output")
