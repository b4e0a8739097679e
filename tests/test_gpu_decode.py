"""GPU: raw event files decoded on the device (evrep_decode_dat, evrep_decode_bin5, evrep_dat_seek_time,
recording.DeviceRecording.from_dat / from_bin, recording.DatDeviceRecording).

Everything here is BIT-EQUAL or fails -- the domain is integers: columns, indices and timestamps against
tests/golden/evl_raw.npz (the reference's own readers), compacted columns against the numpy mask of the strict ones, and
builder outputs against the same kernels fed the golden's columns.  No test provokes a fault: the capacity overrun is
exercised with a capacity the kernel declines to pass, checked against a sentinel-filled tail.
"""
import numpy as np
import pytest
import torch

from test_decode_cpu import _G, _M, DAT, SEEK, write_dat

pytestmark = pytest.mark.gpu

BIN = [s["name"] for s in _M["bin"]]
CHUNKS = (16, 64, 1000)
ODD_CHUNKS = (17, 31, 33, 1001)             # n_out leaves the multiples of 16: the groups start anywhere in the payload
SENSOR_H, SENSOR_W = 240, 304
SENTINEL = {"x": 0xABCD, "y": 0xABCD, "t": -0x123456789, "p": 0x55}
DTYPES = {"x": np.uint16, "y": np.uint16, "t": np.int64, "p": np.int8}


def golden_columns(kind, name):
    return {f: _G["%s.%s.%s" % (kind, name, f)] for f in "xytp"}


def assert_columns(rec, want, what):
    assert len(rec) == len(want["t"]) == rec.n, what
    for f in "xytp":
        got = getattr(rec, f).cpu().numpy()
        assert got.dtype == DTYPES[f] == want[f].dtype and got.shape == want[f].shape, (what, f, got.dtype, got.shape)
        assert np.array_equal(got, want[f]), (what, f, int((got != want[f]).sum()), np.flatnonzero(got != want[f])[:4])


def oob_mask(cols, H, W):
    return (cols["x"] >= W) | (cols["y"] >= H)


def expected_state(cols, H, W, kept=None):
    """the fields of evrep_decode_state after a whole file, from its (strict) columns"""
    t, bad = cols["t"], oob_mask(cols, H, W)
    desc = np.flatnonzero(np.diff(t) < 0) + 1
    n = len(t)
    return dict(n_in=n, n_out=n if kept is None else kept, oob_count=int(bad.sum()), oob_first=int(np.flatnonzero(bad)[0]) if bad.any() else -1,
                desc_count=len(desc), desc_first=int(desc[0]) if len(desc) else -1, t_first=int(t[0]) if n else -1, t_last=int(t[-1]) if n else -1)


def dat_bytes(x, y, p01, t):
    word = x.astype(np.uint32) | (y.astype(np.uint32) << 14) | (p01.astype(np.uint32) << 28)
    return np.stack([t.astype(np.uint32), word], axis=1).astype("<u4").tobytes()


def decode(payload, fmt, H, W, flags, chunk=None, stride=8, capacity=None):
    """The C entry points on a payload held in memory, chunk by chunk on the current stream -> (columns as numpy, over the
    whole capacity + 64 sentinel entries, state dict).  One read-back at the end."""
    from event_representation_study_amd import _lib
    from event_representation_study_amd.engine import _ptr, _stream_ptr
    lib = _lib.load()
    rec_bytes = stride if fmt == "dat" else 5
    raw = np.frombuffer(bytes(payload), np.uint8)
    n = len(raw) // rec_bytes
    capacity = n if capacity is None else capacity
    chunk = max(n, 1) if chunk is None else chunk
    cols = {f: torch.from_numpy(np.full(capacity + 64, SENTINEL[f]).astype(DTYPES[f])).to("cuda:0") for f in "xytp"}
    state = torch.empty(8, dtype=torch.int64, device="cuda:0")
    scratch = torch.empty(lib.evrep_decode_scratch_bytes(chunk), dtype=torch.uint8, device="cuda:0")
    _lib.check(lib.evrep_decode_state_init(_ptr(state), _stream_ptr()))
    keep = []
    for first in range(0, n, chunk):
        m = min(chunk, n - first)
        piece = np.zeros((m * rec_bytes + 15) // 16 * 16, np.uint8)
        piece[:m * rec_bytes] = raw[first * rec_bytes:(first + m) * rec_bytes]
        d = torch.from_numpy(piece).to("cuda:0")
        keep.append(d)
        args = (first, H, W, flags, _ptr(cols["x"]), _ptr(cols["y"]), _ptr(cols["t"]), _ptr(cols["p"]), capacity, _ptr(state), _ptr(scratch),
                _stream_ptr())
        if fmt == "dat":
            _lib.check(lib.evrep_decode_dat(_ptr(d), m, stride, *args), "evrep_decode_dat")
        else:
            _lib.check(lib.evrep_decode_bin5(_ptr(d), m, *args), "evrep_decode_bin5")
    st = dict(zip(_lib.DECODE_STATE_FIELDS, (int(v) for v in state.cpu().numpy())))
    return {f: cols[f].cpu().numpy() for f in "xytp"}, st


def assert_decoded(got, want, n_out, what):
    """the first n_out entries equal `want`, everything behind them is still the sentinel"""
    for f in "xytp":
        assert np.array_equal(got[f][:n_out], want[f]), (what, f, np.flatnonzero(got[f][:n_out] != want[f])[:4])
        assert np.all(got[f][n_out:] == np.array(SENTINEL[f]).astype(DTYPES[f])), (what, f, "written behind n_out")


def group_heads(chunks, kept=None):
    """The `head` values (records in front of the first whole group, evrep_decode.hip: strict_body) of the calls that run the
    16-record group body at least once, when chunks of `chunks[k]` records are decoded one behind the other and `kept[k]` of
    them are written.  A chunk with drops takes the one-record path.  DAT groups are 16-byte aligned in the payload for an
    even head; BIN groups start 5 * head mod 16 bytes into their piece, and 5 is a unit modulo 16: sixteen heads, sixteen shifts."""
    heads, out0 = set(), 0
    for m, k in zip(chunks, chunks if kept is None else kept):
        head = min(-out0 % 16, m)
        if k == m and (m - head) // 16:
            heads.add(head)
        out0 += k
    return heads


def chunk_sizes(n, chunk):
    return [min(chunk, n - first) for first in range(0, n, chunk)]


def load_dat(tmp_path, name, **kw):
    from event_representation_study_amd.recording import DeviceRecording
    size = {} if int(_G["dat.%s.parse" % name][3]) >= 0 else dict(height=SENSOR_H, width=SENSOR_W)
    return DeviceRecording.from_dat(write_dat(tmp_path, name), **size, **kw)


def load_bin(tmp_path, name, H=256, W=256, **kw):
    from event_representation_study_amd.recording import DeviceRecording
    path = tmp_path / (name + ".bin")
    path.write_bytes(_G["bin.%s.payload" % name].tobytes())
    return DeviceRecording.from_bin(path, H, W, **kw)


# ------------------------------------------------------------------------------------------------ decode
@pytest.mark.parametrize("name", [n for n in DAT if n not in ("oob", "alloob")])
def test_dat_files_decode_to_the_references_columns(tmp_path, name):
    from event_representation_study_amd.recording import DatDeviceRecording
    want = golden_columns("dat", name)
    rec = load_dat(tmp_path, name)
    assert type(rec) is DatDeviceRecording and (rec.height, rec.width) == (SENSOR_H, SENSOR_W)
    assert_columns(rec, want, name)
    assert rec.decode_state == expected_state(want, SENSOR_H, SENSOR_W), rec.decode_state
    if len(want["t"]):
        lim = rec.get_time_limits()
        assert lim == (want["t"][0], want["t"][-1]) and all(isinstance(v, np.int64) for v in lim)
    else:
        with pytest.raises(IndexError):
            rec.get_time_limits()
    for chunk in CHUNKS + ODD_CHUNKS:
        again = load_dat(tmp_path, name, chunk_events=chunk)
        assert_columns(again, want, "%s chunk %d" % (name, chunk))
        assert again.decode_state == rec.decode_state and again._limits == rec._limits


@pytest.mark.parametrize("name", BIN)
def test_bin_files_decode_to_the_references_columns(tmp_path, name):
    from event_representation_study_amd.recording import DeviceRecording
    want = golden_columns("bin", name)
    rec = load_bin(tmp_path, name)
    assert type(rec) is DeviceRecording and (rec.height, rec.width) == (256, 256)
    assert_columns(rec, want, name)
    assert rec.decode_state == expected_state(want, 256, 256), rec.decode_state
    if len(want["t"]):
        assert rec.get_time_limits() == (want["t"][0], want["t"][-1])
    for chunk in CHUNKS + ODD_CHUNKS + (3, 7):             # (3 and 7 form no group: the one-record path and the upload's padding)
        again = load_bin(tmp_path, name, chunk_events=chunk)
        assert_columns(again, want, "%s chunk %d" % (name, chunk))
        assert again.decode_state == rec.decode_state


def test_trailing_partial_record_is_ignored(tmp_path):
    from event_representation_study_amd.recording import DeviceRecording
    path = tmp_path / "cut_td.dat"
    path.write_bytes(_G["dat.n65.header"].tobytes() + _G["dat.n65.payload"].tobytes()[:-3])
    rec = DeviceRecording.from_dat(path)
    assert_columns(rec, {f: v[:64] for f, v in golden_columns("dat", "n65").items()}, "cut")


def bin5_bytes(x, y, p01, t):
    return np.stack([x & 255, y & 255, (p01 << 7) | ((t >> 16) & 127), (t >> 8) & 255, t & 255], axis=1).astype(np.uint8).tobytes()


def descent_stream():
    """9000 records on the 304x240 sensor whose only descent lies at record 8000 -> x, y, p (0 / 1), t, the columns"""
    rng = np.random.default_rng(3)
    n = 9000
    t = np.sort(rng.integers(1, 10 ** 6, n))
    t[8000:] = np.sort(rng.integers(1, int(t[7999]), n - 8000))
    assert np.flatnonzero(np.diff(t) < 0).tolist() == [7999]
    x, y, p = rng.integers(0, SENSOR_W, n), rng.integers(0, SENSOR_H, n), rng.integers(0, 2, n)
    return x, y, p, t, dict(x=x.astype(np.uint16), y=y.astype(np.uint16), t=t.astype(np.int64), p=np.where(p, 1, -1).astype(np.int8))


@pytest.mark.parametrize("chunk", (None,) + CHUNKS)
def test_a_descent_on_a_chunk_joint_is_seen(chunk):
    """The only descent of the stream lies at record 8000, the first of a chunk for 16, 64 and 1000 records per chunk."""
    x, y, p, t, want = descent_stream()
    n = len(t)
    for flags in (0, 1):
        got, st = decode(dat_bytes(x, y, p, t), "dat", SENSOR_H, SENSOR_W, flags, chunk)
        assert st == expected_state(want, SENSOR_H, SENSOR_W) and st["desc_first"] == 8000 and st["desc_count"] == 1, (flags, st)
        assert_decoded(got, want, n, "descent, flags %d" % flags)
    got, st = decode(bin5_bytes(x, y, p, t), "bin", 256, 256, 0, chunk)
    assert (st["desc_first"], st["desc_count"], st["t_first"], st["t_last"]) == (8000, 1, int(t[0]), int(t[-1]))
    assert np.array_equal(got["t"][:n], t) and np.array_equal(got["p"][:n], want["p"])


def test_the_chunkings_run_the_group_body_at_every_alignment():
    """Host side: what the chunk sizes of this file make the kernels do.  16, 64 and 1000 records per chunk only ever start a
    group at head 0 or 8; 31 per chunk walks n_out through every residue modulo 16 with at least one whole group behind it."""
    for n in (1025, 4097, 9000):
        assert group_heads(chunk_sizes(n, 31)) == set(range(16)), n
        assert group_heads(chunk_sizes(n, 17)) == {0, 1} and group_heads(chunk_sizes(n, 1001)) >= {0, 7}
        assert set().union(*(group_heads(chunk_sizes(n, c)) for c in CHUNKS)) <= {0, 8}
    assert group_heads(chunk_sizes(1025, 3)) == group_heads(chunk_sizes(1025, 7)) == set()
    assert {h & 1 for h in group_heads(chunk_sizes(4097, 31))} == {0, 1}                  # DAT: aligned and 8-byte groups
    assert {5 * h % 16 for h in group_heads(chunk_sizes(1025, 31))} == set(range(16))     # BIN: every byte shift


@pytest.mark.parametrize("chunk", ODD_CHUNKS)
def test_groups_at_every_alignment_decode_and_check_alike(chunk):
    """The descent stream (9000 records, its descent at 8000 now INSIDE a group or in front of one) and the largest golden
    streams through the C entry points at chunk sizes that leave n_out odd: columns, sentinel tail and state."""
    x, y, p, t, want = descent_stream()
    n = len(t)
    for flags in (0, 1):
        got, st = decode(dat_bytes(x, y, p, t), "dat", SENSOR_H, SENSOR_W, flags, chunk)
        assert st == expected_state(want, SENSOR_H, SENSOR_W), (flags, st)
        assert_decoded(got, want, n, "descent, flags %d" % flags)
        wantb = dict(want, x=want["x"] & 255, y=want["y"] & 255)
        got, st = decode(bin5_bytes(x, y, p, t), "bin", 256, 256, flags, chunk)
        assert st == expected_state(wantb, 256, 256), (flags, st)
        assert_decoded(got, wantb, n, "descent bin, flags %d" % flags)
    for kind, name, H, W in (("dat", "n4097", SENSOR_H, SENSOR_W), ("dat", "bits29", SENSOR_H, SENSOR_W), ("bin", "n1025", 256, 256)):
        want = golden_columns(kind, name)
        got, st = decode(_G["%s.%s.payload" % (kind, name)], kind, H, W, 0, chunk)
        assert st == expected_state(want, H, W)
        assert_decoded(got, want, len(want["t"]), "%s chunk %d" % (name, chunk))


@pytest.mark.parametrize("fmt", ["dat", "bin"])
def test_a_clean_stretch_behind_dropped_records_starts_its_groups_anywhere(fmt):
    """DROP_OOB, 300 records in chunks of 100: d = 0 .. 15 records of the first chunk lie outside the frame, the other two
    chunks are clean and run the group body at n_out = 100 - d and 200 - d: every head, every BIN shift, both DAT alignments."""
    from event_representation_study_amd._lib import DECODE_DROP_OOB
    H, W = 200, 180
    heads = set()
    for d in range(16):
        rng = np.random.default_rng(40 + d)
        n = 300
        x, y, p = rng.integers(0, W, n), rng.integers(0, H, n), rng.integers(0, 2, n)
        t = np.sort(rng.integers(1, 10 ** 6, n))
        bad = rng.choice(100, d, replace=False)
        x[bad[::2]], y[bad[1::2]] = W + rng.integers(0, 256 - W, len(bad[::2])), H + rng.integers(0, 256 - H, len(bad[1::2]))
        want = dict(x=x.astype(np.uint16), y=y.astype(np.uint16), t=t.astype(np.int64), p=np.where(p, 1, -1).astype(np.int8))
        keep = ~oob_mask(want, H, W)
        assert int((~keep).sum()) == d and keep[100:].all()
        heads |= group_heads([100, 100, 100], [100 - d, 100, 100])
        got, st = decode(dat_bytes(x, y, p, t) if fmt == "dat" else bin5_bytes(x, y, p, t), fmt, H, W, DECODE_DROP_OOB, 100)
        assert st == expected_state(want, H, W, kept=n - d), (d, st)
        assert_decoded(got, {f: v[keep] for f, v in want.items()}, n - d, "%s, %d dropped" % (fmt, d))
    assert heads == set(range(16))


# ------------------------------------------------------------------------------------------------ out of bounds
@pytest.mark.parametrize("chunk", (None,) + CHUNKS)
def test_drop_equals_the_mask_of_the_strict_columns(chunk):
    from event_representation_study_amd._lib import DECODE_DROP_OOB, DECODE_STRICT
    want = golden_columns("dat", "oob")
    payload = _G["dat.oob.payload"]
    strict, st = decode(payload, "dat", SENSOR_H, SENSOR_W, DECODE_STRICT, chunk)
    assert st == expected_state(want, SENSOR_H, SENSOR_W) and st["oob_count"] >= 100
    assert_decoded(strict, want, len(want["t"]), "oob strict")
    keep = ~oob_mask(want, SENSOR_H, SENSOR_W)
    dropped, st = decode(payload, "dat", SENSOR_H, SENSOR_W, DECODE_DROP_OOB, chunk)
    assert st == expected_state(want, SENSOR_H, SENSOR_W, kept=int(keep.sum()))
    assert_decoded(dropped, {f: v[keep] for f, v in want.items()}, int(keep.sum()), "oob dropped")
    # 28-byte records: the one-record path, strict and dropped
    want40 = golden_columns("dat", "type40")
    keep40 = ~oob_mask(want40, 120, 150)
    got, st = decode(_G["dat.type40.payload"], "dat", 120, 150, DECODE_DROP_OOB, chunk, stride=28)
    assert st == expected_state(want40, 120, 150, kept=int(keep40.sum())) and 0 < keep40.sum() < len(keep40)
    assert_decoded(got, {f: v[keep40] for f, v in want40.items()}, int(keep40.sum()), "type40 dropped")
    # 5-byte records on a frame some of them miss
    wantb = golden_columns("bin", "n1025")
    keepb = ~oob_mask(wantb, 200, 180)
    got, st = decode(_G["bin.n1025.payload"], "bin", 200, 180, DECODE_DROP_OOB, chunk)
    assert st == expected_state(wantb, 200, 180, kept=int(keepb.sum())) and 0 < keepb.sum() < 1025
    assert_decoded(got, {f: v[keepb] for f, v in wantb.items()}, int(keepb.sum()), "bin dropped")


@pytest.mark.parametrize("name", ["n4097", "n17", "bits29", "tmax"])
def test_drop_of_a_clean_stream_equals_its_strict_columns(tmp_path, name):
    want = golden_columns("dat", name)
    for chunk in (1 << 24,) + CHUNKS:
        rec = load_dat(tmp_path, name, out_of_bounds="drop", chunk_events=chunk)
        assert_columns(rec, want, "%s drop chunk %d" % (name, chunk))
        assert rec.decode_state == expected_state(want, SENSOR_H, SENSOR_W)
    rec = load_bin(tmp_path, "n1025", out_of_bounds="drop")
    assert_columns(rec, golden_columns("bin", "n1025"), "bin drop")


def test_from_dat_raises_or_drops_out_of_bounds_records(tmp_path):
    want = golden_columns("dat", "oob")
    bad = oob_mask(want, SENSOR_H, SENSOR_W)
    first, count = int(np.flatnonzero(bad)[0]), int(bad.sum())
    with pytest.raises(ValueError, match=r"%d of 2000 records .* first at index %d$" % (count, first)):
        load_dat(tmp_path, "oob")
    for chunk in (1 << 24, 64):
        rec = load_dat(tmp_path, "oob", out_of_bounds="drop", chunk_events=chunk)
        kept = {f: v[~bad] for f, v in want.items()}
        assert_columns(rec, kept, "oob drop")
        assert rec.get_time_limits() == (kept["t"][0], kept["t"][-1]) and rec.decode_state["oob_count"] == count
    # every record out of bounds: an empty recording
    with pytest.raises(ValueError, match=r"40 of 40 records .* first at index 0$"):
        load_dat(tmp_path, "alloob")
    empty = load_dat(tmp_path, "alloob", out_of_bounds="drop")
    assert len(empty) == 0 and empty.x.numel() == 0 and empty.decode_state["n_in"] == 40 and empty.decode_state["n_out"] == 0
    with pytest.raises(IndexError):
        empty.get_time_limits()


@pytest.mark.parametrize("flags", (0, 1))
def test_a_capacity_overrun_is_declined_not_written(flags):
    """Chunks of 1000 into columns of 2500 entries: the third chunk would end at 3000.  It and every later chunk write
    nothing, the state says so, and the checks still cover the whole file."""
    from event_representation_study_amd._lib import DECODE_N_IN_OVERRUN
    want = golden_columns("dat", "n4097")
    got, st = decode(_G["dat.n4097.payload"], "dat", SENSOR_H, SENSOR_W, flags, chunk=1000, capacity=2500)
    assert st["n_in"] == 4097 | DECODE_N_IN_OVERRUN and st["n_out"] == 2000
    full = expected_state(want, SENSOR_H, SENSOR_W)
    assert {k: st[k] for k in full if k not in ("n_in", "n_out")} == {k: full[k] for k in full if k not in ("n_in", "n_out")}
    assert_decoded(got, {f: v[:2000] for f, v in want.items()}, 2000, "overrun")
    got, st = decode(_G["bin.n1025.payload"], "bin", 256, 256, flags, chunk=64, capacity=1024)
    assert st["n_in"] == 1025 | DECODE_N_IN_OVERRUN and st["n_out"] == 1024
    assert_decoded(got, {f: v[:1024] for f, v in golden_columns("bin", "n1025").items()}, 1024, "overrun bin")


# ------------------------------------------------------------------------------------------------ seek and cuts
def seek_file(tmp_path, name):
    t = _G["seek.%s.t" % name]
    i = np.arange(len(t), dtype=np.int64)
    cols = dict(x=(i % SENSOR_W).astype(np.uint16), y=((i // SENSOR_W) % SENSOR_H).astype(np.uint16), t=t, p=np.where(i & 1, 1, -1).astype(np.int8))
    path = tmp_path / (name + "_td.dat")
    path.write_bytes(_G["dat.n17.header"].tobytes() + dat_bytes(cols["x"], cols["y"], i & 1, t))
    return path, cols


@pytest.fixture(scope="module")
def seek_recordings(tmp_path_factory):
    from event_representation_study_amd.recording import DeviceRecording
    out = {}
    for name in SEEK:
        path, cols = seek_file(tmp_path_factory.mktemp("seek"), name)
        out[name] = (DeviceRecording.from_dat(path, chunk_events=100000), cols)
    return out


@pytest.mark.parametrize("name", SEEK)
def test_seek_time_equals_the_reference(seek_recordings, name):
    rec, cols = seek_recordings[name]
    assert_columns(rec, cols, name)
    q, want = _G["seek.%s.queries" % name], _G["seek.%s.index" % name]
    got = rec.seek_time_index(q)                                           # every query of the stream in ONE call
    assert got.dtype == np.int64 and np.array_equal(got, want), np.flatnonzero(got != want)
    if name == "big":
        assert int(np.sum(got != np.searchsorted(cols["t"], q, "left"))) >= 3          # the equal-probe branch ran
    for nq in (1, 3, 4, 5):                                                # partial workgroups
        for k in range(0, 20, nq):
            assert np.array_equal(rec.seek_time_index(q[k:k + nq]), want[k:k + nq]), (nq, k)
    one = rec.seek_time_index(int(q[13]))
    assert np.ndim(one) == 0 and isinstance(one, np.integer) and one == want[13]
    assert np.array_equal(rec.seek_time_index(q, term=len(cols["t"])), np.searchsorted(cols["t"], q, "left") * (q > 0))


@pytest.mark.parametrize("kind", ["time", "idx"])
@pytest.mark.parametrize("name", SEEK)
def test_cuts_equal_the_reference(seek_recordings, name, kind):
    rec, cols = seek_recordings[name]
    excs = next(s for s in _M["seek"] if s["name"] == name)[kind + "_exc"]
    call = rec.get_between_time if kind == "time" else rec.get_between_idx
    for (a, b), (row, length, first, last), exc in zip(_G["seek.%s.%s_pairs" % (name, kind)].tolist(),
                                                       _G["seek.%s.%s_rows" % (name, kind)].tolist(), excs):
        if exc is not None:
            with pytest.raises({"ValueError": ValueError, "IndexError": IndexError}[exc]):
                call(a, b)
            continue
        batch = call(a, b, rebase="none")
        rows = batch.events.cpu().numpy()
        assert batch.B == 1 and len(rows) == length, (a, b, len(rows), length)
        if length:
            want = np.stack([cols[f][row:row + length].astype(np.int32) for f in "xytp"], axis=1)
            assert np.array_equal(rows, want) and (rows[0, 2], rows[-1, 2]) == (first, last), (a, b)


def test_a_descending_recording_answers_index_cuts_only(tmp_path):
    from event_representation_study_amd.recording import DeviceRecording
    rng = np.random.default_rng(9)
    n = 3000
    t = np.concatenate([np.sort(rng.integers(10 ** 6, 2 * 10 ** 6, 2000)), np.sort(rng.integers(1, 10 ** 5, 1000))])      # a clock that wrapped
    x, y, p = rng.integers(0, SENSOR_W, n), rng.integers(0, SENSOR_H, n), rng.integers(0, 2, n)
    path = tmp_path / "wrapped_td.dat"
    path.write_bytes(_G["dat.n17.header"].tobytes() + dat_bytes(x, y, p, t))
    rec = DeviceRecording.from_dat(path)
    assert len(rec) == n and rec.decode_state["desc_first"] == 2000 and rec.decode_state["desc_count"] == 1
    want = np.stack([x, y, t, np.where(p, 1, -1)], axis=1).astype(np.int32)
    assert np.array_equal(rec.windows([1990], [2010], rebase="none").events.cpu().numpy(), want[1990:2010])
    assert np.array_equal(rec.get_between_idx(-5, 10, rebase="none").events.cpu().numpy(), want[:15])
    w = rec.windows_before([500, 2500], 100)
    assert np.array_equal(w.events.cpu().numpy()[:, [0, 1, 3]], np.concatenate([want[400:500], want[2400:2500]])[:, [0, 1, 3]])
    assert rec.get_time_limits() == (t[0], t[-1])
    for ask in (lambda: rec.get_between_time(10, 500), lambda: rec.seek_time_index(5), lambda: rec.find_index_from_timestamp(7),
                lambda: rec.compute_time_and_index_windows(100, 1000, "us", "us")):
        with pytest.raises(ValueError, match="record 2000"):
            ask()
    b = tmp_path / "wrapped.bin"
    b.write_bytes(np.stack([x & 255, y & 255, (p << 7) | ((t >> 16) & 127), (t >> 8) & 255, t & 255], axis=1).astype(np.uint8).tobytes())
    recb = DeviceRecording.from_bin(b, 256, 256)
    assert recb.decode_state["desc_first"] == 2000
    with pytest.raises(ValueError, match="record 2000"):
        recb.get_between_time(10, 500)


def test_windows_of_a_dat_file_build_what_the_columns_build(seek_recordings):
    from event_representation_study_amd.recording import DeviceRecording
    rec, cols = seek_recordings["big"]
    plain = DeviceRecording(cols["x"], cols["y"], cols["t"], cols["p"], SENSOR_H, SENSOR_W)
    idx = np.array([2000, 2001, 77777, 125001, 250001])
    a, b = rec.windows_before(idx, 2000), plain.windows_before(idx, 2000)
    assert np.array_equal(a.events.cpu().numpy(), b.events.cpu().numpy()) and np.array_equal(a.t_base, b.t_base)
    ra, rb = a.optimized().cpu().numpy(), b.optimized().cpu().numpy()
    assert ra.shape == (5, SENSOR_H, SENSOR_W, 12) and np.array_equal(ra.view(np.uint8), rb.view(np.uint8))
