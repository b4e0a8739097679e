"""Record tests/golden/evl_raw.npz: what the REFERENCE's own readers return for Prophesee DAT files and 5-byte BIN files.

    python tests/golden/make_golden_evl_raw.py /path/to/event_representation_study

The reference's modules ev-licious/src/evlicious/io/utils/prophesee_utils.py, io/dat_event_handle.py, io/bin_event_handle.py,
io/h5_event_handle.py, io/utils/event_handle.py and io/utils/events.py are imported from the given checkout with `h5py`,
`hdf5plugin`, `tqdm`, the `H5Writer` and `Visualizer` modules and the `render` module of `Events` stubbed (none of them is on
the path of the recorded calls).  The generator writes its own DAT and BIN files to a temporary directory from seeded streams
and reads them back through the reference.  Recorded:

* decode, DAT: per stream the header bytes and the payload bytes of the file, `parse_header`'s four results, and the columns
  after `stream_events` + `_cd_events_to_standard_format` (read with `load_n_events(event_count())`);
* decode, BIN: per stream the file's bytes and the columns of `load_bin` + `Events.from_array(height=256, width=256)`;
* seek and cuts: two DAT streams stored as their t column only (x, y, p follow from the record index, see `index_columns`):
  `seek_time` queries with the reader's position afterwards, `get_between_time` pairs and `get_between_idx` pairs with the
  first row and the length of what came back, its first and last timestamp, or the type of the exception.

Only data is written; no program text of the reference.
"""
import importlib.util
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SENSOR_W, SENSOR_H = 304, 240
DAT_SIZES = (0, 1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 4097)
BIN_SIZES = (0, 1, 3, 4, 5, 63, 64, 65, 1025)
SEEK_STREAMS = (("big", 250001), ("small", 5000))
FULL_HEADER = b"%% Date 2024-03-01 10:00:00\n%% Version 2\n%% Height %d\n%% Width %d\n" % (SENSOR_H, SENSOR_W)
DATE_HEADER = b"% Date 2024-03-01 10:00:00\n"


def load_reference(ref_root):
    src = os.path.join(ref_root, "ev-licious", "src", "evlicious")

    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    def load(name, path, package):
        spec = importlib.util.spec_from_file_location(name, path)
        m = importlib.util.module_from_spec(spec)
        m.__package__ = package
        sys.modules[name] = m
        spec.loader.exec_module(m)
        return m

    stub("h5py")
    stub("hdf5plugin")
    stub("tqdm")
    for pkg in ("evlicious", "evlicious.io", "evlicious.io.utils"):
        stub(pkg).__path__ = []
    stub("evlicious.io.utils.render", _render=None, RenderingType=types.SimpleNamespace(RED_BLUE_OVERLAP=0))
    stub("evlicious.io.utils.h5_writer", H5Writer=None)
    stub("evlicious.io.utils.visualization", Visualizer=None)
    utils = sys.modules["evlicious.io.utils"]
    events = load("evlicious.io.utils.events", os.path.join(src, "io", "utils", "events.py"), "evlicious.io.utils")
    utils.event_handle = load("evlicious.io.utils.event_handle", os.path.join(src, "io", "utils", "event_handle.py"), "evlicious.io.utils")
    pu = load("evlicious.io.utils.prophesee_utils", os.path.join(src, "io", "utils", "prophesee_utils.py"), "evlicious.io.utils")
    load("evlicious.io.h5_event_handle", os.path.join(src, "io", "h5_event_handle.py"), "evlicious.io")
    dat = load("evlicious.io.dat_event_handle", os.path.join(src, "io", "dat_event_handle.py"), "evlicious.io")
    bin_ = load("evlicious.io.bin_event_handle", os.path.join(src, "io", "bin_event_handle.py"), "evlicious.io")
    return pu, dat, bin_, events.Events


def dat_payload(x, y, p01, t, high_bits=None, extra=None):
    """The records of a DAT file: uint32 t, uint32 x | y << 14 | p << 28 (| bits 29-31), then `extra` (n, k) bytes per record."""
    word = x.astype(np.uint32) | (y.astype(np.uint32) << 14) | (p01.astype(np.uint32) << 28)
    if high_bits is not None:
        word |= high_bits.astype(np.uint32) << 29
    rec = np.stack([t.astype(np.uint32), word], axis=1).astype("<u4").view(np.uint8).reshape(len(t), 8)
    if extra is not None:
        rec = np.concatenate([rec, extra], axis=1)
    return np.ascontiguousarray(rec).reshape(-1)


def index_columns(n):
    """x, y, p (0 / 1) of the seek streams: functions of the record index, so that the t column alone restores the file."""
    i = np.arange(n, dtype=np.int64)
    return (i % SENSOR_W).astype(np.uint16), ((i // SENSOR_W) % SENSOR_H).astype(np.uint16), (i & 1).astype(np.uint8)


def dat_streams():
    """name -> dict(header bytes incl. the type and size bytes, payload bytes, H, W or None)"""
    out = {}

    def stream(name, n, seed, ev_type=12, header=FULL_HEADER, t_hi=200000, high_bits=False, oob=None):
        rng = np.random.default_rng(seed)
        x = rng.integers(0, SENSOR_W, n)
        y = rng.integers(0, SENSOR_H, n)
        if oob == "some" and n:
            k = rng.choice(n, n // 10, replace=False)
            x[k[:len(k) // 2]] = rng.integers(SENSOR_W, 16384, len(k) // 2)
            y[k[len(k) // 2:]] = rng.integers(SENSOR_H, 16384, len(k) - len(k) // 2)
            x[7], y[7], x[n - 3], y[n - 3], x[n // 2], y[n // 2] = 16383, 5, 5, 16383, 16383, 16383
        if oob == "all":
            x = rng.integers(SENSOR_W, 16384, n)
        t = np.sort(rng.integers(1, t_hi, n, dtype=np.int64))
        if name == "tmax":
            t[-3:] = [0xFFFFFFFE, 0xFFFFFFFF, 0xFFFFFFFF]
        if name == "headerless" and n:
            t[0] = 7                                                 # the file must not begin with b"% "
        p = rng.integers(0, 2, n)
        hb = rng.integers(0, 8, n) if high_bits else None
        extra = rng.integers(0, 256, (n, 20), dtype=np.uint8) if ev_type == 40 else None
        size = 28 if ev_type == 40 else 8
        out[name] = dict(header=header + bytes([ev_type, size]) if header is not None else b"",
                         payload=dat_payload(x, y, p, t, hb, extra), ev_type=ev_type, ev_size=size,
                         size=(SENSOR_H, SENSOR_W) if header == FULL_HEADER else None, n=n)

    for k, n in enumerate(DAT_SIZES):
        stream("n%d" % n, n, 100 + k)
    stream("bits29", 1000, 201, high_bits=True)
    stream("tmax", 300, 202, t_hi=1 << 32)
    stream("type0", 777, 203, ev_type=0)
    stream("type40", 333, 204, ev_type=40)
    stream("headerless", 200, 205, ev_type=0, header=None)
    stream("date_only", 50, 206, header=DATE_HEADER)
    stream("oob", 2000, 207, oob="some")
    stream("alloob", 40, 208, oob="all")
    return out


def seek_t(n, seed):
    """n timestamps drawn with repetition from n / 5 distinct values in [1, 8 n / 5)"""
    rng = np.random.default_rng(seed)
    values = np.sort(rng.choice(np.arange(1, 8 * n // 5), n // 5, replace=False))
    return np.sort(rng.choice(values, n)).astype(np.int64)


def seek_queries(t, seed):
    rng = np.random.default_rng(seed)
    n, t0, t1 = len(t), int(t[0]), int(t[-1])
    probes = [n // 2, n // 4, (n // 2 + 1 + n) // 2, 3 * n // 4]             # the first- and second-level middles, and 3n/4
    q = [-1000, -1, 0, 1, t0 - 1, t0, t0 + 1, t1 - 1, t1, t1 + 1, t1 + 1000]
    for i in probes:
        q += [int(t[i]) - 1, int(t[i]), int(t[i]) + 1]
    on = rng.choice(t, 12)
    absent = np.setdiff1d(np.arange(t0, t1), t)
    q += on.tolist() + rng.choice(absent, 12).tolist() + rng.integers(t0 - 10, t1 + 10, 14).tolist()
    return np.array(q, np.int64)


def time_pairs(t, seed):
    rng = np.random.default_rng(seed)
    n, t1 = len(t), int(t[-1])
    m2, m4 = int(t[n // 2]), int(t[n // 4])
    pairs = [(-3, 50), (0, 100), (-100, -50), (-7, 0), (0, 0), (5, 5), (10, 9), (0, 1), (t1 + 1, t1 + 100), (t1 + 5, t1 + 5),
             (t1 + 9, t1 + 2), (t1, t1 + 1), (t1 - 50, t1 + 50), (m2, m2 + 100), (m4, m4 + 1), (m2 - 1, m2 + 1), (m2 + 1, m2 + 2),
             (m4, m4 + 40000), (1, t1 + 10), (int(t[0]), int(t[0]) + 1)]
    for _ in range(10):
        a = int(rng.integers(1, t1))
        pairs.append((a, a + int(rng.integers(1, 3000))))
    return np.array(pairs, np.int64)


def idx_pairs(n):
    return np.array([(0, 10), (-5, 10), (100, 100), (n - 5, n + 5), (n, n + 3), (n + 10, n + 20), (5, 3), (5, 4), (-10, -5),
                     (0, n), (n // 2 - 7, n // 2 + 1000), (n - 1, n), (-3, n + 3), (17, 18), (n + 4, n)], np.int64)


def main(ref_root):
    pu, dat_mod, bin_mod, Events = load_reference(ref_root)
    arrays, manifest = {}, {"dat": [], "bin": [], "seek": []}
    tmp = tempfile.mkdtemp()

    def write(name, *parts):
        path = os.path.join(tmp, name)
        with open(path, "wb") as f:
            for part in parts:
                f.write(bytes(part))
        return path

    # ---------------------------------------------------------------- decode, DAT
    for name, s in dat_streams().items():
        path = write(name + "_td.dat", s["header"], s["payload"].tobytes())
        with open(path, "rb") as f:
            bod, ev_type, ev_size, size = pu.parse_header(f)
        assert (int(ev_type), ev_size) == (s["ev_type"], s["ev_size"]) and bod == len(s["header"])
        assert list(size) == (list(s["size"]) if s["size"] else [None, None]), (name, size)
        reader = pu.EventDatReader(path)
        assert reader.event_count() == s["n"]
        ev = reader.load_n_events(reader.event_count())
        cols = pu._cd_events_to_standard_format(ev, 16384, 16384)         # (a frame every record fits: Events asserts the bounds)
        assert len(cols) == s["n"] and set(np.unique(cols.p)) <= {-1, 1}
        refuses = 0
        try:
            pu._cd_events_to_standard_format(ev, SENSOR_H, SENSOR_W)
        except AssertionError:
            refuses = 1
        assert refuses == (name in ("oob", "alloob")), name
        key = "dat.%s." % name
        arrays[key + "header"] = np.frombuffer(s["header"], np.uint8)
        arrays[key + "payload"] = s["payload"]
        arrays[key + "parse"] = np.array([bod, ev_type, ev_size] + [-1 if v is None else v for v in size], np.int64)
        for f in "xytp":
            arrays[key + f] = getattr(cols, f)
        manifest["dat"].append(dict(name=name, n=s["n"], ev_type=s["ev_type"], ev_size=s["ev_size"], events_refuses=refuses))
    assert int(arrays["dat.tmax.t"][-1]) == 0xFFFFFFFF and arrays["dat.tmax.t"].dtype == np.int64
    assert int(arrays["dat.oob.x"].max()) == 16383 and int(arrays["dat.oob.y"].max()) == 16383

    # ---------------------------------------------------------------- decode, BIN
    for k, n in enumerate(BIN_SIZES):
        raw = np.random.default_rng(300 + k).integers(0, 256, 5 * n, dtype=np.uint8)
        path = write("n%d.bin" % n, raw.tobytes())
        ev = Events.from_array(bin_mod.load_bin(path), height=256, width=256)
        assert len(ev) == n
        key = "bin.n%d." % n
        arrays[key + "payload"] = raw
        for f in "xytp":
            arrays[key + f] = getattr(ev, f)
        manifest["bin"].append(dict(name="n%d" % n, n=n))

    # ---------------------------------------------------------------- seek and cuts
    for k, (name, n) in enumerate(SEEK_STREAMS):
        t = seek_t(n, 400 + k)
        x, y, p = index_columns(n)
        path = write(name + "_td.dat", FULL_HEADER + bytes([12, 8]), dat_payload(x, y, p, t).tobytes())
        h = dat_mod.DatEventHandle.from_path(path)
        assert len(h) == n and (h.height, h.width) == (SENSOR_H, SENSOR_W)
        pm1 = np.where(p == 0, -1, 1).astype(np.int8)

        def first_row(ev):
            """the row the returned Events start at: x, y name the row modulo the frame, the columns decide"""
            if len(ev) == 0:
                return -1
            code = int(ev.x[0]) + SENSOR_W * int(ev.y[0])
            hits = [a for a in range(code, n, SENSOR_W * SENSOR_H)
                    if a + len(ev) <= n and np.array_equal(ev.t, t[a:a + len(ev)]) and np.array_equal(ev.x, x[a:a + len(ev)])
                    and np.array_equal(ev.y, y[a:a + len(ev)]) and np.array_equal(ev.p, pm1[a:a + len(ev)])]
            assert len(hits) == 1, hits
            return hits[0]

        def record(call, pairs):
            rows, excs = [], []
            for a, b in pairs.tolist():
                try:
                    ev = call(a, b)
                    rows.append([first_row(ev), len(ev), int(ev.t[0]) if len(ev) else -1, int(ev.t[-1]) if len(ev) else -1])
                    excs.append(None)
                except Exception as e:                               # the type is the recorded result
                    rows.append([-1, -1, -1, -1])
                    excs.append(type(e).__name__)
            return np.array(rows, np.int64), excs

        q = seek_queries(t, 500 + k)
        pos = []
        for v in q.tolist():
            h.reader.seek_time(v)
            pos.append(h.reader.current_event_index())
        key = "seek.%s." % name
        arrays[key + "t"] = t
        arrays[key + "queries"], arrays[key + "index"] = q, np.array(pos, np.int64)
        tp, ip = time_pairs(t, 600 + k), idx_pairs(n)
        arrays[key + "time_pairs"], arrays[key + "idx_pairs"] = tp, ip
        arrays[key + "time_rows"], time_exc = record(h.get_between_time, tp)
        arrays[key + "idx_rows"], idx_exc = record(h.get_between_idx, ip)
        quirks = int(np.sum(arrays[key + "index"] != np.searchsorted(t, q, "left")))
        manifest["seek"].append(dict(name=name, n=n, time_exc=time_exc, idx_exc=idx_exc, quirks=quirks))
        print(name, "quirks", quirks, "time_exc", time_exc, "idx_exc", idx_exc)
    big, small = manifest["seek"]
    assert big["quirks"] >= 3, big["quirks"]                 # the m == q branch of seek_time: position = middle + 1
    assert small["quirks"] == 0                              # at most term records: the bisection never runs

    arrays["manifest"] = np.array(json.dumps(manifest))
    path = os.path.join(HERE, "evl_raw.npz")
    np.savez_compressed(path, **arrays)
    with open(os.path.join(HERE, "README_evl_raw.md"), "w") as f:
        f.write(README % dict(size=os.path.getsize(path), quirks=big["quirks"]))
    assert os.path.getsize(path) < 1 << 20
    print("wrote", path, os.path.getsize(path))


README = """# evl_raw.npz

Written by `make_golden_evl_raw.py <reference checkout>` (%(size)d bytes): what the reference's readers return for DAT and
BIN files the generator wrote from seeded streams -- `parse_header`, `EventDatReader.load_n_events` +
`_cd_events_to_standard_format`, `load_bin` + `Events.from_array`, and `EventBaseReader.seek_time`,
`DatEventHandle.get_between_time` / `get_between_idx` (ev-licious/src/evlicious/io/utils/prophesee_utils.py,
io/dat_event_handle.py, io/bin_event_handle.py).  Data only.

Keys: `dat.<s>.{header,payload}` (the file is header + payload; the header ends with the type and size bytes),
`dat.<s>.parse` (payload offset, event type, event size, height, width; -1 for None), `dat.<s>.{x,y,t,p}`;
`bin.<s>.{payload,x,y,t,p}`; `seek.<s>.t` (x = i %% 304, y = (i // 304) %% 240, p = +1 for odd i),
`seek.<s>.{queries,index}`, `seek.<s>.{time_pairs,time_rows,idx_pairs,idx_rows}` (rows: first row, length, first t, last t;
-1 where empty or where the call raised); `manifest` (JSON: per stream n, event type and size, whether `Events` refuses the
stream on its 304 x 240 frame, the exception type per pair or null, the number of seek results that differ from
`np.searchsorted(t, q, "left")`).

Conditions the generator asserts (the tests assert them again):
- the `big` stream (250 001 records) holds %(quirks)d seek results that differ from `np.searchsorted(t, q, "left")`, at
  least three: the bisection's equal-probe branch; the `small` stream (5 000 records, below the termination criterion) none;
- `tmax` ends at t = 0xFFFFFFFF as a positive int64; `oob` holds x = 16383 and y = 16383.
"""


if __name__ == "__main__":
    main(sys.argv[1])
