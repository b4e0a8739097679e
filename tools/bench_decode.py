#!/usr/bin/env python3
"""HIP-event times of decoding raw event files on the device (evrep_decode_dat, evrep_decode_bin5, evrep_dat_seek_time,
recording.DeviceRecording.from_dat), beside the route it replaces and a copy yardstick measured in the same run.

    python tools/bench_decode.py [--reps 50] [--scale 1.0] [--out FILE.json]

Inputs generated in memory: 5 * 10^6 records on a 304x240 sensor and 5 * 10^7 on a 1280x720 sensor (times --scale).  Per input,
median us over `reps` runs after warm-up:
  (a) numpy_route   numpy decode of the DAT payload (masks, shifts, casts: what the reference's reader does on the host) +
                    DeviceRecording(x, y, t, p): the 13 B / event upload.  Host clock, device drained.
  (b) from_dat      DeviceRecording.from_dat of the same file (8 B / event up, chunked, decoded on the device).  Host clock.
  (c) decode_dat    evrep_decode_dat alone on a resident payload (HIP events): STRICT; DROP_OOB with nothing to drop (the write
                    launch runs the strict body); DROP_OOB on the same payload with 1 % of the records moved out of the frame
                    (the write launch places one record per lane with narrow stores);
  (d) decode_bin5   evrep_decode_bin5 alone on a resident payload (HIP events);
  (e) d2d_copy      torch's device-to-device copy of the same algorithmic bytes: 8 + 13 per DAT record, 5 + 13 per BIN record;
  (f) seek          evrep_dat_seek_time for 64 and 4 096 queries beside evrep_time_to_index for the same counts.
GB/s is on the algorithmic bytes: the record read once, 13 B of columns written.  One JSON line.
"""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from event_representation_study_amd import _lib  # noqa: E402
from event_representation_study_amd.recording import DeviceRecording, dat_seek_index  # noqa: E402

INPUTS = {"304x240_5e6": (304, 240, 5_000_000), "1280x720_5e7": (1280, 720, 50_000_000)}
COLUMN_BYTES = 13
HEADER = b"%% Date 2024-03-01 10:00:00\n%% Version 2\n%% Height %d\n%% Width %d\n"


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def median_us(launch, reps, warmup=5):
    for _ in range(warmup):
        launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return float(np.median(times))


def median_host_us(run, reps, warmup=2):
    for _ in range(warmup):
        run()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(times))


def numpy_decode(payload):
    """The host route: the 8-byte records of a DAT payload to the columns a DeviceRecording holds (the inverse of the packing
    in main(): t, then x | y << 14 | p << 28), with numpy."""
    words = np.frombuffer(payload, dtype="<u4").reshape(-1, 2)
    w = words[:, 1]
    x = (w & 0x3FFF).astype(np.uint16)
    y = ((w >> 14) & 0x3FFF).astype(np.uint16)
    p = np.where((w >> 28) & 1, 1, -1).astype(np.int8)
    return x, y, words[:, 0].astype(np.int64), p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_decode.py needs a HIP device"
    assert args.reps >= 50 or args.scale < 1.0, "at least 50 repetitions at the full size"
    lib = _lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    result = dict(bench="decode", reps=args.reps, scale=args.scale, inputs={})
    tmp = tempfile.mkdtemp()
    for name, (W, H, n) in INPUTS.items():
        n = max(1024, int(n * args.scale))
        rng = np.random.default_rng(2)
        x, y = rng.integers(0, W, n, dtype=np.uint32), rng.integers(0, H, n, dtype=np.uint32)
        t = np.sort(rng.integers(1, 60_000_000, n, dtype=np.uint32))                  # a minute
        p = rng.integers(0, 2, n, dtype=np.uint32)
        payload = np.stack([t, x | (y << 14) | (p << 28)], axis=1).astype("<u4").tobytes()
        raw5 = np.stack([x & 255, y & 255, (p << 7) | ((t >> 16) & 127), (t >> 8) & 255, t & 255], axis=1).astype(np.uint8)
        path = os.path.join(tmp, name + "_td.dat")
        with open(path, "wb") as f:
            f.write(HEADER % (H, W) + bytes([12, 8]) + payload)
        want = numpy_decode(payload)
        row = dict(records=n)
        host_reps = max(5, args.reps // 10)
        row["numpy_route_us"] = round(median_host_us(lambda: DeviceRecording(*numpy_decode(payload), H, W), host_reps), 1)
        row["from_dat_us"] = round(median_host_us(lambda: DeviceRecording.from_dat(path), host_reps), 1)
        rec = DeviceRecording.from_dat(path)
        assert all(np.array_equal(getattr(rec, f).cpu().numpy(), w) for f, w in zip("xytp", want)), "from_dat and numpy disagree"

        cols = [torch.empty(n, dtype=d, device="cuda") for d in (torch.uint16, torch.uint16, torch.int64, torch.int8)]
        state = torch.empty(8, dtype=torch.int64, device="cuda")
        scratch = torch.empty(lib.evrep_decode_scratch_bytes(n), dtype=torch.uint8, device="cuda")
        d_dat = torch.from_numpy(np.frombuffer(payload, np.uint8).copy()).cuda()
        d_bin = torch.from_numpy(np.concatenate([raw5.reshape(-1), np.zeros(16, np.uint8)])).cuda()

        def decode(fmt, flags):
            assert lib.evrep_decode_state_init(ptr(state), stream) == 0
            args_ = (0, H, W, flags, ptr(cols[0]), ptr(cols[1]), ptr(cols[2]), ptr(cols[3]), n, ptr(state), ptr(scratch), stream)
            rc = lib.evrep_decode_dat(ptr(d_dat), n, 8, *args_) if fmt == "dat" else lib.evrep_decode_bin5(ptr(d_bin), n, *args_)
            assert rc == 0

        for key, fmt, flags, rec_bytes in (("decode_dat_strict", "dat", _lib.DECODE_STRICT, 8), ("decode_dat_drop", "dat", _lib.DECODE_DROP_OOB, 8),
                                           ("decode_bin5_strict", "bin", _lib.DECODE_STRICT, 5)):
            us = median_us(lambda: decode(fmt, flags), args.reps)
            if fmt == "dat":
                assert all(np.array_equal(c.cpu().numpy(), w) for c, w in zip(cols, want)), key
            else:
                assert np.array_equal(cols[2].cpu().numpy(), want[2] & 0x7FFFFF) and np.array_equal(cols[3].cpu().numpy(), want[3]), key
            nbytes = n * (rec_bytes + COLUMN_BYTES)
            # a copy of N bytes reads N and writes N: the decode's bytes are matched by a copy of half as many
            src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
            dst = torch.empty_like(src)
            us_c = median_us(lambda: dst.copy_(src), args.reps)
            row[key] = dict(us=round(us, 2), GBps=round(nbytes / us / 1e3, 1), d2d_copy_us=round(us_c, 2),
                            d2d_copy_GBps=round(nbytes / us_c / 1e3, 1), over_copy=round(us / us_c, 2))
            del src, dst
        # DROP_OOB with something to drop: 1 % of the records out of the frame, evenly spread
        bad = rng.random(n) < 0.01
        x_oob = np.where(bad, W + (x % (16384 - W)), x).astype(np.uint32)
        payload_oob = np.stack([t, x_oob | (y << 14) | (p << 28)], axis=1).astype("<u4").tobytes()
        d_dat = torch.from_numpy(np.frombuffer(payload_oob, np.uint8).copy()).cuda()
        us = median_us(lambda: decode("dat", _lib.DECODE_DROP_OOB), args.reps)
        kept = int(n - bad.sum())
        assert int(state.cpu()[1]) == kept
        assert all(np.array_equal(c[:kept].cpu().numpy(), w[~bad]) for c, w in zip(cols, numpy_decode(payload_oob))), "drop 1 %"
        nbytes = 2 * n * 8 + kept * COLUMN_BYTES                    # the payload read twice, the kept columns written
        row["decode_dat_drop_1pct"] = dict(us=round(us, 2), dropped=int(bad.sum()), GBps=round(nbytes / us / 1e3, 1),
                                           over_strict=round(us / row["decode_dat_strict"]["us"], 2))
        del payload_oob, x_oob
        row["drop_over_strict"] = round(row["decode_dat_drop"]["us"] / row["decode_dat_strict"]["us"], 2)
        row["numpy_route_over_from_dat"] = round(row["numpy_route_us"] / row["from_dat_us"], 2)
        row["seek"] = {}
        for nq in (64, 4096):
            q = rng.integers(1, int(t[-1]), nq).astype(np.int64)
            q[:8] = want[2][[n // 2, n // 4, 3 * n // 4, n // 8, 0, n - 1, n // 2 + 1, n // 3]]
            d_q, idx = torch.from_numpy(q).cuda(), torch.empty(nq, dtype=torch.int64, device="cuda")
            us_s = median_us(lambda: lib.evrep_dat_seek_time(ptr(rec.t), n, ptr(d_q), nq, 100000, ptr(idx), stream), args.reps)
            assert np.array_equal(idx.cpu().numpy(), dat_seek_index(want[2], q))
            us_i = median_us(lambda: lib.evrep_time_to_index(ptr(rec.t), n, ptr(d_q), nq, ptr(idx), stream), args.reps)
            row["seek"][str(nq)] = dict(dat_seek_time_us=round(us_s, 2), time_to_index_us=round(us_i, 2))
        result["inputs"][name] = row
        os.remove(path)
        del rec, cols, d_dat, d_bin
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
