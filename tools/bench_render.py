#!/usr/bin/env python3
"""Times of the device renderings (EventBatch.render) beside the route they replace and beside their yardsticks.

    python tools/bench_render.py [--shapes gen1,hd] [--streams uniform,circle] [--reps 50] [--host-reps 50] [--out FILE.jsonl]

Per shape (32 windows x 50 000 events at 304x240 and at 1280x720) and stream (synthetic.make_events, make_events_moving_circle),
medians over `reps` after warm-up, rotating over three resident batches:
  (a) host     the reference's statements in numpy, one window per Python call in a loop over the 32 host windows, on a host
               clock (one core).  numba is absent here: the *_NO_OVERLAP loop is stated as np.unique on the reversed pixel ids
               (first visit of the reversed stream = last event), which is what a compiled loop computes, vectorised;
  (b) render   EventBatch.render(type, check=False) per type, HIP events: state + compose + the allocations of the call;
  (c) kernels  evrep_render_state (three forms: flags only, + net, + surface) and evrep_render_compose per type, alone, into
               tensors allocated once;
  (d) binning  the binning pass of the same batch (rebin);
  (e) copy     a device-to-device copy of the output's bytes; and EventStack's stream builder on the same batch, the launch
               k_render_state shares its skeleton with.
One GPU process.  Every line is one JSON object."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from event_representation_study_amd import synthetic  # noqa: E402
from event_representation_study_amd.engine import EventBatch  # noqa: E402
from event_representation_study_amd.evlicious_render import RenderingType, jet_lut, render_compose, render_state  # noqa: E402

SHAPES = {"gen1": (304, 240), "hd": (1280, 720)}      # name: (W, H)
STREAMS = {"uniform": synthetic.make_events, "circle": synthetic.make_events_moving_circle}
B, N = 32, 50000


def median_us(launch, items, reps, warmup=5):
    for i in range(warmup):
        launch(items[i % len(items)])
    torch.cuda.synchronize()
    times = []
    for i in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch(items[i % len(items)])
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return float(np.median(times))


def host_render(win, H, W, rt, lut):
    """One window as the reference states it (render.py), in numpy."""
    x, y, t, p = win[:, 0], win[:, 1], win[:, 2].astype(np.int64), win[:, 3]
    if rt == RenderingType.EVENT_FRAME:
        img = np.zeros((H, W), np.float32)
        np.add.at(img, (y, x), p)
        gray = np.clip(20 * img + 128, 0, 255).astype(np.uint8)
        return np.stack([gray, gray, gray], axis=-1)
    if rt == RenderingType.TIME_SURFACE:
        img = np.zeros((H, W), np.float32)
        np.add.at(img, (y, x), np.exp(-(t[-1] - t) / 3e4))
        return lut[np.minimum((img * np.float32(256)).astype(np.int64), 255)]
    out = np.full((H, W, 3), 255, np.uint8)
    if rt == RenderingType.RED_BLUE_OVERLAP:
        out[y, x, :] = 0
        out[y, x, p + 1] = 255
        return out
    _, first = np.unique((y.astype(np.int64) * W + x)[::-1], return_index=True)
    last = len(x) - 1 - first
    pos = p[last] > 0
    if rt == RenderingType.RED_BLUE_NO_OVERLAP:
        out[y[last], x[last]] = np.where(pos[:, None], np.array([0, 0, 255], np.uint8), np.array([255, 0, 0], np.uint8))
    else:
        out[y[last], x[last]] = np.where(pos[:, None], np.uint8(255), np.uint8(0))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="gen1,hd")
    ap.add_argument("--streams", default="uniform,circle")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--host-reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_render.py needs a HIP device"
    rows, lut = [], jet_lut()

    def emit(**row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    for shape in args.shapes.split(","):
        W, H = SHAPES[shape]
        for stream in args.streams.split(","):
            wins = [[STREAMS[stream](N, W, H, seed=100 * c + b) for b in range(B)] for c in range(3)]
            bs = [EventBatch.from_numpy(w, H, W) for w in wins]
            idx = {b: i for i, b in enumerate(bs)}
            base = dict(shape=shape, W=W, H=H, stream=stream, windows=B, events_per_window=N, binning_pass=int(bs[0].plan.reserved))
            bin_us = median_us(lambda b: b.rebin(), bs, args.reps)
            emit(what="binning", us=round(bin_us, 2), **base)
            es_out = torch.empty((B, H, W, 12), dtype=torch.float32, device="cuda:0")
            emit(what="event_stack_builder", us=round(median_us(lambda b: b.event_stack(out=es_out), bs, args.reps), 2), **base)
            st = [torch.empty((B, H, W), dtype=torch.uint8, device="cuda:0") for _ in bs]
            net = [torch.empty((B, H, W), dtype=torch.int32, device="cuda:0") for _ in bs]
            surf = [torch.empty((B, H, W), dtype=torch.float32, device="cuda:0") for _ in bs]
            for form, kw in (("flags", {}), ("flags+net", dict(net=True)), ("flags+surface", dict(surface=True))):
                def launch(b, kw=kw):
                    i = idx[b]
                    render_state(b, state=st[i], net=net[i] if "net" in kw else False, surface=surf[i] if "surface" in kw else False)
                emit(what="k_render_state", form=form, us=round(median_us(launch, bs, args.reps), 2), **base)
            for b in bs:        # every state tensor filled for the compose launches
                render_state(b, state=st[idx[b]], net=net[idx[b]], surface=surf[idx[b]])
            for rt in RenderingType:
                ts = rt == RenderingType.TIME_SURFACE
                out = torch.empty((B, H, W, 4 if ts else 3), dtype=torch.float64 if ts else torch.uint8, device="cuda:0")
                dst = torch.empty_like(out)
                nbytes = out.numel() * out.element_size()
                copy_us = median_us(lambda b: dst.copy_(out), bs, args.reps)
                for cast in ((True, False) if rt <= RenderingType.BLACK_WHITE_NO_OVERLAP else (True,)):
                    us_c = median_us(lambda b: render_compose(st[idx[b]], rt, cast=cast, net=net[idx[b]], surface=surf[idx[b]], out=out),
                                     bs, args.reps)
                    us_r = median_us(lambda b: b.render(rt, cast=cast, check=False), bs, args.reps)
                    emit(what="render", type=rt.name, cast=cast, render_us=round(us_r, 2), compose_us=round(us_c, 2),
                         copy_us=round(copy_us, 2), out_bytes=nbytes, compose_over_copy=round(us_c / copy_us, 2),
                         out_gb_per_s=round(nbytes / us_c / 1e3, 1), **base)
                if args.host_reps > 0:
                    times = []
                    for r in range(args.host_reps + 1):
                        t0 = time.perf_counter()
                        for w in wins[r % 3]:
                            host_render(w, H, W, rt, lut)
                        times.append((time.perf_counter() - t0) * 1e6)
                    emit(what="host_numpy_loop", type=rt.name, us=round(float(np.median(times[1:]))), reps=args.host_reps,
                         note="numpy statements, one window per call, one core; NO_OVERLAP as np.unique on reversed pixel ids (no numba)",
                         **base)
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
