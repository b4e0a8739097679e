#!/usr/bin/env python3
"""Times of the head's decode and tail (detector_head.predict / train_outputs / predict_batch) beside the reference's route, in
the same run.

    python tools/bench_detector_head.py [--reps 50] [--out FILE.json] [--dtype float32|float16|bfloat16]

With --dtype float16 / bfloat16 the tool times a 16-bit model's maps instead (amp_rows below): the cast route against the typed
entry.  The default float32 gives what is described here.

B = 32 images at 640 x 640, three levels (strides 8, 16, 32: N = 8400) and four levels (strides 8 .. 64: N = 8500), nc in
{2, 80}, reg_max = 16.  Medians over `reps` runs after warm-up, in us.  Device calls are bracketed by HIP events; the torch
routes are taken with the host clock, the device drained before and after.
  (a) reference_eval    the statements of Detect.forward's evaluation branch behind the convolutions as torch calls on the device
                        in float32: per level reshape, permute, softmax, the 1 x 1 convolution with 0 .. reg_max, sigmoid; the
                        concatenations and permutes, the anchors made anew on every call, dist2bbox(xywh), the multiply by the
                        strides, torch.ones and the last cat.
  (b) predict           one launch.
  (c) copy              a device-to-device copy of HALF the bytes (b) reads plus writes, so that the copy's own reads plus
                        writes are that many bytes.
  (d) train             the training branch as torch calls (a sigmoid per level, flatten / permute / cat) forward plus
                        autograd's backward, against train_outputs forward plus backward, both driven by
                        torch.autograd.backward with given gradients of the two outputs.  Also train_outputs' forward alone:
                        it reads what (b) reads, writes more, and has no DFL exponentials.
  (e) detections        predict_batch against (a) followed by nms_batch.
  (f) kernels           the three launches apart, from torch.profiler's device times (an error text where it gives none): (b)
                        and (d) also hold the host's part of a call -- the checks of the maps, the level table, the allocation.
The expectations are (b) < (a), (b) within a small multiple of (c), and that the float64 exp of E1 (68 per anchor and pass at
R = 16) does not dominate (b).  The tool prints the figures and asserts nothing about them; it does compare the two routes'
outputs (1e-3 pixels, 1e-6 on the scores: the reference route runs in float32)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from event_representation_study_amd import detector_head as dh  # noqa: E402
from event_representation_study_amd.detector_output import nms_batch  # noqa: E402

S, R = 640, 16
CONF, IOU = 0.25, 0.45
KERNELS = ("k_dethead_predict", "k_dethead_train", "k_dethead_backward")


def event_us(launch, reps, warmup=5):
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


def host_us(call, reps, warmup=5):
    times = []
    for k in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        if k >= warmup:
            times.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(times))


def kernel_us(launch, reps=10):
    """Mean device time per launch of each of the head's kernels, by name; {} where the profiler gives none."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                launch()
            torch.cuda.synchronize()
        out = {}
        for e in prof.key_averages():
            for name in KERNELS:
                if name in e.key:
                    total = getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0)
                    out[name] = round(float(total) / max(e.count, 1), 1)
        return out
    except Exception as exc:  # these figures are optional: say why they are missing
        return {"error": repr(exc)[:200]}


def reference_eval(cls_maps, reg_maps, strides, proj):
    """The evaluation branch behind the convolutions, statement by statement, as torch calls."""
    scores, dists, points, stride_t = [], [], [], []
    dev = cls_maps[0].device
    for c, r, s in zip(cls_maps, reg_maps, strides):
        b, _, h, w = c.shape
        n = h * w
        r = r.reshape([-1, 4, R + 1, n]).permute(0, 2, 1, 3)
        r = F.conv2d(F.softmax(r, dim=1), proj)
        scores.append(torch.sigmoid(c).reshape([b, -1, n]))
        dists.append(r.reshape([b, 4, n]))
        sx = torch.arange(end=w, device=dev) + 0.5
        sy = torch.arange(end=h, device=dev) + 0.5
        sy, sx = torch.meshgrid(sy, sx, indexing="ij")
        points.append(torch.stack([sx, sy], axis=-1).to(torch.float).reshape([-1, 2]))
        stride_t.append(torch.full((n, 1), s, dtype=torch.float, device=dev))
    scores = torch.cat(scores, axis=-1).permute(0, 2, 1)
    dists = torch.cat(dists, axis=-1).permute(0, 2, 1)
    points, stride_t = torch.cat(points), torch.cat(stride_t)
    lt, rb = torch.split(dists, 2, -1)
    x1y1, x2y2 = points - lt, points + rb
    boxes = torch.cat([(x1y1 + x2y2) / 2, x2y2 - x1y1], -1)
    boxes *= stride_t
    return torch.cat([boxes, torch.ones((boxes.shape[0], boxes.shape[1], 1), device=dev, dtype=boxes.dtype), scores], axis=-1)


def reference_train(cls_maps, reg_maps):
    scores = torch.cat([torch.sigmoid(c).flatten(2).permute((0, 2, 1)) for c in cls_maps], axis=1)
    distri = torch.cat([r.flatten(2).permute((0, 2, 1)) for r in reg_maps], axis=1)
    return scores, distri


def amp_rows(args, dev, B, K, dtype):
    """--dtype float16 / bfloat16: a 16-bit model's maps.  (a) today's route for them -- .float() per map, the float32 entry,
    and in training autograd's cast of every gradient map back to the maps' dtype -- against (b) the typed entry on the 16-bit
    maps as they are, with (c) a device copy of half the bytes (b) reads plus writes; evaluation (predict), the training
    forward, and forward plus backward.  HIP events around the whole of each; the three launches apart from torch.profiler."""
    rows = []
    for strides in ((8, 16, 32), (8, 16, 32, 64)):
        shapes = [(S // s, S // s) for s in strides]
        N = sum(h * w for h, w in shapes)
        for nc in (2, 80):
            g = torch.Generator(device=dev).manual_seed(100 * len(strides) + nc)
            cls = [(torch.randn((B, nc, h, w), device=dev, generator=g) * 2.0 - 5.0).to(dtype) for h, w in shapes]
            reg = [(torch.randn((B, 4 * K, h, w), device=dev, generator=g) * 2.0).to(dtype) for h, w in shapes]
            out = torch.empty((B, N, 5 + nc), device=dev)
            gs, gd = torch.randn((B, N, nc), device=dev, generator=g), torch.randn((B, N, 4 * K), device=dev, generator=g)
            cls_g, reg_g = [c.clone().requires_grad_(True) for c in cls], [r.clone().requires_grad_(True) for r in reg]
            in_bytes, out_bytes = sum(t.numel() * 2 for t in cls + reg), out.numel() * 4
            half = (in_bytes + out_bytes) // 2
            src, dst = torch.empty(half, dtype=torch.uint8, device=dev), torch.empty(half, dtype=torch.uint8, device=dev)

            def clear():
                for t in cls_g + reg_g:
                    t.grad = None

            def train_cast():
                clear()
                torch.autograd.backward(list(dh.train_outputs([c.float() for c in cls_g], [r.float() for r in reg_g], R, True)), [gs, gd])

            def train_typed():
                clear()
                torch.autograd.backward(list(dh.train_outputs(cls_g, reg_g, R, True)), [gs, gd])

            train_cast()
            want_g = [t.grad.clone() for t in cls_g + reg_g]
            train_typed()
            same = all(t.grad.dtype == dtype and torch.equal(t.grad.view(torch.int16), w_.view(torch.int16)) for t, w_ in zip(cls_g + reg_g, want_g))
            same = same and torch.equal(dh.predict(cls, reg, strides, R, True).view(torch.int32),
                                        dh.predict([c.float() for c in cls], [r.float() for r in reg], strides, R, True).view(torch.int32))
            t = {"a_predict_cast_us": event_us(lambda: dh.predict([c.float() for c in cls], [r.float() for r in reg], strides, R, True, out=out), args.reps),
                 "b_predict_typed_us": event_us(lambda: dh.predict(cls, reg, strides, R, True, out=out), args.reps),
                 "c_copy_us": event_us(lambda: dst.copy_(src), args.reps),
                 "a_train_cast_fwd_bwd_us": event_us(train_cast, args.reps), "b_train_typed_fwd_bwd_us": event_us(train_typed, args.reps)}
            with torch.no_grad():
                t["a_train_cast_fwd_us"] = event_us(lambda: dh.train_outputs([c.float() for c in cls], [r.float() for r in reg], R, True), args.reps)
                t["b_train_typed_fwd_us"] = event_us(lambda: dh.train_outputs(cls, reg, R, True), args.reps)
            kernels = kernel_us(lambda: dh.predict(cls, reg, strides, R, True, out=out))
            kernels.update(kernel_us(train_typed))
            row = {"dtype": str(dtype).replace("torch.", ""), "B": B, "levels": len(strides), "N": N, "nc": nc, "reps": args.reps}
            row.update({k: round(v, 1) for k, v in t.items()})
            row.update({"bytes_read_plus_written_mb": round((in_bytes + out_bytes) / 1e6, 1), "kernels_us": kernels,
                        "b_below_a_predict": bool(t["b_predict_typed_us"] < t["a_predict_cast_us"]),
                        "b_below_a_train": bool(t["b_train_typed_fwd_bwd_us"] < t["a_train_cast_fwd_bwd_us"]),
                        "b_over_c": round(t["b_predict_typed_us"] / t["c_copy_us"], 2), "routes_agree_bit_for_bit": bool(same)})
            rows.append(row)
            print(json.dumps(row), flush=True)
            del cls, reg, out, src, dst, gs, gd, cls_g, reg_g, want_g
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default=None)
    ap.add_argument("--dtype", choices=("float32", "float16", "bfloat16"), default="float32",
                    help="the maps' dtype; a 16-bit one times the cast route against the typed entry instead")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_detector_head needs the GPU: no time is taken without one")
    dev, B, K = torch.device("cuda:0"), args.batch, R + 1
    proj = torch.linspace(0, R, K, device=dev).view(1, K, 1, 1)
    rows = []
    if args.dtype != "float32":
        rows = amp_rows(args, dev, B, K, getattr(torch, args.dtype))
    for strides in ((8, 16, 32), (8, 16, 32, 64)) if args.dtype == "float32" else ():
        shapes = [(S // s, S // s) for s in strides]
        N = sum(h * w for h, w in shapes)
        for nc in (2, 80):
            g = torch.Generator(device=dev).manual_seed(100 * len(strides) + nc)
            cls = [torch.randn((B, nc, h, w), device=dev, generator=g) * 2.0 - 5.0 for h, w in shapes]
            reg = [torch.randn((B, 4 * K, h, w), device=dev, generator=g) * 2.0 for h, w in shapes]
            out = torch.empty((B, N, 5 + nc), device=dev)
            want = reference_eval(cls, reg, strides, proj)
            got = dh.predict(cls, reg, strides, R, True, out=out)
            box_diff = float((got[..., :4] - want[..., :4]).abs().max())
            cls_diff = float((got[..., 5:] - want[..., 5:]).abs().max())
            in_bytes = sum(t.numel() * 4 for t in cls + reg)
            out_bytes = out.numel() * 4
            half = (in_bytes + out_bytes) // 2
            src, dst = torch.empty(half, dtype=torch.uint8, device=dev), torch.empty(half, dtype=torch.uint8, device=dev)
            gs, gd = torch.randn((B, N, nc), device=dev, generator=g), torch.randn((B, N, 4 * K), device=dev, generator=g)
            cls_g, reg_g = [c.clone().requires_grad_(True) for c in cls], [r.clone().requires_grad_(True) for r in reg]

            def clear():
                for t in cls_g + reg_g:
                    t.grad = None

            def train_reference():
                clear()
                torch.autograd.backward(list(reference_train(cls_g, reg_g)), [gs, gd])

            def train_ours():
                clear()
                torch.autograd.backward(list(dh.train_outputs(cls_g, reg_g, R, True)), [gs, gd])

            train_reference()
            want_g = [t.grad.clone() for t in cls_g + reg_g]
            train_ours()
            grad_diff = max(float((t.grad - w_).abs().max()) for t, w_ in zip(cls_g + reg_g, want_g))

            t_a = host_us(lambda: reference_eval(cls, reg, strides, proj), args.reps)
            t_b = event_us(lambda: dh.predict(cls, reg, strides, R, True, out=out), args.reps)
            t_c = event_us(lambda: dst.copy_(src), args.reps)
            t_d_ref = host_us(train_reference, args.reps)
            t_d_ours = event_us(train_ours, args.reps)
            with torch.no_grad():
                t_d_fwd = event_us(lambda: dh.train_outputs(cls, reg, R, True), args.reps)
            t_e_ref = host_us(lambda: nms_batch(reference_eval(cls, reg, strides, proj).contiguous(), CONF, IOU), args.reps)
            t_e_ours = event_us(lambda: dh.predict_batch(cls, reg, CONF, IOU, strides=strides, reg_max=R), args.reps)
            t_nms = event_us(lambda: nms_batch(out, CONF, IOU), args.reps)
            kernels = kernel_us(lambda: dh.predict(cls, reg, strides, R, True, out=out))
            kernels.update(kernel_us(train_ours))
            row = {"B": B, "levels": len(strides), "N": N, "nc": nc, "reps": args.reps,
                   "a_reference_eval_host_us": round(t_a, 1), "b_predict_us": round(t_b, 1), "c_copy_us": round(t_c, 1),
                   "bytes_read_plus_written_mb": round((in_bytes + out_bytes) / 1e6, 1),
                   "b_gb_per_s": round((in_bytes + out_bytes) / t_b / 1e3, 1), "a_over_b": round(t_a / t_b, 1),
                   "b_over_c": round(t_b / t_c, 2), "b_below_a": bool(t_b < t_a),
                   "d_train_reference_fwd_bwd_host_us": round(t_d_ref, 1), "d_train_outputs_fwd_bwd_us": round(t_d_ours, 1),
                   "d_train_outputs_fwd_us": round(t_d_fwd, 1), "b_minus_train_fwd_us": round(t_b - t_d_fwd, 1),
                   "e_reference_eval_plus_nms_host_us": round(t_e_ref, 1), "e_predict_batch_us": round(t_e_ours, 1),
                   "nms_batch_us": round(t_nms, 1), "kernels_us": kernels,
                   "box_max_abs_diff_px": box_diff, "class_max_abs_diff": cls_diff, "grad_max_abs_diff": grad_diff,
                   "routes_agree": bool(box_diff < 1e-3 and cls_diff < 1e-6 and grad_diff < 1e-6)}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del cls, reg, out, src, dst, gs, gd, cls_g, reg_g, want, got, want_g
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
