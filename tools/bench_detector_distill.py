#!/usr/bin/env python3
"""Times of the distillation losses (detector_distill.distill_batch and distill_cw, forward and backward) beside the
reference's route and beside loss_batch on the same shape, in the same run.

    python tools/bench_detector_distill.py [--reps 50] [--batch 32] [--out FILE.json] [--dtype float32|float16|bfloat16]

With --dtype float16 / bfloat16 the tool times distill_cw on a 16-bit model's maps instead: the cast route (.float() per map,
the float32 entry, autograd's cast back) against the maps as they are, and a copy of the typed route's bytes.

distill_batch: B = 32 images at 640 x 640 (A = 8400 anchors), nc in {2, 80}, 50 labels per image, T = 20; the targets are
assign_batch's on tests/detector_assign_cases' head, the logits tests/detector_loss_cases', the teacher
tests/detector_distill_cases'.  distill_cw: the three neck maps of configs/gen1_optimized.py at 640 x 640, (B, 128, 80, 80),
(B, 256, 40, 40), (B, 512, 20, 20).  Medians over `reps` runs after warm-up, in us:
  (a) reference_route   the statements of loss_distill.py restated as torch calls on the device, float32 predictions and
                        float64 targets (tests/detector_distill_ref.py), with autograd's backward.  Host clock, device drained
                        before and after (the route reads the device).
  (b) ours              HIP events around distill_batch(...) / distill_cw(...) and loss.backward().
  (c) loss_batch        the same for detector_loss.loss_batch on the same shape: what the distillation entry adds.
  (d) kernels           the launches apart, from torch.profiler's device times (null where the profiler gives none), with the
                        bytes each must move (inputs read once, outputs written once) and the time of a device-to-device copy
                        that moves as many bytes (a copy of n / 2 bytes reads and writes n): copy_share = copy time / kernel time.
  (e) launches          device launches of one forward + backward on either side, counted by torch.profiler.
The tool prints the figures and asserts nothing about them.  It does compare the losses: with the reference's route run once in
float64 (`loss_rel_diff`, `losses_agree` below 1e-9), and with its float32 run that is timed (`loss_rel_diff_f32_route`: the KL
sums cancel, so float32 loses digits there)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import detector_assign_cases as acases  # noqa: E402
import detector_distill_cases as dcases  # noqa: E402
import detector_distill_ref as ref  # noqa: E402
import detector_loss_cases as lcases  # noqa: E402
from event_representation_study_amd import detector_assign as da, detector_distill as dd, detector_loss as dl  # noqa: E402

S, R, T, EPOCH, MAX_EPOCH = 640, 16, 20.0, 3, 10
KERNELS = ("k_detloss_rows", "k_detdistill_cls", "k_detloss_cls", "k_detloss_box", "k_detloss_fold", "k_detdistill_cw_fold", "k_detdistill_cw")
FEATS = ((128, 80, 80), (256, 40, 40), (512, 20, 20))


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


def host_us(call, reps, warmup=3):
    times = []
    for k in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        if k >= warmup:
            times.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(times))


def profiled(launch, reps):
    """(mean device time per launch of each of the library's kernels by name, device launches per call); the first is a dict
    with "error" where the profiler gives nothing."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                launch()
            torch.cuda.synchronize()
        out, count = {}, 0
        for e in prof.key_averages():
            total = getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0)
            if total > 0:
                count += e.count
            for name in KERNELS:
                if name in e.key and name not in out and not (name == "k_detdistill_cw" and "fold" in e.key):
                    out[name] = round(float(total) / max(e.count, 1), 1)
        return out, round(count / reps, 1)
    except Exception as exc:  # the figures of (d) and (e) are optional: say why they are missing
        return {"error": repr(exc)[:200]}, None


def copy_us(nbytes, reps):
    """A device-to-device copy that moves nbytes in all (reads half, writes half)."""
    n = max(int(nbytes) // 8, 1)
    a, b = torch.empty(n, dtype=torch.float32, device="cuda:0"), torch.empty(n, dtype=torch.float32, device="cuda:0")
    return event_us(lambda: b.copy_(a), reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default=None)
    ap.add_argument("--dtype", choices=("float32", "float16", "bfloat16"), default="float32",
                    help="the feature maps' dtype; a 16-bit one times distill_cw's cast route against the typed entry instead")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_detector_distill needs the GPU: no time is taken without one")
    dev, B, K = torch.device("cuda:0"), args.batch, R + 1
    rows, n_lab = [], 50
    if args.dtype != "float32":
        # the channel-wise term on a 16-bit model's maps: (a) today's route -- .float() per map (six launches), the float32
        # entry, autograd's cast of the three gradients back -- against (b) the maps as they are, and (c) a copy of (b)'s bytes
        dtype = getattr(torch, args.dtype)
        rng = np.random.default_rng(8200)
        s0 = [torch.from_numpy(rng.normal(0, 1.5, (B,) + sh).astype(np.float32)).to(dev).to(dtype) for sh in FEATS]
        t0 = [(x.float() + 0.7 * torch.randn_like(x.float())).to(dtype) for x in s0]

        def cw(cast, scale=65536.0):
            s = [x.detach().requires_grad_(True) for x in s0]
            loss = dd.distill_cw([x.float() for x in s], [x.float() for x in t0]) if cast else dd.distill_cw(s, t0)
            (loss * scale).backward()
            return loss.detach(), [x.grad for x in s]
        (la, ga), (lb, gb) = cw(True), cw(False)
        same = bool(la.item() == lb.item()) and all(a.dtype == b.dtype == dtype and torch.equal(a.view(torch.int16), b.view(torch.int16))
                                                    for a, b in zip(ga, gb))
        t_a, t_b = event_us(lambda: cw(True), args.reps), event_us(lambda: cw(False), args.reps)
        with torch.no_grad():
            t_a_fwd = event_us(lambda: dd.distill_cw([x.float() for x in s0], [x.float() for x in t0]), args.reps)
            t_b_fwd = event_us(lambda: dd.distill_cw(s0, t0), args.reps)
        kern, launches = profiled(lambda: cw(False), 10)
        _, launches_a = profiled(lambda: cw(True), 10)
        nbytes = sum(x.numel() for x in s0) * (2 + 2 + 4)
        tc = copy_us(nbytes, args.reps)
        row = {"what": "distill_cw", "dtype": args.dtype, "B": B, "maps": [list(sh) for sh in FEATS], "reps": args.reps,
               "a_cast_fwd_bwd_us": round(t_a, 1), "b_typed_fwd_bwd_us": round(t_b, 1), "a_cast_fwd_us": round(t_a_fwd, 1),
               "b_typed_fwd_us": round(t_b_fwd, 1), "c_copy_us": round(tc, 1), "bytes": nbytes, "kernels_us": kern,
               "launches": {"typed": launches, "cast": launches_a}, "b_below_a": bool(t_b < t_a), "routes_agree_bit_for_bit": same}
        print(json.dumps(row), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                f.write(json.dumps(row) + "\n")
        return
    for nc in (2, 80):
        scores_h, _, anc_h = acases.head(8000 + nc, B, S, nc)
        c = dcases.with_teacher(lcases.base(8001 + nc, S=S, B=B, nc=1), 8002 + nc, T=T, epoch=EPOCH, max_epoch=MAX_EPOCH)
        rng = np.random.default_rng(8003 + nc)
        anc, stride = (torch.from_numpy(v).to(dev) for v in da.anchor_points(S))
        p0, z0 = torch.from_numpy(scores_h).to(dev), torch.from_numpy(c["z"]).to(dev)
        tp0 = torch.from_numpy(np.clip(scores_h + rng.normal(0, 0.1, scores_h.shape), 0.01, 0.99).astype(np.float32)).to(dev)
        tz0 = torch.from_numpy(c["tz"]).to(dev)
        A = len(anc_h)
        t = torch.from_numpy(acases.targets(8100 + n_lab, [n_lab] * B, nc)).to(dev)
        _, boxes_px = dl.decode_boxes(z0, anc, stride, R, True)
        labels, tb, ts, fg, _ = da.assign_batch(p0, boxes_px, anc, t, (S, S), nc, max_labels=n_lab)

        def reference():
            return ref.distill_terms(p0, z0, tp0, tz0, anc, stride, labels, tb, ts, fg, nc, R, True, lcases.WEIGHTS, T, EPOCH, MAX_EPOCH,
                                     dtype=torch.float32, scalars=False)

        def ours():
            p, z = p0.detach().requires_grad_(True), z0.detach().requires_grad_(True)
            loss, items = dd.distill_batch(p, z, tp0, tz0, anc, stride, labels, tb, ts, fg, nc, T, EPOCH, MAX_EPOCH, R, True)
            loss.backward()
            return loss

        def plain():
            p, z = p0.detach().requires_grad_(True), z0.detach().requires_grad_(True)
            loss, items = dl.loss_batch(p, z, anc, stride, labels, tb, ts, fg, nc, R, True)
            loss.backward()
            return loss

        r, o = reference(), ours().detach()
        r64 = ref.distill_terms(p0, z0, tp0, tz0, anc, stride, labels, tb, ts, fg, nc, R, True, lcases.WEIGHTS, T, EPOCH, MAX_EPOCH,
                                scalars=False)
        rel32 = abs(float(r["loss"]) - float(o)) / abs(float(o))
        rel = abs(float(r64["loss"]) - float(o)) / abs(float(o))
        del r64
        t_ref = host_us(reference, max(args.reps // 5, 5))
        t_ours, t_plain = event_us(ours, args.reps), event_us(plain, args.reps)
        kern, launches = profiled(ours, 10)
        kern_plain, launches_plain = profiled(plain, 10)
        _, launches_ref = profiled(reference, 3)
        ba = B * A
        must = {"k_detloss_rows": ba * nc * 8 + ba + ba * 8,
                "k_detdistill_cls": ba * nc * (4 + 4 + 8 + 4) + ba * 9,
                "k_detloss_box": ba * 4 * K * 4 + ba * 9 + int(fg.sum()) * 4 * K * 8}
        detail = {}
        for name, nbytes in must.items():
            tc = copy_us(nbytes, args.reps)
            detail[name] = {"bytes": nbytes, "copy_us": round(tc, 1), "kernel_us": kern.get(name),
                            "copy_share": round(tc / kern[name], 2) if kern.get(name) else None}
        row = {"what": "distill_batch", "B": B, "A": A, "nc": nc, "labels_per_image": n_lab, "reps": args.reps, "foreground": int(fg.sum()),
               "reference_route_host_us": round(t_ref, 1), "distill_batch_fwd_bwd_us": round(t_ours, 1),
               "loss_batch_fwd_bwd_us": round(t_plain, 1), "teacher_bytes": ba * (nc + 4 * K) * 4,
               "teacher_copy_us": round(copy_us(2 * ba * (nc + 4 * K) * 4, args.reps) / 2, 1),
               "reference_over_ours": round(t_ref / t_ours, 1), "kernels_us": kern, "loss_batch_kernels_us": kern_plain, "kernels": detail,
               "launches": {"ours": launches, "loss_batch": launches_plain, "reference_route": launches_ref},
               "loss_rel_diff": rel, "loss_rel_diff_f32_route": rel32, "losses_agree": bool(rel < 1e-9)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del p0, z0, tp0, tz0, labels, tb, ts, fg
    # the channel-wise term
    rng = np.random.default_rng(8200)
    s0 = [torch.from_numpy(rng.normal(0, 1.5, (B,) + sh).astype(np.float32)).to(dev) for sh in FEATS]
    t0 = [(x + 0.7 * torch.randn_like(x)) for x in s0]

    def reference_cw():
        return ref.cw_terms(s0, t0, 1, dtype=torch.float32, scalars=False)

    def ours_cw():
        s = [x.detach().requires_grad_(True) for x in s0]
        loss = dd.distill_cw(s, t0)
        loss.backward()
        return loss

    r, o = reference_cw(), ours_cw().detach()
    rel32 = abs(float(r["loss"]) - float(o)) / abs(float(o))
    rel = abs(float(ref.cw_terms(s0, t0, 1, scalars=False)["loss"]) - float(o)) / abs(float(o))
    t_ref = host_us(reference_cw, max(args.reps // 5, 5))
    t_ours = event_us(ours_cw, args.reps)
    kern, launches = profiled(ours_cw, 10)
    _, launches_ref = profiled(reference_cw, 3)
    nbytes = sum(x.numel() for x in s0) * 12
    tc = copy_us(nbytes, args.reps)
    row = {"what": "distill_cw", "B": B, "maps": [list(sh) for sh in FEATS], "reps": args.reps, "reference_route_host_us": round(t_ref, 1),
           "distill_cw_fwd_bwd_us": round(t_ours, 1), "reference_over_ours": round(t_ref / t_ours, 1), "kernels_us": kern,
           "kernels": {"k_detdistill_cw": {"bytes": nbytes, "copy_us": round(tc, 1), "kernel_us": kern.get("k_detdistill_cw"),
                                           "copy_share": round(tc / kern["k_detdistill_cw"], 2) if kern.get("k_detdistill_cw") else None}},
           "launches": {"ours": launches, "reference_route": launches_ref}, "loss_rel_diff": rel, "loss_rel_diff_f32_route": rel32,
           "losses_agree": bool(rel < 1e-9)}
    rows.append(row)
    print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
