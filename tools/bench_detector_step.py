#!/usr/bin/env python3
"""Times of the parameter update (detector_step.TrainStep) beside the reference's route, in the same run.

    python tools/bench_detector_step.py [--reps 50] [--blocks 8] [--out FILE.json]

The parameter set is built here and reads nothing else: for each width w in 32, 64, 128, 256, 512, `blocks` times
Conv2d(w, w, 3, bias=False) + BatchNorm2d(w) + Conv2d(w, w, 1, bias=True).  With 8 blocks that is 200 parameter tensors in the
three groups of build_optimizer and 80 floating buffers (the BN statistics), about 28 M parameter elements; the tool prints
the counts.  Gradients are random float32 tensors that stay in place, scaled by the scaler's 1024; no forward or backward pass
runs.  Medians over `reps` runs after warm-up, in us.
  (a) reference        the reference's route as torch calls on the device: torch.amp.GradScaler.step(torch.optim.SGD(nesterov)),
                       update(), zero_grad() and the ModelEMA loop over the state dict (two statements per floating entry).
                       Host clock with the device drained before and after, since that route reads the device; the
                       gradients are handed back before every run, outside the clock, because zero_grad() drops them.
  (b) train_step       TrainStep(optimizer, scaler, ema)(model), bracketed by HIP events; and the host's share of the call
                       (the clock around the call alone, nothing drained).
  (c) kernels          the three launches apart, from torch.profiler's device times (an error text where it gives none).
  (d) copy             a device-to-device copy whose reads plus writes equal the bytes (b) moves: 20 B read and 16 B written per
                       parameter element (g twice, p, buf, e; p, buf, e, g), 8 and 4 per buffer element.
  (e) launches         device kernels per step of (a), counted by torch.profiler.
The expectations are (b) < (a) and the apply launch within a small multiple of (d).  The tool prints the figures and says in
`b_below_a` / `apply_over_copy` how they fell; it asserts nothing about them.  It does compare the two routes' parameters
after the same steps (the torch route contracts its multiply-adds, so within 1e-6 relative, not bit for bit)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from event_representation_study_amd import detector_step as ds  # noqa: E402

WIDTHS = (32, 64, 128, 256, 512)
LR0, MOMENTUM, WEIGHT_DECAY, SCALE = 0.0032, 0.843, 0.00036, 1024.0
KERNELS = ("k_step_check", "k_step_apply", "k_step_finish")


def make_model(blocks, dev, seed=0):
    torch.manual_seed(seed)
    layers = []
    for w in WIDTHS:
        for _ in range(blocks):
            layers += [torch.nn.Conv2d(w, w, 3, bias=False), torch.nn.BatchNorm2d(w), torch.nn.Conv2d(w, w, 1, bias=True)]
    return torch.nn.Sequential(*layers).to(dev)


def groups_of(model):
    bn, w, b = [], [], []
    for m in model.modules():
        if isinstance(getattr(m, "bias", None), torch.nn.Parameter):
            b.append(m.bias)
        if isinstance(m, torch.nn.BatchNorm2d):
            bn.append(m.weight)
        elif isinstance(getattr(m, "weight", None), torch.nn.Parameter):
            w.append(m.weight)
    return bn, w, b


@torch.no_grad()
def ema_per_entry(averaged, model, decay):
    """Route (a)'s moving average: per floating entry of the state dict two in-place torch operations and one temporary,
    avg <- avg * decay, then avg <- avg + (1 - decay) * value.  Three launches per entry."""
    values = model.state_dict()
    for name, avg in averaged.state_dict().items():
        if torch.is_floating_point(avg):
            avg.mul_(decay)
            avg.add_(values[name] * (1 - decay))


def event_us(launch, reps, warmup=5):
    for _ in range(warmup):
        launch()
    torch.cuda.synchronize()
    times, host = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        t0 = time.perf_counter()
        launch()
        host.append((time.perf_counter() - t0) * 1e6)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return float(np.median(times)), float(np.median(host))


def host_us(call, reps, prepare=lambda: None, warmup=5):
    times = []
    for k in range(warmup + reps):
        prepare()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        if k >= warmup:
            times.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(times))


def profiled(launch, reps=5, prepare=lambda: None):
    """(mean device time per launch of each of the step's kernels by name, device kernels per run); an error text where the
    profiler gives none."""
    try:
        from torch.profiler import ProfilerActivity, profile
        prepare()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                prepare()
                launch()
            torch.cuda.synchronize()
        per, n = {}, 0
        for e in prof.key_averages():
            total = getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0)
            if not total or "memcpy" in e.key.lower() or "memset" in e.key.lower():
                continue
            n += e.count
            for name in KERNELS:
                if name in e.key:
                    per[name] = round(float(total) / max(e.count, 1), 1)
        return per, round(n / reps, 1)
    except Exception as exc:  # these figures are optional: say why they are missing
        return {"error": repr(exc)[:200]}, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_detector_step needs the GPU: no time is taken without one")
    dev = torch.device("cuda:0")

    # the two routes on two equal models, fed the same gradients
    ours_m, ref_m = make_model(args.blocks, dev), make_model(args.blocks, dev)
    n_param = sum(p.numel() for p in ours_m.parameters())
    n_buf = sum(b.numel() for b in ours_m.buffers() if b.dtype.is_floating_point)
    n_tensors = len(list(ours_m.parameters())) + sum(1 for b in ours_m.buffers() if b.dtype.is_floating_point)
    g = torch.Generator(device=dev).manual_seed(1)
    grads = [torch.randn(p.shape, device=dev, generator=g) * SCALE for p in ours_m.parameters()]

    import types
    cfg = types.SimpleNamespace(solver=types.SimpleNamespace(optim="SGD", lr0=LR0, momentum=MOMENTUM, weight_decay=WEIGHT_DECAY))
    opt = ds.build_optimizer(cfg, ours_m)
    step = ds.TrainStep(opt, ds.GradScaler(init_scale=SCALE), ds.ModelEMA(ours_m))
    own = [gr.clone() for gr in grads]
    for p, gr in zip(ours_m.parameters(), own):
        p.grad = gr

    def refill():
        torch._foreach_copy_(own, grads)

    bn, w, b = groups_of(ref_m)
    ref_opt = torch.optim.SGD(bn, lr=LR0, momentum=MOMENTUM, nesterov=True)
    ref_opt.add_param_group({"params": w, "weight_decay": WEIGHT_DECAY})
    ref_opt.add_param_group({"params": b})
    ref_scaler = torch.amp.GradScaler("cuda", init_scale=SCALE)
    ref_ema = ds.ModelEMA(ref_m)          # (its .ema, .updates and .decay only: the average is ema_per_entry's)

    def ref_prepare():
        for p, gr in zip(ref_m.parameters(), grads):
            p.grad = gr.clone()
        ref_scaler.scale(torch.zeros((), device=dev))

    def ref_step():
        ref_scaler.step(ref_opt)
        ref_scaler.update()
        ref_opt.zero_grad()
        ref_ema.updates += 1
        ema_per_entry(ref_ema.ema, ref_m, ref_ema.decay(ref_ema.updates))

    for _ in range(3):                                                  # the same three steps on both, then compare
        refill()
        step(ours_m)
        ref_prepare()
        ref_step()
    torch.cuda.synchronize()
    with torch.no_grad():
        rel = max(float((p - q).abs().max() / q.abs().max().clamp_min(1e-30)) for p, q in zip(ours_m.parameters(), ref_m.parameters()))
        rel_ema = max(float((p - q).abs().max() / q.abs().max().clamp_min(1e-30))
                      for p, q in zip(step.ema.ema.parameters(), ref_ema.ema.parameters()))

    t_a = host_us(ref_step, args.reps, ref_prepare)
    t_b, t_b_host = event_us(lambda: step(ours_m), args.reps)            # (gradients left at zero: the same bytes move)
    moved = 36 * n_param + 12 * n_buf
    src, dst = torch.empty(moved // 2, dtype=torch.uint8, device=dev), torch.empty(moved // 2, dtype=torch.uint8, device=dev)
    t_d, _ = event_us(lambda: dst.copy_(src), args.reps)
    kernels, _ = profiled(lambda: step(ours_m))
    _, launches_a = profiled(ref_step, prepare=ref_prepare)
    _, launches_b = profiled(lambda: step(ours_m))
    apply_us = kernels.get("k_step_apply")
    row = {"blocks": args.blocks, "tensors": n_tensors, "parameter_elements": n_param, "buffer_elements": n_buf, "reps": args.reps,
           "chunks": step._table.n_chunks, "table_uploads": step.table_uploads,
           "a_reference_host_us": round(t_a, 1), "b_train_step_us": round(t_b, 1), "b_host_call_us": round(t_b_host, 1),
           "c_kernels_us": kernels, "d_copy_us": round(t_d, 1), "bytes_moved_mb": round(moved / 1e6, 1),
           "b_gb_per_s": round(moved / t_b / 1e3, 1), "d_gb_per_s": round(moved / t_d / 1e3, 1),
           "e_launches_reference": launches_a, "e_launches_train_step": launches_b,
           "a_over_b": round(t_a / t_b, 1), "b_below_a": bool(t_b < t_a),
           "apply_over_copy": None if not apply_us else round(apply_us / t_d, 2),
           "parameters_max_rel_diff": rel, "ema_max_rel_diff": rel_ema, "routes_agree": bool(rel < 1e-6 and rel_ema < 1e-6)}
    print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
