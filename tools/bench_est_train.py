#!/usr/bin/env python3
"""Training the EST quantisation layer: forward + backward at 32 x 50 000 events on 304x240, C = 6 and C = 8.

    python tools/bench_est_train.py [--out FILE]

HIP events, median of 50 after warm-up, one JSON line per C:
  (a) ref_statements_fwd_bwd_ms  the reference's statements in torch on the device: t * mlp(t - i/(C-1)) per bin and
                                 put_(accumulate=True), forward + backward (the route the table replaces)
  (b) layer_fwd_bwd_ms           est.TrainableQuantizationLayer forward + backward (host preparation of the events and the
                                 table rebuild included, as a training step pays them)
  (c) backward_kernel_ms         EventBatch.est_voxel_backward alone
  (d) forward_kernel_ms          EventBatch.est_voxel alone (binned stream; the binning pass is bin_ms)
  (e) table_rebuild_ms           PiecewiseLinearKernel + piece_coefficients on the host (wall clock)
  (b') layer_cuda_fwd_bwd_ms     (b) with the events handed as a CUDA tensor: prepared on the device (est.prepare_events_device)
  (f) prepare_kernel_ms          evrep_est_prepare alone (engine.est_prepare: two launches and a memset, allocations included)
  (g) copy_40B_per_event_ms      a device-to-device copy of the same (N, 5) float32 rows: 20 B read + 20 B written per event
The value MLP is the trained one of tests/golden/est.npz (97 pieces).
"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from event_representation_study_amd import est  # noqa: E402
from event_representation_study_amd.engine import est_prepare  # noqa: E402
from event_representation_study_amd.synthetic import make_events  # noqa: E402


def median_ms(fn, k=50, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(k):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def reference_statements(vl, x, y, t, p, b, B, C, H, W, wt):
    """learned_repr.py:143-176 restated for device tensors (t already normalised), loss = (wt * vox).sum(), backward."""
    vox = torch.zeros(2 * C * H * W * B, dtype=torch.float32, device=t.device)
    idx0 = x + W * y + W * H * C * p + W * H * C * 2 * b
    for i in range(C):
        values = t * vl(t - i / (C - 1))
        vox = vox.put(idx0 + W * H * i, values, accumulate=True)
    (wt * vox).sum().backward()


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    H, W, B, N = 240, 304, 32, 50000
    g = np.load(os.path.join(ROOT, "tests", "golden", "est.npz"))
    state = {k[2:]: g[k] for k in g.files if k.startswith("w_")}
    wins = [make_events(N, W, H, seed=i, polarity="01") for i in range(B)]
    ev = np.concatenate([np.concatenate([w.astype(np.float32), np.full((N, 1), i, np.float32)], axis=1) for i, w in enumerate(wins)])
    ev[:, 2] += 1.0                                    # t.max() > 0 in every item
    events = torch.from_numpy(ev)
    events_dev = events.to("cuda:0")
    copy_dst = torch.empty_like(events_dev)
    t_prep = median_ms(lambda: est_prepare(events_dev, B, H, W))
    t_copy = median_ms(lambda: copy_dst.copy_(events_dev))
    lines = []
    for C in (6, 8):
        layer = est.TrainableQuantizationLayer((C, H, W), est.ValueLayer(state), image_size=None)
        batch, tn = est.prepare_events(events, H, W, layer.device)
        kern = layer.table()
        seg, bucket = kern.device_table(layer.device)
        wt = torch.randn((B, H, W, 2 * C), device=layer.device)
        batch.bin()
        t_bin = median_ms(lambda: batch.rebin())
        t_fwd = median_ms(lambda: batch.est_voxel(tn, C, seg, bucket, kern.lo, kern.hi))
        t_bwd = median_ms(lambda: batch.est_voxel_backward(tn, C, seg, bucket, kern.lo, kern.hi, wt))

        def rebuild():
            k = layer.table()
            est.piece_coefficients([q for _, q in layer.value_layer.named_parameters()], k)
        t0 = time.perf_counter()
        for _ in range(20):
            rebuild()
        t_table = (time.perf_counter() - t0) / 20 * 1e3

        wt_l = wt.permute(0, 3, 1, 2)

        def layer_step():
            layer.zero_grad(set_to_none=True)
            (wt_l * layer(events)).sum().backward()
        t_layer = median_ms(layer_step)

        def layer_step_cuda():
            layer.zero_grad(set_to_none=True)
            (wt_l * layer(events_dev)).sum().backward()
        t_layer_cuda = median_ms(layer_step_cuda)

        vl = est.ValueLayer(state).to(layer.device)
        rows = batch.events
        x, y, p = (rows[:, j].to(torch.int64) for j in (0, 1, 3))
        b = torch.repeat_interleave(torch.arange(B, device=layer.device), N)
        wt_r = torch.randn(2 * C * H * W * B, device=layer.device)

        def ref_step():
            vl.zero_grad(set_to_none=True)
            reference_statements(vl, x, y, tn, p, b, B, C, H, W, wt_r)
        t_ref = median_ms(ref_step, warm=2)
        lines.append(json.dumps({"dim": [C, H, W], "batch": B, "events_per_item": N, "pieces": len(kern),
                                 "ref_statements_fwd_bwd_ms": round(t_ref, 3), "layer_fwd_bwd_ms": round(t_layer, 3),
                                 "layer_cuda_fwd_bwd_ms": round(t_layer_cuda, 3), "prepare_kernel_ms": round(t_prep, 4),
                                 "copy_40B_per_event_ms": round(t_copy, 4),
                                 "backward_kernel_ms": round(t_bwd, 4), "forward_kernel_ms": round(t_fwd, 4),
                                 "bin_ms": round(t_bin, 4), "table_rebuild_ms": round(t_table, 3)}))
        print(lines[-1], flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
