#!/usr/bin/env python3
"""Times of one exhaustive step of the representation search (representations/representation_search/optimization.py) beside the
per-candidate route it replaces.

    python tools/bench_search.py [--reps 5] [--events 50000] [--out FILE.json]

Gen1 304 x 240, windows of `events` events (edge-cluster model), img_size 240, B = 2 windows (the reference's chosen[:2]) and
B = 8, K = 0, 5 and 11 channels chosen (the first K ERGO-12 triples), all 147 "SBN" candidates.  Per (B, K), median ms over
`reps` runs after one warm-up run:
  (a) per_candidate   measure_cp_device with one mdes builder per candidate (a host clock around a synchronise);
  (b) score           optimization.score_candidates (a host clock around a synchronise);
  (c) gwd             the gwd_padded_l1_batch call of (b) alone, on the clouds (b) leaves (HIP events);
  (d) bank_clouds     evrep_otmi_rep_clouds_bank alone, beside evrep_otmi_rep_clouds on the materialised items and the
                      materialisation itself (HIP events), with the bytes each reads and writes.
The tool checks that (a) and (b) give the same C_p vector.  One JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from event_representation_study_amd import engine as eng  # noqa: E402
from event_representation_study_amd.gwd_pipeline import measure_cp_device, rep_for_gwd_batch  # noqa: E402
from event_representation_study_amd.representations.representation_search import optimization as opt  # noqa: E402
from event_representation_study_amd.synthetic import make_events_edges  # noqa: E402

H, W, S = 240, 304, 240
ERGO12 = list(zip([0, 3, 2, 6, 5, 6, 2, 5, 1, 0, 4, 1],
                  ["polarity", "timestamp_neg", "count_neg", "polarity", "count_pos", "count",
                   "timestamp_pos", "count_neg", "timestamp_neg", "timestamp_pos", "timestamp", "count"],
                  ["variance", "variance", "mean", "sum", "mean", "sum", "mean", "mean", "max", "max", "max", "mean"]))


def median_event_ms(launch, reps, warmup=1):
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
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def median_host_ms(run, reps, warmup=1):
    for _ in range(warmup):
        run()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--events", type=int, default=50000)
    ap.add_argument("--windows", type=int, nargs="*", default=[2, 8])
    ap.add_argument("--chosen", type=int, nargs="*", default=[0, 5, 11])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_search.py needs a HIP device"
    cands = opt.candidates()
    R, D = len(cands), opt.N_CHANNELS + 2
    result = dict(bench="search", events_per_window=args.events, reps=args.reps, candidates=R, sensor=[H, W], img_size=S, rows=[])
    for B in args.windows:
        wins = [make_events_edges(args.events, W, H, seed=300 + b) for b in range(B)]
        batch = eng.EventBatch.from_numpy(wins, H, W)
        ws = eng.GwdWorkspace()
        for K in args.chosen:
            chosen = [{w: [f, a]} for w, f, a in ERGO12[:K]]
            cw, cf, ca = [t[0] for t in ERGO12[:K]], [t[1] for t in ERGO12[:K]], [t[2] for t in ERGO12[:K]]
            pad = [None] * (opt.N_CHANNELS - K - 1)

            def builder(c):
                return lambda b: b.mdes(cw + [c[0]] + pad, cf + [c[1]] + pad, ca + [c[2]] + pad, scale=1.0)
            builders = {j: builder(c) for j, c in enumerate(cands)}
            row = dict(windows=B, chosen=K)
            ref = measure_cp_device(wins, builders, H, W, img_size=S, workspace=ws)
            C_p = opt.score_candidates(batch, chosen, H, W, img_size=S, workspace=ws)[0].cpu().numpy()
            row["same_C_p"] = bool(np.array_equal(C_p, np.array([ref[j][0] for j in range(R)])))
            row["per_candidate_ms"] = round(median_host_ms(lambda: measure_cp_device(wins, builders, H, W, img_size=S, workspace=ws), args.reps), 2)
            row["score_ms"] = round(median_host_ms(lambda: opt.score_candidates(batch, chosen, H, W, img_size=S, workspace=ws), args.reps), 2)
            # the pieces of (b), on its own tensors
            base = rep_for_gwd_batch(batch.mdes(cw + [None] + pad, cf + [None] + pad, ca + [None] + pad, scale=1.0), S)
            bank = rep_for_gwd_batch(batch.mdes([c[0] for c in cands], [c[1] for c in cands], [c[2] for c in cands], scale=1.0), S)
            Xs, n, quad = eng.otmi_event_clouds(batch.events, batch.offsets_host, H, W, workspace=ws)
            cap = int(Xs.shape[2])
            Xt, m, m_cap = eng.otmi_rep_clouds_bank(base, bank, K, range(R), quad, B, workspace=ws)
            P = R * B * 3
            pair = torch.arange(B * 3, device="cuda", dtype=torch.int64).repeat(R)
            n_p, xs_row = n.view(-1)[pair].contiguous(), (pair * cap).contiguous()
            xt_row = torch.arange(P, device="cuda", dtype=torch.int64) * m_cap
            costs = torch.empty(P, dtype=torch.float64, device="cuda")
            row["gwd_ms"] = round(median_event_ms(lambda: eng.gwd_padded_l1_batch(
                Xs.view(-1, 4), n_p, Xt.view(-1, D), m.view(-1), cap, m_cap, xs_row=xs_row, xt_row=xt_row, out=costs, workspace=ws), args.reps), 2)
            row["pairs"] = P
            row["bank_clouds_ms"] = round(median_event_ms(lambda: eng.otmi_rep_clouds_bank(base, bank, K, range(R), quad, B, workspace=ws),
                                                          args.reps, warmup=2), 3)
            kept = int(m.sum().item())
            px = B * S * S * 8
            groups = (R + 15) // 16
            # both launches read a quadrant's base pixels once per group of 16 candidates and each candidate value once
            # (3 of 4 quadrants, up to the shared middle row and column); the rows leave once
            row["bank_clouds_bytes_read"] = int(2 * 0.75 * px * (groups * opt.N_CHANNELS + R))
            row["bank_clouds_bytes_written"] = kept * D * 8

            def materialise():
                items = base[None].repeat(R, 1, 1, 1, 1)
                items[..., K] = bank.permute(3, 0, 1, 2)
                return items.view(R * B, S, S, opt.N_CHANNELS)
            ws2 = eng.GwdWorkspace()
            row["materialise_ms"] = round(median_event_ms(materialise, args.reps), 3)
            items = materialise()
            row["materialised_clouds_ms"] = round(median_event_ms(lambda: eng.otmi_rep_clouds(items, quad, B, workspace=ws2), args.reps, warmup=2), 3)
            row["materialised_bytes_read"] = int(2 * 0.75 * px * R * opt.N_CHANNELS)
            row["materialised_bytes_written"] = kept * D * 8
            row["materialise_bytes"] = int(px * opt.N_CHANNELS * (1 + 2 * R) + px * R * 2)
            Xr, mr, _ = eng.otmi_rep_clouds(items, quad, B, workspace=ws2)
            row["same_clouds"] = bool(torch.equal(m, mr))
            del items, Xr, mr, ws2, base, bank
            torch.cuda.empty_cache()
            print(json.dumps(row), file=sys.stderr, flush=True)
            result["rows"].append(row)
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
