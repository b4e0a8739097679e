"""The greedy, channel-by-channel representation search -- mirrors representation_search/optimization.py:116-304.

The reference asks Gryffin for ``budget`` (window, function, aggregation) triples per channel, scores each with
``measure_otmi`` (build the stack of the chosen channels plus the candidate, letterbox it, ``otmi`` per window, mean) and
keeps the triple with the smallest C_p.  ``known_constraints_cat`` admits 21 (function, aggregation) pairs, so a channel
has 7 x 21 = 147 admissible triples under "SBN" (8 x 21 = 168 under "SBT"): fewer than the reference's budget of 100
evaluations would need to find the minimum by sampling, so one step here is EXHAUSTIVE and returns the true argmin.
Gryffin is not used.

``score_candidates`` scores every candidate of a step in one batch on the device: the chosen channels are built, resized
and letterboxed once; all candidates are channels of one bank; the candidate clouds come from
``evrep_otmi_rep_clouds_bank`` (no (R, B, S, S, 12) tensor exists); all solves are batched GWD calls in which the
candidates of a window share its event cloud.  ``measure_otmi`` keeps the per-representation route for ONE candidate.

The search is not sharded over ranks: every rank that calls it scores all windows itself.  ``measure_cp_device`` keeps
the role of dealing windows to the ranks of a process group.
"""
import os
import pickle

import numpy as np
import torch

N_CHANNELS = 12

# optimization.py:169-181, in the reference's order
window_options = [i for i in range(7)]   # 7 windows (N, [0, N/3], [N/3, 2N/3], [2N/3, N], N/2, N/4, N/8)
function_options = ["timestamp", "polarity", "count", "timestamp_pos", "timestamp_neg", "count_pos", "count_neg"]
aggregation_options = ["mean", "max", "sum", "variance"]

POSSIBLE_SCENARIOS = {
    "timestamp": ["variance", "mean", "max", "sum"],
    "polarity": ["mean", "variance", "sum"],
    "count": ["mean", "sum"],
    "timestamp_pos": ["variance", "mean", "max", "sum"],
    "timestamp_neg": ["variance", "mean", "max", "sum"],
    "count_pos": ["mean", "sum"],
    "count_neg": ["mean", "sum"],
}


def known_constraints_cat(param):
    """optimization.py:148-165: is the (function, aggregation) pair of ``param`` admissible?"""
    return param["aggregation"] in POSSIBLE_SCENARIOS[param["function"]]


def candidates(stacking="SBN"):
    """The admissible (window, function, aggregation) triples: window-major, then function, then aggregation, each in
    option order.  147 for "SBN" (windows 0..6), 168 for "SBT" (windows 0..7)."""
    if stacking not in ("SBN", "SBT"):
        raise ValueError("stacking_type %r" % (stacking,))
    windows = window_options if stacking == "SBN" else window_options + [7]
    return [(w, f, a) for w in windows for f in function_options for a in aggregation_options
            if known_constraints_cat({"function": f, "aggregation": a})]


_all_candidates = candidates     # (the functions below take the candidate list as a parameter of that name)


def _triple(c):
    if isinstance(c, dict):
        return c["window"], c["function"], c["aggregation"]
    w, f, a = c
    return w, f, a


def _chosen_lists(window_indexes_dict):
    """optimization.py:121-123: the list of {window: [function, aggregation]} -> three lists."""
    ws = [next(iter(i)) for i in window_indexes_dict]
    fs = [i[next(iter(i))][0] for i in window_indexes_dict]
    ags = [i[next(iter(i))][1] for i in window_indexes_dict]
    return ws, fs, ags


def _as_batch(windows, height, width):
    from ... import engine as eng
    if isinstance(windows, eng.EventBatch):
        if (windows.H, windows.W) != (int(height), int(width)):
            raise ValueError("the EventBatch is %d x %d, not %d x %d" % (windows.H, windows.W, height, width))
        return windows
    wins = [np.ascontiguousarray(w, dtype=np.int32).reshape(-1, 4) for w in windows]
    return eng.EventBatch.from_numpy(wins, height, width, device=torch.device("cuda", torch.cuda.current_device()))


def _as_window_list(windows):
    from ... import engine as eng
    if isinstance(windows, eng.EventBatch):
        ev, off = windows.events.cpu().numpy(), windows.offsets_host.numpy()
        return [ev[off[b]:off[b + 1]] for b in range(windows.B)]
    return list(windows)


def score_candidates(windows, window_indexes_dict, height, width, candidates=None, img_size=240, stacking="SBN", h=0.7,
                     max_bytes=None, workspace=None):
    """C_p of "the K chosen channels plus one candidate" for every candidate, on the device.

    windows: a list of raw (n, 4) integer arrays [x, y, t, p], or an engine.EventBatch.  window_indexes_dict: the
    reference's list of {window: [function, aggregation]} for the K < 12 channels chosen so far.  candidates: triples
    (or dicts with "window", "function", "aggregation"); None: ``candidates(stacking)``.
    Returns (C_p (R,), scores (R, B), quadrant costs (R, B, 3)), float64 device tensors; nothing is read back.

    Candidates are processed in chunks so that a chunk's bank (raw, gathered and letterboxed), its clouds and its GWD
    scratch stay under ``max_bytes``; None: HALF of the device memory that is free when the call starts.  A chunk
    also keeps items = chunk * B and the 3 * items solves within 65535."""
    from ... import _lib, engine as eng
    from ...gwd_pipeline import rep_for_gwd_batch
    K = len(window_indexes_dict)
    if K >= N_CHANNELS:
        raise ValueError("all %d channels are chosen" % N_CHANNELS)
    cands = [_triple(c) for c in (_all_candidates(stacking) if candidates is None else candidates)]
    if not cands:
        raise ValueError("no candidates")
    batch = _as_batch(windows, height, width)
    dev, B = batch.device, batch.B
    ws = workspace or eng._default_workspace(dev)
    pad = [None] * (N_CHANNELS - K)                                           # optimization.py:48-52
    cw, cf, ca = _chosen_lists(window_indexes_dict)
    with torch.cuda.device(dev):
        base = rep_for_gwd_batch(batch.mdes(cw + pad, cf + pad, ca + pad, scale=1.0, dtype=torch.float64, stacking=stacking), img_size)
        Xs, n, quad = eng.otmi_event_clouds(batch.events, batch.offsets_host, height, width, workspace=ws)
        cap, S, D = int(Xs.shape[2]), int(base.shape[1]), N_CHANNELS + 2
        m_cap = (S - (S // 2 - 1)) ** 2
        if max_bytes is None:
            max_bytes = torch.cuda.mem_get_info(dev)[0] // 2
        per_cand = (B * 8 * (2 * batch.H * batch.W + S * S) + B * 3 * m_cap * D * 8
                    + _lib.api().evrep_gwd_batch_scratch_bytes(3 * B, 4, D, cap, m_cap))
        chunk = max(1, min(len(cands), int(max_bytes) // per_cand, 65535 // (3 * B)))
        slot = torch.arange(B * 3, device=dev, dtype=torch.int64)             # pair -> its window's (b, k) event cloud
        q = torch.empty((len(cands), B, 3), dtype=torch.float64, device=dev)
        for c0 in range(0, len(cands), chunk):
            part = cands[c0:c0 + chunk]
            R = len(part)
            bank = rep_for_gwd_batch(batch.mdes([c[0] for c in part], [c[1] for c in part], [c[2] for c in part], scale=1.0,
                                                dtype=torch.float64, stacking=stacking), img_size)
            Xt, m, m_cap = eng.otmi_rep_clouds_bank(base, bank, K, range(R), quad, B, workspace=ws)
            P = R * B * 3
            pair = slot.repeat(R)
            eng.gwd_padded_l1_batch(Xs.view(-1, 4), n.view(-1)[pair].contiguous(), Xt.view(-1, D), m.view(-1), cap, m_cap,
                                    xs_row=(pair * cap).contiguous(), xt_row=torch.arange(P, device=dev, dtype=torch.int64) * m_cap,
                                    h=h, out=q[c0:c0 + R].view(-1), workspace=ws)
        scores = q.mean(dim=2)                                                # as measure_cp_device: quadrants, then windows
        return scores.mean(dim=1), scores, q


def measure_otmi(param, windows, window_indexes_dict, height, width, img_size=240, stacking="SBN", h=0.7, workspace=None):
    """optimization.py:116-145 for ONE candidate ``param`` ({"window", "function", "aggregation"}): the stack of the chosen
    channels plus the candidate, through the per-representation route (measure_cp_device with one mdes builder).
    Sets param["C_p"] and returns param."""
    from ...gwd_pipeline import measure_cp_device
    cw, cf, ca = _chosen_lists(window_indexes_dict)
    cw, cf, ca = cw + [param["window"]], cf + [param["function"]], ca + [param["aggregation"]]
    pad = [None] * (N_CHANNELS - len(cw))
    build = lambda b: b.mdes(cw + pad, cf + pad, ca + pad, scale=1.0, dtype=torch.float64, stacking=stacking)
    res = measure_cp_device(_as_window_list(windows), {"candidate": build}, height, width, img_size=img_size, h=h, workspace=workspace)
    param["C_p"] = float(res["candidate"][0])
    return param


def sequential_optimization(windows, budget, WINDOW_INDEXES_DICT, height=None, width=None, candidates=None, img_size=240,
                            stacking="SBN", h=0.7, max_bytes=None, workspace=None):
    """One channel of the search (optimization.py:168-265) as ONE exhaustive step over the admissible candidates.
    ``budget`` is accepted for the reference's signature and ignored: every candidate is scored.  height / width may be
    omitted when ``windows`` is an EventBatch.  Returns (best_observation, WINDOW_INDEXES_DICT): the observation is the
    reference's dict {"window", "function", "aggregation", "C_p"}, and {window: [function, aggregation]} is appended to the
    list.  The first minimum in candidate order wins, like ``C_ps.index(min(C_ps))``; a NaN score never wins; all NaN
    raises ValueError.  The C_p vector is the step's single host read."""
    if (height is None or width is None) and hasattr(windows, "H"):
        height, width = windows.H, windows.W
    cands = [_triple(c) for c in (_all_candidates(stacking) if candidates is None else candidates)]
    C_p = score_candidates(windows, WINDOW_INDEXES_DICT, height, width, candidates=cands, img_size=img_size, stacking=stacking,
                           h=h, max_bytes=max_bytes, workspace=workspace)[0]
    C_ps = np.asarray(C_p.detach().cpu().numpy() if isinstance(C_p, torch.Tensor) else C_p, dtype=np.float64).reshape(-1)
    if C_ps.shape[0] != len(cands):
        raise ValueError("%d scores for %d candidates" % (C_ps.shape[0], len(cands)))
    valid = np.flatnonzero(~np.isnan(C_ps))
    if valid.size == 0:
        raise ValueError("every candidate's C_p is NaN")
    best = int(valid[np.argmin(C_ps[valid])])                                 # the first of equal minima (inf may win, NaN never)
    w, f, a = cands[best]
    best_observation = {"window": w, "function": f, "aggregation": a, "C_p": float(C_ps[best])}
    WINDOW_INDEXES_DICT.append({w: [f, a]})
    return best_observation, WINDOW_INDEXES_DICT


def run_optimization(windows, number_of_channels, budget=None, SAVE_PATH=None, height=None, width=None, **options):
    """optimization.py:268-287: ``number_of_channels`` steps, each on top of the channels chosen before it (a triple already
    chosen stays a candidate, as in the reference).  Returns (best_observations, WINDOW_INDEXES_DICT); with SAVE_PATH it
    also writes the reference's best_observations.pkl and windows_indexes.pkl there.  ``options`` go to
    sequential_optimization.  (Raw windows are uploaded and binned once per step; pass an EventBatch to do it once.)"""
    WINDOW_INDEXES_DICT = []
    best_observations = []
    for _ in range(number_of_channels):
        best_observation, WINDOW_INDEXES_DICT = sequential_optimization(windows, budget, WINDOW_INDEXES_DICT, height=height,
                                                                        width=width, **options)
        best_observations.append(best_observation)
    if SAVE_PATH is not None:
        with open(os.path.join(SAVE_PATH, "best_observations.pkl"), "wb") as f:
            pickle.dump(best_observations, f)
        with open(os.path.join(SAVE_PATH, "windows_indexes.pkl"), "wb") as f:
            pickle.dump(WINDOW_INDEXES_DICT, f)
    return best_observations, WINDOW_INDEXES_DICT
