"""GPU: one step of the representation search on the device.

* evrep_otmi_rep_clouds_bank against evrep_otmi_rep_clouds of the materialised items, bit for bit; the same call on guarded
  regions of exactly the stated sizes.
* optimization.score_candidates against the per-candidate route (one mdes builder per candidate through measure_cp_device and
  its own calls), against measure_cp_device's ERGO-12, and against the reference's recorded stacks and costs
  (tests/golden/search_step.npz, made by tests/golden/make_golden_search.py).
* sequential_optimization / measure_otmi on top of it.
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden
from guarded import Arena

pytestmark = pytest.mark.gpu

ERGO12 = ([0, 3, 2, 6, 5, 6, 2, 5, 1, 0, 4, 1],
          ["polarity", "timestamp_neg", "count_neg", "polarity", "count_pos", "count",
           "timestamp_pos", "count_neg", "timestamp_neg", "timestamp_pos", "timestamp", "count"],
          ["variance", "variance", "mean", "sum", "mean", "sum", "mean", "mean", "max", "max", "max", "mean"])
CHOSEN11 = [{w: [f, a]} for w, f, a in zip(*ERGO12)][:11]


def _bits(t):
    return t.contiguous().view(torch.int64)


def _windows(height, width, sizes=(1500, 2300, 3000), seed=70):
    from event_representation_study_amd.synthetic import make_events
    wins = [make_events(n, width, height, seed=seed + b) for b, n in enumerate(sizes)]
    rng = np.random.default_rng(seed)
    k = sizes[1] // 3                      # window 1 skewed: a third of its events gathered in the bottom-right quadrant
    idx = rng.choice(sizes[1], k, replace=False)
    wins[1][idx, 0] = rng.integers(width // 2, width, k)
    wins[1][idx, 1] = rng.integers(height // 2, height, k)
    return wins


# ---------------------------------------------------------------------------------------------------------------- the entry
def _bank_case(S, C, slot, dtype, seed=5, B=3, R=21):
    """base / bank / cand / quad of the entry's test: letterbox rows of 114, about 70 % all-zero pixels, pixels where only the
    base and pixels where only the candidate is non-zero, one candidate zero inside the image, NaN in one candidate, in a base
    channel and in the base's `slot` channel (which is replaced, so it must not count)."""
    from event_representation_study_amd import engine as eng
    rng = np.random.default_rng(seed)
    pad = 6
    base = rng.random((B, S, S, C)) * (rng.random((B, S, S, 1)) < 0.2)
    base[..., slot] = 0.0                                               # not chosen yet: zeros inside the image
    bank = rng.random((B, S, S, R)) * (rng.random((B, S, S, R)) < 0.12)
    bank[..., 7] = 0.0                                                  # a candidate that is zero everywhere inside the image
    bank[0, 10, 11, 3] = bank[1, S - 9, 8, 3] = bank[2, S // 2 - 1, S // 2 - 1, 3] = np.nan
    base[1, 20, 30, (slot + 1) % C] = np.nan
    base[2, 12, 13, slot] = np.nan
    base[:, :pad] = base[:, S - pad:] = 114.0
    bank[:, :pad] = bank[:, S - pad:] = 114.0
    inside = np.zeros((B, S, S), bool)
    inside[:, pad:S - pad] = True
    only_base = inside & (np.nan_to_num(base) != 0).any(-1) & (np.nan_to_num(bank) == 0).all(-1)
    only_cand = inside & (base == 0).all(-1) & (np.nan_to_num(bank[..., 0]) != 0)
    zero = (base == 0).all(-1) & (bank[..., 0] == 0)                    # per item: the base and ONE candidate
    assert only_base.any() and only_cand.any() and 0.6 < zero[:, pad:S - pad].mean() < 0.8
    perm = rng.permutation(R)
    cand = [int(v) for v in np.concatenate([perm[:9], perm[4:5], perm[9:], perm[4:5]])]   # 23 entries, perm[4] three times
    assert len(cand) == 23 and sorted(set(cand)) == list(range(R))
    wins = _windows(36, 48)
    batch = eng.EventBatch.from_numpy(wins, 36, 48)
    _, _, quad = eng.otmi_event_clouds(batch.events, batch.offsets_host, 36, 48, workspace=eng.GwdWorkspace())
    quad = quad.clone()
    q = quad.cpu().numpy()
    assert not np.array_equal(q[0], q[1])                               # the skewed window skips another quadrant
    base_t, bank_t = torch.from_numpy(base).to("cuda", dtype), torch.from_numpy(bank).to("cuda", dtype)
    items = base_t[None].repeat(len(cand), 1, 1, 1, 1)                  # (n_cand, B, S, S, C): item j * B + b
    items[..., slot] = bank_t[..., cand].permute(3, 0, 1, 2)
    return base_t, bank_t, cand, quad, items.reshape(len(cand) * B, S, S, C).contiguous()


BANK_CASES = [(48, 12, 0, torch.float64), (48, 12, 5, torch.float64), (47, 12, 11, torch.float64), (48, 5, 4, torch.float64),
              (47, 12, 5, torch.float32), (48, 5, 4, torch.float32), (47, 12, 0, torch.float32), (48, 12, 11, torch.float32)]


@pytest.mark.parametrize("S,C,slot,dtype", BANK_CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_bank_clouds_equal_the_materialised_items(S, C, slot, dtype):
    from event_representation_study_amd import engine as eng
    base, bank, cand, quad, items = _bank_case(S, C, slot, dtype)
    B = int(base.shape[0])
    Xr, mr, cap_r = eng.otmi_rep_clouds(items, quad, B, workspace=eng.GwdWorkspace())
    ws = eng.GwdWorkspace()
    m_cap = (S - (S // 2 - 1)) ** 2
    ws.typed("otmi_xt", (len(cand) * B, 3, m_cap, C + 2), torch.float64).view(torch.int64).fill_(-7)    # rows behind m stay as they are
    Xt, m, cap = eng.otmi_rep_clouds_bank(base, bank, slot, cand, quad, B, workspace=ws)
    assert cap == cap_r == m_cap and Xt.shape == Xr.shape == (len(cand) * B, 3, m_cap, C + 2) and m.dtype == torch.int64
    assert torch.equal(m, mr)
    assert int(m.min()) > 0 and int(m.max()) < m_cap                    # something is kept everywhere, something dropped everywhere
    row = torch.arange(m_cap, device="cuda")[None, None, :] < m[:, :, None]
    assert torch.equal(_bits(Xt)[row], _bits(Xr)[row])
    assert bool((_bits(Xt)[~row] == -7).all())
    j = [i for i, c in enumerate(cand) if c == cand[9]]                 # the repeated candidate: the same cloud three times
    assert len(j) == 3
    first = slice(j[0] * B, (j[0] + 1) * B)
    for other in j[1:]:
        again = slice(other * B, (other + 1) * B)
        assert torch.equal(m[first], m[again]) and torch.equal(_bits(Xt[first])[row[first]], _bits(Xt[again])[row[first]])
    assert not torch.isnan(Xt[row]).any()


@pytest.mark.parametrize("S,C,slot,dtype", [(47, 12, 5, torch.float64), (48, 5, 4, torch.float32)], ids=lambda v: str(v).replace("torch.", ""))
def test_bank_clouds_in_guarded_regions(S, C, slot, dtype):
    """Every region exactly as long as include/evrep.h states, under two fills: guards and inputs intact, rows from m_out on
    untouched, results bit-equal across the fills (no read of scratch or output that the call did not write)."""
    from event_representation_study_amd import _lib
    lib = _lib.load()
    base, bank, cand, quad, _ = _bank_case(S, C, slot, dtype, seed=9)
    B, R, items = int(base.shape[0]), int(bank.shape[3]), len(cand) * int(base.shape[0])
    m_cap = (S - (S // 2 - 1)) ** 2
    nscratch = int(lib.evrep_otmi_scratch_bytes(items))
    got = []
    for k, fill in enumerate(("ones", "random")):
        arena = Arena("cuda:0", seed=20 + k)
        gb, gk, gq = arena.carve_like(base, "base"), arena.carve_like(bank, "bank"), arena.carve_like(quad, "quad")
        Xt = arena.carve_shape((items, 3, m_cap, C + 2), torch.float64, fill, "Xt")
        m = arena.carve_shape((items, 3), torch.int64, fill, "m_out")
        sc = arena.carve(nscratch, 256, fill, "scratch")
        before = Xt.clone()
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        rc = lib.evrep_otmi_rep_clouds_bank(p(gb), p(gk), {torch.float64: _lib.F64, torch.float32: _lib.F32}[dtype], B, S, C, R, slot,
                                            _lib.int32_array(cand), len(cand), p(gq), m_cap, p(Xt), p(m), p(sc),
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
        torch.cuda.synchronize()
        arena.check()
        arena.check_inputs()
        assert int(m.min()) > 0 and int(m.max()) < m_cap
        row = torch.arange(m_cap, device="cuda")[None, None, :] < m[:, :, None]
        assert torch.equal(_bits(Xt)[~row], _bits(before)[~row])
        got.append((m.clone(), _bits(Xt)[row].clone()))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])


# ---------------------------------------------------------------------------------------------------------------- the step
SENSORS = {"36x48@48": (36, 48, 48), "30x40@24": (30, 40, 24)}
CHOSEN = {0: [], 3: CHOSEN11[:3], 11: CHOSEN11}
_CACHE = {}


def _opt():
    from event_representation_study_amd.representations.representation_search import optimization
    return optimization


def _step(sensor, K, stacking="SBN", cands=None):
    """score_candidates of all candidates (computed once per case, results cloned)."""
    key = (sensor, K, stacking, None if cands is None else tuple(cands))
    if key not in _CACHE:
        H, W, S = SENSORS[sensor]
        wins = _windows(H, W)
        res = _opt().score_candidates(wins, CHOSEN[K], H, W, candidates=cands, img_size=S, stacking=stacking)
        _CACHE[key] = (wins, tuple(t.clone() for t in res))
    return _CACHE[key]


def _per_candidate(wins, chosen, cands, H, W, S, stacking):
    """The per-representation route, candidate by candidate: measure_cp_device with one mdes builder each (C_p, scores), and the
    same calls made here for the quadrant costs, which measure_cp_device does not return."""
    from event_representation_study_amd import engine as eng
    from event_representation_study_amd.gwd_pipeline import measure_cp_device, rep_for_gwd_batch
    cw, cf, ca = [next(iter(d)) for d in chosen], [d[next(iter(d))][0] for d in chosen], [d[next(iter(d))][1] for d in chosen]
    pad = [None] * (12 - len(chosen) - 1)

    def builder(c):
        return lambda b: b.mdes(cw + [c[0]] + pad, cf + [c[1]] + pad, ca + [c[2]] + pad, scale=1.0, stacking=stacking)
    res = measure_cp_device(wins, {j: builder(c) for j, c in enumerate(cands)}, H, W, img_size=S, workspace=eng.GwdWorkspace())
    ws = eng.GwdWorkspace()
    batch = eng.EventBatch.from_numpy(wins, H, W)
    Xs, n, quad = eng.otmi_event_clouds(batch.events, batch.offsets_host, H, W, workspace=ws)
    cap, B = int(Xs.shape[2]), len(wins)
    P = 3 * B
    q = torch.empty((len(cands), B, 3), dtype=torch.float64, device="cuda")
    for j, c in enumerate(cands):
        Xt, m, m_cap = eng.otmi_rep_clouds(rep_for_gwd_batch(builder(c)(batch), S), quad, B, workspace=ws)
        eng.gwd_padded_l1_batch(Xs.view(-1, 4), n.view(-1), Xt.view(-1, int(Xt.shape[-1])), m.view(-1), cap, m_cap,
                                xs_row=torch.arange(P, device="cuda", dtype=torch.int64) * cap,
                                xt_row=torch.arange(P, device="cuda", dtype=torch.int64) * m_cap, out=q[j].view(-1), workspace=ws)
    C_p = torch.tensor([res[j][0] for j in range(len(cands))], dtype=torch.float64)
    scores = torch.stack([res[j][1] for j in range(len(cands))]).cpu()
    return C_p, scores, q


@pytest.mark.parametrize("K", [0, 3, 11])
@pytest.mark.parametrize("sensor", list(SENSORS))
def test_score_candidates_equals_the_per_candidate_route(sensor, K):
    H, W, S = SENSORS[sensor]
    cands = _opt().candidates()
    wins, (C_p, scores, q) = _step(sensor, K)
    assert q.shape == (147, 3, 3) and scores.shape == (147, 3) and C_p.shape == (147,) and q.is_cuda and q.dtype == torch.float64
    rC, rs, rq = _per_candidate(wins, CHOSEN[K], cands, H, W, S, "SBN")
    assert torch.isfinite(rq).all() and len(torch.unique(rq)) > 147
    assert torch.equal(_bits(q), _bits(rq))
    assert torch.equal(scores.cpu(), rs) and torch.equal(C_p.cpu(), rC)


def test_score_candidates_sbt_sample_with_window_7():
    H, W, S = SENSORS["36x48@48"]
    sbt = _opt().candidates("SBT")
    cands = sbt[::7]                                                    # 24 candidates over all eight windows
    assert len(cands) == 24 and sum(c[0] == 7 for c in cands) >= 3
    wins, (C_p, scores, q) = _step("36x48@48", 3, "SBT", cands)
    rC, rs, rq = _per_candidate(wins, CHOSEN[3], cands, H, W, S, "SBT")
    assert torch.equal(_bits(q), _bits(rq)) and torch.equal(scores.cpu(), rs) and torch.equal(C_p.cpu(), rC)
    _, (_, _, q_sbn) = _step("36x48@48", 3)
    assert not torch.equal(q[:3], q_sbn[:3])                            # SBT cuts its windows by time: other channels


@pytest.mark.parametrize("max_bytes", [1, 12 << 20])
def test_chunked_run_is_bit_equal(max_bytes):
    H, W, S = SENSORS["30x40@24"]
    wins, (C_p, scores, q) = _step("30x40@24", 3)
    sample = list(range(0, 147, 5))                                     # 30 candidates: 30 chunks of one, or a few chunks
    cands = [_opt().candidates()[i] for i in sample]
    c2, s2, q2 = _opt().score_candidates(wins, CHOSEN[3], H, W, candidates=cands, img_size=S, max_bytes=max_bytes)
    assert torch.equal(_bits(q2), _bits(q[sample])) and torch.equal(s2, scores[sample]) and torch.equal(c2, C_p[sample])


def test_twelfth_ergo_channel_equals_the_ergo12_builder():
    from event_representation_study_amd.gwd_pipeline import measure_cp_device
    H, W, S = SENSORS["30x40@24"]
    wins = _windows(H, W)
    twelfth = (ERGO12[0][11], ERGO12[1][11], ERGO12[2][11])
    C_p, scores, q = _opt().score_candidates(wins, CHOSEN11, H, W, candidates=[twelfth], img_size=S)
    ref = measure_cp_device(wins, {"ergo": lambda b: b.optimized()}, H, W, img_size=S)["ergo"]
    assert C_p.shape == (1,) and float(C_p[0].item()) == ref[0] and torch.equal(scores[0].cpu(), ref[1].cpu())


def test_against_the_references_stacks_and_costs():
    from event_representation_study_amd import engine as eng
    g = load_golden("search_step")
    H, W, S = int(g["height"]), int(g["width"]), int(g["img_size"])
    wins = [g["events_0"], g["events_1"]]
    chosen = [{int(w): [str(f), str(a)]} for w, f, a in zip(g["chosen_windows"], g["chosen_functions"], g["chosen_aggregations"])]
    cands = [(int(w), str(f), str(a)) for w, f, a in zip(g["cand_windows"], g["cand_functions"], g["cand_aggregations"])]
    assert len(chosen) == 3 and len(cands) == 8 and g["costs"].shape == (8, 2)
    batch = eng.EventBatch.from_numpy(wins, H, W)
    for i, j in enumerate(g["stacks_of"]):
        triples = [(next(iter(d)), d[next(iter(d))][0], d[next(iter(d))][1]) for d in chosen] + [cands[int(j)]]
        pad = [None] * (12 - len(triples))
        rep = batch.mdes([t[0] for t in triples] + pad, [t[1] for t in triples] + pad, [t[2] for t in triples] + pad, scale=1.0)
        assert g["stacks"][i].shape == (2, H, W, 12) and np.abs(g["stacks"][i][..., :4]).sum() > 0 and not g["stacks"][i][..., 4:].any()
        assert np.array_equal(rep.cpu().numpy().view(np.int64), g["stacks"][i].view(np.int64))
    C_p, scores, q = _opt().score_candidates(wins, chosen, H, W, candidates=cands, img_size=S)
    got = scores.cpu().numpy()
    for j in range(8):
        for b in range(2):
            print("candidate %d window %d: %.12g (reference %.12g, relative %.3g)"
                  % (j, b, got[j, b], g["costs"][j, b], abs(got[j, b] - g["costs"][j, b]) / abs(g["costs"][j, b])))
    assert np.all(np.abs(got - g["costs"]) <= 1e-5 * np.abs(g["costs"]))
    assert np.all(np.abs(C_p.cpu().numpy() - g["costs"].mean(1)) <= 1e-5 * g["costs"].mean(1))


def test_step_returns_the_argmin_and_measure_otmi_reproduces_it():
    opt = _opt()
    H, W, S = SENSORS["36x48@48"]
    wins, (C_p, scores, q) = _step("36x48@48", 3)
    chosen = list(CHOSEN[3])
    best, out = opt.sequential_optimization(wins, 100, chosen, height=H, width=W, img_size=S)
    vals = C_p.cpu().numpy()
    j = int(np.argmin(vals))
    assert out is chosen and len(chosen) == 4
    assert (best["window"], best["function"], best["aggregation"]) == opt.candidates()[j] and best["C_p"] == float(vals[j])
    assert chosen[3] == {best["window"]: [best["function"], best["aggregation"]]}
    one = opt.measure_otmi({"window": best["window"], "function": best["function"], "aggregation": best["aggregation"]},
                           wins, CHOSEN[3], H, W, img_size=S)
    assert one["C_p"] == best["C_p"] and set(one) == {"window", "function", "aggregation", "C_p"}
