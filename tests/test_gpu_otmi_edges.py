"""GPU: the kernels that build the point clouds of the OTMI harness (k_otmi_ev_stats / _plan / _rows, k_otmi_rep,
k_otmi_rep_bank) against the per-quadrant numpy restatement tests/otmi_ref.py, which tests/test_otmi_ref_cpu.py pins to the
oracle, at the edges listed in tests/otmi_edge_cases.py.

The rule everywhere: n, m and quad are equal; rows [0, n) equal the restatement widened to float64 BIT FOR BIT, infinities and
-0.0 included; NaN sits in the same cells (its bits are not compared: numpy's float32 0 / 0 is the negative quiet NaN, the
device's the positive one).  Bit equality is the right bar: every operand is an integer that the documented float32
rounding represents exactly, and each value is one correctly rounded float32 division or a copy.
"""
import numpy as np
import pytest
import torch

import otmi_edge_cases as cases
from otmi_ref import event_cloud, rep_cloud, same_cloud, scored_quadrants

pytestmark = pytest.mark.gpu

FILL = -7                         # int64 pattern behind the rows a call may write


def _bits(t):
    return t.contiguous().view(torch.int64)


def _assert_same(got, want, what):
    diff = same_cloud(got, want)
    assert diff is None, "%s: %s" % (what, diff)


# ------------------------------------------------------------------------------------------------------------- events
@pytest.mark.parametrize("H,W", cases.SENSORS, ids=lambda v: str(v))
def test_event_clouds_at_the_edges(H, W):
    """One batched call per sensor with every listed window in it, offsets on the device."""
    from event_representation_study_amd import engine as eng
    wins = cases.event_windows(H, W)
    B = len(wins)
    offs = np.zeros(B + 1, dtype=np.int64)
    np.cumsum([len(ev) for _, ev, _ in wins], out=offs[1:])
    cap = int(np.diff(offs).max())
    dev = torch.device("cuda:0")
    events = torch.from_numpy(np.concatenate([ev for _, ev, _ in wins])).to(dev)
    ws = eng.GwdWorkspace()
    ws.typed("otmi_xs", (B, 3, cap, 4), torch.float64).view(torch.int64).fill_(FILL)
    Xs, n, quad = eng.otmi_event_clouds(events, torch.from_numpy(offs).to(dev), H, W, workspace=ws)
    assert Xs.shape == (B, 3, cap, 4) and n.shape == (B, 3) and quad.shape == (B, 3)
    Xs, n, quad = Xs.cpu().numpy(), n.cpu().numpy(), quad.cpu().numpy()
    skipped, vacant_slots = set(), 0
    for b, (name, ev, vacant) in enumerate(wins):
        what = "%dx%d window %d (%s)" % (H, W, b, name)
        want_quads = scored_quadrants(ev, H, W)
        assert quad[b].tolist() == want_quads, what
        skipped.add(({0, 1, 2, 3} - set(want_quads)).pop())
        clouds = [event_cloud(ev, q, H, W) for q in want_quads]
        assert vacant == (any(c is None for c in clouds) or event_cloud(ev, 6 - sum(want_quads), H, W) is None), what
        for k, cloud in enumerate(clouds):
            if cloud is None:                   # a vacant scored quadrant: no rows, the slot left alone
                vacant_slots += 1
                assert n[b, k] == 0, what
                assert (Xs[b, k].view(np.int64) == FILL).all(), what
                continue
            assert n[b, k] == len(cloud), "%s slot %d: n = %d, restatement %d" % (what, k, n[b, k], len(cloud))
            _assert_same(Xs[b, k, : len(cloud)], cloud.astype(np.float64), "%s slot %d (quadrant %d)" % (what, k, want_quads[k]))
            if min(H, W) == 2:
                assert len(cloud) == 0, what    # (W - 1) // 2 = 0: no row survives the mask, nothing is divided
    assert skipped == {0, 1, 2, 3}
    if min(H, W) > 2:
        cases.assert_specials_occur(wins, H, W)    # on the restatement: NaN, +inf and -inf are really in the list
    assert vacant_slots == 3 + 1 + 2 + 3        # empty; vacant_q3; vacant_q0_q2; vacant_all_but_q1 (quadrant 1 is the skipped one in the last three)


# --------------------------------------------------------------------------------------------------- representations
@pytest.mark.parametrize("S,C,dtype", cases.REP_CASES, ids=lambda v: str(v))
def test_rep_clouds_at_the_edges(S, C, dtype):
    """A hand-made quadrant table (every quadrant at every slot position, four windows with four tables), items = 2 * B."""
    from event_representation_study_amd import engine as eng
    items, _ = cases.rep_items(S, C, dtype)
    B = cases.REP_QUAD.shape[0]
    assert items.shape[0] == 2 * B
    for k in range(3):
        assert set(cases.REP_QUAD[:, k].tolist()) == {0, 1, 2, 3}
    dev = torch.device("cuda:0")
    m_cap = (S - (S // 2 - 1)) ** 2
    ws = eng.GwdWorkspace()
    ws.typed("otmi_xt", (2 * B, 3, m_cap, C + 2), torch.float64).view(torch.int64).fill_(FILL)
    Xt, m, cap = eng.otmi_rep_clouds(torch.from_numpy(items).to(dev), torch.from_numpy(cases.REP_QUAD).to(dev), B, workspace=ws)
    assert cap == m_cap and Xt.shape == (2 * B, 3, m_cap, C + 2)
    Xt, m = Xt.cpu().numpy(), m.cpu().numpy()
    full_br = False
    for i in range(2 * B):
        for k in range(3):
            q = int(cases.REP_QUAD[i % B, k])
            want = rep_cloud(items[i], q)
            what = "S=%d C=%d %s item %d slot %d (quadrant %d)" % (S, C, dtype, i, k, q)
            assert m[i, k] == len(want), "%s: m = %d, restatement %d" % (what, m[i, k], len(want))
            _assert_same(Xt[i, k, : len(want)], want, what)
            assert (Xt[i, k, len(want):].view(np.int64) == FILL).all(), what + ": rows from m on were written"
            if i == 2:
                assert m[i, k] == 0
            if i == 1:
                assert m[i, k] == (S // 2 if not q & 1 else S - S // 2 + 1) * (S // 2 if not q & 2 else S - S // 2 + 1)
                full_br |= q == 3 and m[i, k] == m_cap
    assert full_br                                   # the bottom-right cut with every pixel kept fills its slot to the last row


# ------------------------------------------------------------------------------------------------------------ the bank
@pytest.mark.parametrize("case", cases.BANK_CASES, ids=lambda v: "-".join(str(x) for x in v))
def test_bank_clouds_at_the_edges(case):
    """Against the restatement of the items materialised in numpy, and bit for bit against otmi_rep_clouds of them."""
    from event_representation_study_amd import engine as eng
    S, C, slot, n_cand, B, dtype = case
    base, bank, cand, quad = cases.bank_case(*case)
    items = cases.bank_items(base, bank, slot, cand)
    if case in cases.BANK_MULTI_STEP:
        none, full, mixed = cases.bank_step_kinds(items, quad, B)
        assert none > 0 and full > 0 and mixed > 0, (none, full, mixed)
    dev = torch.device("cuda:0")
    n_items = n_cand * B
    m_cap = (S - (S // 2 - 1)) ** 2
    quad_t = torch.from_numpy(quad).to(dev)
    ws = eng.GwdWorkspace()
    ws.typed("otmi_xt", (n_items, 3, m_cap, C + 2), torch.float64).view(torch.int64).fill_(FILL)
    Xt, m, cap = eng.otmi_rep_clouds_bank(torch.from_numpy(base).to(dev), torch.from_numpy(bank).to(dev), slot, cand, quad_t, B,
                                          workspace=ws)
    assert cap == m_cap and Xt.shape == (n_items, 3, m_cap, C + 2) and m.shape == (n_items, 3)
    Xr, mr, _ = eng.otmi_rep_clouds(torch.from_numpy(items).to(dev), quad_t, B, workspace=eng.GwdWorkspace())
    assert torch.equal(m, mr)
    row = torch.arange(m_cap, device=dev)[None, None, :] < m[:, :, None]
    assert torch.equal(_bits(Xt)[row], _bits(Xr)[row])
    assert bool((_bits(Xt)[~row] == FILL).all()), "rows from m on were written"
    Xh, mh = Xt.cpu().numpy(), m.cpu().numpy()
    for i in range(n_items):
        for k in range(3):
            want = rep_cloud(items[i], int(quad[i % B, k]))
            what = "case %s item %d slot %d" % (case, i, k)
            assert mh[i, k] == len(want), "%s: m = %d, restatement %d" % (what, mh[i, k], len(want))
            _assert_same(Xh[i, k, : len(want)], want, what)
    assert 0 < mh.max() < m_cap
    # a repeated candidate gives the same cloud each time; behind candidate 512 the second launch wrote it
    first_of = {}
    repeats = 0
    for j, c in enumerate(cand):
        if c not in first_of:
            first_of[c] = j
            continue
        a, b = slice(first_of[c] * B, (first_of[c] + 1) * B), slice(j * B, (j + 1) * B)
        assert np.array_equal(mh[a], mh[b]) and np.array_equal(Xh[a].view(np.int64), Xh[b].view(np.int64)), (case, c, j)
        repeats += 1
    assert repeats == max(0, n_cand - cases.BANK_R)
    if n_cand > 512:
        assert all(c in cand[:512] and cand[:512].count(c) > 1 for c in set(cand[512:]))


# ---------------------------------------------------------------------------------------------------------- end to end
def test_otmi_batch_costs_on_the_odd_sensor(oracle):
    """R = 2 representations x B = 2 windows (one skewed) at S = 131 on the 239 x 305 sensor: every quadrant cost within the
    project's stated 1e-5 (include/evrep.h) of the oracle's closed form on the restatement's clouds."""
    from event_representation_study_amd import engine as eng
    H, W, S, C, R, B = 239, 305, 131, 5, 2, 2
    rng = np.random.default_rng(131)
    wins = [cases.window(rng, H, W, [300, 500, 400, 350]), cases.window(rng, H, W, [250, 300, 350, 1400], "01")]
    reps = (rng.random((R, B, S, S, C)) + 0.05) * (rng.random((R, B, S, S, 1)) < 0.3)
    reps[:, :, :9] = 114.0                                           # letterbox rows count as points
    dev = torch.device("cuda:0")
    offs = torch.tensor([0, len(wins[0]), len(wins[0]) + len(wins[1])], dtype=torch.int64)
    mean, q = eng.otmi_batch(torch.from_numpy(np.concatenate(wins)).to(dev), offs, torch.from_numpy(reps).to(dev), H, W,
                             workspace=eng.GwdWorkspace())
    mean, q = mean.cpu().numpy(), q.cpu().numpy()
    assert q.shape == (R, B, 3) and scored_quadrants(wins[0], H, W) != scored_quadrants(wins[1], H, W)
    for r in range(R):
        for b in range(B):
            for k, quadrant in enumerate(scored_quadrants(wins[b], H, W)):
                ref = oracle.gwd(event_cloud(wins[b], quadrant, H, W).astype(np.float64), rep_cloud(reps[r, b], quadrant))
                rel = abs(q[r, b, k] - ref) / abs(ref)
                print("rep %d window %d quadrant %d: %.12g (oracle %.12g, relative %.3g)" % (r, b, quadrant, q[r, b, k], ref, rel))
                assert rel <= 1e-5
            assert abs(mean[r, b] - q[r, b].mean()) <= 1e-12 * abs(mean[r, b])
