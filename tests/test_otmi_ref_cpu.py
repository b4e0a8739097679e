"""CPU: the per-quadrant restatement of the OTMI harness (tests/otmi_ref.py) and the package's host mirror
(compute_otmi.otmi_point_clouds) against the oracle's restatement of compute_otmi.py:96-205, over the case lists that
tests/test_gpu_otmi_edges.py runs on the device (tests/otmi_edge_cases.py).

For every window on which the oracle does not raise: the same three quadrants, the same shapes, the same bits outside NaN,
NaN in the same cells.  The oracle raises exactly on the windows the list marks `vacant` (a quadrant without an event: the
reference's min() of nothing), and at least four fifths of the windows are not marked.  Each test prints how many windows it
compared and how many were marked (`pytest -s` or `-rP` shows it).
"""
import numpy as np
import pytest
import torch

import otmi_edge_cases as cases
from otmi_ref import event_cloud, quadrant_counts, rep_box, rep_cloud, same_cloud, scored_quadrants


def _small_rep(S, C=2, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.random((S, S, C)) + 0.05) * (rng.random((S, S, 1)) < 0.6)


def _oracle_pairs(oracle, ev, rep, H, W):
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return oracle.otmi_point_clouds(ev, rep, H, W, rep.shape[0])


def _mirror_pairs(ev, rep, H, W):
    from event_representation_study_amd.representations.representation_search.compute_otmi import otmi_point_clouds
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return otmi_point_clouds(torch.from_numpy(ev.copy()), rep, H, W, rep.shape[0])


def _check_window(oracle, name, ev, rep, H, W):
    """The helpers and the mirror against the oracle on one window the oracle answers for."""
    ref = _oracle_pairs(oracle, ev, rep, H, W)
    quads = scored_quadrants(ev, H, W)
    assert len(ref) == len(quads) == 3, name
    mirror = _mirror_pairs(ev, rep, H, W)
    assert len(mirror) == 3, name
    for k, q in enumerate(quads):
        xs, xt = event_cloud(ev, q, H, W), rep_cloud(rep, q)
        assert xs is not None and xs.dtype == np.float32 and xt.dtype == np.float64, (name, q)
        for what, got, want in (("restated events", xs, ref[k][0]), ("restated representation", xt, ref[k][1]),
                                ("mirror events", mirror[k][0], ref[k][0]), ("mirror representation", mirror[k][1], ref[k][1])):
            diff = same_cloud(got, want)
            assert diff is None, "%s, slot %d = quadrant %d, %s: %s" % (name, k, q, what, diff)


@pytest.mark.parametrize("H,W", cases.SENSORS, ids=lambda v: str(v))
def test_event_windows_against_the_oracle(oracle, H, W):
    wins = cases.event_windows(H, W)
    raised, marked, skipped = set(), set(), set()
    for i, (name, ev, vacant) in enumerate(wins):
        rep = _small_rep((4, 5, 8)[i % 3], seed=i)
        if vacant:
            marked.add(name)
            assert min(quadrant_counts(ev, H, W)) == 0, name           # the mark says what it means
        try:
            _oracle_pairs(oracle, ev, rep, H, W)
        except (ValueError, IndexError):
            raised.add(name)
            continue
        skipped.add(({0, 1, 2, 3} - set(scored_quadrants(ev, H, W))).pop())
        _check_window(oracle, "%dx%d %s" % (H, W, name), ev, rep, H, W)
    assert raised == marked
    assert len(set(n for n, _, _ in wins)) == len(wins) and 5 * (len(wins) - len(marked)) >= 4 * len(wins)
    assert skipped == {0, 1, 2, 3}
    print("sensor %dx%d: %d windows compared with the oracle, %d marked vacant" % (H, W, len(wins) - len(marked), len(marked)))


def test_vacant_quadrants_leave_their_neighbours_answerable():
    """What the oracle cannot say: beside a vacant quadrant the occupied ones still have clouds, and the skipped quadrant
    is still the first maximum."""
    H, W = 5, 7
    wins = {n: ev for n, ev, v in cases.event_windows(H, W) if v}
    assert scored_quadrants(wins["empty"], H, W) == [1, 2, 3]
    assert all(event_cloud(wins["empty"], q, H, W) is None for q in range(4))
    assert scored_quadrants(wins["vacant_q3"], H, W) == [0, 2, 3] and event_cloud(wins["vacant_q3"], 3, H, W) is None
    assert scored_quadrants(wins["vacant_q0_q2"], H, W) == [0, 2, 3] and event_cloud(wins["vacant_q0_q2"], 3, H, W) is not None
    assert scored_quadrants(wins["vacant_all_but_q1"], H, W) == [0, 2, 3]
    assert [event_cloud(wins["vacant_all_but_q1"], q, H, W) is None for q in range(4)] == [True, False, True, True]


def test_expected_specials_occur_in_the_restated_event_clouds():
    """NaN, +inf and -inf where the case list means them to be (checked on every sensor on which a row survives the mask)."""
    for H, W in cases.SENSORS[1:]:
        cases.assert_specials_occur(cases.event_windows(H, W), H, W)
    H, W = cases.SENSORS[0]                                             # (2, 2): (W - 1) // 2 = 0, no row survives
    assert all(c is None or c.shape == (0, 4) for _, ev, _ in cases.event_windows(H, W) for c in [event_cloud(ev, q, H, W) for q in range(4)])


@pytest.mark.parametrize("S,C,dtype", cases.REP_CASES, ids=lambda v: str(v))
def test_representation_items_against_the_oracle(oracle, S, C, dtype):
    items, special = cases.rep_items(S, C, dtype)
    H, W = 5, 7
    compared = 0
    for i, rep in enumerate(items):
        for skip in range(4):
            if S > 100 and skip != i % 4:                               # the large cuts: one window per item, every quadrant cut
                continue
            ev = cases.skip_window(skip, H, W)
            assert scored_quadrants(ev, H, W) == [q for q in range(4) if q != skip]
            _check_window(oracle, "S=%d item %d skip %d" % (S, i, skip), ev, rep, H, W)
            compared += 1
    for q in range(4):
        y0, y1, x0, x1 = rep_box(S, q)
        npx = (y1 - y0 + 1) * (x1 - x0 + 1)
        full, none, mixed, spec = rep_cloud(items[1], q), rep_cloud(items[2], q), rep_cloud(items[0], q), rep_cloud(items[3], q)
        assert full.shape == (npx, C + 2) and none.shape == (0, C + 2) and 0 < len(mixed) and (len(mixed) < npx or S < 8)
        assert npx == (S - (S // 2 - 1)) ** 2 or q != 3
        for cl in (mixed, spec):                                        # the corners of the cut are kept: positions exactly 0 and 1
            assert cl[0, C] == 0 and cl[0, C + 1] == 0 and cl[-1, C] == 1 and cl[-1, C + 1] == 1
    # the special pixels of item 3, found in the clouds of the cuts that contain them
    found = {}
    for kind, (r, c) in special.items():
        for q in range(4):
            y0, y1, x0, x1 = rep_box(S, q)
            if y0 <= r <= y1 and x0 <= c <= x1:
                cl = rep_cloud(items[3], q)
                pos = (cl[:, C] == (r - y0) / (y1 - y0)) & (cl[:, C + 1] == (c - x0) / (x1 - x0))
                found.setdefault(kind, []).append(int(pos.sum()))
    assert all(set(found[k]) == {0} for k in ("minus_zero", "nan")), found
    assert all(set(found[k]) == {1} for k in ("negative", "subnormal", "plus_inf", "minus_inf")), found
    print("S=%d C=%d %s: %d item x window pairs compared with the oracle" % (S, C, dtype, compared))


@pytest.mark.parametrize("case", cases.BANK_CASES, ids=lambda v: "-".join(str(x) for x in v))
def test_bank_items_against_the_oracle(oracle, case):
    S, C, slot, n_cand, B, dtype = case
    base, bank, cand, quad = cases.bank_case(*case)
    items = cases.bank_items(base, bank, slot, cand)
    assert items.shape == (n_cand * B, S, S, C) and items.dtype == base.dtype
    assert n_cand <= cases.BANK_R or len(set(cand)) == cases.BANK_R
    H, W = 5, 7
    step = max(1, len(items) // 24)                                     # a sample of the items, every window and every table row
    for i in range(0, len(items), step):
        skip = ({0, 1, 2, 3} - set(int(v) for v in quad[i % B])).pop()
        _check_window(oracle, "bank item %d" % i, cases.skip_window(skip, H, W), items[i], H, W)
    if case in cases.BANK_MULTI_STEP:
        none, full, mixed = cases.bank_step_kinds(items, quad, B)
        print("S=%d: %d steps keep nothing, %d keep all 64 lanes, %d are mixed" % (S, none, full, mixed))
        assert none > 0 and full > 0 and mixed > 0
