"""The case lists of the OTMI harness's edge tests, shared by tests/test_otmi_ref_cpu.py (oracle against the per-quadrant
restatement and the package's host mirror) and tests/test_gpu_otmi_edges.py (the device kernels against the restatement).
Everything is numpy and deterministic; nothing here touches a device.
"""
import numpy as np

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1

SENSORS = [(2, 2), (3, 3), (4, 6), (5, 7), (240, 304), (239, 305)]
# window lengths: one event per quadrant; around the 16 slices; around slices x 1024 threads, where a thread's share goes
# from 1 to 2 (16384 -> 16385) and on to 3 (32769)
LENGTHS = [4, 15, 16, 17, 1023, 1025, 16383, 16384, 16385, 32769, 40000]


def _span(n, q_bit):
    """Pixels [lo, hi] of the first (q_bit = 0) / second half of an axis of n pixels: v <= n / 2 - 1 on the first."""
    last_first = (n - 2) // 2            # the largest integer <= n / 2 - 1
    return (last_first + 1, n - 1) if q_bit else (0, last_first)


def window(rng, H, W, counts, pol="pm1"):
    """counts[q] events in quadrant q, quadrants interleaved at random, timestamps strictly ascending, the first event of a
    quadrant at its first pixel and (where it has two) the second at its last pixel."""
    qs = np.repeat(np.arange(4), counts)
    rng.shuffle(qs)
    ev = np.zeros((len(qs), 4), np.int32)
    for q in range(4):
        idx = np.flatnonzero(qs == q)
        (x0, x1), (y0, y1) = _span(W, q & 1), _span(H, q >> 1)
        ev[idx, 0] = rng.integers(x0, x1 + 1, len(idx))
        ev[idx, 1] = rng.integers(y0, y1 + 1, len(idx))
        if len(idx) > 0:
            ev[idx[0], :2] = (x0, y0)
        if len(idx) > 1:
            ev[idx[1], :2] = (x1, y1)
    ev[:, 2] = np.cumsum(rng.integers(1, 40, len(qs)))
    p = rng.integers(0, 2, len(qs))
    ev[:, 3] = 2 * p - 1 if pol == "pm1" else p
    return ev


def _spread(rng, n, weights):
    """n events over the four quadrants, at least one each."""
    w = np.asarray(weights, float)
    return rng.multinomial(n - 4, w / w.sum()) + 1


def out_of_frame(H, W):
    return np.array([[-1, 0, 5, 1], [W, 0, 6, -1], [0, -1, 7, 1], [0, H, 8, -1], [I32_MAX, I32_MAX, 9, 1], [I32_MIN, 0, 10, -1]],
                    np.int32)


def event_windows(H, W):
    """-> list of (name, events int32 (n, 4), vacant).  `vacant`: some quadrant holds no event (the reference raises)."""
    rng = np.random.default_rng(1000 * H + W)
    wins = []
    heavy = 0
    for n in LENGTHS:
        if n == 4:
            counts = [1, 1, 1, 1]
        else:
            w = [1.0, 1.0, 1.0, 1.0]
            w[heavy % 4] = 2.5
            heavy += 1
            counts = _spread(rng, n, w)
        wins.append(("len%d" % n, window(rng, H, W, counts, "01" if n % 2 else "pm1"), False))
        if n == 17:
            wins.append(("empty", np.zeros((0, 4), np.int32), True))

    def add(name, ev, vacant=False):
        wins.append((name, np.ascontiguousarray(ev, dtype=np.int32), vacant))

    base = window(rng, H, W, [40, 70, 50, 60])
    oof = out_of_frame(H, W)
    add("out_of_frame", np.concatenate([oof[::-1], base[:100], oof[:3], base[100:], oof]))
    add("tie01", window(rng, H, W, [50, 50, 20, 30]))
    add("tie23", window(rng, H, W, [20, 30, 50, 50]))
    add("tie_all", window(rng, H, W, [25, 25, 25, 25]))
    for q in range(4):
        c = [30, 30, 30, 30]
        c[q] = 90
        add("most%d" % q, window(rng, H, W, c))
    # quadrant 1's events share one timestamp (0 / 0 in the t column), quadrant 2's one polarity (0 / 0 in the p column)
    ev = window(rng, H, W, [60, 40, 40, 40])
    ev[_in(ev, 1, H, W), 2] = 777
    add("one_timestamp_q1", ev)
    ev = window(rng, H, W, [60, 40, 40, 40])
    ev[_in(ev, 2, H, W), 3] = 1
    add("one_polarity_q2", ev)
    ev = window(rng, H, W, [40, 40, 40, 60])
    ev[:, 3] = np.where(ev[:, 3] > 0, I32_MAX, I32_MIN)
    for q in range(3):                                   # both extremes in every scored quadrant
        i = np.flatnonzero(_in(ev, q, H, W))
        ev[i[0], 3], ev[i[-1], 3] = I32_MIN, I32_MAX
    add("polarity_int32_extremes", ev)
    ev = window(rng, H, W, [40, 60, 40, 40])
    ev[:, 2] = np.linspace(I32_MIN, I32_MAX, len(ev)).astype(np.int64)
    ev[0, 2], ev[-1, 2] = I32_MIN, I32_MAX
    i = np.flatnonzero(_in(ev, 0, H, W))                 # quadrant 0 spans the whole int32 range by itself
    ev[i[0], 2], ev[i[-1], 2] = I32_MIN, I32_MAX
    add("timestamps_int32_range", ev)
    ev = window(rng, H, W, [40, 40, 60, 40])
    ev[:, 2] = ev[::-1, 2].copy()
    add("timestamps_descending", ev)
    # shuffled timestamps; quadrant 0's first and last member are equal in time, its other members lie on both sides of them
    # and one more is equal: +inf, -inf and NaN in one t column
    ev = window(rng, H, W, [40, 40, 40, 60])
    ev[:, 2] = rng.permutation(ev[:, 2])
    i = np.flatnonzero(_in(ev, 0, H, W))
    ev[i, 2] = 5000 + rng.permutation(len(i)) - len(i) // 2
    ev[i[0], 2] = ev[i[-1], 2] = ev[i[7], 2] = 5000
    ev[i[3], 2], ev[i[4], 2] = 4000, 6000
    ev[i[[3, 4, 7]], :2] = 0                             # pixel (0, 0) survives the mask wherever anything does
    add("shuffled_t0_equals_t1_q0", ev)
    add("vacant_q3", window(rng, H, W, [30, 50, 40, 0]), True)
    add("vacant_q0_q2", window(rng, H, W, [0, 50, 0, 40]), True)
    add("vacant_all_but_q1", window(rng, H, W, [0, 20, 0, 0]), True)
    return wins


def assert_specials_occur(windows, H, W):
    """NaN, +inf and -inf sit where the list means them to be -- asserted on the restatement (tests/otmi_ref.py), for a
    sensor on which rows survive the mask (H, W > 2)."""
    from otmi_ref import event_cloud
    wins = {n: ev for n, ev, _ in windows}
    t = event_cloud(wins["one_timestamp_q1"], 1, H, W)
    assert len(t) and np.isnan(t[:, 2]).all() and not np.isnan(t[:, [0, 1]]).any()
    p = event_cloud(wins["one_polarity_q2"], 2, H, W)
    assert len(p) and np.isnan(p[:, 3]).all() and np.isfinite(p[:, :3]).all()
    s = event_cloud(wins["shuffled_t0_equals_t1_q0"], 0, H, W)[:, 2]
    assert np.isnan(s).any() and (s == np.inf).any() and (s == -np.inf).any()
    one = event_cloud(wins["len4"], 1, H, W)
    assert one.shape == (1, 4) and np.isnan(one[0, 2:]).all() and np.array_equal(one[0, :2], [0, 0])
    d = event_cloud(wins["timestamps_descending"], 0, H, W)[:, 2]
    assert d[0] == 0 and (d >= 0).all() and d.max() <= 1
    e = event_cloud(wins["polarity_int32_extremes"], 0, H, W)[:, 3]
    assert set(np.unique(e)) == {0.0, 1.0}


def _in(ev, q, H, W):
    (x0, x1), (y0, y1) = _span(W, q & 1), _span(H, q >> 1)
    return (ev[:, 0] >= x0) & (ev[:, 0] <= x1) & (ev[:, 1] >= y0) & (ev[:, 1] <= y1)


def skip_window(q, H=5, W=7):
    """A small window without a vacant quadrant whose most populated quadrant is q."""
    c = [3, 3, 3, 3]
    c[q] = 6
    return window(np.random.default_rng(50 + q), H, W, c)


# ------------------------------------------------------------------------------------------------------- representations
# every quadrant at every slot position; four windows with four different tables
REP_QUAD = np.array([[0, 1, 2], [3, 0, 1], [2, 3, 0], [1, 2, 3]], np.int32)
# S = 362: the small quadrant (181^2 = 32761 pixels) stays at one pixel per thread of its 32 x 1024, the large ones
# (182^2 = 33124) reach two; S = 363: 181^2 and 183^2
REP_CASES = [(4, 1, "f64"), (5, 3, "f32"), (47, 30, "f64"), (48, 30, "f32"), (362, 2, "f32"), (363, 1, "f64")]
NP_DTYPE = {"f64": np.float64, "f32": np.float32}


def rep_items(S, C, dtype):
    """(2 * B, S, S, C) items for REP_QUAD (item i belongs to window i % B), and for item 3 the dict of its special pixels.
    0: about 70 % all-zero pixels;  1: every pixel kept (m == npx, == m_cap for quadrant 3);  2: all zero (m == 0);
    3: about 70 % zero plus pixels that hold only a negative value, only -0.0 (dropped), only a subnormal (kept), +inf,
    -inf (kept) and a NaN beside a non-zero value (dropped);  4-7: about 70 % zero.  Items 0 and 3-7 keep the nine pixels at
    rows / columns {0, S / 2 - 1, S - 1}, which are the corners of every cut: the positional channels show exactly 0 and 1."""
    dt = NP_DTYPE[dtype]
    rng = np.random.default_rng(7 * S + C)
    B = REP_QUAD.shape[0]
    items = (rng.random((2 * B, S, S, C)) + 0.05) * (rng.random((2 * B, S, S, 1)) < 0.3)
    items = items.astype(dt)
    items[1] = (rng.random((S, S, C)) + 0.05).astype(dt)
    items[2] = 0
    ih = S // 2 - 1
    for i in (0, 3, 4, 5, 6, 7):
        for r in (0, ih, S - 1):
            for c in (0, ih, S - 1):
                items[i, r, c, 0] = 0.5 + r + c
    tiny = np.float64(5e-324) if dt is np.float64 else np.float32(1e-45)
    free = [p for p in rng.permutation(S * S) if (p // S) not in (0, ih, S - 1) or (p % S) not in (0, ih, S - 1)]
    kinds = ["negative", "minus_zero", "subnormal", "plus_inf", "minus_inf", "nan"]
    special = {}
    for kind, p in zip(kinds, free):
        r, c = int(p) // S, int(p) % S
        items[3, r, c, :] = 0
        items[3, r, c, C - 1] = {"negative": -3.25, "minus_zero": -0.0, "subnormal": tiny, "plus_inf": np.inf,
                                 "minus_inf": -np.inf, "nan": np.nan}[kind]
        if kind == "nan" and C > 1:
            items[3, r, c, 0] = 2.0
        special[kind] = (r, c)
    assert tiny > 0 and np.signbit(items[3][special["minus_zero"]][C - 1])
    return items, special


# ------------------------------------------------------------------------------------------------------------- the bank
# (S, C, slot, n_cand, B, dtype).  A wave owns ceil(npx / 32) pixels of a quadrant and walks them 64 at a time:
#   96: 48^2 -> 72 (64 + 8), 49^2 -> 76;   131: 65^2 -> 133 (64 + 64 + 5), 67^2 -> 141;   240: 120^2 -> 450, 121^2 -> 458 (8 steps)
BANK_CASES = [(96, 5, 2, 20, 2, "f64"), (131, 5, 4, 17, 2, "f32"), (240, 12, 5, 16, 1, "f64"),
              (48, 30, 0, 23, 3, "f64"), (48, 30, 29, 23, 3, "f32"), (48, 1, 0, 18, 2, "f64"),
              (8, 3, 1, 1, 1, "f64"), (8, 3, 1, 512, 1, "f64"), (8, 3, 1, 513, 1, "f32"), (8, 3, 1, 530, 2, "f64")]
BANK_MULTI_STEP = [c for c in BANK_CASES if c[0] in (96, 131, 240)]
BANK_R = 11
BANK_QUAD = np.array([[0, 2, 3], [1, 2, 3], [0, 1, 3]], np.int32)
BANK_BAND = 6


def bank_case(S, C, slot, n_cand, B, dtype):
    """-> base (B, S, S, C), bank (B, S, S, BANK_R), cand (n_cand host ints), quad (B, 3).
    Image rows come in bands of BANK_BAND: all zero (base and bank) / every bank channel non-zero / about 70 % zero pixels
    with a sparse bank, so that a wave's 64-pixel steps include some that keep nothing, some that keep every lane, and mixed
    ones.  Bank channel 7 is zero inside the sparse band; one NaN sits in a bank channel and one in a base channel.
    cand walks the bank channels with a stride, so every channel repeats wherever n_cand > BANK_R (in the 513- and
    530-candidate cases both before and behind candidate 512, where the second launch begins)."""
    dt = NP_DTYPE[dtype]
    rng = np.random.default_rng(S * 100 + C * 3 + slot + n_cand)
    R = BANK_R
    base = (rng.random((B, S, S, C)) + 0.05) * (rng.random((B, S, S, 1)) < 0.2)
    bank = (rng.random((B, S, S, R)) + 0.05) * (rng.random((B, S, S, R)) < 0.12)
    bank[..., 7] = 0.0
    band = (np.arange(S) // BANK_BAND) % 3
    base[:, band == 0] = 0.0
    bank[:, band == 0] = 0.0
    bank[:, band == 1] = rng.random((B, int((band == 1).sum()), S, R)) + 0.05
    base[..., slot] = 0.0
    if S >= 48:
        bank[0, S // 2 + 5, S // 2 + 3, 3] = np.nan
        base[B - 1, S // 2 - 4, S // 2 - 6, (slot + 1) % C] = np.nan       # C = 1: the replaced channel itself, which must not count
    cand = [int((5 * j + 2) % R) for j in range(n_cand)]
    quad = BANK_QUAD[:B].copy()
    return base.astype(dt), bank.astype(dt), cand, quad


def bank_items(base, bank, slot, cand):
    """The materialised items (n_cand * B, S, S, C): item j * B + b = base[b] with channel `slot` from bank[b, ..., cand[j]]."""
    items = np.repeat(base[None], len(cand), axis=0)
    items[..., slot] = np.moveaxis(bank[..., cand], -1, 0)
    return items.reshape((len(cand) * base.shape[0],) + base.shape[1:])


def bank_step_kinds(items, quad, B, slices=32, lanes=64):
    """From the inputs alone: how many 64-pixel steps of the bank kernel's walk (a wave per slice of ceil(npx / slices)
    pixels of a cut, row-major) keep no pixel of an item, keep all 64, or keep some -> (none, all, mixed)."""
    from otmi_ref import rep_box
    S = items.shape[1]
    with np.errstate(invalid="ignore"):
        kept_px = np.abs(items.astype(np.float64)).sum(-1) > 0
    none = full = mixed = 0
    for i in range(items.shape[0]):
        for k in range(3):
            y0, y1, x0, x1 = rep_box(S, int(quad[i % B, k]))
            kept = kept_px[i, y0: y1 + 1, x0: x1 + 1].reshape(-1)
            per = -(-kept.size // slices)
            for s0 in range(0, kept.size, per):
                s1 = min(s0 + per, kept.size)
                for c0 in range(s0, s1, lanes):
                    nk = int(kept[c0: min(c0 + lanes, s1)].sum())
                    if nk == 0:
                        none += 1
                    elif nk == lanes:
                        full += 1
                    else:
                        mixed += 1
    return none, full, mixed
