"""The composed windows restated on the host (cough_detector_amd/windows.py, csrc/windows.hip): the background power in
the device's order of summation, the gains, and the mix written twice -- sample by sample and by whole slices -- so that
the two forms can be held against each other; the plan's draws row by row; the labels of sliding windows by brute force;
and the ragged batch that the host and the GPU suites both run.  The float32 ``fmaf`` and the gain come from
tests/scenes_ref.py."""
import math

import numpy as np

import scenes_ref as R

MAX_EVENTS = 4
THREADS = 256
DEFECTS = ("onset_off_by_one", "reverse_order", "wrap_one_short", "gain_from_visible_part", "power_of_whole_clip")


# ------------------------------------------------------------------------------------------------ the power, in order
def power_order(x):
    """float64 mean of double(x)^2 over the float32 samples ``x`` in cough_span_power's order: thread t adds samples t, t
    + 256, ... ascending from 0.0 (a thread whose samples have run out adds +0.0, which changes nothing), p[t] += p[t ^
    m] for m = 1 .. 32, then (w0 + w1) + (w2 + w3)."""
    x = np.asarray(x, dtype=np.float32)
    n = len(x)
    if n == 0:
        return 0.0
    with np.errstate(all="ignore"):
        sq = np.zeros(-(-n // THREADS) * THREADS, dtype=np.float64)
        sq[:n] = x.astype(np.float64) ** 2
        acc = np.zeros(THREADS, dtype=np.float64)
        for row in sq.reshape(-1, THREADS):
            acc = acc + row
        lane = np.arange(THREADS)
        for m in (1, 2, 4, 8, 16, 32):
            acc = acc + acc[lane ^ m]
        return float(((acc[0] + acc[64]) + (acc[128] + acc[192])) / np.float64(n))


def power_order_loop(x):
    """The same, thread by thread in plain Python."""
    x = [float(v) for v in np.asarray(x, dtype=np.float32)]
    if not x:
        return 0.0
    with np.errstate(all="ignore"):
        p = []
        for t in range(THREADS):
            acc = np.float64(0.0)
            for i in range(t, len(x), THREADS):
                acc = acc + np.float64(x[i]) * np.float64(x[i])
            p.append(acc)
        for m in (1, 2, 4, 8, 16, 32):
            p = [p[t] + p[t ^ m] for t in range(THREADS)]
        return float(((p[0] + p[64]) + (p[128] + p[192])) / np.float64(len(x)))


# ------------------------------------------------------------------------------------------------ one row, twice
def _background(bg):
    return None if bg is None or len(bg) == 0 else np.asarray(bg, dtype=np.float32)


def row_gains(bg, bg_start, bg_gain, width, events, p_ev=None, p_bg=None):
    """``(P_bg, [gain])`` of one row.  ``events``: ``[(samples float32, onset, snr_linear)]``; ``p_ev``: the clips' powers
    (default: ``power_order`` of each whole clip); ``p_bg``: the background's power (default: ``power_order`` of the
    span)."""
    bg = _background(bg)
    if p_bg is None:
        p_bg = 0.0 if bg is None else power_order(R.span_ref(bg, bg_start, width))
    if bg is None:
        p_bg = 0.0
    if p_ev is None:
        p_ev = [power_order(x) for x, _, _ in events]
    return p_bg, [R.gain_ref(snr, bg_gain, p_bg, pe) for (_, _, snr), pe in zip(events, p_ev)]


def compose_loop(bg, bg_start, bg_gain, width, events, p_ev=None, p_bg=None):
    """One row, sample by sample: ``(out float32, P_bg, gains)``."""
    bg = _background(bg)
    p_bg, gains = row_gains(bg, bg_start, bg_gain, width, events, p_ev, p_bg)
    g, out = np.float32(bg_gain), np.empty(width, dtype=np.float32)
    with np.errstate(all="ignore"):
        for i in range(width):
            acc = np.float32(0.0) if bg is None else np.float32(g * bg[(bg_start + i) % len(bg)])
            for (x, onset, _), gain in zip(events, gains):
                if onset <= i < onset + len(x):
                    acc = R.fmaf(gain, x[i - onset], acc)
            out[i] = acc
    return out, p_bg, gains


def compose_slices(bg, bg_start, bg_gain, width, events, p_ev=None, p_bg=None, defect=None):
    """The same row by whole slices.  ``defect``: one of ``DEFECTS``, planted on purpose (tests only)."""
    assert defect is None or defect in DEFECTS
    bg = _background(bg)
    if defect == "power_of_whole_clip" and bg is not None:
        p_bg = power_order(bg)
    if defect == "gain_from_visible_part":
        p_ev = []
        for x, onset, _ in events:
            lo, hi = max(onset, 0), min(onset + len(x), width)
            p_ev.append(power_order(x[lo - onset:hi - onset]) if lo < hi else power_order(x))
    p_bg, gains = row_gains(bg, bg_start, bg_gain, width, events, p_ev, p_bg)
    with np.errstate(all="ignore"):
        if bg is None:
            out = np.zeros(width, dtype=np.float32)
        elif defect == "wrap_one_short" and len(bg) > 1:
            out = (np.float32(bg_gain) * bg[(bg_start + np.arange(width)) % (len(bg) - 1)]).astype(np.float32)
        else:
            out = (np.float32(bg_gain) * R.span_ref(bg, bg_start, width)).astype(np.float32)
        order = list(zip(events, gains))
        for (x, onset, _), gain in (order[::-1] if defect == "reverse_order" else order):
            x = np.asarray(x, dtype=np.float32)
            onset = onset + 1 if defect == "onset_off_by_one" else onset
            lo, hi = max(onset, 0), min(onset + len(x), width)
            if lo < hi:
                out[lo:hi] = R.fmaf(gain, x[lo - onset:hi - onset], out[lo:hi])
    return out, p_bg, gains


# ------------------------------------------------------------------------------------------------ the ragged batch
BG_LENGTHS = [1, 1000, 3, 2, 16000, 50000, 333, 50, 1001]
BG_ONE, BG_1000, BG_THREE, BG_TWO, BG_16000, BG_50000, BG_NAN, BG_SILENT, BG_INF = range(9)
EV_LENGTHS = [1, 30, 255, 1601, 4000, 20, 20000, 12, 2]
EV_ZERO, EV_LONG = 5, 6


def banks():
    """The two banks of the batch as lists of float32 clips.  Packed end to end, the clips of each start at all four
    4-byte phases."""
    rng = np.random.default_rng(7)
    bgs = [(rng.standard_normal(n) * 0.1).astype(np.float32) for n in BG_LENGTHS]
    bgs[BG_NAN][100] = np.nan
    bgs[BG_SILENT][:] = 0.0
    bgs[BG_INF][7] = np.inf
    evs = [rng.standard_normal(n).astype(np.float32) for n in EV_LENGTHS]
    evs[EV_ZERO][:] = 0.0
    for lengths in (BG_LENGTHS, EV_LENGTHS):
        assert {int(o) % 4 for o in np.concatenate([[0], np.cumsum(lengths)[:-1]])} == {0, 1, 2, 3}
    return bgs, evs


def batch_rows(width):
    """About 50 rows ``(background, bg_start, bg_gain, [(event clip, onset, snr_db)])`` for rows of ``width``: every
    background length with ``bg_start`` at 0 and at its last sample; onsets of ``-(n_e - 1)``, ``-n_e``, 0, ``width - 1``,
    ``width`` and the middle for clips of 1, 30, 255, 1601 and 4000 samples; a clip longer than the row that covers all of
    it; two and four events over each other and one clip twice; silence by index and by content; an all-zero event; a
    NaN and an Inf in a background; a row without events; and rows whose events lie inside the row side by side."""
    W, n = int(width), EV_LENGTHS
    cases = [lambda m: -(m - 1), lambda m: -m, lambda m: 0, lambda m: W - 1, lambda m: W, lambda m: (W - m) // 2]
    rows, k = [], 0
    for b in (BG_ONE, BG_THREE, BG_1000, BG_16000, BG_50000):
        for start in (0, BG_LENGTHS[b] - 1):
            c = k % 5
            rows.append((b, start, [1.0, 0.5, 1.7][k % 3], [(c, cases[k % 6](n[c]), 5.0 + 1.5 * k)]))
            k += 1
    for case in cases:
        for c in range(5):
            b = (BG_16000, BG_50000, BG_1000)[k % 3]
            rows.append((b, (37 * k) % BG_LENGTHS[b], [1.0, 0.8][k % 2], [(c, case(n[c]), 5.0 + (k % 11) * 1.5)]))
            k += 1
    rows.append((-1, 0, 1.0, [(1, 3, 10.0)]))
    rows.append((-1, 0, 0.5, []))
    rows.append((BG_50000, 123, 1.0, []))
    rows.append((BG_50000, 49999, 1.0, [(EV_LONG, -1000, 8.0)]))
    rows.append((BG_16000, 5, 0.8, [(3, 10, 6.0), (2, 100, 12.0)]))
    rows.append((BG_16000, 15999, 1.0, [(4, -100, 5.0), (3, 50, 10.0), (2, 60, 15.0), (1, 70, 20.0)]))
    rows.append((BG_1000, 999, 1.3, [(2, 0, 10.0), (2, 7, 10.0)]))
    rows.append((BG_TWO, 1, 1.0, [(7, W - 5, 9.0), (8, -1, 11.0)]))
    rows.append((BG_SILENT, 10, 1.0, [(1, 5, 10.0)]))
    rows.append((BG_1000, 0, 1.0, [(EV_ZERO, 3, 10.0), (1, 8, 10.0)]))
    rows.append((BG_NAN, 0, 1.0, [(1, 2, 10.0)]))
    rows.append((BG_INF, 0, 1.0, [(1, 2, 10.0)]))
    for b, start in ((BG_16000, 77), (BG_THREE, 2), (BG_50000, 40000)):       # side by side, as many as fit
        events, at = [], 0
        for c in (0, 1, 2, 3):
            if at + n[c] <= W:
                events.append((c, at, 6.0 + 3 * c))
                at += n[c] + 1
        rows.append((b, start, 1.2, events))
    return rows


def plan_arrays(rows):
    """The rows as the seven arrays of a ``WindowPlan``."""
    b = len(rows)
    clip, onset, snr = np.full((b, MAX_EVENTS), -1, np.int64), np.zeros((b, MAX_EVENTS), np.int64), np.zeros((b, MAX_EVENTS))
    for r, (_, _, _, events) in enumerate(rows):
        for e, (c, on, db) in enumerate(events):
            clip[r, e], onset[r, e], snr[r, e] = c, on, db
    return (np.array([r[0] for r in rows], np.int64), np.array([r[1] for r in rows], np.int64),
            np.array([r[2] for r in rows], np.float32), np.array([len(r[3]) for r in rows], np.int64), clip, onset, snr)


def row_events(row, evs, snr_linear):
    """The events of one row as the restatements take them; ``snr_linear``: the row's four linear SNRs."""
    return [(evs[c], int(on), float(snr_linear[e])) for e, (c, on, _) in enumerate(row[3])]


def inside_and_apart(row, width):
    """Whether the row is one ``compose_scenes`` accepts: a background, every event inside the row, none over another."""
    spans = sorted((on, on + EV_LENGTHS[c]) for c, on, _ in row[3])
    return (row[0] >= 0 and all(a >= 0 and b <= width for a, b in spans)
            and all(spans[k + 1][0] >= spans[k][1] for k in range(len(spans) - 1)))


# ------------------------------------------------------------------------------------------------ the draws, row by row
def draw_ref(bg_lengths, ev_lengths, ev_labels, b, width, sample_rate, seed, p_cough=0.5, p_distractor=None,
             coughs_per_window=(1, 2), snr_range=(5, 20), bg_gain_range=(1.0, 1.0), min_overlap_seconds=0.1, margin=0,
             rho_min=1.0):
    """``draw_window_plan``'s draws in its documented order, the rows then worked out one by one."""
    bl, el, lab = np.asarray(bg_lengths), np.asarray(ev_lengths), np.asarray(ev_labels)
    coughs, others = np.flatnonzero(lab == 1), np.flatnonzero(lab == 0)
    if p_distractor is None:
        p_distractor = 0.3 if others.size else 0.0
    m = max(1, math.ceil(min_overlap_seconds * sample_rate))
    rng = np.random.Generator(np.random.Philox(seed))
    if bl.size:
        background = rng.integers(0, bl.size, size=b)
        start = rng.integers(0, bl[background])
    else:
        background, start = np.full(b, -1), np.zeros(b, int)
    gain = rng.uniform(bg_gain_range[0], bg_gain_range[1], size=b)
    cough_coin = rng.random(b)
    cough_count = rng.integers(coughs_per_window[0], coughs_per_window[1] + 1, size=b)
    other_coin = rng.random(b)
    other_count = rng.integers(1, 3, size=b)
    pick_c = rng.integers(0, max(coughs.size, 1), size=(b, MAX_EVENTS))
    pick_d = rng.integers(0, max(others.size, 1), size=(b, MAX_EVENTS))
    snr = rng.uniform(snr_range[0], snr_range[1], size=(b, MAX_EVENTS))
    lowest, highest = np.zeros((b, MAX_EVENTS), np.int64), np.zeros((b, MAX_EVENTS), np.int64)
    clip, n_events = np.full((b, MAX_EVENTS), -1, np.int64), np.zeros(b, np.int64)
    for r in range(b):
        n_c = int(cough_count[r]) if cough_coin[r] < p_cough else 0
        n_d = min(int(other_count[r]), MAX_EVENTS - n_c) if other_coin[r] < p_distractor else 0
        n_events[r] = n_c + n_d
        for e in range(n_c + n_d):
            clip[r, e] = coughs[pick_c[r, e]] if e < n_c else others[pick_d[r, e]]
            length = int(el[clip[r, e]])
            need = min(length, int(math.ceil(min(m, length) / rho_min)))
            lowest[r, e], highest[r, e] = margin + need - length, width - margin - need
    onset = rng.integers(lowest, highest + 1)
    used = np.arange(MAX_EVENTS)[None, :] < n_events[:, None]
    return dict(background=background, bg_start=start, bg_gain=gain.astype(np.float32), n_events=n_events, event_clip=clip,
                onset=np.where(used, onset, 0), snr_db=np.where(used, snr, 0.0), lowest=lowest, highest=highest)


# ------------------------------------------------------------------------------------------------ window labels
def window_labels_brute(onsets, offsets, n_samples, window, hop, m):
    """``[(label, overlap)]`` of every window of ONE recording of ``n_samples`` with events ``[onset, offset)``: every
    window against every event."""
    out = []
    for k in range(0 if n_samples < window else 1 + (n_samples - window) // hop):
        shared = [min(k * hop + window, b) - max(k * hop, a) for a, b in zip(onsets, offsets)]
        hit = any(s >= min(m, b - a) for s, a, b in zip(shared, onsets, offsets))
        touched = any(s > 0 for s in shared)
        out.append((1 if hit else -1 if touched else 0, max([0] + shared)))
    return out
