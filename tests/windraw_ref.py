"""The draw contract of ``include/cough_amd_windraw.h`` restated in numpy (``csrc/windraw.hip``,
``cough_detector_amd.windows.draw_window_records``), on ``draws_ref``'s Philox4x32-10 and ``unit``.

It is written twice: ``draw_rows`` row by row and slot by slot in Python scalars (floats are IEEE float64, ``int()``
truncates toward zero), ``draw_batch`` vectorised over the batch (numpy has no fused multiply-add; ``astype`` truncates).
The host test holds the two equal; the GPU test compares ``draw_batch`` bit for bit with what ``cough_draw_window_plans``
wrote.  ``draw_batch(..., defect=)`` plants one of ``DEFECTS`` -- mistakes a kernel could make -- which the record
comparison has to catch.
"""
import math

import numpy as np

from draws_ref import philox4x32_10, unit

SLOTS, LEVELS, THREADS, LAST_WORD = 4, 1024, 64, 6
PLAN_DTYPE = np.dtype([("background", "<i4"), ("bg_start", "<i4"), ("bg_gain", "<f4"), ("n_events", "<i4"),
                       ("clip", "<i4", (SLOTS,)), ("onset", "<i4", (SLOTS,)), ("snr_linear", "<f8", (SLOTS,))])   # cough_window_plan
DEFECTS = ("onset_range_one_short", "need_without_rho", "distractors_first", "count_not_cut", "level_from_low_bits")


def snr_levels(lo, hi):
    lo, hi = float(lo), float(hi)
    return 10.0 ** ((lo + (hi - lo) * (np.arange(LEVELS, dtype=np.float64) + 0.5) / 1024) / 10)


def arguments(bg_lengths, ev_lengths, ev_labels, width, p_cough=0.5, p_distractor=None, coughs_per_window=(1, 2),
              snr_range=(5, 20), bg_gain_range=(1.0, 1.0), m=1600, margin=0, rho_min=1.0):
    """What a draw reads, as ``cough_draw_window_plans`` takes it: the lists of clips labelled 1 and 0, the SNR table,
    ``p_distractor=None`` resolved as ``draw_window_plan`` resolves it."""
    lab = np.asarray(ev_labels, dtype=np.int64)
    coughs, others = np.flatnonzero(lab == 1), np.flatnonzero(lab == 0)
    if p_distractor is None:
        p_distractor = 0.3 if others.size else 0.0
    return dict(bg_lengths=np.asarray(bg_lengths, dtype=np.int64), ev_lengths=np.asarray(ev_lengths, dtype=np.int64),
                coughs=coughs, others=others, width=int(width), p_cough=float(p_cough), p_distractor=float(p_distractor),
                c_lo=int(coughs_per_window[0]), c_hi=int(coughs_per_window[1]), g_lo=float(bg_gain_range[0]),
                g_hi=float(bg_gain_range[1]), snr=snr_levels(*snr_range), m=int(m), margin=int(margin), rho_min=float(rho_min))


def _key(seed):
    seed = int(seed) & (2**64 - 1)
    return seed & 0xFFFFFFFF, seed >> 32


# ------------------------------------------------------------------------------------------------ row by row
def _integer(u, lo, hi):
    return lo + min(int(u * float(hi - lo + 1)), hi - lo)


def draw_rows(seed, b, a):
    """-> (records: PLAN_DTYPE (b,), labels: int64 (b,)), one row and one slot at a time."""
    rec, labels = np.zeros(b, dtype=PLAN_DTYPE), np.zeros(b, dtype=np.int64)
    key = _key(seed)
    for row in range(b):
        block = lambda s: [int(w) for w in philox4x32_10((s, row, 0, LAST_WORD), key)]
        x, y, z, w = block(0)
        background, start = -1, 0
        if a["bg_lengths"].size:
            pick = _integer(float(unit(x)), 0, a["bg_lengths"].size - 1)
            n_b = int(a["bg_lengths"][pick])
            if n_b >= 1:
                background, start = pick, _integer(float(unit(y)), 0, n_b - 1)
        gain = np.float32(a["g_lo"] + (a["g_hi"] - a["g_lo"]) * float(unit(z)))
        positive = float(unit(w)) <= a["p_cough"]
        x, y, z, _ = block(1)
        n_coughs = _integer(float(unit(x)), a["c_lo"], a["c_hi"]) if positive else 0
        distracted = float(unit(y)) <= a["p_distractor"] and a["others"].size > 0
        n_others = min(_integer(float(unit(z)), 1, 2), SLOTS - n_coughs) if distracted else 0
        r = rec[row]
        r["background"], r["bg_start"], r["bg_gain"], r["n_events"] = background, start, gain, n_coughs + n_others
        for e in range(SLOTS):
            clip, onset, snr = -1, 0, 1.0
            if e < n_coughs + n_others:
                x, y, z, w = block(2 + e)
                if e < n_coughs:
                    clip = int(a["coughs"][_integer(float(unit(x)), 0, a["coughs"].size - 1)])
                else:
                    clip = int(a["others"][_integer(float(unit(y)), 0, a["others"].size - 1)])
                snr = float(a["snr"][z >> 22])
                n_c = int(a["ev_lengths"][clip])
                need = min(n_c, int(math.ceil(float(min(a["m"], n_c)) / a["rho_min"])))
                onset = _integer(float(unit(w)), a["margin"] + need - n_c, a["width"] - a["margin"] - need)
            r["clip"][e], r["onset"][e], r["snr_linear"][e] = clip, onset, snr
        labels[row] = n_coughs > 0
    return rec, labels


# ------------------------------------------------------------------------------------------------ the batch at once
def _integers(u, lo, hi):
    lo, hi = np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)
    return lo + np.minimum((u * (hi - lo + 1).astype(np.float64)).astype(np.int64), hi - lo)


def draw_batch(seed, b, a, defect=None):
    """-> (records: PLAN_DTYPE (b,), labels: int64 (b,)), every draw vectorised over the rows."""
    assert defect is None or defect in DEFECTS
    rows, key = np.arange(b, dtype=np.uint64), _key(seed)
    block = lambda s: philox4x32_10((np.full(b, s, dtype=np.uint64), rows, 0, LAST_WORD), key)
    rec = np.zeros(b, dtype=PLAN_DTYPE)
    s0, s1 = block(0), block(1)
    bl = a["bg_lengths"]
    if bl.size:
        pick = _integers(unit(s0[0]), 0, bl.size - 1)
        n_b = bl[pick]
        rec["background"] = np.where(n_b >= 1, pick, -1)
        rec["bg_start"] = np.where(n_b >= 1, _integers(unit(s0[1]), 0, np.maximum(n_b, 1) - 1), 0)
    else:
        rec["background"] = -1
    rec["bg_gain"] = (a["g_lo"] + (a["g_hi"] - a["g_lo"]) * unit(s0[2])).astype(np.float32)
    positive = unit(s0[3]) <= a["p_cough"]
    n_coughs = np.where(positive, _integers(unit(s1[0]), a["c_lo"], a["c_hi"]), 0)
    distracted = (unit(s1[1]) <= a["p_distractor"]) & (a["others"].size > 0)
    n_others = _integers(unit(s1[2]), 1, 2)
    if defect != "count_not_cut":
        n_others = np.minimum(n_others, SLOTS - n_coughs)
    n_others = np.where(distracted, n_others, 0)
    rec["n_events"] = n_coughs + n_others
    for e in range(SLOTS):
        d = block(2 + e)
        used = e < n_coughs + n_others
        is_cough = (e >= n_others) & used if defect == "distractors_first" else e < n_coughs
        cough = a["coughs"][_integers(unit(d[0]), 0, max(a["coughs"].size, 1) - 1)] if a["coughs"].size else np.full(b, -1)
        other = a["others"][_integers(unit(d[1]), 0, max(a["others"].size, 1) - 1)] if a["others"].size else np.full(b, -1)
        clip = np.where(used, np.where(is_cough, cough, other), -1)
        level = (d[2] & np.uint64(LEVELS - 1)) if defect == "level_from_low_bits" else d[2] >> np.uint64(22)
        n_c = np.where(used, a["ev_lengths"][np.maximum(clip, 0)] if a["ev_lengths"].size else 0, 0)
        m_c = np.minimum(a["m"], n_c)
        need = np.minimum(n_c, m_c if defect == "need_without_rho" else np.ceil(m_c / a["rho_min"]).astype(np.int64))
        highest = a["width"] - a["margin"] - need - (defect == "onset_range_one_short")
        onset = _integers(unit(d[3]), a["margin"] + need - n_c, highest)
        rec["clip"][:, e] = clip
        rec["onset"][:, e] = np.where(used, onset, 0)
        rec["snr_linear"][:, e] = np.where(used, a["snr"][level.astype(np.int64)], 1.0)
    return rec, (n_coughs > 0).astype(np.int64)


def same_records(x, y):
    """Bit for bit: the records as bytes."""
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.dtype == y.dtype == PLAN_DTYPE and x.shape == y.shape and x.tobytes() == y.tobytes()
