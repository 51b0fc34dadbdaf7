"""The scenes restated on the host (cough_detector_amd/scenes.py, csrc/scenes.hip): span powers, gains, the mix, the
window ranges of a truth event and the matcher -- plain Python and numpy, each of the last three written twice in
different ways so that the two forms can be held against each other."""
import math

import numpy as np

HIT, REPEAT, FALSE_ALARM = 0, 1, 2


# ------------------------------------------------------------------------------------------------ powers and gains
def span_ref(clip, start, n):
    """The ``n`` samples a span reads: ``clip[(start + i) mod len]``."""
    clip = np.asarray(clip, dtype=np.float32)
    return clip[(start + np.arange(n, dtype=np.int64)) % len(clip)] if n else clip[:0]


def power_ref(clip, start, n):
    """float64 mean of double(x)^2 over a span; 0.0 for an empty one."""
    if n == 0:
        return 0.0
    x = span_ref(clip, start, n).astype(np.float64)
    with np.errstate(all="ignore"):
        return float(np.sum(x * x) / n)


def gain_ref(snr_linear, bg_gain, p_bg, p_ev):
    """float32: the device's float64 operations in its order, rounded once; 1.0 where a power is 0 or not finite."""
    if p_bg == 0 or not math.isfinite(p_bg) or p_ev == 0 or not math.isfinite(p_ev):
        return np.float32(1.0)
    b = float(np.float32(bg_gain))
    with np.errstate(all="ignore"):
        return np.float32(np.sqrt(np.float64(((snr_linear * (b * b)) * p_bg) / p_ev)))


def fmaf(a, b, c):
    """float32 fused multiply-add, exactly rounded, of scalars or arrays.  The product of two float32 is exact in
    float64; its float64 sum ``s`` with ``c`` comes with its exact rounding error (TwoSum).  Rounding ``s`` to float32
    equals rounding the exact sum unless ``s`` lies exactly half way between two float32 values while the error is not
    zero: then the error's sign decides."""
    with np.errstate(all="ignore"):
        p = np.asarray(a, dtype=np.float32).astype(np.float64) * np.asarray(b, dtype=np.float32).astype(np.float64)
        c = np.asarray(c, dtype=np.float32).astype(np.float64)
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        r = s.astype(np.float32)
        other = np.nextafter(r, np.where(s > r, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
        tie = np.isfinite(s) & (s != r.astype(np.float64)) & (s == (r.astype(np.float64) + other.astype(np.float64)) / 2)
        fix = tie & (err != 0) & np.isfinite(err)
        up, down = np.maximum(r, other), np.minimum(r, other)
        return np.where(fix, np.where(err > 0, up, down), r).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the mix, twice
def mix_loop(bg, bg_start, bg_gain, length, events):
    """One scene, sample by sample.  ``events``: ``[(onset, samples float32, gain float32)]``."""
    bg, g = np.asarray(bg, dtype=np.float32), np.float32(bg_gain)
    out = np.empty(length, dtype=np.float32)
    with np.errstate(all="ignore"):
        for i in range(length):
            acc = np.float32(g * bg[(bg_start + i) % len(bg)])
            for onset, x, gain in events:
                if onset <= i < onset + len(x):
                    acc = fmaf(gain, x[i - onset], acc)
            out[i] = acc
    return out


def mix_slices(bg, bg_start, bg_gain, length, events):
    """The same scene by whole slices."""
    with np.errstate(all="ignore"):
        out = (np.float32(bg_gain) * span_ref(bg, bg_start, length)).astype(np.float32)
        for onset, x, gain in events:
            x = np.asarray(x, dtype=np.float32)
            out[onset:onset + len(x)] = fmaf(gain, x, out[onset:onset + len(x)])
    return out


# ------------------------------------------------------------------------------------------------ window ranges, twice
def least_windows(samples, hop):
    g = 0
    while g * hop < samples:
        g += 1
    return g


def min_overlap_samples(min_overlap_seconds, sr):
    return max(1, math.ceil(min_overlap_seconds * sr))


def ranges_closed(onset, offset, n_windows, hop, window, m, collar):
    """(k_lo, k_hi) of one event in a recording of ``n_windows`` windows: the closed forms.  The collar extends a range
    that holds a window; a range that holds none (k_lo > k_hi) stays as it is."""
    m_j = min(m, offset - onset)
    k_lo = max(0, -((window - onset - m_j) // hop))
    k_hi = min((offset - m_j) // hop, n_windows - 1)
    return (k_lo, min(k_hi + collar, n_windows - 1)) if k_lo <= k_hi else (k_lo, k_hi)


def ranges_brute(onset, offset, n_windows, hop, window, m, collar):
    """The same from the set ``{k : overlap(k, j) >= m_j}``; an empty set gives some range with k_lo > k_hi."""
    m_j = min(m, offset - onset)
    ks = [k for k in range(n_windows) if min(k * hop + window, offset) - max(k * hop, onset) >= m_j]
    if not ks:
        return None
    assert ks == list(range(ks[0], ks[-1] + 1))
    return ks[0], min(ks[-1] + collar, n_windows - 1)


# ------------------------------------------------------------------------------------------------ the matcher, twice
def match_walk(fired, k_lo, k_hi):
    """The pointer walk over ONE recording: ``fired`` ascending window indices -> (classes, hit_of) where ``hit_of[j]`` is
    the window that hit event ``j`` or -1."""
    ptr, last, classes, hit_of = 0, -1, [], [-1] * len(k_lo)
    for k in fired:
        while ptr < len(k_lo) and k_hi[ptr] < k:
            ptr += 1
        if ptr < len(k_lo) and k_lo[ptr] <= k:
            last, hit_of[ptr] = ptr, k
            ptr += 1
            classes.append(HIT)
        elif last >= 0 and k <= k_hi[last]:
            classes.append(REPEAT)
        else:
            classes.append(FALSE_ALARM)
    return classes, hit_of


def match_greedy(fired, k_lo, k_hi):
    """The same by brute force: every detection, in time order, goes to the earliest event nobody hit yet whose range
    holds it; failing that it repeats the event hit last if that one's range still reaches it."""
    hit_of, classes, last = [-1] * len(k_lo), [], -1
    for k in fired:
        holders = [j for j in range(len(k_lo)) if hit_of[j] < 0 and k_lo[j] <= k <= k_hi[j]]
        if holders:
            last = holders[0]
            hit_of[last] = k
            classes.append(HIT)
        elif last >= 0 and k <= k_hi[last]:
            classes.append(REPEAT)
        else:
            classes.append(FALSE_ALARM)
    return classes, hit_of


def match_ref(smoothed, thresholds, gap, truth_offsets, k_lo, k_hi, onset, hop, window, events_ref, walk=match_walk):
    """All recordings and thresholds: int arrays ``hits``, ``false_alarms``, ``repeats``, ``latency`` ``[n][T]``.
    ``events_ref`` is score_ref's decision (the windows that fire)."""
    n, T = len(smoothed), len(thresholds)
    out = {k: np.zeros((n, T), dtype=np.int64) for k in ("hits", "false_alarms", "repeats", "latency")}
    for c, s in enumerate(smoothed):
        a, b = int(truth_offsets[c]), int(truth_offsets[c + 1])
        for t, thr in enumerate(thresholds):
            fired = events_ref(s, thr, gap)
            classes, hit_of = walk(fired, list(k_lo[a:b]), list(k_hi[a:b]))
            out["hits"][c, t] = classes.count(HIT)
            out["repeats"][c, t] = classes.count(REPEAT)
            out["false_alarms"][c, t] = classes.count(FALSE_ALARM)
            out["latency"][c, t] = sum(k * hop + window - int(onset[a + j]) for j, k in enumerate(hit_of) if k >= 0)
    return out
