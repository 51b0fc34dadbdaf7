"""The offline scorer restated on the host (cough_detector_amd/score.py, csrc/score.hip): the windows of a recording,
the engine's deque mean, the debounce gap, the decision at a threshold, the sweep, the peak and the report -- plain Python
and numpy, a window at a time, as the reference's ``process_audio_chunk`` writes them."""
import math
from collections import deque

import numpy as np

CLASSES = ["non_cough", "cough"]


def windows_per_clip(n, window, hop):
    return 0 if n < window else 1 + (n - window) // hop


def smooth_ref(p, w):
    """float64 [len(p)]: ``float(np.mean(history))`` over a ``deque(maxlen=w)`` of the float32 probabilities of ONE recording."""
    history = deque(maxlen=w)
    out = np.empty(len(p), dtype=np.float64)
    for k, v in enumerate(np.asarray(p, dtype=np.float32)):
        history.append(float(v))
        out[k] = float(np.mean(history))
    return out


def ordered_sum(a):
    """The order rule 3 states for <= 32 float64 values (what the device does), one addition at a time."""
    a = [float(v) for v in a]
    n = len(a)
    if n < 8:
        total = a[0]
        for v in a[1:]:
            total = total + v
        return total
    r = a[:8]
    whole = n - n % 8
    for i in range(8, whole, 8):
        for j in range(8):
            r[j] = r[j] + a[i + j]
    total = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for v in a[whole:]:
        total = total + v
    return total


def gap_ref(debounce_seconds, sample_rate, hop):
    need = float(debounce_seconds) * sample_rate
    g = 1
    while g * hop < need:
        g += 1
    return g


def events_ref(s, t, gap):
    """The window indices of ONE recording that fire at threshold ``t``."""
    fired, last = [], None
    for k, v in enumerate(s):
        if v >= t and (last is None or k - last >= gap):
            fired.append(k)
            last = k
    return fired


def peak_ref(s):
    best, at = math.nan, -1
    for k, v in enumerate(s):
        if not math.isnan(v) and (at < 0 or v > best):
            best, at = float(v), k
    return best, at


def sweep_ref(smoothed, thresholds, gap):
    """``smoothed``: one float64 array per recording -> counts and first_window (int lists [n][T]), peak_conf, peak_window."""
    counts, first, peak_conf, peak_window = [], [], [], []
    for s in smoothed:
        fired = [events_ref(s, t, gap) for t in thresholds]
        counts.append([len(f) for f in fired])
        first.append([f[0] if f else -1 for f in fired])
        best, at = peak_ref(s)
        peak_conf.append(best)
        peak_window.append(at)
    return dict(counts=counts, first_window=first, peak_conf=peak_conf, peak_window=peak_window)


def table_ref(smoothed, t, gap, hop, window, sample_rate):
    """The event table at one threshold: by recording, then time."""
    tab = dict(clip=[], window=[], time=[], confidence=[], counts=[])
    for c, s in enumerate(smoothed):
        fired = events_ref(s, t, gap)
        tab["counts"].append(len(fired))
        for k in fired:
            tab["clip"].append(c)
            tab["window"].append(k)
            tab["time"].append((k * hop + window) / sample_rate)
            tab["confidence"].append(float(s[k]))
    return tab


def report_ref(lengths, labels, smoothed, thresholds, gap, sample_rate):
    sweep = sweep_ref(smoothed, thresholds, gap)
    out = {}
    for label, name in enumerate(CLASSES):
        mine = [c for c in range(len(labels)) if labels[c] == label]
        minutes = float(sum(int(lengths[c]) for c in mine)) / sample_rate / 60.0
        events = [sum(sweep["counts"][c][j] for c in mine) for j in range(len(thresholds))]
        hit = [sum(1 for c in mine if sweep["counts"][c][j] > 0) for j in range(len(thresholds))]
        out[name] = dict(recordings=len(mine), minutes=minutes, events=events,
                         events_per_minute=[e / minutes if minutes > 0 else None for e in events],
                         recordings_with_event=hit, share_with_event=[h / len(mine) if mine else None for h in hit])
    return out
