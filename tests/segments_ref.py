"""The segment finder of cough_detector_amd/segments.py restated in numpy, float64 throughout, one clip at a time.

``frame_energy_ref`` and ``segments_ref`` follow the specification step by step.  For every decision the algorithm
takes, ``segments_ref`` also returns the RELATIVE MARGIN by which it was taken -- each ``e[f]`` against the activity
threshold, ``E_max`` against the floor, a kept run's largest energy against its runner-up -- and ``margin`` is the
smallest of them.  A device sum of 400 float64 terms in another order moves an energy by about 5e-14 relative; a test
that uses only inputs whose margin exceeds 1e-9 may therefore demand the same decisions, index for index.
"""
import math

import numpy as np

DEFAULTS = dict(frame_length=400, hop_length=160, threshold_db=-30.0, floor_db=-60.0, min_duration=0.1, max_segments=8)


def n_frames(n, frame_length, hop_length):
    return 1 if n < frame_length else 1 + (n - frame_length) // hop_length


def frame_energy_ref(x, frame_length=400, hop_length=160):
    """e[f] = sum(double(x[i])**2 over frame f) / (samples of frame f), float64 [n_frames]."""
    sq = np.asarray(x, dtype=np.float64) ** 2
    n = sq.size
    if n < frame_length:
        return np.array([sq.sum() / n])
    starts = np.arange(n_frames(n, frame_length, hop_length), dtype=np.int64) * hop_length
    with np.errstate(invalid="ignore", over="ignore"):
        return np.array([sq[s:s + frame_length].sum() for s in starts]) / frame_length


def _rel(a, b):
    """|a - b| relative to the larger magnitude (1.0 when both are 0 would be a tie: returned as 0)."""
    m = max(abs(a), abs(b))
    return abs(a - b) / m if m > 0 else 0.0


def segments_ref(x, seg_len, sample_rate, frame_length=400, hop_length=160, threshold_db=-30.0, floor_db=-60.0,
                 min_duration=0.1, max_segments=8):
    """-> dict(start=[...], length=[...], peak_db=[float32 ...], margin=float, energy=e)."""
    x = np.asarray(x)
    n = x.size
    e = frame_energy_ref(x, frame_length, hop_length)
    out = dict(start=[], length=[], peak_db=[], margin=math.inf, energy=e)
    if not np.isfinite(e).all():
        return out                                                # a non-finite sample is no close call
    e_max = float(e.max())
    floor = 10.0 ** (floor_db / 10.0)
    out["margin"] = min(out["margin"], _rel(e_max, floor))
    if e_max < floor:
        if e_max == 0.0:
            out["margin"] = math.inf                              # the all-zero clip: the one allowed tie
        return out
    r = 10.0 ** (threshold_db / 10.0)
    thr = e_max * r
    active = e >= thr
    out["margin"] = min(out["margin"], min(_rel(float(v), thr) for v in e))
    min_frames = max(1, math.ceil(min_duration * sample_rate / hop_length))
    runs, f = [], 0
    while f < e.size:
        if not active[f]:
            f += 1
            continue
        g = f
        while g < e.size and active[g]:
            g += 1
        if g - f >= min_frames:
            runs.append((f, g))
        f = g
    last_end = None
    for lo, hi in runs:
        if len(out["start"]) >= max_segments:
            break
        p = lo + int(np.argmax(e[lo:hi]))                         # argmax: the first of equal values
        others = np.delete(e[lo:hi], p - lo)
        if others.size:
            out["margin"] = min(out["margin"], _rel(float(e[p]), float(others.max())))
        c = p * hop_length + frame_length // 2
        length = min(seg_len, n)
        start = min(max(c - seg_len // 2, 0), max(n - seg_len, 0))
        if last_end is not None and start < last_end:
            continue
        out["start"].append(start)
        out["length"].append(length)
        with np.errstate(divide="ignore"):
            out["peak_db"].append(np.float32(10.0 * np.log10(e[p])))
        last_end = start + length
    return out


def table_ref(clips, seg_len, sample_rate, **params):
    """The whole table for a list of clips: dict(counts, clip, start, length, peak_db, margin)."""
    tab = dict(counts=[], clip=[], start=[], length=[], peak_db=[], margin=math.inf)
    for k, x in enumerate(clips):
        r = segments_ref(x, seg_len, sample_rate, **params)
        tab["counts"].append(len(r["start"]))
        tab["clip"] += [k] * len(r["start"])
        for key in ("start", "length", "peak_db"):
            tab[key] += r[key]
        tab["margin"] = min(tab["margin"], r["margin"])
    return tab


# ------------------------------------------------------------------------------------------------ hand-built clips
def burst(rng, length, amplitude=0.3):
    """Noise under a Hann envelope: one peak, near the middle."""
    return (amplitude * np.hanning(length) * rng.standard_normal(length)).astype(np.float32)


def recording(rng, n, bursts, background=1e-4):
    """``n`` samples of faint noise (80 dB below the bursts' peak: never active) with ``bursts`` = [(centre, length)]
    or [(centre, length, amplitude)] added."""
    x = (background * rng.standard_normal(n)).astype(np.float32)
    for b in bursts:
        centre, length = b[0], b[1]
        lo = centre - length // 2
        x[lo:lo + length] += burst(rng, length, *(b[2:]))
    return x


def case_clips(seed=0, seg_len=16000):
    """{name: clip}: the cases the finder has to get right, at ``seg_len`` = 16000 and the default parameters."""
    rng = np.random.default_rng(seed)
    clips = {
        "middle": recording(rng, 80000, [(40000, 4000)]),
        "start_and_end": recording(rng, 64000, [(2500, 4000), (61500, 4000)]),
        "two_close": recording(rng, 80000, [(30000, 4000), (38000, 4000)]),
        "many": recording(rng, 160000, [(8000 + 17000 * k, 4000) for k in range(9)]),
        "click": recording(rng, 40000, [(20000, 8)]),
        "short": recording(rng, 8000, [(4000, 3000)]),
        "silent": np.zeros(24000, dtype=np.float32),
    }
    return clips
