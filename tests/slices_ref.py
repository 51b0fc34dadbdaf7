"""The window decision of cough_detector_amd/slices.py (include/cough_amd_slices.h) restated in numpy from the float64
frame energies, one clip at a time -- twice.

``clip_closed`` uses what the kernel uses: closed forms for a window's first and last frame and a prefix sum of the
activity.  ``clip_brute`` uses only the definitions: it walks every (window, frame) pair, asks whether the frame's extent
lies inside the window's, and caps by a plain sort on ``(-m, w)``.  tests/test_slices_host.py holds the two against each
other; the GPU tests hold the kernels against ``clip_closed`` on the device's own energies, so every comparison the
kernel makes is made here on the same float64 values, in the same single operations (one product for the threshold, one
for the share): integers and bits must be equal, no tolerance.
"""
import math

import numpy as np

DEFAULTS = dict(frame_length=400, hop_length=160, threshold_db=-30.0, floor_db=-60.0, min_active=0.5)


def n_frames(n, frame_length, hop_length):
    return 1 if n < frame_length else 1 + (n - frame_length) // hop_length


def n_windows(n, seg_len, stride):
    return 1 if n < seg_len else 1 + (n - seg_len) // stride


def window_extent(w, n, seg_len, stride):
    return (0, n) if n < seg_len else (w * stride, w * stride + seg_len)


def frame_extent(f, n, frame_length, hop_length):
    return f * hop_length, min(f * hop_length + frame_length, n)


def levels(threshold_db=-30.0, floor_db=-60.0):
    """(ratio, floor) as the Python side forms them."""
    return 10.0 ** (float(threshold_db) / 10.0), 10.0 ** (float(floor_db) / 10.0)


def _activity(e, ratio, floor):
    """-> (peak, active bool [F] or None when the clip is gated)"""
    e = np.asarray(e, dtype=np.float64)
    if not np.isfinite(e).all():
        return math.nan, None
    e_max = float(e.max())
    if e_max < floor:
        return e_max, None
    thr = max(e_max * ratio, floor)                              # one double product
    return e_max, e >= thr


def _qualifies(m, cnt, min_active):
    return m >= 1 and float(m) >= min_active * float(cnt)        # one double product


def clip_closed(e, n, frame_length, hop_length, seg_len, stride, ratio, floor, min_active, cap=None):
    """-> dict(peak, clip_active, m [W], cnt [W], keep [W] 0/1, count)"""
    F, W = n_frames(n, frame_length, hop_length), n_windows(n, seg_len, stride)
    assert len(e) == F and seg_len >= frame_length
    peak, active = _activity(e, ratio, floor)
    first, last = np.zeros(W, dtype=np.int64), np.zeros(W, dtype=np.int64)
    if n >= frame_length:
        w = np.arange(W, dtype=np.int64)
        a = w * stride
        b = a + min(seg_len, n)
        first = -((-a) // hop_length)
        last = np.minimum((b - frame_length) // hop_length, F - 1)
    cnt = np.maximum(last - first + 1, 0)
    m, keep = np.zeros(W, dtype=np.int64), np.zeros(W, dtype=np.int64)
    if active is None:
        return dict(peak=peak, clip_active=0, m=m, cnt=cnt, keep=keep, count=0)
    below = np.concatenate([[0], np.cumsum(active)])             # active frames in front of frame f
    has = cnt > 0
    m[has] = below[last[has] + 1] - below[first[has]]
    q = np.array([_qualifies(int(m[w]), int(cnt[w]), min_active) for w in range(W)], dtype=bool)
    idx = np.flatnonzero(q)
    if cap is not None and idx.size > cap:
        idx = idx[np.argsort(-m[idx], kind="stable")[:cap]]      # stable: ties go to the earlier window
    keep[idx] = 1
    return dict(peak=peak, clip_active=int(active.sum()), m=m, cnt=cnt, keep=keep, count=int(keep.sum()))


def clip_brute(e, n, frame_length, hop_length, seg_len, stride, ratio, floor, min_active, cap=None):
    """The same by the set definition: a loop over every (window, frame) pair."""
    F, W = n_frames(n, frame_length, hop_length), n_windows(n, seg_len, stride)
    peak, active = _activity(e, ratio, floor)
    m, cnt, keep = [0] * W, [0] * W, [0] * W
    for w in range(W):
        a, b = window_extent(w, n, seg_len, stride)
        for f in range(F):
            lo, hi = frame_extent(f, n, frame_length, hop_length)
            if a <= lo and hi <= b:
                cnt[w] += 1
                if active is not None and active[f]:
                    m[w] += 1
    count = 0
    if active is not None:
        order = sorted((-m[w], w) for w in range(W) if _qualifies(m[w], cnt[w], min_active))
        for _, w in (order if cap is None else order[:cap]):
            keep[w] = 1
        count = sum(keep)
    return dict(peak=peak, clip_active=0 if active is None else int(np.sum(active)), m=np.array(m, dtype=np.int64),
                cnt=np.array(cnt, dtype=np.int64), keep=np.array(keep, dtype=np.int64), count=count)


def table_ref(energies, lengths, seg_len, stride, frame_length=400, hop_length=160, threshold_db=-30.0, floor_db=-60.0,
              min_active=0.5, cap=None, clip_fn=clip_closed):
    """The whole answer for a bank: per window ``active`` and ``keep`` (concatenated in clip order), per clip ``counts``,
    ``clip_active``, ``peak`` and ``windows``, and the rows ``clip`` / ``start`` / ``length`` / ``row_active``."""
    ratio, floor = levels(threshold_db, floor_db)
    out = dict(active=[], keep=[], counts=[], clip_active=[], peak=[], windows=[], clip=[], start=[], length=[],
               row_active=[])
    for k, (e, n) in enumerate(zip(energies, lengths)):
        r = clip_fn(e, int(n), frame_length, hop_length, seg_len, stride, ratio, floor, float(min_active), cap)
        out["active"] += r["m"].tolist()
        out["keep"] += r["keep"].tolist()
        out["counts"].append(r["count"])
        out["clip_active"].append(r["clip_active"])
        out["peak"].append(r["peak"])
        out["windows"].append(len(r["m"]))
        for w in np.flatnonzero(r["keep"]):
            out["clip"].append(k)
            out["start"].append(int(w) * stride)
            out["length"].append(min(seg_len, int(n)))
            out["row_active"].append(int(r["m"][w]))
    return out
