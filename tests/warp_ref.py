"""The arithmetic of ``include/cough_amd_warp.h`` restated in numpy float64 (``cough_detector_amd/warp.py``,
``csrc/warp.hip``): the per-tap windowed-sinc coefficient, the resampled row with the time shift fused into its read,
and the speed draw.

``warp_ref`` keeps everything in float64 except the coefficient, which is rounded once to float32 as the contract
says; it returns per output ``y_ref`` and ``A_m = sum_i |x_s[i]| |h_i|``, the scale of the per-sample bound
``|y - y_ref| <= (2 * width + 4) * 2^-24 * A_m``:

* 2 u for a coefficient that the device may round one float32 away from this one (its sin / cos come from a float64
  rotation, this one's from numpy's), u = 2^-24;
* (2 * width + 1) u for the float32 fma chain of 2 * width + 2 taps (one rounding per tap, each at most u of the
  partial sum, which is at most A_m (1 + small));
* one more u of slack for the second-order terms.

``draw_speed_ref`` restates the speed draw with ``tests/draws_ref.py``'s generator, one IEEE operation per operator.
"""
import math

import numpy as np

import draws_ref as D

ROLLOFF, LOWPASS = 0.99, 6
MAX_RATE, MAX_RATIO, MAX_LEN = 1 << 20, 4, 1 << 30
U = 2.0 ** -24


def usable(orig, new):
    return 1 <= orig <= MAX_RATE and 1 <= new <= MAX_RATE and orig <= MAX_RATIO * new and new <= MAX_RATIO * orig


def filter_width(orig, new):
    """ceil(6 * orig / (0.99 * min(orig, new))) in float64."""
    return math.ceil(LOWPASS * orig / (min(orig, new) * ROLLOFF))


def new_length(n, orig, new):
    """ceil(n * new / orig) in exact integer arithmetic."""
    return (int(n) * int(new) + int(orig) - 1) // int(orig)


def bound_factor(orig, new):
    return (2 * filter_width(orig, new) + 4) * U


def coefficient(num, orig, new):
    """h for num = i * new - m * orig (an integer array): float64 arithmetic, rounded once to float32."""
    base = min(orig, new) * ROLLOFF
    c = base / (float(orig) * float(new))
    t = np.clip(np.asarray(num, dtype=np.int64).astype(np.float64) * c, -float(LOWPASS), float(LOWPASS))
    window = np.cos(t * math.pi / LOWPASS / 2) ** 2
    tp = t * math.pi
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(tp == 0, 1.0, np.sin(tp) / tp)
    return (sinc * (window * (base / orig))).astype(np.float32)


def shifted(x, shift):
    """x_s[i] = x[i - shift] for 0 <= i - shift < n, else 0; any shift."""
    x = np.asarray(x)
    n = x.size
    out = np.zeros_like(x)
    s = max(-n, min(n, int(shift)))
    if s >= 0:
        out[s:] = x[:n - s]
    else:
        out[:n + s] = x[-s:]
    return out


def warp_ref(x, shift, orig, new):
    """-> (y_ref float64 (n',), A float64 (n',), n').  A pair the kernel cannot use counts as orig == new."""
    x = np.asarray(x, dtype=np.float32)
    n = x.size
    xs = shifted(x, shift).astype(np.float64)
    if not usable(orig, new) or orig == new:
        return xs.copy(), np.abs(xs), n
    n_new = new_length(n, orig, new)
    w = filter_width(orig, new)
    m = np.arange(n_new, dtype=np.int64)
    i = (m * orig // new)[:, None] + np.arange(-w, w + 2, dtype=np.int64)[None, :]
    h = coefficient(i * new - m[:, None] * orig, orig, new).astype(np.float64)
    inside = (i >= 0) & (i < n)
    xv = np.where(inside, xs[np.clip(i, 0, max(n - 1, 0))] if n else 0.0, 0.0)
    return (xv * h).sum(axis=1), (np.abs(xv) * np.abs(h)).sum(axis=1), n_new


def draw_speed_ref(seed, lengths, p, lo, hi, sample_rate):
    """-> (plans int32 (B, 3): shift, orig, new; new lengths int32 (B,); fired: dict of the two coins)."""
    n = np.minimum(np.asarray(lengths, dtype=np.int64), MAX_LEN)
    rows = np.arange(n.size, dtype=np.uint64)
    seed = int(seed) & (2**64 - 1)
    key = (seed & 0xFFFFFFFF, seed >> 32)
    zero = np.zeros(rows.shape, dtype=np.uint64)
    s0 = [D.unit(w) for w in D.philox4x32_10((zero, rows, 0, 1), key)]
    sp = [D.unit(w) for w in D.philox4x32_10((zero, rows, 0, 2), key)]
    live = n >= 1
    f_shift, f_speed = (s0[0] <= p) & live, (sp[0] <= p) & live
    shift = (n.astype(np.float64) * (-0.2 + 0.4 * s0[1])).astype(np.int32)             # astype truncates toward zero
    factor = lo + (hi - lo) * sp[1]
    orig = (factor * float(sample_rate)).astype(np.int32)
    plans = np.zeros((n.size, 3), dtype=np.int32)
    plans[:, 0] = np.where(f_shift, shift, 0)
    plans[:, 1] = np.where(f_speed, orig, sample_rate)
    plans[:, 2] = sample_rate
    o = plans[:, 1].astype(np.int64)
    n_new = np.where(live, (n * sample_rate + o - 1) // np.maximum(o, 1), 0)
    return plans, np.minimum(n_new, MAX_LEN).astype(np.int32), {"shift": f_shift, "speed": f_speed}
