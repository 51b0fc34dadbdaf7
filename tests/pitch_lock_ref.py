"""The locked stretch of ``include/cough_amd_pitch.h`` (mode bit 0, identity phase locking after Laroche & Dolson)
restated in numpy float64 on top of ``tests/pitch_ref.py``: everything this file does not name -- the frames, the floor,
``u()``, ``mag``, the inverse transform, the overlap-add, the envelope, the special rows -- is ``pitch_ref``'s.

``stretch_lock_ref`` returns, besides ``y_ref``, the first-order bound ``E_lock`` of the contract
``|y - y_ref| <= 2^-24 |y_ref| + E_lock[m]``: the plain bound's ``delta`` and ``eu``, with the phase of a bin that a peak
owns uncertain by the peak's accumulated phase plus the two phasors that tie it to the peak.

Two implementations can only agree when they pick the same peaks, so the result also holds the peak margin: the least
``|m_k| / delta`` over the bins above the floor, where ``m_k = min(M[k] - floor, min over neighbours (M[k] - M[j]) / 2)``
is what a perturbation must overcome to flip the decision on bin ``k``.
"""
import math

import numpy as np

import pitch_ref as P
import warp_ref as W
from pitch_ref import BINS, HALF, HOP, N_FFT, R1, R2, SAMPLE_RATE, WINDOW

PHASE_LOCK = 1
REACH = 2                                   # a peak exceeds its neighbours up to this many bins away


def _neighbours(M):
    """(T, 257, 4): M[j] for j in k-2, k-1, k+1, k+2, -inf where j is not a bin."""
    pad = np.pad(M, ((0, 0), (REACH, REACH)), constant_values=-np.inf)
    return np.stack([pad[:, REACH + d:REACH + d + BINS] for d in (-2, -1, 1, 2)], axis=2)


def peaks_of(M, level):
    """(T, 257) bool: bin k is a peak when M[k] > floor and M[k] > M[j] for the existing j within two bins."""
    return (M > level) & (M[:, :, None] > _neighbours(M)).all(axis=2)


def owners(is_peak):
    """(T, 257) int: the nearest peak of every bin, the lower one on a tie; the bin itself in a frame without peaks."""
    own = np.tile(np.arange(BINS), (is_peak.shape[0], 1))
    k = np.arange(BINS)
    for f in range(is_peak.shape[0]):
        p = np.flatnonzero(is_peak[f])
        if p.size == 0:
            continue
        at = np.searchsorted(p, k)                                         # the first peak >= k
        below, above = p[np.maximum(at - 1, 0)], p[np.minimum(at, p.size - 1)]
        below = np.where(at == 0, above, below)
        above = np.where(at == p.size, below, above)
        own[f] = np.where(np.abs(k - below) <= np.abs(above - k), below, above)
    return own


def stretch_lock_ref(x, shift, rate, perturb=None):
    """-> dict(y float64 (n_s,), E float64 (n_s,), n_s, margin, peak_margin, peak, peaks_per_frame)."""
    x = np.asarray(x, dtype=np.float32)[:P.MAX_LEN]
    n = x.size
    xs = W.shifted(x, shift).astype(np.float64)
    blank = dict(margin=math.inf, peak_margin=math.inf, peaks_per_frame=0.0)
    if not P.stretchable(rate, n):
        return dict(y=xs.copy(), E=np.zeros(n), n_s=n, peak=float(np.abs(xs).max()) if n else 0.0, **blank)
    n_s = int(np.rint(n / rate))
    if not np.isfinite(xs).all():
        return dict(y=np.full(n_s, np.nan), E=np.zeros(n_s), n_s=n_s, peak=math.nan, **blank)
    peak = float(np.abs(xs).max())
    if peak == 0.0:
        return dict(y=np.zeros(n_s), E=np.zeros(n_s), n_s=n_s, peak=0.0, **blank)
    S = P.spectra(xs)
    T = S.shape[0]
    if perturb is not None:
        S = S + perturb
    S = np.concatenate([S, np.zeros((2, BINS), dtype=complex)])              # frames T and T + 1 are zero
    mags = np.abs(S)
    delta = 16.0 * 2.0 ** -53 * 256.0 * peak
    level = 2.0 ** -24 * 256.0 * peak
    above = mags > level
    margin = float((np.abs(mags[:T] - level) / delta).min())
    # the peaks and what it takes to flip a decision
    M = mags[:T]
    is_peak = np.concatenate([peaks_of(M, level), np.zeros((2, BINS), dtype=bool)])
    m = np.minimum(M - level, ((M[:, :, None] - _neighbours(M)) / 2.0).min(axis=2))
    assert ((m > 0) == is_peak[:T])[above[:T]].all()
    peak_margin = float((np.abs(m[above[:T]]) / delta).min())
    own = owners(is_peak)
    bins = np.arange(BINS)

    T_out = int(math.ceil(T / rate))
    ts = np.arange(T_out, dtype=np.float64) * rate
    i0 = np.floor(ts).astype(np.int64)
    a = (ts - i0)[:, None]
    mag = a * mags[i0 + 1] + (1.0 - a) * mags[i0]
    with np.errstate(invalid="ignore", divide="ignore"):
        u = np.where(above, S / np.where(above, mags, 1.0), 1.0 + 0.0j)
        eu = np.where(above, delta / np.where(above, mags, 1.0), 0.0)
    Q = np.empty((T_out, BINS), dtype=complex)
    eQ = np.empty((T_out, BINS))
    R, eR = u[0].copy(), eu[0].copy()
    for t in range(T_out):
        f = i0[t]
        p = own[f]
        led = p != bins
        Q[t] = np.where(led, R[p] * u[f] * np.conj(u[f][p]), R)
        eQ[t] = np.where(led, eR[p] + eu[f] + eu[f][p], eR)
        R = Q[t] * u[f + 1] * np.conj(u[f])
        eR = eQ[t] + eu[f + 1] + eu[f]
    Y = mag * Q
    eY = mag * eQ + delta
    frames = np.fft.irfft(Y, n=N_FFT, axis=1) * WINDOW[None, :]
    env = P._overlap_add(np.broadcast_to(WINDOW ** 2, (T_out, N_FFT)), T_out)
    acc = P._overlap_add(frames, T_out)
    e_frame = (eY[:, 0] + 2.0 * eY[:, 1:HALF].sum(axis=1) + eY[:, HALF]) / N_FFT
    e_acc = P._overlap_add(e_frame[:, None] * WINDOW[None, :], T_out)
    y, E = np.zeros(n_s), np.zeros(n_s)
    have = min(n_s, acc.size - HALF)
    y[:have] = acc[HALF:HALF + have] / env[HALF:HALF + have]
    E[:have] = e_acc[HALF:HALF + have] / env[HALF:HALF + have]
    return dict(y=y, E=E, n_s=n_s, margin=margin, peak_margin=peak_margin, peak=peak,
                peaks_per_frame=float(is_peak[:T].sum(axis=1).mean()), telescopes=bool((i0 == np.arange(T_out)).all()))


def pitch_shift_lock_ref(x, n_steps, sample_rate):
    """``pitch_ref.pitch_shift_ref`` with the locked stretch."""
    x = np.asarray(x, dtype=np.float32)
    rate = P.pitch_rate(n_steps)
    y = stretch_lock_ref(x, 0, rate)["y"].astype(np.float32)
    z = W.warp_ref(y, 0, int(sample_rate / rate), sample_rate)[0]
    out = np.zeros(x.size)
    out[:min(x.size, z.size)] = z[:x.size]
    return out


# ------------------------------------------------------------------------------------------------ the inputs of the tests
def _sines(n, parts, pad=True):
    """A sum of ``(hz, amplitude, phase)`` sines between exact zeros."""
    i = np.arange(n)
    x = sum(amp * np.sin(2.0 * np.pi * hz * i / SAMPLE_RATE + ph) for hz, amp, ph in parts).astype(np.float32)
    if pad:
        x[:n // 5] = 0.0
        x[n - n // 6:] = 0.0
    return x


BIN_HZ = SAMPLE_RATE / N_FFT                # 31.25


def lock_cases(seed=20261019):
    """``pitch_ref.make_cases()`` plus the rows that exercise the peaks: two tones far apart, a harmonic stack whose
    partials lie under five bins apart (the +-2 windows of neighbouring peaks interact), and two tones on bin centres
    an even number of bins apart, so that the bin halfway is tied and goes to the lower peak."""
    stack = [(147.3 * h, 0.4 / h, 0.7 * h) for h in range(1, 13)]
    tied = [(40 * BIN_HZ, 0.40, 0.3), (46 * BIN_HZ, 0.31, 1.1)]
    return P.make_cases(seed) + [
        ("8000 two tones", _sines(8000, [(440.0, 0.45, 0.0), (1730.0, 0.30, 0.5)]), 0, 1 / R2),
        ("8000 stack", _sines(8000, stack), 37, 1 / R2),
        ("8000 stack down", _sines(8000, stack, pad=False), 0, R2),
        ("6000 tie", _sines(6000, tied, pad=False), 0, 1 / R2),
    ]


_REFS = {}


def lock_refs(seed=20261019):
    """``lock_cases`` with each row's locked and plain restatement, computed once per process:
    ``[(name, x, shift, rate, locked, plain)]``."""
    if seed not in _REFS:
        _REFS[seed] = [(name, x, shift, rate, stretch_lock_ref(x, shift, rate), P.stretch_ref(x, shift, rate))
                       for name, x, shift, rate in lock_cases(seed)]
    return _REFS[seed]


# ------------------------------------------------------------------------------------------------ the pitch draw
def step_table(lo, hi, sample_rate, modes=None):
    """[(rate, orig, mode word)] for n_steps = lo .. hi; ``modes``: one word for all, or one per entry."""
    if modes is None or isinstance(modes, int):
        modes = [modes or 0] * (hi - lo + 1)
    return [(r, o, int(m)) for (r, o), m in zip(P.step_table(lo, hi, sample_rate), modes)]


def draw_pitch_lock_ref(seed, lengths, p, lo, hi, sample_rate, modes=None):
    """``pitch_ref.draw_pitch_ref`` and the mode the draw writes into each stretch plan: bit 0 of the drawn entry's word
    when the coin fired with ``n_steps != 0``, else 0 -> (rates, warp plans, stretched lengths, n_steps, fired, modes)."""
    rates, plans, n_s, steps, fired = P.draw_pitch_ref(seed, lengths, p, lo, hi, sample_rate)
    table = step_table(lo, hi, sample_rate, modes)
    mode = np.array([table[s - lo][2] & 1 if fi and s != 0 else 0 for s, fi in zip(steps, fired)], dtype=np.int32)
    return rates, plans, n_s, steps, fired, mode
