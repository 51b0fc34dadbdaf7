"""The arithmetic of ``include/cough_amd_pitch.h`` restated in numpy float64 (``cough_detector_amd/pitch.py``,
``csrc/pitch.hip``): the phase vocoder with its magnitude floor, twice -- in torchaudio's ``angle`` / ``cumsum`` form
and as a running product of unit phasors -- the first-order error bound that goes with it, and the pitch draw.

``stretch_ref`` returns, besides ``y_ref``, the per-sample bound ``E`` of the contract
``|y - y_ref| <= 2^-24 |y_ref| + E[m]``:

* an implementation's spectrum may differ from this one's by ``delta = 16 * 2^-53 * 256 * peak`` per bin (a float64 FFT
  of 512 points in another order moves a bin by a few 2^-53 of the spectrum's scale, 256 * peak);
* the unit phasor of a bin above the floor is then uncertain by ``delta / |S|``; one at or below the floor is (1, 0)
  exactly.  The accumulated phase of an output frame is uncertain by the sum over the steps that used those phasors;
* an output bin ``mag * P`` is uncertain by ``mag`` times that, plus ``delta`` for the interpolated magnitude;
* the inverse transform sums ``(E_0 + 2 sum E_k + E_256) / 512``; the window, the overlap-add and the division by the
  summed squared window are applied to the bound as they are to the signal.

It also returns the floor margin ``min over bins of ||S| - floor| / delta``: an input is fit for a comparison only if no
bin sits so close to the floor that two implementations could fall on different sides of it.

``draw_pitch_ref`` restates the pitch draw with ``tests/draws_ref.py``'s generator, one IEEE operation per operator.
"""
import math

import numpy as np

import draws_ref as D
import warp_ref as W

N_FFT, HOP, HALF, BINS = 512, 128, 256, 257
MAX_LEN, MAX_STEPS = 1 << 20, 12
WINDOW = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT) / N_FFT)
U24 = 2.0 ** -24


def stretchable(rate, n):
    return bool(0.5 <= rate <= 2.0 and rate != 1.0 and n >= HALF + 1)        # a NaN fails the comparisons


def stretched_length(n, rate):
    n = max(0, min(int(n), MAX_LEN))
    return int(np.rint(n / rate)) if stretchable(rate, n) else n


def pitch_rate(n_steps):
    return 2.0 ** (-n_steps / 12)


def spectra(xs):
    """(T, 257) complex: the centred, reflect-padded, Hann-windowed one-sided DFTs of the float64 row ``xs``."""
    n = xs.size
    padded = np.pad(xs, HALF, mode="reflect")
    T = 1 + n // HOP
    idx = (np.arange(T) * HOP)[:, None] + np.arange(N_FFT)[None, :]
    return np.fft.rfft(padded[idx] * WINDOW[None, :], axis=1)


def _overlap_add(frames, T_out):
    total = (T_out - 1) * HOP + N_FFT
    acc = np.zeros(total)
    for t in range(T_out):
        acc[t * HOP:t * HOP + N_FFT] += frames[t]
    return acc


def stretch_ref(x, shift, rate, form="phasor", floor=True, perturb=None):
    """-> dict(y float64 (n_s,), E float64 (n_s,), n_s, margin, peak).  ``form``: "phasor" or "angle"; ``floor=False``
    drops the magnitude floor (the formula two implementations cannot agree on); ``perturb``: a (T, 257) complex array
    added to the spectrum."""
    x = np.asarray(x, dtype=np.float32)[:MAX_LEN]
    n = x.size
    xs = W.shifted(x, shift).astype(np.float64)
    if not stretchable(rate, n):
        return dict(y=xs.copy(), E=np.zeros(n), n_s=n, margin=math.inf, peak=float(np.abs(xs).max()) if n else 0.0)
    n_s = int(np.rint(n / rate))
    if not np.isfinite(xs).all():
        return dict(y=np.full(n_s, np.nan), E=np.zeros(n_s), n_s=n_s, margin=math.inf, peak=math.nan)
    peak = float(np.abs(xs).max())
    if peak == 0.0:
        return dict(y=np.zeros(n_s), E=np.zeros(n_s), n_s=n_s, margin=math.inf, peak=0.0)
    S = spectra(xs)
    T = S.shape[0]
    if perturb is not None:
        S = S + perturb
    S = np.concatenate([S, np.zeros((2, BINS), dtype=complex)])              # frames T and T + 1 are zero
    mags = np.abs(S)
    delta = 16.0 * 2.0 ** -53 * 256.0 * peak
    level = 2.0 ** -24 * 256.0 * peak if floor else 0.0
    above = mags > level
    margin = float((np.abs(mags[:T] - level) / delta).min()) if floor else math.inf
    T_out = int(math.ceil(T / rate))
    ts = np.arange(T_out, dtype=np.float64) * rate
    i0 = np.floor(ts).astype(np.int64)
    a = (ts - i0)[:, None]
    mag = a * mags[i0 + 1] + (1.0 - a) * mags[i0]
    if form == "phasor":
        with np.errstate(invalid="ignore", divide="ignore"):
            u = np.where(above, S / np.where(above, mags, 1.0), 1.0 + 0.0j)
        step = u[i0 + 1] * np.conj(u[i0])
        P = np.empty((T_out, BINS), dtype=complex)
        P[0] = u[0]
        for t in range(T_out - 1):
            P[t + 1] = P[t] * step[t]
        Y = mag * P
    elif form == "angle":
        ang = np.where(above, np.angle(S), 0.0)
        advance = np.linspace(0.0, np.pi * HOP, BINS)[None, :]
        ph = ang[i0 + 1] - ang[i0] - advance
        ph = ph - 2.0 * np.pi * np.round(ph / (2.0 * np.pi))
        ph = ph + advance
        ph = np.concatenate([ang[:1], ph[:-1]])
        Y = mag * np.exp(1j * np.cumsum(ph, axis=0))
    else:
        raise ValueError(form)
    frames = np.fft.irfft(Y, n=N_FFT, axis=1) * WINDOW[None, :]
    env = _overlap_add(np.broadcast_to(WINDOW ** 2, (T_out, N_FFT)), T_out)
    acc = _overlap_add(frames, T_out)
    # the bound, pushed through the same steps
    with np.errstate(divide="ignore"):
        eu = np.where(above, delta / np.where(above, mags, 1.0), 0.0)
    per_step = eu[i0 + 1] + eu[i0]
    eP = eu[:1] + np.concatenate([np.zeros((1, BINS)), np.cumsum(per_step, axis=0)[:-1]])
    eY = mag * eP + delta
    e_frame = (eY[:, 0] + 2.0 * eY[:, 1:HALF].sum(axis=1) + eY[:, HALF]) / N_FFT
    e_acc = _overlap_add(e_frame[:, None] * WINDOW[None, :], T_out)
    y, E = np.zeros(n_s), np.zeros(n_s)
    have = min(n_s, acc.size - HALF)
    y[:have] = acc[HALF:HALF + have] / env[HALF:HALF + have]
    E[:have] = e_acc[HALF:HALF + have] / env[HALF:HALF + have]
    return dict(y=y, E=E, n_s=n_s, margin=margin, peak=peak, env_min=float(env[HALF:HALF + have].min()), frames=T)


def perturbation(x, shift, scale, seed):
    """A (T, 257) complex array of magnitude ``scale * 2^-53 * 256 * peak`` and random phase: what a float64 FFT that
    sums in another order does to the spectrum of the shifted row."""
    xs = W.shifted(np.asarray(x, dtype=np.float32), shift).astype(np.float64)
    T = 1 + xs.size // HOP
    rng = np.random.default_rng(seed)
    return scale * 2.0 ** -53 * 256.0 * float(np.abs(xs).max()) * np.exp(2j * np.pi * rng.random((T, BINS)))


def pitch_shift_ref(x, n_steps, sample_rate):
    """stretch by 2^(-n_steps / 12), resample from int(sample_rate / rate) to sample_rate, cut or pad to n."""
    x = np.asarray(x, dtype=np.float32)
    rate = pitch_rate(n_steps)
    y = stretch_ref(x, 0, rate)["y"].astype(np.float32)
    z = W.warp_ref(y, 0, int(sample_rate / rate), sample_rate)[0]
    out = np.zeros(x.size)
    out[:min(x.size, z.size)] = z[:x.size]
    return out


# ------------------------------------------------------------------------------------------------ the inputs of the tests
SAMPLE_RATE = 16000
R1, R2 = 2.0 ** (1 / 12), 2.0 ** (2 / 12)


def _burst(rng, n):
    """A cough-like burst between exact zeros."""
    x = np.zeros(n, dtype=np.float32)
    lo, hi = n // 4, n // 4 + max(n // 3, 1)
    k = np.arange(hi - lo)
    x[lo:hi] = (rng.standard_normal(hi - lo) * np.exp(-4.0 * k / max(hi - lo, 1)) * 0.6).astype(np.float32)
    return x


def _tone(n, hz=440.0, pad=True):
    x = (0.5 * np.sin(2.0 * np.pi * hz * np.arange(n) / SAMPLE_RATE)).astype(np.float32)
    if pad:
        x[:n // 5] = 0.0
        x[n - n // 6:] = 0.0
    return x


def make_cases(seed=20261019):
    """[(name, x float32, shift, rate)]: the ragged batch of tests/test_gpu_pitch.py -- every length at which the kernel
    takes another path (0, 1, 256 | 257: the reflect padding; 383 | 384, 511 | 512, 640: the frame count; 1000, 16000,
    48000: several frames, a second, three), every rate class (the four semitone rates, both ends of the range, 1, and
    3 and NaN which are refused), shifts inside and beyond the row, and the signals of the contract's special cases."""
    rng = np.random.default_rng(seed)
    noise = lambda n: (rng.random(n) - 0.5).astype(np.float32)                # noqa: E731
    nan = float("nan")
    cases = [
        ("empty", noise(0), 0, R1), ("one", noise(1), 0, R1), ("256", noise(256), 0, 1 / R1), ("256 shifted", noise(256), 37, R2),
        ("257", noise(257), 0, R1), ("257 slow", noise(257), -37, 0.5), ("383", noise(383), 0, 1 / R2), ("384", noise(384), 37, 2.0),
        ("511", noise(511), 0, R2), ("512", noise(512), -37, 1 / R1), ("640", noise(640), 0, 0.5), ("640 fast", noise(640), 0, 2.0),
        ("1000", noise(1000), 37, R1), ("1000 burst", _burst(rng, 1000), 0, 1 / R2),
        ("1000 rate 1", noise(1000), -37, 1.0), ("1000 rate 3", noise(1000), 37, 3.0), ("1000 rate nan", noise(1000), 0, nan),
        ("1000 shifted out", noise(1000), 5000, R1), ("1000 shifted out left", noise(1000), -(2 ** 31), 1 / R1),
        ("1000 dc", np.full(1000, 0.25, dtype=np.float32), 0, R2), ("1000 dc shifted", np.full(1000, -0.75, dtype=np.float32), 37, 1 / R2),
        ("1000 zeros", np.zeros(1000, dtype=np.float32), 0, R1),
        ("16000 noise", noise(16000), 0, R1), ("16000 burst", _burst(rng, 16000), -37, 1 / R1),
        ("16000 burst slow", _burst(rng, 16000), 0, R2), ("16000 tone", _tone(16000), 0, 1 / R2), ("16000 tone up", _tone(16000), 37, R2),
        ("16000 half", _burst(rng, 16000), 0, 0.5), ("16000 double", _tone(16000), 0, 2.0),
        ("48000 burst", _burst(rng, 48000), 37, 1 / R2), ("48000 noise", noise(48000), 0, R2),
    ]
    bad = noise(1000)
    bad[700] = nan
    cases.append(("1000 nan", bad, 0, R1))
    bad = noise(16000)
    bad[8000] = np.inf
    cases.append(("16000 inf", bad, -37, 1 / R1))
    bad = noise(1000)
    bad[998] = -np.inf
    cases.append(("1000 inf copied", bad, 0, 1.0))
    return cases


_REFS = {}


def case_refs(seed=20261019):
    """``make_cases`` with each row's ``stretch_ref`` result, computed once per process and shared by the tests."""
    if seed not in _REFS:
        _REFS[seed] = [(name, x, shift, rate, stretch_ref(x, shift, rate)) for name, x, shift, rate in make_cases(seed)]
    return _REFS[seed]


def pack(cases, gap=3):
    """The rows packed at odd offsets into one float32 buffer with NaN between them -> (buffer, offsets int64)."""
    parts, offs, at = [np.full(1, np.nan, dtype=np.float32)], [], 1
    for _, x, _, _ in cases:
        offs.append(at)
        parts += [x, np.full(gap + (x.size + gap + at) % 2, np.nan, dtype=np.float32)]
        at += x.size + parts[-1].size
    return np.concatenate(parts), np.asarray(offs, dtype=np.int64)


# ------------------------------------------------------------------------------------------------ the pitch draw
def step_table(lo, hi, sample_rate):
    """[(rate, orig)] for n_steps = lo .. hi: what the host hands ``cough_draw_pitch``."""
    return [(pitch_rate(s), int(sample_rate / pitch_rate(s))) for s in range(lo, hi + 1)]


def draw_pitch_ref(seed, lengths, p, lo, hi, sample_rate):
    """-> (rates float64 (B,), warp plans int32 (B, 3), stretched lengths int32 (B,), n_steps int32 (B,), fired)."""
    n = np.minimum(np.asarray(lengths, dtype=np.int64), MAX_LEN)
    rows = np.arange(n.size, dtype=np.uint64)
    seed = int(seed) & (2**64 - 1)
    key = (seed & 0xFFFFFFFF, seed >> 32)
    zero = np.zeros(rows.shape, dtype=np.uint64)
    d = [D.unit(w) for w in D.philox4x32_10((zero, rows, 0, 3), key)]
    fired = (d[0] <= p) & (n >= 1)
    steps = np.where(fired, lo + (float(hi - lo + 1) * d[1]).astype(np.int32), 0).astype(np.int32)
    table = step_table(lo, hi, sample_rate)
    rates = np.array([table[s - lo][0] if s != 0 else 1.0 for s in steps], dtype=np.float64)
    plans = np.zeros((n.size, 3), dtype=np.int32)
    plans[:, 1] = [table[s - lo][1] if s != 0 else sample_rate for s in steps]
    plans[:, 2] = sample_rate
    n_s = np.array([stretched_length(v, r) if v >= 1 else 0 for v, r in zip(n, rates)], dtype=np.int32)
    return rates, plans, n_s, steps, fired
