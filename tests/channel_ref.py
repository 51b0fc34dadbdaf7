"""The contract of ``include/cough_amd_channel.h`` restated in numpy (``cough_detector_amd/channel.py``, ``csrc/channel.hip``).

* ``recurrence``: the sequential direct-form-II-transposed cascade, vectorised over the rows of a batch, in any numpy
  float type: in float64 it is held bit-equal to ``scipy.signal.sosfilt`` by the host test, in ``np.longdouble`` it is
  the reference ``y_ref`` of the bound.
* ``blob_ref``: ``cough_channel_prepare``'s blob, word by word in the header's order.
* ``emulate``: the kernel's chunked-scan algorithm in numpy float64, operation by operation (no fma, which numpy does not
  have).  ``defect`` plants one of ``DEFECTS`` so that the host test can show that the GPU test's bound sees it.
* ``clip_ref``: the ceiling.  ``draw_channel_ref`` / ``host_channel_draw``: the device's and the host's draws.
* ``batch``: the one ragged test batch, its references computed once.

THE BOUND.  ``|y - y_ref| <= 2^-24 |y_ref| + K * 2^-53 * G * peak(x)`` with ``y_ref`` the long-double recurrence, ``G`` the
product of the sections' ``sum |h|`` and ``K = BOUND_K``.  ``K`` is 16 times the largest error, in units of
``2^-53 G peak(x)``, that the clean float64 ``emulate`` shows against long double on the rows of ``batch()`` (measured:
``EMULATE_UNITS``; the factor 16 covers fma contraction and another association of the scan on the device).  The
largest figure, 1.9e5 units, belongs to DC through the 20 Hz high-pass: its output decays to nothing while its state
stays at the input's size, and the start states carry the rounding of M^128 = A^8192, thirteen squarings deep
(``scipy.signal.sosfilt`` itself shows 4.2e2 units there; noise rows stay near 3e3).  With K = 3.2e6 the absolute term is
3.6e-10 G peak(x), still two orders under a float32 ulp of the peak.
"""
import functools
import random

import numpy as np
from scipy import signal

import draws_ref as D

CHUNK, THREADS, SPAN, MAX_SECTIONS, POWERS, ENTRY_WORDS, REC_WORDS = 64, 256, 16384, 4, 8, 160, 40
MAX_LEN = 1 << 30
PLAN_DTYPE = np.dtype([("filter", "<i4"), ("clip_ratio", "<f4")])
U24, U53 = 2.0 ** -24, 2.0 ** -53
DEFECTS = ("carry_t2", "power_off_by_one", "section_skipped", "z_swapped", "span_seed_zero")
# the largest error of the clean float64 emulation against long double over batch(), in units of 2^-53 G peak(x)
# (tests/test_channel_host.py measures it again and holds it below this figure), and the bound's K = 16 times that
EMULATE_UNITS = 2.0e5
BOUND_K = 16 * EMULATE_UNITS
IDENTITY = np.array([1.0, 0.0, 0.0, 1.0, 0.0, 0.0])


def normalized(sos):
    """(S, 5) float64 ``b0, b1, b2, a1, a2``: every row divided by its a0."""
    s = np.asarray(sos, dtype=np.float64).reshape(-1, 6)
    return np.stack([s[:, 0] / s[:, 3], s[:, 1] / s[:, 3], s[:, 2] / s[:, 3], s[:, 4] / s[:, 3], s[:, 5] / s[:, 3]], axis=1)


# ------------------------------------------------------------------------------------------------ the sequential filter
def recurrence(cascades, rows, dtype=np.float64):
    """Row r of ``rows`` (a list of 1-D arrays) through ``cascades[r]`` ((S, 6), or None for no filter), sample by sample,
    all rows at once: a list of 1-D arrays of ``dtype``.  One rounding per operator, in sosfilt's order."""
    b, width = len(rows), max([len(x) for x in rows] + [1])
    coef = np.zeros((MAX_SECTIONS, 5, b), dtype=dtype)
    for r, sos in enumerate(cascades):
        c = normalized(sos if sos is not None else IDENTITY)
        c = np.concatenate([c, normalized(np.tile(IDENTITY, (MAX_SECTIONS - c.shape[0], 1)))]) if c.shape[0] < MAX_SECTIONS else c
        coef[:, :, r] = c.astype(dtype)
    y = np.zeros((b, width), dtype=dtype)
    for r, x in enumerate(rows):
        y[r, :len(x)] = np.asarray(x).astype(dtype)
    y = np.ascontiguousarray(y.T)                                   # (width, b): one sample of every row per step
    for s in range(MAX_SECTIONS):
        b0, b1, b2, a1, a2 = coef[s]
        if not (b1.any() or b2.any() or a1.any() or a2.any()) and (b0 == 1).all():
            continue
        z1, z2 = np.zeros(b, dtype=dtype), np.zeros(b, dtype=dtype)
        for n in range(width):
            x = y[n]
            out = b0 * x + z1
            z1 = b1 * x - a1 * out + z2
            z2 = b2 * x - a2 * out
            y[n] = out
    return [np.ascontiguousarray(y[:len(x), r]) for r, x in enumerate(rows)]


def scipy_sos(sos):
    """The cascade as ``scipy.signal.sosfilt`` takes it: divided by a0, which it wants to be 1."""
    c = normalized(sos)
    return np.stack([c[:, 0], c[:, 1], c[:, 2], np.ones(c.shape[0]), c[:, 3], c[:, 4]], axis=1)


def gain(sos, taps: int = 1 << 17):
    """G: the product of the sections' ``sum |h|`` (each section's impulse response, ``taps`` samples of it)."""
    impulse = np.zeros(taps)
    impulse[0] = 1.0
    return float(np.prod([np.abs(signal.sosfilt(sec.reshape(1, 6), impulse)).sum() for sec in scipy_sos(sos)]))


def bound(y_ref, g, peak, k=BOUND_K):
    """The bound per sample, float64."""
    return U24 * np.abs(np.asarray(y_ref, dtype=np.float64)) + k * U53 * g * peak


def units(y, y_ref, g, peak):
    """The largest error of ``y`` against ``y_ref`` in units of ``2^-53 G peak``, the relative half-ulp term taken off."""
    if len(y) == 0 or peak == 0.0:
        return 0.0
    err = np.abs(np.asarray(y).astype(np.longdouble) - y_ref) - U24 * np.abs(y_ref)
    return float(max(err.max(), 0.0) / (U53 * g * peak))


# ------------------------------------------------------------------------------------------------ the bank's blob
def mat2(x, y):
    """X * Y of two row-major 2x2 matrices, one IEEE operation per operator, in the header's order."""
    return np.array([x[0] * y[0] + x[1] * y[2], x[0] * y[1] + x[1] * y[3], x[2] * y[0] + x[3] * y[2], x[2] * y[1] + x[3] * y[3]])


def blob_ref(cascades):
    """float64 (n, 160): ``cough_channel_prepare``'s blob."""
    blob = np.zeros((len(cascades), ENTRY_WORDS), dtype=np.float64)
    for r, sos in enumerate(cascades):
        c = normalized(sos)
        for s, (b0, b1, b2, a1, a2) in enumerate(c):
            rec = blob[r, REC_WORDS * s:REC_WORDS * (s + 1)]
            rec[:5] = (b0, b1, b2, a1, a2)
            p = np.array([-a1, 1.0, -a2, 0.0])
            for _ in range(6):
                p = mat2(p, p)
            for j in range(POWERS):
                rec[8 + 4 * j:12 + 4 * j] = p
                p = mat2(p, p)
        blob[r, 5] = float(c.shape[0])
    return blob


# ------------------------------------------------------------------------------------------------ the kernel's algorithm
def emulate(x, sos, defect=None):
    """The kernel's float64 result for one row, before the rounding to float32: spans of 256 chunks of 64, per section the
    chunks from zero state, the log-step scan of the carries with the blob's powers, the chunks again from their start
    states.  ``defect``: one of ``DEFECTS``."""
    assert defect is None or defect in DEFECTS
    n = len(x)
    entry = blob_ref([sos])[0]
    n_sec = int(entry[5])
    padded = np.zeros(-(-max(n, 1) // SPAN) * SPAN, dtype=np.float64)
    padded[:n] = np.asarray(x, dtype=np.float64)
    out = np.empty_like(padded)
    carry = np.zeros((MAX_SECTIONS, 2))
    sections = range(n_sec - 1) if defect == "section_skipped" else range(n_sec)

    def chunks(block, rec, z1, z2, keep):
        b0, b1, b2, a1, a2 = rec[:5]
        for k in range(CHUNK):
            xv = block[:, k]
            y = b0 * xv + z1
            z1 = b1 * xv - a1 * y + z2
            z2 = b2 * xv - a2 * y
            if keep:
                block[:, k] = y
        return z1, z2

    for w in range(padded.size // SPAN):
        block = padded[w * SPAN:(w + 1) * SPAN].reshape(THREADS, CHUNK).copy()
        for s in sections:
            rec = entry[REC_WORDS * s:REC_WORDS * (s + 1)]
            s1, s2 = chunks(block, rec, np.zeros(THREADS), np.zeros(THREADS), False)
            in1, in2 = (0.0, 0.0) if defect == "span_seed_zero" else carry[s]
            s1[0] = (rec[8] * in1 + rec[9] * in2) + s1[0]
            s2[0] = (rec[10] * in1 + rec[11] * in2) + s2[0]
            for j in range(POWERS):
                d = 1 << j
                m = rec[8 + 4 * (min(j + 1, POWERS - 1) if defect == "power_off_by_one" else j):][:4]
                p1, p2 = s1[:-d].copy(), s2[:-d].copy()
                s1[d:] = (m[0] * p1 + m[1] * p2) + s1[d:]
                s2[d:] = (m[2] * p1 + m[3] * p2) + s2[d:]
            back = 2 if defect == "carry_t2" else 1
            z1 = np.concatenate([[in1] * back, s1[:-back]])
            z2 = np.concatenate([[in2] * back, s2[:-back]])
            if defect == "z_swapped":
                z1, z2 = z2, z1
            carry[s] = (s1[-1], s2[-1])
            chunks(block, rec, z1, z2, True)
        out[w * SPAN:(w + 1) * SPAN] = block.reshape(-1)
    return out[:n]


# ------------------------------------------------------------------------------------------------ the ceiling, the rules
def clip_ref(y32, ratio):
    """The ceiling on a row's float32 samples: ``c = float32(ratio) * max|y|`` as one float32 product, then
    ``y > c ? c : (y < -c ? -c : y)``; a ratio outside [0, 1) or NaN leaves the row as it is."""
    y32, ratio = np.asarray(y32, dtype=np.float32), np.float32(ratio)
    if not (ratio >= 0 and ratio < 1) or y32.size == 0:
        return y32.copy()
    c = np.float32(ratio * np.abs(y32).max())
    return np.where(y32 > c, c, np.where(y32 < -c, -c, y32)).astype(np.float32)


def rule(x, filtered, clipped):
    """What the rules make of a row before any arithmetic: ``"copy"``, ``"nan"``, ``"zero"`` or None (the filter runs)."""
    if not filtered and not clipped:
        return "copy"
    if not np.isfinite(x).all():
        return "nan"
    if not np.any(x != 0):
        return "zero"
    return None


# ------------------------------------------------------------------------------------------------ the draws
def draw_channel_ref(seed, b, p, n_bank, p_clip, lo, hi):
    """(B,) ``PLAN_DTYPE``: the plans ``cough_draw_channel`` writes."""
    rows = np.arange(b, dtype=np.uint64)
    seed = int(seed) & (2**64 - 1)
    d = [D.unit(v) for v in D.philox4x32_10((np.zeros(rows.shape, dtype=np.uint64), rows, 0, 5), (seed & 0xFFFFFFFF, seed >> 32))]
    fired = d[0] <= p
    plans = np.zeros(b, dtype=PLAN_DTYPE)
    which = np.minimum((float(n_bank) * d[1]).astype(np.int32), max(n_bank - 1, 0)) if n_bank >= 1 else np.full(b, -1, dtype=np.int32)
    plans["filter"] = np.where(fired, which, -1)
    ratio = (np.float64(lo) + (np.float64(hi) - np.float64(lo)) * d[3]).astype(np.float32)
    plans["clip_ratio"] = np.where(fired & (d[2] <= p_clip), ratio, np.float32(1.0))
    return plans


def host_channel_draw(rng: random.Random, p_augment, n_bank, p_clip, clip_range):
    """The host's draw of one clip: ``rng.random() > p_augment`` skips; else ``rng.randrange(n_bank)``, then
    ``rng.random() < p_clip`` gives ``rng.uniform(*clip_range)`` (else the ratio is 1.0)."""
    if rng.random() > p_augment:
        return None
    which = rng.randrange(n_bank)
    return which, (rng.uniform(*clip_range) if rng.random() < p_clip else 1.0)


# ------------------------------------------------------------------------------------------------ the test batch
def bank_sos(sample_rate=16000):
    """The bank of the test batch: 1 to 4 sections."""
    ny = sample_rate / 2.0
    w0 = 2.0 * np.pi * 60.0 / sample_rate
    alpha, a = np.sin(w0) / (2.0 * 30.0), 10.0 ** (12.0 / 40.0)
    peak60 = np.array([[1 + alpha * a, -2 * np.cos(w0), 1 - alpha * a, 1 + alpha / a, -2 * np.cos(w0), 1 - alpha / a]])
    hp20 = signal.butter(2, 20.0 / ny, "highpass", output="sos")
    band2 = signal.butter(2, [300.0 / ny, 3400.0 / ny], "bandpass", output="sos")
    three = np.concatenate([hp20 * np.array([2.0, 2.0, 2.0, 2.0, 2.0, 2.0]), peak60, signal.butter(2, 3000.0 / ny, "lowpass", output="sos")])
    band4 = signal.butter(4, [300.0 / ny, 3400.0 / ny], "bandpass", output="sos")
    return [hp20, peak60, band2, three, band4]                      # 1, 1, 2, 3 (a0 = 2 in its first), 4 sections


LENGTHS = (0, 1, 2, 63, 64, 65, 16383, 16384, 16385, 32769, 48000)
RATIOS = (0.0, 0.25, 1.0, 1.5, float("nan"))
WIDTH = 48000
BEYOND = 99                                                         # a filter the bank does not have


def _signals(rng, n):
    t = np.arange(n)
    burst = np.zeros(n, dtype=np.float32)
    burst[n // 3:n // 3 + max(n // 8, 1)] = (0.9 * rng.standard_normal(max(n // 8, 1))).astype(np.float32)[:n - n // 3]
    return {"noise": (0.3 * rng.standard_normal(n)).astype(np.float32), "burst": burst, "dc": np.full(n, 0.5, dtype=np.float32),
            "tone": (0.7 * np.sin(2 * np.pi * 440.0 / 16000.0 * t)).astype(np.float32)}


@functools.lru_cache(maxsize=None)
def batch():
    """The ragged test batch, computed once: ``(cascades, rows)``.  A row is a dict: ``name``, ``x`` (float32), ``filter``
    (as the plan holds it), ``ratio``, ``sos`` (the cascade that applies, or None), ``rule`` for the unclipped and
    ``rule_clipped`` for the clipped run, and for a filtered row ``ref`` (long double), ``g`` and ``peak``."""
    cascades = bank_sos()
    rng = np.random.default_rng(11)
    rows = []

    def add(name, x, filt, ratio):
        rows.append(dict(name=name, x=np.ascontiguousarray(x, dtype=np.float32), filter=filt, ratio=ratio))

    for i, n in enumerate(LENGTHS):                                 # the chunk and span edges, every cascade and ratio
        add(f"noise n={n}", _signals(rng, n)["noise"], i % 5, RATIOS[i % 5])
    for i, n in enumerate((65, 16385, 32769, 48000)):               # the long rows again with the slowly decaying filters
        add(f"noise n={n} again", _signals(rng, n)["noise"], (0, 1, 0, 1)[i], RATIOS[(i + 1) % 5])
    for f in (0, 1, 2):                                             # every signal through the three named filters
        for i, (kind, x) in enumerate(_signals(rng, 16000).items()):
            add(f"{kind} filter {f}", x, f, RATIOS[(f + i) % 5])
    add("burst 4 sections n=20000", _signals(rng, 20000)["burst"], 4, 0.25)
    add("tone 3 sections", _signals(rng, 16000)["tone"], 3, 0.0)
    nan_first, inf_last, nan_copy = _signals(rng, 16000)["noise"], _signals(rng, 16385)["noise"], _signals(rng, 300)["noise"]
    nan_first[0], inf_last[-1], nan_copy[0] = np.nan, -np.inf, np.nan
    nan_copy[5] = np.float32(-0.0)
    add("zeros", np.zeros(16000, dtype=np.float32), 0, 0.25)
    add("negative zeros, clip only", np.full(70, -0.0, dtype=np.float32), -1, 0.5)
    add("nan first", nan_first, 2, 1.0)
    add("inf last", inf_last, 1, 0.25)
    add("nan first, clip only", nan_first, -1, 0.25)
    add("nan and -0.0, a copy", nan_copy, -1, 1.0)
    add("noise, clip only", _signals(rng, 16385)["noise"], -1, 0.25)
    add("noise, a copy", _signals(rng, 16385)["noise"], -1, float("nan"))
    add("noise, a filter beyond the bank", _signals(rng, 1000)["noise"], BEYOND, 0.25)
    add("noise, a filter beyond the bank, a copy", _signals(rng, 1000)["noise"], BEYOND, -1.0)

    for row in rows:
        row["sos"] = cascades[row["filter"]] if 0 <= row["filter"] < len(cascades) else None
        clipped = bool(np.float32(row["ratio"]) >= 0 and np.float32(row["ratio"]) < 1)
        row["rule"], row["rule_clipped"] = rule(row["x"], row["sos"] is not None, False), rule(row["x"], row["sos"] is not None, clipped)
    live = [row for row in rows if row["rule"] is None]
    for row, ref in zip(live, recurrence([row["sos"] for row in live], [row["x"] for row in live], np.longdouble)):
        row["ref"], row["g"] = ref, gain(row["sos"])
        row["peak"] = float(np.abs(row["x"]).max()) if row["x"].size else 0.0
    return cascades, rows


def plans_of(rows, clipped: bool):
    """(B,) ``PLAN_DTYPE`` of the batch, unchecked (one filter is beyond the bank on purpose); ``clipped=False`` replaces
    every ratio by 1.0."""
    plans = np.zeros(len(rows), dtype=PLAN_DTYPE)
    plans["filter"] = [row["filter"] for row in rows]
    plans["clip_ratio"] = [row["ratio"] if clipped else 1.0 for row in rows]
    return plans


def expect_exact(row, clipped: bool):
    """The float32 row the rules fix without arithmetic, or None."""
    what = row["rule_clipped"] if clipped else row["rule"]
    if what == "copy":
        return row["x"].copy()
    if what == "nan":
        return np.full(row["x"].size, 0x7FC00000, dtype=np.uint32).view(np.float32)
    if what == "zero":
        return np.zeros(row["x"].size, dtype=np.float32)
    return None
