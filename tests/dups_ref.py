"""The duplicate search of cough_detector_amd/duplicates.py (include/cough_amd_dups.h) restated in numpy -- twice.

The ``*_words`` form works the way the kernels do: on 32-bit words, with a popcount, all pairs of a lag at once.  The
``*_bits`` form uses only the definitions: a fingerprint is a (frames x 32) matrix of booleans computed one float32
operation at a time, a pair is walked frame by frame, a frame is live when any of its 64 bits is set, an error is a
position where the two rows differ.  tests/test_dups_host.py holds the two against each other; the GPU tests hold the
kernels against ``fingerprint_words`` on the device's own images and against ``match_words`` on the same words, so every
comparison a kernel makes is made here on the same values: integers and bits must be equal, no tolerance.
"""
import numpy as np

ROWS, HIST_BINS = 33, 65
POP8 = np.array([bin(v).count("1") for v in range(256)], dtype=np.uint8)


def default_rows(n_mels):
    return tuple((k * (n_mels - 1)) // 32 for k in range(ROWS))


def lag_order(L):
    """0, -1, +1, -2, +2, ..., -L, +L"""
    return [0] + [s * m for m in range(1, L + 1) for s in (-1, 1)]


def popcount(x):
    x = np.ascontiguousarray(x, dtype=np.uint32)
    return POP8[x.view(np.uint8)].reshape(x.shape + (4,)).sum(axis=-1, dtype=np.int64)


# ---------------------------------------------------------------------------------------------------- fingerprints
def fingerprint_words(images, rows, W, D):
    """``(words (n, Tw) uint32, live (n,) int32)`` of float32 ``images`` (n, F, T): whole-array float32 operations, each
    rounded once (numpy adds float32 arrays in float32)."""
    E = np.asarray(images, dtype=np.float32)
    n, _, T = E.shape
    Tw = T - W + 1 - D
    assert Tw >= 1 and len(rows) == ROWS
    with np.errstate(invalid="ignore"):
        S = []
        for r in rows:
            s = E[:, r, 0:Tw + D]
            for j in range(1, W):
                s = s + E[:, r, j:j + Tw + D]                    # ascending: ((E[t] + E[t+1]) + E[t+2]) + ...
            S.append(s)
        words = np.zeros((n, Tw), dtype=np.uint32)
        for k in range(ROWS - 1):
            d = S[k] - S[k + 1]
            assert d.dtype == np.float32
            words |= ((d[:, D:D + Tw] - d[:, 0:Tw]) > 0).astype(np.uint32) << np.uint32(k)
    return words, (words != 0).sum(axis=1).astype(np.int32)


def fingerprint_bits(images, rows, W, D):
    """``(n, Tw, 32)`` booleans, one scalar float32 operation at a time."""
    E = np.asarray(images, dtype=np.float32)
    n, _, T = E.shape
    Tw = T - W + 1 - D
    out = np.zeros((n, Tw, 32), dtype=bool)
    with np.errstate(invalid="ignore"):
        for c in range(n):
            def S(k, t):
                s = E[c, rows[k], t]
                for j in range(1, W):
                    s = np.float32(s + E[c, rows[k], t + j])
                return s
            sums = [[S(k, t) for t in range(Tw + D)] for k in range(ROWS)]
            for k in range(32):
                for t in range(Tw):
                    d0 = np.float32(sums[k][t] - sums[k + 1][t])
                    d1 = np.float32(sums[k][t + D] - sums[k + 1][t + D])
                    out[c, t, k] = bool(np.float32(d1 - d0) > 0)
    return out


def words_to_bits(words):
    w = np.asarray(words, dtype=np.uint32)
    return ((w[..., None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)).astype(bool)


def bits_to_words(bits):
    return (np.asarray(bits, dtype=np.uint32) << np.arange(32, dtype=np.uint32)).sum(axis=-1, dtype=np.uint64).astype(np.uint32)


# ---------------------------------------------------------------------------------------------------- one pair
def better(err, bits, best_err, best_bits):
    """The strict-replace rule: integers, ties keep the earlier lag."""
    return err * best_bits < best_err * bits


def pair_bits(A, B, L, min_live):
    """``(lag, err, bits)`` of the best lag of two (Tw, 32) boolean fingerprints, or None: frame by frame."""
    Tw, best = A.shape[0], None
    for lag in lag_order(L):
        live = err = 0
        for t in range(Tw):
            u = t + lag
            if not 0 <= u < Tw:
                continue                                         # frame t of a meets no frame of b
            if A[t].any() or B[u].any():
                live += 1
            err += int((A[t] != B[u]).sum())
        if live < min_live:
            continue
        if best is None or better(err, 32 * live, best[1], best[2]):
            best = (lag, err, 32 * live)
    return best


def matches(err, bits, max_err_1024):
    return err * 1024 <= max_err_1024 * bits


# ---------------------------------------------------------------------------------------------------- all pairs
def _finish(n, lag, err, bits, max_err_1024):
    """From (n, n) int64 arrays with ``bits == 0`` where a pair has no best lag."""
    has = bits > 0
    hit = has & (err * 1024 <= max_err_1024 * bits)
    a, b = np.nonzero(hit)                                       # row-major: sorted by (a, b)
    hist = np.bincount((err[has] * 64) // bits[has], minlength=HIST_BINS).astype(np.int64)
    return dict(counts=hit.sum(axis=1).astype(np.int32), a=a.astype(np.int32), b=b.astype(np.int32),
                lag=lag[hit].astype(np.int32), err=err[hit].astype(np.int32), bits=bits[hit].astype(np.int32), hist=hist,
                best_lag=lag, best_err=err, best_bits=bits)


def match_words(words, L, max_err_1024, min_live):
    """Everything the matcher gives, from (n, Tw) uint32 words: a lag at a time over all pairs."""
    w = np.asarray(words, dtype=np.uint32)
    n, Tw = w.shape
    flat = (w != 0).sum(axis=1) == 0
    valid = np.triu(np.ones((n, n), dtype=bool), k=1) & ~flat[:, None] & ~flat[None, :]
    b_lag, b_err, b_bits = (np.zeros((n, n), dtype=np.int64) for _ in range(3))
    for lag in lag_order(L):
        t0, t1 = max(0, -lag), min(Tw, Tw - lag)
        if t1 <= t0:
            continue                                             # no frame meets: zero live frames, min_live >= 1
        A, B = w[:, None, t0:t1], w[None, :, t0 + lag:t1 + lag]
        err = popcount(A ^ B).sum(axis=-1)
        bits = 32 * ((A | B) != 0).sum(axis=-1, dtype=np.int64)
        take = valid & (bits >= 32 * min_live) & ((b_bits == 0) | better(err, bits, b_err, b_bits))
        b_lag[take], b_err[take], b_bits[take] = lag, err[take], bits[take]
    return _finish(n, b_lag, b_err, b_bits, max_err_1024)


def match_bits(bits, L, max_err_1024, min_live):
    """The same from (n, Tw, 32) booleans, a pair at a time through ``pair_bits``."""
    bits = np.asarray(bits, dtype=bool)
    n = bits.shape[0]
    b_lag, b_err, b_bits = (np.zeros((n, n), dtype=np.int64) for _ in range(3))
    for a in range(n):
        for b in range(a + 1, n):
            if not bits[a].any() or not bits[b].any():
                continue                                         # a flat clip is never paired
            best = pair_bits(bits[a], bits[b], L, min_live)
            if best is not None:
                b_lag[a, b], b_err[a, b], b_bits[a, b] = best
    return _finish(n, b_lag, b_err, b_bits, max_err_1024)


KEYS = ("counts", "a", "b", "lag", "err", "bits", "hist")


def same(x, y):
    """None, or the first key in which two results differ."""
    for key in KEYS:
        if x[key].tolist() != y[key].tolist():
            return key
    return None


# ---------------------------------------------------------------------------------------------------- a synthetic corpus
SR = 16000


def base_clip(seed, n=SR):
    """One second with 2-3 coloured noise bursts (a random two-pole resonance each) on a noise floor 54 dB below."""
    rng = np.random.default_rng(1000 + seed)
    x = rng.standard_normal(n) * 10.0 ** (-54.0 / 20.0)
    for _ in range(int(rng.integers(2, 4))):
        length = int(rng.integers(1200, 4000))
        start = int(rng.integers(0, n - length))
        f, r = rng.uniform(300.0, 3500.0), rng.uniform(0.7, 0.95)
        noise = rng.standard_normal(length)
        y = np.zeros(length)
        c1, c2 = 2.0 * r * np.cos(2.0 * np.pi * f / SR), -r * r
        for k in range(length):
            y[k] = noise[k] + c1 * (y[k - 1] if k >= 1 else 0.0) + c2 * (y[k - 2] if k >= 2 else 0.0)
        y *= np.hanning(length) / max(np.abs(y).max(), 1e-12)
        x[start:start + length] += y * rng.uniform(0.3, 1.0)
    return (0.8 * x / np.abs(x).max()).astype(np.float32)


KINDS = ("gain", "delay320", "delay37", "cut")


def planted(x, kind):
    """A copy of ``x``: gain x 0.3; delayed by 320 or 37 samples (zeros in front, the end falls off); the last 0.2 s cut
    and padded with zeros."""
    y = np.zeros_like(x)
    if kind == "gain":
        y[:] = x * np.float32(0.3)
    elif kind in ("delay320", "delay37"):
        d = int(kind[5:])
        y[d:] = x[:-d]
    elif kind == "cut":
        keep = len(x) - SR // 5
        y[:keep] = x[:keep]
    else:
        raise ValueError(kind)
    return y


def corpus(n_base=8):
    """``(clips, group)``: for each of ``n_base`` base clips the clip and its four planted copies, in that order;
    ``group[k]`` is the index of the base clip's entry."""
    clips, group = [], []
    for s in range(n_base):
        x = base_clip(s)
        first = len(clips)
        clips.append(x)
        clips += [planted(x, kind) for kind in KINDS]
        group += [first] * (1 + len(KINDS))
    return clips, np.array(group, dtype=np.int64)
