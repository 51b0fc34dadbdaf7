"""The contract of ``include/cough_amd_reverb.h`` restated in numpy (``cough_detector_amd/reverb.py``,
``csrc/reverb.hip``).

* ``reverb_ref``: the float64 reference -- ``np.convolve`` on the shifted, zero-extended row.
* ``bad_spans`` / ``silent_spans``: the span rules for non-finite and for all-zero input.
* ``bound``: the header's per-sample bound ``K * 2^-24 * ||z_w||_2 * ||h||_1``, per span.
* ``draw_reverb_ref`` / ``host_reverb_draws``: the device's and the host's reverb draws.
* ``emulate``: the kernel's own algorithm in float32 numpy, operation by operation (no fma, which numpy does not have):
  pair packing of the two overlap-save segments, the seven radix-4 passes with the same rounded table, the product
  with the digit-reversed pre-scaled spectrum, the inverse.  ``defect`` plants one of ``DEFECTS`` so that the host test
  can show that the GPU test's checks see it.
"""
import math
import random

import numpy as np

import draws_ref as D
import warp_ref as W

N, HALF, MAX_TAPS, MAX_LEN = 16384, 8192, 8193, 1 << 30
BOUND_K = 160                      # COUGH_REVERB_BOUND_K
U24 = 2.0 ** -24
RMS_FACTOR = 4.0                   # the device's RMS error may be this many times the emulation's, per row
DEFECTS = ("twiddle_off_by_one", "segment_b_late", "no_scale", "valid_from_8191")
# a defect of the rule, not of the arithmetic: the load-time OR is skipped and a NaN or an Inf goes through the transform
NO_LOAD_RULE = "no_load_rule"
QUIET_NAN = 0x7FC00000             # what the rule writes; NaNs that arithmetic makes need not have these bits

_m = np.arange(N, dtype=np.float64)
TW_R = np.cos(-2.0 * np.pi * _m / N).astype(np.float32)          # float64, rounded once
TW_I = np.sin(-2.0 * np.pi * _m / N).astype(np.float32)
_J = np.arange(N // 4)


def n_spans(width):
    return (int(width) + N - 1) // N


def shifted_ext(x, shift, lo, hi):
    """x_s[lo .. hi-1]: the shifted row, zero outside [0, n)."""
    x = np.asarray(x, dtype=np.float32)
    xs = W.shifted(x, shift)
    out = np.zeros(hi - lo, dtype=np.float32)
    a, b = max(lo, 0), min(hi, x.size)
    if b > a:
        out[a - lo:b - lo] = xs[a:b]
    return out


def span_inputs(x, shift, w):
    """(segment a, segment b) of span w: x_s[16384 w - 8192 ..] and the 16384 samples 8192 later."""
    s = N * w
    return shifted_ext(x, shift, s - HALF, s + HALF), shifted_ext(x, shift, s, s + N)


def bad_spans(x, shift, out_len):
    """Per span that holds a column below out_len: whether any of its 2 x 16384 inputs is not finite."""
    return [not (np.isfinite(a).all() and np.isfinite(b).all())
            for a, b in (span_inputs(x, shift, w) for w in range(n_spans(out_len)))]


def silent_spans(x, shift, out_len):
    return [not (a.any() or b.any()) for a, b in (span_inputs(x, shift, w) for w in range(n_spans(out_len)))]


def reverb_ref(x, shift, h, out_len):
    """float64 (out_len,): y[m] = sum_k h[k] x_s[m - k].  The inputs must be finite (replace the samples the span rule
    answers for by zeros first).  h None: the shifted copy of min(n, out_len) samples, zeros behind."""
    x = np.asarray(x, dtype=np.float32)
    xs = W.shifted(x, shift).astype(np.float64)
    y = np.zeros(out_len, dtype=np.float64)
    full = xs if h is None else (np.convolve(xs, np.asarray(h, dtype=np.float32).astype(np.float64)) if x.size else xs)
    k = min(out_len, full.size)
    y[:k] = full[:k]
    return y


def bound(x, shift, h, out_len):
    """float64 (out_len,): K * 2^-24 * ||z_w||_2 * ||h||_1 for the span each column lies in."""
    h1 = float(np.abs(np.asarray(h, dtype=np.float64)).sum())
    e = np.zeros(out_len, dtype=np.float64)
    for w in range(n_spans(out_len)):
        a, b = span_inputs(x, shift, w)
        z2 = math.sqrt(float((a.astype(np.float64) ** 2).sum() + (b.astype(np.float64) ** 2).sum()))
        e[N * w:N * (w + 1)] = BOUND_K * U24 * z2 * h1
    return e


# ------------------------------------------------------------------------------------------------ the draws
def draw_reverb_ref(seed, lengths, p, n_rirs):
    """int32 (B, 4): the plans ``cough_draw_reverb`` writes -- (0, rir or -1, n, 0)."""
    n = np.clip(np.asarray(lengths, dtype=np.int64), 0, MAX_LEN)
    rows = np.arange(n.size, dtype=np.uint64)
    seed = int(seed) & (2**64 - 1)
    key = (seed & 0xFFFFFFFF, seed >> 32)
    d = [D.unit(v) for v in D.philox4x32_10((np.zeros(rows.shape, dtype=np.uint64), rows, 0, 4), key)]
    fired = (d[0] <= p) & (n >= 1) & (n_rirs >= 1)
    rir = np.minimum((float(n_rirs) * d[1]).astype(np.int32), max(n_rirs - 1, 0))
    plans = np.zeros((n.size, 4), dtype=np.int32)
    plans[:, 1] = np.where(fired, rir, -1)
    plans[:, 2] = n
    return plans


def host_reverb_draw(rng: random.Random, p_augment, n_rirs):
    """The host's draw of one clip: ``rng.random() > p_augment`` skips, else ``rng.randrange(n_rirs)``."""
    if rng.random() > p_augment:
        return None
    return rng.randrange(n_rirs)


# ------------------------------------------------------------------------------------------------ the emulation
def _cmul(ar, ai, wr, wi, conj=False):
    if conj:
        return ar * wr + ai * wi, ai * wr - ar * wi
    return ar * wr - ai * wi, ar * wi + ai * wr


def _dft4(x, inverse):
    (r0, i0), (r1, i1), (r2, i2), (r3, i3) = x
    a0r, a0i, a1r, a1i = r0 + r2, i0 + i2, r0 - r2, i0 - i2
    a2r, a2i, a3r, a3i = r1 + r3, i1 + i3, r1 - r3, i1 - i3
    y0, y2 = (a0r + a2r, a0i + a2i), (a0r - a2r, a0i - a2i)
    minus, plus = (a1r + a3i, a1i - a3r), (a1r - a3i, a1i + a3r)      # a1 - i a3, a1 + i a3
    return (y0, plus, y2, minus) if inverse else (y0, minus, y2, plus)


def _pass(zr, zi, q, inverse, off=0):
    """One radix-4 pass over sub-transforms of length 4 q, in place; ``off`` is added to the first twiddle's index."""
    k = _J & (q - 1)
    base = ((_J - k) << 2) + k
    step = N // 4 // q
    idx = [base + p * q for p in range(4)]
    x = [(zr[i], zi[i]) for i in idx]
    tw = [None] + [((p * k * step + (off if p == 1 else 0)) % N) for p in (1, 2, 3)]
    if inverse and q > 1:
        x = [x[0]] + [_cmul(x[p][0], x[p][1], TW_R[tw[p]], TW_I[tw[p]], conj=True) for p in (1, 2, 3)]
    y = _dft4(x, inverse)
    if not inverse and q > 1:
        y = [y[0]] + [_cmul(y[p][0], y[p][1], TW_R[tw[p]], TW_I[tw[p]]) for p in (1, 2, 3)]
    for p in range(4):
        zr[idx[p]], zi[idx[p]] = y[p]


def _forward(zr, zi, defect=None):
    q = N // 4
    while q >= 1:
        _pass(zr, zi, q, False, off=1 if (defect == "twiddle_off_by_one" and q == 256) else 0)
        q >>= 2


def _inverse(zr, zi):
    q = 1
    while q <= N // 4:
        _pass(zr, zi, q, True)
        q <<= 2


def spectrum(h, scale=True):
    """The stored spectrum of a response: digit-reversed, scaled by 2^-14.  (re, im) float32."""
    h = np.asarray(h, dtype=np.float32)
    assert 1 <= h.size <= MAX_TAPS
    zr, zi = np.zeros(N, dtype=np.float32), np.zeros(N, dtype=np.float32)
    zr[:h.size] = h
    _forward(zr, zi)
    s = np.float32(1.0 / N) if scale else np.float32(1.0)
    return zr * s, zi * s


def emulate(x, shift, h, out_len, defect=None, spec=None):
    """float32 (out_len,): what the kernel's algorithm gives in float32 without fma, rules included."""
    assert defect is None or defect in DEFECTS or defect == NO_LOAD_RULE
    x = np.asarray(x, dtype=np.float32)
    y = np.zeros(out_len, dtype=np.float32)
    if h is None:
        k = min(x.size, out_len)
        y[:k] = W.shifted(x, shift)[:k]
        return y
    hr, hi = spec if spec is not None else spectrum(h, scale=defect != "no_scale")
    for w in range(n_spans(out_len)):
        s = N * w
        a, b = span_inputs(x, shift, w)
        if defect == "segment_b_late":
            b = shifted_ext(x, shift, s + 1, s + 1 + N)
        lo, hi_ = s, min(s + N, out_len)
        if not (np.isfinite(a).all() and np.isfinite(b).all()) and defect != NO_LOAD_RULE:
            y[lo:hi_] = np.array([QUIET_NAN], dtype=np.uint32).view(np.float32)[0]
            continue
        if not (a.any() or b.any()):
            continue
        zr, zi = a.copy(), b.copy()
        with np.errstate(over="ignore", invalid="ignore"):
            _forward(zr, zi, defect)
            zr, zi = _cmul(zr, zi, hr, hi)
            _inverse(zr, zi)
        first = HALF - 1 if defect == "valid_from_8191" else HALF
        both = np.concatenate([zr[first:first + HALF], zi[first:first + HALF]])
        y[lo:hi_] = both[:hi_ - lo]
    return y


# ------------------------------------------------------------------------------------------------ the shared cases
LENGTHS = (0, 1, 2, 255, 8191, 8192, 8193, 16000, 16383, 16384, 16385, 32768, 32769, 48000)      # one to three spans


def bank_responses():
    """Responses of 1, 2, 3, 8192 and 8193 taps, then unit impulses at taps 0, 1, 8191 and 8192."""
    rng = np.random.default_rng(77)
    bank = []
    for taps in (1, 2, 3, 8192, 8193):
        h = rng.standard_normal(taps) * np.exp(-6.9 * np.arange(taps) / 8193.0)
        bank.append((h / math.sqrt(float((h * h).sum()))).astype(np.float32))
    for at in (0, 1, 8191, 8192):
        h = np.zeros(at + 1, dtype=np.float32)
        h[at] = 1.0
        bank.append(h)
    return bank


def _content(kind, n, rng):
    if kind == "noise":
        return rng.standard_normal(n).astype(np.float32)
    if kind == "burst":                                  # a burst between exact zeros
        x = np.zeros(n, dtype=np.float32)
        lo, hi = n // 3, max(n // 3 + 1, n // 2)
        x[lo:hi] = rng.standard_normal(hi - lo).astype(np.float32)
        return x
    if kind == "dc":
        return np.full(n, 0.625, dtype=np.float32)
    if kind == "tone":
        return np.sin(2.0 * np.pi * 440.0 * np.arange(n) / 16000.0).astype(np.float32)
    return np.zeros(n, dtype=np.float32)


def _shift(kind, n):
    return {"0": 0, "+1": 1, "-1": -1, "+n/5": n // 5, "-n/5": -(n // 5), ">=n": n, "<=-n": -n - 3}[kind]


# every length twice: (content, response, shift, out_len as "0" / "half" / "n" / "full")
_ROWS = (("noise", 0, "0", "full"), ("dc", 4, "0", "full"), ("noise", 1, "+1", "full"), ("tone", 2, "-1", "full"),
         ("noise", 8, "+n/5", "full"), ("noise", 3, "0", "full"), ("burst", 4, "-n/5", "full"), ("noise", 4, "+n/5", "n"),
         ("dc", 3, "+1", "n"), ("tone", 7, "-1", "full"), ("noise", 6, "0", "n"), ("zeros", 4, "0", "n"),
         ("noise", 3, ">=n", "full"), ("burst", 4, "0", "full"),
         ("dc", 2, "+1", "0"), ("noise", 5, "0", "n"), ("noise", 4, "-1", "half"), ("noise", 4, "+n/5", "full"),
         ("tone", 1, "0", "half"), ("burst", 8, "-1", "full"), ("noise", 7, "+1", "n"), ("tone", 3, "<=-n", "n"),
         ("noise", 0, "-n/5", "0"), ("noise", 4, "+1", "n"), ("noise", 3, "-1", "full"), ("noise", 8, "+n/5", "full"),
         ("noise", 0, "0", "half"), ("noise", 4, "-n/5", "n"))


def cases():
    """-> (bank, rows): the ragged batch of the GPU test.  A row is a dict ``name, x, shift, rir, out_len, twin``; ``twin``
    is the index of the row that differs from this one only in the non-finite sample being 0, or None."""
    bank = bank_responses()
    rng = np.random.default_rng(4242)
    rows = []
    for n, (kind, rir, shift_kind, mode) in zip(LENGTHS + LENGTHS, _ROWS):
        taps = bank[rir].size
        out_len = {"0": 0, "half": n // 2, "n": n, "full": n + taps - 1}[mode]
        shift = _shift(shift_kind, n)
        rows.append(dict(name=f"{kind} n={n} L={taps} shift={shift} out={out_len}", x=_content(kind, n, rng), shift=shift,
                         rir=rir, out_len=out_len, twin=None))
    for n, shift, out_len in ((16000, 0, 16000), (16385, -1, 16385), (255, 300, 255), (8193, 17, 8000)):    # copies
        rows.append(dict(name=f"copy n={n} shift={shift}", x=_content("noise", n, rng), shift=shift, rir=-1, out_len=out_len,
                         twin=None))
    # a NaN or an Inf at the first sample of a span, at the last, and 8192 before a span's start
    # the NaNs are negative and carry a payload: arithmetic hands such a NaN on as it is, the load-time rule writes QUIET_NAN
    loud = np.array([0xFFC12345], dtype=np.uint32).view(np.float32)[0]
    for at, value, rir, shift in ((16384, loud, 3, 0), (32767, np.inf, 4, 0), (8192, -np.inf, 2, 0), (32768 - 5, loud, 8, 5)):
        x = _content("noise", 48000, rng)
        clean = dict(name=f"twin of non-finite at {at}", x=x.copy(), shift=shift, rir=rir, out_len=48000 + bank[rir].size - 1,
                     twin=None)
        clean["x"][at] = 0.0
        x[at] = value
        rows.append(clean)
        rows.append(dict(name=f"{value} at x[{at}] shift={shift}", x=x, shift=shift, rir=rir, out_len=clean["out_len"],
                         twin=len(rows) - 1))
    return bank, rows


_EXPECTED = {}


def expected():
    """Computed once and shared: ``(bank, rows, width, exp)`` with ``exp[r]`` the dict ``ref`` (float64), ``bound``,
    ``emu`` (float32 emulation), ``bad`` / ``silent`` (per span) of row r."""
    if not _EXPECTED:
        bank, rows = cases()
        specs = [spectrum(h) for h in bank]
        exp = []
        for row in rows:
            h = bank[row["rir"]] if row["rir"] >= 0 else None
            clean = rows[row["twin"]]["x"] if row["twin"] is not None else row["x"]
            e = dict(ref=reverb_ref(clean, row["shift"], h, row["out_len"]),
                     emu=emulate(row["x"], row["shift"], h, row["out_len"], spec=specs[row["rir"]] if h is not None else None))
            if h is not None:
                e.update(bound=bound(clean, row["shift"], h, row["out_len"]), bad=bad_spans(row["x"], row["shift"], row["out_len"]),
                         silent=silent_spans(row["x"], row["shift"], row["out_len"]))
            exp.append(e)
        _EXPECTED["v"] = (bank, rows, max(max(r["out_len"] for r in rows), 1), exp)
    return _EXPECTED["v"]


def rms_errors(y, row, e):
    """(device RMS error, emulation RMS error) against float64 over the row's columns outside the NaN spans."""
    keep = np.ones(row["out_len"], dtype=bool)
    for w, bad in enumerate(e.get("bad", [])):
        if bad:
            keep[N * w:N * (w + 1)] = False
    if not keep.any():
        return 0.0, 0.0
    d = (np.asarray(y[:row["out_len"]], dtype=np.float64) - e["ref"])[keep]
    m = (e["emu"].astype(np.float64) - e["ref"])[keep]
    return math.sqrt(float((d * d).mean())), math.sqrt(float((m * m).mean()))


def check_row(y, row, e, width):
    """Every check the GPU test applies to one output row ``y`` (float32 (width,)); raises AssertionError."""
    name, out_len = row["name"], row["out_len"]
    y = np.asarray(y)
    assert y.dtype == np.float32 and y.shape == (width,), name
    assert not y[out_len:].view(np.uint32).any(), f"{name}: padding columns are not +0.0"
    if row["rir"] < 0:
        want = e["ref"].astype(np.float32)
        assert y[:out_len].view(np.uint32).tolist() == want.view(np.uint32).tolist(), f"{name}: the copy differs"
        return
    for w, (bad, silent) in enumerate(zip(e["bad"], e["silent"])):
        span = slice(N * w, min(N * (w + 1), out_len))
        if bad:
            assert np.isnan(y[span]).all(), f"{name}: span {w} holds a non-finite input and is not all NaN"
            # the rule's own NaN, not whatever the transform makes of an Inf: only the load-time OR writes these bits everywhere
            assert (y[span].view(np.uint32) == QUIET_NAN).all(), f"{name}: span {w} is NaN, but not by the load-time rule"
        elif silent:
            assert not y[span].any(), f"{name}: span {w} is silent and does not compare equal to zero"
        else:
            assert np.isfinite(y[span]).all(), f"{name}: span {w} is not finite"
            err = np.abs(y[span].astype(np.float64) - e["ref"][span])
            worst = int(np.argmax(err - e["bound"][span]))
            assert (err <= e["bound"][span]).all(), (f"{name}: column {N * w + worst} is off by {err[worst]:.3e}, the bound is "
                                                    f"{e['bound'][span][worst]:.3e}")
    dev, emu = rms_errors(y, row, e)
    assert dev <= RMS_FACTOR * emu, f"{name}: RMS error {dev:.3e} against the emulation's {emu:.3e} (x{dev / emu if emu else math.inf:.1f})"
