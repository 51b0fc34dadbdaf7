"""The waveform chain stated on its own, from its documented meaning: ``time shift -> speed -> pitch -> reverb -> gain and
noise``.  Nothing here imports ``cough_detector_amd.chain``, ``data`` or ``augmentation``; the arithmetic of each launch is
the restatement that launch already has (``warp_ref``, ``pitch_ref``, ``pitch_lock_ref``, ``reverb_ref``) and, for
``cough_augment_waveforms``, ``augment_ref`` below, written from the contract in ``include/cough_amd.h``.

* ``expected_links``: the ordered launches a batch must make -- ``warp``, ``stretch``, ``back`` (the resampling behind the
  stretch), ``reverb``, ``augment`` -- and per row what each reads, which shift and parameter its plan carries, what it
  writes and how wide its matrix is.
* ``link_ref``: the float64 result and the tolerance of one link on one float32 row.
* ``run_links`` / ``chain_ref``: a list of links executed in float64, each fed the float32 rounding of the one before, in
  the form ``tests/chain_trace.py`` records a real run in (``run_links`` executes whatever list it is given, a defective
  one too: the host test plants its defects that way).
* ``check_trace``: what a recorded (or executed) run has to satisfy.  Pure numpy.
* ``drawn_links``: the expected links of a ``draws="device"`` batch, from the restated draws.
* ``sensitivity``: how far the chain's result moves when every link's output is perturbed by that link's tolerance.

A link is a dict: ``kind``; per row the int arrays ``read`` (samples it reads), ``shift``, ``wrote`` (samples it writes;
zeros from there to ``width``) and ``leave`` (samples the next link reads), the list ``param`` -- ``(orig, new)`` for
``warp`` / ``back``, ``(rate, mode)`` for ``stretch``, ``(rir, out_len)`` for ``reverb``, None for ``augment`` -- and
``width``.  ``back`` writes ``min(ceil(n_s new / orig), width)`` samples, which may be a few more or fewer than the ``n'``
it leaves (torchaudio's crop or pad back to the length before the stretch): the only link whose two lengths differ.

A recorded link (``chain_trace``, ``run_links``) is a dict: ``kind``, ``rows`` (the float32 rows it was given), ``lengths``,
``shift`` and ``param`` as read back from its plans, ``out`` (float32 (B, width)); an ``augment`` link also holds
``records`` (``draws_ref.CLIP_DTYPE``), ``gaussian`` ((B, >= width) float32 or None) and ``bank`` (a list of float32 arrays).
"""
import hashlib
import math

import numpy as np

import draws_ref as D
import pitch_lock_ref as L
import pitch_ref as P
import reverb_ref as R
import warp_ref as W

REL = 1e-6                                   # of the row's peak: the figure of tests/test_gpu_waveform_augment.py
PHASE_LOCK = 1
KINDS = ("warp", "stretch", "back", "reverb", "augment")
MIN_MARGIN, MAX_E, MIN_ENV = 64.0, 2.0 ** -20, 0.25      # tests/test_pitch_host.py::test_the_inputs_are_fit_for_a_comparison
WHOLE_CHAIN_FACTOR = 4.0                     # the signs of ``sensitivity`` are sampled, not worst-case


# ------------------------------------------------------------------------------------------------ lengths and pairs
def warped_length(n, orig, new):
    return W.new_length(n, orig, new) if W.usable(orig, new) and orig != new else int(n)


def pitch_pair(n_steps, sample_rate):
    """(orig, new) of the resampling behind a stretch by ``n_steps`` semitones: ``(int(sr / rate), sr)``."""
    return int(sample_rate / P.pitch_rate(n_steps)), int(sample_rate)


def speed_width(row_len, lo, sample_rate):
    """The width a ``draws="device"`` batch with a speed step gives its matrices before it knows the draws: the longest
    row at the slowest factor."""
    return max(int(row_len), warped_length(row_len, int(float(lo) * sample_rate), int(sample_rate))) if row_len > 0 else 0


def pitch_width(row_len, lo, hi):
    """Likewise the width of the stretched rows: the longest row at every semitone count of the range."""
    return max([int(row_len)] + [P.stretched_length(row_len, P.pitch_rate(s)) for s in range(lo, hi + 1)]) if row_len > 0 else 0


# ------------------------------------------------------------------------------------------------ the links a batch must make
def expected_links(shifts, pairs, steps, rirs, lengths, n, sample_rate=16000, phase_lock=False, launches="fired",
                   copy_pair=(1, 1), width=None, stretch_width=None):
    """The ordered links of one batch.  Per row: ``shifts``; ``pairs`` (the speed step's ``(orig, new)`` or None),
    ``steps`` (semitones or None; 0 shifts nothing) and ``rirs`` (a response or None), each None as a whole when the step
    is switched off; ``lengths``; ``n`` is the width of the input rows.

    ``launches="fired"`` (host draws): a step's launch exists if and only if it fired for at least one row.
    ``launches="on"`` (device draws, which the host never sees): if and only if the step is switched on.  ``copy_pair`` is
    the pair of a row the resampler only copies: ``(1, 1)`` from the host, ``(sample_rate, sample_rate)`` from the device's
    draws.  ``width`` / ``stretch_width``: the widths of a caller that fixes them before the draws (``speed_width``,
    ``pitch_width``); by default the output is ``max n'`` wide with a speed step and ``n`` wide without, and the stretched
    rows ``max n_s``."""
    b = len(lengths)
    lengths = np.asarray([int(v) for v in lengths], dtype=np.int64)
    shifts = np.asarray([int(v) for v in shifts], dtype=np.int64)
    zero = np.zeros(b, dtype=np.int64)
    fired = {"speed": pairs is not None and any(p is not None for p in pairs),
             "pitch": steps is not None and any(bool(s) for s in steps),
             "reverb": rirs is not None and any(r is not None for r in rirs)}
    if launches == "on":
        fired = {"speed": pairs is not None, "pitch": steps is not None, "reverb": rirs is not None}
    elif launches != "fired":
        raise ValueError(launches)
    pair_of = [tuple(p) if (pairs is not None and p is not None) else None for p in (pairs or [None] * b)]
    new = np.asarray([l if p is None else warped_length(l, *p) for l, p in zip(lengths, pair_of)], dtype=np.int64)
    any_launch = any(fired.values())
    if width is None:
        width = (int(new.max()) if b else 0) if (pairs is not None and any_launch) else int(n)
    links = []
    if fired["speed"]:
        links.append(dict(kind="warp", read=lengths, param=[p or tuple(copy_pair) for p in pair_of], wrote=np.minimum(new, width),
                          leave=new, width=int(width)))
    if fired["pitch"]:
        semis = [int(s) if s else 0 for s in steps]
        rates = [P.pitch_rate(s) if s else 1.0 for s in semis]
        n_s = np.asarray([P.stretched_length(l, r) for l, r in zip(new, rates)], dtype=np.int64)
        if stretch_width is None:
            stretch_width = int(n_s.max()) if b else 0
        back = [pitch_pair(s, sample_rate) if s else tuple(copy_pair) for s in semis]
        links.append(dict(kind="stretch", read=new, param=[(r, PHASE_LOCK if phase_lock and s else 0) for r, s in zip(rates, semis)],
                          wrote=np.minimum(n_s, stretch_width), leave=np.minimum(n_s, stretch_width), width=int(stretch_width)))
        links.append(dict(kind="back", read=links[-1]["leave"], param=back,
                          wrote=np.asarray([min(warped_length(m, *p), width) for m, p in zip(links[-1]["leave"], back)], dtype=np.int64),
                          leave=new, width=int(width)))
    if fired["reverb"]:
        links.append(dict(kind="reverb", read=new, param=[(-1 if r is None else int(r), int(l)) for r, l in zip(rirs, new)],
                          wrote=new, leave=new, width=int(width)))
    links.append(dict(kind="augment", read=new, param=[None] * b, wrote=new, leave=new, width=int(width)))
    for k, link in enumerate(links):                                         # the first link of the list carries the shift
        link["shift"] = shifts.copy() if k == 0 else zero.copy()
    return links


# ------------------------------------------------------------------------------------------------ one link in float64
def augment_ref(x, shift, rec, z, bank):
    """``cough_augment_waveforms`` on one row, record-driven, in float64 (include/cough_amd.h): ``y[i] = x[i - shift]``
    inside the row, else 0; ``y *= gain``; with the gaussian step ``P = mean(y^2)``, ``Pz = mean(z^2)`` of the noise given,
    ``y += sqrt(P / (10^(snr / 10) Pz)) z``; with the bank step ``P = mean(y^2)`` again, the crop ``entry[(bank_start + i)
    % entry_len]``, ``y += sqrt(P / (10^(snr / 10) Pn)) crop`` when ``Pn = mean(crop^2) > 0``."""
    x = np.asarray(x, dtype=np.float32)
    n = x.size
    y = W.shifted(x, shift).astype(np.float64) * float(np.float32(rec["gain"]))
    if n and int(rec["gaussian"]):
        zz = np.asarray(z, dtype=np.float32)[:n].astype(np.float64)
        power, pz = float((y * y).mean()), float((zz * zz).mean())
        y = y + math.sqrt(power / (10.0 ** (float(rec["gaussian_snr_db"]) / 10.0) * pz)) * zz
    if n and int(rec["bank_index"]) >= 0:
        entry = np.asarray(bank[int(rec["bank_index"])], dtype=np.float32).astype(np.float64)
        crop = entry[(int(rec["bank_start"]) + np.arange(n, dtype=np.int64)) % entry.size]
        power, pn = float((y * y).mean()), float((crop * crop).mean())
        if pn > 0.0:
            y = y + math.sqrt(power / (10.0 ** (float(rec["bank_snr_db"]) / 10.0) * pn)) * crop
    return y


def _fitness(ref):
    """The figures ``test_the_inputs_are_fit_for_a_comparison`` asks of a stretched row: the floor margin, the least of
    the summed squared window over the kept range, and ``max E`` over the peak of ``y_ref``."""
    peak = float(np.abs(ref["y"]).max()) if ref["y"].size else 0.0
    return dict(margin=float(ref["margin"]), env_min=float(ref.get("env_min", math.inf)),
                e_over_peak=float(ref["E"].max() / peak) if peak > 0.0 else 0.0)


def link_ref(kind, x, shift, param, taps=None, aux=None):
    """One link on the float32 row ``x`` -> dict(``y`` float64, ``tol`` float64 per sample, ``copy``: the link only copies
    the (shifted) row, which must then come out bit for bit).  ``stretch`` adds ``fitness``; ``reverb`` needs ``taps`` (the
    bank's float32 responses) and adds ``row`` / ``e``, what ``reverb_ref.check_row`` takes; ``augment`` needs ``aux`` =
    ``(record, gaussian row or None, noise bank)``."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    shift = int(shift)
    if kind in ("warp", "back"):
        orig, new = int(param[0]), int(param[1])
        y, a, _ = W.warp_ref(x, shift, orig, new)
        return dict(y=y, tol=W.bound_factor(orig, new) * a if W.usable(orig, new) else np.zeros(y.size),
                    copy=not W.usable(orig, new) or orig == new)
    if kind == "stretch":
        rate, mode = float(param[0]), int(param[1])
        if not P.stretchable(rate, x.size):
            return dict(y=W.shifted(x, shift).astype(np.float64), tol=np.zeros(x.size), copy=True, fitness=None)
        ref = P.stretch_ref(x, shift, rate)
        if mode & PHASE_LOCK:                                                # the envelope is the plain stretch's: the same frames
            ref = dict(L.stretch_lock_ref(x, shift, rate), env_min=ref.get("env_min", math.inf))
        return dict(y=ref["y"], tol=2.0 ** -24 * np.abs(ref["y"]) + ref["E"], copy=False, fitness=_fitness(ref))
    if kind == "reverb":
        rir, out_len = int(param[0]), int(param[1])
        if rir < 0:
            return dict(y=R.reverb_ref(x, shift, None, out_len), tol=np.zeros(out_len), copy=True)
        h = taps[rir]
        row = dict(name=f"reverb n={x.size} rir={rir} shift={shift} out={out_len}", x=x, shift=shift, rir=rir, out_len=out_len, twin=None)
        e = dict(ref=R.reverb_ref(x, shift, h, out_len), emu=R.emulate(x, shift, h, out_len, spec=_spectrum(h)),
                 bound=R.bound(x, shift, h, out_len), bad=R.bad_spans(x, shift, out_len), silent=R.silent_spans(x, shift, out_len))
        return dict(y=e["ref"], tol=e["bound"], copy=False, row=row, e=e)
    if kind == "augment":
        rec, z, bank = aux
        y = augment_ref(x, shift, rec, z, bank)
        return dict(y=y, tol=np.full(y.size, REL * (float(np.abs(y).max()) if y.size else 0.0)), copy=False)
    raise ValueError(kind)


_SPECTRA, _CACHE = {}, {}


def _spectrum(h):
    key = hashlib.sha1(np.ascontiguousarray(h, dtype=np.float32).tobytes()).digest()
    if key not in _SPECTRA:
        _SPECTRA[key] = R.spectrum(h)
    return _SPECTRA[key]


def cached_link_ref(kind, x, shift, param, taps=None, aux=None):
    """``link_ref``, remembered by the bytes of its input: the configurations of a test share most of their rows."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    h = hashlib.sha1(x.tobytes())
    h.update(repr((kind, int(shift), tuple(param) if param is not None else None)).encode())
    if kind == "reverb" and int(param[0]) >= 0:
        h.update(np.ascontiguousarray(taps[int(param[0])], dtype=np.float32).tobytes())
    if kind == "augment":
        rec, z, bank = aux
        h.update(np.asarray(rec).tobytes())
        if int(rec["gaussian"]):
            h.update(np.ascontiguousarray(z, dtype=np.float32)[:x.size].tobytes())
        if int(rec["bank_index"]) >= 0:
            h.update(np.ascontiguousarray(bank[int(rec["bank_index"])], dtype=np.float32).tobytes())
    key = h.digest()
    if key not in _CACHE:
        _CACHE[key] = link_ref(kind, x, shift, param, taps=taps, aux=aux)
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------ the chain in float64
def run_links(links, source, records=None, gaussian=None, bank=(), taps=None, perturb=None, stop_after=None):
    """The links executed one after the other in float64, each fed the float32 rounding of the one before (the first
    one ``source``, a list of float32 rows) -> the recorded links, in ``chain_trace``'s form, each with ``y64`` (per row
    the float64 result) besides.  The list is executed as it stands, whatever it says: a link reads ``read`` samples of
    what lies in front of it, applies its ``shift`` and ``param`` and writes ``wrote`` samples; a link with ``late_shift``
    resamples first and shifts afterwards.  ``perturb``: a ``numpy.random.Generator``; every sample of every link's result
    then moves by that link's tolerance, with a random sign, before it is rounded."""
    trace, prev = [], None
    b = len(source)
    for link in links:
        kind, width = link["kind"], int(link["width"])
        out = np.zeros((b, max(width, 0)), dtype=np.float32)
        rows, y64 = [], []
        for r in range(b):
            have = prev[r] if prev is not None else np.asarray(source[r], dtype=np.float32)
            x = np.ascontiguousarray(have[:int(link["read"][r])], dtype=np.float32)
            shift = int(link["shift"][r])
            aux = (records[r], None if gaussian is None else gaussian[r], bank) if kind == "augment" else None
            if link.get("late_shift"):
                y = W.shifted(cached_link_ref(kind, x, 0, link["param"][r], taps=taps, aux=aux)["y"], shift)
                tol = np.zeros(y.size)
            else:
                ref = cached_link_ref(kind, x, shift, link["param"][r], taps=taps, aux=aux)
                y, tol = ref["y"], ref["tol"]
            if perturb is not None:                                          # a copy has the tolerance 0 and stays a copy
                y = y + tol * perturb.choice([-1.0, 1.0], size=y.size)
            k = min(int(link["wrote"][r]), y.size, width)
            out[r, :k] = y[:k].astype(np.float32)
            rows.append(x)
            y64.append(y)
        rec = dict(kind=kind, rows=rows, lengths=np.asarray(link["read"], dtype=np.int64).copy(),
                   shift=np.asarray(link["shift"], dtype=np.int64).copy(), param=list(link["param"]), out=out, y64=y64)
        if kind == "augment":
            rec.update(records=np.asarray(records).copy(), gaussian=gaussian, bank=list(bank))
            rec["records"]["shift"] = rec["shift"]
        trace.append(rec)
        prev = [out[r] for r in range(b)]
        if kind == stop_after:
            break
    return trace


def chain_ref(source, shifts, pairs, steps, rirs, records, gaussian, bank, taps, n=None, sample_rate=16000, phase_lock=False,
              **kw):
    """The whole chain in float64 on the float32 rows ``source`` with the host's draws -> ``(trace, links)``: the executed
    ``expected_links`` and the links themselves.  The result is ``trace[-1]["out"]``."""
    lengths = [len(x) for x in source]
    links = expected_links(shifts, pairs, steps, rirs, lengths, max(lengths) if n is None else n, sample_rate, phase_lock)
    return run_links(links, source, records, gaussian, bank, taps, **kw), links


def sensitivity(links, source, records, gaussian, bank, taps, seeds=8):
    """How far the chain's result moves when every sample of every link's result is moved by that link's own tolerance
    with a random sign: per row the worst ``|moved - plain|`` over ``seeds`` draws of the signs, and that over the row's
    peak -> ``(absolute (B,), relative (B,))``."""
    plain = run_links(links, source, records, gaussian, bank, taps)[-1]["out"].astype(np.float64)
    worst = np.zeros(len(source))
    for seed in range(seeds):
        moved = run_links(links, source, records, gaussian, bank, taps, perturb=np.random.default_rng(1000 + seed))[-1]["out"]
        worst = np.maximum(worst, np.abs(moved.astype(np.float64) - plain).max(axis=1))
    peak = np.abs(plain).max(axis=1)
    return worst, worst / np.where(peak > 0, peak, 1.0)


# ------------------------------------------------------------------------------------------------ what a run has to satisfy
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_param(kind, got, want):
    if kind == "augment":
        return True
    if kind == "stretch":                                                    # the rate is a float64 word: the same bits
        return np.float64(got[0]).tobytes() == np.float64(want[0]).tobytes() and int(got[1]) == int(want[1])
    return tuple(int(v) for v in got) == tuple(int(v) for v in want)


def check_trace(trace, expected, source=None, float_checks=True, taps=None, last_values=True, worst=None):
    """Raises AssertionError unless the recorded ``trace`` is the chain ``expected`` describes:

    * ``links``: the kinds, in order;
    * ``input``: every link read exactly the expected number of samples per row, and they are, bit for bit, what the link
      before it wrote (``source`` for the first);
    * ``plan``: the shift and the parameter in every plan word are the expected ones -- so one link carries the shift, the
      first, and the augmentation records carry none whenever a launch ran before them;
    * ``layout``: every matrix has the expected width and every row is zero from the length it wrote to the width;
    * with ``float_checks``, ``value``: every row of every link lies inside ``link_ref``'s tolerance of that link's own
      recorded input, a row the link only copies is the same bits (NaN payloads included), a reverberated row passes
      ``reverb_ref.check_row``; and ``fitness``: every stretched row's recorded input is fit for the comparison.
      ``last_values=False`` leaves out the values of the last link (its noise was drawn on the device).

    ``worst``: a dict that receives the worst ``|y - y_ref| / tolerance`` per kind."""
    kinds = [link["kind"] for link in trace]
    assert kinds == [link["kind"] for link in expected], f"links: ran {kinds}, expected {[link['kind'] for link in expected]}"
    carried = np.zeros(len(expected[0]["shift"]), dtype=np.int64)
    for k, (got, want) in enumerate(zip(trace, expected)):
        kind, b = want["kind"], len(want["read"])
        where = f"link {k} ({kind})"
        assert len(got["rows"]) == b and len(got["lengths"]) == b, f"input: {where} got {len(got['rows'])} rows, expected {b}"
        for r in range(b):
            n = int(want["read"][r])
            assert int(got["lengths"][r]) == n and got["rows"][r].size == n, \
                f"input: {where} row {r} read {int(got['lengths'][r])} samples, expected {n}"
            if k == 0 and source is None:
                continue
            before = np.asarray(source[r], dtype=np.float32)[:n] if k == 0 else trace[k - 1]["out"][r, :n]
            assert before.size == n and (_bits(got["rows"][r]) == _bits(before)).all(), \
                f"input: {where} row {r} did not read what " + ("the source holds" if k == 0 else f"link {k - 1} wrote")
        for r in range(b):
            assert int(got["shift"][r]) == int(want["shift"][r]), \
                f"plan: {where} row {r} carries the shift {int(got['shift'][r])}, expected {int(want['shift'][r])}"
            assert _same_param(kind, got["param"][r], want["param"][r]), \
                f"plan: {where} row {r} has {got['param'][r]}, expected {want['param'][r]}"
        carried += (np.asarray(got["shift"]) != 0)
        out = got["out"]
        assert out.dtype == np.float32 and out.shape == (b, int(want["width"])), \
            f"layout: {where} wrote a {out.shape} matrix, expected {(b, int(want['width']))}"
        for r in range(b):
            assert not out[r, int(want["wrote"][r]):].any(), f"layout: {where} row {r} is not zero from {int(want['wrote'][r])} on"
        if not float_checks or (kind == "augment" and not last_values and k == len(expected) - 1):
            continue
        for r in range(b):
            aux = (got["records"][r], None if got["gaussian"] is None else got["gaussian"][r], got["bank"]) if kind == "augment" else None
            ref = cached_link_ref(kind, got["rows"][r], got["shift"][r], got["param"][r], taps=taps, aux=aux)
            m = int(want["wrote"][r])
            assert ref["y"].size >= m or kind == "reverb", f"value: {where} row {r}: the reference holds {ref['y'].size} samples, not {m}"
            y, y_ref, tol = out[r, :m], ref["y"][:m], ref["tol"][:m]
            if ref["copy"]:
                assert (_bits(y) == _bits(y_ref.astype(np.float32))).all(), f"value: {where} row {r} is a copy and not the same bits"
                continue
            if kind == "stretch":
                f = ref["fitness"]
                assert f["margin"] >= MIN_MARGIN and f["e_over_peak"] <= MAX_E and f["env_min"] >= MIN_ENV, \
                    f"fitness: {where} row {r}: margin {f['margin']:.3g}, max E / peak {f['e_over_peak']:.3g}, env_min {f['env_min']:.3g}"
            if kind == "reverb":
                R.check_row(out[r], ref["row"], ref["e"], out.shape[1])
                dev, emu = R.rms_errors(out[r], ref["row"], ref["e"])
                if worst is not None and emu:
                    worst["reverb rms / emulation"] = max(worst.get("reverb rms / emulation", 0.0), dev / emu)
            err = np.abs(y.astype(np.float64) - y_ref)
            live = tol > 0
            if worst is not None and live.any():
                worst[kind] = max(worst.get(kind, 0.0), float((err[live] / tol[live]).max()))
            at = int(np.argmax(err - tol)) if m else 0
            assert np.isfinite(y).all() and (err <= tol).all(), \
                f"value: {where} row {r} sample {at} is off by {err[at]:.3e}, the tolerance is {tol[at]:.3e}" if m else where
    shifted = np.asarray(expected[0]["shift"]) != 0
    assert (carried[shifted] == 1).all() and not carried[~shifted].any(), f"plan: the shift is carried {carried.tolist()} times per row"


# ------------------------------------------------------------------------------------------------ the device's draws
def drawn_links(seed, lengths, p, on, speed_range=(0.9, 1.1), pitch_range=(-2, 2), n_rirs=0, bank_lengths=(), sample_rate=16000,
                phase_lock=False):
    """The expected links of a ``draws="device"`` batch under ``seed`` -> ``(links, records)``.  ``on``: which of (speed,
    pitch, reverb) the augmentor has.  The draws are the restated ones (``warp_ref.draw_speed_ref``,
    ``pitch_ref.draw_pitch_ref``, ``reverb_ref.draw_reverb_ref``, ``draws_ref.draw_ref``): the speed step draws first, for
    the rows' lengths; everything else is drawn for ``n'``, and with a speed step the record's shift is the one the speed
    draw made for ``n``.  The widths are fixed before the draws; a step that is on launches whatever it drew."""
    speed, pitch, reverb = on
    lengths = [int(v) for v in lengths]
    row_len = max(lengths)
    pairs = steps = rirs = None
    new = np.asarray(lengths, dtype=np.int32)
    if speed:
        plans, new, _ = W.draw_speed_ref(seed, lengths, p, speed_range[0], speed_range[1], sample_rate)
        pairs = [(int(o), int(m)) for _, o, m in plans]
        row_len = speed_width(row_len, speed_range[0], sample_rate)
    if pitch:
        _, _, _, semis, fired = P.draw_pitch_ref(seed, new, p, pitch_range[0], pitch_range[1], sample_rate)
        steps = [int(s) if f else None for s, f in zip(semis, fired)]
    if reverb:
        rev = R.draw_reverb_ref(seed, new, p, n_rirs)
        rirs = [int(r) if r >= 0 else None for r in rev[:, 1]]
    records, _, _ = D.draw_ref(seed, new, p, list(bank_lengths), None, 0, 0, 0, 0, 1, 1)
    if speed:
        records["shift"] = plans[:, 0]
    links = expected_links(records["shift"], pairs, steps, rirs, lengths, row_len, sample_rate, phase_lock, launches="on",
                           copy_pair=(sample_rate, sample_rate), width=row_len,
                           stretch_width=pitch_width(row_len, *pitch_range) if pitch else None)
    return links, records


# ------------------------------------------------------------------------------------------------ the shared batch
# The smallest sizes that matter: below 257 samples the stretch copies, 4097 crosses a warp tile, 16385 needs two reverb
# spans.  Row 1 is stretched only behind the speed step (256 -> 274) and row 2 only without it (257 -> 215): a pitch step
# that read n instead of n' would take the other path.  Row 3 is shifted by its whole length.
LENGTHS = [2, 256, 257, 700, 4097, 9000, 16385, 20000]
SHIFTS = [1, -51, 0, 700, -819, 1800, -3277, 4000]
PAIRS = [(19200, 16000), (15000, 16000), (19200, 16000), None, (15000, 16000), None, (19200, 16000), (15000, 16000)]
STEPS = [1, -2, 2, None, 0, -1, 2, 1]
RIRS = [0, None, 3, 6, None, 2, 5, 1]
IDLE_STEPS = [None, 0, None, None, 0, None, None, 0]                          # semitones of 0 are drawn and shift nothing
BANK_LENGTHS = (700, 9000)
N_RIRS = 7
STATES = ("off", "idle", "fired")
CONFIGS = [(s, p, r) for s in STATES for p in STATES for r in STATES]        # all 27
ON_CONFIGS = [c for c in CONFIGS if "off" not in c]                           # the 8 fired / not fired with every step on


def batch_rows(seed=20261020):
    """The rows: uniform noise under an envelope, float32."""
    rng = np.random.default_rng(seed)
    return [((rng.random(n) - 0.5) * 0.8 * np.linspace(0.4, 1.0, n)).astype(np.float32) for n in LENGTHS]


def batch_noise(seed=20261021):
    """``(gaussian (B, 22000) float32, noise bank: two float32 entries)``."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((len(LENGTHS), 22000)).astype(np.float32), [(rng.standard_normal(n) * 0.3).astype(np.float32)
                                                                           for n in BANK_LENGTHS]


def batch_draws(config):
    """``(shifts, pairs, steps, rirs)`` of one configuration: each of (speed, pitch, reverb) off, on with nothing fired, or
    fired.  Where the augmentation record carries the shift, row 3's is 699: the record's contract refuses ``|shift| >=
    len`` (include/cough_amd.h), the three launches in front of it take it."""
    speed, pitch, reverb = config
    none = [None] * len(LENGTHS)
    pick = lambda state, fired, idle: None if state == "off" else (list(idle) if state == "idle" else list(fired))   # noqa: E731
    shifts = list(SHIFTS)
    if "fired" not in config:
        shifts[3] = LENGTHS[3] - 1
    return shifts, pick(speed, PAIRS, none), pick(pitch, STEPS, IDLE_STEPS), pick(reverb, RIRS, none)


def batch_records(shifts, new_lengths):
    """The augmentation records of the batch (``draws_ref.CLIP_DTYPE``): gain on most rows, the gaussian step on five,
    the bank step on four, the crop start valid for the row's length after the chain."""
    rec = np.zeros(len(LENGTHS), dtype=D.CLIP_DTYPE)
    rec["shift"] = shifts
    rec["gain"] = [1.0, 0.8, 1.2, 0.9, 1.0, 1.1, 0.75, 1.3]
    rec["gaussian"] = [1, 0, 1, 1, 0, 1, 1, 0]
    rec["gaussian_snr_db"] = [12.0 + 2.0 * r if g else 0.0 for r, g in enumerate(rec["gaussian"])]
    rec["bank_index"] = [-1, 0, 1, -1, 0, 1, 0, -1]
    for r, (k, n) in enumerate(zip(rec["bank_index"], new_lengths)):
        if k >= 0:
            rep = int(D.repeated_length(np.int64(BANK_LENGTHS[k]), np.int64(n)))
            rec["bank_snr_db"][r], rec["bank_start"][r] = 6.0 + r, min(37 * r + 5, rep - int(n))
    return rec


def measure(taps, lock=False, seeds=8):
    """The whole-chain figures of ``profiles/chain_links.txt``: ``sensitivity`` of the all-fired configuration -> per row
    the worst ``|moved - plain|`` over the row's peak."""
    rows, (gaussian, bank) = batch_rows(), batch_noise()
    shifts, pairs, steps, rirs = batch_draws(("fired", "fired", "fired"))
    links = expected_links(shifts, pairs, steps, rirs, LENGTHS, max(LENGTHS), phase_lock=lock)
    return sensitivity(links, rows, batch_records(shifts, links[-1]["read"]), gaussian, bank, taps, seeds)[1]


# ``measure`` as it came out (8 seeds), per row, plain and phase-locked: what the GPU test allows WHOLE_CHAIN_FACTOR times
# of between the device's final output and ``chain_ref``'s.  Nearly all of it is the reverb link's bound (K = 160 float32
# roundings of the span's norm), which is why the short rows that only the reverb changes move most for their size; row 3
# is shifted out and stays exactly zero.  tests/test_chain_ref_host.py measures again and compares.
WHOLE_CHAIN_MOVED = {False: [3.205e-4, 3.694e-6, 6.199e-4, 0.0, 3.250e-6, 2.916e-3, 1.603e-3, 5.570e-3],
                     True: [3.205e-4, 3.694e-6, 6.199e-4, 0.0, 3.250e-6, 3.675e-3, 1.435e-3, 5.258e-3]}


# the draws="device" cases of the GPU test: every on / off combination of (speed, pitch, reverb) at two seeds
DEVICE_SEEDS = (7, 2**63 + 12345)
DEVICE_P = 0.5
DEVICE_CASES = [(seed, (s, p, r)) for seed in DEVICE_SEEDS for s in (False, True) for p in (False, True) for r in (False, True)]


def device_links(seed, on):
    """``drawn_links`` of the shared batch under the shipped ranges."""
    return drawn_links(seed, LENGTHS, DEVICE_P, on, n_rirs=N_RIRS, bank_lengths=BANK_LENGTHS)
