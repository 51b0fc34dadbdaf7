"""Offline scoring without a GPU: the fifth library's symbols and argument checks, the build's staleness rule, the
Python front's parameter checks, and the restatement (tests/score_ref.py) on hand-built sequences whose answers are
known."""
import math
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

import cough_detector_amd as cda
from cough_detector_amd import _lib
from cough_detector_amd import build as cbuild
from cough_detector_amd import score as cscore
import score_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cough_amd_score.h")
SHIPPED = dict(use_pcen=False, use_pre_emphasis=False, use_delta_delta=False, use_spectral_contrast=False)


# ------------------------------------------------------------------------------------------------ the library
def _exported(path):
    nm = shutil.which("nm") or os.path.join(os.path.dirname(os.path.realpath(cbuild._hipcc())), "..", "lib", "llvm", "bin", "llvm-nm")
    out = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_score_library_exports_exactly_its_header():
    text = open(HEADER).read()
    declared = set(re.findall(r"\b(cough_[a-z_0-9]+)\s*\(", text))
    assert declared == set(_lib.SCORE_SYMBOLS), declared ^ set(_lib.SCORE_SYMBOLS)
    assert len(_lib.SCORE_SYMBOLS) == len(set(_lib.SCORE_SYMBOLS)) == 5
    lib = _lib.load_score()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.cough_score_abi_version() == 1
    assert "#define COUGH_SCORE_ABI_VERSION 1" in text
    assert re.search(rf"#define COUGH_MAX_SMOOTHING {_lib.MAX_SMOOTHING}\b", text) and _lib.MAX_SMOOTHING == 32
    assert re.search(rf"#define COUGH_MAX_THRESHOLDS {_lib.MAX_THRESHOLDS}\b", text) and _lib.MAX_THRESHOLDS == 1024
    assert _exported(_lib.SCORE_LIB_PATH) == declared


def test_the_other_four_libraries_are_untouched():
    others = (("cough_amd.h", _lib.SYMBOLS, _lib.LIB_PATH, 53, _lib.load().cough_amd_abi_version(), 5),
              ("cough_amd_loop.h", _lib.LOOP_SYMBOLS, _lib.LOOP_LIB_PATH, 3, _lib.load_loop().cough_loop_abi_version(), 1),
              ("cough_amd_data.h", _lib.DATA_SYMBOLS, _lib.DATA_LIB_PATH, 5, _lib.load_data().cough_data_abi_version(), 1),
              ("cough_amd_segments.h", _lib.SEGMENTS_SYMBOLS, _lib.SEGMENTS_LIB_PATH, 6,
               _lib.load_segments().cough_segments_abi_version(), 1))
    for header, symbols, path, count, version, want in others:
        assert len(symbols) == count and version == want, header
        assert not set(_lib.SCORE_SYMBOLS) & set(symbols), header
        assert _exported(path) == set(symbols), header
        text = open(os.path.join(ROOT, "include", header)).read()
        for s in _lib.SCORE_SYMBOLS:
            assert s not in text, (header, s)


FAKE = 1 << 20


def _err():
    return _lib.load_score().cough_score_last_error()


def test_smooth_windows_refuses_bad_arguments_without_a_gpu():
    lib = _lib.load_score()

    def call(prob=FAKE, offs=FAKE, n=3, windows=100, w=3, out=FAKE):
        return lib.cough_smooth_windows(prob, offs, n, windows, w, out, None)

    E = _lib.EINVAL
    for kw in ("prob", "offs", "out"):
        assert call(**{kw: None}) == E and b"NULL" in _err() and b"cough_smooth_windows" in _err(), kw
    assert call(n=-1) == E and b"n_clips" in _err() and b"cough_smooth_windows" in _err()
    for v in (-1, 1 << 38):
        assert call(windows=v) == E and b"n_windows" in _err(), v
    for v in (0, 33, -1):
        assert call(w=v) == E and b"smoothing_window" in _err() and b"cough_smooth_windows" in _err(), v
    assert call(prob=FAKE + 2) == E and b"4-byte" in _err()
    for kw in ("offs", "out"):
        assert call(**{kw: FAKE + 4}) == E and b"8-byte" in _err() and b"cough_smooth_windows" in _err(), kw
    for w in (1, 32):
        assert call(n=0, w=w) == _lib.OK and call(windows=0, w=w) == _lib.OK     # nothing to do: no launch
    with pytest.raises(ValueError, match="cough_smooth_windows: .*smoothing_window"):
        _lib.check_score(call(w=0), "cough_smooth_windows")
    assert b"smoothing_window" not in _lib.load_segments().cough_segments_last_error()   # the messages stay apart


def test_sweep_thresholds_refuses_bad_arguments_without_a_gpu():
    lib = _lib.load_score()

    def call(s=FAKE, offs=FAKE, n=3, windows=100, thr=FAKE, nt=101, gap=2, counts=FAKE, first=FAKE, conf=FAKE, at=FAKE):
        return lib.cough_sweep_thresholds(s, offs, n, windows, thr, nt, gap, counts, first, conf, at, None)

    E = _lib.EINVAL
    for kw in ("s", "offs", "thr"):
        assert call(**{kw: None}) == E and b"NULL" in _err() and b"cough_sweep_thresholds" in _err(), kw
    assert call(n=-1) == E and b"n_clips" in _err()
    assert call(windows=-1) == E and b"n_windows" in _err()
    for v in (0, 1025, -1):
        assert call(nt=v) == E and b"n_thresholds" in _err() and b"cough_sweep_thresholds" in _err(), v
    for v in (0, -1):
        assert call(gap=v) == E and b"gap" in _err(), v
    for kw in ("counts", "first", "at"):
        assert call(**{kw: FAKE + 2}) == E and b"4-byte" in _err() and b"cough_sweep_thresholds" in _err(), kw
    for kw in ("s", "offs", "thr", "conf"):
        assert call(**{kw: FAKE + 4}) == E and b"8-byte" in _err(), kw
    for nt in (1, 1024):
        assert call(n=0, nt=nt) == _lib.OK
    assert call(n=0, counts=None, first=None, conf=None, at=None) == _lib.OK     # every output is optional


def test_list_events_refuses_bad_arguments_without_a_gpu():
    lib = _lib.load_score()

    def call(s=FAKE, offs=FAKE, n=3, windows=100, t=0.5, gap=2, eoffs=FAKE, events=7, at=FAKE, conf=FAKE):
        return lib.cough_list_events(s, offs, n, windows, t, gap, eoffs, events, at, conf, None)

    E = _lib.EINVAL
    for kw in ("s", "offs", "eoffs", "at", "conf"):
        assert call(**{kw: None}) == E and b"NULL" in _err() and b"cough_list_events" in _err(), kw
    assert call(n=-1) == E and b"n_clips" in _err()
    assert call(windows=-1) == E and b"n_windows" in _err()
    assert call(events=-1) == E and b"n_events" in _err()
    assert call(t=math.nan) == E and b"threshold" in _err() and b"cough_list_events" in _err()
    for v in (0, -5):
        assert call(gap=v) == E and b"gap" in _err(), v
    assert call(at=FAKE + 2) == E and b"4-byte" in _err()
    for kw in ("s", "offs", "eoffs", "conf"):
        assert call(**{kw: FAKE + 4}) == E and b"8-byte" in _err() and b"cough_list_events" in _err(), kw
    assert call(n=0) == _lib.OK and call(events=0) == _lib.OK
    assert call(n=0, t=math.inf) == _lib.OK                                      # a threshold nothing reaches is legal


# ------------------------------------------------------------------------------------------------ the Python front
def _cpu_scores(per_clip=(3, 0, 5), w=3):
    n = int(sum(per_clip))
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(per_clip)]), dtype=torch.int64)
    return cda.WindowScores(torch.zeros(n), torch.zeros(n, dtype=torch.float64), offsets, offsets.clone(), 4000, 16000, 16000, w)


def _cpu_bank():
    return cda.DeviceClipBank([torch.zeros(800), torch.ones(20000), torch.ones(40000)], [0, 1, 0], device="cpu")


def test_the_package_exports_the_scorer():
    for name in ("WindowScores", "ThresholdSweep", "EventTable", "score_bank", "sweep_thresholds", "detect_events",
                 "event_windows", "detection_report"):
        assert name in cda.__all__ and getattr(cda, name) is getattr(cscore, name), name


def test_bad_parameters_raise_before_any_launch():
    # a CPU bank / CPU scores would raise RuntimeError at the launch: a ValueError shows the check came first
    bank, pipe = _cpu_bank(), types.SimpleNamespace(pre=cda.AudioPreprocessor(**SHIPPED))
    for v in (0, 33, -1, 3.0, True, None):
        with pytest.raises(ValueError, match="smoothing_window"):
            cda.score_bank(bank, pipe, smoothing_window=v)
        with pytest.raises(ValueError, match="smoothing_window"):
            cda.WindowScores.from_probabilities(torch.zeros(4), [4], 4000, 16000, 16000, v, device="cpu")
    for v in (0.0, 1e-6, -0.25, math.nan, math.inf, "quarter"):
        with pytest.raises(ValueError, match="hop"):
            cda.score_bank(bank, pipe, hop_duration=v)
    for v in (0, -4, 2.5, True):
        with pytest.raises(ValueError, match="batch"):
            cda.score_bank(bank, pipe, batch=v)
    scores = _cpu_scores()
    for v in ([], [0.5, math.nan], [math.inf], [-math.inf, 0.2], np.linspace(0, 1, 1025), "half"):
        with pytest.raises(ValueError, match="thresholds"):
            cda.sweep_thresholds(scores, v)
    for v in (math.nan, math.inf, None):
        with pytest.raises(ValueError, match="threshold"):
            cda.detect_events(scores, threshold=v)
    for v in (-0.1, math.nan, math.inf, "long"):
        with pytest.raises(ValueError, match="debounce_seconds"):
            cda.sweep_thresholds(scores, [0.5], debounce_seconds=v)
        with pytest.raises(ValueError, match="debounce_seconds"):
            cda.detect_events(scores, 0.5, debounce_seconds=v)
    with pytest.raises(ValueError, match="probabilities"):
        cda.WindowScores.from_probabilities(torch.zeros(5), [4], 4000, 16000, 16000, 3, device="cpu")
    with pytest.raises(ValueError, match="hop_samples"):
        cda.WindowScores.from_probabilities(torch.zeros(4), [4], 0, 16000, 16000, 3, device="cpu")


def test_data_off_the_gpu_cannot_launch():
    bank, pipe, scores = _cpu_bank(), types.SimpleNamespace(pre=cda.AudioPreprocessor(**SHIPPED)), _cpu_scores()
    sweep = cda.ThresholdSweep(torch.tensor([0.5], dtype=torch.float64), torch.zeros((3, 1), dtype=torch.int32),
                               torch.zeros((3, 1), dtype=torch.int32), torch.zeros(3, dtype=torch.float64),
                               torch.zeros(3, dtype=torch.int32), 2)
    events = cda.EventTable(torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int32),
                            torch.zeros(0, dtype=torch.float64), torch.zeros(0, dtype=torch.float64),
                            torch.zeros(3, dtype=torch.int32))
    for call in (lambda: cda.score_bank(bank, pipe),
                 lambda: cda.WindowScores.from_probabilities(torch.zeros(4), [4], 4000, 16000, 16000, 3, device="cpu"),
                 lambda: cda.sweep_thresholds(scores, [0.5]), lambda: cda.detect_events(scores, 0.5),
                 lambda: cda.event_windows(bank, scores, events), lambda: cda.detection_report(bank, scores, sweep)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_window_counts_follow_the_rule():
    lengths = np.array([1, 100, 15999, 16000, 16001, 19999, 20000, 24001, 52000, 160000])
    assert cscore.windows_per_clip(lengths, 16000, 4000).tolist() == [0, 0, 0, 1, 1, 1, 2, 3, 10, 37]
    assert cscore.windows_per_clip(lengths, 16000, 4000).dtype == np.int64
    assert cscore.windows_per_clip(lengths, 8000, 1600).tolist() == [R.windows_per_clip(int(n), 8000, 1600) for n in lengths]
    assert cscore.hop_samples("t", 16000, 0.25) == 4000 and cscore.hop_samples("t", 16000, 0.1) == 1600


@pytest.mark.parametrize("debounce,sr,hop,want", [(0.5, 16000, 4000, 2), (0.0, 16000, 4000, 1), (0.0, 8000, 1, 1),
                                                  (0.6, 16000, 4000, 3), (10.0, 16000, 4000, 40), (0.3, 16000, 1600, 3),
                                                  (0.25, 16000, 4000, 1), (0.2500001, 16000, 4000, 2)])
def test_the_debounce_gap(debounce, sr, hop, want):
    assert R.gap_ref(debounce, sr, hop) == want
    g = cscore.debounce_gap(debounce, sr, hop)
    assert g == want and g >= 1 and g * hop >= debounce * sr and (g == 1 or (g - 1) * hop < debounce * sr)


def test_the_debounce_gap_is_checked_by_its_inequality():
    rng = np.random.default_rng(0)
    for _ in range(2000):
        d, sr, hop = float(rng.uniform(0, 20)), int(rng.integers(1, 48001)), int(rng.integers(1, 20001))
        g = cscore.debounce_gap(d, sr, hop)
        assert g >= 1 and g * hop >= d * sr and (g == 1 or (g - 1) * hop < d * sr), (d, sr, hop, g)
    for k in range(1, 200):                                                # exact multiples: g = k, not k + 1
        assert cscore.debounce_gap(k * 0.25, 16000, 4000) == k


# ------------------------------------------------------------------------------------------------ the restatement
def test_reference_fires_every_gap_windows():
    s = R.smooth_ref([0.9] * 10, 1)
    assert R.events_ref(s, 0.5, 2) == [0, 2, 4, 6, 8]
    assert R.events_ref(s, 0.5, 1) == list(range(10)) and R.events_ref(s, 0.5, 40) == [0]
    assert R.events_ref(s, 0.95, 2) == []


def test_reference_smoothing_delays_the_first_fire():
    p = [0, 0, 0.75, 0.75, 0.75, 0, 0, 0, 0, 0]
    s = R.smooth_ref(p, 3)
    assert s[:6].tolist() == [0.0, 0.0, 0.25, 0.5, 0.75, 0.5]
    assert R.events_ref(s, 0.5, 2)[0] == 3
    assert R.events_ref(R.smooth_ref(p, 1), 0.5, 2)[0] == 2


def test_reference_compares_with_greater_or_equal():
    s = R.smooth_ref([0.5] * 9, 3)
    assert (s == 0.5).all()
    assert R.events_ref(s, 0.5, 2) == [0, 2, 4, 6, 8]
    assert R.events_ref(s, np.nextafter(0.5, 1.0), 2) == []


def test_reference_nan_silences_the_windows_that_hold_it():
    p = [0.9] * 12
    p[5] = math.nan
    s = R.smooth_ref(p, 3)
    assert np.flatnonzero(np.isnan(s)).tolist() == [5, 6, 7]
    assert R.events_ref(s, 0.5, 1) == [0, 1, 2, 3, 4, 8, 9, 10, 11]
    assert R.peak_ref(s) == (pytest.approx(0.9), 0)
    assert R.peak_ref(np.array([math.nan, math.nan]))[1] == -1 and math.isnan(R.peak_ref(np.array([math.nan]))[0])
    assert R.peak_ref(np.zeros(0))[1] == -1
    assert R.peak_ref(np.array([0.2, 0.7, 0.7, 0.1])) == (0.7, 1)          # the first of equal peaks


def test_reference_history_does_not_cross_recordings():
    a, b = [0.9, 0.9, 0.9], [0.0, 0.0, 0.9]
    sb = R.smooth_ref(b, 3)
    assert sb.tolist() == [0.0, 0.0, pytest.approx(0.3)]                   # not (0.9 + 0.9 + 0) / 3
    sweep = R.sweep_ref([R.smooth_ref(a, 3), sb], [0.5], 2)
    assert sweep["counts"] == [[2], [0]] and sweep["first_window"] == [[0], [-1]]
    tab = R.table_ref([R.smooth_ref(a, 3), sb], 0.25, 2, 4000, 16000, 16000)
    assert tab["counts"] == [2, 1] and tab["clip"] == [0, 0, 1] and tab["window"] == [0, 2, 2]
    assert tab["time"] == [1.0, 1.5, 1.5]


def test_the_stated_summation_order_is_numpys():
    rng = np.random.default_rng(5)
    for n in range(1, 33):
        for trial in range(50):
            a = rng.random(n).astype(np.float32).astype(np.float64) * (10.0 ** rng.integers(-3, 4) if trial % 2 else 1.0)
            assert R.ordered_sum(a) / n == float(np.mean(deque_of(a))), (n, trial)
            assert R.ordered_sum(a) == float(np.add.reduce(a)), (n, trial)


def deque_of(a):
    from collections import deque
    return deque([float(v) for v in a], maxlen=32)


def test_report_ref_on_a_known_case():
    smoothed = [np.array([0.9, 0.9, 0.9]), np.zeros(0), np.array([0.1, 0.6])]
    rep = R.report_ref([24000, 100, 20000], [1, 0, 0], smoothed, [0.5, 0.95], 2, 16000)
    assert rep["cough"] == dict(recordings=1, minutes=24000 / 16000 / 60.0, events=[2, 0], events_per_minute=[2 / 0.025, 0.0],
                                recordings_with_event=[1, 0], share_with_event=[1.0, 0.0])
    assert rep["non_cough"]["recordings"] == 2 and rep["non_cough"]["events"] == [1, 0]
    assert rep["non_cough"]["share_with_event"] == [0.5, 0.0]
    empty = R.report_ref([24000], [1], smoothed[:1], [0.5], 2, 16000)["non_cough"]
    assert empty["recordings"] == 0 and empty["events_per_minute"] == [None] and empty["share_with_event"] == [None]
