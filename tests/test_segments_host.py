"""Corpus curation without a GPU: the fourth library's symbols and argument checks, the build's staleness rule, the
Python front's parameter checks, and the numpy restatement (tests/segments_ref.py) on hand-built clips whose answers are
known."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import cough_detector_amd as cda
from cough_detector_amd import _lib
from cough_detector_amd import build as cbuild
from cough_detector_amd import segments as cseg
import segments_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cough_amd_segments.h")
SHIPPED = dict(use_pcen=False, use_pre_emphasis=False, use_delta_delta=False, use_spectral_contrast=False)
SEG, SR = 16000, 16000


# ------------------------------------------------------------------------------------------------ the library
def test_segments_library_exports_exactly_its_header():
    text = open(HEADER).read()
    declared = set(re.findall(r"\b(cough_[a-z_0-9]+)\s*\(", text))
    assert declared == set(_lib.SEGMENTS_SYMBOLS), declared ^ set(_lib.SEGMENTS_SYMBOLS)
    assert len(_lib.SEGMENTS_SYMBOLS) == len(set(_lib.SEGMENTS_SYMBOLS))
    lib = _lib.load_segments()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.cough_segments_abi_version() == 1
    assert "#define COUGH_SEGMENTS_ABI_VERSION 1" in text
    assert re.search(rf"#define COUGH_MAX_SEGMENTS {_lib.MAX_SEGMENTS}\b", text) and _lib.MAX_SEGMENTS == 16
    assert re.search(rf"#define COUGH_MAX_FRAME_LENGTH {_lib.MAX_FRAME_LENGTH}\b", text)
    nm = shutil.which("nm") or os.path.join(os.path.dirname(os.path.realpath(cbuild._hipcc())), "..", "lib", "llvm", "bin", "llvm-nm")
    out = subprocess.run([nm, "-D", "--defined-only", _lib.SEGMENTS_LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert exported == declared, sorted(exported ^ declared)


def test_the_other_three_libraries_are_untouched():
    others = set(_lib.SYMBOLS) | set(_lib.LOOP_SYMBOLS) | set(_lib.DATA_SYMBOLS)
    assert not set(_lib.SEGMENTS_SYMBOLS) & others
    assert len(_lib.SYMBOLS) == 53 and _lib.load().cough_amd_abi_version() == 5
    assert len(_lib.LOOP_SYMBOLS) == 3 and _lib.load_loop().cough_loop_abi_version() == 1
    assert len(_lib.DATA_SYMBOLS) == 5 and _lib.load_data().cough_data_abi_version() == 1
    for header in ("cough_amd.h", "cough_amd_loop.h", "cough_amd_data.h"):
        text = open(os.path.join(ROOT, "include", header)).read()
        for s in _lib.SEGMENTS_SYMBOLS:
            assert s not in text, (header, s)


FAKE = 1 << 20


def _err():
    return _lib.load_segments().cough_segments_last_error()


def test_frame_energy_refuses_bad_arguments_without_a_gpu():
    lib = _lib.load_segments()

    def call(bank=FAKE, offs=FAKE, lens=FAKE, foffs=FAKE, n=3, tiles=FAKE, n_tiles=5, frame=400, hop=160, out=FAKE):
        return lib.cough_frame_energy(bank, offs, lens, foffs, n, tiles, n_tiles, frame, hop, out, None)

    E = _lib.EINVAL
    for kw in ("bank", "offs", "lens", "foffs", "tiles", "out"):
        assert call(**{kw: None}) == E and b"NULL" in _err() and b"cough_frame_energy" in _err(), kw
    assert call(n=-1) == E and b"n_clips" in _err() and b"cough_frame_energy" in _err()
    assert call(n_tiles=-1) == E and b"n_tiles" in _err()
    assert call(n=-2 ** 31) == E
    for v in (0, -1):
        assert call(frame=v) == E and b"frame_length" in _err() and b"cough_frame_energy" in _err(), v
        assert call(hop=v) == E and b"hop_length" in _err() and b"cough_frame_energy" in _err(), v
    assert call(frame=_lib.MAX_FRAME_LENGTH + 1) == _lib.EUNSUPPORTED and b"frame_length" in _err()
    for kw in ("bank", "lens", "tiles"):
        assert call(**{kw: FAKE + 2}) == E and b"4-byte" in _err() and b"cough_frame_energy" in _err(), kw
    for kw in ("offs", "foffs", "out"):
        assert call(**{kw: FAKE + 4}) == E and b"8-byte" in _err(), kw
    assert call(n=0) == _lib.OK and call(n_tiles=0) == _lib.OK            # nothing to do: no launch
    with pytest.raises(ValueError, match="cough_frame_energy: .*hop_length"):
        _lib.check_segments(call(hop=0), "cough_frame_energy")
    assert b"hop_length" not in _lib.load_data().cough_data_last_error()   # the libraries keep their messages apart
    # the frames of a tile: positive for every pair the call accepts, 0 otherwise
    for pair in ((400, 160), (512, 512), (256, 64), (7, 3), (400, 1000), (1, 1), (4096, 1), (4096, 4096), (4095, 3)):
        assert lib.cough_frame_energy_tile_frames(*pair) >= 1, pair
    for pair in ((0, 160), (400, 0), (-1, -1), (4097, 160)):
        assert lib.cough_frame_energy_tile_frames(*pair) == 0, pair


def test_pick_segments_refuses_bad_arguments_without_a_gpu():
    lib = _lib.load_segments()

    def call(e=FAKE, foffs=FAKE, lens=FAKE, n=3, frame=400, hop=160, seg=16000, min_frames=10, max_segments=8, ratio=1e-3,
             floor=1e-6, counts=FAKE, starts=FAKE, seg_lens=FAKE, peak=FAKE):
        return lib.cough_pick_segments(e, foffs, lens, n, frame, hop, seg, min_frames, max_segments, ratio, floor, counts,
                                       starts, seg_lens, peak, None)

    E = _lib.EINVAL
    for kw in ("e", "foffs", "lens", "counts", "starts", "seg_lens", "peak"):
        assert call(**{kw: None}) == E and b"NULL" in _err() and b"cough_pick_segments" in _err(), kw
    assert call(n=-1) == E and b"n_clips" in _err() and b"cough_pick_segments" in _err()
    for v in (0, -3):
        assert call(frame=v) == E and b"frame_length" in _err() and b"cough_pick_segments" in _err(), v
        assert call(hop=v) == E and b"hop_length" in _err() and b"cough_pick_segments" in _err(), v
        assert call(seg=v) == E and b"seg_len" in _err(), v
        assert call(min_frames=v) == E and b"min_frames" in _err(), v
    for v in (0, -1, 17, 1 << 20):
        assert call(max_segments=v) == E and b"max_segments" in _err() and b"cough_pick_segments" in _err(), v
    for v in (1, 16):
        assert call(max_segments=v, n=0) == _lib.OK, v
    for kw in ("ratio", "floor"):
        for v in (-1.0, math.inf, math.nan):
            assert call(**{kw: v}) == E and b"ratio and floor" in _err(), (kw, v)
    for kw in ("lens", "counts", "starts", "seg_lens", "peak"):
        assert call(**{kw: FAKE + 2}) == E and b"4-byte" in _err() and b"cough_pick_segments" in _err(), kw
    for kw in ("e", "foffs"):
        assert call(**{kw: FAKE + 4}) == E and b"8-byte" in _err(), kw
    assert call(n=0) == _lib.OK


def test_copy_segments_refuses_bad_arguments_without_a_gpu():
    lib = _lib.load_segments()

    def call(src=FAKE, soffs=FAKE, starts=FAKE, lens=FAKE, doffs=FAKE, n=4, max_len=16000, dst=FAKE):
        return lib.cough_copy_segments(src, soffs, starts, lens, doffs, n, max_len, dst, None)

    E = _lib.EINVAL
    for kw in ("src", "soffs", "starts", "lens", "doffs", "dst"):
        assert call(**{kw: None}) == E and b"NULL" in _err() and b"cough_copy_segments" in _err(), kw
    assert call(n=-1) == E and b"n_rows" in _err() and b"cough_copy_segments" in _err()
    for v in (0, -2):
        assert call(max_len=v) == E and b"max_len" in _err(), v
    for kw in ("src", "starts", "lens", "dst"):
        assert call(**{kw: FAKE + 1}) == E and b"4-byte" in _err() and b"cough_copy_segments" in _err(), kw
    for kw in ("soffs", "doffs"):
        assert call(**{kw: FAKE + 4}) == E and b"8-byte" in _err(), kw
    assert call(n=0) == _lib.OK


# ------------------------------------------------------------------------------------------------ the Python front
def _bank(clips=None, labels=None):
    clips = clips if clips is not None else [torch.zeros(800), torch.ones(20000)]
    return cda.DeviceClipBank(clips, labels if labels is not None else [0] * len(clips), device="cpu")


def test_the_package_exports_the_finder():
    for name in ("SegmentTable", "frame_energy", "find_segments", "extract_segments"):
        assert name in cda.__all__ and getattr(cda, name) is getattr(cseg, name), name


def test_bad_parameters_raise_before_any_launch():
    bank, pre = _bank(), cda.AudioPreprocessor(**SHIPPED)
    # a CPU bank would raise RuntimeError at the launch: a ValueError shows the check came first
    for kw in (dict(frame_length=0), dict(frame_length=-5), dict(hop_length=0), dict(frame_length=400.0),
               dict(frame_length=_lib.MAX_FRAME_LENGTH + 1), dict(hop_length=True)):
        with pytest.raises(ValueError, match="frame_length|hop_length"):
            cda.frame_energy(bank, **kw)
        with pytest.raises(ValueError, match="frame_length|hop_length"):
            cda.find_segments(bank, pre, **kw)
    for v in (0, -1, 17, 8.0):
        with pytest.raises(ValueError, match="max_segments"):
            cda.find_segments(bank, pre, max_segments=v)
        with pytest.raises(ValueError, match="max_segments"):
            cda.extract_segments(bank, pre, max_segments=v)
    for kw in (dict(threshold_db=math.nan), dict(floor_db=math.inf), dict(min_duration=-0.1), dict(min_duration=math.nan),
               dict(threshold_db="loud"), dict(threshold_db=4000.0)):
        with pytest.raises(ValueError, match="|".join(kw)):
            cda.find_segments(bank, pre, **kw)
    with pytest.raises(TypeError):
        cda.find_segments(bank, pre, no_such_parameter=1)


def test_a_bank_off_the_gpu_cannot_launch():
    bank, pre = _bank(), cda.AudioPreprocessor(**SHIPPED)
    for call in (lambda: cda.frame_energy(bank), lambda: cda.find_segments(bank, pre), lambda: cda.extract_segments(bank, pre)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_frame_counts_follow_the_rule():
    lengths = np.array([1, 399, 400, 401, 559, 560, 561, 16000, 16001, 40001])
    assert cseg.frame_counts(lengths, 400, 160).tolist() == [1, 1, 1, 1, 1, 2, 2, 98, 98, 248]
    assert cseg.frame_counts(lengths, 400, 1000).tolist() == [1, 1, 1, 1, 1, 1, 1, 16, 16, 40]
    assert cseg.frame_counts(lengths, 7, 3).tolist() == [R.n_frames(int(n), 7, 3) for n in lengths]
    assert cseg.frame_counts(lengths, 400, 160).dtype == np.int64


def test_the_parameters_reach_the_kernel_as_the_specification_states():
    pre = cda.AudioPreprocessor(**SHIPPED)
    frame, hop, seg, min_frames, max_segments, ratio, floor = cseg._params("t", pre)
    assert (frame, hop, seg, min_frames, max_segments) == (400, 160, pre.segment_samples, 10, 8)
    assert ratio == 10.0 ** (-30.0 / 10.0) and floor == 10.0 ** (-60.0 / 10.0)
    assert cseg._params("t", pre, min_duration=0.0)[3] == 1 and cseg._params("t", pre, min_duration=0.101)[3] == 11
    assert cseg._params("t", pre, hop_length=1000, min_duration=0.01)[3] == 1


# ------------------------------------------------------------------------------------------------ the restatement
def test_reference_energy_on_known_signals():
    x = np.arange(1, 1001, dtype=np.float32)
    e = R.frame_energy_ref(x, 400, 160)
    assert e.size == 4 and e.dtype == np.float64
    for f in range(4):
        lo = 160 * f
        want = sum(float(v) ** 2 for v in range(lo + 1, lo + 401)) / 400.0
        assert e[f] == pytest.approx(want, rel=1e-15), f
    short = R.frame_energy_ref(np.full(399, 2.0, dtype=np.float32), 400, 160)
    assert short.tolist() == [4.0]                                         # one frame: the mean over the clip's 399 samples
    gaps = R.frame_energy_ref(np.ones(3000, dtype=np.float32), 400, 1000)  # hop > frame: gaps between frames
    assert gaps.tolist() == [1.0, 1.0, 1.0]
    assert R.frame_energy_ref(np.ones(1, dtype=np.float32), 7, 3).tolist() == [1.0]


@pytest.fixture(scope="module")
def cases():
    return R.case_clips(seed=0, seg_len=SEG)


def _peak_sample(x, lo, hi):
    e = R.frame_energy_ref(x)
    f0, f1 = max((lo - 400) // 160 + 1, 0), min(hi // 160, e.size - 1)
    return (f0 + int(np.argmax(e[f0:f1 + 1]))) * 160 + 200


def test_reference_on_a_burst_in_the_middle(cases):
    x = cases["middle"]
    r = R.segments_ref(x, SEG, SR)
    c = _peak_sample(x, 38000, 42000)
    assert 39000 < c < 41000                                               # the Hann envelope peaks at the burst's centre
    assert r["start"] == [c - SEG // 2] and r["length"] == [SEG]
    assert r["peak_db"][0] == np.float32(10 * np.log10(r["energy"][(c - 200) // 160]))
    assert -14.0 < r["peak_db"][0] < -9.0 and r["margin"] > 1e-9           # 0.3^2 = -10.5 dB under the envelope's top


def test_reference_clamps_at_both_ends(cases):
    x = cases["start_and_end"]
    r = R.segments_ref(x, SEG, SR)
    assert r["start"] == [0, x.size - SEG] and r["length"] == [SEG, SEG] and r["margin"] > 1e-9


def test_reference_drops_a_burst_that_overlaps_the_last_segment(cases):
    x = cases["two_close"]
    r = R.segments_ref(x, SEG, SR)
    first = _peak_sample(x, 28000, 32000)
    assert r["start"] == [first - SEG // 2] and r["length"] == [SEG]       # the second, 8000 samples on, starts inside it
    apart = R.recording(np.random.default_rng(4), 80000, [(20000, 4000), (50000, 4000)])
    assert len(R.segments_ref(apart, SEG, SR)["start"]) == 2


def test_reference_stops_at_max_segments(cases):
    x = cases["many"]
    r = R.segments_ref(x, SEG, SR)
    assert len(r["start"]) == 8 and r["length"] == [SEG] * 8
    for k, s in enumerate(r["start"]):
        assert abs(s + SEG // 2 - (8000 + 17000 * k)) < 1000 or (k == 0 and s <= 40), (k, s)
    assert all(b >= a + SEG for a, b in zip(r["start"], r["start"][1:]))
    assert len(R.segments_ref(x, SEG, SR, max_segments=16)["start"]) == 9
    assert R.segments_ref(x, SEG, SR, max_segments=3)["start"] == r["start"][:3]


def test_reference_rejects_a_click(cases):
    x = cases["click"]
    r = R.segments_ref(x, SEG, SR)
    e = r["energy"]
    assert int((e >= e.max() * 1e-3).sum()) == 3                           # frames 123..125 hold the 8-sample click
    assert r["start"] == [] and r["margin"] > 1e-9
    assert len(R.segments_ref(x, SEG, SR, min_duration=0.03)["start"]) == 1      # 3 frames are enough then


def test_reference_returns_a_short_clip_whole(cases):
    x = cases["short"]
    r = R.segments_ref(x, SEG, SR)
    assert r["start"] == [0] and r["length"] == [x.size] and x.size < SEG
    tiny = np.full(100, 0.5, dtype=np.float32)                             # shorter than a frame: one frame, the clip
    r = R.segments_ref(tiny, SEG, SR, min_duration=0.0)
    assert r["start"] == [0] and r["length"] == [100] and r["peak_db"] == [np.float32(10 * np.log10(0.25))]
    assert R.segments_ref(tiny, SEG, SR)["start"] == []                    # one frame is no 10-frame run


def test_reference_yields_nothing_for_silence_and_non_finite_samples(cases):
    r = R.segments_ref(cases["silent"], SEG, SR)
    assert r["start"] == [] and r["margin"] == math.inf
    faint = (1e-4 * np.random.default_rng(1).standard_normal(30000)).astype(np.float32)
    assert R.segments_ref(faint, SEG, SR)["start"] == []                   # -80 dB: under the floor
    assert len(R.segments_ref(faint, SEG, SR, floor_db=-90.0)["start"]) == 1
    for bad in (np.nan, np.inf, -np.inf):
        x = cases["middle"].copy()
        x[12345] = bad
        assert R.segments_ref(x, SEG, SR)["start"] == [], bad
    x = cases["middle"].copy()
    x[-1] = np.nan                                                         # past the last full frame: takes no part
    assert R.segments_ref(x, SEG, SR)["start"] == R.segments_ref(cases["middle"], SEG, SR)["start"]


def test_table_ref_orders_by_clip_then_time(cases):
    names = ["silent", "start_and_end", "click", "middle"]
    tab = R.table_ref([cases[k] for k in names], SEG, SR)
    assert tab["counts"] == [0, 2, 0, 1] and tab["clip"] == [1, 1, 3]
    assert tab["start"][:2] == [0, 48000] and tab["margin"] > 1e-9
