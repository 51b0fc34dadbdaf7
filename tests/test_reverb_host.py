"""Room reverberation, without a GPU: the float32 emulation of the kernel's algorithm (tests/reverb_ref.py) against the
float64 reference on the GPU test's own cases, the planted defects against the GPU test's own checks, the synthetic and
the measured banks, the chain's host plans and draws, and the library's entries in the open tables (``_lib.OPEN`` /
``build.OPEN_UNITS``: this test asks whether "reverb" is in them, never what else is)."""
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import cough_detector_amd as cda
from cough_detector_amd import _lib
from cough_detector_amd import build as cbuild
from cough_detector_amd import chain as cchain
from cough_detector_amd import reverb as crev
from cough_detector_amd.preprocessing import load_wave
import reverb_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "reverb"


def _dense(y, width):
    return np.concatenate([y, np.zeros(width - y.size, dtype=np.float32)])


# ------------------------------------------------------------------------------------------------ emulation and defects
def test_the_cases_cover_what_the_issue_lists():
    bank, rows, width, exp = R.expected()
    assert [h.size for h in bank] == [1, 2, 3, 8192, 8193, 1, 2, 8192, 8193]
    assert sorted({r["x"].size for r in rows[:28]}) == list(R.LENGTHS)
    live = [(r, e) for r, e in zip(rows, exp) if r["rir"] >= 0 and r["out_len"] and not all(e["silent"])]
    assert {r["rir"] for r, _ in live} == set(range(len(bank)))                 # every response convolves something
    assert {len(e["bad"]) for _, e in live} >= {1, 2, 3, 4}                        # one to four spans
    assert sum(any(e["bad"]) for _, e in live) == 4 and any(sum(e["bad"]) == 2 for _, e in live)
    assert any(r["out_len"] == 0 for r in rows) and any(0 < r["out_len"] < r["x"].size for r in rows)
    assert any(abs(r["shift"]) >= r["x"].size > 0 for r in rows) and width == 48000 + 8192


def test_the_clean_emulation_passes_every_check():
    bank, rows, width, exp = R.expected()
    worst = 0.0
    for row, e in zip(rows, exp):
        R.check_row(_dense(e["emu"], width), row, e, width)
        if row["rir"] >= 0 and row["out_len"]:
            ok = np.isfinite(e["emu"])
            worst = max(worst, float((np.abs(e["emu"][ok] - e["ref"][ok]) / np.maximum(e["bound"][ok], 1e-300)).max()))
    assert 0.0 < worst < 1e-2                             # the worst-case bound is loose: hence the RMS check


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_every_planted_defect_is_caught(defect):
    bank, rows, width, exp = R.expected()
    caught = []
    for r in (5, 7, 9, 13, 19, 24, 27):                   # rows that convolve something, one to four spans
        row, e = rows[r], exp[r]
        y = R.emulate(row["x"], row["shift"], bank[row["rir"]], row["out_len"], defect=defect)
        try:
            R.check_row(_dense(y, width), row, e, width)
        except AssertionError:
            caught.append(r)
    assert len(caught) >= 5, (defect, caught)


def test_nan_by_propagation_is_told_from_the_load_time_rule():
    """A kernel that lets the non-finite sample run through the transform also ends in NaNs; the checks tell it apart:
    the rows' NaNs are negative with a payload, which arithmetic hands on, and the rule writes 0x7FC00000 everywhere."""
    bank, rows, width, exp = R.expected()
    seen = 0
    for r, (row, e) in enumerate(zip(rows, exp)):
        if row["twin"] is None:
            continue
        assert (e["emu"][np.isnan(e["emu"])].view(np.uint32) == R.QUIET_NAN).all()
        if not np.isnan(row["x"]).any():
            continue                                       # an Inf: Inf - Inf gives the platform's default NaN
        y = R.emulate(row["x"], row["shift"], bank[row["rir"]], row["out_len"], defect=R.NO_LOAD_RULE)
        with pytest.raises(AssertionError, match="load-time rule|not all NaN"):
            R.check_row(_dense(y, width), row, e, width)
        seen += 1
    assert seen == 2


def test_an_impulse_response_delays_the_row():
    rng = np.random.default_rng(3)
    x = rng.standard_normal(20000).astype(np.float32)
    for at in (0, 1, 8191, 8192):
        h = np.zeros(at + 1, dtype=np.float32)
        h[at] = 1.0
        ref = R.reverb_ref(x, 0, h, 20000 + at)
        assert not ref[:at].any() and ref[at:].tolist() == x.astype(np.float64).tolist()
    assert R.reverb_ref(x, 7, None, 100).tolist() == [0.0] * 7 + x[:93].astype(np.float64).tolist()


def test_the_span_rule():
    x = np.ones(48000, dtype=np.float32)
    for at, want in ((16384, [False, True, False]), (32767, [False, True, True]), (8192, [True, True, False]),
                     (0, [True, False, False]), (8191, [True, False, False])):
        y = x.copy()
        y[at] = np.inf
        assert R.bad_spans(y, 0, 48000) == want, at
    y = x.copy()
    y[100] = np.nan
    assert R.bad_spans(y, -101, 48000) == [False] * 3     # shifted out of the row
    assert R.bad_spans(y, 16384, 16385) == [False, True]


# ------------------------------------------------------------------------------------------------ the synthetic bank
def test_synth_rirs_in_float64():
    sr = 16000
    taps, table = crev.synth_rir_taps(12, sr, seed=5)
    gap = int(0.002 * sr)
    assert table.shape == (12, 3) and len(taps) == 12
    for h, (rt60, drr_db, L) in zip(taps, table):
        assert 0.15 <= rt60 <= 0.5 and 0.0 <= drr_db <= 15.0
        assert h.dtype == np.float64 and h.size == L == min(8193, int(np.ceil(rt60 * sr)))
        assert abs(float((h * h).sum()) - 1.0) <= 1e-12
        assert h[0] > 0 and not h[1:gap].any() and h[gap:].all()
        assert abs(10.0 * np.log10(h[0] ** 2 / float((h[gap:] ** 2).sum())) - drr_db) <= 1e-9
        k = np.arange(gap, int(L), dtype=np.float64)                        # 60 dB down after rt60 seconds
        env = np.exp(-3.0 * np.log(10.0) * k / (rt60 * sr))
        assert np.abs(h[gap:] / env).max() / (h[gap:] / env).std() < 6.0        # what is left is stationary noise
    assert (table[:, 2] == 8193).any() or table[:, 0].max() * sr < 8193
    long_taps, long_table = crev.synth_rir_taps(3, sr, rt60_range=(0.6, 0.9), seed=1)
    assert [h.size for h in long_taps] == [8193] * 3 == long_table[:, 2].astype(int).tolist()


def test_synth_rirs_is_seeded_and_rounds_once():
    a, ta = cda.synth_rirs(6, seed=11)
    b, tb = cda.synth_rirs(6, seed=11)
    c, _ = cda.synth_rirs(6, seed=12)
    assert isinstance(a, cda.RirBank) and len(a) == 6 and a.packed.tobytes() == b.packed.tobytes() and ta.tobytes() == tb.tobytes()
    assert a.packed.tobytes() != c.packed.tobytes()
    taps, _ = crev.synth_rir_taps(6, seed=11)
    for h32, h64 in zip(a.taps, taps):
        assert h32.dtype == np.float32 and h32.tobytes() == h64.astype(np.float32).tobytes()
    assert a.lengths.tolist() == [h.size for h in taps] and a.offsets.tolist() == np.cumsum([0] + [h.size for h in taps])[:-1].tolist()
    assert a.max_taps == max(h.size for h in taps)
    # the documented order of the draws
    rng = np.random.Generator(np.random.Philox(11))
    rt60, drr = rng.uniform(0.15, 0.5), rng.uniform(0.0, 15.0)
    assert (rt60, drr) == (ta[0, 0], ta[0, 1])
    with pytest.raises(ValueError):
        cda.synth_rirs(0)
    with pytest.raises(ValueError):
        cda.synth_rirs(2, rt60_range=(0.0, 0.1))


def test_rir_bank_refuses_what_the_kernel_cannot_take():
    with pytest.raises(ValueError, match="8193"):
        cda.RirBank([np.ones(8194, dtype=np.float32)])
    with pytest.raises(ValueError):
        cda.RirBank([])
    with pytest.raises(ValueError):
        cda.RirBank([np.zeros((2, 3))])
    with pytest.raises(ValueError):
        cda.RirBank([np.array([1.0, np.nan])])
    bank = cda.RirBank([np.ones(8193), torch.ones(2)])
    assert len(bank) == 2 and bank.packed.dtype == np.float32 and bank.lengths.dtype == np.int32 and bank.offsets.dtype == np.int64


class _HostPreprocessor:
    """The loading path of AudioPreprocessor for files that are already at the rate: load_audio, resample, to_mono."""
    sample_rate = 16000
    load_audio = staticmethod(load_wave)

    def resample(self, waveform, sr):
        assert sr == self.sample_rate
        return waveform

    @staticmethod
    def to_mono(waveform):
        return waveform.mean(dim=0, keepdim=True) if waveform.shape[0] > 1 else waveform


def test_from_directory_trims_cuts_and_normalises(tmp_path):
    from scipy.io import wavfile
    rng = np.random.default_rng(9)
    lead = np.concatenate([0.01 * rng.standard_normal(500), [-0.9], 0.2 * rng.standard_normal(299)]).astype(np.float32)
    long = np.concatenate([[0.5], 0.1 * rng.standard_normal(11999)]).astype(np.float32)
    stereo = np.stack([np.r_[0.0, 0.8, 0.1, 0.05], np.r_[0.0, 0.4, 0.1, 0.05]], axis=1).astype(np.float32)
    wavfile.write(tmp_path / "b_lead.wav", 16000, lead)
    wavfile.write(tmp_path / "a_long.wav", 16000, long)
    wavfile.write(tmp_path / "c_stereo.wav", 16000, stereo)
    (tmp_path / "notes.txt").write_text("not a response")
    bank = cda.RirBank.from_directory(tmp_path, _HostPreprocessor())
    assert bank.lengths.tolist() == [8193, 300, 3]                              # sorted by name; cut; trimmed
    for h in bank.taps:
        assert abs(float((h.astype(np.float64) ** 2).sum()) - 1.0) <= 1e-6
        assert abs(h[0]) == np.abs(h).max()
    assert bank.taps[1][0] < 0                                                  # the largest |h| keeps its sign
    want = crev.RirBank.conditioned(lead).astype(np.float32)
    assert bank.taps[1].tobytes() == want.tobytes()
    assert np.allclose(bank.taps[2], np.array([0.6, 0.1, 0.05]) / np.sqrt(0.36 + 0.01 + 0.0025), atol=1e-7)
    (tmp_path / "empty").mkdir()
    with pytest.raises(ValueError, match="no WAVE"):
        cda.RirBank.from_directory(tmp_path / "empty", _HostPreprocessor())
    with pytest.raises(ValueError):
        crev.RirBank.conditioned(np.zeros(10))


# ------------------------------------------------------------------------------------------------ plans and draws
def test_plan_array_refuses_before_any_launch():
    arr = crev.plan_array([(3, 0, 10), (-2, -1, 0), (2**40, 4, 7)], n_rirs=5, width=10)
    assert arr.dtype == np.int32 and arr.tolist() == [[3, 0, 10, 0], [-2, -1, 0, 0], [2**31 - 1, 4, 7, 0]]
    for bad in ((0, 5, 1), (0, -2, 1), (0, 0, -1), (0, 0, 11)):
        with pytest.raises(ValueError):
            crev.plan_array([(0, 0, 1), bad], n_rirs=5, width=10)
        with pytest.raises(ValueError):
            crev.check_plans(np.array([[0, 0, 1, 0], list(bad) + [0]], dtype=np.int32), 5, 10)
    assert crev.check_plans(arr[:2], 5, 10).tolist() == arr[:2].tolist()
    assert crev.PLAN_WORDS * 4 == 16 and crev.MAX_TAPS == R.MAX_TAPS and crev.BOUND_K == R.BOUND_K


def test_the_reverb_keyword_is_inert_when_nothing_fires():
    """``host_plans`` with the keyword left out, with ``reverb=None`` and with no coin fired: one and the same result.
    That this result is the parent's is pinned by the untouched tests/test_chain_host.py, not here."""
    shifts, lengths = [5, -3, 0, 9], [1000, 2000, 1500, 800]
    pairs, steps = [(15000, 16000), None, None, (17000, 16000)], [2, None, 0, -1]
    for p, s in ((None, None), (pairs, None), (None, steps), (pairs, steps), ([None] * 4, [None] * 4)):
        a = cchain.host_plans(shifts, p, s, lengths, 16000, 2000)
        b = cchain.host_plans(shifts, p, s, lengths, 16000, 2000, False, reverb=None)
        c = cchain.host_plans(shifts, p, s, lengths, 16000, 2000, reverb=[None] * 4)       # no coin fired
        for other in (b, c):
            assert list(a.arrays) == list(other.arrays) and "reverb" not in other.arrays
            assert all(a.arrays[k].tobytes() == other.arrays[k].tobytes() for k in a.arrays)
            assert a[1:] == other[1:]
    assert cchain.HostPlans._fields == ("arrays", "new_lengths", "width", "stretch_width")


def test_the_first_launch_that_reads_the_rows_carries_the_shift():
    shifts, lengths, rirs = [5, -3, 0, 9], [1000, 2000, 1500, 800], [2, None, 0, None]
    pairs, steps = [(15000, 16000), None, None, (17000, 16000)], [2, None, 0, -1]
    alone = cchain.host_plans(shifts, None, None, lengths, 16000, 2000, reverb=rirs)
    assert list(alone.arrays) == ["reverb"] and alone.width == 2000 and alone.new_lengths == lengths
    assert alone.arrays["reverb"].tolist() == [[5, 2, 1000, 0], [-3, -1, 2000, 0], [0, 0, 1500, 0], [9, -1, 800, 0]]
    for p, s, carrier in ((pairs, None, "warp"), (None, steps, "stretch"), (pairs, steps, "warp"), ([None] * 4, steps, "stretch"),
                          ([None] * 4, [None, None, 0, None], "reverb")):
        plans = cchain.host_plans(shifts, p, s, lengths, 16000, 2000, reverb=rirs)
        assert list(plans.arrays)[-1] == "reverb" and list(plans.arrays)[0] == carrier
        rev = plans.arrays["reverb"]
        assert rev[:, 0].tolist() == (shifts if carrier == "reverb" else [0] * 4)
        assert rev[:, 1].tolist() == [2, -1, 0, -1] and rev[:, 2].tolist() == plans.new_lengths      # out_len = n'
        without = cchain.host_plans(shifts, p, s, lengths, 16000, 2000)
        assert all(plans.arrays[k].tobytes() == without.arrays[k].tobytes() for k in without.arrays)
        assert plans[1:] == without[1:]


def _stream(aug, lengths):
    random.seed(77)
    items = [aug.draw_item_reverb(n) for n in lengths]
    return items, random.random()


def test_the_host_draws_leave_the_stream_alone_without_a_bank():
    lengths = [16000, 9000, 12000, 700, 16000, 4000]
    bank, _ = cda.synth_rirs(5, seed=2)
    for kw in (dict(), dict(speed=True), dict(pitch=True), dict(speed=True, pitch=True)):
        plain = cda.AudioAugmentor(p_augment=0.6, **kw)
        assert plain.reverb is None
        random.seed(77)
        want = [plain.draw_item_pitched(n) for n in lengths]
        after = random.random()
        items, after_reverb_none = _stream(plain, lengths)
        assert after == after_reverb_none and all(it[4] is None for it in items)
        for a, b in zip(want, items):
            assert bytes(a[0]) == bytes(b[0]) and a[1:] == b[1:4]
        # with a bank: coin and randrange sit behind the pitch step's draws and before the gain's
        wet = cda.AudioAugmentor(p_augment=0.6, reverb=bank, **kw)
        items, _ = _stream(wet, lengths[:1])
        random.seed(77)
        c = wet._blank()
        c.shift = wet._draw_shift(lengths[0])
        pair = wet._draw_speed() if wet.speed else None
        steps = wet._draw_pitch() if wet.pitch else None
        rir = R.host_reverb_draw(random, 0.6, len(bank))
        gain = wet._draw_gain()
        assert items[0][1] == pair and items[0][3] == steps and items[0][4] == rir
        assert items[0][0].shift == c.shift and items[0][0].gain == np.float32(gain if gain is not None else 1.0)
    random.seed(5)
    fired = [cda.AudioAugmentor(p_augment=0.5, reverb=bank).draw_item_reverb(100)[4] for _ in range(64)]
    assert 8 < sum(f is not None for f in fired) < 56 and {f for f in fired if f is not None} == set(range(5))
    with pytest.raises(TypeError):
        cda.AudioAugmentor(reverb=[np.ones(3)])
    aug, _ = cda.create_augmentation_pipeline(reverb=bank)
    assert aug.reverb is bank and cda.create_augmentation_pipeline()[0].reverb is None


def test_the_device_draw_restated():
    plans = R.draw_reverb_ref(7, [16000, 0, 5, 2**31 - 1, -4] + [100] * 200, 0.5, 9)
    assert plans.dtype == np.int32 and plans[:5, 2].tolist() == [16000, 0, 5, 2**30, 0]
    assert plans[1, 1] == plans[4, 1] == -1 and not plans[:, 0].any() and not plans[:, 3].any()
    fired = plans[5:, 1] >= 0
    assert 60 < fired.sum() < 140 and set(plans[5:, 1][fired].tolist()) == set(range(9))
    assert (R.draw_reverb_ref(7, [100] * 50, 0.5, 0)[:, 1] == -1).all()
    assert (R.draw_reverb_ref(7, [100] * 50, 1.0, 3)[:, 1] >= 0).all() and (R.draw_reverb_ref(7, [100] * 50, 0.0, 3)[:, 1] == -1).all()


def test_cache_features_refuses_a_reverb_augmentor():
    bank, _ = cda.synth_rirs(2, seed=1)
    clips = cda.DeviceClipBank([torch.zeros(100), torch.ones(50)], [0, 1], device="cpu")
    with pytest.raises(ValueError, match="cache_features"):
        cda.DeviceDataLoader(clips, None, audio_augmentor=cda.AudioAugmentor(reverb=bank), cache_features=True)
    cda.DeviceDataLoader(clips, None, audio_augmentor=cda.AudioAugmentor(reverb=bank), cache_features=True, is_training=False)


# ------------------------------------------------------------------------------------------------ the library
def _header():
    with open(os.path.join(ROOT, "include", f"cough_amd_{NAME}.h")) as f:
        return f.read()


def _declared():
    body = _header().split("#pragma GCC visibility push(default)")[1].split("#pragma GCC visibility pop")[0]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"\b(cough_\w+)\s*\(", body)


def test_the_library_is_in_the_open_tables():
    assert NAME in _lib.OPEN and NAME in cbuild.OPEN_UNITS and NAME in cbuild.OPEN_LIBS
    assert list(_lib.OPEN).index(NAME) == list(cbuild.OPEN_UNITS).index(NAME) == 2          # the third entry of both
    assert cbuild.OPEN_UNITS[NAME] == (NAME + ".hip",) and NAME + ".hip" not in cbuild.SOURCES
    assert NAME not in _lib.LIBRARIES and NAME not in _lib.LATER and NAME not in cbuild.UNITS and NAME not in cbuild.LATER_UNITS
    assert os.path.basename(cbuild.OPEN_LIBS[NAME]) == f"libcough_amd_{NAME}.so" == _lib.OPEN[NAME].soname
    assert os.path.exists(os.path.join(cbuild.CSRC, f"exports_{NAME}.map"))
    assert _lib.load_reverb == _lib.OPEN[NAME].load and _lib.REVERB_SYMBOLS == _lib.OPEN[NAME].symbols


def test_the_binding_declares_what_the_header_declares():
    rec, text = _lib.OPEN[NAME], _header()
    assert list(rec.symbols) == _declared() and len(set(rec.symbols)) == 6
    assert rec.abi == int(re.search(r"#define COUGH_REVERB_ABI_VERSION (\d+)", text).group(1))
    assert int(re.search(r"#define COUGH_REVERB_FFT (\d+)", text).group(1)) == crev.FFT == R.N
    assert int(re.search(r"#define COUGH_REVERB_MAX_TAPS (\d+)", text).group(1)) == crev.MAX_TAPS
    assert int(re.search(r"#define COUGH_REVERB_BOUND_K (\d+)", text).group(1)) == crev.BOUND_K == R.BOUND_K
    assert "rounding noise" in text and "not exact zeros" in text             # the header says so
    for symbol, (_, argtypes) in rec.prototypes.items():
        decl = re.search(r"\b" + symbol + r"\s*\(([^)]*)\)", re.sub(r"/\*.*?\*/", "", text, flags=re.S)).group(1)
        n_args = 0 if decl.strip() == "void" else decl.count(",") + 1
        assert argtypes is None and n_args == 0 or len(argtypes) == n_args, symbol


def test_the_built_library_exports_the_header_and_nothing_else():
    lib = cbuild.OPEN_LIBS[NAME]
    assert os.path.exists(lib), "the library is not built"
    # binutils' nm, or the llvm-nm that ships next to hipcc: the check runs wherever the library can be built
    nm = shutil.which("nm") or os.path.join(os.path.dirname(os.path.realpath(cbuild._hipcc())), "..", "lib", "llvm", "bin", "llvm-nm")
    out = subprocess.run([nm, "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    exported = sorted(line.split()[-1] for line in out.splitlines() if line.strip())
    assert exported == sorted(_declared())


def test_the_source_has_no_float_atomics_and_no_device_sincos():
    source = open(os.path.join(cbuild.CSRC, NAME + ".hip")).read()
    assert "atomic" not in source and "__sincosf" not in source and "sincosf(" not in source
    assert "__sinf" not in source and "__cosf" not in source and "sincospi" not in source
    # the two load-time predicates are reduced one by one: __syncthreads_or returns the OR of !!p, not a bitwise OR
    assert source.count("__syncthreads_or(bad)") == 1 and source.count("__syncthreads_or(live)") == 1
