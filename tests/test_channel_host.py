"""The capture channel without a GPU: the references of tests/channel_ref.py against scipy and against each other, the
planted defects against the bound the GPU test applies, the host-side refusals, the synthetic microphones, the host
draws and the library's place in the tables."""
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest
from scipy import signal

import cough_detector_amd as cda
from cough_detector_amd import _lib
from cough_detector_amd import build as cbuild
from cough_detector_amd import channel as cch
import channel_ref as R

NAME = "channel"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _live():
    return [row for row in R.batch()[1] if row["rule"] is None]


def test_the_batch_covers_what_the_issue_lists():
    cascades, rows = R.batch()
    assert 35 <= len(rows) <= 45
    assert {len(row["x"]) for row in rows} >= {0, 1, 2, 63, 64, 65, 16383, 16384, 16385, 32769, 48000}
    assert sorted({len(c) for c in cascades}) == [1, 2, 3, 4]
    assert {row["filter"] for row in rows} >= {-1, 0, 1, 2, 3, 4, R.BEYOND} and R.BEYOND >= len(cascades)
    ratios = [row["ratio"] for row in rows]
    assert {0.0, 0.25, 1.0, 1.5} <= set(ratios) and any(np.isnan(r) for r in ratios)
    assert {row["rule"] for row in rows} == {None, "copy", "nan", "zero"}
    first = [row for row in rows if row["x"].size and not np.isfinite(row["x"][0])]
    last = [row for row in rows if row["x"].size and not np.isfinite(row["x"][-1])]
    assert first and last and any(np.isinf(row["x"][-1]) for row in last)
    assert any(np.signbit(row["x"]).all() and not row["x"].any() for row in rows if row["x"].size)     # a row of -0.0
    assert any(row["x"][:100].any() == 0 and row["x"].any() for row in rows if row["x"].size > 100)     # a burst between zeros
    assert cascades[3][0, 3] == 2.0                                                                     # an a0 that is not 1


def test_the_restatement_is_sosfilt_bit_for_bit():
    live = _live()
    got = R.recurrence([row["sos"] for row in live], [row["x"] for row in live], np.float64)
    for row, y in zip(live, got):
        want = signal.sosfilt(R.scipy_sos(row["sos"]), row["x"].astype(np.float64))
        assert y.tobytes() == want.tobytes(), row["name"]


def test_the_clean_emulation_stays_inside_the_bound_and_fixes_k():
    worst = 0.0
    for row in _live():
        y = R.emulate(row["x"], row["sos"])
        worst = max(worst, R.units(y, row["ref"], row["g"], row["peak"]))
        err = np.abs(y.astype(np.float32).astype(np.longdouble) - row["ref"])
        assert (err <= R.bound(row["ref"], row["g"], row["peak"])).all(), row["name"]
    print(f"clean emulation against long double: {worst:.4g} units of 2^-53 G peak")
    # K is 16 times the measured figure: the recorded one may round it up, by less than a quarter
    assert worst <= R.EMULATE_UNITS <= 1.25 * worst and R.BOUND_K == 16 * R.EMULATE_UNITS


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_every_planted_defect_exceeds_the_bound(defect):
    hit = []
    for row in _live():
        if row["x"].size:
            y = R.emulate(row["x"], row["sos"], defect).astype(np.float32).astype(np.longdouble)
            if (np.abs(y - row["ref"]) > R.bound(row["ref"], row["g"], row["peak"])).any():
                hit.append(row["name"])
    assert hit, defect


def test_the_blob_restated():
    cascades = R.bank_sos()
    blob = R.blob_ref(cascades)
    assert blob.shape == (5, R.ENTRY_WORDS) and blob[:, 5].tolist() == [1.0, 1.0, 2.0, 3.0, 4.0]
    for r, sos in enumerate(cascades):
        c = R.normalized(sos)
        for s in range(R.MAX_SECTIONS):
            rec = blob[r, R.REC_WORDS * s:R.REC_WORDS * (s + 1)]
            if s >= len(c):
                assert not rec.any()
                continue
            assert rec[:5].tolist() == c[s].tolist() and not rec[6:8].any() and (s == 0 or rec[5] == 0.0)
            a = np.array([[-c[s, 3], 1.0], [-c[s, 4], 0.0]], dtype=np.longdouble)
            m = np.eye(2, dtype=np.longdouble)
            for _ in range(R.CHUNK):
                m = m @ a
            # M^(2^j) = A^n, n = 64 * 2^j, against long-double products.  This checks the layout and the order of the
            # restatement, not the precision (the bound does that): a wrong power or a transposed matrix is off by the
            # size of the entries.  The slow filters' A is close to a Jordan block (a double pole near 1), whose n-th
            # power moves by about n^2 times a perturbation of A, and every rounding of the squarings is such a
            # perturbation of relative size 2^-53: 8192^2 * 2^-53 = 7.5e-9 of the largest entry, taken twice
            for j in range(R.POWERS):
                top = max(1.0, float(np.abs(m).max()))
                np.testing.assert_allclose(rec[8 + 4 * j:12 + 4 * j].reshape(2, 2), m.astype(np.float64), rtol=0, atol=1.5e-8 * top)
                m = m @ m
    assert cch.ENTRY_WORDS == R.ENTRY_WORDS and (cch.CHUNK, cch.THREADS, cch.MAX_SECTIONS) == (R.CHUNK, R.THREADS, R.MAX_SECTIONS)


def test_the_clip_restated():
    y = np.array([0.5, -1.0, 0.25, -0.0, 0.0, 0.1], dtype=np.float32)
    assert R.clip_ref(y, 0.25).tobytes() == np.array([0.25, -0.25, 0.25, -0.0, 0.0, 0.1], dtype=np.float32).tobytes()
    for ratio in (1.0, 1.5, -0.5, float("nan")):
        assert R.clip_ref(y, ratio).tobytes() == y.tobytes()
    zero = R.clip_ref(y, 0.0)
    assert not zero.any() and np.signbit(zero).tolist() == [False, True, False, True, False, False]      # the sign of a zero stays
    rng = np.random.default_rng(0)
    y = rng.standard_normal(1000).astype(np.float32)
    c = np.float32(np.float32(0.3) * np.abs(y).max())
    assert np.array_equal(R.clip_ref(y, 0.3), np.clip(y, -c, c))


def test_channel_bank_refuses_what_prepare_refuses():
    good = signal.butter(2, 0.1, output="sos")
    bank = cda.ChannelBank.from_sos([good, np.concatenate([good] * 4)])
    assert len(bank) == 2 and bank.n_sections.tolist() == [1, 4] and bank.sos[0].dtype == np.float64
    bad = [np.concatenate([good] * 5),                           # five sections
           good[0],                                              # not (S, 6)
           np.zeros((0, 6)),
           good * np.array([1, 1, 1, 0, 1, 1]),                  # a0 = 0
           good * np.array([1, np.nan, 1, 1, 1, 1]),
           good * np.array([1, 1, 1, 1, 1, np.inf]),
           np.array([[1.0, 0, 0, 1, 0, 1.0]]),                   # |a2| = 1
           np.array([[1.0, 0, 0, 1, 0, -1.0]]),
           np.array([[1.0, 0, 0, 1, 1.6, 0.6]]),                 # |a1| = 1 + a2
           np.array([[1.0, 0, 0, 1, -1.7, 0.6]]),
           np.array([[1.0, 0, 0, 0.5, 0, 0.6]])]                 # a2 / a0 = 1.2
    for sos in bad:
        with pytest.raises(ValueError):
            cda.ChannelBank.from_sos([good, sos])
    with pytest.raises(ValueError):
        cda.ChannelBank.from_sos([])
    cda.ChannelBank.from_sos([np.array([[1.0, 0, 0, 2.0, 3.1, 1.2]])])          # stable after the division by a0


def test_plan_array_refuses_before_any_launch():
    arr = cch.plan_array([(3, 0.25), (-1, 1.0), (0, float("nan")), (4, -2.0)], n_bank=5)
    assert arr.dtype == cch.PLAN_DTYPE == R.PLAN_DTYPE and arr.itemsize == 8
    assert arr["filter"].tolist() == [3, -1, 0, 4] and arr["clip_ratio"][:2].tolist() == [0.25, 1.0] and np.isnan(arr["clip_ratio"][2])
    for bad in ((5, 0.5), (-2, 0.5), (2**40, 0.5)):
        with pytest.raises(ValueError):
            cch.plan_array([(0, 1.0), bad], n_bank=5)
    raw = np.zeros(2, dtype=cch.PLAN_DTYPE)
    raw["filter"] = (0, 7)
    with pytest.raises(ValueError):
        cch.check_plans(raw, 5)
    with pytest.raises(ValueError):
        cch.check_plans(np.zeros((2, 2), dtype=np.int32), 5)
    assert cch.check_plans(arr, 5).tobytes() == arr.tobytes()
    for p_clip, clip_range in ((-0.1, (0.25, 1.0)), (1.5, (0.25, 1.0)), (0.3, (0.8, 0.2)), (0.3, (0.25, 1.5)), (0.3, (float("nan"), 1.0))):
        with pytest.raises(ValueError):
            cda.AudioAugmentor(channel=cda.synth_channels(1)[0], p_clip=p_clip, clip_range=clip_range)
    with pytest.raises(TypeError):
        cda.AudioAugmentor(channel=[signal.butter(2, 0.1, output="sos")])


def test_the_rbj_sections_at_their_design_points():
    sr = 16000
    for f0 in (20.0, 400.0, 3000.0, 7800.0):
        for kind, far in (("highpass", sr / 2), ("lowpass", 0.0)):
            sos = cch.rbj_section(kind, f0, sr, 1 / np.sqrt(2)).reshape(1, 6)
            sos = sos / sos[0, 3]
            _, h = signal.sosfreqz(sos, worN=[f0, far, (sr / 2) - far], fs=sr)
            np.testing.assert_allclose(np.abs(h), [1 / np.sqrt(2), 1.0, 0.0], atol=1e-9)      # 3 dB down, unity, a zero
    for f0, gain_db, q in ((200.0, -12.0, 0.5), (1000.0, 6.0, 2.0), (6000.0, 12.0, 4.0)):
        sos = cch.rbj_section("peak", f0, sr, q, gain_db).reshape(1, 6)
        sos = sos / sos[0, 3]
        _, h = signal.sosfreqz(sos, worN=[f0, 0.0, sr / 2], fs=sr)
        np.testing.assert_allclose(20 * np.log10(np.abs(h)), [gain_db, 0.0, 0.0], atol=1e-9)


def test_synth_channels_is_seeded_and_follows_its_table():
    bank, table = cda.synth_channels(40, seed=3)
    again, table2 = cda.synth_channels(40, seed=3)
    other, _ = cda.synth_channels(40, seed=4)
    assert len(bank) == 40 and table.shape == (40, 9) and table.tobytes() == table2.tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(bank.sos, again.sos)) and bank.sos[0].tobytes() != other.sos[0].tobytes()
    assert ((table[:, 0] >= 20) & (table[:, 0] <= 400) & (table[:, 1] >= 3000) & (table[:, 1] <= 7800)).all()
    assert set(table[:, 2].astype(int).tolist()) == {0, 1, 2}
    for sos, row in zip(bank.sos, table):
        k = int(row[2])
        assert sos.shape == (2 + k, 6) and np.isnan(row[3 + 3 * k:]).all() and np.isfinite(row[:3 + 3 * k]).all()
        want = [cch.rbj_section("highpass", row[0], 16000, 1 / np.sqrt(2)), cch.rbj_section("lowpass", row[1], 16000, 1 / np.sqrt(2))]
        want += [cch.rbj_section("peak", *row[3 + 3 * j:4 + 3 * j], 16000, row[5 + 3 * j], row[4 + 3 * j]) for j in range(k)]
        assert np.stack(want).tobytes() == sos.tobytes()
        for j in range(k):
            f0, gain_db, q = row[3 + 3 * j:6 + 3 * j]
            assert 200 <= f0 <= 6000 and -12 <= gain_db <= 12 and 0.5 <= q <= 4
    for kw in (dict(peaks=(0, 3)), dict(lowpass_hz=(3000, 8000)), dict(highpass_hz=(0, 400)), dict(peak_q=(4, 0.5)), dict(n=0)):
        with pytest.raises(ValueError):
            cda.synth_channels(**{"n": 2, **kw})


def _stream(aug, lengths, method):
    random.seed(77)
    items = [getattr(aug, method)(n) for n in lengths]
    return items, random.random()


def test_the_host_draws_come_last_and_leave_the_stream_alone_without_a_bank():
    lengths = [16000, 9000, 12000, 700, 16000, 4000]
    bank, _ = cda.synth_channels(5, seed=2)
    rirs, _ = cda.synth_rirs(3, seed=2)
    for kw in (dict(), dict(speed=True), dict(pitch=True), dict(speed=True, pitch=True, reverb=rirs)):
        plain = cda.AudioAugmentor(p_augment=0.6, **kw)
        assert plain.channel is None
        want, after = _stream(plain, lengths, "draw_item_reverb")
        items, after_none = _stream(plain, lengths, "draw_item_channel")
        assert after == after_none and all(it[5] is None and len(it) == 6 for it in items)
        for a, b in zip(want, items):
            assert bytes(a[0]) == bytes(b[0]) and a[1:] == b[1:5]
        # with a bank: the existing draws are the same, the channel's follow them
        mic = cda.AudioAugmentor(p_augment=0.6, channel=bank, p_clip=0.5, clip_range=(0.3, 0.9), **kw)
        random.seed(77)
        for n in lengths:
            state = random.getstate()
            got = mic.draw_item_channel(n)
            end = random.getstate()
            random.setstate(state)
            base = plain.draw_item_reverb(n)
            drawn = R.host_channel_draw(random, 0.6, len(bank), 0.5, (0.3, 0.9))
            assert random.getstate() == end
            assert bytes(got[0]) == bytes(base[0]) and got[1:5] == base[1:] and got[5] == drawn
            assert mic.draw_item_reverb(n) is not None                  # the old methods keep their shape
        assert len(mic.draw_item_reverb(100)) == 5 and len(mic.draw_item_pitched(100)) == 4 and len(mic.draw_item(100)) == 3
    random.seed(5)
    aug = cda.AudioAugmentor(p_augment=0.5, channel=bank)
    fired = [aug.draw_item_channel(100)[5] for _ in range(200)]
    hits = [f for f in fired if f is not None]
    assert 60 < len(hits) < 140 and {f[0] for f in hits} == set(range(5))
    clipped = [f[1] for f in hits if f[1] != 1.0]
    assert 0.1 * len(hits) < len(clipped) < 0.55 * len(hits) and all(0.25 <= r <= 1.0 for r in clipped)
    pipe, _ = cda.create_augmentation_pipeline(channel=bank, p_clip=0.1, clip_range=(0.5, 0.6))
    assert pipe.channel is bank and pipe.p_clip == 0.1 and pipe.clip_range == (0.5, 0.6)
    assert cda.create_augmentation_pipeline()[0].channel is None


def test_the_device_draw_restated():
    plans = R.draw_channel_ref(7, 400, 0.5, 9, 0.3, 0.25, 1.0)
    assert plans.dtype == R.PLAN_DTYPE
    fired = plans["filter"] >= 0
    assert 140 < fired.sum() < 260 and set(plans["filter"][fired].tolist()) == set(range(9))
    assert (plans["clip_ratio"][~fired] == 1.0).all()
    clipped = plans["clip_ratio"][fired] != 1.0
    assert 0.15 * fired.sum() < clipped.sum() < 0.45 * fired.sum()
    assert ((plans["clip_ratio"] >= 0.25) & (plans["clip_ratio"] <= 1.0)).all()
    none = R.draw_channel_ref(7, 50, 1.0, 0, 1.0, 0.5, 0.5)
    assert (none["filter"] == -1).all() and (none["clip_ratio"] == 0.5).all()       # no bank: the ceiling alone
    assert (R.draw_channel_ref(7, 50, 0.0, 3, 1.0, 0.0, 0.5)["filter"] == -1).all()
    # the counter is the channel's own: another last word gives other draws
    words = R.D.philox4x32_10((0, np.arange(4, dtype=np.uint64), 0, 5), (7, 0))
    assert not np.array_equal(words[0], R.D.philox4x32_10((0, np.arange(4, dtype=np.uint64), 0, 4), (7, 0))[0])


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
    assert list(_lib.OPEN).index(NAME) == list(cbuild.OPEN_UNITS).index(NAME) == 3          # the fourth entry of both
    assert cbuild.OPEN_UNITS[NAME] == (NAME + ".hip",) and NAME + ".hip" not in cbuild.SOURCES
    assert NAME not in _lib.LIBRARIES and NAME not in _lib.LATER and NAME not in cbuild.UNITS and NAME not in cbuild.LATER_UNITS
    assert os.path.basename(cbuild.OPEN_LIBS[NAME]) == f"libcough_amd_{NAME}.so" == _lib.OPEN[NAME].soname
    assert os.path.exists(os.path.join(cbuild.CSRC, f"exports_{NAME}.map"))
    assert _lib.load_channel == _lib.OPEN[NAME].load and _lib.CHANNEL_SYMBOLS == _lib.OPEN[NAME].symbols
    assert len(_lib.LIBRARIES) + len(_lib.LATER) + len(_lib.OPEN) >= 13


def test_the_binding_declares_what_the_header_declares():
    rec, text = _lib.OPEN[NAME], _header()
    assert list(rec.symbols) == _declared() and len(set(rec.symbols)) == 6
    assert rec.abi == int(re.search(r"#define COUGH_CHANNEL_ABI_VERSION (\d+)", text).group(1))
    for macro, value in (("MAX_SECTIONS", cch.MAX_SECTIONS), ("CHUNK", cch.CHUNK), ("THREADS", cch.THREADS),
                         ("ENTRY_WORDS", cch.ENTRY_WORDS)):
        assert int(re.search(rf"#define COUGH_CHANNEL_{macro} (\d+)", text).group(1)) == value
    for symbol, (_, argtypes) in rec.prototypes.items():
        decl = re.search(r"\b" + symbol + r"\s*\(([^)]*)\)", re.sub(r"/\*.*?\*/", "", text, flags=re.S)).group(1)
        n_args = 0 if decl.strip() == "void" else decl.count(",") + 1
        assert argtypes is None and n_args == 0 or len(argtypes) == n_args, symbol
    for name in ("ChannelBank", "synth_channels", "channel_rows", "draw_channel"):
        assert name in cda.__all__ and getattr(cda, name) is getattr(cch, name), name


def test_the_built_library_exports_the_header_and_nothing_else():
    lib = cbuild.OPEN_LIBS[NAME]
    assert os.path.exists(lib), "the library is not built"
    nm = shutil.which("nm") or os.path.join(os.path.dirname(os.path.realpath(cbuild._hipcc())), "..", "lib", "llvm", "bin", "llvm-nm")
    out = subprocess.run([nm, "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    exported = sorted(line.split()[-1] for line in out.splitlines() if line.strip())
    assert exported == sorted(_declared())


def test_the_source_is_plain_hip_without_atomics():
    source = open(os.path.join(cbuild.CSRC, NAME + ".hip")).read()
    assert "atomic" not in source and "asm" not in source
    assert source.count("__syncthreads_or(bad)") == 1 and source.count("__syncthreads_or(live)") == 1
