"""The window plans drawn on the device, without a GPU: the two numpy restatements of the draw contract
(tests/windraw_ref.py) against each other, the distributions over 20 000 restated rows, the labels against
``WindowPlan.labels``, defects planted in the restatement, the refusals of the raw C ABI, and the library's entries in the
open tables (this test asks where "windraw" is in them, never what else is)."""
import inspect
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
from cough_detector_amd import windows as cwin
import windraw_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "windraw"
SR = 16000
BG = (48000, 7, 20000)
EV, LAB = (1600, 3000, 800, 1, 5000, 2400, 40000), (1, 1, 1, 1, 0, 0, 1)
AUG = cda.AudioAugmentor(sample_rate=SR, speed=True)
CHAIN = dict(margin=cda.edge_margin(AUG, 16000), rho_min=cwin.speed_ratios(AUG)[0])
CASES = [dict(), dict(p_cough=0.8, p_distractor=0.9, coughs_per_window=(1, 4), bg_gain_range=(0.5, 2.0), **CHAIN),
         dict(p_cough=1.0, p_distractor=1.0, coughs_per_window=(4, 4), snr_range=(0, 3)), dict(p_cough=0.0, p_distractor=0.0)]


# ------------------------------------------------------------------------------------------------ the restatements
@pytest.mark.parametrize("seed", [0, 2**32 - 1, 2**64 - 1])
def test_the_two_forms_of_the_draw_agree_bit_for_bit(seed):
    for kw in CASES:
        for bg in (BG, (), (1,)):
            a = D.arguments(bg, EV, LAB, 16000, **kw)
            (r1, l1), (r2, l2) = D.draw_rows(seed, 67, a), D.draw_batch(seed, 67, a)
            assert D.same_records(r1, r2) and l1.tolist() == l2.tolist(), (seed, kw, bg)
    a = D.arguments(BG, EV[:4], LAB[:4], 257, m=16)                      # no distractors: the default p_distractor is 0
    assert a["p_distractor"] == 0.0 and D.same_records(D.draw_rows(seed, 9, a)[0], D.draw_batch(seed, 9, a)[0])
    assert D.same_records(D.draw_batch(seed, 130, a)[0][:9], D.draw_batch(seed, 9, a)[0])      # a row is (seed, row) alone


def test_the_table_of_levels_is_the_packages():
    for rng in ((5, 20), (0, 3), (-10.5, 40)):
        got, want = cda.snr_levels(rng), D.snr_levels(*rng)
        assert got.dtype == np.float64 and got.shape == (1024,) and got.tobytes() == want.tobytes()
    levels = 10 * np.log10(cda.snr_levels((5, 20)))
    assert abs(levels[0] - (5 + 15 / 2048)) < 1e-12 and abs(levels[-1] - (20 - 15 / 2048)) < 1e-12
    assert np.allclose(np.diff(levels), 15 / 1024, atol=1e-12) and 0.0146 < 15 / 1024 < 0.015
    with pytest.raises(ValueError, match="lo <= hi"):
        cda.snr_levels((20, 5))


def test_twenty_thousand_restated_rows_have_the_contracts_distributions():
    b, width, p = 20000, 16000, 0.4
    ev, lab = (1600, 3000, 800, 15990, 5000, 2400), (1, 1, 1, 1, 0, 0)
    a = D.arguments(BG, ev, lab, width, p_cough=p, coughs_per_window=(1, 3), bg_gain_range=(0.25, 1.0))
    rec, labels = D.draw_batch(12345, b, a)
    share, sd = labels.mean(), np.sqrt(p * (1 - p) / b)
    assert abs(share - p) <= 4 * sd, (share, sd)
    el, labs = np.array(ev), np.array(lab)
    used = np.arange(4)[None, :] < rec["n_events"][:, None]
    assert (rec["clip"][~used] == -1).all() and (rec["onset"][~used] == 0).all() and (rec["snr_linear"][~used] == 1.0).all()
    is_cough = used & (labs[np.maximum(rec["clip"], 0)] == 1)
    assert set(rec["clip"][is_cough].tolist()) == {0, 1, 2, 3} and set(rec["clip"][used & ~is_cough].tolist()) == {4, 5}
    n_coughs, n_others = is_cough.sum(1), (used & ~is_cough).sum(1)
    assert set(n_coughs.tolist()) == {0, 1, 2, 3} and set(n_others.tolist()) == {0, 1, 2}
    assert abs((n_others > 0).mean() - 0.3) <= 4 * np.sqrt(0.3 * 0.7 / b)
    for r in range(0, b, 97):                                            # the coughs take the first slots
        assert is_cough[r, :n_coughs[r]].all() and not is_cough[r, n_coughs[r]:].any()
    # every used onset inside [lowest, highest]; clip 3 (15990 samples, need 1600) has 16000 - 1600 - (1600 - 15990) + 1
    # = 28791 onsets -- a long range; clip 2 needs all of its 800 samples inside: 15201 onsets, both ends of it drawn
    n_c = el[np.maximum(rec["clip"], 0)]
    need = np.minimum(n_c, 1600)
    assert ((rec["onset"] >= need - n_c) & (rec["onset"] <= width - need))[used].all()
    short = D.arguments(BG, (5, 9), (1, 1), 8, p_cough=1.0, coughs_per_window=(4, 4), m=2)     # onsets -3..6 and -7..6
    srec, _ = D.draw_batch(7, 2000, short)
    for c, lo in ((0, -3), (1, -7)):
        mine = srec["onset"][srec["clip"] == c]
        assert set(mine.tolist()) == set(range(lo, 7)), c
    table = D.snr_levels(5, 20)
    drawn = set(rec["snr_linear"][used].tolist())
    assert drawn <= set(table.tolist()) and table[0] in drawn and table[1023] in drawn and len(drawn) > 1000
    assert ((rec["background"] >= 0) & (rec["background"] < 3)).all() and set(rec["background"].tolist()) == {0, 1, 2}
    assert ((rec["bg_start"] >= 0) & (rec["bg_start"] < np.array(BG)[rec["background"]])).all()
    assert ((rec["bg_gain"] >= 0.25) & (rec["bg_gain"] <= 1.0)).all() and rec["bg_gain"].std() > 0.2


def test_the_labels_are_window_plans_labels_of_the_same_clips():
    for kw in CASES:
        a = D.arguments(BG, EV, LAB, 16000, **kw)
        rec, labels = D.draw_batch(3, 500, a)
        plan = cda.WindowPlan(rec["background"], rec["bg_start"], rec["bg_gain"], rec["n_events"], rec["clip"], rec["onset"],
                              np.zeros((500, 4)))
        assert labels.tolist() == plan.labels(np.array(LAB)).tolist(), kw
        checked = plan.checked(np.array(BG), np.array(EV), 16000)        # what the device draws, the host would accept
        assert checked.records()["clip"].tolist() == rec["clip"].tolist()
    assert set(labels.tolist()) == {0} and D.draw_batch(3, 500, D.arguments(BG, EV, LAB, 16000, **CASES[2]))[1].all()


@pytest.mark.parametrize("defect", D.DEFECTS)
def test_a_planted_defect_is_caught_by_the_record_comparison(defect):
    a = D.arguments(BG, EV, LAB, 16000, **CASES[1])
    good, bad = D.draw_batch(0, 129, a), D.draw_batch(0, 129, a, defect=defect)
    assert D.same_records(*[D.draw_batch(0, 129, a)[0], good[0]]) and not D.same_records(good[0], bad[0]), defect


# ------------------------------------------------------------------------------------------------ the Python front
def _banks(ev=EV, lab=LAB, bg=BG):
    rng = np.random.default_rng(2)
    backgrounds = cda.DeviceClipBank([torch.from_numpy(rng.standard_normal(n).astype(np.float32)) for n in bg], [0] * len(bg), device="cpu")
    events = cda.DeviceClipBank([torch.from_numpy(rng.standard_normal(n).astype(np.float32)) for n in ev], list(lab), device="cpu")
    return backgrounds, events


def test_draw_window_records_checks_its_arguments_as_draw_window_plan_does():
    backgrounds, events = _banks()                               # CPU banks: whatever reaches a kernel raises RuntimeError
    for kw, match in ((dict(p_cough=1.5), "p_cough"), (dict(p_distractor=-0.1), "p_distractor"), (dict(coughs_per_window=(0, 2)), "coughs_per_window"),
                      (dict(coughs_per_window=(1, 5)), "coughs_per_window"), (dict(snr_range=(20, 5)), "lo <= hi"), (dict(seed=-1), "seed"),
                      (dict(b=-1), "b="), (dict(margin=-1), "margin"), (dict(rho_min=1.5), "rho_min"), (dict(min_overlap_seconds=-1), "negative"),
                      (dict(bg_gain_range=(1.0, float("inf"))), "finite"), (dict(width=1000), "inner window"), (dict(width=2**20 + 1), "width")):
        args = dict(b=4, width=16000, seed=0)
        args.update(kw)
        with pytest.raises(ValueError, match=match) as mine:
            cda.draw_window_records(backgrounds, events, **args)
        with pytest.raises(ValueError, match=match) as theirs:
            cda.draw_window_plan(backgrounds, events, args.pop("b"), args.pop("width"), SR, args.pop("seed"), **args)
        assert str(mine.value) == str(theirs.value).replace("draw_window_plan", "draw_window_records")
    with pytest.raises(ValueError, match="no clip labelled 1"):
        cda.draw_window_records(backgrounds, events.subset([4, 5]), 4, 16000, 0)
    with pytest.raises(ValueError, match="no clip labelled 0"):
        cda.draw_window_records(backgrounds, events.subset([0, 1]), 4, 16000, 0, p_distractor=0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cda.draw_window_records(backgrounds, events, 4, 16000, 0)
    for records in (torch.zeros((4, 72), dtype=torch.uint8), torch.zeros((4, 80), dtype=torch.int8), torch.zeros(320, dtype=torch.uint8),
                    torch.zeros((4, 160), dtype=torch.uint8)[:, :80], None):
        with pytest.raises(ValueError, match="records must be"):
            cda.compose_window_records(backgrounds, events, records, 16000)
        with pytest.raises(ValueError, match="records must be"):
            cwin.read_window_records(records)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cda.compose_window_records(backgrounds, events, torch.zeros((4, 80), dtype=torch.uint8), 16000)
    rec = D.draw_batch(0, 5, D.arguments(BG, EV, LAB, 16000))[0]
    back = cwin.read_window_records(torch.from_numpy(rec.view(np.uint8).reshape(5, 80).copy()))
    assert back.dtype == cwin.PLAN_DTYPE == D.PLAN_DTYPE and D.same_records(back, rec)


def test_the_loader_takes_plan_draws_and_defaults_to_the_host():
    assert inspect.signature(cda.ComposedWindowLoader).parameters["plan_draws"].default == "host"
    for fn in (cda.DeviceDataLoader.launch_batch, cda.DeviceDataLoader.launch_batch_drawn, cda.DeviceDataLoader._tail):
        assert inspect.signature(fn).parameters["targets"].default is None
    backgrounds, events = _banks()
    pre = cda.AudioPreprocessor(device="cpu", use_spectral_contrast=False)
    with pytest.raises(ValueError, match="plan_draws must be 'device' or 'host'"):
        cda.ComposedWindowLoader(backgrounds, events, pre, plan_draws="gpu")
    host = cda.ComposedWindowLoader(backgrounds, events, pre, batch_size=4)
    assert host.plan_draws == "host" and host._scalars is None and host.last_records is None and host.last_labels is None
    for draws in ("host", "device"):
        dev = cda.ComposedWindowLoader(backgrounds, events, pre, batch_size=4, plan_draws="device", draws=draws, snr_range=(3, 12),
                                       audio_augmentor=AUG, coughs_per_window=(2, 3), bg_gain_range=(0.5, 1))
        assert dev._scalars == ((0.5, 2, 3, 0.3, 0.5, 1.0), (1600, CHAIN["margin"], CHAIN["rho_min"])) and dev.last_plan is None
    with pytest.raises(ValueError, match="inner window"):                # refused when it is built, in both modes
        cda.ComposedWindowLoader(backgrounds, events, cda.AudioPreprocessor(device="cpu", segment_duration=0.05, use_spectral_contrast=False),
                                 plan_draws="device")


def test_the_split_of_train_windows():
    kept, held = cwin.holdout_split(12, 0.2, 42, 1)
    assert len(held) == 3 and sorted(kept + held) == list(range(12)) and kept == sorted(kept) and held == sorted(held)
    assert (kept, held) == cwin.holdout_split(12, 0.2, 42, 1) and held != cwin.holdout_split(12, 0.2, 43, 1)[1]
    assert cwin.holdout_split(1, 0.2)[0] == [] and cwin.holdout_split(0, 0.2) == ([], [])
    for bad in (0.0, 1.0, 1, None):
        with pytest.raises(ValueError, match="holdout"):
            cwin.holdout_split(5, bad)
    backgrounds, events = _banks(bg=(900, 800, 700, 600, 500, 400))
    train_bg, train_ev, held_bg, held_coughs = cwin.window_split(backgrounds, events)
    assert (len(train_bg), len(held_bg)) == (4, 2) and sorted(train_bg.lengths.tolist() + held_bg.lengths.tolist()) == sorted(backgrounds.lengths.tolist())
    assert held_coughs.labels.tolist() == [1] and train_ev.labels.tolist().count(1) == 4 and train_ev.labels.tolist().count(0) == 1
    assert not set(held_coughs.lengths.tolist()) & set(train_ev.lengths.tolist())
    with pytest.raises(ValueError, match="held-out side without a cough"):
        cwin.window_split(backgrounds, events.subset([4, 5]))
    with pytest.raises(ValueError, match="training side without a cough"):
        cwin.window_split(backgrounds, events.subset([0, 4, 5]))
    with pytest.raises(ValueError, match="training side without a background"):
        cwin.window_split(backgrounds.subset([0]), events)
    with pytest.raises(ValueError, match="p_cough"):
        cda.train_windows(backgrounds, events, "unused", p_cough=1.0)
    with pytest.raises(ValueError, match="unknown model type"):
        cda.train_windows(backgrounds, events, "unused", model_type="large")
    args = cwin.build_parser().parse_args(["bg", "ev", "--output-dir", "out", "--model-type", "small", "--epochs", "2", "--batch-size", "8",
                                           "--lr", "0.01", "--weight-decay", "0.1", "--patience", "3", "--resume", "x.pt",
                                           "--batches-per-epoch", "4", "--val-scenes", "4", "--seconds", "5", "--events", "1,2", "--snr",
                                           "0,10", "--p-cough", "0.4", "--p-augment", "0.2", "--speed", "--draws", "host", "--plan-draws",
                                           "host", "--seed", "7"])
    assert (args.background_dir, args.event_dir, args.output_dir, args.speed, args.plan_draws, args.seed) == ("bg", "ev", "out", True, "host", 7)
    defaults = cwin.build_parser().parse_args(["bg", "ev"])
    assert (defaults.draws, defaults.plan_draws, defaults.speed, defaults.seed, defaults.events, defaults.snr) == ("device", "device", False, 0, "3,6", "5,20")


# ------------------------------------------------------------------------------------------------ the library
def _header():
    return open(os.path.join(ROOT, "include", f"cough_amd_{NAME}.h")).read()


def _declared():
    return set(re.findall(r"^(?:int|size_t|const char\*|void) (cough_[a-z_0-9]+)\s*\(", _header(), flags=re.M))


def _exported(path):
    nm = shutil.which("nm") or os.path.join(os.path.dirname(os.path.realpath(cbuild._hipcc())), "..", "lib", "llvm", "bin", "llvm-nm")
    out = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_the_library_is_the_sixth_of_the_open_tables():
    assert list(_lib.OPEN)[5] == list(cbuild.OPEN_UNITS)[5] == list(cbuild.OPEN_LIBS)[5] == NAME
    assert list(_lib.OPEN)[4] == "windows"
    assert NAME not in _lib.LIBRARIES and NAME not in _lib.LATER and NAME not in cbuild.UNITS and NAME not in cbuild.LATER_UNITS
    assert cbuild.OPEN_UNITS[NAME] == (NAME + ".hip",) and NAME + ".hip" not in cbuild.SOURCES
    for f in (NAME + ".hip", f"exports_{NAME}.map"):
        assert os.path.exists(os.path.join(cbuild.CSRC, f)), f
    assert os.path.basename(cbuild.OPEN_LIBS[NAME]) == f"libcough_amd_{NAME}.so" == _lib.OPEN[NAME].soname
    assert os.path.exists(cbuild.OPEN_LIBS[NAME])


def test_header_record_and_file_name_the_same_entry_points():
    rec, text, declared = _lib.OPEN[NAME], _header(), _declared()
    assert declared == set(rec.symbols) == set(rec.prototypes) == {"cough_windraw_abi_version", "cough_windraw_last_error",
                                                                  "cough_draw_window_plans"}
    assert rec.symbols[0] == rec.abi_symbol and rec.symbols[1] == rec.error_symbol
    assert _exported(rec.path) == declared, sorted(_exported(rec.path) ^ declared)
    assert _lib.WINDRAW_SYMBOLS is rec.symbols and _lib.load_windraw == rec.load and _lib.check_windraw == rec.check
    lib = rec.load()
    assert getattr(lib, rec.abi_symbol)() == rec.abi == 1 and "#define COUGH_WINDRAW_ABI_VERSION 1\n" in text
    assert isinstance(getattr(lib, rec.error_symbol)(), bytes)
    for other in (*_lib.LIBRARIES.values(), *_lib.LATER.values(), *(r for r in _lib.OPEN.values() if r.name != NAME)):
        assert not declared & set(other.symbols), other.name
    assert re.search(rf"#define COUGH_WINDRAW_SNR_LEVELS {cwin.SNR_LEVELS}\b", text) and D.LEVELS == cwin.SNR_LEVELS == 1024
    assert re.search(rf"#define COUGH_WINDRAW_THREADS {D.THREADS}\b", text)
    for symbol, (_, argtypes) in rec.prototypes.items():
        params = re.search(rf"\b{symbol}\s*\(([^)]*)\)", text).group(1)
        count = 0 if params.strip() == "void" else params.count(",") + 1
        assert count == (len(argtypes) if argtypes else 0), symbol
    # the contract, word by word
    for words in ("Philox4x32-10", "(slot, row, 0, 6)", "u = (x + 0.5) * 2^-32", "fires iff u <= p",
                  "lo + min((long long)(u * (double)(hi - lo + 1)), hi - lo)", "j = z >> 22", "lowest = margin + need - n_c",
                  "highest = width - margin - need", "clip = -1, onset = 0, snr_linear = 1.0", "not numpy's"):
        assert words in text, words
    source = open(os.path.join(cbuild.CSRC, NAME + ".hip")).read()
    assert "#pragma clang fp contract(off)" in source and '#include "philox.h"' in source


def test_the_c_abi_refuses_what_the_header_says_it_refuses():
    lib = _lib.load_windraw()
    err = lambda: lib.cough_windraw_last_error().decode()
    nan, inf = float("nan"), float("inf")
    #       seed rows width bgl n_bg evl n_ev cc n_c dc n_d p_c lo hi p_d g_lo g_hi snr  m   margin rho plans labels stream
    good = [0, 0, 16000, 8, 1, 8, 2, 8, 1, 8, 1, 0.5, 1, 2, 0.3, 1.0, 1.0, 8, 1600, 0, 1.0, 8, 8, None]
    assert lib.cough_draw_window_plans(*good) == _lib.OK                                     # n_rows == 0 launches nothing
    assert lib.cough_draw_window_plans(0, 0, 1, None, 0, None, 0, None, 0, None, 0, 0.0, 1, 1, 0.0, 0.0, 0.0, None, 1, 0, 1.0, None, None,
                                       None) == _lib.OK
    for at, value, match in ((1, -1, "negative"), (4, -1, "negative"), (6, -1, "negative"), (8, -1, "negative"), (10, -1, "negative"),
                             (19, -1, "negative"), (2, 0, "width"), (2, 2**20 + 1, "width"), (11, nan, "p_cough"), (11, 1.5, "p_cough"),
                             (11, -0.1, "p_cough"), (14, nan, "p_distractor"), (14, 2.0, "p_distractor"), (12, 0, "coughs per window"),
                             (13, 5, "coughs per window"), (12, 3, "coughs per window"), (8, 0, "no cough clip"),
                             (10, 0, "no distractor clip"), (20, 0.0, "rho_min"), (20, 1.5, "rho_min"), (20, nan, "rho_min"),
                             (18, 0, "min_overlap_samples"), (19, 7201, "inner window"), (18, 16001, "inner window"),
                             (15, nan, "gain range"), (16, inf, "gain range"), (15, -1e39, "gain range")):
        args = list(good)
        args[at] = value
        assert lib.cough_draw_window_plans(*args) == _lib.EINVAL and match in err(), (at, value, err())
    tight = list(good)
    tight[18], tight[19], tight[20] = 1455, 7200, 16000 / 17600          # ceil(1455 / rho) = 1601 > 1600
    assert lib.cough_draw_window_plans(*tight) == _lib.EINVAL and "inner window" in err()
    tight[18] = 1454                                                     # ceil(1599.4) = 1600 fits
    assert lib.cough_draw_window_plans(*tight) == _lib.OK
    one = list(good)
    one[1] = 1
    for at, value, match in ((17, None, "NULL argument"), (21, None, "NULL argument"), (22, None, "NULL argument"),
                             (3, None, "NULL background lengths"), (5, None, "NULL event lengths"), (7, None, "NULL clip list"),
                             (9, None, "NULL clip list"), (3, 2, "4-byte aligned"), (5, 6, "4-byte aligned"), (7, 2, "4-byte aligned"),
                             (9, 2, "4-byte aligned"), (17, 4, "8-byte aligned"), (21, 4, "8-byte aligned"), (22, 4, "8-byte aligned")):
        args = list(one)
        args[at] = value
        assert lib.cough_draw_window_plans(*args) == _lib.EINVAL and match in err(), (at, err())


def test_the_package_exports_the_names():
    for name in ("train_windows", "draw_window_records", "compose_window_records", "snr_levels"):
        assert name in cda.__all__ and getattr(cda, name) is getattr(cwin, name), name
    assert len(set(cda.__all__)) == len(cda.__all__)
    assert "plan_draws" in cwin.ComposedWindowLoader.__doc__ and "cough_amd_windraw.h" in cwin.draw_window_records.__doc__
