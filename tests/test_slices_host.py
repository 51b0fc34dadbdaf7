"""Slicing recordings into active clips, without a GPU: the two numpy restatements (tests/slices_ref.py) against each
other and against hand-written rows, the tenth library's table entries (what tests/test_libraries_host.py checks for the
nine, applied to ``_lib.LATER`` / ``build.LATER_UNITS``), the C-ABI's argument checks, the Python front's parameter
checks, the group split and the WAVE writer."""
import inspect
import os
import re
import shutil
import subprocess
import wave

import numpy as np
import pytest
import torch

import cough_detector_amd as cda
from cough_detector_amd import _lib
from cough_detector_amd import build as cbuild
from cough_detector_amd import data as cdata
from cough_detector_amd import slices as cslices
import slices_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINE = ("amd", "loop", "data", "segments", "score", "draws", "soft", "warp", "pitch")
SMALL = dict(frame_length=8, hop_length=4, seg_len=32)
SHIPPED = dict(use_pcen=False, use_pre_emphasis=False, use_delta_delta=False, use_spectral_contrast=False)


# ------------------------------------------------------------------------------------------------ the restatements
def _same(a, b, what):
    assert a["count"] == b["count"] and a["clip_active"] == b["clip_active"], what
    for key in ("m", "cnt", "keep"):
        assert a[key].tolist() == b[key].tolist(), (what, key, a[key].tolist(), b[key].tolist())
    assert a["peak"] == b["peak"] or (np.isnan(a["peak"]) and np.isnan(b["peak"])), what


@pytest.mark.parametrize("stride", [32, 16, 10, 48])
def test_closed_forms_equal_the_set_definition(stride):
    """Every clip length 1..200 at frame 8 / hop 4 / window 32: random activity on three energy levels (few levels:
    many windows tie in m), all frames active, nothing active; caps None, 1, 2, 3; shares 0, 0.5 and 1."""
    rng = np.random.default_rng(stride)
    ratio, floor = 0.25, 1e-3
    seen_cap, seen_tie = 0, 0
    for n in range(1, 201):
        F = R.n_frames(n, SMALL["frame_length"], SMALL["hop_length"])
        min_active = (0.0, 0.5, 1.0)[n % 3]
        cases = [(rng.choice([1e-6, 0.3, 1.0], size=F), cap) for cap in (None, 1, 2, 3)]
        cases += [(np.full(F, 0.7), None), (np.full(F, 0.7), 2), (np.full(F, 1e-4), None), (np.zeros(F), 1)]
        for e, cap in cases:
            args = (e, n, 8, 4, 32, stride, ratio, floor, min_active, cap)
            closed, brute = R.clip_closed(*args), R.clip_brute(*args)
            _same(closed, brute, (n, stride, cap))
            assert len(closed["m"]) == R.n_windows(n, 32, stride) and (closed["m"] <= closed["cnt"]).all()
            uncapped = R.clip_closed(*args[:-1], None)
            if cap is not None and uncapped["count"] > cap:
                seen_cap += 1
                assert closed["count"] == cap and (closed["keep"] <= uncapped["keep"]).all()
                kept, dropped = closed["m"][closed["keep"] == 1], closed["m"][(uncapped["keep"] == 1) & (closed["keep"] == 0)]
                assert kept.min() >= dropped.max()
                seen_tie += int(kept.min() == dropped.max())
            else:
                assert closed["keep"].tolist() == uncapped["keep"].tolist()
        assert R.clip_closed(np.full(F, 1e-4), n, 8, 4, 32, stride, ratio, floor, 0.0)["count"] == 0     # below the floor
        everything = R.clip_closed(np.full(F, 0.7), n, 8, 4, 32, stride, ratio, floor, 1.0)
        assert everything["m"].tolist() == everything["cnt"].tolist()
        assert everything["keep"].tolist() == (everything["cnt"] > 0).astype(int).tolist()
    assert seen_cap > 100 and seen_tie > 50                              # the cap and its tie rule were exercised


@pytest.mark.parametrize("n,stride,frames,windows,cnt", [
    (5, 16, 1, 1, [1]),                      # n < frame_length: one frame, the whole clip, in the one window
    (31, 16, 6, 1, [6]),                     # seg_len - 1: one short window; frames start at 0..20
    (32, 16, 7, 1, [7]),                     # seg_len: frames start at 0..24, the last ends at 32
    (47, 16, 10, 1, [7]),                    # seg_len + stride - 1: still one window, the frames from 28 on lie outside
    (48, 16, 11, 2, [7, 7]),                 # seg_len + stride: [0, 32) and [16, 48)
    (52, 10, 12, 3, [7, 6, 7]),              # a stride that is no multiple of the hop: [10, 42) holds the starts 12..32
    (60, 48, 14, 1, [7]),                    # a stride above the window: the tail is in no window
    (80, 48, 19, 2, [7, 7]),
])
def test_hand_written_window_geometry(n, stride, frames, windows, cnt):
    assert R.n_frames(n, 8, 4) == frames and R.n_windows(n, 32, stride) == windows
    for fn in (R.clip_closed, R.clip_brute):
        r = fn(np.ones(frames), n, 8, 4, 32, stride, 0.5, 0.1, 0.5)
        assert r["cnt"].tolist() == cnt and r["m"].tolist() == cnt and r["keep"].tolist() == [1] * windows
        assert r["peak"] == 1.0 and r["clip_active"] == frames and r["count"] == windows
    assert cslices.window_counts(np.array([n]), 32, stride).tolist() == [windows]


def test_hand_written_rows():
    e = np.array([1, 1, 1, 0, 0, 0, 0, 0, 0, 1, 1, .9], dtype=np.float64)      # n = 52, stride 10: windows of 7, 6, 7 frames
    for fn in (R.clip_closed, R.clip_brute):
        r = fn(e, 52, 8, 4, 32, 10, 0.5, 0.1, 0.4)
        assert r["m"].tolist() == [3, 0, 3] and r["keep"].tolist() == [1, 0, 1] and r["clip_active"] == 6     # 3 >= 0.4 * 7
        assert fn(e, 52, 8, 4, 32, 10, 0.5, 0.1, 0.4, 1)["keep"].tolist() == [1, 0, 0]       # the tie goes to the earlier
        assert fn(e, 52, 8, 4, 32, 10, 0.5, 0.1, 0.5)["keep"].tolist() == [0, 0, 0]          # 3 < 0.5 * 7
        assert fn(e, 52, 8, 4, 32, 10, 0.95, 0.1, 0.0)["m"].tolist() == [3, 0, 2]            # 0.9 < 0.95
        assert fn(e, 52, 8, 4, 32, 10, 0.95, 0.1, 0.0, 1)["keep"].tolist() == [1, 0, 0]
        assert fn(e * 0.05, 52, 8, 4, 32, 10, 0.5, 0.1, 0.0)["keep"].tolist() == [0, 0, 0]   # E_max = 0.05 < floor
        assert fn(e * 0.15, 52, 8, 4, 32, 10, 0.5, 0.1, 0.0)["m"].tolist() == [3, 0, 3]      # thr = max(0.075, 0.1): 0.135 stays
        assert fn(e * 0.105, 52, 8, 4, 32, 10, 0.5, 0.1, 0.0)["m"].tolist() == [3, 0, 2]     # ... and 0.0945 < floor does not
        for bad in (np.nan, np.inf):
            x = e.copy()
            x[4] = bad
            r = fn(x, 52, 8, 4, 32, 10, 0.5, 0.1, 0.0)
            assert np.isnan(r["peak"]) and r["count"] == 0 and r["clip_active"] == 0 and r["m"].tolist() == [0, 0, 0]
    tab = R.table_ref([e, np.ones(1)], [52, 5], 32, 10, 8, 4, threshold_db=-3.0, floor_db=-10.0, min_active=0.4)
    assert tab["counts"] == [2, 1] and tab["windows"] == [3, 1] and tab["keep"] == [1, 0, 1, 1]
    assert (tab["clip"], tab["start"], tab["length"], tab["row_active"]) == ([0, 0, 1], [0, 20, 0], [32, 32, 5], [3, 3, 1])


# ------------------------------------------------------------------------------------------------ the tenth library
def _header(name):
    return open(os.path.join(ROOT, "include", "cough_amd.h" if name == "amd" else f"cough_amd_{name}.h")).read()


def _exported(path):
    nm = shutil.which("nm") or os.path.join(os.path.dirname(os.path.realpath(cbuild._hipcc())), "..", "lib", "llvm", "bin", "llvm-nm")
    out = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_the_later_tables_list_the_tenth_library_and_the_nine_stay():
    assert tuple(_lib.LATER) == tuple(cbuild.LATER_UNITS) == tuple(cbuild.LATER_LIBS) == ("slices",)
    assert tuple(_lib.LIBRARIES) == tuple(cbuild.UNITS) == tuple(cbuild.LIBS) == NINE
    assert cbuild.LATER_UNITS["slices"] == ("slices.hip",) and not set(_lib.LATER) & set(_lib.LIBRARIES)
    for doc in (_lib.__doc__, cbuild.__doc__):
        assert "two tables" in doc and "test_libraries_host" in doc


@pytest.mark.parametrize("name", list(_lib.LATER))
def test_header_record_and_file_name_the_same_entry_points(name):
    rec, text = _lib.LATER[name], _header(name)
    declared = set(re.findall(r"^(?:int|size_t|const char\*|void) (cough_[a-z_0-9]+)\s*\(", text, flags=re.M))
    assert declared == set(rec.symbols) == set(rec.prototypes), declared ^ set(rec.symbols)
    assert len(rec.symbols) == len(set(rec.symbols)) == 4
    assert rec.symbols[0] == rec.abi_symbol == f"cough_{name}_abi_version" and rec.symbols[1] == rec.error_symbol == f"cough_{name}_last_error"
    assert os.path.basename(rec.path) == rec.soname == f"libcough_amd_{name}.so"
    assert _exported(rec.path) == declared, sorted(_exported(rec.path) ^ declared)
    assert getattr(_lib, f"{name.upper()}_SYMBOLS") is rec.symbols and getattr(_lib, f"{name.upper()}_LIB_PATH") == rec.path
    assert getattr(_lib, f"load_{name}") == rec.load and getattr(_lib, f"check_{name}") == rec.check
    lib = rec.load()
    for s in rec.symbols:
        assert hasattr(lib, s), s
    assert getattr(lib, rec.abi_symbol)() == rec.abi == 1
    assert f"#define COUGH_{name.upper()}_ABI_VERSION 1\n" in text
    assert isinstance(getattr(lib, rec.error_symbol)(), bytes)
    # none of the nine binds, exports or so much as mentions one of them
    for other in NINE:
        assert not declared & set(_lib.LIBRARIES[other].symbols), other
        for s in declared:
            assert not hasattr(_lib.LIBRARIES[other].load(), s), (other, s)
            assert s not in _header(other), (other, s)


@pytest.mark.parametrize("name", list(_lib.LATER))
def test_a_missing_library_is_an_error(name, monkeypatch):
    rec = _lib.LATER[name]
    monkeypatch.setattr(rec, "handle", None)
    monkeypatch.setattr(rec, "path", os.path.join(ROOT, "no_such_dir", rec.soname))
    with pytest.raises(RuntimeError, match=r"is missing: the HIP extension is not built\. Run `python -m cough_detector_amd\.build`"):
        getattr(_lib, f"load_{name}")()


@pytest.mark.parametrize("name", list(_lib.LATER))
def test_the_build_covers_the_library(name, monkeypatch):
    assert cbuild.LATER_UNITS[name] == (name + ".hip",) and name + ".hip" not in cbuild.SOURCES
    assert os.path.basename(cbuild.LATER_LIBS[name]) == f"libcough_amd_{name}.so" == _lib.LATER[name].soname
    assert os.path.dirname(cbuild.LATER_LIBS[name]) == os.path.dirname(cbuild.LIB) and os.path.exists(cbuild.LATER_LIBS[name])
    own = (name + ".hip", f"exports_{name}.map")
    for s in own:
        assert os.path.exists(os.path.join(cbuild.CSRC, s)), s
    newer = []
    monkeypatch.setattr(cbuild.os.path, "getmtime", lambda p: 2.0 if os.path.basename(p) in newer else 1.0)
    assert not cbuild.is_stale()
    for dep in own + (f"cough_amd_{name}.h", "common.h", "build.py"):
        newer[:] = [dep]
        assert cbuild.is_stale(), dep
    newer[:] = []
    assert not cbuild.is_stale()
    monkeypatch.setitem(cbuild.LATER_LIBS, name, os.path.join(ROOT, "no_such_dir", f"libcough_amd_{name}.so"))
    assert cbuild.is_stale()


# ------------------------------------------------------------------------------------------------ the C-ABI's checks
FAKE = 1 << 20


def _activity_args(**kw):
    a = dict(energy=FAKE, frame_offs=FAKE, lengths=FAKE, window_offs=FAKE, n=4, frame_length=400, hop_length=160,
             seg_len=16000, stride=8000, max_windows=3, ratio=1e-3, floor=1e-6, min_active=0.5, peak=FAKE, clip_active=FAKE,
             active=FAKE, keep=FAKE, counts=FAKE, stream=None)
    a.update(kw)
    return list(a.values())


def _list_args(**kw):
    a = dict(keep=FAKE, active=FAKE, lengths=FAKE, window_offs=FAKE, row_offs=FAKE, n=4, seg_len=16000, stride=8000,
             clip=FAKE, start=FAKE, length=FAKE, row_active=FAKE, stream=None)
    a.update(kw)
    return list(a.values())


@pytest.mark.parametrize("kw,word", [
    (dict(energy=None), "NULL"), (dict(keep=None), "NULL"), (dict(counts=None), "NULL"), (dict(n=-1), "n_clips"),
    (dict(frame_length=0), "frame_length"), (dict(hop_length=0), "hop_length"), (dict(seg_len=399), "seg_len"),
    (dict(stride=0), "stride"), (dict(max_windows=0), "max_windows"), (dict(ratio=-1.0), "ratio"),
    (dict(ratio=float("nan")), "ratio"), (dict(floor=float("inf")), "floor"), (dict(min_active=-0.5), "min_active"),
    (dict(min_active=float("nan")), "min_active"), (dict(active=FAKE + 2), "4-byte"), (dict(peak=FAKE + 4), "8-byte"),
    (dict(window_offs=FAKE + 4), "8-byte")])
def test_window_activity_checks_its_arguments_before_the_launch(kw, word):
    lib = _lib.load_slices()
    assert lib.cough_window_activity(*_activity_args(**kw)) == _lib.EINVAL
    msg = lib.cough_slices_last_error().decode()
    assert msg.startswith("cough_window_activity: ") and word in msg, msg
    with pytest.raises(ValueError, match="cough_window_activity"):
        _lib.check_slices(_lib.EINVAL, "cough_window_activity")


@pytest.mark.parametrize("kw,word", [
    (dict(keep=None), "NULL"), (dict(row_active=None), "NULL"), (dict(n=-1), "n_clips"), (dict(seg_len=0), "seg_len"),
    (dict(stride=0), "stride"), (dict(start=FAKE + 1), "4-byte"), (dict(clip=FAKE + 4), "8-byte"),
    (dict(row_offs=FAKE + 4), "8-byte")])
def test_list_windows_checks_its_arguments_before_the_launch(kw, word):
    lib = _lib.load_slices()
    assert lib.cough_list_windows(*_list_args(**kw)) == _lib.EINVAL
    msg = lib.cough_slices_last_error().decode()
    assert msg.startswith("cough_list_windows: ") and word in msg, msg


def test_no_clips_launch_nothing():
    lib = _lib.load_slices()
    assert lib.cough_window_activity(*_activity_args(n=0)) == _lib.OK and lib.cough_list_windows(*_list_args(n=0)) == _lib.OK


# ------------------------------------------------------------------------------------------------ the Python front
class _Pre:
    segment_samples, sample_rate = 16000, 16000


@pytest.mark.parametrize("kw,name", [
    (dict(stride=0), "stride"), (dict(stride=1.5), "stride"), (dict(stride=True), "stride"), (dict(stride=2**31), "stride"),
    (dict(frame_length=0), "frame_length"), (dict(hop_length=-1), "hop_length"), (dict(frame_length=5000), "frame_length"),
    (dict(threshold_db=float("nan")), "threshold_db"), (dict(floor_db="x"), "floor_db"), (dict(floor_db=1e6), "floor_db"),
    (dict(min_active=-0.1), "min_active"), (dict(min_active=1.5), "min_active"), (dict(min_active=float("inf")), "min_active"),
    (dict(max_per_clip=0), "max_per_clip"), (dict(max_per_clip=2.0), "max_per_clip")])
def test_find_windows_checks_its_parameters(kw, name):
    bank = cda.DeviceClipBank([torch.zeros(100)], [0], device="cpu")
    with pytest.raises(ValueError, match=rf"find_windows: .*{name}"):
        cda.find_windows(bank, _Pre(), **kw)
    with pytest.raises(ValueError, match=rf"find_windows: .*{name}"):
        cda.slice_bank(bank, _Pre(), **kw)


def test_find_windows_needs_the_gpu_and_a_window_no_shorter_than_a_frame():
    bank = cda.DeviceClipBank([torch.zeros(100)], [0], device="cpu")
    with pytest.raises(RuntimeError, match="find_windows: the bank lives on cpu.*no CPU fallback"):
        cda.find_windows(bank, _Pre())

    class Short:
        segment_samples, sample_rate = 300, 16000
    with pytest.raises(ValueError, match="find_windows: .*segment_samples=300 is below frame_length=400"):
        cda.find_windows(bank, Short())
    p = cslices._params("find_windows", _Pre())
    assert p[:5] == (400, 160, 16000, 16000, 2**31 - 1) and p[5:] == (*R.levels(), 0.5)
    assert cslices._params("find_windows", _Pre(), stride=5000, max_per_clip=np.int64(3), min_active=1)[3:5] == (5000, 3)


def test_inactive_clips_reads_the_counts():
    z = torch.zeros(0)
    table = cda.WindowTable(z, z, z, z, z, z, z, torch.tensor([2, 0, 1, 0, 0], dtype=torch.int32))
    got = cda.inactive_clips(table)
    assert got.dtype == torch.int64 and got.device.type == "cpu" and got.tolist() == [1, 3, 4]


# ------------------------------------------------------------------------------------------------ the group split
LABELS = [0, 1, 0, 0, 1, 1, 0, 1, 0, 0, 1, 0, 1, 1, 0, 0, 1, 0, 1, 0]
PARENT = {(0.2, 42): ([8, 18, 12, 19, 7, 15, 17, 4, 14, 2, 1, 5, 9, 3, 13, 0], [6, 16, 10, 11]),
          (0.25, 7): ([2, 0, 13, 9, 1, 10, 5, 15, 4, 19, 3, 14, 12, 6, 7], [16, 18, 8, 17, 11])}


def test_group_split_keeps_every_group_on_one_side():
    rng = np.random.default_rng(5)
    group_labels = rng.integers(0, 2, size=30)
    groups = rng.permutation(np.repeat(np.arange(30) * 7 + 3, rng.integers(1, 6, size=30)))     # names are not 0..n-1
    labels = group_labels[(groups - 3) // 7]
    for split, seed in ((0.2, 42), (0.4, 1)):
        train, val = cda.stratified_group_split(labels, groups, split, seed)
        assert sorted(train + val) == list(range(len(labels))) and not set(groups[train]) & set(groups[val])
        names = np.unique(groups)
        want = cda.stratified_split(group_labels[(names - 3) // 7], split, seed)
        for side, side_groups in zip((train, val), want):
            # the groups in the order stratified_split gave them, each group's members ascending
            assert side == [int(i) for g in side_groups for i in np.flatnonzero(groups == names[g])]
        assert (train, val) == cda.stratified_group_split(torch.tensor(labels), torch.tensor(groups), split, seed)


def test_group_split_of_singletons_is_the_stratified_split():
    for (split, seed), want in PARENT.items():
        assert cda.stratified_group_split(LABELS, list(range(len(LABELS))), split, seed) == want
        assert cda.stratified_group_split(LABELS, [f"rec{k:02d}" for k in range(len(LABELS))], split, seed) == want
    assert cda.stratified_group_split(LABELS, range(20)) == cda.stratified_split(LABELS)


def test_group_split_refuses_a_group_with_two_labels_and_ragged_input():
    with pytest.raises(ValueError, match=r"stratified_group_split: group 3 holds clips of different labels \(\[0, 1\]\)"):
        cda.stratified_group_split([0, 0, 1, 1, 0, 1], [1, 1, 2, 2, 3, 3])
    with pytest.raises(ValueError, match="stratified_group_split: labels and groups"):
        cda.stratified_group_split([0, 1, 0], [1, 2])
    with pytest.raises(ValueError, match="stratified_split: class .* has a single member"):
        cda.stratified_group_split([0, 0, 0, 0, 1, 1], [0, 1, 2, 3, 4, 4])      # one cough recording, however many clips


def test_prepare_group_split_keeps_groups_whole_and_prepare_dataset_split_is_unchanged():
    clips = [torch.full((10 + k,), float(k)) for k in range(len(LABELS))]
    bank = cda.DeviceClipBank(clips, LABELS, device="cpu")

    def same(a, idx):
        assert a.lengths.tolist() == [10 + k for k in idx] and a.labels.tolist() == [LABELS[k] for k in idx]
        assert torch.equal(a.data, torch.cat([clips[k] for k in idx]))
    for (split, seed), want in PARENT.items():                    # the indices the parent commit gave
        assert cda.stratified_split(LABELS, split, seed) == want
        train, val = cda.prepare_dataset_split(bank, val_split=split, random_state=seed)
        same(train, want[0]), same(val, want[1])
        train, val = cda.prepare_group_split(bank, range(len(LABELS)), split, seed)      # every clip its own group
        same(train, want[0]), same(val, want[1])
    groups = [k // 2 * 2 if LABELS[k // 2 * 2] == LABELS[k] else k for k in range(len(LABELS))]
    assert len(set(groups)) < len(groups)
    train, val = cda.prepare_group_split(bank, groups)
    want = cda.stratified_group_split(LABELS, groups)
    same(train, want[0]), same(val, want[1])
    assert want != PARENT[(0.2, 42)] and not {groups[k] for k in want[0]} & {groups[k] for k in want[1]}
    same(cda.prepare_group_split(bank, torch.tensor(groups), 0.25, 7)[1], cda.stratified_group_split(LABELS, groups, 0.25, 7)[1])
    # the reference's argument list stays: groups go through a function of their own
    assert list(inspect.signature(cda.prepare_dataset_split).parameters) == ["data_dir_or_bank", "preprocessor", "val_split",
                                                                             "random_state", "device"]


# ------------------------------------------------------------------------------------------------ write_clips
def test_write_clips_round_trips_within_one_pcm_step(tmp_path):
    g = torch.Generator().manual_seed(2)
    clips = [(torch.rand(n, generator=g) - 0.5) * 2.4 for n in (1, 1600, 16000)]          # beyond +-1: clipped
    clips.append(torch.tensor([0.0, 1.0, -1.0, 0.5, -0.25, 1.5, -3.0]))
    bank = cda.DeviceClipBank(clips, [0, 1, 0, 1], device="cpu")
    paths = cda.write_clips(bank, tmp_path, ["a_0", "b_160", "c.wav", "d"], sample_rate=8000)
    assert paths == [str(tmp_path / "non_cough" / "a_0.wav"), str(tmp_path / "cough" / "b_160.wav"),
                     str(tmp_path / "non_cough" / "c.wav"), str(tmp_path / "cough" / "d.wav")]
    for path, x in zip(paths, clips):
        with wave.open(path, "rb") as f:
            assert (f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()) == (1, 2, 8000, x.numel())
            pcm = np.frombuffer(f.readframes(x.numel()), dtype="<i2")
        want = x.numpy().astype(np.float64).clip(-1.0, 1.0)
        assert np.abs(pcm / 32767.0 - want).max() <= 2.0 ** -15
        assert pcm.tolist() == np.rint(want * 32767.0).astype(np.int64).tolist()
    with wave.open(paths[3], "rb") as f:
        assert np.frombuffer(f.readframes(7), dtype="<i2").tolist() == [0, 32767, -32767, 16384, -8192, 32767, -32767]
    with pytest.raises(ValueError, match="write_clips: 4 clips but 1 names"):
        cda.write_clips(bank, tmp_path, ["x"])
    # a bank read back from the directory holds the clips again (non_cough first), within the reader's own scale
    pre = cda.AudioPreprocessor(device="cpu", **SHIPPED)
    cda.write_clips(bank, tmp_path / "again", ["a", "b", "c", "d"], sample_rate=pre.sample_rate)
    back = cda.DeviceClipBank.from_directory(str(tmp_path / "again"), pre, device="cpu")
    assert sorted(back.lengths.tolist()) == sorted(bank.lengths.tolist()) and back.labels.tolist() == [0, 0, 1, 1]


# ------------------------------------------------------------------------------------------------ exports
def test_package_exports():
    for name in ("WindowTable", "find_windows", "slice_bank", "inactive_clips", "write_clips"):
        assert name in cda.__all__ and getattr(cda, name) is getattr(cslices, name), name
    for name in ("stratified_group_split", "prepare_group_split"):
        assert name in cda.__all__ and getattr(cda, name) is getattr(cdata, name), name
    assert len(set(cda.__all__)) == len(cda.__all__) and "slices" not in cda.__all__
    p = inspect.signature(cda.find_windows).parameters
    assert list(p) == ["bank", "preprocessor", "stride", "frame_length", "hop_length", "threshold_db", "floor_db",
                       "min_active", "max_per_clip"]
    assert [p[k].default for k in list(p)[2:]] == [None, 400, 160, -30.0, -60.0, 0.5, None]
    p = inspect.signature(cda.stratified_group_split).parameters
    assert list(p) == ["labels", "groups", "val_split", "random_state"] and (p["val_split"].default, p["random_state"].default) == (0.2, 42)
    assert list(inspect.signature(cda.prepare_group_split).parameters) == ["bank", "groups", "val_split", "random_state"]
