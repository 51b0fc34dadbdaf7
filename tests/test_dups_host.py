"""The duplicate search, without a GPU: the two numpy restatements (tests/dups_ref.py) against each other and against
hand-worked cases, the library's entries in the open tables (``_lib.OPEN`` / ``build.OPEN_UNITS``: this test asks whether
"dups" is in them, never what else is), the C-ABI's argument checks, the Python front (groups, conflicts, the keep rule)
and, on the oracle featuriser, a synthetic corpus with planted copies."""
import ctypes
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest
import torch

import cough_detector_amd as cda
from cough_detector_amd import _lib
from cough_detector_amd import build as cbuild
from cough_detector_amd import duplicates as cdups
import dups_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dups"


# ------------------------------------------------------------------------------------------------ the restatements
def _both(words, L, thr, min_live):
    by_words, by_bits = R.match_words(words, L, thr, min_live), R.match_bits(R.words_to_bits(words), L, thr, min_live)
    assert R.same(by_words, by_bits) is None, R.same(by_words, by_bits)
    for key in ("best_lag", "best_err", "best_bits"):
        assert by_words[key].tolist() == by_bits[key].tolist(), key
    return by_words


def _random_words(rng, n, Tw, density=0.5):
    return (rng.random((n, Tw, 32)) < density).astype(np.uint32) @ (np.uint32(1) << np.arange(32, dtype=np.uint32))


def test_words_and_bits_convert_both_ways():
    w = _random_words(np.random.default_rng(0), 3, 7).astype(np.uint32)
    assert R.bits_to_words(R.words_to_bits(w)).tolist() == w.tolist()
    assert R.popcount(w).tolist() == R.words_to_bits(w).sum(axis=-1).tolist()
    assert R.popcount(np.array([0, 1, 0xFFFFFFFF, 0x80000001], dtype=np.uint32)).tolist() == [0, 1, 32, 2]


@pytest.mark.parametrize("seed,n,Tw,L,min_live", [(1, 6, 9, 3, 1), (2, 5, 12, 0, 4), (3, 4, 5, 8, 2), (4, 7, 20, 2, 16)])
def test_the_two_forms_agree_on_random_words(seed, n, Tw, L, min_live):
    """Random words (unrelated: rates near 0.5), copies at a lag, sparse words with dead frames, a flat row; L >= Tw in
    the third case."""
    rng = np.random.default_rng(seed)
    w = _random_words(rng, n, Tw).astype(np.uint32)
    w[1, 1:] = w[0, :-1]                                         # row 1 is row 0 one frame later
    w[2] = w[0] ^ np.uint32(1 << (seed % 32))                    # one bit per frame away from row 0
    w[3, rng.random(Tw) < 0.5] = 0                               # dead frames
    w[n - 1] = 0                                                 # flat
    for thr in (0, 256, 600, 1024):
        got = _both(w, L, thr, min_live)
        assert got["counts"][n - 1] == 0 and not (got["b"] == n - 1).any()
    assert int(_both(w, L, 1024, 1)["hist"].sum()) == int((R.match_words(w, L, 1024, 1)["best_bits"] > 0).sum())


def test_periodic_rows_tie_between_lags_and_the_earlier_lag_stays():
    a = np.array([1, 2, 1, 2, 1, 2], dtype=np.uint32)
    w = np.stack([a, a[::-1].copy()])                            # b[t] = a[t + 1] = a[t - 1]
    assert R.lag_order(3) == [0, -1, 1, -2, 2, -3, 3] and R.lag_order(0) == [0]
    # lag 0: 6 frames, 2 errors each; lags -1 and +1: 5 frames, no error -- a tie, -1 was there first
    assert R.pair_bits(*R.words_to_bits(w), 0, 1) == (0, 12, 192)
    assert R.pair_bits(*R.words_to_bits(w), 1, 1) == (-1, 0, 160)
    assert R.pair_bits(*R.words_to_bits(w), 5, 1) == (-1, 0, 160)                 # ... and -3 / +3 (3 frames) tie with it too
    got = _both(w, 3, 0, 1)
    assert (got["lag"].tolist(), got["err"].tolist(), got["bits"].tolist()) == ([-1], [0], [160])
    # the rule is a product of integers: 1/64 against 2/128 is a tie, 1/64 against 3/128 is not a replacement, 1/64
    # replaces 3/128
    assert not R.better(2, 128, 1, 64) and not R.better(3, 128, 1, 64) and R.better(1, 64, 3, 128)
    # a later lag that is strictly better does replace: b is a one frame EARLIER (lag -1 is visited before +1; here +1 wins)
    rng = np.random.default_rng(7)
    x = _random_words(rng, 1, 12).astype(np.uint32)[0]
    late = np.concatenate([[np.uint32(5)], x[:-1]])
    got = _both(np.stack([x, late]), 2, 1024, 1)
    assert got["lag"].tolist() == [1] and got["err"].tolist() == [0] and got["bits"].tolist() == [32 * 11]


def test_the_threshold_holds_at_equality_and_fails_one_error_later():
    rng = np.random.default_rng(11)
    a = _random_words(rng, 1, 32).astype(np.uint32)[0] | np.uint32(1 << 31)       # 32 live frames: 1024 bits
    flips = np.uint32(0xFF)                                                         # 8 bits per frame: 256 errors
    at, past = a ^ flips, (a ^ flips)
    past = past.copy()
    past[5] ^= np.uint32(1 << 20)                                                   # 257
    for other, err, hit in ((at, 256, True), (past, 257, False)):
        got = _both(np.stack([a, other]), 0, 256, 16)
        assert got["best_err"][0, 1] == err and got["best_bits"][0, 1] == 1024
        assert got["counts"].tolist() == [int(hit), 0] and len(got["a"]) == int(hit)
        assert got["hist"][(err * 64) // 1024] == 1 and got["hist"].sum() == 1      # counted whether it matches or not
        assert R.matches(err, 1024, 256) is hit
    assert cdups.max_err_1024(0.25) == 256 and cdups.max_err_1024(0.2499) == 255 and cdups.max_err_1024(1.0) == 1024
    assert cdups.max_err_1024(0) == 0
    with pytest.raises(ValueError, match="max_ber"):
        cdups.max_err_1024(1.5)


def test_min_live_counts_frames_where_either_word_is_set():
    a = np.zeros(20, dtype=np.uint32)
    a[:15] = np.arange(1, 16, dtype=np.uint32)
    b = a.copy()
    assert R.pair_bits(*R.words_to_bits(np.stack([a, b])), 0, 16) is None          # 15 live frames
    assert R.pair_bits(*R.words_to_bits(np.stack([a, b])), 0, 15) == (0, 0, 480)
    b[19] = 7                                                                       # a frame is live if EITHER word is set
    assert R.pair_bits(*R.words_to_bits(np.stack([a, b])), 0, 16) == (0, 3, 512)
    assert _both(np.stack([a, b]), 0, 1024, 17)["hist"].sum() == 0                  # no best lag: not in the histogram
    # a lag pushed under min_live by dead frames does not count (the perfect lag +1 has 15 live frames): a worse lag wins
    c = np.zeros(20, dtype=np.uint32)
    c[1:16] = a[:15]                                                                # a one frame later: lag +1 has 15 live frames
    got = _both(np.stack([a, c]), 1, 1024, 16)
    assert got["best_lag"][0, 1] in (0, -1) and got["best_bits"][0, 1] == 32 * 16 and got["best_err"][0, 1] > 0
    got = _both(np.stack([a, c]), 1, 1024, 15)
    assert (got["best_lag"][0, 1], got["best_err"][0, 1], got["best_bits"][0, 1]) == (1, 0, 32 * 15)


@pytest.mark.parametrize("W,D", [(3, 2), (1, 1), (8, 8)])
def test_the_two_fingerprint_forms_agree(W, D):
    rng = np.random.default_rng(W * 10 + D)
    n, F, T = 4, 40, W + D + 5
    images = rng.random((n, F, T)).astype(np.float32)
    images[1] = np.nan                                           # a non-finite clip
    images[2] = rng.random((F, 1)).astype(np.float32)            # constant rows: every difference is 0, never > 0
    images[3] = rng.integers(0, 3, size=(F, T)).astype(np.float32)   # few levels: many differences are exactly 0
    rows = R.default_rows(33)
    words, live = R.fingerprint_words(images, rows, W, D)
    bits = R.fingerprint_bits(images, rows, W, D)
    assert words.shape == (n, T - W + 1 - D) and R.bits_to_words(bits).tolist() == words.tolist()
    assert live.tolist() == (words != 0).sum(axis=1).tolist() and live[1] == 0 and live[2] == 0 and live[0] > 0
    assert R.default_rows(64)[0] == 0 and R.default_rows(64)[32] == 63 and R.default_rows(33) == tuple(range(33))
    assert cdups.default_rows(64) == R.default_rows(64) and cdups.default_rows(40) == R.default_rows(40)
    with pytest.raises(ValueError, match="n_mels=32"):
        cdups.default_rows(32)


# ------------------------------------------------------------------------------------------------ the library
def _header(name):
    return open(os.path.join(ROOT, "include", f"cough_amd_{name}.h")).read()


def _exported(path):
    nm = shutil.which("nm") or os.path.join(os.path.dirname(os.path.realpath(cbuild._hipcc())), "..", "lib", "llvm", "bin", "llvm-nm")
    out = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_the_library_is_in_the_open_tables():
    assert NAME in _lib.OPEN and NAME in cbuild.OPEN_UNITS and NAME in cbuild.OPEN_LIBS
    assert NAME not in _lib.LIBRARIES and NAME not in _lib.LATER and NAME not in cbuild.UNITS and NAME not in cbuild.LATER_UNITS
    assert set(_lib.OPEN) == set(cbuild.OPEN_UNITS) == set(cbuild.OPEN_LIBS)
    assert cbuild.OPEN_UNITS[NAME] == (NAME + ".hip",) and NAME + ".hip" not in cbuild.SOURCES
    for doc in (_lib.__doc__, cbuild.__doc__):
        assert "OPEN" in doc


def test_header_record_and_file_name_the_same_entry_points():
    rec, text = _lib.OPEN[NAME], _header(NAME)
    declared = set(re.findall(r"^(?:int|size_t|const char\*|void) (cough_[a-z_0-9]+)\s*\(", text, flags=re.M))
    assert declared == set(rec.symbols) == set(rec.prototypes), declared ^ set(rec.symbols)
    assert {"cough_fingerprint_images", "cough_match_workspace_bytes", "cough_count_matches", "cough_list_matches"} < declared
    assert rec.symbols[0] == rec.abi_symbol == f"cough_{NAME}_abi_version" and rec.symbols[1] == rec.error_symbol == f"cough_{NAME}_last_error"
    assert os.path.basename(rec.path) == rec.soname == f"libcough_amd_{NAME}.so"
    assert _exported(rec.path) == declared, sorted(_exported(rec.path) ^ declared)
    assert getattr(_lib, f"{NAME.upper()}_SYMBOLS") is rec.symbols and getattr(_lib, f"{NAME.upper()}_LIB_PATH") == rec.path
    assert _lib.load_dups == rec.load and _lib.check_dups == rec.check
    lib = rec.load()
    assert getattr(lib, rec.abi_symbol)() == rec.abi == 1 and f"#define COUGH_{NAME.upper()}_ABI_VERSION 1\n" in text
    assert isinstance(getattr(lib, rec.error_symbol)(), bytes)
    for other in (*_lib.LIBRARIES.values(), *_lib.LATER.values()):
        assert not declared & set(other.symbols), other.name
    for macro, value in (("ROWS", cdups.ROWS), ("MAX_FRAMES", cdups.MAX_FRAMES), ("HIST_BINS", cdups.HIST_BINS),
                         ("MAX_CLIPS", cdups.MAX_CLIPS)):
        assert re.search(rf"#define COUGH_DUPS_{macro} {value}\b", text), macro
    assert cdups.MAX_CLIPS >= 32768 and (R.ROWS, R.HIST_BINS) == (cdups.ROWS, cdups.HIST_BINS)


def test_a_missing_library_is_an_error(monkeypatch):
    rec = _lib.OPEN[NAME]
    monkeypatch.setattr(rec, "handle", None)
    monkeypatch.setattr(rec, "path", os.path.join(ROOT, "no_such_dir", rec.soname))
    with pytest.raises(RuntimeError, match=r"is missing: the HIP extension is not built\. Run `python -m cough_detector_amd\.build`"):
        _lib.load_dups()


def test_the_build_covers_the_library(monkeypatch):
    assert os.path.basename(cbuild.OPEN_LIBS[NAME]) == f"libcough_amd_{NAME}.so" == _lib.OPEN[NAME].soname
    assert os.path.dirname(cbuild.OPEN_LIBS[NAME]) == os.path.dirname(cbuild.LIB) and os.path.exists(cbuild.OPEN_LIBS[NAME])
    own = (NAME + ".hip", f"exports_{NAME}.map")
    for s in own:
        assert os.path.exists(os.path.join(cbuild.CSRC, s)), s
    newer = []
    monkeypatch.setattr(cbuild.os.path, "getmtime", lambda p: 2.0 if os.path.basename(p) in newer else 1.0)
    assert not cbuild.is_stale() and not cbuild.later_stale(NAME)
    for dep in own + (f"cough_amd_{NAME}.h", "common.h", "build.py"):
        newer[:] = [dep]
        assert cbuild.is_stale() and cbuild.later_stale(NAME), dep
    newer[:] = ["slices.hip"]                                    # another library's source: the build is stale, this one is not
    assert cbuild.is_stale() and not cbuild.later_stale(NAME)
    newer[:] = []
    monkeypatch.setitem(cbuild.OPEN_LIBS, NAME, os.path.join(ROOT, "no_such_dir", f"libcough_amd_{NAME}.so"))
    assert cbuild.is_stale() and cbuild.later_stale(NAME)


def test_a_forced_build_links_the_nine_and_an_open_library_only_when_stale(monkeypatch):
    linked = []

    def run(cmd, check=True):
        if "-o" in cmd and "-shared" in cmd:
            linked.append(os.path.basename(cmd[cmd.index("-o") + 1]))
    monkeypatch.setattr(cbuild.subprocess, "run", run)
    monkeypatch.setattr(cbuild, "later_stale", lambda name: False)
    cbuild.build_library(force=True, verbose=False)
    assert len(linked) == 9 and f"libcough_amd_{NAME}.so" not in linked
    linked.clear()
    monkeypatch.setattr(cbuild, "later_stale", lambda name: name == NAME)
    cbuild.build_library(force=True, verbose=False)
    assert len(linked) == 10 and linked[-1] == f"libcough_amd_{NAME}.so"
    linked.clear()
    monkeypatch.setattr(cbuild, "later_stale", lambda name: False)
    cbuild.build_library(force=True, verbose=False, force_later=True)
    assert f"libcough_amd_{NAME}.so" in linked and "libcough_amd_slices.so" in linked


# ------------------------------------------------------------------------------------------------ the C-ABI's checks
FAKE = 1 << 20
ROWS33 = (ctypes.c_int * 33)(*R.default_rows(64))


def _fp_args(**kw):
    a = dict(images=FAKE, n=4, F=90, T=101, rows=ROWS33, window=8, delta=8, words=FAKE, live=FAKE, stream=None)
    a.update(kw)
    return list(a.values())


def _match_args(kind, **kw):
    a = dict(words=FAKE, live=FAKE, n=100, Tw=86, L=8, max_err_1024=256, min_live=16)
    if kind == "count":
        a.update(counts=FAKE, hist=FAKE, ws=FAKE, ws_bytes=1 << 30, stream=None)
    else:
        a.update(ws=FAKE, ws_bytes=1 << 30, row_offs=FAKE, a=FAKE, b=FAKE, lag=FAKE, err=FAKE, bits=FAKE, stream=None)
    a.update(kw)
    return list(a.values())


def _rows_with(k, v):
    rows = list(R.default_rows(64))
    rows[k] = v
    return (ctypes.c_int * 33)(*rows)


@pytest.mark.parametrize("kw,word", [
    (dict(images=None), "NULL"), (dict(rows=None), "NULL"), (dict(words=None), "NULL"), (dict(live=None), "NULL"),
    (dict(n=-1), "n must"), (dict(F=0), "F = 0"), (dict(window=0), "window"), (dict(delta=0), "delta"),
    (dict(T=15), "Tw"), (dict(T=272), "Tw"), (dict(window=94), "Tw"), (dict(rows=_rows_with(32, 90)), "rows[32]"),
    (dict(rows=_rows_with(0, -1)), "rows[0]"), (dict(words=FAKE + 2), "4-byte"), (dict(images=FAKE + 1), "4-byte")])
def test_fingerprint_images_checks_its_arguments_before_the_launch(kw, word):
    lib = _lib.load_dups()
    assert lib.cough_fingerprint_images(*_fp_args(**kw)) == _lib.EINVAL
    msg = lib.cough_dups_last_error().decode()
    assert msg.startswith("cough_fingerprint_images: ") and word in msg, msg
    with pytest.raises(ValueError, match="cough_fingerprint_images"):
        _lib.check_dups(_lib.EINVAL, "cough_fingerprint_images")


COMMON = [(dict(words=None), "NULL"), (dict(live=None), "NULL"), (dict(ws=None), "NULL"), (dict(n=-1), "n = -1"),
          (dict(n=65537), "refused"), (dict(Tw=0), "Tw"), (dict(Tw=257), "Tw"), (dict(L=-1), "lag"),
          (dict(max_err_1024=-1), "max_err_1024"), (dict(max_err_1024=1025), "max_err_1024"), (dict(min_live=0), "min_live"),
          (dict(words=FAKE + 2), "4-byte"), (dict(ws=FAKE + 64), "256-byte")]


@pytest.mark.parametrize("kw,word", COMMON + [(dict(counts=None), "NULL"), (dict(hist=None), "NULL"),
                                              (dict(counts=FAKE + 1), "4-byte"), (dict(hist=FAKE + 4), "8-byte")])
def test_count_matches_checks_its_arguments_before_the_launch(kw, word):
    lib = _lib.load_dups()
    assert lib.cough_count_matches(*_match_args("count", **kw)) == _lib.EINVAL
    msg = lib.cough_dups_last_error().decode()
    assert msg.startswith("cough_count_matches: ") and word in msg, msg


@pytest.mark.parametrize("kw,word", COMMON + [(dict(row_offs=None), "NULL"), (dict(bits=None), "NULL"), (dict(a=None), "NULL"),
                                              (dict(lag=FAKE + 2), "4-byte"), (dict(row_offs=FAKE + 4), "8-byte")])
def test_list_matches_checks_its_arguments_before_the_launch(kw, word):
    lib = _lib.load_dups()
    assert lib.cough_list_matches(*_match_args("list", **kw)) == _lib.EINVAL
    msg = lib.cough_dups_last_error().decode()
    assert msg.startswith("cough_list_matches: ") and word in msg, msg


def test_the_workspace_size_is_stated_and_a_short_one_is_refused():
    lib = _lib.load_dups()
    for n, tiles in ((1, 1), (64, 1), (65, 2), (130, 3), (8192, 128), (65536, 1024)):
        assert lib.cough_match_workspace_bytes(n, 86) == 4 * 64 * tiles * (tiles + 1), n
    for n, tw in ((0, 86), (65537, 86), (10, 0), (10, 257)):
        assert lib.cough_match_workspace_bytes(n, tw) == 0
    need = lib.cough_match_workspace_bytes(100, 86)
    for kind, fn in (("count", lib.cough_count_matches), ("list", lib.cough_list_matches)):
        assert fn(*_match_args(kind, ws_bytes=need - 1)) == _lib.EWORKSPACE
        assert "workspace" in lib.cough_dups_last_error().decode()
    with pytest.raises(RuntimeError, match="status 4"):
        _lib.check_dups(_lib.EWORKSPACE, "cough_count_matches")


def test_no_clips_launch_nothing():
    lib = _lib.load_dups()
    assert lib.cough_fingerprint_images(*_fp_args(n=0)) == _lib.OK
    assert lib.cough_count_matches(*_match_args("count", n=0)) == _lib.OK
    assert lib.cough_list_matches(*_match_args("list", n=0)) == _lib.OK


# ------------------------------------------------------------------------------------------------ the Python front
def _table(pairs, n, err=None, bits=None):
    a = np.array([p[0] for p in pairs], dtype=np.int32)
    b = np.array([p[1] for p in pairs], dtype=np.int32)
    err = np.zeros(len(pairs), np.int32) if err is None else np.array(err, dtype=np.int32)
    bits = np.full(len(pairs), 1024, np.int32) if bits is None else np.array(bits, dtype=np.int32)
    return cda.DuplicateTable(a, b, np.zeros(len(pairs), np.int32), err, bits, np.bincount(a, minlength=n).astype(np.int32),
                              np.zeros(65, np.int64), np.zeros(0, np.int64), n)


def test_duplicate_groups_is_a_union_find_named_by_the_smallest_member():
    t = _table([(1, 4), (2, 3), (3, 7), (4, 6)], 9)
    assert cda.duplicate_groups(t).tolist() == [0, 1, 2, 2, 1, 5, 1, 2, 8]
    assert cda.duplicate_groups(_table([], 4)).tolist() == [0, 1, 2, 3]
    # an existing grouping (pieces of one recording) is merged first: 0 and 5 are pieces of "r0", 8 and 2 of "r7"
    rec = ["r0", "r1", "r7", "r3", "r4", "r0", "r6", "r5", "r7"]
    assert cda.duplicate_groups(t, rec).tolist() == [0, 1, 2, 2, 1, 0, 1, 2, 2]
    assert cda.duplicate_groups(t, torch.tensor([0, 1, 7, 3, 4, 0, 6, 5, 7])).tolist() == [0, 1, 2, 2, 1, 0, 1, 2, 2]
    chain = _table([(5, 6), (4, 5), (3, 4), (0, 3)], 7)          # joined from the far end: the id is still the smallest
    assert cda.duplicate_groups(chain).tolist() == [0, 1, 2, 0, 0, 0, 0]
    with pytest.raises(ValueError, match="duplicate_groups: groups has shape"):
        cda.duplicate_groups(t, [0, 1])
    assert cda.duplicate_groups(t).dtype == np.int64


def test_label_conflicts_orders_by_bit_error_rate():
    t = _table([(0, 1), (0, 2), (1, 3), (2, 3), (4, 5)], 6, err=[100, 50, 10, 50, 0], bits=[1024, 512, 1024, 1024, 64])
    labels = [0, 1, 1, 0, 1, 1]
    rows = cda.label_conflicts(t, labels)                        # (0,1) 0.098, (0,2) 0.098, (1,3) 0.0098, (2,3) 0.049
    assert rows.tolist() == [2, 3, 0, 1] and rows.dtype == np.int64            # the tie keeps the table's order
    assert cda.label_conflicts(t, torch.tensor(labels)).tolist() == [2, 3, 0, 1]
    assert cda.label_conflicts(t, [0] * 6).tolist() == [] and t.ber[1] == 50 / 512 and len(t) == 5
    with pytest.raises(ValueError, match="label_conflicts: labels has shape"):
        cda.label_conflicts(t, [0, 1])


def test_drop_duplicates_keeps_the_first_of_a_group_and_disputed_groups_whole():
    labels = [0, 0, 1, 1, 0, 0, 1, 1, 0]
    clips = [torch.full((5 + k,), float(k)) for k in range(9)]
    bank = cda.DeviceClipBank(clips, labels, device="cpu")
    t = _table([(0, 1), (1, 4), (2, 3), (5, 6)], 9)              # {0,1,4} and {2,3} agree; {5,6} carries both labels
    with pytest.warns(UserWarning, match=r"1 group\(s\) hold copies under both labels and are kept whole: groups \[5\]"):
        kept_bank, kept = cda.drop_duplicates(bank, t)
    assert kept.tolist() == [0, 2, 5, 6, 7, 8] and kept_bank.lengths.tolist() == [5, 7, 10, 11, 12, 13]
    assert kept_bank.labels.tolist() == [0, 1, 0, 1, 1, 0]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        kept_bank, kept = cda.drop_duplicates(bank, _table([(0, 1), (2, 3)], 9))
    assert kept.tolist() == [0, 2, 4, 5, 6, 7, 8]
    with pytest.raises(ValueError, match="drop_duplicates: the bank holds 9 clips, the table compares 4"):
        cda.drop_duplicates(bank, _table([], 4))


def test_the_front_checks_its_parameters_and_needs_the_gpu():
    images = torch.zeros(2, 90, 101)
    for kw, name in ((dict(window=0), "window"), (dict(delta=True), "delta"), (dict(window=1.5), "window")):
        with pytest.raises(ValueError, match=rf"fingerprint_images: {name}"):
            cda.fingerprint_images(images, 64, **kw)
    with pytest.raises(ValueError, match="n_mels=20"):
        cda.fingerprint_images(images, 20)
    with pytest.raises(RuntimeError, match="fingerprint_images: the images live on cpu.*no CPU fallback"):
        cda.fingerprint_images(images, 64)
    with pytest.raises(ValueError, match="must be .n, F, T. float32"):
        cda.fingerprint_images(images[0], 64)
    bank = cda.DeviceClipBank([torch.zeros(100)], [0], device="cpu")

    class Pre:
        n_mels, segment_samples = 32, 16000
    with pytest.raises(ValueError, match="n_mels=32"):
        cda.fingerprint_bank(bank, Pre())
    Pre.n_mels = 64
    with pytest.raises(RuntimeError, match="fingerprint_bank: the bank lives on cpu"):
        cda.fingerprint_bank(bank, Pre())
    fp = cda.Fingerprints(torch.zeros((3, 86), dtype=torch.int32), torch.zeros(3, dtype=torch.int32), 8, 8, R.default_rows(64))
    for kw, name in ((dict(max_lag=-1), "max_lag"), (dict(min_live=0), "min_live"), (dict(max_ber=-0.1), "max_ber"),
                     (dict(max_ber=float("nan")), "max_ber")):
        with pytest.raises(ValueError, match=rf"find_duplicates: {name}"):
            cda.find_duplicates(fp, **kw)
    with pytest.raises(RuntimeError, match="find_duplicates: the fingerprints live on cpu"):
        cda.find_duplicates(fp)
    assert len(fp) == 3


def test_package_exports():
    for name in ("Fingerprints", "DuplicateTable", "fingerprint_images", "fingerprint_bank", "find_duplicates",
                 "duplicate_groups", "label_conflicts", "drop_duplicates"):
        assert name in cda.__all__ and getattr(cda, name) is getattr(cdups, name), name
    assert len(set(cda.__all__)) == len(cda.__all__)
    import inspect
    p = inspect.signature(cda.find_duplicates).parameters
    assert [(k, v.default) for k, v in list(p.items())[1:]] == [("max_lag", 8), ("max_ber", 0.25), ("min_live", 16)]
    p = inspect.signature(cda.fingerprint_images).parameters
    assert [(k, v.default) for k, v in list(p.items())[2:]] == [("window", 8), ("delta", 8), ("rows", None)]
    from cough_detector_amd import audit
    assert "out of scope" not in audit.__doc__ and "duplicates" in audit.__doc__


# ------------------------------------------------------------------------------------------------ the oracle featuriser
def test_planted_copies_lie_below_the_threshold_and_unrelated_clips_above_on_the_oracle():
    """8 base clips, 4 planted copies each (gain x 0.3, delays of 320 and 37 samples, the last 0.2 s cut), featurised by
    the oracle as the loader sees them (peak-normalised).  Every pair within a base clip's family -- the copies among
    each other too -- must read <= 0.22, every pair across families >= 0.35.  Observed: planted at most 0.191 (gain 0.0,
    delay 320 at most 0.004, delay 37 at most 0.140, cut at most 0.111, the rest copy against copy), unrelated at least
    0.428."""
    from oracle import featurizer as ofeat
    clips, group = R.corpus(8)
    n = len(clips)
    images = ofeat.extract_features_batch(torch.from_numpy(np.stack(clips)), normalize_first=True).numpy()
    assert images.shape == (n, 90, 101)
    words, live = R.fingerprint_words(images, R.default_rows(64), 8, 8)
    assert words.shape == (n, 86) and (live >= 16).all()
    m = R.match_words(words, 8, cdups.max_err_1024(0.25), 16)
    upper = np.triu(np.ones((n, n), dtype=bool), k=1)
    assert (m["best_bits"][upper] > 0).all()
    ber = m["best_err"] / np.maximum(m["best_bits"], 1)
    family = group[:, None] == group[None, :]
    planted, unrelated = ber[upper & family], ber[upper & ~family]
    print(f"planted max {planted.max():.4f}  unrelated min {unrelated.min():.4f}")
    assert planted.max() <= 0.22 and unrelated.min() >= 0.35
    for k, kind in enumerate(R.KINDS):
        assert max(ber[b, b + 1 + k] for b in range(0, n, 5)) <= 0.22, kind
    assert ber[0, 1] == 0.0                                      # a gain change is gone after peak normalisation
    # the decisions: exactly the planted families
    t = cda.DuplicateTable(m["a"], m["b"], m["lag"], m["err"], m["bits"], m["counts"], m["hist"], np.zeros(0, np.int64), n)
    assert cda.duplicate_groups(t).tolist() == group.tolist() and len(t) == 8 * 10
    assert m["hist"].sum() == n * (n - 1) // 2 and m["hist"][:16].sum() == 80 and m["hist"][16:22].sum() == 0
