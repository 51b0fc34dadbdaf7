"""The duplicate search on the MI355X: the fingerprint kernel against tests/dups_ref.py on the device's own images, the
matcher against it on random words with planted copies (integers and bits: equal, no tolerance), every entry point
between guard zones, and the whole chain on a synthetic corpus with planted copies, where decisions are compared, not
bits (the device's images differ from the oracle's in the last places)."""
import ctypes
import functools
import warnings

import numpy as np
import pytest
import torch

import cough_detector_amd as cda
from cough_detector_amd import _lib
from cough_detector_amd import duplicates as cdups
from cough_detector_amd.data import _featurise_rows, _stream
import dups_ref as R
import guarded as G

pytestmark = pytest.mark.gpu

SHIPPED = dict(use_pcen=False, use_pre_emphasis=False, use_delta_delta=False, use_spectral_contrast=False)
I32 = dict(dtype=torch.int32, device="cuda")


def _as_u32(t):
    return t.cpu().numpy().view(np.uint32)


def _dev_words(words):
    return torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint32).view(np.int32)).cuda()


# ------------------------------------------------------------------------------------------------ the fingerprint
@pytest.fixture(scope="module")
def pre():
    return cda.AudioPreprocessor(device="cuda", **SHIPPED)


def _check_fingerprint(images, n_mels, W, D, rows=None):
    fp = cda.fingerprint_images(images, n_mels, window=W, delta=D, rows=rows)
    want_words, want_live = R.fingerprint_words(images.cpu().numpy(), fp.rows, W, D)
    assert fp.rows == (R.default_rows(n_mels) if rows is None else tuple(rows)) and (fp.window, fp.delta) == (W, D)
    assert fp.words.dtype == torch.int32 and tuple(fp.words.shape) == want_words.shape
    assert _as_u32(fp.words).tolist() == want_words.tolist()
    assert fp.live.cpu().tolist() == want_live.tolist()
    return fp, want_words


def test_fingerprint_of_the_devices_own_images_equals_the_restatement(pre):
    """(n 5, F 90, T 101, W 8, D 8) through the loader's path: a burst clip, a silent clip, a clip with a NaN, a clip whose
    lower mel rows are made constant in the image, and a clip shorter than a second (zero-padded by cough_prepare_rows).
    The flat clips are exactly the silent and the NaN clip."""
    clips = [R.base_clip(0), np.zeros(R.SR, np.float32), R.base_clip(1), R.base_clip(2), R.base_clip(3)[:6000]]
    clips[2] = clips[2].copy()
    clips[2][777] = np.nan
    bank = cda.DeviceClipBank([torch.from_numpy(c) for c in clips], [0, 0, 1, 1, 0])
    images = _featurise_rows(pre, bank.device, bank.data, bank.offsets_dev, bank.lengths_dev)
    assert tuple(images.shape) == (5, 90, 101)
    images[3, :30, :] = images[3, :30, :1].clone()                       # constant rows: their differences never change
    fp, words = _check_fingerprint(images, pre.n_mels, 8, 8)
    assert words.shape == (5, 86)
    live = fp.live.cpu().tolist()
    assert [k for k in range(5) if live[k] == 0] == [1, 2]
    assert live[0] == 86 and 0 < live[4] and 0 < live[3]
    assert (words[3] & np.uint32((1 << 15) - 1) == 0).all()      # rows 0..29 feed the first 15 row pairs
    # the same through fingerprint_bank, in batches that do not divide the bank
    whole = cda.fingerprint_bank(bank, pre, batch_size=2)
    keep = [0, 1, 2, 4]                                          # image 3 was edited above
    assert _as_u32(whole.words)[keep].tolist() == words[keep].tolist() and len(whole) == 5
    assert whole.live.cpu()[keep].tolist() == [live[k] for k in keep]


@pytest.mark.parametrize("n,F,T,n_mels,W,D", [(4, 40, 30, 33, 8, 8), (3, 90, 16, 64, 8, 8), (3, 50, 20, 40, 1, 1),
                                              (3, 64, 271, 64, 8, 8), (70, 33, 12, 33, 3, 2)])
def test_fingerprint_of_random_images_equals_the_restatement(n, F, T, n_mels, W, D):
    """F 40 with 33 mel rows; T = W + D, where Tw = 1; W = D = 1; Tw = 256, the largest; more clips than a wave.  The
    images hold few levels, so sums tie exactly and `> 0` is asked at 0; one image is constant (flat), one NaN."""
    g = torch.Generator().manual_seed(n * 1000 + T)
    images = (torch.randint(0, 4, (n, F, T), generator=g).float() / 4.0 + torch.rand((n, F, T), generator=g) * (torch.rand((n, 1, 1), generator=g) < 0.5)).cuda()
    images[0] = 0.25
    images[1] = float("nan")
    fp, words = _check_fingerprint(images, n_mels, W, D)
    assert words.shape == (n, T - W + 1 - D) and fp.live.cpu()[:2].tolist() == [0, 0] and int(fp.live[2]) > 0
    rows = list(range(F - 33, F))[::-1]                          # rows of the caller's choosing, descending
    _check_fingerprint(images, n_mels, W, D, rows=rows)


def test_fingerprint_refuses_what_the_header_refuses():
    images = torch.zeros((2, 40, 15), device="cuda")
    with pytest.raises(ValueError, match=r"T - window \+ 1 - delta = 0"):
        cda.fingerprint_images(images, 33)
    with pytest.raises(ValueError, match="= 257 must lie in 1..256"):
        cda.fingerprint_images(torch.zeros((1, 40, 272), device="cuda"), 33)
    with pytest.raises(ValueError, match="rows must be 33 image rows"):
        cda.fingerprint_images(images, 33, window=2, delta=2, rows=list(range(8, 41)))
    empty = cda.fingerprint_images(images[:0], 33, window=2, delta=2)
    assert tuple(empty.words.shape) == (0, 12) and len(cda.find_duplicates(empty)) == 0


# ------------------------------------------------------------------------------------------------ the matcher
def _shifted(rng, row, lag):
    """b with b[t + lag] = row[t]: ``row`` met at ``lag``; the frames that fall in are random."""
    Tw = len(row)
    out = _rand_words(rng, 1, Tw)[0]
    if abs(lag) < Tw:
        if lag >= 0:
            out[lag:] = row[:Tw - lag]
        else:
            out[:Tw + lag] = row[-lag:]
    return out


def _rand_words(rng, n, Tw):
    return rng.integers(0, 2**32, size=(n, Tw), dtype=np.uint64).astype(np.uint32)


def _flip(rng, row, count, keep_bit=31):
    """``row`` with exactly ``count`` bits flipped, none of them bit ``keep_bit``."""
    out = row.copy()
    places = [(t, k) for t in range(len(row)) for k in range(32) if k != keep_bit]
    for j in rng.choice(len(places), size=count, replace=False):
        out[places[j][0]] ^= np.uint32(1 << places[j][1])
    return out


@functools.lru_cache(maxsize=None)
def _case(n, Tw, L, thr, min_live):
    """Random words and what is planted in them, as far as ``n`` reaches (rows by index), with the reference result:
    0        a base row with bit 31 set in every frame (every frame live whatever it meets)
    1, 2     row 0 at lags +L and -L (found)             3, 4   at lags +(L+1) and -(L+1) (not found within L)
    5, 6     row 0 with floor(thr * bits / 1024) flipped bits (on the threshold) and one more (past it)
    7, 8     a sparse row with min_live - 1 live frames and its copy (no lag with min_live live frames at lag 0)
    9, 10    period-2 rows that meet at -1 and at +1 alike     11   a flat row     12   a row with half its frames dead"""
    rng = np.random.default_rng(n * 7919 + Tw * 31 + L)
    w = _rand_words(rng, n, Tw)
    w[0] |= np.uint32(1 << 31)
    planted = {}
    for row, lag in ((1, L), (2, -L), (3, L + 1), (4, -(L + 1))):
        if row < n:
            w[row] = _shifted(rng, w[0], lag)
            planted[row] = lag
    on = (thr * 32 * Tw) // 1024
    if n > 6 and on + 1 <= 31 * Tw:
        w[5], w[6] = _flip(rng, w[0], on), _flip(rng, w[0], on + 1)
    if n > 8 and 2 <= min_live <= Tw:
        w[7] = 0
        w[7, rng.choice(Tw, size=min_live - 1, replace=False)] = _rand_words(rng, 1, min_live - 1)[0] | np.uint32(1)
        w[8] = w[7]
    if n > 10:
        x, y = _rand_words(rng, 1, 2)[0] | np.uint32(2)
        w[9, 0::2], w[9, 1::2] = x, y
        w[10, 0::2], w[10, 1::2] = y, x
    if n > 11:
        w[11] = 0
    if n > 12:
        w[12, rng.random(Tw) < 0.5] = 0
    return w, planted, R.match_words(w, L, thr, min_live)


def _run(words, n, Tw, L, thr, min_live, live=None, out=None, rows_out=None, ws=None):
    """Both passes through the C ABI.  ``out``: counts / hist tensors to write into; ``rows_out(rows)``: the five list
    tensors; ``ws``: (pointer, bytes).  Returns name -> tensor."""
    lib = _lib.load_dups()
    dev = _dev_words(words) if isinstance(words, np.ndarray) else words
    if live is None:
        live = (dev != 0).sum(dim=1).to(torch.int32)
    need = lib.cough_match_workspace_bytes(n, Tw)
    if ws is None:
        keep = torch.empty(need // 4, **I32)
        ws = (keep.data_ptr(), need)
    out = out or dict(counts=torch.empty(n, **I32), hist=torch.empty(65, dtype=torch.int64, device="cuda"))
    head = (dev.data_ptr(), live.data_ptr(), n, Tw, L, thr, min_live)
    s = _stream(torch.device("cuda"))
    _lib.check_dups(lib.cough_count_matches(*head, out["counts"].data_ptr(), out["hist"].data_ptr(), ws[0], ws[1], s),
                    "cough_count_matches")
    counts = out["counts"].cpu().numpy()
    offs = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)])
    rows = int(offs[-1])
    lst = rows_out(rows) if rows_out else {k: torch.empty(rows, **I32) for k in ("a", "b", "lag", "err", "bits")}
    if rows:
        offs_dev = torch.from_numpy(offs).cuda()
        _lib.check_dups(lib.cough_list_matches(*head, ws[0], ws[1], offs_dev.data_ptr(),
                                               *(lst[k].data_ptr() for k in ("a", "b", "lag", "err", "bits")), s),
                        "cough_list_matches")
    torch.cuda.synchronize()
    return {**out, **lst}


def _want(ref):
    return {k: torch.from_numpy(np.ascontiguousarray(ref[k])) for k in R.KEYS}


def _equal(got, ref, what=""):
    for key in R.KEYS:
        assert got[key].cpu().tolist() == ref[key].tolist(), (what, key)


CASES = [(1, 86, 8, 256, 16), (2, 86, 8, 256, 16), (63, 31, 3, 256, 16), (64, 86, 8, 256, 16), (65, 86, 0, 256, 16),
         (130, 86, 8, 256, 16), (130, 1, 0, 256, 1), (65, 1, 3, 300, 1), (64, 31, 40, 256, 8), (66, 256, 8, 256, 16),
         (70, 256, 3, 100, 200), (129, 86, 3, 1024, 16), (67, 33, 8, 0, 1), (65, 86, 8, 256, 87)]


@pytest.mark.parametrize("n,Tw,L,thr,min_live", CASES)
def test_matcher_equals_the_restatement_exactly(n, Tw, L, thr, min_live):
    """Clips around the tile edge of 64, Tw 1 / 31 / 86 / 256, L 0 / 3 / 8 and L >= Tw; thr = 1024 makes row 0 match
    every row that is not flat (a full count); thr = 0 only exact copies; min_live above Tw: nothing has a best lag."""
    w, planted, ref = _case(n, Tw, L, thr, min_live)
    got = _run(w, n, Tw, L, thr, min_live)
    _equal(got, ref, "first run")
    a, b = got["a"].cpu().numpy().astype(np.int64), got["b"].cpu().numpy().astype(np.int64)
    assert (a < b).all() and (np.diff(a * n + b) > 0).all()      # sorted by (a, b), no pair twice
    again = _run(w, n, Tw, L, thr, min_live)
    for key in R.KEYS:
        assert torch.equal(got[key], again[key]), key            # the same bytes
    # what was planted, said out loud (the reference agrees by the lines above)
    pairs = {(int(x), int(y)): (int(l), int(e)) for x, y, l, e in zip(a, b, got["lag"].cpu(), got["err"].cpu())}
    if thr == 256 and min_live <= Tw - L and L + 1 < Tw:
        for row, lag in planted.items():
            assert ((0, row) in pairs) == (abs(lag) <= L), (row, lag)
            if abs(lag) <= L and L > 0:
                assert pairs[(0, row)] == (lag, 0)
        if n > 6 and Tw >= 16:
            assert (0, 5) in pairs and (0, 6) not in pairs and pairs[(0, 5)] == (0, (thr * 32 * Tw) // 1024)
        if n > 8:
            assert (7, 8) not in pairs
        if n > 10 and L >= 1 and Tw >= 20:
            assert pairs[(9, 10)] == (-1, 0)
    if n > 11:
        assert int(got["counts"][11]) == 0 and 11 not in b
    if thr == 1024:
        alive = int((np.asarray(w != 0).sum(axis=1) > 0).sum())
        assert int(got["counts"][0]) == alive - 1 and len(a) == int(got["hist"].sum()) > alive
    if min_live > Tw:
        assert len(a) == 0 and int(got["hist"].sum()) == 0


def test_a_pair_reads_the_same_alone_and_inside_a_batch():
    n, Tw, L, thr, min_live = 130, 86, 8, 1024, 16
    w, _, ref = _case(n, Tw, L, thr, min_live)
    for x, y in ((0, 1), (5, 70), (63, 64), (9, 10), (12, 129), (7, 8), (11, 40)):
        alone = _run(np.stack([w[x], w[y]]), 2, Tw, L, thr, min_live)
        have = ref["best_bits"][x, y] > 0
        assert alone["counts"].cpu().tolist() == [int(have), 0]
        if have:
            assert [int(alone[k][0]) for k in ("lag", "err", "bits")] == [ref["best_lag"][x, y], ref["best_err"][x, y],
                                                                         ref["best_bits"][x, y]], (x, y)


def test_find_duplicates_is_the_two_passes(monkeypatch):
    n, Tw, L, thr, min_live = 130, 86, 8, 256, 16
    w, _, ref = _case(n, Tw, L, thr, min_live)
    dev = _dev_words(w)
    fp = cda.Fingerprints(dev, (dev != 0).sum(dim=1).to(torch.int32), 8, 8, R.default_rows(64))
    t = cda.find_duplicates(fp)
    for key, field in (("a", t.a), ("b", t.b), ("lag", t.lag), ("err", t.errors), ("bits", t.bits), ("counts", t.counts),
                       ("hist", t.histogram)):
        assert field.tolist() == ref[key].tolist(), key
    assert t.n == n and t.flat.tolist() == [11] and t.histogram.dtype == np.int64 and len(t) == len(ref["a"])
    assert np.array_equal(t.ber, ref["err"] / ref["bits"])
    none = cda.find_duplicates(fp, max_ber=0.0, min_live=87)
    assert len(none) == 0 and none.counts.tolist() == [0] * n and none.histogram.sum() == 0
    monkeypatch.setattr(cdups, "MAX_CLIPS", 100)
    with pytest.raises(ValueError, match="find_duplicates: 130 clips; the matcher takes at most 100"):
        cda.find_duplicates(fp)


def test_entry_points_between_guard_zones_at_the_promised_sizes():
    """Words flush against a guard (as floats: a load past the end would read the guard word, a live frame), every output
    of exact size at a 4-byte phase (8 for the int64 histogram), the workspace at exactly cough_match_workspace_bytes
    under the three fills; `stale` holds what a call on other words and another threshold left."""
    n, Tw, L, thr, min_live = 130, 86, 8, 256, 16
    w, _, ref = _case(n, Tw, L, thr, min_live)
    other, _, other_ref = _case(n, Tw, 3, 1024, 16)
    lib = _lib.load_dups()
    need = lib.cough_match_workspace_bytes(n, Tw)
    assert need == 4 * 192 * 4
    words = G.Guarded.holding(torch.from_numpy(w.view(np.float32).copy()).cuda(), align=16, phase=4, name="d_words")
    words_view = words.view(torch.int32, n, Tw)
    live = (words_view != 0).sum(dim=1).to(torch.int32)
    rows = len(ref["a"])
    assert rows > 5 and len(other_ref["a"]) > rows

    def stale(ws):
        return G.run_other(ws, need, lambda ptr, nbytes: _run(other, n, Tw, 3, 1024, 16, ws=(ptr, nbytes)))
    for fill, ws, more in G.workspaces(need, stale):
        out = dict(counts=G.output(n, torch.int32, align=16, phase=4, name="d_counts"),
                   hist=G.output(65, torch.int64, align=16, phase=8, name="d_hist"))
        lst = {k: G.output(rows, torch.int32, align=16, phase=4 * (j % 3 + 1), name=f"d_{k}")
               for j, k in enumerate(("a", "b", "lag", "err", "bits"))}
        for g in (*out.values(), *lst.values()):
            g.fill("ones_bits" if fill == "stale" else fill)
        views = dict(counts=out["counts"].int32, hist=out["hist"].int64)
        got = _run(words_view, n, Tw, L, thr, min_live, live=live, out=views, rows_out=lambda r: {k: g.int32 for k, g in lst.items()},
                   ws=(ws.ptr, need))
        G.check([words, ws, *more, *out.values(), *lst.values()], got, _want(ref), f"fill {fill}")

    # the fingerprint: the images flush against a guard, words and live of exact size
    g = torch.Generator().manual_seed(5)
    images = torch.rand((5, 40, 30), generator=g)
    want_words, want_live = R.fingerprint_words(images.numpy(), R.default_rows(40), 8, 8)
    held = G.Guarded.holding(images.cuda(), align=16, phase=4, name="d_images")
    d_words, d_live = G.output((5, 15), torch.int32, align=16, phase=12, name="d_words"), G.output(5, torch.int32, align=16, phase=4, name="d_live")
    rows33 = (ctypes.c_int * 33)(*R.default_rows(40))
    _lib.check_dups(lib.cough_fingerprint_images(held.ptr, 5, 40, 30, rows33, 8, 8, d_words.ptr, d_live.ptr,
                                                 _stream(torch.device("cuda"))), "cough_fingerprint_images")
    torch.cuda.synchronize()
    G.check([held, d_words, d_live], dict(words=d_words.view(torch.int32, 5, 15), live=d_live.int32),
            dict(words=torch.from_numpy(want_words.view(np.int32)), live=torch.from_numpy(want_live)), "fingerprint")


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def corpus():
    clips, group = R.corpus(8)
    labels = [int(g // 5 % 2) for g in group]
    clips.append(clips[0].copy())                                # the same clip once more, under the other label
    labels.append(1 - labels[0])
    return clips, np.append(group, 0), labels


def test_planted_copies_become_groups_and_the_mislabel_is_named(corpus, pre):
    clips, group, labels = corpus
    n = len(clips)
    bank = cda.DeviceClipBank([torch.from_numpy(c) for c in clips], labels)
    fp = cda.fingerprint_bank(bank, pre, batch_size=16)
    assert tuple(fp.words.shape) == (n, 86)
    table = cda.find_duplicates(fp)
    assert table.n == n and table.flat.size == 0 and table.histogram.sum() == n * (n - 1) // 2
    got = cda.duplicate_groups(table)
    assert got.tolist() == group.tolist()                        # exactly the planted families, named by their first clip
    assert len(table) == 7 * 10 + 15 and (table.ber <= 0.25).all()
    assert table.histogram[:17].sum() == len(table) and table.histogram[17:22].sum() == 0      # a gap between copies and the bulk
    conflicts = cda.label_conflicts(table, bank.labels)
    assert sorted(zip(table.a[conflicts].tolist(), table.b[conflicts].tolist())) == [(k, n - 1) for k in range(5)]
    assert (int(table.a[conflicts[0]]), int(table.b[conflicts[0]])) == (0, n - 1) and table.errors[conflicts[0]] == 0
    with pytest.warns(UserWarning, match=r"kept whole: groups \[0\]"):
        kept_bank, kept = cda.drop_duplicates(bank, table)
    assert kept.tolist() == [0, 1, 2, 3, 4] + list(range(5, 40, 5)) + [n - 1] and len(kept_bank) == 13
    with pytest.raises(ValueError, match="group 0 holds clips of different labels"):
        cda.prepare_group_split(bank, got)
    # the listener decides: the last clip takes its family's label; then a group never lies on both sides
    fixed = labels[:-1] + [labels[0]]
    bank = cda.DeviceClipBank([torch.from_numpy(c) for c in clips], fixed)
    assert cda.label_conflicts(table, fixed).size == 0
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        kept_bank, kept = cda.drop_duplicates(bank, table)
    assert kept.tolist() == list(range(0, 40, 5)) and kept_bank.labels.tolist() == [0, 1] * 4     # one clip per group
    for split, seed in ((0.25, 42), (0.5, 3)):
        train_idx, val_idx = cda.stratified_group_split(fixed, got, split, seed)
        assert sorted(train_idx + val_idx) == list(range(n)) and val_idx
        assert not {int(got[k]) for k in train_idx} & {int(got[k]) for k in val_idx}
        train, val = cda.prepare_group_split(bank, got, split, seed)
        assert train.labels.tolist() == [fixed[k] for k in train_idx] and val.labels.tolist() == [fixed[k] for k in val_idx]
    # recordings cut into pieces pull together: families 1 and 2 as pieces of one recording
    pieces = [1 if g in (5, 10) else 100 + k for k, g in enumerate(group)]
    merged = cda.duplicate_groups(table, pieces)
    assert merged.tolist() == [5 if g == 10 else int(g) for g in group]


def test_command_line_names_the_conflict_and_the_groups(corpus, tmp_path, capsys):
    import json
    clips, group, labels = corpus
    keep = [0, 1, 5, 6, 10, 40]                                  # two families of two, a single clip, the mislabelled copy
    bank = cda.DeviceClipBank([torch.from_numpy(clips[k]) for k in keep], [labels[k] for k in keep], device="cpu")
    cda.write_clips(bank, tmp_path, [f"clip{k:02d}" for k in keep])
    report = cdups.main([str(tmp_path), "--top", "5"])
    lines = capsys.readouterr().out.strip().splitlines()
    assert json.loads(lines[-1]) == report
    assert (report["n"], report["pairs"], report["groups"], report["largest"], report["flat"]) == (6, 4, 2, 3, 0)
    assert report["conflicts"] == 2 and len(report["histogram"]) == 65 and sum(report["histogram"]) == 15
    assert lines[0].startswith("conflict  ber 0.000") and "clip40.wav" in lines[0]
    assert lines[2].startswith("group of 3: ") and lines[3].startswith("group of 2: ")
