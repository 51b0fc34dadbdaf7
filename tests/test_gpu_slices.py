"""Slicing recordings into active clips on the MI355X (cough_detector_amd/slices.py, csrc/slices.hip) against
tests/slices_ref.py.

The kernels decide from float64 energies by single comparisons, single products and integer counts.  The reference is
fed the DEVICE's own energies (read back once), so both sides compare the same float64 values with the same operations:
``d_active``, ``d_keep``, ``d_counts``, ``d_clip_active`` and the listed rows must be equal as integers, ``d_peak`` as
bits (NaN matched by ``isnan``).  No tolerance anywhere; extraction moves float32 samples, bit for bit.
"""
import numpy as np
import pytest
import torch

import cough_detector_amd as cda
from cough_detector_amd import _lib
from cough_detector_amd.data import _stream
import guarded as G
import slices_ref as R

pytestmark = pytest.mark.gpu
SHIPPED = dict(use_pcen=False, use_pre_emphasis=False, use_delta_delta=False, use_spectral_contrast=False)
SEG = 16000
STRIDES = (16000, 8000, 5000, 24000)
SHARES = (0.0, 0.5, 1.0)
CAPS = (None, 1, 3)
NO_CAP = 2**31 - 1


class Small:
    """What find_windows reads of a preprocessor, at the small geometry."""
    segment_samples, sample_rate = 32, 16000


@pytest.fixture(scope="module")
def pre():
    return cda.AudioPreprocessor(device="cuda", **SHIPPED)


# ------------------------------------------------------------------------------------------------ the clips
def _noise(rng, n, amplitude=0.3):
    return (amplitude * rng.standard_normal(n)).astype(np.float32)


def _bursts(rng, n):
    """Noise bursts of 0.05..1.5 s between stretches of exact zeros, each burst at a level of its own."""
    x, pos = np.zeros(n, dtype=np.float32), int(rng.integers(0, 4000))
    while pos < n:
        length = int(rng.integers(800, 24000))
        x[pos:pos + length] = _noise(rng, min(length, n - pos), float(rng.choice([0.02, 0.1, 0.4])))
        pos += length + int(rng.integers(800, 30000))
    return x


def _click(rng, n):
    x = np.zeros(n, dtype=np.float32)
    x[n // 2] = 0.9
    return x


def _spoilt(value):
    def make(rng, n):
        x = _noise(rng, n)
        x[(2 * n) // 3] = value
        return x
    return make


def _levels(rng, n):
    """Blocks of 4 samples at one of three levels, the sign at random."""
    level = np.repeat(rng.choice([0.0, 0.02, 0.5], size=(n + 3) // 4), 4)[:n]
    return (level * np.sign(rng.standard_normal(n))).astype(np.float32)


KINDS = {"noise": _noise, "levels": _levels, "bursts": _bursts, "constant": lambda rng, n: np.full(n, 0.25, dtype=np.float32),
         "silent": lambda rng, n: np.zeros(n, dtype=np.float32), "click": _click,
         "quiet": lambda rng, n: (3.1e-4 * np.sign(rng.standard_normal(n))).astype(np.float32),      # -70 dB throughout
         "nan": _spoilt(np.nan), "pinf": _spoilt(np.inf), "ninf": _spoilt(-np.inf)}
RAGGED = [(1, "noise"), (399, "noise"), (400, "constant"), (15999, "bursts"), (16000, "noise"), (16001, "bursts")]
RAGGED += [(SEG + s - 1 + d, kind) for s in STRIDES for d, kind in ((0, "bursts"), (1, "noise"))]
RAGGED += [(32000, "silent"), (40000, "click"), (48000, "constant"), (64000, "quiet"), (80000, "nan"), (56000, "pinf"),
           (100000, "ninf"), (37000, "bursts"), (52345, "bursts"), (73210, "noise"), (96000, "bursts"), (123456, "bursts"),
           (160000, "bursts"), (16000, "silent"), (16000, "click"), (24001, "constant"), (44100, "bursts"), (88200, "bursts"),
           (131072, "bursts"), (33333, "noise"), (20000, "noise"), (28000, "bursts"), (150000, "bursts"), (200000, "bursts"),
           (700000, "bursts"), (65537, "bursts")]


def _bank(spec, seed):
    rng = np.random.default_rng(seed)
    clips = [KINDS[kind](rng, n) for n, kind in spec]
    labels = [k % 2 for k in range(len(clips))]
    return clips, labels, cda.DeviceClipBank(clips, labels, device="cuda")


class Corpus:
    def __init__(self, spec, seed, frame_length, hop_length):
        self.spec, self.frame_length, self.hop_length = spec, frame_length, hop_length
        self.kinds = [kind for _, kind in spec]
        self.clips, self.labels, self.bank = _bank(spec, seed)
        self.lengths = [n for n, _ in spec]
        energy, offsets = cda.frame_energy(self.bank, frame_length=frame_length, hop_length=hop_length)
        self.energy_dev, self.frame_offsets = energy, offsets.numpy()
        host = energy.cpu().numpy()                                   # the one read of the device's energies
        self.energies = [host[a:b] for a, b in zip(self.frame_offsets[:-1], self.frame_offsets[1:])]
        self.frame_offsets_dev = offsets.cuda()

    def ref(self, seg_len, stride, min_active, cap, **kw):
        return R.table_ref(self.energies, self.lengths, seg_len, stride, self.frame_length, self.hop_length,
                           min_active=min_active, cap=cap, **kw)


@pytest.fixture(scope="module")
def ragged():
    c = Corpus(RAGGED, 11, 400, 160)
    assert 38 <= len(c.clips) <= 45 and {200000, 700000, 1, 399, 400, 15999, 16000, 16001} <= set(c.lengths)
    for s in STRIDES:
        assert {SEG + s - 1, SEG + s} <= set(c.lengths)
    return c


@pytest.fixture(scope="module")
def small():
    """Every length 1..200 at frame 8 / hop 4 / window 32: blocks of 4 samples at one of three levels."""
    return Corpus([(n, "levels") for n in range(1, 201)], 4, 8, 4)


# ------------------------------------------------------------------------------------------------ the kernels, directly
def _want(ref):
    peak = torch.tensor(ref["peak"], dtype=torch.float64)
    return dict(active=torch.tensor(ref["active"], dtype=torch.int32), keep=torch.tensor(ref["keep"], dtype=torch.int32),
                counts=torch.tensor(ref["counts"], dtype=torch.int32), clip_active=torch.tensor(ref["clip_active"], dtype=torch.int32),
                peak=torch.nan_to_num(peak, nan=-1.0), peak_nan=torch.isnan(peak).to(torch.int32)), \
        dict(clip=torch.tensor(ref["clip"], dtype=torch.int64), start=torch.tensor(ref["start"], dtype=torch.int32),
             length=torch.tensor(ref["length"], dtype=torch.int32), row_active=torch.tensor(ref["row_active"], dtype=torch.int32))


def _run(c, seg_len, stride, min_active, cap, levels=None, out=None, rows_out=None, energy_ptr=None):
    """Both kernels on ``c``'s energies.  ``out`` / ``rows_out``: name -> tensor to write into (guarded regions);
    otherwise fresh tensors.  -> (per-window and per-clip outputs, rows), peak split into value and isnan."""
    lib, bank, n = _lib.load_slices(), c.bank, len(c.bank)
    ratio, floor = levels or R.levels()
    per_clip = np.array([R.n_windows(v, seg_len, stride) for v in c.lengths], dtype=np.int64)
    woffs = torch.from_numpy(np.concatenate([[0], np.cumsum(per_clip)]).astype(np.int64)).cuda()
    total = int(per_clip.sum())
    i32 = dict(dtype=torch.int32, device="cuda")
    o = out or dict(peak=torch.empty(n, dtype=torch.float64, device="cuda"), clip_active=torch.empty(n, **i32),
                    active=torch.empty(total, **i32), keep=torch.empty(total, **i32), counts=torch.empty(n, **i32))
    assert o["active"].numel() == o["keep"].numel() == total and o["peak"].numel() == n
    _lib.check_slices(lib.cough_window_activity(
        energy_ptr or c.energy_dev.data_ptr(), c.frame_offsets_dev.data_ptr(), bank.lengths_dev.data_ptr(), woffs.data_ptr(),
        n, c.frame_length, c.hop_length, seg_len, stride, NO_CAP if cap is None else cap, ratio, floor, float(min_active),
        o["peak"].data_ptr(), o["clip_active"].data_ptr(), o["active"].data_ptr(), o["keep"].data_ptr(),
        o["counts"].data_ptr(), _stream(bank.device)), "cough_window_activity")
    counts = o["counts"].cpu().numpy().astype(np.int64)
    roffs = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)).cuda()
    rows = int(counts.sum())
    r = rows_out(rows) if rows_out else dict(clip=torch.empty(rows, dtype=torch.int64, device="cuda"), start=torch.empty(rows, **i32),
                                             length=torch.empty(rows, **i32), row_active=torch.empty(rows, **i32))
    _lib.check_slices(lib.cough_list_windows(
        o["keep"].data_ptr(), o["active"].data_ptr(), bank.lengths_dev.data_ptr(), woffs.data_ptr(), roffs.data_ptr(), n,
        seg_len, stride, r["clip"].data_ptr(), r["start"].data_ptr(), r["length"].data_ptr(), r["row_active"].data_ptr(),
        _stream(bank.device)), "cough_list_windows")
    got = {k: v for k, v in o.items() if k != "peak"}
    got["peak"], got["peak_nan"] = torch.nan_to_num(o["peak"], nan=-1.0), torch.isnan(o["peak"]).to(torch.int32)
    return got, r


def _equal(got, want, what):
    assert set(got) == set(want)
    for k in got:
        a, b = got[k].cpu(), want[k]
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k, a.dtype, a.shape, b.shape)
        if not torch.equal(a, b):
            bad = torch.nonzero(a != b).flatten()
            raise AssertionError(f"{what}: {k} differs in {bad.numel()} of {a.numel()}, first at {int(bad[0])}: "
                                 f"{a[bad[0]].item()!r} against {b[bad[0]].item()!r}")


def _sweep(c, seg_len, stride, shares=SHARES, caps=CAPS, levels_db=None):
    kept = capped = 0
    kw = {} if levels_db is None else dict(threshold_db=levels_db[0], floor_db=levels_db[1])
    for min_active in shares:
        for cap in caps:
            ref = c.ref(seg_len, stride, min_active, cap, **kw)
            want, want_rows = _want(ref)
            got, rows = _run(c, seg_len, stride, min_active, cap, levels=None if levels_db is None else R.levels(*levels_db))
            what = f"stride {stride}, min_active {min_active}, cap {cap}"
            _equal(got, want, what)
            _equal(rows, want_rows, what)
            kept += len(ref["clip"])
            if cap is not None:
                full = c.ref(seg_len, stride, min_active, None, **kw)
                capped += sum(1 for a in full["counts"] if a > cap)
    return kept, capped


@pytest.mark.parametrize("stride", STRIDES)
def test_kernels_equal_the_restatement_exactly(ragged, stride):
    kept, capped = _sweep(ragged, SEG, stride)
    print(f"stride {stride}: {kept} kept windows over the sweep, {capped} clips cut by a cap")
    assert kept > 100 and capped > 10
    ref = ragged.ref(SEG, stride, 0.5, None)
    by_kind = {}
    for kind, count, peak in zip(ragged.kinds, ref["counts"], ref["peak"]):
        by_kind.setdefault(kind, []).append((count, peak))
    assert all(np.isnan(p) and k == 0 for kind in ("nan", "pinf", "ninf") for k, p in by_kind[kind])
    assert all(k == 0 for kind in ("silent", "click", "quiet") for k, _ in by_kind[kind])
    assert all(k >= 1 for k, _ in by_kind["constant"]) and sum(k for k, _ in by_kind["bursts"]) > 10


@pytest.mark.parametrize("stride", [32, 16, 10, 48])
def test_small_geometry_equals_the_restatement_exactly(small, stride):
    # -14 dB sits between the two levels (0.02 / 0.5 is -28 dB) and -40 dB below the lower one: a clip that holds only
    # the lower level is active throughout, one that holds both has the lower level inactive
    kept, capped = _sweep(small, 32, stride, caps=(None, 1, 2, 3), levels_db=(-14.0, -40.0))
    print(f"stride {stride}: {kept} kept windows over the sweep, {capped} clips cut by a cap")
    assert kept > 200 and capped > 50


def test_windows_longer_than_a_chunk_of_frames(ragged):
    """A 300 000-sample window holds 1873 frames: more than the kernel keeps bits for at a time, so its count is added
    up over several chunks; and a 1600-sample stride gives the long clips hundreds of windows (several rounds of 64)."""
    for seg_len, stride, caps in ((300000, 100000, (None, 2)), (SEG, 1600, (None, 70))):
        for cap in caps:
            ref = ragged.ref(seg_len, stride, 0.25, cap)
            want, want_rows = _want(ref)
            got, rows = _run(ragged, seg_len, stride, 0.25, cap)
            _equal(got, want, f"window {seg_len}, stride {stride}, cap {cap}")
            _equal(rows, want_rows, f"window {seg_len}, stride {stride}, cap {cap}")
        assert max(ref["windows"]) == (5 if seg_len == 300000 else 428) and sum(ref["counts"]) >= 3


def test_kernels_between_guard_zones_at_the_promised_sizes(ragged):
    """Every output at exactly the size the header promises, flush between two guard zones, under each fill; the
    energies flush against a guard too (a load past their end would feed a NaN to a maximum)."""
    stride, min_active, cap = 5000, 0.5, 3
    ref = ragged.ref(SEG, stride, min_active, cap)
    want, want_rows = _want(ref)
    n, total, rows = len(ragged.bank), len(ref["active"]), len(ref["clip"])
    energy = G.Guarded.holding(ragged.energy_dev, align=8, name="energies")
    stale_ref = ragged.ref(SEG, stride, 0.0, None)                       # what an earlier, different call leaves behind
    for fill in G.FILLS:
        out = dict(peak=G.output(n, torch.float64, name="d_peak"), clip_active=G.output(n, torch.int32, name="d_clip_active"),
                   active=G.output(total, torch.int32, name="d_active"), keep=G.output(total, torch.int32, name="d_keep"),
                   counts=G.output(n, torch.int32, name="d_counts"))
        row = dict(clip=G.output(rows, torch.int64, name="d_clip"), start=G.output(rows, torch.int32, name="d_start"),
                   length=G.output(rows, torch.int32, name="d_length"), row_active=G.output(rows, torch.int32, name="d_row_active"))
        for g in (*out.values(), *row.values()):
            g.fill("ones_bits" if fill == "stale" else fill)
        views = {k: g.view(torch.float64 if k == "peak" else torch.int32) for k, g in out.items()}
        row_views = {k: g.view(torch.int64 if k == "clip" else torch.int32) for k, g in row.items()}
        if fill == "stale":
            _run(ragged, SEG, stride, 0.0, None, out=views,
                 rows_out=lambda r: {k: torch.empty(r, dtype=v.dtype, device="cuda") for k, v in row_views.items()},
                 energy_ptr=energy.ptr)
            assert views["counts"].sum().item() == sum(stale_ref["counts"]) > rows
        got, got_rows = _run(ragged, SEG, stride, min_active, cap, out=views, rows_out=lambda r: row_views,
                             energy_ptr=energy.ptr)
        guards = [energy, *out.values(), *row.values()]
        G.check(guards, {**got, **got_rows}, {**want, **want_rows}, f"fill {fill}")


# ------------------------------------------------------------------------------------------------ find_windows
def _check_table(table, ref, c):
    assert table.counts.dtype == torch.int32 and table.counts.device.type == "cpu" and table.counts.tolist() == ref["counts"]
    for t, dtype, key in ((table.clip, torch.int64, "clip"), (table.start, torch.int32, "start"),
                          (table.length, torch.int32, "length"), (table.active, torch.int32, "row_active"),
                          (table.windows, torch.int32, "windows")):
        assert t.dtype == dtype and t.device.type == "cuda" and t.tolist() == ref[key], key
    assert len(table) == len(ref["clip"])
    peak = np.array(ref["peak"])
    # active_share: one IEEE division of the same integers on both sides.  peak_db: log10 is each side's own library's
    # (documented within 2 ulp each), then one rounded product each: under 5 ulp apart, held to 8
    share = table.active_share.cpu().numpy()
    assert table.active_share.dtype == torch.float64 and table.peak_db.dtype == torch.float64
    assert share.tolist() == (np.array(ref["clip_active"], dtype=np.float64) / np.array([len(e) for e in c.energies])).tolist()
    peak_db = table.peak_db.cpu().numpy()
    assert np.array_equal(np.isnan(peak_db), np.isnan(peak))
    with np.errstate(divide="ignore"):
        want_db = 10.0 * np.log10(peak)
    ok = ~np.isnan(peak)
    assert np.array_equal(np.isinf(peak_db[ok]), peak[ok] == 0.0) and (peak_db[ok][peak[ok] == 0.0] < 0).all()
    fin = ok & (peak > 0)
    assert np.all(np.abs(peak_db[fin] - want_db[fin]) <= 8 * np.spacing(np.abs(want_db[fin])))


@pytest.mark.parametrize("params", [dict(), dict(stride=8000, max_per_clip=3), dict(stride=5000, min_active=1.0),
                                    dict(stride=24000, min_active=0.0, threshold_db=-20.0, floor_db=-50.0, max_per_clip=1)])
def test_find_windows_equals_the_restatement(ragged, pre, params):
    kw = dict(params)
    stride, cap = kw.pop("stride", SEG), kw.pop("max_per_clip", None)
    ref = ragged.ref(SEG, stride, kw.pop("min_active", 0.5), cap, **kw)
    table = cda.find_windows(ragged.bank, pre, **params)
    _check_table(table, ref, ragged)
    again = cda.find_windows(ragged.bank, pre, **params)
    for name in ("clip", "start", "length", "active", "active_share", "windows", "counts"):
        assert torch.equal(getattr(again, name), getattr(table, name)), name
    assert torch.equal(torch.nan_to_num(again.peak_db, nan=1.0), torch.nan_to_num(table.peak_db, nan=1.0))


def test_find_windows_at_the_small_geometry_and_on_an_empty_bank(small):
    ref = small.ref(32, 10, 0.5, 2, threshold_db=-14.0, floor_db=-40.0)
    table = cda.find_windows(small.bank, Small(), stride=10, frame_length=8, hop_length=4, threshold_db=-14.0, floor_db=-40.0,
                             max_per_clip=2)
    _check_table(table, ref, small)
    empty = cda.find_windows(cda.DeviceClipBank([], [], device="cuda"), Small(), frame_length=8, hop_length=4)
    assert len(empty) == 0 and empty.counts.numel() == 0 and empty.peak_db.numel() == 0 and empty.clip.dtype == torch.int64
    assert cda.inactive_clips(empty).numel() == 0


# ------------------------------------------------------------------------------------------------ slice_bank
def test_slice_bank_holds_the_source_samples(ragged, pre):
    params = dict(stride=8000, max_per_clip=3)
    ref = ragged.ref(SEG, 8000, 0.5, 3)
    clips, table = cda.slice_bank(ragged.bank, pre, **params)
    _check_table(table, ref, ragged)
    slices = [ragged.clips[c][s:s + n] for c, s, n in zip(ref["clip"], ref["start"], ref["length"])]
    assert isinstance(clips, cda.DeviceClipBank) and clips.device == ragged.bank.device and len(clips) == len(slices) > 30
    assert clips.lengths.tolist() == ref["length"] and {1, 399, 400, 15999, 16000} <= set(ref["length"])
    assert torch.equal(clips.data.cpu(), torch.from_numpy(np.concatenate(slices)))                 # bit for bit
    assert clips.labels.tolist() == [ragged.labels[c] for c in ref["clip"]] and set(clips.labels.tolist()) == {0, 1}
    again, _ = cda.slice_bank(ragged.bank, pre, **params)
    assert torch.equal(again.data, clips.data) and torch.equal(again.lengths, clips.lengths)
    # the table's clip column keeps a recording on one side of the split
    train_idx, val_idx = cda.stratified_group_split(clips.labels, table.clip)
    source = np.array(ref["clip"])
    assert sorted(train_idx + val_idx) == list(range(len(clips))) and not set(source[train_idx]) & set(source[val_idx])
    assert max(ref["counts"]) == 3 and len(set(source[val_idx])) < len(val_idx)        # recordings with several clips
    train, val = cda.prepare_group_split(clips, table.clip)
    assert torch.equal(train.data, clips.subset(train_idx).data) and torch.equal(val.data, clips.subset(val_idx).data)
    # a bank like any other: one batch through the loader equals the batch over the slices themselves
    direct = cda.DeviceClipBank(slices[:8], clips.labels.tolist()[:8], device="cuda")
    fa, ta = next(iter(cda.DeviceDataLoader(clips.subset(range(8)), pre, batch_size=8, is_training=False)))
    fb, tb = next(iter(cda.DeviceDataLoader(direct, pre, batch_size=8, is_training=False)))
    assert fa.shape == (8, 1, 90, 101) and torch.equal(fa, fb) and torch.equal(ta, tb)


def test_a_silent_bank_gives_an_empty_bank(pre):
    silent = cda.DeviceClipBank([torch.zeros(24000), torch.zeros(100), torch.zeros(160000)], [0, 1, 0], device="cuda")
    for bank in (silent, cda.DeviceClipBank([], [], device="cuda")):
        clips, table = cda.slice_bank(bank, pre, stride=8000)
        assert len(clips) == 0 and clips.data.numel() == 0 and clips.device == bank.device and len(table) == 0
        assert table.counts.tolist() == [0] * len(bank) and cda.inactive_clips(table).tolist() == list(range(len(bank)))
    assert table.windows.numel() == 0
    _, table = cda.slice_bank(silent, pre, stride=8000)
    assert table.windows.tolist() == [2, 1, 19] and table.active_share.tolist() == [0.0] * 3
    assert table.peak_db.tolist() == [-np.inf] * 3


def test_inactive_clips_of_one_second_clips(pre):
    """With the defaults: silence and the -70 dB clip lie below the -60 dB floor, a click lights 3 of 98 frames (< half),
    a non-finite sample gates its clip; noise, bursts that fill the second and a constant pass."""
    kinds = ["noise", "silent", "constant", "click", "noise", "quiet", "nan", "noise", "pinf", "ninf", "constant"]
    c = Corpus([(SEG, k) for k in kinds], 9, 400, 160)
    ref = c.ref(SEG, SEG, 0.5, None)
    want = [k for k, kind in enumerate(kinds) if kind not in ("noise", "constant")]
    assert [k for k, count in enumerate(ref["counts"]) if count == 0] == want == [1, 3, 5, 6, 8, 9]
    assert ref["windows"] == [1] * len(kinds) and ref["active"][3] == 3 and ref["active"][0] == 98
    table = cda.find_windows(c.bank, pre)
    _check_table(table, ref, c)
    got = cda.inactive_clips(table)
    assert got.dtype == torch.int64 and got.device.type == "cpu" and got.tolist() == want


# ------------------------------------------------------------------------------------------------ the command line
def test_command_line_slices_a_directory(tmp_path, capsys):
    import json
    import os
    from cough_detector_amd import slices as cslices
    rng = np.random.default_rng(1)
    src = cda.DeviceClipBank([_noise(rng, 40000), np.zeros(20000, dtype=np.float32), _noise(rng, 16000)], [0, 0, 1], device="cpu")
    cda.write_clips(src, tmp_path / "src", ["talk", "nothing", "cough"])
    report = cslices.main([str(tmp_path / "src"), str(tmp_path / "out"), "--stride", "8000", "--max-per-clip", "3"])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == report
    assert (report["recordings"], report["windows"], report["kept"], report["inactive"]) == (3, 4 + 1 + 1, 3 + 0 + 1, 1)
    assert report["minutes_in"] == {"non_cough": 60000 / 16000 / 60, "cough": 16000 / 16000 / 60}
    assert report["minutes_out"] == {"non_cough": 48000 / 16000 / 60, "cough": 16000 / 16000 / 60}
    assert sorted(os.listdir(tmp_path / "out" / "cough")) == ["cough_0.wav"]
    written = sorted(os.listdir(tmp_path / "out" / "non_cough"))
    assert len(written) == 3 and all(name.startswith("talk_") for name in written)
    # the clips that were written are the source's samples at the 16-bit grid of the source files
    back = cda.DeviceClipBank.from_directory(str(tmp_path / "out"), cda.AudioPreprocessor(device="cpu", **SHIPPED), device="cpu")
    assert back.lengths.tolist() == [16000] * 4 and back.labels.tolist() == [0, 0, 0, 1]
