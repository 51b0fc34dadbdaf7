"""Corpus curation on the MI355X (cough_detector_amd/segments.py, csrc/segments.hip) against tests/segments_ref.py.

Energies: the kernel sums a frame's float64 squares sub-block by sub-block, numpy pairwise; both are within a few
hundred ulp of the exact sum of 400 positive terms, so 1e-12 relative holds with two orders to spare, and the same call
twice must give the same bits (fixed-order sums, no atomics).

Segments: every decision of the finder compares float64 energies.  The inputs here are asserted (on the CPU, by the
reference) to take each decision by a relative margin above 1e-9, four orders above what reordering a sum can move, so
counts, clips, starts and lengths must equal the reference's exactly.  ``peak_db`` is one float32 rounding of
``10*log10(e)`` at magnitudes of 10..80 dB (float32 spacing <= 7.6e-6) plus a few ulp of the device's float64 ``log10``:
within 1e-4 dB.

Extraction moves float32 samples: bit for bit.
"""
import numpy as np
import pytest
import torch

import cough_detector_amd as cda
import segments_ref as R

pytestmark = pytest.mark.gpu
SHIPPED = dict(use_pcen=False, use_pre_emphasis=False, use_delta_delta=False, use_spectral_contrast=False)
ENERGY_LENGTHS = [1, 399, 400, 401, 559, 560, 561, 16000, 16001, 40001]
CASES = ["middle", "start_and_end", "two_close", "many", "click", "short", "silent"]


@pytest.fixture(scope="module")
def pre():
    return cda.AudioPreprocessor(device="cuda", **SHIPPED)


# ------------------------------------------------------------------------------------------------ cough_frame_energy
@pytest.fixture(scope="module", params=["in_order", "reversed"])
def energy_clips(request):
    """The lengths in one bank, in both orders: the odd lengths misalign every later clip, and between the two orders the
    clips start on every phase of 16 bytes."""
    lengths = ENERGY_LENGTHS if request.param == "in_order" else ENERGY_LENGTHS[::-1]
    g = torch.Generator().manual_seed(21)
    clips = [((torch.rand(n, generator=g) - 0.5) * 1.6).numpy() for n in lengths]
    phases = {int(o) % 4 for o in np.cumsum([0] + lengths[:-1])}
    assert phases == ({0, 1, 2} if request.param == "in_order" else {0, 1, 2, 3})
    return lengths, clips, cda.DeviceClipBank(clips, [0] * len(clips), device="cuda")


@pytest.mark.parametrize("frame_length,hop_length", [(400, 160), (512, 512), (256, 64), (7, 3), (400, 1000)])
def test_frame_energy_equals_the_float64_reference(energy_clips, frame_length, hop_length):
    lengths, clips, bank = energy_clips
    energy, offsets = cda.frame_energy(bank, frame_length=frame_length, hop_length=hop_length)
    assert energy.dtype == torch.float64 and energy.device.type == "cuda"
    assert offsets.dtype == torch.int64 and offsets.device.type == "cpu" and offsets.numel() == len(bank) + 1
    frames = [R.n_frames(n, frame_length, hop_length) for n in lengths]
    assert offsets.tolist() == np.concatenate([[0], np.cumsum(frames)]).tolist() and energy.numel() == sum(frames)
    got = energy.cpu().numpy()
    worst = 0.0
    for k, x in enumerate(clips):
        want = R.frame_energy_ref(x, frame_length, hop_length)
        mine = got[int(offsets[k]):int(offsets[k + 1])]
        assert mine.shape == want.shape and (want > 0).all()
        rel = float(np.max(np.abs(mine - want) / want))
        worst = max(worst, rel)
        assert rel <= 1e-12, (k, lengths[k], rel)
    print(f"frame_energy ({frame_length}, {hop_length}): worst relative error {worst:.3e}")
    again, _ = cda.frame_energy(bank, frame_length=frame_length, hop_length=hop_length)
    assert torch.equal(again, energy)                                      # bit for bit


def test_frame_energy_of_an_empty_bank():
    energy, offsets = cda.frame_energy(cda.DeviceClipBank([], [], device="cuda"))
    assert energy.numel() == 0 and energy.dtype == torch.float64 and offsets.tolist() == [0]


# ------------------------------------------------------------------------------------------------ cough_pick_segments
def _corpus(seed=3):
    """The hand-built cases, then seeded recordings of 8000..160000 samples holding bursts of 0.1..2 s (a 2 s burst's
    run crosses several 64-frame chunks), two of them spoilt by a NaN and by an Inf sample."""
    cases = R.case_clips(seed=0)
    clips, names = [cases[k] for k in CASES], list(CASES)
    rng = np.random.default_rng(seed)
    for k in range(10):
        n = int(rng.integers(8000, 160001)) if k else 160000
        bursts, pos = [], int(rng.integers(1000, 6000))
        while True:
            length = int(rng.integers(1600, 32001)) if k else 32000
            centre = pos + length // 2
            if centre + length // 2 >= n:
                break
            bursts.append((centre, length, float(rng.uniform(0.05, 0.5))))
            pos = centre + length // 2 + int(rng.integers(200, 30000))
        clips.append(R.recording(rng, n, bursts))
        names.append(f"random{k}")
    for bad, name in ((np.nan, "nan"), (np.inf, "inf")):
        x = clips[names.index("random0")].copy()
        x[70001] = bad
        at = names.index("random3")
        clips.insert(at, x)                                                # between two clips that have segments
        names.insert(at, name)
    labels = [k % 2 for k in range(len(clips))]
    return clips, names, labels


@pytest.fixture(scope="module")
def corpus():
    clips, names, labels = _corpus()
    return clips, names, labels, cda.DeviceClipBank(clips, labels, device="cuda")


def _check_table(table, ref, n_clips):
    assert table.counts.dtype == torch.int32 and table.counts.device.type == "cpu"
    assert table.counts.tolist() == ref["counts"] and len(table.counts) == n_clips
    assert table.clip.dtype == torch.int64 and table.start.dtype == torch.int32 and table.length.dtype == torch.int32
    assert table.peak_db.dtype == torch.float32 and len(table) == len(ref["clip"])
    assert table.clip.tolist() == ref["clip"]
    assert table.start.tolist() == ref["start"]
    assert table.length.tolist() == ref["length"]
    err = float(np.max(np.abs(table.peak_db.cpu().numpy().astype(np.float64) - np.array(ref["peak_db"], dtype=np.float64)),
                       initial=0.0))
    print(f"peak_db: worst difference {err:.3e} dB over {len(table)} segments")
    assert err <= 1e-4


def test_segments_equal_the_reference_exactly(corpus, pre):
    clips, names, labels, bank = corpus
    seg, sr = pre.segment_samples, pre.sample_rate
    assert (seg, sr) == (16000, 16000)
    assert min(len(x) for x in clips) == 8000 and max(len(x) for x in clips) == 160000
    ref = R.table_ref(clips, seg, sr)
    assert ref["margin"] > 1e-9, ref["margin"]                             # no close call: index equality is a fair demand
    by_name = dict(zip(names, ref["counts"]))
    assert [by_name[k] for k in CASES] == [1, 2, 1, 8, 0, 1, 0] and by_name["nan"] == 0 and by_name["inf"] == 0
    assert by_name["random0"] >= 2 and by_name["random2"] >= 1 and by_name["random3"] >= 1   # the spoilt clips' neighbours
    table = cda.find_segments(bank, pre)
    _check_table(table, ref, len(clips))
    again = cda.find_segments(bank, pre)
    for a, b in ((again.clip, table.clip), (again.start, table.start), (again.length, table.length),
                 (again.peak_db, table.peak_db), (again.counts, table.counts)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("params", [
    dict(frame_length=256, hop_length=64, threshold_db=-20.0, min_duration=0.05, max_segments=3),
    dict(frame_length=400, hop_length=1000, threshold_db=-25.0, floor_db=-50.0, min_duration=0.0, max_segments=16),
    dict(max_segments=1, min_duration=0.3)])
def test_segments_follow_their_parameters(corpus, pre, params):
    clips, names, labels, bank = corpus
    ref = R.table_ref(clips, pre.segment_samples, pre.sample_rate, **params)
    assert ref["margin"] > 1e-9 and sum(ref["counts"]) >= 5
    _check_table(cda.find_segments(bank, pre, **params), ref, len(clips))


def test_non_finite_clips_yield_nothing_and_leave_their_neighbours_alone(corpus, pre):
    clips, names, labels, bank = corpus
    table = cda.find_segments(bank, pre)
    counts = dict(zip(names, table.counts.tolist()))
    assert counts["nan"] == 0 and counts["inf"] == 0
    clean = [k for k, name in enumerate(names) if name not in ("nan", "inf")]
    sub = cda.find_segments(bank.subset(clean), pre)
    assert sub.counts.tolist() == [table.counts[k].item() for k in clean] and sub.counts.sum() == table.counts.sum()
    assert torch.equal(sub.start, table.start) and torch.equal(sub.peak_db, table.peak_db)
    assert counts["random0"] >= 2                                          # the clip the two were copied from


# ------------------------------------------------------------------------------------------------ extract_segments
def test_extracted_bank_holds_the_source_slices(corpus, pre):
    clips, names, labels, bank = corpus
    ref = R.table_ref(clips, pre.segment_samples, pre.sample_rate)
    segs, table = cda.extract_segments(bank, pre)
    _check_table(table, ref, len(clips))
    slices = [clips[c][s:s + n] for c, s, n in zip(ref["clip"], ref["start"], ref["length"])]
    assert isinstance(segs, cda.DeviceClipBank) and segs.device == bank.device and len(segs) == len(slices) > 20
    assert segs.data.dtype == torch.float32 and torch.equal(segs.data.cpu(), torch.from_numpy(np.concatenate(slices)))
    assert segs.lengths.tolist() == ref["length"] and 8000 in ref["length"] and 16000 in ref["length"]
    assert segs.labels.tolist() == [labels[c] for c in ref["clip"]] and set(segs.labels.tolist()) == {0, 1}
    assert segs.offsets.tolist() == np.concatenate([[0], np.cumsum(ref["length"])[:-1]]).tolist()
    for dev, host in ((segs.offsets_dev, segs.offsets), (segs.lengths_dev, segs.lengths), (segs.labels_dev, segs.labels)):
        assert torch.equal(dev.cpu(), host)
    # a bank like any other: subset, and a validation loader equal to one over the slices themselves
    sub = segs.subset([3, 0])
    assert torch.equal(sub.clip(0).cpu()[0], torch.from_numpy(slices[3])) and sub.labels.tolist() == [segs.labels[3], segs.labels[0]]
    direct = cda.DeviceClipBank(slices, segs.labels.tolist(), device="cuda")
    mine = list(cda.DeviceDataLoader(segs, pre, batch_size=8, is_training=False))
    theirs = list(cda.DeviceDataLoader(direct, pre, batch_size=8, is_training=False))
    assert len(mine) == len(theirs) == (len(slices) + 7) // 8
    for (fa, ta), (fb, tb) in zip(mine, theirs):
        assert fa.shape[1:] == (1, 90, 101) and torch.equal(fa, fb) and torch.equal(ta, tb)
    train, val = cda.create_data_loaders(segs, segs.subset(range(5)), pre, batch_size=4)
    assert len(train) == len(segs) // 4 and len(val) == 2


def test_a_corpus_without_a_segment_gives_an_empty_bank(pre):
    silent = cda.DeviceClipBank([torch.zeros(24000), torch.zeros(100), torch.zeros(160000)], [0, 1, 0], device="cuda")
    for bank in (silent, cda.DeviceClipBank([], [], device="cuda")):
        segs, table = cda.extract_segments(bank, pre)
        assert len(segs) == 0 and segs.data.numel() == 0 and segs.device == bank.device and len(table) == 0
        assert table.counts.tolist() == [0] * len(bank) and table.start.numel() == 0 and table.peak_db.numel() == 0
        assert len(cda.DeviceDataLoader(segs, pre, batch_size=4, is_training=False)) == 0
