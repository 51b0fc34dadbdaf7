"""``DeviceClipBank.cut`` (cough_detector_amd/data.py), the one wrapper of ``cough_copy_segments``, on the MI355X.

The copy moves float32 samples, so everything here is bit for bit.  The source samples are ``arange`` floats (exact up to
2^24): a wrong offset shows as a wrong value.  The spans start off 16-byte alignment, their odd lengths leave the later
destinations off it too, lengths 1 and 4 take the kernel's head-only and tail-only paths and 2049 its grid-stride float4
body.  ``extract_segments`` is held against the body of the wrapper it used before ``cut`` existed.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import cough_detector_amd as cda
from cough_detector_amd import _lib
from cough_detector_amd import data as cdata
from cough_detector_amd._native import _stream

pytestmark = pytest.mark.gpu
LENGTHS, LABELS = (7, 2050, 1), (0, 1, 0)
SPANS = [(0, 0, 7), (0, 3, 1), (1, 1, 2049), (1, 5, 1030), (2, 0, 1), (1, 2046, 4)]
EXPLICIT = [1, 0, 0, 1, 1, 0]


@pytest.fixture(scope="module")
def bank():
    samples = torch.arange(sum(LENGTHS), dtype=torch.float32)
    return cda.DeviceClipBank(list(samples.split(list(LENGTHS))), LABELS, device="cuda")


@pytest.fixture
def uploads(monkeypatch):
    calls, real = [], cdata._upload

    def counted(dev, i64, i32):
        calls.append((int(i64.size), int(i32.size)))
        return real(dev, i64, i32)

    monkeypatch.setattr(cdata, "_upload", counted)
    return calls


def _spans():
    clips, starts, lengths = (np.array(v, dtype=np.int64) for v in zip(*SPANS))
    return clips, starts, lengths


def _starts(form: str, starts: np.ndarray):
    return torch.from_numpy(starts.astype(np.int32)).cuda() if form == "device" else starts


def _check(out: cda.DeviceClipBank, bank: cda.DeviceClipBank, labels) -> None:
    host, offsets = bank.data.cpu(), bank.offsets.tolist()
    want = torch.cat([host[offsets[c] + s:offsets[c] + s + n] for c, s, n in SPANS])
    assert isinstance(out, cda.DeviceClipBank) and out.device == bank.device and len(out) == len(SPANS)
    assert out.data.dtype == torch.float32 and out.data.device.type == "cuda" and torch.equal(out.data.cpu(), want)
    lengths = [n for _, _, n in SPANS]
    assert out.lengths.tolist() == lengths and out.lengths_dev.cpu().tolist() == lengths
    assert out.offsets.tolist() == [0, 7, 8, 2057, 3087, 3088] == out.offsets_dev.cpu().tolist()
    assert out.labels.tolist() == list(labels) == out.labels_dev.cpu().tolist()
    for j, (c, s, n) in enumerate(SPANS):                                 # row by row, through the bank's own accessor
        assert torch.equal(out.clip(j).cpu()[0], host[offsets[c] + s:offsets[c] + s + n]), j


@pytest.mark.parametrize("form", ["device", "host"])
def test_cut_equals_host_slicing(bank, uploads, form):
    clips, starts, lengths = _spans()
    assert [int(bank.offsets[c] + s) % 4 for c, s, _ in SPANS] == [0, 3, 0, 0, 1, 1]    # sources off 16-byte alignment
    out = bank.cut(clips, _starts(form, starts), lengths)
    assert uploads == [(2 * len(SPANS), 0 if form == "device" else len(SPANS))]        # one upload; host starts ride in it
    _check(out, bank, [0, 0, 1, 1, 0, 1])
    del uploads[:]
    _check(bank.cut(clips, _starts(form, starts), lengths, labels=EXPLICIT), bank, EXPLICIT)
    assert len(uploads) == 1


def test_both_forms_of_starts_give_the_same_bank(bank):
    clips, starts, lengths = _spans()
    a, b = (bank.cut(clips, _starts(form, starts), lengths, labels=EXPLICIT) for form in ("device", "host"))
    for name in ("data", "offsets", "lengths", "labels", "offsets_dev", "lengths_dev", "labels_dev"):
        u, v = getattr(a, name), getattr(b, name)
        assert u.dtype == v.dtype and u.device == v.device and torch.equal(u, v), name


@pytest.mark.parametrize("form", ["device", "host"])
def test_cut_without_spans_is_an_empty_bank(bank, uploads, form):
    none = np.zeros(0, dtype=np.int64)
    for labels in (None, []):
        out = bank.cut(none, _starts(form, none), none, labels=labels)
        assert isinstance(out, cda.DeviceClipBank) and len(out) == 0 and out.device == bank.device
        assert out.data.numel() == 0 and out.data.dtype == torch.float32 and out.data.device.type == "cuda"
        assert out.lengths.tolist() == out.offsets.tolist() == out.labels.tolist() == []
    assert uploads == []                                                   # no upload (and nothing to launch)


# ------------------------------------------------------------------------------------------------ the wrapper before cut
def _copy_rows_before(bank, counts, starts, seg_len):
    """The body of ``segments._copy_rows`` as it was before ``DeviceClipBank.cut``, with the output bank's members as
    plain values: -> (data, lengths, labels)."""
    dev = bank.device
    per_clip = counts.numpy().astype(np.int64)
    clip = np.repeat(np.arange(len(bank), dtype=np.int64), per_clip)
    lengths = np.minimum(bank.lengths.numpy()[clip], seg_len).astype(np.int32)      # min(seg_len, n): known to the host
    dst = np.concatenate([[0], np.cumsum(lengths, dtype=np.int64)]).astype(np.int64)
    data = torch.empty(int(dst[-1]), dtype=torch.float32, device=dev)
    lengths_dev = torch.tensor(lengths.tolist(), dtype=torch.int32).to(dev)
    if clip.size:
        offs, _ = cdata._upload(dev, np.concatenate([bank.offsets.numpy()[clip], dst[:-1]]), np.zeros(0, np.int32))
        _lib.check_segments(_lib.load_segments().cough_copy_segments(
            bank.data.data_ptr(), offs[:clip.size].data_ptr(), starts.data_ptr(), lengths_dev.data_ptr(),
            offs[clip.size:].data_ptr(), int(clip.size), int(lengths.max()), data.data_ptr(), _stream(dev)),
            "cough_copy_segments")
    return data, lengths.tolist(), bank.labels.numpy()[clip].tolist()


def test_extract_segments_equals_the_wrapper_it_had_before():
    """Bursts of uniform noise of amplitude 0.5 over digital silence: a burst's frames lie within a few per cent of one
    energy and far above the -30 dB activity line, the silence below the floor, so every burst of >= 10 frames is one
    run and one segment: one in clip 0, none in the silent clip 1, two in clip 2 (the second starts past the end of the
    first), none in clip 3 (a single frame is no run of 0.1 s)."""
    g = torch.Generator().manual_seed(17)
    clips = [torch.zeros(n) for n in (16000, 400, 24000, 399)]
    for k, lo, hi in ((0, 6001, 9000), (2, 2000, 5000), (2, 15003, 19000), (3, 0, 399)):
        clips[k][lo:hi] = torch.rand(hi - lo, generator=g) - 0.5
    bank = cda.DeviceClipBank(clips, [1, 0, 1, 0], device="cuda")
    pre = SimpleNamespace(segment_samples=8000, sample_rate=16000)
    segs, table = cda.extract_segments(bank, pre)
    assert table.counts.tolist() == [1, 0, 2, 0] and len(segs) == 3
    data, lengths, labels = _copy_rows_before(bank, table.counts, table.start, 8000)
    assert torch.equal(segs.data, data) and segs.data.numel() == 24000
    assert segs.lengths.tolist() == lengths == [8000] * 3 and segs.labels.tolist() == labels == [1, 1, 1]
    starts = table.start.cpu().tolist()
    for j, c in enumerate(table.clip.cpu().tolist()):                      # and both are the samples they name
        assert torch.equal(segs.clip(j).cpu()[0], clips[c][starts[j]:starts[j] + 8000]), j
