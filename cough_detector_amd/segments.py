"""Corpus curation on the MI355X: cut cough-length segments out of long recordings and drop the silence.

The reference names this as its next step and has an empty stub for it (``find_energy_peaks`` / ``extract_segments``):
``cough_prepare_rows`` centre-trims every clip to ``segment_samples`` as ``CoughDataset`` does, so a 10 s recording
gives the loader its middle second, whatever that second holds.  Here a ``DeviceClipBank`` of long recordings becomes a
``DeviceClipBank`` of segments of at most ``segment_samples``, each centred on a short-time-energy peak:

1. frames: ``n_frames = 1`` if ``n < frame_length`` else ``1 + (n - frame_length) // hop_length``; ``e[f]`` is the mean of
   ``double(x)**2`` over frame ``f`` (``cough_frame_energy``; samples past the last full frame take no part);
2. gate: a clip with a non-finite ``e[f]``, or with ``max(e) < 10**(floor_db/10)``, yields nothing;
3. activity: ``e[f] >= max(e) * 10**(threshold_db/10)``;
4. runs of at least ``max(1, ceil(min_duration * sample_rate / hop_length))`` consecutive active frames are kept;
5. per kept run, in time order: ``p`` its first largest frame, ``c = p*hop_length + frame_length//2``, ``length =
   min(seg_len, n)``, ``start = min(max(c - seg_len//2, 0), max(n - seg_len, 0))``; a run that would start before the
   end of the clip's last segment is dropped; at most ``max_segments`` per clip (``cough_pick_segments``).

Three kernels of ``libcough_amd_segments.so`` (``include/cough_amd_segments.h``) on the packed bank; the one value the
host reads back is the per-clip segment count, which sizes the outputs.  For negatives -- every active second of a
recording, not its loudest frames -- see ``slices.py`` (``find_windows`` / ``slice_bank``).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Tuple

import numpy as np
import torch

from . import _lib
from .data import DeviceClipBank, _offsets, _owner, _ragged, _stream, _upload


@dataclass
class SegmentTable:
    """Where each segment came from, one entry per segment in clip order and then time order: ``clip`` (int64 index
    into the source bank), ``start`` and ``length`` (int32, samples within that clip), ``peak_db`` (float32,
    ``10*log10`` of the peak frame's energy), all on the bank's device; ``counts`` (host int32) holds the segments of
    every source clip."""
    clip: torch.Tensor
    start: torch.Tensor
    length: torch.Tensor
    peak_db: torch.Tensor
    counts: torch.Tensor

    def __len__(self) -> int:
        return int(self.clip.numel())


def _check_frames(what: str, frame_length, hop_length) -> Tuple[int, int]:
    for name, v in (("frame_length", frame_length), ("hop_length", hop_length)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError(f"{what}: {name}={v!r} must be a positive integer")
    if frame_length > _lib.MAX_FRAME_LENGTH:
        raise ValueError(f"{what}: frame_length={frame_length} is above {_lib.MAX_FRAME_LENGTH}")
    if hop_length > 2**31 - 1:
        raise ValueError(f"{what}: hop_length={hop_length} does not fit 32 bits")
    return int(frame_length), int(hop_length)


def _check_device(what: str, bank: DeviceClipBank) -> torch.device:
    if bank.device.type != "cuda":
        raise RuntimeError(f"{what}: the bank lives on {bank.device}; the kernels need it on the GPU (there is no CPU "
                           "fallback)")
    return bank.device


def frame_counts(lengths: np.ndarray, frame_length: int, hop_length: int) -> np.ndarray:
    """Frames per clip (int64) for int clip ``lengths``."""
    n = np.asarray(lengths, dtype=np.int64)
    return np.where(n < frame_length, 1, 1 + (n - frame_length) // hop_length).astype(np.int64)


def _frame_energy(bank: DeviceClipBank, frame_length: int, hop_length: int):
    """-> (energy float64 [total frames] on the device, frame offsets on the host (numpy int64 [n + 1]) and on the device)"""
    dev, lib, n = bank.device, _lib.load_segments(), len(bank)
    frames = frame_counts(bank.lengths.numpy(), frame_length, hop_length)
    frame_offsets = _offsets(frames)
    energy = torch.empty(int(frame_offsets[-1]), dtype=torch.float64, device=dev)
    if n == 0:
        return energy, frame_offsets, torch.zeros(1, dtype=torch.int64, device=dev)
    tile_frames = lib.cough_frame_energy_tile_frames(frame_length, hop_length)
    tile_offsets, tile_clip, tile_rank = _ragged((frames + tile_frames - 1) // tile_frames)
    n_tiles = int(tile_offsets[-1])
    if n_tiles > 2**31 - 1:
        raise ValueError(f"frame_energy: {n_tiles} tiles do not fit one launch; split the bank")
    tiles = np.empty((n_tiles, 2), dtype=np.int32)
    tiles[:, 0], tiles[:, 1] = tile_clip, tile_rank * tile_frames
    offs_dev, tiles_dev = _upload(dev, frame_offsets, tiles.reshape(-1))
    _lib.check_segments(lib.cough_frame_energy(bank.data.data_ptr(), bank.offsets_dev.data_ptr(),
                                               bank.lengths_dev.data_ptr(), offs_dev.data_ptr(), n, tiles_dev.data_ptr(),
                                               n_tiles, frame_length, hop_length, energy.data_ptr(), _stream(dev)),
                        "cough_frame_energy")
    return energy, frame_offsets, offs_dev


def frame_energy(bank: DeviceClipBank, frame_length: int = 400, hop_length: int = 160) -> Tuple[torch.Tensor, torch.Tensor]:
    """The short-time energy of every frame of every clip: ``(energy, frame_offsets)`` with ``energy`` a float64 device
    tensor and clip ``k``'s frames at ``energy[frame_offsets[k] : frame_offsets[k + 1]]`` (``frame_offsets``: host int64,
    ``len(bank) + 1`` entries).  Stream-ordered; nothing waits for the device."""
    frame_length, hop_length = _check_frames("frame_energy", frame_length, hop_length)
    _check_device("frame_energy", bank)
    energy, frame_offsets, _ = _frame_energy(bank, frame_length, hop_length)
    return energy, torch.from_numpy(frame_offsets)


def _db_ratios(what: str, threshold_db, floor_db, **number) -> Tuple[float, float]:
    """``(10**(threshold_db/10), 10**(floor_db/10))``, once the two and the further ``number`` (by name) are finite numbers."""
    for name, v in (("threshold_db", threshold_db), ("floor_db", floor_db), *number.items()):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
            raise ValueError(f"{what}: {name}={v!r} must be a finite number")
    try:
        return 10.0 ** (float(threshold_db) / 10.0), 10.0 ** (float(floor_db) / 10.0)
    except OverflowError:
        raise ValueError(f"{what}: threshold_db={threshold_db} / floor_db={floor_db} overflow a double") from None


def _params(what: str, preprocessor, frame_length=400, hop_length=160, threshold_db=-30.0, floor_db=-60.0,
            min_duration=0.1, max_segments=8):
    frame_length, hop_length = _check_frames(what, frame_length, hop_length)
    if isinstance(max_segments, bool) or not isinstance(max_segments, (int, np.integer)) or \
            not 1 <= max_segments <= _lib.MAX_SEGMENTS:
        raise ValueError(f"{what}: max_segments={max_segments!r} must be an integer in 1..{_lib.MAX_SEGMENTS}")
    ratio, floor = _db_ratios(what, threshold_db, floor_db, min_duration=min_duration)
    if min_duration < 0:
        raise ValueError(f"{what}: min_duration={min_duration} must not be negative")
    seg_len, sr = int(preprocessor.segment_samples), int(preprocessor.sample_rate)
    if seg_len < 1 or sr < 1:
        raise ValueError(f"{what}: the preprocessor's segment_samples={seg_len} and sample_rate={sr} must be positive")
    min_frames = max(1, math.ceil(float(min_duration) * sr / hop_length))
    if min_frames > 2**31 - 1:
        raise ValueError(f"{what}: min_duration={min_duration} is {min_frames} frames")
    return frame_length, hop_length, seg_len, min_frames, int(max_segments), ratio, floor


def find_segments(bank: DeviceClipBank, preprocessor, **params) -> SegmentTable:
    """The segments of every clip of ``bank`` (module docstring).  ``params``: ``frame_length=400, hop_length=160,
    threshold_db=-30.0, floor_db=-60.0, min_duration=0.1`` (seconds), ``max_segments=8`` (1..16); the segment length
    and the sample rate are ``preprocessor.segment_samples`` and ``preprocessor.sample_rate``.  One host read (the
    per-clip counts); everything else is stream-ordered."""
    frame_length, hop_length, seg_len, min_frames, max_segments, ratio, floor = _params("find_segments", preprocessor,
                                                                                      **params)
    dev, n = _check_device("find_segments", bank), len(bank)
    i32 = dict(dtype=torch.int32, device=dev)
    if n == 0:
        return SegmentTable(torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros(0, **i32), torch.zeros(0, **i32),
                            torch.zeros(0, dtype=torch.float32, device=dev), torch.zeros(0, dtype=torch.int32))
    energy, _, offs_dev = _frame_energy(bank, frame_length, hop_length)
    counts_dev = torch.empty(n, **i32)
    starts, lengths = torch.empty((n, max_segments), **i32), torch.empty((n, max_segments), **i32)
    peak_db = torch.empty((n, max_segments), dtype=torch.float32, device=dev)
    _lib.check_segments(_lib.load_segments().cough_pick_segments(
        energy.data_ptr(), offs_dev.data_ptr(), bank.lengths_dev.data_ptr(), n, frame_length, hop_length, seg_len,
        min_frames, max_segments, ratio, floor, counts_dev.data_ptr(), starts.data_ptr(), lengths.data_ptr(),
        peak_db.data_ptr(), _stream(dev)), "cough_pick_segments")
    counts = counts_dev.cpu()                                    # the one host read: it sizes the table
    _, clip, rank = _ragged(counts)
    flat = clip * max_segments + rank
    idx, _ = _upload(dev, np.concatenate([clip, flat]), np.zeros(0, np.int32))
    clip_dev, flat_dev = idx[:clip.size], idx[clip.size:]
    return SegmentTable(clip_dev, starts.view(-1)[flat_dev], lengths.view(-1)[flat_dev], peak_db.view(-1)[flat_dev], counts)


def _cut_rows(bank: DeviceClipBank, table, seg_len: int) -> DeviceClipBank:
    """The bank of the rows of a table: ``table.counts[k]`` (host) rows of source clip ``k``, row ``j`` the ``min(seg_len,
    n)`` samples of its clip from ``table.start[j]`` (device int32) on, with that clip's label."""
    clip = _owner(table.counts)
    return bank.cut(clip, table.start, np.minimum(bank.lengths.numpy()[clip], seg_len))   # min(seg_len, n): known to the host


def extract_segments(bank: DeviceClipBank, preprocessor, **params) -> Tuple[DeviceClipBank, SegmentTable]:
    """``(segments, table)``: a ``DeviceClipBank`` on ``bank``'s device whose clip ``j`` is samples ``table.start[j] ..
    + table.length[j]`` of source clip ``table.clip[j]`` with that clip's label -- a bank like any other (``subset``,
    ``DeviceDataLoader``, ``create_data_loaders``).  A corpus without a segment gives an empty bank.  ``params`` as
    ``find_segments``."""
    table = find_segments(bank, preprocessor, **params)
    return _cut_rows(bank, table, int(preprocessor.segment_samples)), table
