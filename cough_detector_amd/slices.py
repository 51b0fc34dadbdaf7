"""Corpus curation on the MI355X: slice long recordings into fixed-length clips and keep the ones that are not silence.

The reference's plan asks for a non-cough class built from real recordings (speech, laughing, breathing, noise)
"segmented into 1-2 second clips" with silence kept minimal, and leaves it as a stub (``prepare_librispeech``).
``extract_segments`` is the wrong tool for that: it centres at most 8 segments per clip on the loudest frames, which is
right for coughs and keeps only the loudest syllables of an utterance.  Here every recording of a ``DeviceClipBank`` is
tiled into windows of ``segment_samples`` at a ``stride`` and a window is kept when enough of its frames are active:

1. windows: a clip of ``n`` samples has one window ``[0, n)`` if ``n < seg_len``, else ``1 + (n - seg_len) // stride``
   windows ``[w*stride, w*stride + seg_len)``;
2. frames and their energies as in ``segments.py`` (``cough_frame_energy``); a frame belongs to a window iff its whole
   extent lies inside it, ``cnt[w]`` such frames;
3. gate: a clip with a non-finite energy has ``peak = NaN`` and no window; a clip with ``E_max = max(e) <
   10**(floor_db/10)`` has no window;
4. activity: ``e[f] >= max(E_max * 10**(threshold_db/10), 10**(floor_db/10))``;
5. window ``w`` with ``m[w]`` active frames qualifies iff ``m[w] >= 1`` and ``m[w] >= min_active * cnt[w]``;
6. with ``max_per_clip``, the qualifying windows with the largest ``m`` are kept, ties going to the earlier window.

Two kernels of ``libcough_amd_slices.so`` (``include/cough_amd_slices.h`` states the arithmetic word by word); the one
value the host reads back is the per-clip count of kept windows, which sizes the table.  The kept windows are copied
with ``cough_copy_segments``.  ``table.clip`` names the recording of every clip and is what
``prepare_group_split(clips, table.clip)`` takes to keep a recording on one side of the split.

    python -m cough_detector_amd.slices recordings out --stride 8000 --min-active 0.5 --max-per-clip 20
"""
from __future__ import annotations

import json
import wave
from dataclasses import dataclass
from pathlib import Path
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .data import CLASSES, DeviceClipBank, _offsets, _stream, _upload
from .segments import _check_device, _check_frames, _cut_rows, _db_ratios, _frame_energy

NO_CAP = 2**31 - 1


@dataclass
class WindowTable:
    """Where each kept window came from, one entry per window in clip order and then time order: ``clip`` (int64 index
    into the source bank), ``start`` and ``length`` (int32, samples within that clip) and ``active`` (int32, its active
    frames); and per source clip ``peak_db`` (float64, ``10*log10`` of the largest frame energy, NaN for a clip with a
    non-finite energy), ``active_share`` (float64, active frames / frames) and ``windows`` (int32, how many windows the
    clip had) -- all on the bank's device; ``counts`` (host int32) holds the kept windows of every source clip."""
    clip: torch.Tensor
    start: torch.Tensor
    length: torch.Tensor
    active: torch.Tensor
    peak_db: torch.Tensor
    active_share: torch.Tensor
    windows: torch.Tensor
    counts: torch.Tensor

    def __len__(self) -> int:
        return int(self.clip.numel())


def window_counts(lengths: np.ndarray, seg_len: int, stride: int) -> np.ndarray:
    """Windows per clip (int64) for int clip ``lengths``."""
    n = np.asarray(lengths, dtype=np.int64)
    return np.where(n < seg_len, 1, 1 + (n - seg_len) // stride).astype(np.int64)


def _params(what: str, preprocessor, stride=None, frame_length=400, hop_length=160, threshold_db=-30.0, floor_db=-60.0,
            min_active=0.5, max_per_clip=None):
    frame_length, hop_length = _check_frames(what, frame_length, hop_length)
    seg_len = int(preprocessor.segment_samples)
    if seg_len < frame_length:
        raise ValueError(f"{what}: the preprocessor's segment_samples={seg_len} is below frame_length={frame_length}")
    if stride is None:
        stride = seg_len
    for name, v in (("stride", stride),) + ((("max_per_clip", max_per_clip),) if max_per_clip is not None else ()):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= 2**31 - 1:
            raise ValueError(f"{what}: {name}={v!r} must be a positive integer that fits 32 bits")
    ratio, floor = _db_ratios(what, threshold_db, floor_db, min_active=min_active)
    if not 0.0 <= min_active <= 1.0:
        raise ValueError(f"{what}: min_active={min_active} must lie in 0..1")
    return (frame_length, hop_length, seg_len, int(stride), NO_CAP if max_per_clip is None else int(max_per_clip), ratio,
            floor, float(min_active))


def find_windows(bank: DeviceClipBank, preprocessor, stride: Optional[int] = None, frame_length: int = 400,
                 hop_length: int = 160, threshold_db: float = -30.0, floor_db: float = -60.0, min_active: float = 0.5,
                 max_per_clip: Optional[int] = None) -> WindowTable:
    """The kept windows of every clip of ``bank`` (module docstring).  The window length is
    ``preprocessor.segment_samples``; ``stride=None`` means that length (no overlap), ``max_per_clip=None`` no cap;
    ``min_active`` is the share of a window's frames that must be active (0..1; at least one frame always).  One host
    read (the per-clip counts); everything else is stream-ordered."""
    frame_length, hop_length, seg_len, stride, cap, ratio, floor, min_active = _params(
        "find_windows", preprocessor, stride, frame_length, hop_length, threshold_db, floor_db, min_active, max_per_clip)
    dev, n = _check_device("find_windows", bank), len(bank)
    i32, f64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float64, device=dev)
    if n == 0:
        return WindowTable(torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros(0, **i32), torch.zeros(0, **i32),
                           torch.zeros(0, **i32), torch.zeros(0, **f64), torch.zeros(0, **f64), torch.zeros(0, **i32),
                           torch.zeros(0, dtype=torch.int32))
    lib = _lib.load_slices()
    per_clip = window_counts(bank.lengths.numpy(), seg_len, stride)
    window_offsets = _offsets(per_clip)
    energy, _, offs_dev = _frame_energy(bank, frame_length, hop_length)
    woffs_dev, windows_dev = _upload(dev, window_offsets, per_clip.astype(np.int32))
    total = int(window_offsets[-1])
    peak, clip_active, counts_dev = torch.empty(n, **f64), torch.empty(n, **i32), torch.empty(n, **i32)
    active, keep = torch.empty(total, **i32), torch.empty(total, **i32)
    _lib.check_slices(lib.cough_window_activity(
        energy.data_ptr(), offs_dev.data_ptr(), bank.lengths_dev.data_ptr(), woffs_dev.data_ptr(), n, frame_length,
        hop_length, seg_len, stride, cap, ratio, floor, min_active, peak.data_ptr(), clip_active.data_ptr(),
        active.data_ptr(), keep.data_ptr(), counts_dev.data_ptr(), _stream(dev)), "cough_window_activity")
    counts = counts_dev.cpu()                                    # the one host read: it sizes the table
    row_offsets = _offsets(counts)
    rows = int(row_offsets[-1])
    roffs_dev, _ = _upload(dev, row_offsets, np.zeros(0, np.int32))
    clip = torch.empty(rows, dtype=torch.int64, device=dev)
    start, length, row_active = torch.empty(rows, **i32), torch.empty(rows, **i32), torch.empty(rows, **i32)
    if rows:                                                     # an empty tensor has no address to pass
        _lib.check_slices(lib.cough_list_windows(
            keep.data_ptr(), active.data_ptr(), bank.lengths_dev.data_ptr(), woffs_dev.data_ptr(), roffs_dev.data_ptr(), n,
            seg_len, stride, clip.data_ptr(), start.data_ptr(), length.data_ptr(), row_active.data_ptr(), _stream(dev)),
            "cough_list_windows")
    frames = (offs_dev[1:] - offs_dev[:-1]).to(torch.float64)
    return WindowTable(clip, start, length, row_active, 10.0 * torch.log10(peak), clip_active.to(torch.float64) / frames,
                       windows_dev, counts)


def slice_bank(bank: DeviceClipBank, preprocessor, **params) -> Tuple[DeviceClipBank, WindowTable]:
    """``(clips, table)``: a ``DeviceClipBank`` on ``bank``'s device whose clip ``j`` is samples ``table.start[j] ..
    + table.length[j]`` of source clip ``table.clip[j]`` with that clip's label -- a bank like any other.  A corpus
    without a kept window gives an empty bank.  ``params`` as ``find_windows``."""
    table = find_windows(bank, preprocessor, **params)
    return _cut_rows(bank, table, int(preprocessor.segment_samples)), table


def inactive_clips(table: WindowTable) -> torch.Tensor:
    """The source clips without a kept window (host int64 indices, ascending): silence, clicks, clips below the floor
    and clips with a non-finite sample.  For a bank of one-second clips these are the ones to hold against the plan's
    "silence: 100-200"."""
    return torch.from_numpy(np.flatnonzero(table.counts.numpy() == 0).astype(np.int64))


def write_clips(bank: DeviceClipBank, out_dir, names: Sequence[str], sample_rate: int = 16000) -> List[str]:
    """Write clip ``k`` of ``bank`` to ``out_dir/non_cough/names[k].wav`` or ``out_dir/cough/names[k].wav`` by its label:
    16-bit PCM mono WAVE at ``sample_rate`` (the preprocessor's), samples ``round(clip(x, -1, 1) * 32767)``.  Returns
    the paths in the bank's order."""
    names = [str(v) for v in names]
    if len(names) != len(bank):
        raise ValueError(f"write_clips: {len(bank)} clips but {len(names)} names")
    if isinstance(sample_rate, bool) or not isinstance(sample_rate, (int, np.integer)) or sample_rate < 1:
        raise ValueError(f"write_clips: sample_rate={sample_rate!r} must be a positive integer")
    root = Path(out_dir)
    data = bank.data.cpu().numpy()
    paths = []
    for k, name in enumerate(names):
        class_dir = root / CLASSES[int(bank.labels[k])]
        class_dir.mkdir(parents=True, exist_ok=True)
        o, n = int(bank.offsets[k]), int(bank.lengths[k])
        pcm = np.rint(np.clip(data[o:o + n].astype(np.float64), -1.0, 1.0) * 32767.0).astype("<i2")
        path = class_dir / (name if name.lower().endswith(".wav") else name + ".wav")
        with wave.open(str(path), "wb") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(int(sample_rate))
            f.writeframes(pcm.tobytes())
        paths.append(str(path))
    return paths


def main(argv=None) -> dict:
    import argparse

    from .audit import bank_files
    from .preprocessing import AudioPreprocessor
    from . import train as _train

    ap = argparse.ArgumentParser(prog="python -m cough_detector_amd.slices", description=__doc__.split("\n\n")[0])
    ap.add_argument("src_dir", help="directory with non_cough/ and cough/ WAVE files")
    ap.add_argument("out_dir", help="where the clips go: out_dir/non_cough and out_dir/cough, STEM_START.wav")
    ap.add_argument("--stride", type=int, default=None, help="samples between windows (default: the window length)")
    ap.add_argument("--frame-length", type=int, default=400)
    ap.add_argument("--hop-length", type=int, default=160)
    ap.add_argument("--threshold-db", type=float, default=-30.0)
    ap.add_argument("--floor-db", type=float, default=-60.0)
    ap.add_argument("--min-active", type=float, default=0.5)
    ap.add_argument("--max-per-clip", type=int, default=None)
    args = ap.parse_args(argv)
    pre = AudioPreprocessor(device="cuda", **_train.preprocessor_config())
    files = bank_files(args.src_dir)
    bank = DeviceClipBank.from_directory(args.src_dir, pre)
    if len(files) != len(bank):
        raise RuntimeError(f"{args.src_dir} changed while it was read: {len(files)} files, {len(bank)} clips")
    clips, table = slice_bank(bank, pre, stride=args.stride, frame_length=args.frame_length, hop_length=args.hop_length,
                              threshold_db=args.threshold_db, floor_db=args.floor_db, min_active=args.min_active,
                              max_per_clip=args.max_per_clip)
    source, start = table.clip.cpu().tolist(), table.start.cpu().tolist()
    write_clips(clips, args.out_dir, [f"{Path(files[c]).stem}_{s}" for c, s in zip(source, start)], pre.sample_rate)

    def minutes(b: DeviceClipBank) -> dict:
        return {name: float(b.lengths[b.labels == label].sum()) / pre.sample_rate / 60.0 for label, name in enumerate(CLASSES)}

    report = dict(recordings=len(bank), windows=int(table.windows.sum()), kept=len(table),
                  inactive=int(inactive_clips(table).numel()), minutes_in=minutes(bank), minutes_out=minutes(clips))
    print(json.dumps(report))
    return report


if __name__ == "__main__":
    main()
