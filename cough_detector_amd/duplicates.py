"""Corpus curation on the MI355X: find the clips of a corpus that are copies of one another.

``fit`` picks its best model by validation F1 and ``audit_labels`` trusts out-of-fold scores; both assume that no clip
sits on both sides of a split.  ``prepare_group_split`` keeps the pieces of one recording together, but it cannot know
that two files hold the same audio: a re-upload, the same sound at another gain, trimmed, or starting a few
milliseconds later.  And two copies of one sound filed under ``cough/`` and ``non_cough/`` are the cheapest evidence of
a mislabel there is.

1. fingerprint: every clip is judged as the loader sees it (``cough_prepare_rows`` with peak normalisation, then the
   featuriser).  Of that image only 33 mel rows are used (dB scaled to 0..1, so the sign of a difference does not change
   with gain): sums over ``window`` frames, differences between neighbouring rows, and one bit per row pair and frame
   for the sign of that difference's change over ``delta`` frames -- the binary fingerprint of Haitsma and Kalker ("A
   Highly Robust Audio Fingerprinting System", ISMIR 2002) on this package's own features.  A clip whose words are all
   zero (silence, a non-finite sample) is *flat*: reported, never paired.
2. match: all pairs ``a < b`` at the lags ``0, -1, +1, ..., -max_lag, +max_lag``; at a lag the bit error rate is the
   popcount of the XOR over the frames that meet, counting only frames where either word is non-zero; the lag with the
   smallest rate wins (ties: the earlier one) if it has ``min_live`` such frames, and the pair matches when
   ``errors * 1024 <= floor(max_ber * 1024) * bits``.  Integers and bits only.

Three kernels of ``libcough_amd_dups.so`` (``include/cough_amd_dups.h`` states the arithmetic word by word); the one value
the host reads back before the list is the per-clip count of matches, which sizes it.

What it catches, measured on synthetic one-second clips (noise bursts on a -54 dB floor) with the defaults: gain changes
(rate exactly 0), delays of 37 to 400 samples and an advance of 1000 samples (at most 0.19), where unrelated clips read
0.41 at the least.  What it does not catch: re-recordings of the same event, copies under additive noise (0.33 at 30 dB
SNR) and offsets beyond ``max_lag`` frames.  Nothing was measured on real audio: look at ``table.histogram`` of your own
corpus before trusting ``max_ber``.

    python -m cough_detector_amd.duplicates data --max-ber 0.25 --max-lag 8 --top 20
"""
from __future__ import annotations

import ctypes as C
import json
import math
import warnings
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .data import DeviceClipBank, _featurise_rows, _offsets, _stream, _upload
from .segments import _check_device

ROWS, MAX_FRAMES, HIST_BINS, MAX_CLIPS = 33, 256, 65, 65536   # COUGH_DUPS_ROWS / _MAX_FRAMES / _HIST_BINS / _MAX_CLIPS


@dataclass
class Fingerprints:
    """``words`` (n, Tw) int32 on the device -- the 32 bits of a frame, bit k in bit k, held in a signed word --
    ``live`` (n,) int32 on the device, the frames of each clip whose word is not zero, and the ``window``, ``delta`` and
    ``rows`` (33 image rows) they were taken with."""
    words: torch.Tensor
    live: torch.Tensor
    window: int
    delta: int
    rows: Tuple[int, ...]

    def __len__(self) -> int:
        return int(self.words.shape[0])


@dataclass
class DuplicateTable:
    """The matching pairs, sorted by ``(a, b)`` with ``a < b``: ``a``, ``b``, ``lag`` (frame ``t`` of ``a`` met frame
    ``t + lag`` of ``b``), ``errors`` and ``bits`` (int32 numpy arrays); ``counts`` (n,) int32, the matches ``b > a`` of
    every clip; ``histogram`` (65,) int64, ``[(errors * 64) // bits]`` of the best lag of every pair that has one,
    matching or not; ``flat``, the indices of the flat clips (int64); ``n``, the clips compared."""
    a: np.ndarray
    b: np.ndarray
    lag: np.ndarray
    errors: np.ndarray
    bits: np.ndarray
    counts: np.ndarray
    histogram: np.ndarray
    flat: np.ndarray
    n: int

    def __len__(self) -> int:
        return int(self.a.size)

    @property
    def ber(self) -> np.ndarray:
        """``errors / bits`` of every pair (float64)."""
        return self.errors.astype(np.float64) / self.bits.astype(np.float64)


def default_rows(n_mels: int) -> Tuple[int, ...]:
    """33 mel rows spread over ``n_mels`` bands: ``(k * (n_mels - 1)) // 32``."""
    if isinstance(n_mels, bool) or not isinstance(n_mels, (int, np.integer)) or n_mels < ROWS:
        raise ValueError(f"fingerprint_images: n_mels={n_mels!r} must be an integer >= {ROWS} (one bit per pair of 33 rows)")
    return tuple((k * (int(n_mels) - 1)) // 32 for k in range(ROWS))


def _positive(what: str, **values) -> None:
    for name, v in values.items():
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= 2**31 - 1:
            raise ValueError(f"{what}: {name}={v!r} must be a positive integer that fits 32 bits")


def fingerprint_images(images: torch.Tensor, n_mels: int, window: int = 8, delta: int = 8,
                       rows: Optional[Sequence[int]] = None) -> Fingerprints:
    """The fingerprints of ``images`` (n, F, T) float32 on the GPU, whose first ``n_mels`` rows are the mel rows.
    ``rows=None`` takes ``default_rows(n_mels)``; ``T - window + 1 - delta`` must lie in 1..256."""
    what = "fingerprint_images"
    _positive(what, window=window, delta=delta)
    rows = default_rows(n_mels) if rows is None else tuple(int(r) for r in rows)
    if images.dim() != 3 or images.dtype != torch.float32:
        raise ValueError(f"{what}: images must be (n, F, T) float32, got {tuple(images.shape)} {images.dtype}")
    if images.device.type != "cuda":
        raise RuntimeError(f"{what}: the images live on {images.device}; the kernels need them on the GPU (there is no CPU "
                           "fallback)")
    n, f, t = (int(v) for v in images.shape)
    tw = t - int(window) + 1 - int(delta)
    if len(rows) != ROWS or any(r < 0 or r >= f for r in rows):
        raise ValueError(f"{what}: rows must be {ROWS} image rows in 0..{f - 1}, got {rows}")
    if not 1 <= tw <= MAX_FRAMES:
        raise ValueError(f"{what}: T - window + 1 - delta = {tw} must lie in 1..{MAX_FRAMES} (T={t}, window={window}, "
                         f"delta={delta})")
    images = images.contiguous()
    words = torch.empty((n, tw), dtype=torch.int32, device=images.device)
    live = torch.empty(n, dtype=torch.int32, device=images.device)
    if n:                                                        # an empty tensor has no address to pass
        _lib.check_dups(_lib.load_dups().cough_fingerprint_images(
            images.data_ptr(), n, f, t, (C.c_int * ROWS)(*rows), int(window), int(delta), words.data_ptr(), live.data_ptr(),
            _stream(images.device)), "cough_fingerprint_images")
    return Fingerprints(words, live, int(window), int(delta), rows)


def fingerprint_bank(bank: DeviceClipBank, preprocessor, batch_size: int = 4096, **kw) -> Fingerprints:
    """The fingerprints of every clip of ``bank`` as the loader sees it, ``batch_size`` clips at a time;
    ``kw`` as ``fingerprint_images``.  ``preprocessor.n_mels < 33`` raises."""
    what = "fingerprint_bank"
    _positive(what, batch_size=batch_size)
    default_rows(preprocessor.n_mels)
    dev, n = _check_device(what, bank), len(bank)
    parts: List[Fingerprints] = []
    for lo in range(0, n, int(batch_size)):
        hi = min(lo + int(batch_size), n)
        images = _featurise_rows(preprocessor, dev, bank.data, bank.offsets_dev[lo:hi], bank.lengths_dev[lo:hi])
        parts.append(fingerprint_images(images, preprocessor.n_mels, **kw))
    if not parts:
        raise ValueError(f"{what}: the bank holds no clip")
    first = parts[0]
    return Fingerprints(torch.cat([p.words for p in parts]), torch.cat([p.live for p in parts]), first.window, first.delta,
                        first.rows)


def max_err_1024(max_ber: float) -> int:
    """``floor(max_ber * 1024)``: the threshold the matcher compares integers with."""
    if isinstance(max_ber, bool) or not isinstance(max_ber, (int, float, np.integer, np.floating)) or not 0.0 <= max_ber <= 1.0:
        raise ValueError(f"find_duplicates: max_ber={max_ber!r} must lie in 0..1")
    return int(math.floor(float(max_ber) * 1024.0))


def find_duplicates(fp: Fingerprints, max_lag: int = 8, max_ber: float = 0.25, min_live: int = 16) -> DuplicateTable:
    """All pairs of ``fp`` that match (module docstring).  One host read sizes the list (the per-clip counts); the list,
    the histogram and the flat clips are read once the list pass has run.  More than 65536 clips are refused."""
    what = "find_duplicates"
    _positive(what, min_live=min_live)
    if isinstance(max_lag, bool) or not isinstance(max_lag, (int, np.integer)) or not 0 <= max_lag <= 2**31 - 1:
        raise ValueError(f"{what}: max_lag={max_lag!r} must be a non-negative integer that fits 32 bits")
    thr = max_err_1024(max_ber)
    words, live = fp.words, fp.live
    if words.device.type != "cuda":
        raise RuntimeError(f"{what}: the fingerprints live on {words.device}; the kernels need them on the GPU (there is no "
                           "CPU fallback)")
    n, tw = (int(v) for v in words.shape)
    i32 = np.zeros(0, np.int32)
    if n == 0:
        return DuplicateTable(i32, i32, i32, i32, i32, i32, np.zeros(HIST_BINS, np.int64), np.zeros(0, np.int64), 0)
    if n > MAX_CLIPS:
        raise ValueError(f"{what}: {n} clips; the matcher takes at most {MAX_CLIPS} (split the corpus; nothing is truncated)")
    lib, dev = _lib.load_dups(), words.device
    words, live = words.contiguous(), live.contiguous()
    ws_bytes = int(lib.cough_match_workspace_bytes(n, tw))
    ws = torch.empty(ws_bytes // 4, dtype=torch.int32, device=dev)
    counts_dev = torch.empty(n, dtype=torch.int32, device=dev)
    hist = torch.empty(HIST_BINS, dtype=torch.int64, device=dev)
    head = (words.data_ptr(), live.data_ptr(), n, tw, int(max_lag), thr, int(min_live))
    _lib.check_dups(lib.cough_count_matches(*head, counts_dev.data_ptr(), hist.data_ptr(), ws.data_ptr(), ws_bytes,
                                            _stream(dev)), "cough_count_matches")
    counts = counts_dev.cpu().numpy()                            # the one host read: it sizes the list
    row_offsets = _offsets(counts)
    rows = int(row_offsets[-1])
    out = torch.empty((5, max(rows, 1)), dtype=torch.int32, device=dev)
    if rows:
        roffs_dev, _ = _upload(dev, row_offsets, i32)
        _lib.check_dups(lib.cough_list_matches(*head, ws.data_ptr(), ws_bytes, roffs_dev.data_ptr(),
                                               *(out[k].data_ptr() for k in range(5)), _stream(dev)), "cough_list_matches")
    a, b, lag, err, bits = out[:, :rows].cpu().numpy()
    flat = np.flatnonzero(live.cpu().numpy() == 0).astype(np.int64)
    return DuplicateTable(a, b, lag, err, bits, counts, hist.cpu().numpy(), flat, n)


def duplicate_groups(table: DuplicateTable, groups: Optional[Sequence[int]] = None) -> np.ndarray:
    """``(n,)`` int64: the group of every clip, a group's id being its smallest member's index.  Clips are joined by the
    table's pairs; ``groups=`` (one entry per clip, e.g. ``WindowTable.clip`` or ``SegmentTable.clip``) first joins the
    clips of equal entry, so copies of one recording pull their pieces together.  The result is what
    ``prepare_group_split(bank, groups)`` takes."""
    n = int(table.n)
    parent = np.arange(n, dtype=np.int64)

    def find(x: int) -> int:
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root

    def union(x: int, y: int) -> None:
        rx, ry = find(x), find(y)
        if rx != ry:
            parent[max(rx, ry)] = min(rx, ry)                    # the smaller index stays the root

    if groups is not None:
        g = np.asarray(groups.tolist() if isinstance(groups, torch.Tensor) else groups)
        if g.shape != (n,):
            raise ValueError(f"duplicate_groups: groups has shape {g.shape}, the table compares {n} clips")
        first = {}
        for k, name in enumerate(g.tolist()):
            union(first.setdefault(name, k), k)
    for x, y in zip(table.a.tolist(), table.b.tolist()):
        union(x, y)
    return np.array([find(k) for k in range(n)], dtype=np.int64)


def label_conflicts(table: DuplicateTable, labels) -> np.ndarray:
    """The rows of ``table`` (int64 indices into ``table.a`` ...) whose two clips carry different labels, by ascending
    bit error rate (ties in the table's order): the closest copies filed under two classes first."""
    y = np.asarray(labels.tolist() if isinstance(labels, torch.Tensor) else labels)
    if y.shape != (int(table.n),):
        raise ValueError(f"label_conflicts: labels has shape {y.shape}, the table compares {table.n} clips")
    rows = np.flatnonzero(y[table.a] != y[table.b]).astype(np.int64)
    return rows[np.argsort(table.ber[rows], kind="stable")]


def drop_duplicates(bank: DeviceClipBank, table: DuplicateTable) -> Tuple[DeviceClipBank, np.ndarray]:
    """``(bank.subset(kept), kept)``: the first clip of every group of ``duplicate_groups(table)``, in the bank's order.
    A group that holds a label conflict is left whole -- which copy is right is for a listener to say -- and named in a
    warning."""
    if len(bank) != int(table.n):
        raise ValueError(f"drop_duplicates: the bank holds {len(bank)} clips, the table compares {table.n}")
    group = duplicate_groups(table)
    disputed = sorted({int(group[table.a[r]]) for r in label_conflicts(table, bank.labels)})
    if disputed:
        warnings.warn(f"drop_duplicates: {len(disputed)} group(s) hold copies under both labels and are kept whole: groups "
                      f"{disputed}", stacklevel=2)
    kept = np.flatnonzero((group == np.arange(len(group))) | np.isin(group, disputed)).astype(np.int64)
    return bank.subset(kept.tolist()), kept


def main(argv=None) -> dict:
    import argparse

    from .audit import bank_files
    from .preprocessing import AudioPreprocessor
    from . import train as _train

    ap = argparse.ArgumentParser(prog="python -m cough_detector_amd.duplicates", description=__doc__.split("\n\n")[0])
    ap.add_argument("data_dir", help="directory with non_cough/ and cough/ WAVE files")
    ap.add_argument("--max-ber", type=float, default=0.25)
    ap.add_argument("--max-lag", type=int, default=8)
    ap.add_argument("--min-live", type=int, default=16)
    ap.add_argument("--top", type=int, default=20, help="how many conflicts and groups to print")
    args = ap.parse_args(argv)
    pre = AudioPreprocessor(device="cuda", **_train.preprocessor_config())
    files = bank_files(args.data_dir)
    bank = DeviceClipBank.from_directory(args.data_dir, pre)
    if len(files) != len(bank):
        raise RuntimeError(f"{args.data_dir} changed while it was read: {len(files)} files, {len(bank)} clips")
    table = find_duplicates(fingerprint_bank(bank, pre), max_lag=args.max_lag, max_ber=args.max_ber, min_live=args.min_live)
    conflicts = label_conflicts(table, bank.labels)
    for r in conflicts[:max(args.top, 0)].tolist():
        print(f"conflict  ber {table.ber[r]:.3f}  lag {int(table.lag[r]):+d}  {files[table.a[r]]}  {files[table.b[r]]}")
    group = duplicate_groups(table)
    ids, sizes = np.unique(group, return_counts=True)
    order = np.argsort(-sizes, kind="stable")
    for g in order[:max(args.top, 0)].tolist():
        if sizes[g] > 1:
            print(f"group of {int(sizes[g])}: " + "  ".join(files[k] for k in np.flatnonzero(group == ids[g]).tolist()))
    report = dict(n=int(table.n), pairs=len(table), groups=int((sizes > 1).sum()), largest=int(sizes.max()) if sizes.size else 0,
                  conflicts=int(conflicts.size), flat=int(table.flat.size), histogram=table.histogram.tolist())
    print(json.dumps(report))
    return report


if __name__ == "__main__":
    main()
