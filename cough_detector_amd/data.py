"""The reference's dataset module (``/root/reference/src/dataset.py``) with the whole input pipeline on the MI355X.

* ``DeviceClipBank``: what ``CoughDataset`` (:22-173) holds -- the clips of a ``non_cough`` / ``cough`` directory tree,
  resampled and averaged to mono, with its ``class_counts`` and ``sample_weights`` -- packed into ONE device buffer.  A
  cough corpus is thousands of short clips at 64 KB per second of audio: it fits in HBM many times over.
* ``DeviceDataLoader``: what a ``DataLoader`` over that dataset yields, ``(features (B, 1, F, T), targets (B,))`` on the
  device, a batch per five launches instead of a clip per ``__getitem__``: ``cough_gather_rows`` (ragged clips -> a
  matrix), ``cough_augment_waveforms``, ``cough_prepare_rows`` (``normalize`` -> ``pad_or_trim``; the peak is that of the
  whole augmented clip, before the trim, as in :158-160), the featuriser, ``cough_mask_images`` (SpecAugment with a
  coin and masks per item, :169-171).  The three new kernels live in ``libcough_amd_data.so``
  (``include/cough_amd_data.h``).
* ``create_data_loaders`` (:368-418): the ``WeightedRandomSampler`` / ``drop_last=True`` training loader and the
  sequential validation loader.
* ``stratified_split`` / ``prepare_dataset_split`` (:421-483): the stratified 80 / 20 split of a directory's clips, the
  indices scikit-learn's ``train_test_split`` gives, drawn in numpy.  ``DeviceClipBank.from_esc50`` / ``esc50_rows``:
  ``ESC50Dataset`` (:176-264); ``DeviceClipBank.concat``: ``CombinedDataset`` (:299-330).  Host bookkeeping around the
  bank; ``cough_detector_amd/train.py`` assembles them.

The random draws are the reference's, in the order a ``num_workers=0`` loader makes them: the sampler's indices for the
epoch, then item by item in batch order the augmentor's draws for that clip's length, its ``torch.randn`` when the
gaussian step fired (``noise="host"``), SpecAugment's coin and, when it fired, its masks.  All of them are host draws;
everything else is stream-ordered device work, so drawing batch k + 1 overlaps the kernels of batch k.

Differences a caller can observe: WAVE files only (``load_audio``); ``noise="device"`` (the default) draws the gaussian
noise with the seeded counter-based generator of ``cough_augment_waveforms`` instead of ``torch.randn``;
``cache_features`` keeps the unmasked features of the whole bank in one device tensor and is refused when a waveform
augmentation could run (the reference's ``cache_spectrograms`` would silently freeze the first epoch's augmentation).

``draws="device"`` moves every per-item draw to the device as well (``cough_detector_amd/draws.py``): the host draws the
epoch's indices and ONE seed per epoch, and a batch is four launches -- draw, augment the rows in place in the bank,
``cough_prepare_rows``, the featuriser -- plus ``cough_mask_images`` when there are masks.  The draws then have the
reference's distributions but are not its random stream (the masks are drawn in float64, the reference's in float32).

``mixup=MixUp(alpha)`` mixes every training batch with a permutation of itself after the features and the SpecAugment
masks (one more launch, ``cough_mix_batch``), and the loader then yields ``(features, soft targets (B, 2) float32)``,
which the trainers' soft-target steps, ``train_epoch_async`` and ``fit`` take as they are.

An ``AudioAugmentor`` with ``speed=True``, ``pitch=True``, a ``reverb`` or a ``channel`` bank adds that step's launches
to a training batch: ``cough_warp_rows``; ``cough_stretch_rows`` and ``cough_warp_rows``; ``cough_reverb_rows``; and,
behind the augmentation kernel, ``cough_channel_rows``.  The first of them reads the clips in place from the bank and
applies the time shift; the rest of the batch works on the rows' new lengths ``n'``.  With ``draws="host"`` the plans
travel with the batch's pinned upload, and a batch in which a step's coin never fired runs the launches it ran before;
with ``draws="device"`` the plans are drawn on the device first, the rows are as wide as the slowest speed factor can
make the longest one, and nothing is read back.  The loader names none of these steps: the chain lives in
``cough_detector_amd/chain.py``; a new step is added there, in the augmentor's one draw method, and as a ``BatchPlan`` column.
"""
from __future__ import annotations

import csv
import math
import random
import warnings
from pathlib import Path
from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch.utils.data import RandomSampler, WeightedRandomSampler

from . import _lib
from . import chain as _chain
from ._native import _stream, cuda_device
from .augmentation import AudioAugmentor, MixUp, SpecAugment, mask_images, mix_batch_rows, mix_coefficients

CLASSES = ["non_cough", "cough"]
_AUDIO_EXTENSIONS = {".wav", ".mp3", ".flac", ".ogg", ".webm"}      # dataset.py:86
ESC50_COUGH_CLASS = 24                                              # "coughing" (dataset.py:185)
ESC50_NEGATIVE_CLASSES = (20, 21, 22, 23, 25, 26, 38)               # the sounds closest to a cough (dataset.py:188-196)


def _approximate_mode(counts: np.ndarray, n_draws: int, rng: np.random.RandomState) -> np.ndarray:
    """How many of ``n_draws`` each class gets: the floor of its proportional share, the remainder handed out by
    descending fractional part, ties broken by ``rng.choice(..., replace=False)`` (one call per distinct fraction)."""
    share = counts / counts.sum() * n_draws
    taken = np.floor(share)
    left = int(n_draws - taken.sum())
    if left > 0:
        frac = share - taken
        for value in np.unique(frac)[::-1]:
            inds, = np.where(frac == value)
            k = min(len(inds), left)
            taken[rng.choice(inds, size=k, replace=False)] += 1
            left -= k
            if left == 0:
                break
    return taken.astype(int)


def stratified_split(labels: Sequence[int], val_split: float = 0.2, random_state: int = 42) -> Tuple[List[int], List[int]]:
    """``(train_idx, val_idx)`` of ``sklearn.model_selection.train_test_split(range(n), test_size=val_split,
    random_state=random_state, stratify=labels)`` (dataset.py:454-459), index for index and in its order, in numpy:
    ``ceil(val_split * n)`` clips go to validation; each class is allotted its share of both sides (``_approximate_mode``,
    training first, then validation from what the class has left), permuted, and cut; both lists are permuted once
    more.  All draws come from one ``np.random.RandomState(random_state)``.  Inputs that scikit-learn refuses raise
    ``ValueError``: a ``val_split`` outside (0, 1), a class with a single member, a side smaller than the number of
    classes."""
    y = np.asarray(labels.tolist() if isinstance(labels, torch.Tensor) else labels)
    if y.ndim != 1:
        raise ValueError(f"stratified_split: labels must be one-dimensional, got shape {y.shape}")
    n = int(y.shape[0])
    if isinstance(val_split, bool) or not isinstance(val_split, (float, np.floating)) or not 0.0 < val_split < 1.0:
        raise ValueError(f"stratified_split: val_split={val_split!r} must be a float in the (0, 1) range")
    n_test = int(math.ceil(val_split * n))
    n_train = n - n_test
    if n_train <= 0:
        raise ValueError(f"stratified_split: with {n} clip(s) and val_split={val_split} the training side is empty")
    classes, y_idx = np.unique(y, return_inverse=True)
    counts = np.bincount(y_idx)
    if counts.min() < 2:
        raise ValueError(f"stratified_split: class {classes[int(counts.argmin())]!r} has a single member; a stratified "
                         "split needs at least 2 of every class")
    for side, size in (("training", n_train), ("validation", n_test)):
        if size < len(classes):
            raise ValueError(f"stratified_split: the {side} side would hold {size} clip(s) for {len(classes)} classes; "
                             "it needs at least one per class")
    by_class = np.split(np.argsort(y_idx, kind="mergesort"), np.cumsum(counts)[:-1])
    rng = np.random.RandomState(random_state)
    n_i = _approximate_mode(counts, n_train, rng)
    t_i = _approximate_mode(counts - n_i, n_test, rng)
    train, test = [], []
    for c, members in enumerate(by_class):
        members = members[rng.permutation(int(counts[c]))]
        train.extend(members[:n_i[c]])
        test.extend(members[n_i[c]:n_i[c] + t_i[c]])
    train = rng.permutation(np.asarray(train, dtype=np.int64))
    test = rng.permutation(np.asarray(test, dtype=np.int64))
    return [int(i) for i in train], [int(i) for i in test]


def stratified_group_split(labels: Sequence[int], groups: Sequence[int], val_split: float = 0.2,
                           random_state: int = 42) -> Tuple[List[int], List[int]]:
    """``(train_idx, val_idx)`` of a split that keeps every group on one side: for clips cut from recordings
    (``groups=table.clip`` of a ``WindowTable`` or ``SegmentTable``), pieces of one recording never land on both
    sides.  The groups are taken in ``np.unique`` order, each with the label its members share (two different labels
    in one group raise ``ValueError``); those labels go through ``stratified_split(group_labels, val_split,
    random_state)`` unchanged, so ``val_split`` is a share of the groups.  Each side is its groups in the order
    ``stratified_split`` returned them, the members of a group in ascending index."""
    y = np.asarray(labels.tolist() if isinstance(labels, torch.Tensor) else labels)
    g = np.asarray(groups.tolist() if isinstance(groups, torch.Tensor) else groups)
    if y.ndim != 1 or g.shape != y.shape:
        raise ValueError(f"stratified_group_split: labels and groups must be one-dimensional and of one length, got "
                         f"shapes {y.shape} and {g.shape}")
    names, member_of = np.unique(g, return_inverse=True)
    order = np.argsort(member_of, kind="mergesort")               # members of a group in ascending index
    members = np.split(order, np.cumsum(np.bincount(member_of, minlength=len(names)))[:-1]) if len(names) else []
    group_labels = []
    for name, idx in zip(names.tolist(), members):
        if (y[idx] != y[idx[0]]).any():
            raise ValueError(f"stratified_group_split: group {name!r} holds clips of different labels "
                             f"({sorted(set(y[idx].tolist()))}); a group is one recording and has one label")
        group_labels.append(y[idx[0]])
    train_groups, val_groups = stratified_split(group_labels, val_split=val_split, random_state=random_state)
    return ([int(i) for k in train_groups for i in members[k]], [int(i) for k in val_groups for i in members[k]])


def esc50_rows(csv_path, is_training: bool = True, fold: Optional[int] = None,
               include_all_negatives: bool = True) -> List[Tuple[str, int]]:
    """``[(filename, label)]`` of ``ESC50Dataset`` (dataset.py:227-264) from ``meta/esc50.csv``, in csv order: with
    ``fold`` set, training keeps the rows of the other folds and validation the rows of that fold; rows whose
    ``audio/<filename>`` (beside ``meta/``) does not exist are skipped; target 24 ("coughing") is labelled 1, any other
    target 0 when ``include_all_negatives`` is set or the target is one of ``ESC50_NEGATIVE_CLASSES``, else dropped."""
    csv_path = Path(csv_path)
    if not csv_path.exists():
        raise FileNotFoundError(f"ESC-50 metadata not found at {csv_path}; nothing here downloads it: put a checkout of "
                                "ESC-50 (meta/esc50.csv, audio/*.wav) there or pass its directory as esc50_dir")
    audio_dir = csv_path.parent.parent / "audio"
    rows = []
    with open(csv_path, newline="") as f:
        for row in csv.DictReader(f):
            if fold is not None and (int(row["fold"]) != int(fold)) != bool(is_training):
                continue
            if not (audio_dir / row["filename"]).exists():
                continue
            target = int(row["target"])
            if target == ESC50_COUGH_CLASS:
                rows.append((row["filename"], 1))
            elif include_all_negatives or target in ESC50_NEGATIVE_CLASSES:
                rows.append((row["filename"], 0))
    return rows


def _upload(dev: torch.device, i64: np.ndarray, i32: np.ndarray) -> Tuple[torch.Tensor, torch.Tensor]:
    """One host-to-device copy of an int64 and an int32 array through pinned memory, without waiting for it: torch's
    pinned allocator hands the staging block out again only once the copy has run."""
    n64, n32 = int(i64.size), int(i32.size)
    host = torch.empty(max(n64 * 8 + n32 * 4, 1), dtype=torch.uint8, pin_memory=True)
    raw = host.numpy()
    raw[:n64 * 8].view(np.int64)[:] = i64
    raw[n64 * 8:n64 * 8 + n32 * 4].view(np.int32)[:] = i32
    d = host.to(dev, non_blocking=True)
    return d[:n64 * 8].view(torch.int64), d[n64 * 8:n64 * 8 + n32 * 4].view(torch.int32)


def _offsets(counts) -> np.ndarray:
    """int64 ``[n + 1]``: 0, then the running sum of ``counts`` (an array, a host tensor or a list of n >= 0 counts)."""
    return np.concatenate([[0], np.cumsum(np.asarray(counts), dtype=np.int64)]).astype(np.int64)


def _owner(counts) -> np.ndarray:
    """int64 ``[total]``: the row of every element when row ``k`` holds ``counts[k]`` of them, row after row."""
    return np.repeat(np.arange(len(counts), dtype=np.int64), np.asarray(counts, dtype=np.int64))


def _ragged(counts) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``(offsets, owner, rank)``: ``_offsets(counts)``, ``_owner(counts)`` and every element's place within its row (int64)."""
    offsets, owner = _offsets(counts), _owner(counts)
    return offsets, owner, np.arange(owner.size, dtype=np.int64) - offsets[:-1][owner]


def mix_draws(seed: int, b: int, alpha: float) -> Tuple[np.ndarray, np.ndarray]:
    """``(perm int32 (b,), lam float64 (b,))`` of a ``draws="device"`` batch: a permutation, then ``Beta(alpha, alpha)``
    variates, from ``numpy.random.Generator(Philox(key=seed mod 2^64))`` on the host."""
    rng = np.random.Generator(np.random.Philox(key=int(seed) & (2**64 - 1)))
    perm = rng.permutation(b).astype(np.int32)
    return perm, rng.beta(alpha, alpha, size=b)


_TORCH_DTYPE = {np.float32: torch.float32, np.uint8: torch.uint8}


class UploadWords:
    """The int32 side of a batch's pinned upload (``_upload``), assembled by name: ``add`` appends an array of 4-byte
    words (int32, float32, or bytes in fours), behind one word of padding if it has to start on an 8-byte boundary;
    ``array`` is what travels; ``view`` is an array again, dtype and shape, cut out of the uploaded tensor.  ``lengths``:
    a flat int32 array that every batch leads with, under that name."""

    def __init__(self, lengths: Optional[np.ndarray] = None):
        self._parts: List[np.ndarray] = []
        self._at: Dict[str, tuple] = {}                  # name -> (first word, end, torch dtype, shape); None: as it is
        self.size = 0
        if lengths is not None:
            self._parts.append(lengths)
            self.size = lengths.size
            self._at["lengths"] = (0, self.size, None, None)

    def add(self, name: str, array: np.ndarray, align8: bool = False) -> None:
        words = array.reshape(-1)
        if words.dtype != np.int32:
            words = words.view(np.int32)
        if align8 and self.size & 1:
            self._parts.append(np.zeros(1, np.int32))
            self.size += 1
        self._at[name] = (self.size, self.size + words.size, None if array.dtype == np.int32 else _TORCH_DTYPE[array.dtype.type],
                          array.shape if array.ndim > 1 else None)
        self._parts.append(words)
        self.size += words.size

    def __contains__(self, name: str) -> bool:
        return name in self._at

    def at(self, name: str) -> int:
        """The word offset of the array ``name``."""
        return self._at[name][0]

    def array(self) -> np.ndarray:
        return self._parts[0] if len(self._parts) == 1 else np.concatenate(self._parts or [np.zeros(0, np.int32)])

    def view(self, i32: torch.Tensor, name: str) -> torch.Tensor:
        lo, hi, dtype, shape = self._at[name]
        words = i32[lo:hi] if dtype is None else i32[lo:hi].view(dtype)
        return words if shape is None else words.view(shape)


class DeviceClipBank:
    """Mono float32 clips of any lengths >= 1, packed end to end into one buffer ``data`` on ``device``; clip k is
    ``data[offsets[k] : offsets[k] + lengths[k]]`` with label ``labels[k]`` (0 = non_cough, 1 = cough).  ``offsets``
    (int64), ``lengths`` (int32) and ``labels`` (int64) are host tensors, ``offsets_dev`` / ``lengths_dev`` /
    ``labels_dev`` their device copies."""

    classes = CLASSES

    def __init__(self, waveforms: Sequence, labels: Sequence[int], device=None):
        clips = []
        for k, w in enumerate(waveforms):
            t = torch.as_tensor(w)
            if not t.dtype.is_floating_point:
                raise TypeError(f"DeviceClipBank: clip {k} is {t.dtype}; expected floating-point samples")
            if t.dim() == 2 and t.shape[0] == 1:
                t = t[0]
            if t.dim() != 1 or t.numel() < 1:
                raise ValueError(f"DeviceClipBank: clip {k} has shape {tuple(t.shape)}; expected (n,) or (1, n) mono "
                                 "samples, n >= 1")
            clips.append(t.detach().to("cpu", torch.float32))
        labels = [int(v) for v in (labels.tolist() if isinstance(labels, torch.Tensor) else labels)]
        if len(labels) != len(clips):
            raise ValueError(f"DeviceClipBank: {len(clips)} clips but {len(labels)} labels")
        if any(v not in (0, 1) for v in labels):
            raise ValueError("DeviceClipBank: labels are 0 (non_cough) or 1 (cough)")
        lengths = [int(c.numel()) for c in clips]
        if lengths and max(lengths) > 2**31 - 1:
            raise ValueError("DeviceClipBank: a clip is longer than 2^31 - 1 samples")
        packed = torch.cat(clips) if clips else torch.zeros(0, dtype=torch.float32)
        data = packed.to(torch.device(device) if device is not None else cuda_device())
        self.device = data.device                # where the data lives: "cuda" has become the current GPU
        self._set(data, lengths, labels)

    def _set(self, data: torch.Tensor, lengths: Sequence[int], labels: Sequence[int]) -> None:
        self.data = data
        self.lengths = torch.tensor(lengths, dtype=torch.int32)
        self.offsets = torch.tensor(_offsets(lengths)[:-1], dtype=torch.int64)
        self.labels = torch.tensor(labels, dtype=torch.int64)
        self.offsets_dev = self.offsets.to(self.device)
        self.lengths_dev = self.lengths.to(self.device)
        self.labels_dev = self.labels.to(self.device)

    @classmethod
    def from_packed(cls, data: torch.Tensor, lengths: Sequence[int], labels: Sequence[int]) -> "DeviceClipBank":
        """The bank of samples that are packed already: ``data`` (1-D contiguous float32, where the bank is to live) holds
        clips of ``lengths`` end to end.  Only what the host knows is checked; nothing is read from the device."""
        lengths, labels = np.asarray(lengths, dtype=np.int64).reshape(-1), np.asarray(labels, dtype=np.int64).reshape(-1)
        if data.dim() != 1 or data.dtype != torch.float32:
            raise ValueError(f"DeviceClipBank.from_packed: data is {data.dtype} {tuple(data.shape)}, not one-dimensional float32")
        if lengths.size != labels.size:
            raise ValueError(f"DeviceClipBank.from_packed: {lengths.size} lengths but {labels.size} labels")
        if int(lengths.sum()) != data.numel():
            raise ValueError(f"DeviceClipBank.from_packed: lengths of {int(lengths.sum())} samples, data of {data.numel()}")
        out = object.__new__(cls)
        out.device = data.device
        out._set(data, lengths, labels)
        return out

    def cut(self, clips: np.ndarray, starts, lengths: np.ndarray, labels: Optional[Sequence[int]] = None) -> "DeviceClipBank":
        """A bank of spans of this one's clips: row ``j`` is samples ``starts[j] .. starts[j] + lengths[j]`` of clip
        ``clips[j]`` (host int64), labelled ``labels[j]`` or, without ``labels``, as that clip.  ``starts``: an int32 tensor
        on the bank's device or a host array; ``lengths``: a host array of entries >= 1; the caller sees to it that every
        span lies inside its clip.  One upload and one launch (``cough_copy_segments``), none without rows; no waiting."""
        if self.device.type != "cuda":
            raise RuntimeError(f"DeviceClipBank.cut: the bank lives on {self.device}; the kernels need it on the GPU (there "
                               "is no CPU fallback)")
        clips, lengths = np.asarray(clips, dtype=np.int64), np.asarray(lengths)
        dev, r = self.device, int(clips.size)
        out = self.from_packed(torch.empty(int(lengths.sum()), dtype=torch.float32, device=dev), lengths,
                               self.labels.numpy()[clips] if labels is None else labels)
        if r:
            on_host = not isinstance(starts, torch.Tensor)
            i64, i32 = _upload(dev, np.concatenate([self.offsets.numpy()[clips], out.offsets.numpy()]),
                               np.asarray(starts).astype(np.int32) if on_host else np.zeros(0, np.int32))
            _lib.check_segments(_lib.load_segments().cough_copy_segments(
                self.data.data_ptr(), i64[:r].data_ptr(), (i32 if on_host else starts).data_ptr(), out.lengths_dev.data_ptr(),
                i64[r:].data_ptr(), r, int(lengths.max()), out.data.data_ptr(), _stream(dev)), "cough_copy_segments")
        return out

    def __len__(self) -> int:
        return int(self.labels.numel())

    @property
    def class_counts(self) -> Dict[int, int]:
        """{0: clips labelled non_cough, 1: clips labelled cough} (dataset.py:102-107)."""
        counts = {i: 0 for i in range(len(CLASSES))}
        for v in self.labels.tolist():
            counts[v] += 1
        return counts

    @property
    def sample_weights(self) -> torch.Tensor:
        """``total / (2 * class_counts[label])`` per clip (dataset.py:109-116): what ``WeightedRandomSampler`` takes."""
        counts, total = self.class_counts, len(self)
        return torch.tensor([total / (len(CLASSES) * counts[v]) for v in self.labels.tolist()])

    def clip(self, k: int) -> torch.Tensor:
        """Clip ``k`` as a (1, n) view of the device buffer."""
        o, n = int(self.offsets[k]), int(self.lengths[k])
        return self.data[o:o + n].unsqueeze(0)

    def subset(self, indices: Sequence[int]) -> "DeviceClipBank":
        """A bank of the clips ``indices`` in that order (a train / validation split), on the same device."""
        idx = [int(i) for i in (indices.tolist() if isinstance(indices, torch.Tensor) else indices)]
        n = len(self)
        if any(i < -n or i >= n for i in idx):
            raise IndexError(f"DeviceClipBank.subset: indices must lie in 0..{n - 1}")
        parts = [self.clip(i)[0] for i in idx]
        data = torch.cat(parts) if parts else torch.zeros(0, dtype=torch.float32, device=self.device)
        return DeviceClipBank.from_packed(data, [int(self.lengths[i]) for i in idx], [int(self.labels[i]) for i in idx])

    @classmethod
    def from_directory(cls, data_dir: str, preprocessor, device=None) -> "DeviceClipBank":
        """The clips ``CoughDataset`` collects (dataset.py:83-100): ``data_dir/non_cough`` then ``data_dir/cough``, the
        files of each in directory order, read with ``preprocessor.load_audio``, ``resample`` and ``to_mono``.  WAVE
        files only: files with one of the reference's other suffixes are skipped, with one warning naming the count."""
        root = Path(data_dir)
        waveforms, labels, skipped = [], [], 0
        for label, class_name in enumerate(CLASSES):
            class_dir = root / class_name
            if not class_dir.exists():
                warnings.warn(f"DeviceClipBank: class directory {class_dir} not found", stacklevel=2)
                continue
            for audio_file in class_dir.iterdir():
                suffix = audio_file.suffix.lower()
                if suffix not in _AUDIO_EXTENSIONS:
                    continue
                if suffix != ".wav":
                    skipped += 1
                    continue
                waveform, sr = preprocessor.load_audio(str(audio_file))
                waveform = preprocessor.to_mono(preprocessor.resample(waveform, sr))
                waveforms.append(waveform.cpu())
                labels.append(label)
        if skipped:
            warnings.warn(f"DeviceClipBank: skipped {skipped} audio file(s) that are not WAVE files; this build decodes "
                          "WAVE only", stacklevel=2)
        return cls(waveforms, labels, device=device)

    @classmethod
    def concat(cls, banks: Sequence["DeviceClipBank"]) -> "DeviceClipBank":
        """What ``CombinedDataset`` (dataset.py:299-330) is to its datasets: one bank of the clips of ``banks``, bank
        after bank in their order, packed with one ``torch.cat`` where the banks live (no host round trip).  The banks
        share a device; no banks give an empty bank on the default device."""
        banks = list(banks)
        if not banks:
            return cls([], [])
        devices = {b.data.device for b in banks}
        if len(devices) != 1:
            raise ValueError(f"DeviceClipBank.concat: the banks live on {sorted(str(d) for d in devices)}; they must "
                             "share one device")
        return cls.from_packed(torch.cat([b.data for b in banks]), [n for b in banks for n in b.lengths.tolist()],
                               [v for b in banks for v in b.labels.tolist()])

    @classmethod
    def from_esc50(cls, data_dir: str, preprocessor, is_training: bool = True, fold: Optional[int] = None,
                   include_all_negatives: bool = True, device=None) -> "DeviceClipBank":
        """The clips ``ESC50Dataset`` collects (dataset.py:176-264) from an ESC-50 checkout at ``data_dir``: the rows
        ``esc50_rows(data_dir/meta/esc50.csv, is_training, fold, include_all_negatives)`` in csv order, each
        ``audio/<filename>`` read with ``preprocessor.load_audio``, ``resample`` (ESC-50 is 44.1 kHz: ``cough_resample``)
        and ``to_mono``.  ``download_esc50`` has no counterpart: a missing csv raises ``FileNotFoundError`` that says
        where the checkout belongs."""
        root = Path(data_dir)
        waveforms, labels = [], []
        for filename, label in esc50_rows(root / "meta" / "esc50.csv", is_training, fold, include_all_negatives):
            waveform, sr = preprocessor.load_audio(str(root / "audio" / filename))
            waveforms.append(preprocessor.to_mono(preprocessor.resample(waveform, sr)).cpu())
            labels.append(label)
        return cls(waveforms, labels, device=device)


def prepare_dataset_split(data_dir_or_bank, preprocessor=None, val_split: float = 0.2, random_state: int = 42,
                          device=None) -> Tuple[DeviceClipBank, DeviceClipBank]:
    """``(train_bank, val_bank)`` as the reference's ``prepare_dataset_split`` (dataset.py:421-483): the clips of a
    directory (``DeviceClipBank.from_directory(data_dir, preprocessor, device)``) or of a bank that exists already,
    split by ``stratified_split(bank.labels, val_split, random_state)``.  The augmentors are not arguments: they belong
    to the loader (``create_data_loaders``), not to the bank.  For clips cut from recordings see
    ``prepare_group_split``."""
    bank = data_dir_or_bank
    if not isinstance(bank, DeviceClipBank):
        if preprocessor is None:
            raise ValueError("prepare_dataset_split: reading a directory needs a preprocessor")
        bank = DeviceClipBank.from_directory(str(bank), preprocessor, device=device)
    train_idx, val_idx = stratified_split(bank.labels, val_split=val_split, random_state=random_state)
    return bank.subset(train_idx), bank.subset(val_idx)


def prepare_group_split(bank: DeviceClipBank, groups: Sequence[int], val_split: float = 0.2,
                        random_state: int = 42) -> Tuple[DeviceClipBank, DeviceClipBank]:
    """``(train_bank, val_bank)`` of a bank of clips cut from recordings: ``prepare_dataset_split`` with
    ``stratified_group_split(bank.labels, groups, val_split, random_state)`` in the place of ``stratified_split``, so a
    recording stays on one side.  ``groups`` has one entry per clip: ``table.clip`` of ``slice_bank`` or
    ``extract_segments``.  (A function of its own because ``prepare_dataset_split`` keeps the reference's argument
    list.)"""
    train_idx, val_idx = stratified_group_split(bank.labels, groups, val_split=val_split, random_state=random_state)
    return bank.subset(train_idx), bank.subset(val_idx)


def _featurise_rows(pre, dev: torch.device, src: torch.Tensor, offsets: torch.Tensor, lens: torch.Tensor) -> torch.Tensor:
    """Features (B, F, T) of B rows of the flat buffer ``src`` as the loader sees them: ``cough_prepare_rows`` (centre
    crop / zero pad to ``segment_samples``, peak-normalised), then the featuriser.  The loader and the duplicate search
    (``duplicates.fingerprint_bank``) both judge a clip by this image."""
    b = lens.numel()
    seg = torch.empty((b, pre.segment_samples), dtype=torch.float32, device=dev)
    _lib.check_data(_lib.load_data().cough_prepare_rows(src.data_ptr(), offsets.data_ptr(), lens.data_ptr(), b,
                                                        seg.data_ptr(), pre.segment_samples, _lib.PREP_NORMALIZE,
                                                        _stream(dev)), "cough_prepare_rows")
    return pre.featurize_batch(seg, normalize=False)


class BatchPlan:
    """The host draws of one batch: ``clips`` (a ``CoughAugClip`` per item, or None without waveform augmentation),
    ``gaussian`` (the ``torch.randn`` rows of ``noise="host"``, or None), ``seed`` (the device generator's) and ``masks``
    (per item the ``[(axis, start, end)]`` of SpecAugment, empty when its coin did not fire; None without it); with a
    ``MixUp``, ``perm`` (the batch's ``torch.randperm``) and ``lam`` (its float64 λ), else None.  One column per optional
    step of the augmentor (``chain.columns``), None as a whole when the step is switched off and None at an item whose
    coin did not fire: ``pairs`` (the speed step's ``(orig, new)``) with ``new_lengths`` (per item ``n'``; ``gaussian``
    rows then hold ``n'`` samples), ``steps`` (the pitch step's semitones), ``rirs`` (the reverb step's response) and
    ``channels`` (the channel step's ``(filter, clip_ratio)``)."""

    __slots__ = ("clips", "gaussian", "seed", "masks", "perm", "lam", "pairs", "new_lengths", "steps", "rirs", "channels")

    def __init__(self, clips=None, gaussian=None, seed=0, masks=None, perm=None, lam=None, pairs=None, new_lengths=None,
                 steps=None, rirs=None, channels=None):
        self.clips, self.gaussian, self.seed, self.masks = clips, gaussian, seed, masks
        self.perm, self.lam = perm, lam
        self.pairs, self.new_lengths = pairs, new_lengths
        self.steps, self.rirs, self.channels = steps, rirs, channels

    def mics(self) -> bool:
        """Whether a channel step fired in this batch."""
        return self.channels is not None and any(c is not None for c in self.channels)

    def reverbs(self) -> bool:
        """Whether a reverb step fired in this batch."""
        return self.rirs is not None and any(r is not None for r in self.rirs)

    def pitches(self) -> bool:
        """Whether a pitch step fired (with semitones other than 0) in this batch."""
        return self.steps is not None and any(self.steps)

    def warps(self) -> bool:
        """Whether a speed step fired in this batch."""
        return self.pairs is not None and any(p is not None for p in self.pairs)


class DeviceDataLoader:
    """Batches of a ``DeviceClipBank`` as ``(features (B, 1, F, T) float32, targets (B,) int64)`` on the bank's device,
    ready for ``trainer.step``, ``train_epoch_async``, ``validate`` and ``fit``.  Iterating it anew is a new epoch.

    Indices: training with ``use_weighted_sampler`` visits ``WeightedRandomSampler(bank.sample_weights, len(bank), True,
    generator=generator)``, training without it ``RandomSampler(range(n), generator=generator)``; otherwise the order is
    sequential.  ``drop_last`` defaults to ``is_training``.  The augmentors run only when ``is_training``.
    ``noise``: where the gaussian step's noise comes from (``AudioAugmentor.augment_batch``); with ``"device"`` one
    Philox seed is drawn per batch from torch's CPU generator, after the batch's per-item draws.
    ``cache_features``: featurise the bank once (unmasked) and gather later batches from that tensor; refused when a
    waveform augmentation can run.
    ``draws``: ``"host"`` (the default) makes the per-item draws on the host, in the reference's order, as described
    above.  ``"device"`` makes them on the device (needs ``noise="device"``): after the epoch's indices, ``__iter__``
    draws one ``epoch_seed`` from ``generator`` (kept as ``last_epoch_seed``), and batch k draws its records, its masks
    and its gaussian noise under ``(epoch_seed + k) mod 2^64`` in ``launch_batch_drawn``; no per-clip Python runs and
    nothing is copied from pageable memory.  These draws have the reference's distributions, not its random stream
    (float64 masks where the reference draws float32): a seeded run repeats itself, not a reference loader.  A loader that
    has nothing to draw (no augmentor, or not training) behaves the same in both modes.
    ``mixup``: a ``MixUp``; a training loader then mixes every batch with a permutation of itself, after the features
    and the SpecAugment masks, in one launch (``cough_mix_batch``) and yields ``(features, soft targets (B, 2) float32)``
    instead of class indices; a batch of 1 mixes with itself.  With ``draws="host"`` the loader draws, after the batch's
    per-item draws (and its noise seed), ``torch.randperm(B)`` and then ``np.random.beta(alpha, alpha, size=B)``:
    ``MixUp.mix_batch``'s order.  With ``draws="device"`` the permutation and the λ of batch k come from
    ``mix_draws((epoch_seed + k) mod 2^64, B, alpha)``, a Philox-keyed numpy generator ON THE HOST: drawing Beta variates
    and a permutation on the device is out of scope.  In both modes they travel with the batch's index upload through
    pinned memory, and nothing is read back.  A validation loader (``is_training=False``) never mixes."""

    def __init__(self, bank: DeviceClipBank, preprocessor, batch_size: int = 32,
                 audio_augmentor: Optional[AudioAugmentor] = None, spec_augmentor: Optional[SpecAugment] = None,
                 is_training: bool = True, use_weighted_sampler: bool = True, drop_last: Optional[bool] = None,
                 generator: Optional[torch.Generator] = None, noise: str = "device", cache_features: bool = False,
                 draws: str = "host", mixup: Optional[MixUp] = None):
        if batch_size < 1:
            raise ValueError(f"DeviceDataLoader: batch_size={batch_size} must be positive")
        if noise not in ("device", "host"):
            raise ValueError(f"DeviceDataLoader: noise must be 'device' or 'host', got {noise!r}")
        if draws not in ("device", "host"):
            raise ValueError(f"DeviceDataLoader: draws must be 'device' or 'host', got {draws!r}")
        if draws == "device" and noise == "host":
            raise ValueError("DeviceDataLoader: draws='device' takes the gaussian noise from the device generator too; "
                             "it cannot be combined with noise='host'")
        self.bank, self.preprocessor, self.batch_size = bank, preprocessor, int(batch_size)
        self.audio_augmentor, self.spec_augmentor = audio_augmentor, spec_augmentor
        self.is_training, self.use_weighted_sampler = bool(is_training), bool(use_weighted_sampler)
        self.drop_last = self.is_training if drop_last is None else bool(drop_last)
        self.generator, self.noise, self.cache_features = generator, noise, bool(cache_features)
        self._augments = self.is_training and audio_augmentor is not None
        self._masks = self.is_training and spec_augmentor is not None
        if mixup is not None and not (float(mixup.alpha) > 0):
            raise ValueError(f"DeviceDataLoader: MixUp's alpha = {mixup.alpha} must be positive")
        self.mixup = mixup
        self._mixes = self.is_training and mixup is not None
        if self.cache_features and self._augments:
            raise ValueError("DeviceDataLoader: cache_features=True with a waveform augmentor on a training loader would "
                             "freeze the first epoch's augmentation; drop one of the two")
        self._n_masks = len(self._mask_slots()) if self._masks else 0
        if self._n_masks > _lib.MAX_MASKS:
            raise ValueError(f"DeviceDataLoader: at most {_lib.MAX_MASKS} masks per image")
        self._cache: Optional[torch.Tensor] = None
        self.draws = draws
        self.last_epoch_seed: Optional[int] = None

    def _mask_slots(self) -> List[int]:
        s = self.spec_augmentor
        return [0] * (s.n_freq_masks if s.freq_mask_param >= 1 else 0) + [1] * (s.n_time_masks if s.time_mask_param >= 1 else 0)

    def feature_shape(self) -> Tuple[int, int]:
        pre = self.preprocessor
        return pre.get_num_features(), pre._frames(pre.segment_samples)

    def __len__(self) -> int:
        n, b = len(self.bank), self.batch_size
        return n // b if self.drop_last else (n + b - 1) // b

    # ------------------------------------------------------------------ host side: indices and draws
    def epoch_indices(self) -> List[int]:
        """The clip indices of one epoch, drawn the way the reference's samplers draw them."""
        n = len(self.bank)
        if not self.is_training:
            return list(range(n))
        if self.use_weighted_sampler:
            return list(WeightedRandomSampler(self.bank.sample_weights, n, True, generator=self.generator))
        return list(RandomSampler(range(n), generator=self.generator))

    def draw_batch(self, indices: Sequence[int]) -> BatchPlan:
        """One batch's host draws, item by item in batch order (what ``CoughDataset.__getitem__`` draws per item)."""
        plan = self._draw_items(BatchPlan(), indices)
        if self._mixes:
            plan.perm = torch.randperm(len(indices))
            plan.lam = np.random.beta(self.mixup.alpha, self.mixup.alpha, size=len(indices))
        return plan

    def _draw_items(self, plan: BatchPlan, indices: Sequence[int]) -> BatchPlan:
        if not (self._augments or self._masks):
            return plan
        lengths = self.bank.lengths.numpy()[np.asarray(indices, dtype=np.int64)].tolist()    # one gather, not a tensor read per item
        f, t = self.feature_shape()
        draw = self.audio_augmentor.draw_item_channel if self._augments else None
        spec = self.spec_augmentor if self._masks else None
        items = []
        if spec is not None:
            plan.masks = []
        if self._augments and self.noise == "host":      # as wide as the speed step can make the longest row
            plan.gaussian = torch.zeros((len(indices), _chain.drawn_width(max(lengths), self.audio_augmentor)),
                                        dtype=torch.float32, pin_memory=self.bank.device.type == "cuda")
        for row, n in enumerate(lengths):
            if draw is not None:
                item = draw(n)
                items.append(item)
                if plan.gaussian is not None and item.record.gaussian:
                    plan.gaussian[row, :item.length] = torch.randn(item.length)      # n' samples; n without a speed step
            if spec is not None:
                fired = not (random.random() > spec.p)
                plan.masks.append(spec.draw_masks(f, t) if fired else [])
        if self._augments:                               # one column per step that is switched on, None for the others
            for name, column in _chain.columns(items, self.audio_augmentor).items():
                setattr(plan, name, column)
            if self.noise == "device":
                plan.seed = int(torch.randint(0, 2**62, (1,)).item())
        return plan

    # ------------------------------------------------------------------ device side: five launches
    def _mask_arrays(self, masks: List[list]) -> np.ndarray:
        """[3][B][n_masks] int32 (axis, start, end); an image whose coin did not fire keeps all of its masks empty."""
        arr = np.zeros((3, len(masks), self._n_masks), dtype=np.int32)
        for b, ms in enumerate(masks):
            for k, m in enumerate(ms):
                arr[:, b, k] = m
        return arr

    def _featurise(self, src: torch.Tensor, offsets: torch.Tensor, lens: torch.Tensor) -> torch.Tensor:
        """Unmasked features (B, F, T) of B rows of the flat buffer ``src``: ``cough_prepare_rows``, the featuriser."""
        return _featurise_rows(self.preprocessor, self.bank.device, src, offsets, lens)

    def _fill_cache(self) -> None:
        n, f_t = len(self.bank), self.feature_shape()
        self._cache = torch.empty((n,) + f_t, dtype=torch.float32, device=self.bank.device)
        for lo in range(0, n, self.batch_size):
            hi = min(lo + self.batch_size, n)
            self._cache[lo:hi] = self._featurise(self.bank.data, self.bank.offsets_dev[lo:hi], self.bank.lengths_dev[lo:hi])

    def _head(self, indices: Sequence[int]) -> Tuple[np.ndarray, np.ndarray, UploadWords]:
        """What both modes start with: the device check, the indices and the clips' lengths on the host, and the upload's
        int32 words with the lengths in front."""
        dev = self.bank.device
        if dev.type != "cuda":
            raise RuntimeError(f"DeviceDataLoader: the bank lives on {dev}; the loader's kernels need it on the GPU "
                               "(there is no CPU fallback)")
        idx = np.asarray(indices, dtype=np.int64)
        host_lens = self.bank.lengths.numpy()[idx]
        return idx, host_lens, UploadWords(host_lens)

    def _send(self, idx: np.ndarray, row_len: int, words: UploadWords) -> Tuple[torch.Tensor, torch.Tensor]:
        """The batch's one upload: int64 bank offsets, offsets of the rows of a (B, row_len) matrix, labels and indices;
        then the int32 words."""
        bank = self.bank
        return _upload(bank.device, np.concatenate([bank.offsets.numpy()[idx], np.arange(len(idx), dtype=np.int64) * row_len,
                                                    bank.labels.numpy()[idx], idx]), words.array())

    def _tail(self, i64: torch.Tensor, rows, masks, mix, targets: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """What both modes end with: the features of ``rows`` -- ``(src, offsets, lens)``, the batch's waveforms after the
        chain -- or, when ``rows`` is None, the cached ones; ``cough_mask_images`` with the device arrays ``masks`` (None:
        no masks); ``cough_mix_batch`` with ``mix``, the upload's ``(coefficients, permutation)`` (None: no MixUp).
        ``targets``: the rows' labels where they already are on the device (None: the uploaded ones)."""
        b = i64.numel() // 4
        if targets is None:
            targets = i64[2 * b:3 * b]
        elif not isinstance(targets, torch.Tensor) or targets.dtype != torch.int64 or tuple(targets.shape) != (b,) \
                or targets.device != i64.device or not targets.is_contiguous():
            raise ValueError(f"DeviceDataLoader: targets must be a contiguous int64 tensor of {b} labels on {i64.device}")
        if rows is None:
            if self._cache is None:
                self._fill_cache()
            feats = self._cache[i64[3 * b:4 * b]]
        else:
            feats = self._featurise(*rows)
        if masks is not None:
            mask_images(feats, feats, masks[0], masks[1], masks[2], self._n_masks)
        if mix is not None:
            mixed, soft = mix_batch_rows(feats.contiguous(), targets, mix[1], mix[0])
            return mixed.unsqueeze(1), soft
        return feats.unsqueeze(1), targets

    def launch_batch(self, indices: Sequence[int], plan: BatchPlan,
                     targets: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Everything of a batch that runs on the device, stream-ordered; nothing here waits for the device.
        ``targets``: a device int64 ``(B,)`` tensor of the rows' labels, used (for MixUp too) instead of the bank's
        uploaded labels -- for a bank whose labels were made on the device."""
        idx, host_lens, words = self._head(indices)
        b, bank, dev = len(idx), self.bank, self.bank.device
        row_len = int(host_lens.max())
        n_masks = self._n_masks if plan.masks is not None else 0
        if n_masks:
            words.add("masks", self._mask_arrays(plan.masks))
        if plan.perm is not None:
            words.add("coef", mix_coefficients(plan.lam), align8=True)
            words.add("perm", np.asarray(plan.perm).astype(np.int32))
        aug, plans = self.audio_augmentor, None
        if plan.clips is not None and (plan.warps() or plan.pitches() or plan.reverbs() or plan.mics()):
            plans = _chain.host_plans([c.shift for c in plan.clips], plan.pairs, plan.steps, host_lens, aug.sample_rate,
                                      row_len, aug.phase_lock, reverb=plan.rirs, channel=plan.channels,
                                      n_channels=len(aug.channel or ()))
            row_len = plans.width
            for name, array in plans.arrays.items():     # the plans ride behind the other words
                words.add(name, array, align8=name == "stretch")
        i64, i32 = self._send(idx, row_len, words)

        rows = None
        if not self.cache_features:
            src, offsets, lens, out_offsets = bank.data, i64[:b], words.view(i32, "lengths"), i64[b:2 * b]
            if plan.clips is not None:
                go = _chain.launches(plans, lambda name: words.view(i32, name), aug, keep=True)
                if not go.front:                 # no launch in front of the kernel: cough_augment_waveforms takes a matrix
                    src = torch.empty((b, row_len), dtype=torch.float32, device=dev)
                    _lib.check_data(_lib.load_data().cough_gather_rows(bank.data.data_ptr(), offsets.data_ptr(),
                                                                       lens.data_ptr(), b, src.data_ptr(), row_len, row_len,
                                                                       _stream(dev)), "cough_gather_rows")
                    clips, lens_now = plan.clips, host_lens
                else:                            # read in place from the bank; the first launch shifts the rows
                    src, _, lens = _chain.run(src, offsets, lens, go.speed, go.pitch, out_offsets, reverb=go.reverb)
                    clips, lens_now = _chain.unshifted(plan.clips), plans.new_lengths
                gaussian = plan.gaussian
                if gaussian is not None:
                    if gaussian.shape[1] != row_len:                 # drawn for the widest that the speed step can give
                        gaussian = gaussian[:, :row_len].contiguous()
                    gaussian = gaussian.to(dev, non_blocking=True)
                src, offsets = aug._run(src, clips, lens_now, gaussian, plan.seed), out_offsets
                if go.channel is not None:       # the microphone hears the room and the noise: in place on the kernel's matrix
                    _chain.finish(src, offsets, lens, go.channel, aug.channel, out=src)
            rows = (src, offsets, lens)
        return self._tail(i64, rows, words.view(i32, "masks") if n_masks else None,
                          (words.view(i32, "coef"), words.view(i32, "perm")) if plan.perm is not None else None, targets)

    def launch_batch_drawn(self, indices: Sequence[int], seed: int,
                           targets: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """``launch_batch`` with the batch's draws made on the device under ``seed`` (its records, its masks and its
        gaussian noise) by ``chain.run_drawn``, then ``cough_prepare_rows``, the featuriser, and ``cough_mask_images`` when
        there are masks.  The result equals ``launch_batch(indices, plan)`` for the ``BatchPlan`` that holds the same draws
        with ``seed`` as its noise seed.  The rows are sized for the slowest speed factor: no draw is read back.
        ``targets`` as in ``launch_batch``."""
        idx, host_lens, words = self._head(indices)
        b, aug = len(idx), self.audio_augmentor if self._augments else None
        if self._mixes:
            perm, lam = mix_draws(seed, b, self.mixup.alpha)
            words.add("coef", mix_coefficients(lam), align8=True)
            words.add("perm", perm)
        row_len = _chain.drawn_width(int(host_lens.max()), aug)
        i64, i32 = self._send(idx, row_len, words)
        rows, masks = _chain.run_drawn(seed, self.bank.data, i64[:b], words.view(i32, "lengths"), i64[b:2 * b], row_len, aug,
                                       self.spec_augmentor if self._n_masks else None, self.feature_shape())
        return self._tail(i64, None if self.cache_features else rows, masks,      # cached features: no augmentor ran
                          (words.view(i32, "coef"), words.view(i32, "perm")) if self._mixes else None, targets)

    def __iter__(self) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
        indices = self.epoch_indices()
        stop = len(self) * self.batch_size if self.drop_last else len(indices)
        drawn = self.draws == "device" and (self._augments or self._masks or self._mixes)
        if drawn:
            self.last_epoch_seed = int(torch.randint(0, 2**62, (1,), generator=self.generator).item())
        for k, lo in enumerate(range(0, stop, self.batch_size)):
            batch = indices[lo:min(lo + self.batch_size, stop)]
            if drawn:
                yield self.launch_batch_drawn(batch, (self.last_epoch_seed + k) & (2**64 - 1))
            else:
                yield self.launch_batch(batch, self.draw_batch(batch))


def create_data_loaders(train_bank: DeviceClipBank, val_bank: DeviceClipBank, preprocessor, batch_size: int = 32,
                        use_weighted_sampler: bool = True, audio_augmentor: Optional[AudioAugmentor] = None,
                        spec_augmentor: Optional[SpecAugment] = None, mixup: Optional[MixUp] = None,
                        **kw) -> Tuple[DeviceDataLoader, DeviceDataLoader]:
    """(train_loader, val_loader) as the reference's ``create_data_loaders`` (dataset.py:368-418): the training loader
    samples with ``WeightedRandomSampler`` (or shuffles), augments and drops the last ragged batch; the validation
    loader is sequential, unaugmented and keeps it.  ``mixup`` goes to the training loader only.  ``kw`` goes to the training loader (``generator``, ``noise``,
    ``cache_features``, ``draws``); ``cache_features`` also to the validation loader."""
    train = DeviceDataLoader(train_bank, preprocessor, batch_size=batch_size, audio_augmentor=audio_augmentor,
                             spec_augmentor=spec_augmentor, is_training=True, use_weighted_sampler=use_weighted_sampler,
                             mixup=mixup, **kw)
    val = DeviceDataLoader(val_bank, preprocessor, batch_size=batch_size, is_training=False,
                           cache_features=kw.get("cache_features", False))
    return train, val
