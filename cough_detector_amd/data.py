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

An ``AudioAugmentor(speed=True)`` adds the speed step to a training batch (``cough_detector_amd/warp.py``): one more
launch, ``cough_warp_rows``, reads the clips in place from the bank, shifts and resamples each by its own rate pair, and
the rest of the chain and ``cough_prepare_rows`` then work on the warped rows and their new lengths ``n'``.  With
``draws="host"`` the per-row plans and ``n'`` travel with the batch's pinned upload (a batch in which no speed coin
fired runs the launches it ran before); with ``draws="device"`` ``cough_draw_speed`` draws them first, the output is as
wide as the slowest factor can make the longest row, and nothing is read back.

An ``AudioAugmentor(pitch=True)`` adds the pitch step behind it (``cough_detector_amd/pitch.py``): two more launches,
``cough_stretch_rows`` and ``cough_warp_rows``, which keep every row's length.  Without a speed step the stretch reads
the clips in place from the bank and applies the time shift.  With ``draws="host"`` the two plans per row travel with
the pinned upload (a batch in which no pitch coin fired runs the launches it ran before); with ``draws="device"``
``cough_draw_pitch`` draws them, and the stretched rows are as wide as the largest number of semitones can make the
longest row.
"""
from __future__ import annotations

import random
import warnings
from pathlib import Path
from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch.utils.data import RandomSampler, WeightedRandomSampler

from . import _lib
from . import draws as _draws
from . import pitch as _pitch
from . import warp as _warp
from ._native import cuda_device
from .augmentation import AudioAugmentor, MixUp, SpecAugment, mask_images, mix_batch_rows, mix_coefficients

CLASSES = ["non_cough", "cough"]
_AUDIO_EXTENSIONS = {".wav", ".mp3", ".flac", ".ogg", ".webm"}      # dataset.py:86


def _stream(dev: torch.device) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


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


def mix_draws(seed: int, b: int, alpha: float) -> Tuple[np.ndarray, np.ndarray]:
    """``(perm int32 (b,), lam float64 (b,))`` of a ``draws="device"`` batch: a permutation, then ``Beta(alpha, alpha)``
    variates, from ``numpy.random.Generator(Philox(key=seed mod 2^64))`` on the host."""
    rng = np.random.Generator(np.random.Philox(key=int(seed) & (2**64 - 1)))
    perm = rng.permutation(b).astype(np.int32)
    return perm, rng.beta(alpha, alpha, size=b)


def _mix_words(n_before: int, perm: np.ndarray, lam: np.ndarray) -> Tuple[np.ndarray, int]:
    """The int32 words a mixed batch adds to its upload behind ``n_before`` words: padding to an 8-byte boundary, the
    (b, 2) float32 coefficients, the permutation.  Returns them and the coefficients' word offset."""
    pad = n_before & 1
    words = np.concatenate([np.zeros(pad, np.int32), mix_coefficients(lam).reshape(-1).view(np.int32),
                            np.asarray(perm, dtype=np.int32)])
    return words, n_before + pad


def _pitch_words(n_before: int, stretch: np.ndarray, back: np.ndarray) -> Tuple[np.ndarray, int]:
    """The int32 words a batch with a pitch step adds to its upload behind ``n_before`` words: padding to an 8-byte
    boundary, the (b, 16)-byte stretch plans, the (b, 3) int32 plans of the resampling that follows.  Returns them and
    the stretch plans' word offset."""
    pad = n_before & 1
    words = np.concatenate([np.zeros(pad, np.int32), np.ascontiguousarray(stretch).reshape(-1).view(np.int32),
                            np.asarray(back, dtype=np.int32).reshape(-1)])
    return words, n_before + pad


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
        self.device = torch.device(device) if device is not None else cuda_device()
        packed = torch.cat(clips) if clips else torch.zeros(0, dtype=torch.float32)
        self._set(packed.to(self.device), lengths, labels)

    def _set(self, data: torch.Tensor, lengths: List[int], labels: List[int]) -> None:
        self.data = data
        self.lengths = torch.tensor(lengths, dtype=torch.int32)
        self.offsets = torch.tensor(np.concatenate([[0], np.cumsum(lengths, dtype=np.int64)[:-1]]) if lengths else [],
                                    dtype=torch.int64)
        self.labels = torch.tensor(labels, dtype=torch.int64)
        self.offsets_dev = self.offsets.to(self.device)
        self.lengths_dev = self.lengths.to(self.device)
        self.labels_dev = self.labels.to(self.device)

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
        out = object.__new__(DeviceClipBank)
        out.device = self.device
        parts = [self.clip(i)[0] for i in idx]
        data = torch.cat(parts) if parts else torch.zeros(0, dtype=torch.float32, device=self.device)
        out._set(data, [int(self.lengths[i]) for i in idx], [int(self.labels[i]) for i in idx])
        return out

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


class BatchPlan:
    """The host draws of one batch: ``clips`` (a ``CoughAugClip`` per item, or None without waveform augmentation),
    ``gaussian`` (the ``torch.randn`` rows of ``noise="host"``, or None), ``seed`` (the device generator's) and ``masks``
    (per item the ``[(axis, start, end)]`` of SpecAugment, empty when its coin did not fire; None without it); with a
    ``MixUp``, ``perm`` (the batch's ``torch.randperm``) and ``lam`` (its float64 λ), else None.  With an augmentor that
    has ``speed=True``, ``pairs`` (per item the speed step's ``(orig, new)``, None when its coin did not fire) and
    ``new_lengths`` (per item ``n'``); else None.  ``gaussian`` rows then hold ``n'`` samples.  With an augmentor that
    has ``pitch=True``, ``steps`` (per item the pitch step's semitones, None when its coin did not fire); else None."""

    __slots__ = ("clips", "gaussian", "seed", "masks", "perm", "lam", "pairs", "new_lengths", "steps")

    def __init__(self, clips=None, gaussian=None, seed=0, masks=None, perm=None, lam=None, pairs=None, new_lengths=None,
                 steps=None):
        self.clips, self.gaussian, self.seed, self.masks = clips, gaussian, seed, masks
        self.perm, self.lam = perm, lam
        self.pairs, self.new_lengths = pairs, new_lengths
        self.steps = steps

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
        self._pitch_table: Optional[torch.Tensor] = None     # cough_draw_pitch's table, on the device

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
        lengths = [int(self.bank.lengths[i]) for i in indices]
        f, t = self.feature_shape()
        speed = self._augments and self.audio_augmentor.speed
        pitch = self._augments and self.audio_augmentor.pitch
        if self._augments:
            plan.clips = []
            if speed:
                plan.pairs, plan.new_lengths = [], []
            if pitch:
                plan.steps = []
            if self.noise == "host":
                aug = self.audio_augmentor
                wide = _warp.drawn_width(max(lengths), aug.speed_range, aug.sample_rate) if speed else max(lengths)
                plan.gaussian = torch.zeros((len(indices), wide), dtype=torch.float32, pin_memory=self._pinned())
        if self._masks:
            plan.masks = []
        for row, n in enumerate(lengths):
            if self._augments:
                c, pair, n, steps = self.audio_augmentor.draw_item_pitched(n)    # n' from here on; n without a speed step
                plan.clips.append(c)
                if pitch:
                    plan.steps.append(steps)
                if speed:
                    plan.pairs.append(pair)
                    plan.new_lengths.append(n)
                if c.gaussian and plan.gaussian is not None:
                    plan.gaussian[row, :n] = torch.randn(n)
            if self._masks:
                fired = not (random.random() > self.spec_augmentor.p)
                plan.masks.append(self.spec_augmentor.draw_masks(f, t) if fired else [])
        if self._augments and self.noise == "device":
            plan.seed = int(torch.randint(0, 2**62, (1,)).item())
        return plan

    def _pinned(self) -> bool:
        return self.bank.device.type == "cuda"

    # ------------------------------------------------------------------ device side: five launches
    def _mask_arrays(self, masks: List[list]) -> np.ndarray:
        """[3][B][n_masks] int32 (axis, start, end); an image whose coin did not fire keeps all of its masks empty."""
        arr = np.zeros((3, len(masks), self._n_masks), dtype=np.int32)
        for b, ms in enumerate(masks):
            for k, m in enumerate(ms):
                arr[:, b, k] = m
        return arr

    def _features(self, indices: Sequence[int], plan: BatchPlan, i64: torch.Tensor, lens: torch.Tensor,
                  warp: Optional[Tuple[torch.Tensor, torch.Tensor, int]] = None,
                  pitch: Optional[Tuple[torch.Tensor, torch.Tensor, int, int]] = None) -> torch.Tensor:
        """Unmasked features (B, F, T) of the clips ``indices``; ``i64`` holds their bank offsets, then B matrix-row
        offsets, on the device.  ``warp``: ``(plans, new lengths, width)`` of a batch in which a speed step fired, the
        first two on the device; the matrix rows are then ``width`` apart.  ``pitch``: ``(stretch plans, resampling
        plans, stretch width, width)`` of a batch in which a pitch step fired, the first two on the device."""
        bank, pre, dev = self.bank, self.preprocessor, self.bank.device
        lib, b = _lib.load_data(), len(indices)
        seg = torch.empty((b, pre.segment_samples), dtype=torch.float32, device=dev)
        src, offsets = bank.data, i64[:b]
        if plan.clips is not None and (warp is not None or pitch is not None):
            host_lens = [int(bank.lengths[i]) for i in indices]
            if warp is not None:                                     # shift and speed, read in place from the bank
                plans, lens_new, width = warp
                src = _warp.warp_rows(bank.data, offsets, lens, plans, width)
                offsets, lens, host_lens = i64[b:2 * b], lens_new, plan.new_lengths
            if pitch is not None:                                    # the shift rides in the stretch's read if not in the warp's
                stretch, back, stretch_width, width = pitch
                src = _pitch.pitch_shift_rows(src.reshape(-1), offsets, lens, stretch, back, width, stretch_width)
                offsets = i64[b:2 * b]
            unshifted = [_lib.CoughAugClip.from_buffer_copy(c) for c in plan.clips]
            for c in unshifted:
                c.shift = 0                                          # the first kernel's read has shifted the row
            gaussian = (plan.gaussian[:, :width].contiguous().to(dev, non_blocking=True) if plan.gaussian is not None
                        else None)
            src = self.audio_augmentor._run(src, unshifted, host_lens, gaussian, plan.seed)
        elif plan.clips is not None:
            host_lens = [int(bank.lengths[i]) for i in indices]
            row_len = max(host_lens)
            rows = torch.empty((b, row_len), dtype=torch.float32, device=dev)
            _lib.check_data(lib.cough_gather_rows(bank.data.data_ptr(), offsets.data_ptr(), lens.data_ptr(), b,
                                                  rows.data_ptr(), row_len, row_len, _stream(dev)), "cough_gather_rows")
            gaussian = plan.gaussian
            if gaussian is not None and gaussian.shape[1] != row_len:    # drawn for a speed step that did not fire
                gaussian = gaussian[:, :row_len].contiguous()
            gaussian = gaussian.to(dev, non_blocking=True) if gaussian is not None else None
            src = self.audio_augmentor._run(rows, plan.clips, host_lens, gaussian, plan.seed)
            offsets = i64[b:2 * b]
        _lib.check_data(lib.cough_prepare_rows(src.data_ptr(), offsets.data_ptr(), lens.data_ptr(), b, seg.data_ptr(),
                                               pre.segment_samples, _lib.PREP_NORMALIZE, _stream(dev)), "cough_prepare_rows")
        return pre.featurize_batch(seg, normalize=False)

    def _fill_cache(self) -> None:
        n, f_t = len(self.bank), self.feature_shape()
        self._cache = torch.empty((n,) + f_t, dtype=torch.float32, device=self.bank.device)
        for lo in range(0, n, self.batch_size):
            idx = list(range(lo, min(lo + self.batch_size, n)))
            self._cache[lo:lo + len(idx)] = self._features(idx, BatchPlan(), self.bank.offsets_dev[lo:lo + len(idx)],
                                                            self.bank.lengths_dev[lo:lo + len(idx)])

    def launch_batch(self, indices: Sequence[int], plan: BatchPlan) -> Tuple[torch.Tensor, torch.Tensor]:
        """Everything of a batch that runs on the device, stream-ordered; nothing here waits for the device."""
        bank, dev = self.bank, self.bank.device
        if dev.type != "cuda":
            raise RuntimeError(f"DeviceDataLoader: the bank lives on {dev}; the loader's kernels need it on the GPU "
                               "(there is no CPU fallback)")
        b = len(indices)
        idx = np.asarray(indices, dtype=np.int64)
        host_lens = bank.lengths.numpy()[idx]
        row_len = int(host_lens.max())
        masks = self._mask_arrays(plan.masks) if plan.masks is not None and self._n_masks else np.zeros(0, np.int32)
        words, mix_at = [host_lens, masks.reshape(-1)], 0
        if plan.perm is not None:
            mix, mix_at = _mix_words(b + masks.size, np.asarray(plan.perm), plan.lam)
            words.append(mix)
        warps, warp_at = plan.clips is not None and plan.warps(), 0
        if warps:                                # the speed step's plans and new lengths ride behind the other words
            row_len = max(plan.new_lengths)
            warp_at = sum(int(w.size) for w in words)
            words.append(_warp.plan_array([(c.shift,) + (p if p is not None else (1, 1))
                                           for c, p in zip(plan.clips, plan.pairs)]).reshape(-1))
            words.append(np.asarray(plan.new_lengths, dtype=np.int32))
        pitched, pitch_at, stretch_width = plan.clips is not None and plan.pitches() and not self.cache_features, 0, 0
        if pitched:                              # the pitch step's two plans per row ride behind those
            lens_now = plan.new_lengths if warps else host_lens.tolist()
            rates = [_pitch.pitch_rate(s) if s else 1.0 for s in plan.steps]
            sr = self.audio_augmentor.sample_rate
            stretch_width = max(_pitch.stretched_length(n, r) for n, r in zip(lens_now, rates))
            pitch_words, pitch_at = _pitch_words(
                sum(int(w.size) for w in words),
                _pitch.plan_array([(0 if warps else c.shift, r) for c, r in zip(plan.clips, rates)]),
                _warp.plan_array([(0,) + (_pitch.pitch_rate_pair(s, sr) if s else (1, 1)) for s in plan.steps]))
            words.append(pitch_words)
        i64, i32 = _upload(dev, np.concatenate([bank.offsets.numpy()[idx], np.arange(b, dtype=np.int64) * row_len,
                                                bank.labels.numpy()[idx], idx]), np.concatenate(words))
        targets = i64[2 * b:3 * b]
        if self.cache_features:
            if self._cache is None:
                self._fill_cache()
            feats = self._cache[i64[3 * b:4 * b]]
        else:
            warp = None
            if warps:
                n_plan = b * _warp.PLAN_WORDS
                warp = (i32[warp_at:warp_at + n_plan].view(b, _warp.PLAN_WORDS), i32[warp_at + n_plan:warp_at + n_plan + b],
                        row_len)
            pitch = None
            if pitched:
                n_plan = b * _pitch.PLAN_BYTES // 4
                pitch = (i32[pitch_at:pitch_at + n_plan].view(torch.uint8).view(b, _pitch.PLAN_BYTES),
                         i32[pitch_at + n_plan:pitch_at + n_plan + b * _warp.PLAN_WORDS].view(b, _warp.PLAN_WORDS),
                         stretch_width, row_len)
            feats = self._features(indices, plan, i64, i32[:b], warp, pitch)
        if masks.size:
            m = i32[b:b + masks.size].view(3, b, self._n_masks)
            mask_images(feats, feats, m[0], m[1], m[2], self._n_masks)
        if plan.perm is not None:
            return self._mix(feats, targets, i32, mix_at)
        return feats.unsqueeze(1), targets

    def _mix(self, feats: torch.Tensor, targets: torch.Tensor, i32: torch.Tensor, at: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """The batch mixed by ``cough_mix_batch``; its coefficients and permutation are the ``_mix_words`` at word ``at``
        of the batch's upload."""
        b = feats.shape[0]
        coef = i32[at:at + 2 * b].view(torch.float32).view(b, 2)
        mixed, soft = mix_batch_rows(feats.contiguous(), targets, i32[at + 2 * b:at + 3 * b], coef)
        return mixed.unsqueeze(1), soft

    def launch_batch_drawn(self, indices: Sequence[int], seed: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """``launch_batch`` with the batch's draws made on the device under ``seed`` (its records, its masks and its
        gaussian noise): draw, augment the rows in place in the bank, ``cough_prepare_rows``, the featuriser, and
        ``cough_mask_images`` when there are masks.  The result equals ``launch_batch(indices, plan)`` for the
        ``BatchPlan`` that holds the same records and masks with ``seed`` as its noise seed.  With an augmentor that has
        ``speed=True``, ``cough_draw_speed`` runs first and the records are drawn for the new lengths; ``cough_warp_rows``
        then shifts and resamples the rows from the bank, and the augmentation runs on its output with the shifts
        cleared.  With ``pitch=True``, ``cough_draw_pitch`` draws the two plans of the pitch step for the (new) lengths;
        ``cough_stretch_rows`` and ``cough_warp_rows`` run behind the speed step -- the time shift rides in the stretch's
        read when there is no speed step: its word is copied from the records into the stretch plans on the device."""
        bank, pre, dev = self.bank, self.preprocessor, self.bank.device
        if dev.type != "cuda":
            raise RuntimeError(f"DeviceDataLoader: the bank lives on {dev}; the loader's kernels need it on the GPU "
                               "(there is no CPU fallback)")
        b = len(indices)
        idx = np.asarray(indices, dtype=np.int64)
        host_lens = bank.lengths.numpy()[idx]
        row_len = int(host_lens.max())
        words, mix_at = [host_lens], 0
        if self._mixes:
            mix, mix_at = _mix_words(b, *mix_draws(seed, b, self.mixup.alpha))
            words.append(mix)
        aug = self.audio_augmentor if self._augments else None
        speed = aug is not None and aug.speed and not self.cache_features
        if speed:                                # wide enough for the slowest factor: the draws are never read back
            row_len = _warp.drawn_width(row_len, aug.speed_range, aug.sample_rate)
        i64, i32 = _upload(dev, np.concatenate([bank.offsets.numpy()[idx], np.arange(b, dtype=np.int64) * row_len,
                                                bank.labels.numpy()[idx], idx]), np.concatenate(words))
        lens = i32[:b]
        targets = i64[2 * b:3 * b]
        plans, lens_new = (_warp.draw_speed(seed, lens, aug.p_augment, aug.speed_range, aug.sample_rate) if speed
                           else (None, lens))
        pitch = aug is not None and aug.pitch and not self.cache_features
        if pitch:
            if self._pitch_table is None:
                self._pitch_table = torch.from_numpy(_pitch.step_table(aug.pitch_range, aug.sample_rate)).to(dev)
            stretch, back, _ = _pitch.draw_pitch(seed, lens_new, aug.p_augment, aug.pitch_range, aug.sample_rate,
                                                 self._pitch_table)
        clips, masks = _draws.draw_batch(seed, lens_new, aug, self.spec_augmentor if self._n_masks else None,
                                         self.feature_shape())
        if self.cache_features:
            if self._cache is None:
                self._fill_cache()
            feats = self._cache[i64[3 * b:4 * b]]
        else:
            src, offsets = bank.data, i64[:b]
            if speed or pitch:
                if speed:
                    src = _warp.warp_rows(bank.data, offsets, lens, plans, row_len)
                    offsets, lens = i64[b:2 * b], lens_new
                else:                            # the records' shift words into the stretch plans' (both lead their struct)
                    stretch.view(torch.int32).view(b, _pitch.PLAN_BYTES // 4)[:, 0] = \
                        clips.view(torch.int32).view(b, _draws.CLIP_BYTES // 4)[:, 0]
                _warp.clear_shifts(clips)
                if pitch:
                    src = _pitch.pitch_shift_rows(src.reshape(-1), offsets, lens, stretch, back, row_len,
                                                  _pitch.drawn_width(row_len, aug.pitch_range))
                    offsets = i64[b:2 * b]
                src = _draws.augment_rows_drawn(src, offsets, lens, row_len, clips, aug, seed)
            elif clips is not None:
                src = _draws.augment_rows_drawn(bank.data, offsets, lens, row_len, clips, self.audio_augmentor, seed)
                offsets = i64[b:2 * b]
            seg = torch.empty((b, pre.segment_samples), dtype=torch.float32, device=dev)
            _lib.check_data(_lib.load_data().cough_prepare_rows(src.data_ptr(), offsets.data_ptr(), lens.data_ptr(), b,
                                                                seg.data_ptr(), pre.segment_samples, _lib.PREP_NORMALIZE,
                                                                _stream(dev)), "cough_prepare_rows")
            feats = pre.featurize_batch(seg, normalize=False)
        if masks is not None:
            mask_images(feats, feats, masks[0], masks[1], masks[2], self._n_masks)
        if self._mixes:
            return self._mix(feats, targets, i32, mix_at)
        return feats.unsqueeze(1), targets

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
