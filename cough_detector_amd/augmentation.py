"""The reference's augmentation module (``/root/reference/src/augmentation.py``) on the MI355X, with its interface.

* ``AudioAugmentor`` (:19-268): the waveform chain ``time_shift -> speed_perturbation -> volume_perturbation ->
  add_gaussian_noise -> add_noise`` runs in ``cough_augment_waveforms`` (``csrc/augment.hip``).  Every coin and uniform is
  drawn on the host with Python ``random``, per clip, in the reference's order, so a seeded run draws what the reference
  draws.  ``augment`` and the single methods take one ``(1, N)`` clip and draw their gaussian noise with
  ``torch.randn_like`` on the CPU generator as the reference does; ``augment_batch`` runs a whole ``(B, N)`` batch
  (ragged lengths allowed) in one launch, with the noise drawn on the device (counter-based, seeded) or on the host.
* ``SpecAugment`` (:271-331): random draws on the host in the reference's order -- ``random.random()`` for the coin, then
  per mask two ``torch.rand(1)`` as torchaudio's ``mask_along_axis`` draws them -- so a seeded run masks the same rows /
  columns as the reference.  The masking itself is one pass of ``cough_mask_axes`` over the whole batch (all frequency and
  time masks at once) instead of one ``masked_fill`` pass per mask.  ``mask_batch`` draws a coin and masks per image, as
  a Dataset that calls SpecAugment per item does, and applies them in one pass of ``cough_mask_images``.
* ``MixUp`` (:334-369) and ``create_augmentation_pipeline`` (:372-398); the mixing runs in ``cough_mix_rows``.

``AudioAugmentor(speed=True)`` makes ``speed_perturbation`` real (the reference disabled it: torchaudio's resampler
needs a polyphase table of about 1 GB for a pair such as 15999 -> 16000).  ``cough_warp_rows``
(``cough_detector_amd/warp.py``) evaluates the filter per tap instead, with the time shift fused into its read, and the
rest of the chain then runs on the warped clip of ``n' = ceil(n * sample_rate / int(factor * sample_rate))`` samples.
The default ``speed=False`` draws nothing for it and changes no result.

``AudioAugmentor(pitch=True)`` makes ``pitch_shift`` real and puts it into the chain behind the speed step (the
reference calls sox for it and returns its input when sox is missing).  It is a float64 phase vocoder with a magnitude
floor, ``cough_stretch_rows``, followed by ``cough_warp_rows`` (``cough_detector_amd/pitch.py``): stretch by
``2 ** (-n_steps / 12)``, resample from ``int(sample_rate / rate)`` to ``sample_rate``, cut or pad back to the clip's
length.  The default ``pitch=False`` changes no result and moves no random stream.  ``phase_lock=True`` (with
``pitch=True``) stretches with identity phase locking, which keeps a steady tone's level where the plain vocoder returns
it at 0.6; it draws nothing, and the default ``phase_lock=False`` is the plain vocoder, bit for bit.

``AudioAugmentor(reverb=RirBank(...))`` adds a step the reference does not have: the clip convolved with a room impulse
response of the bank (``cough_reverb_rows``, ``cough_detector_amd/reverb.py``), behind the pitch step and before gain,
gaussian noise and the noise bank -- noise in a room is not convolved with the talker's response.  It keeps the clip's
length (the tail is dropped).  Its draws (coin, ``random.randrange(len(bank))``) sit behind the pitch step's and before
the gain's.  The default ``reverb=None`` draws nothing and changes no result, no random stream and no launch.

``AudioAugmentor(channel=ChannelBank(...))`` adds the last link: the device that records.  The matrix the augmentation
kernel wrote goes through a microphone response of the bank and a hard clip relative to the clip's own peak
(``cough_channel_rows``, ``cough_detector_amd/channel.py``) -- behind the noise, because a microphone hears the room and
the noise.  Its draws come last in an item's sequence, behind the noise bank's: coin, ``random.randrange(len(bank))``,
then ``random.random() < p_clip`` gives ``random.uniform(*clip_range)``.  It keeps the clip's length.  The default
``channel=None`` draws nothing and changes no result, no random stream and no launch; a batch in which no channel coin
fired runs the launches it ran before.

Differences a caller can observe: results come back where the input lives, as float32.  With ``pitch=False``
``pitch_shift`` draws its coin and semitones as the reference does and returns its input unchanged -- the reference's
own result when sox is absent (its ``except`` branch) -- and ``augment`` never calls it.  The noise bank decodes WAVE files only (``load_wave``); other files
are skipped like the reference's undecodable ones.
"""
from __future__ import annotations

import ctypes as C
import math
import random
from pathlib import Path
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, _tables
from . import chain as _chain
from . import pitch as _pitch
from . import channel as _channel
from . import reverb as _reverb
from . import warp as _warp
from ._native import cuda_device
from .preprocessing import load_wave


def mask_images(src: torch.Tensor, out: torch.Tensor, axis: torch.Tensor, start: torch.Tensor, end: torch.Tensor,
                n_masks: int) -> None:
    """One ``cough_mask_images`` launch over the (..., F, T) float32 GPU tensor ``src`` into ``out`` (which may be
    ``src``): image b gets masks ``[b][0 .. n_masks)`` of the device int32 arrays ``axis`` / ``start`` / ``end``."""
    dev = src.device
    if not (src.is_contiguous() and out.is_contiguous() and src.dtype == out.dtype == torch.float32 and out.shape == src.shape
            and out.device == dev and dev.type == "cuda" and src.dim() >= 2):
        raise ValueError("mask_images: src and out must be contiguous float32 (..., F, T) tensors of one shape on the GPU")
    h, w = src.shape[-2], src.shape[-1]
    n_img = src.numel() // (h * w) if h * w else 0
    arrays = [a if n_masks else None for a in (axis, start, end)]
    for a in arrays:
        if a is not None and not (a.device == dev and a.dtype == torch.int32 and a.is_contiguous()
                                  and a.numel() == n_img * n_masks):
            raise ValueError(f"mask_images: the mask arrays must be contiguous int32 [{n_img}][{n_masks}] on {dev}")
    if n_img == 0:
        return
    ptr = lambda a: None if a is None else a.data_ptr()      # noqa: E731
    _lib.check_data(_lib.load_data().cough_mask_images(src.data_ptr(), out.data_ptr(), n_img, h, w, n_masks, ptr(arrays[0]),
                                                       ptr(arrays[1]), ptr(arrays[2]),
                                                       torch.cuda.current_stream(dev).cuda_stream), "cough_mask_images")


class SpecAugment:
    def __init__(self, freq_mask_param: int = 10, time_mask_param: int = 20, n_freq_masks: int = 2,
                 n_time_masks: int = 2, p: float = 0.5):
        self.freq_mask_param, self.time_mask_param = freq_mask_param, time_mask_param
        self.n_freq_masks, self.n_time_masks = n_freq_masks, n_time_masks
        self.p = p
        if n_freq_masks + n_time_masks > 16:
            raise ValueError("SpecAugment: at most 16 masks per call on the MI355X path")

    @staticmethod
    def _draw(mask_param: int, size: int) -> Tuple[int, int]:
        # torchaudio.functional.mask_along_axis (iid_masks=False, p=1.0)
        value = torch.rand(1) * mask_param
        min_value = torch.rand(1) * (size - value)
        return int(min_value.long()), int(min_value.long() + value.long())

    def draw_masks(self, n_freq: int, n_time: int) -> List[Tuple[int, int, int]]:
        """[(axis, start, end)] in the reference's draw order: frequency masks, then time masks."""
        masks = []
        if self.freq_mask_param >= 1:
            masks += [(0,) + self._draw(self.freq_mask_param, n_freq) for _ in range(self.n_freq_masks)]
        if self.time_mask_param >= 1:
            masks += [(1,) + self._draw(self.time_mask_param, n_time) for _ in range(self.n_time_masks)]
        return masks

    def __call__(self, spectrogram: torch.Tensor) -> torch.Tensor:
        """(C, F, T) or (B, C, F, T) -> same shape, a new tensor when the augmentation fires (as ``masked_fill``)."""
        if random.random() > self.p:
            return spectrogram
        if spectrogram.dim() not in (3, 4):
            raise ValueError(f"SpecAugment: expected (C, F, T) or (B, C, F, T), got {tuple(spectrogram.shape)}")
        masks = self.draw_masks(spectrogram.shape[-2], spectrogram.shape[-1])
        if not masks:
            return spectrogram
        dev = cuda_device()
        src = spectrogram.to(device=dev, dtype=torch.float32).contiguous()
        out = torch.empty_like(src)
        n = len(masks)
        arr = lambda k: (C.c_int * n)(*[m[k] for m in masks])
        n_img = src.numel() // (src.shape[-2] * src.shape[-1])
        if src.numel():
            _lib.check(_lib.load().cough_mask_axes(src.data_ptr(), out.data_ptr(), n_img, src.shape[-2], src.shape[-1], n,
                                                   arr(0), arr(1), arr(2), torch.cuda.current_stream(dev).cuda_stream),
                       "cough_mask_axes")
        return out.to(spectrogram.device) if spectrogram.device.type == "cpu" else out

    def mask_batch(self, features: torch.Tensor) -> torch.Tensor:
        """(B, C, F, T) or (B, F, T) -> a new tensor of that shape where the input lives: item b gets a coin and masks of
        its own, drawn item by item in batch order (``random.random()``, then ``draw_masks`` when it fired -- what a
        Dataset that calls ``self(item)`` per item draws); the channels of an item share its masks.  One pass of
        ``cough_mask_images`` over the batch."""
        if features.dim() not in (3, 4):
            raise ValueError(f"SpecAugment.mask_batch: expected (B, C, F, T) or (B, F, T), got {tuple(features.shape)}")
        b, f, t = features.shape[0], features.shape[-2], features.shape[-1]
        per_item = [self.draw_masks(f, t) if not (random.random() > self.p) else [] for _ in range(b)]
        n = max((len(m) for m in per_item), default=0)
        channels = features.shape[1] if features.dim() == 4 else 1
        arr = np.zeros((3, b, channels, n), dtype=np.int32)
        for i, masks in enumerate(per_item):
            for k, m in enumerate(masks):
                arr[:, i, :, k] = np.asarray(m, dtype=np.int32)[:, None]
        dev = cuda_device()
        src = features.detach().to(device=dev, dtype=torch.float32).contiguous()
        out = torch.empty_like(src)
        d = torch.from_numpy(arr).to(dev)
        mask_images(src, out, d[0].reshape(-1), d[1].reshape(-1), d[2].reshape(-1), n)
        return out.to(features.device)


# ---------------------------------------------------------------------------------------------- waveform augmentation
_SHIFT_LIMIT, _GAIN_RANGE, _GAUSS_SNR, _BANK_SNR = 0.2, (0.7, 1.3), (10, 30), (5, 20)


def _repeated_length(entry_len: int, target_len: int) -> int:
    """Length of a noise entry after the reference's ``repeat`` (augmentation.py:143-147)."""
    return entry_len * (target_len // entry_len + 1) if entry_len < target_len else entry_len


class AudioAugmentor:
    def __init__(self, sample_rate: int = 16000, noise_dir: Optional[str] = None, p_augment: float = 0.5,
                 speed: bool = False, speed_range: Tuple[float, float] = (0.9, 1.1), pitch: bool = False,
                 pitch_range: Tuple[int, int] = (-2, 2), phase_lock: bool = False, reverb=None, channel=None,
                 p_clip: float = 0.3, clip_range: Tuple[float, float] = (0.25, 1.0)):
        self.sample_rate = sample_rate
        if channel is not None and not isinstance(channel, _channel.ChannelBank):
            raise TypeError(f"AudioAugmentor: channel must be a ChannelBank or None, got {type(channel).__name__}")
        self.channel = channel                           # the channel step's bank of microphone responses; None: no step
        self.p_clip, self.clip_range = _channel.check_clip(p_clip, clip_range, "AudioAugmentor")
        if reverb is not None and not isinstance(reverb, _reverb.RirBank):
            raise TypeError(f"AudioAugmentor: reverb must be a RirBank or None, got {type(reverb).__name__}")
        self.reverb = reverb                             # the reverb step's bank of room impulse responses; None: no step
        self.p_augment = p_augment
        self.speed = bool(speed)
        self.speed_range = (float(speed_range[0]), float(speed_range[1]))
        if self.speed:
            _warp.check_speed_range(self.speed_range, sample_rate, "AudioAugmentor")
        self.pitch = bool(pitch)
        self.pitch_range = (pitch_range[0], pitch_range[1])
        if self.pitch:
            self.pitch_range = _pitch.check_pitch_range(self.pitch_range, "AudioAugmentor")
            if not 2 <= int(sample_rate) <= _lib.WARP_MAX_RATE // 2:         # int(sample_rate / rate) stays a rate the resampler takes
                raise ValueError(f"AudioAugmentor: pitch=True needs a sample_rate in 2..2^19, got {sample_rate}")
        self.phase_lock = bool(phase_lock)               # the pitch step's stretch mode; draws nothing
        if self.phase_lock and not self.pitch:
            raise ValueError("AudioAugmentor: phase_lock=True is a mode of the pitch step and needs pitch=True")
        self.noise_samples: List[torch.Tensor] = []      # (1, L) float32 on the host, as the reference keeps them
        self._bank_host = torch.zeros(0, dtype=torch.float32)
        self._bank_offsets: List[int] = []
        self._bank_lengths: List[int] = []
        self._bank_dev = None
        self._bank_tables = None                         # (device, int64 offsets, int32 lengths) on the device
        self._pitch_table: Optional[torch.Tensor] = None     # cough_draw_pitch's table, on the device
        if noise_dir and Path(noise_dir).exists():
            self._load_noise_samples(noise_dir)

    # ------------------------------------------------------------------ noise bank
    def _resample(self, waveform: torch.Tensor, orig_sr: int) -> torch.Tensor:
        """T.Resample(orig_sr, sample_rate) of a (C, N) host tensor on the GPU (``cough_resample``); back on the host."""
        dev = cuda_device()
        kern, width, orig, new = _tables.sinc_resample_kernel(orig_sr, self.sample_rate)
        x = waveform.to(device=dev, dtype=torch.float32).contiguous()
        rows, n = x.shape
        out_len = int(math.ceil(new * n / orig))
        out = torch.empty((rows, out_len), dtype=torch.float32, device=dev)
        kern = kern.to(dev)
        if rows and out_len:
            _lib.check(_lib.load().cough_resample(x.data_ptr(), n, rows, n, kern.data_ptr(), orig, new, width, out.data_ptr(),
                                                  out_len, out_len, torch.cuda.current_stream(dev).cuda_stream), "cough_resample")
        return out.cpu()

    def _load_noise_samples(self, noise_dir: str, max_samples: int = 100):
        """Load background noise samples from directory (reference :57-75): the first ``max_samples`` of the ``.wav``,
        ``.mp3``, ``.flac``, ``.ogg`` files in that order, each resampled to ``sample_rate`` and averaged to mono.  Files
        that do not decode (or hold no samples) are skipped.  The bank is then packed into one buffer, on the device."""
        noise_path = Path(noise_dir)
        noise_files = []
        for ext in ['.wav', '.mp3', '.flac', '.ogg']:
            noise_files.extend(noise_path.glob(f'*{ext}'))
        for f in noise_files[:max_samples]:
            try:
                waveform, sr = load_wave(str(f))
            except ValueError:
                continue
            if waveform.shape[1] == 0:
                continue
            if sr != self.sample_rate:
                waveform = self._resample(waveform, sr)
            if waveform.shape[0] > 1:
                waveform = waveform.mean(dim=0, keepdim=True)
            self.noise_samples.append(waveform)
        self._pack_bank()

    def _pack_bank(self) -> None:
        lengths = [int(w.shape[1]) for w in self.noise_samples]
        self._bank_lengths = lengths
        self._bank_offsets = [sum(lengths[:k]) for k in range(len(lengths))]
        self._bank_host = (torch.cat([w.reshape(-1).float() for w in self.noise_samples]) if lengths
                           else torch.zeros(0, dtype=torch.float32))
        self._bank_dev = None
        self._bank_tables = None
        if lengths and torch.cuda.is_available():
            self._bank_dev = self._bank_host.to(cuda_device())

    def _bank_device(self, dev: torch.device) -> torch.Tensor:
        if self._bank_dev is None or self._bank_dev.device != dev:
            self._bank_dev = self._bank_host.to(dev)
        return self._bank_dev

    def _bank_tables_device(self, dev: torch.device) -> Tuple[torch.Tensor, torch.Tensor]:
        """The bank's offsets (int64) and lengths (int32) as device tensors, uploaded once per packing of the bank."""
        if self._bank_tables is None or self._bank_tables[0] != dev:
            self._bank_tables = (dev, torch.tensor(self._bank_offsets, dtype=torch.int64).to(dev),
                                 torch.tensor(self._bank_lengths, dtype=torch.int32).to(dev))
        return self._bank_tables[1], self._bank_tables[2]

    # ------------------------------------------------------------------ host draws (the reference's order)
    def _coin(self) -> bool:
        return not (random.random() > self.p_augment)

    def _draw_shift(self, n: int, shift_limit: float = _SHIFT_LIMIT) -> int:
        return int(n * random.uniform(-shift_limit, shift_limit)) if self._coin() else 0

    def _draw_speed(self, speed_range=None) -> Optional[Tuple[int, int]]:
        """speed_perturbation's draws: coin, factor; the rate pair of torchaudio's ``speed``."""
        if not self._coin():
            return None
        return _warp.speed_rate_pair(random.uniform(*(speed_range or self.speed_range)), self.sample_rate)

    def _draw_pitch(self, shift_range=None) -> Optional[int]:
        """pitch_shift's draws: coin, ``random.randint`` over the semitone range (the reference's :215-247)."""
        if not self._coin():
            return None
        return random.randint(*(shift_range or self.pitch_range))

    def _draw_reverb(self) -> Optional[int]:
        """The reverb step's draws: coin, ``random.randrange`` over the bank."""
        if not self._coin():
            return None
        return random.randrange(len(self.reverb))

    def _draw_channel(self) -> Optional[Tuple[int, float]]:
        """The channel step's draws: coin, ``random.randrange`` over the bank, the clip coin (``random.random() <
        p_clip``) and, when that fires, ``random.uniform(*clip_range)``: ``(filter, ratio)``, the ratio 1.0 without a clip."""
        if not self._coin():
            return None
        which = random.randrange(len(self.channel))
        return which, (random.uniform(*self.clip_range) if random.random() < self.p_clip else 1.0)

    def _draw_gain(self, gain_range=_GAIN_RANGE) -> Optional[float]:
        return random.uniform(*gain_range) if self._coin() else None

    def _draw_gauss(self, snr_range=_GAUSS_SNR) -> Optional[float]:
        return random.uniform(*snr_range) if self._coin() else None

    def _draw_bank(self, n: int, snr_range=_BANK_SNR) -> Optional[Tuple[int, int, float]]:
        """add_noise's draws: coin, ``random.choice``, ``random.randint`` over the repeated entry, SNR."""
        if random.random() > self.p_augment or len(self.noise_samples) == 0:
            return None
        k = random.choice(range(len(self.noise_samples)))      # the same draw as random.choice(self.noise_samples)
        start = random.randint(0, _repeated_length(self._bank_lengths[k], n) - n)
        return k, start, random.uniform(*snr_range)

    def draw_clip(self, n: int) -> _lib.CoughAugClip:
        """One ``augment`` call's draws for a clip of ``n`` samples (reference :249-268): the item's record."""
        return self.draw_item_channel(n).record

    def draw_item(self, n: int) -> Tuple[_lib.CoughAugClip, Optional[Tuple[int, int]], int]:
        """``(record, rate pair, n')``: the first three fields of ``draw_item_channel``, as a plain tuple."""
        return self.draw_item_channel(n)[:3]

    def draw_item_pitched(self, n: int) -> Tuple[_lib.CoughAugClip, Optional[Tuple[int, int]], int, Optional[int]]:
        """``(record, rate pair, n', n_steps)``: the first four fields of ``draw_item_channel``, as a plain tuple."""
        return self.draw_item_channel(n)[:4]

    def draw_item_reverb(self, n: int) -> Tuple[_lib.CoughAugClip, Optional[Tuple[int, int]], int, Optional[int], Optional[int]]:
        """``(record, rate pair, n', n_steps, rir)``: the first five fields of ``draw_item_channel``, as a plain tuple."""
        return self.draw_item_channel(n)[:5]

    def draw_item_channel(self, n: int) -> _chain.ItemDraw:
        """All draws of one ``augment`` call on a clip of ``n`` samples, in the chain's order -- shift, speed, pitch,
        reverb, gain, gaussian, noise bank, channel -- as ``chain.ItemDraw``: ``(record, pair, length, steps, rir,
        channel)``.  A step that is switched off draws nothing and leaves None; so does, behind its coin, a step whose
        coin did not fire.  ``speed=True``: the noise-bank step, which crops ``n'`` samples, is drawn for the warped
        length ``n'`` (``length``; ``n`` without a pair); the record's shift is the one drawn for ``n``.  ``pitch=True``:
        coin and semitones (0 is a drawn value that shifts nothing).  A ``reverb`` bank: coin and
        ``random.randrange(len(bank))``.  Neither changes ``n'``.  A ``channel`` bank: ``(filter, clip_ratio)``.  Every
        other draw method (``draw_clip``, ``draw_batch``, ``draw_item*``) calls this one and so consumes the channel's draws too."""
        c = self._blank()
        c.shift = self._draw_shift(n)
        pair = self._draw_speed() if self.speed else None         # speed=False: speed_perturbation draws nothing
        n = n if pair is None else _warp.warped_length(n, *pair)
        steps = self._draw_pitch() if self.pitch else None       # pitch=False: pitch_shift is not part of the chain
        rir = self._draw_reverb() if self.reverb is not None else None      # no bank: the step draws nothing
        gain = self._draw_gain()
        if gain is not None:
            c.gain = gain
        snr = self._draw_gauss()
        if snr is not None:
            c.gaussian, c.gaussian_snr_db = 1, snr
        if len(self.noise_samples) > 0:
            d = self._draw_bank(n)
            if d is not None:
                c.bank_index, c.bank_start, c.bank_snr_db = d
        mic = self._draw_channel() if self.channel is not None else None     # no bank: the step draws nothing
        return tuple.__new__(_chain.ItemDraw, (c, pair, n, steps, rir, mic))  # per item: skips the Python-level __new__

    def _run_channel(self, x: torch.Tensor, lengths: Sequence[int], plans: Sequence[Optional[Tuple[int, float]]]) -> torch.Tensor:
        """The channel step on the (B, N) matrix the kernel wrote (``chain.finish`` into a new matrix: ``src`` is ``x`` itself
        when ``x`` is float32 on the device), row b its first ``lengths[b]`` samples with ``plans[b]`` (None: a copy)."""
        dev = cuda_device()
        src = x.detach().to(device=dev, dtype=torch.float32).contiguous()
        b, n = src.shape
        mics = torch.from_numpy(_chain.channel_plans(plans, len(self.channel))).to(dev)
        out = _chain.finish(src, _chain.dense_offsets(b, n, dev), torch.tensor([int(v) for v in lengths], dtype=torch.int32).to(dev),
                            mics, self.channel)
        return out.to(device=x.device, dtype=x.dtype)

    def pitch_table(self, dev: torch.device) -> torch.Tensor:
        """``cough_draw_pitch``'s table on the device, uploaded once; the stretch mode rides in its entries."""
        if self._pitch_table is None or self._pitch_table.device != dev:
            self._pitch_table = torch.from_numpy(_pitch.step_table(self.pitch_range, self.sample_rate, self.phase_lock)).to(dev)
        return self._pitch_table

    def draw_batch(self, lengths: Sequence[int]) -> List[_lib.CoughAugClip]:
        """The draws of ``augment_batch``: ``draw_clip`` for each clip in order, as a Dataset calls ``augment`` per item."""
        return [self.draw_clip(int(n)) for n in lengths]

    # ------------------------------------------------------------------ the kernel
    def _run(self, x: torch.Tensor, clips: List[_lib.CoughAugClip], lengths: Optional[Sequence[int]],
             gaussian: Optional[torch.Tensor], seed: int) -> torch.Tensor:
        """One cough_augment_waveforms launch over the rows of the 2-D ``x``; the result where ``x`` lives."""
        dev = cuda_device()
        src = x.detach().to(device=dev, dtype=torch.float32)
        if src.stride(-1) != 1 or src.stride(0) < src.shape[1]:
            src = src.contiguous()
        b, n = src.shape
        out = torch.empty((b, n), dtype=torch.float32, device=dev)
        if b == 0:
            return out.to(x.device)
        lib = _lib.load()
        arr = (_lib.CoughAugClip * b)(*clips)
        lens = (C.c_int * b)(*[int(v) for v in lengths]) if lengths is not None else None
        nb = len(self._bank_lengths)
        bank = self._bank_device(dev) if nb else None
        offs = (C.c_longlong * nb)(*self._bank_offsets) if nb else None
        blen = (C.c_int * nb)(*self._bank_lengths) if nb else None
        z = gaussian.to(device=dev, dtype=torch.float32).contiguous() if gaussian is not None else None
        ws = torch.empty(max(int(lib.cough_augment_workspace_bytes(b)), 1), dtype=torch.uint8, device=dev)
        stride = src.stride(0) if b > 1 else n
        _lib.check(lib.cough_augment_waveforms(src.data_ptr(), stride, out.data_ptr(), b, n, lens, arr,
                                               bank.data_ptr() if bank is not None else None,
                                               bank.numel() if bank is not None else 0, offs, blen, nb,
                                               z.data_ptr() if z is not None else None, seed & (2**64 - 1),
                                               ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream),
                   "cough_augment_waveforms")
        return out.to(x.device)

    def _run_chain(self, x: torch.Tensor, clips: List[_lib.CoughAugClip], lengths: Optional[Sequence[int]],
                   pairs: Optional[Sequence[Optional[Tuple[int, int]]]], steps: Optional[Sequence[Optional[int]]],
                   gaussian: Optional[torch.Tensor], seed: int, rirs: Optional[Sequence[Optional[int]]] = None) -> torch.Tensor:
        """``_run`` behind the speed, pitch and reverb steps (``chain.host_plans`` has the rules, ``chain.run`` the
        launches): ``cough_warp_rows`` when a speed coin fired, ``cough_stretch_rows`` and ``cough_warp_rows`` when a row
        has semitones, ``cough_reverb_rows`` when a row of ``rirs`` has a response, then ``cough_augment_waveforms`` on
        the result with the records' shifts zeroed and the lengths ``n'``.  ``pairs`` / ``steps`` / ``rirs`` are None
        when the step is switched off.  Returns (B, max n') with a speed step and (B, N) without.  ``gaussian`` is cut to
        the width of the rows that ``_run`` gets.  When nothing fired the launches are skipped and the path is ``_run``'s."""
        b, n = x.shape
        lens = [int(v) for v in lengths] if lengths is not None else [n] * b
        plans = _chain.host_plans([c.shift for c in clips], pairs, steps, lens, self.sample_rate, n, self.phase_lock,
                                  reverb=rirs)
        width = plans.width if plans.arrays else n
        if gaussian is not None and gaussian.shape[1] != width:
            gaussian = gaussian[:, :width].contiguous()
        if not plans.arrays:                             # nothing fired: the records keep their shifts
            out = self._run(x, clips, lengths, gaussian, seed)
            return out[:, :plans.width].contiguous() if pairs is not None else out
        dev = cuda_device()
        src = x.detach().to(device=dev, dtype=torch.float32).contiguous()
        go = _chain.launches(plans, lambda name: torch.from_numpy(plans.arrays[name]).to(dev), self)
        rows, _, _ = _chain.run(src.reshape(-1), _chain.dense_offsets(b, n, dev), torch.tensor(lens, dtype=torch.int32).to(dev),
                                go.speed, go.pitch, _chain.dense_offsets(b, plans.width, dev) if go.chained else None, reverb=go.reverb)
        return self._run(rows, _chain.unshifted(clips), plans.new_lengths, gaussian, seed).to(x.device)

    @staticmethod
    def _one_clip(waveform: torch.Tensor, who: str) -> None:
        if not isinstance(waveform, torch.Tensor) or not waveform.dtype.is_floating_point:
            raise TypeError(f"{who}: expected a floating-point torch.Tensor")
        if waveform.dim() != 2 or waveform.shape[0] != 1 or waveform.shape[1] < 1:
            raise ValueError(f"{who}: expected one (1, N) clip, got {tuple(waveform.shape)}")

    def _single(self, waveform: torch.Tensor, c: _lib.CoughAugClip) -> torch.Tensor:
        gaussian = torch.randn_like(waveform, dtype=torch.float32, device="cpu") if c.gaussian else None
        return self._run(waveform, [c], None, gaussian, 0).to(waveform.dtype)

    @staticmethod
    def _blank() -> _lib.CoughAugClip:
        return _lib.CoughAugClip(shift=0, gain=1.0, gaussian=0, bank_index=-1, gaussian_snr_db=0.0, bank_snr_db=0.0,
                                 bank_start=0)

    # ------------------------------------------------------------------ the reference's methods (one (1, N) clip)
    def time_shift(self, waveform: torch.Tensor, shift_limit: float = _SHIFT_LIMIT) -> torch.Tensor:
        if random.random() > self.p_augment:
            return waveform
        self._one_clip(waveform, "time_shift")
        c = self._blank()
        c.shift = int(waveform.shape[1] * random.uniform(-shift_limit, shift_limit))
        return waveform if c.shift == 0 else self._single(waveform, c)

    def speed_perturbation(self, waveform: torch.Tensor, speed_range: Optional[Tuple[float, float]] = None) -> torch.Tensor:
        """With ``speed=False`` the identity, as in the reference (:107-117), and no draw.  With ``speed=True`` what the
        reference meant to run: coin, ``factor = random.uniform(*speed_range)`` (the augmentor's range by default), then
        ``torchaudio.functional.speed``'s resampling by ``(int(factor * sample_rate), sample_rate)``: (1, n')."""
        if not self.speed:
            return waveform
        if speed_range is not None:
            _warp.check_speed_range(speed_range, self.sample_rate, "speed_perturbation")
        pair = self._draw_speed(speed_range)
        if pair is None:
            return waveform
        self._one_clip(waveform, "speed_perturbation")
        return self._run_chain(waveform, [self._blank()], None, [pair], None, None, 0).to(waveform.dtype)

    def add_noise(self, waveform: torch.Tensor, snr_range: Tuple[float, float] = _BANK_SNR) -> torch.Tensor:
        self._one_clip(waveform, "add_noise")
        d = self._draw_bank(waveform.shape[1], snr_range)
        if d is None:
            return waveform
        c = self._blank()
        c.bank_index, c.bank_start, c.bank_snr_db = d
        return self._single(waveform, c)

    def add_gaussian_noise(self, waveform: torch.Tensor, snr_range: Tuple[float, float] = _GAUSS_SNR) -> torch.Tensor:
        self._one_clip(waveform, "add_gaussian_noise")
        snr = self._draw_gauss(snr_range)
        if snr is None:
            return waveform
        c = self._blank()
        c.gaussian, c.gaussian_snr_db = 1, snr
        return self._single(waveform, c)

    def volume_perturbation(self, waveform: torch.Tensor, gain_range: Tuple[float, float] = _GAIN_RANGE) -> torch.Tensor:
        self._one_clip(waveform, "volume_perturbation")
        gain = self._draw_gain(gain_range)
        if gain is None:
            return waveform
        c = self._blank()
        c.gain = gain
        return self._single(waveform, c)

    def pitch_shift(self, waveform: torch.Tensor, shift_range: Optional[Tuple[int, int]] = None) -> torch.Tensor:
        """With ``pitch=False``: draws the reference's coin and semitones (:215-247; (-2, 2) by default), then returns
        the input unchanged -- what the reference returns when sox is not available; ``augment`` does not call it.
        With ``pitch=True``: the same draws (the augmentor's range by default), the input itself for 0 semitones, and
        otherwise the clip shifted by that many semitones, (1, n): ``pitch_shift_rows``, in the augmentor's stretch mode
        (``phase_lock``)."""
        if not self.pitch:
            if random.random() > self.p_augment:
                return waveform
            random.randint(*(shift_range or (-2, 2)))
            return waveform
        if shift_range is not None:
            _pitch.check_pitch_range(shift_range, "pitch_shift")
        steps = self._draw_pitch(shift_range)
        if not steps:
            return waveform
        self._one_clip(waveform, "pitch_shift")
        return self._run_chain(waveform, [self._blank()], None, None, [steps], None, 0).to(waveform.dtype)

    def augment(self, waveform: torch.Tensor) -> torch.Tensor:
        """The reference's chain on one (1, N) clip (:249-268) in one launch; the input itself when no step fired."""
        self._one_clip(waveform, "augment")
        item = self.draw_item_channel(waveform.shape[1])
        c = item.record
        if item.steps or item.pair is not None or item.rir is not None:     # the pitch, the speed or the reverb step fired: (1, n')
            gaussian = torch.randn((1, item.length), dtype=torch.float32) if c.gaussian else None
            out = self._run_chain(waveform, [c], None, [item.pair] if self.speed else None, [item.steps], gaussian,
                                  0, rirs=[item.rir] if self.reverb is not None else None).to(waveform.dtype)
        elif c.shift == 0 and c.gain == 1.0 and not c.gaussian and c.bank_index < 0:
            out = waveform
        else:
            out = self._single(waveform, c)
        # the channel step hears what the kernel wrote: the room and the noise
        return out if item.channel is None else self._run_channel(out, [out.shape[1]], [item.channel])

    def augment_batch(self, waveforms: torch.Tensor, lengths=None, noise: str = "device",
                      seed: Optional[int] = None, return_lengths: bool = False):
        """``augment`` of every row of a (B, N) batch in ONE launch: clip b is its first ``lengths[b]`` samples (all N
        when ``lengths`` is None), gets its own draws (in row order, as a Dataset calls ``augment`` per item) and its tail
        is written as 0.  ``noise="device"``: the gaussian noise comes from the seeded counter-based generator on the GPU
        (``seed``: 64-bit; None draws one from torch's CPU generator); ``noise="host"``: ``torch.randn`` on the CPU
        generator, one clip after the other, as the reference's ``randn_like``.  Returns (B, N) where the input lives.
        With ``speed=True`` a clip whose speed step fired has ``n'`` samples instead of its ``n``: the result is
        (B, max n'), and ``noise="host"`` draws ``randn(n')``.  ``return_lengths=True`` returns ``(result, lengths)``
        with the clips' lengths after the chain as an int32 (B,) host tensor.  With ``pitch=True`` the pitch step runs
        behind the speed step; it keeps every clip's length."""
        if noise not in ("device", "host"):
            raise ValueError(f"augment_batch: noise must be 'device' or 'host', got {noise!r}")
        if not isinstance(waveforms, torch.Tensor) or not waveforms.dtype.is_floating_point:
            raise TypeError("augment_batch: expected a floating-point torch.Tensor")
        if waveforms.dim() != 2 or waveforms.shape[1] < 1:
            raise ValueError(f"augment_batch: expected (B, N), got {tuple(waveforms.shape)}")
        b, n = waveforms.shape
        if lengths is not None:
            lengths = [int(v) for v in (lengths.tolist() if isinstance(lengths, torch.Tensor) else lengths)]
            if len(lengths) != b or any(v < 1 or v > n for v in lengths):
                raise ValueError(f"augment_batch: need {b} lengths in 1..{n}")
        items = [self.draw_item_channel(v) for v in (lengths if lengths is not None else [n] * b)]
        col = _chain.columns(items, self)
        clips, new_lens = col["clips"], [it.length for it in items]
        gaussian = None
        if noise == "host":
            # rows of n' samples; _run_chain cuts the matrix to (B, max n') when a speed step fired
            gaussian = torch.zeros((b, max(new_lens + [n])), dtype=torch.float32)
            for i, c in enumerate(clips):
                if c.gaussian:
                    gaussian[i, :new_lens[i]] = torch.randn(new_lens[i])
        if seed is None:
            seed = int(torch.randint(0, 2**62, (1,)).item()) if noise == "device" else 0
        out = self._run_chain(waveforms, clips, lengths, col["pairs"], col["steps"], gaussian, int(seed), rirs=col["rirs"])
        if any(it.channel is not None for it in items):  # no channel coin fired: the launches of a batch without the step
            out = self._run_channel(out, new_lens, col["channels"])
        return (out, torch.tensor(new_lens, dtype=torch.int32)) if return_lengths else out


def _mix(x1: torch.Tensor, x2: torch.Tensor, lam: np.ndarray, index: Optional[torch.Tensor], who: str) -> torch.Tensor:
    """rows of x1 (B rows, or one row of everything) mixed with rows of x2: one ``cough_mix_rows`` launch."""
    dev = cuda_device()
    a = x1.detach().to(device=dev, dtype=torch.float32).contiguous()
    b = x2.detach().to(device=dev, dtype=torch.float32).contiguous()
    rows = len(lam)
    if a.numel() % rows or b.numel() != a.numel():
        raise ValueError(f"{who}: shapes {tuple(x1.shape)} and {tuple(x2.shape)} do not mix")
    out = torch.empty_like(a)
    lam64 = np.asarray(lam, dtype=np.float64)
    coef = torch.from_numpy(np.stack([lam64, 1.0 - lam64], axis=1).astype(np.float32)).to(dev)
    idx = index.to(device=dev, dtype=torch.int32).contiguous() if index is not None else None
    if out.numel():
        _lib.check(_lib.load().cough_mix_rows(a.data_ptr(), b.data_ptr(), idx.data_ptr() if idx is not None else None,
                                              out.data_ptr(), rows, a.numel() // rows, coef.data_ptr(),
                                              torch.cuda.current_stream(dev).cuda_stream), "cough_mix_rows")
    return out.to(x1.device)


def mix_coefficients(lam) -> np.ndarray:
    """(B, 2) float32 ``(lam, 1 - lam)``, each formed in float64 and then rounded: the coefficients ``_mix`` hands to
    ``cough_mix_rows`` and ``mix_batch_rows`` expects."""
    lam64 = np.asarray(lam, dtype=np.float64).reshape(-1)
    return np.stack([lam64, 1.0 - lam64], axis=1).astype(np.float32)


def mix_batch_rows(x: torch.Tensor, labels: torch.Tensor, perm: torch.Tensor,
                   coef: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """MixUp of a device batch with a permutation of itself in ONE launch (``cough_mix_batch`` of
    ``libcough_amd_soft.so``): ``x`` (B, ...) float32, ``labels`` (B,) int64, ``perm`` (B,) int32, ``coef`` (B, 2) float32
    (``mix_coefficients``), all contiguous on the GPU.  Returns ``(mixed x, soft targets (B, 2) float32)``:
    ``lam x[b] + (1 - lam) x[perm[b]]`` and the same mix of the one-hot labels, both bit-equal to what
    ``MixUp.mix_batch(x, onehot(labels), perm)`` gives with the same λ.  A ``perm`` entry outside ``0..B-1`` leaves its
    row as it is.  Nothing is read back."""
    b = int(x.shape[0]) if x.dim() else 0
    want = (("x", x, torch.float32, None), ("labels", labels, torch.int64, (b,)), ("perm", perm, torch.int32, (b,)),
            ("coef", coef, torch.float32, (b, 2)))
    for name, t, dtype, shape in want:
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_contiguous() or t.device != x.device:
            raise ValueError(f"mix_batch_rows: {name} must be a contiguous {dtype} tensor on {x.device}")
        if shape is not None and tuple(t.shape) != shape:
            raise ValueError(f"mix_batch_rows: {name} must have shape {shape}, got {tuple(t.shape)}")
    if b < 1 or x.numel() < b:
        raise ValueError(f"mix_batch_rows: expected x (B, ...) with B >= 1 and at least one value per row, got {tuple(x.shape)}")
    if x.device.type != "cuda":
        raise RuntimeError(f"mix_batch_rows: the tensors live on {x.device}; the kernel needs them on the GPU (there is "
                           "no CPU fallback)")
    out = torch.empty_like(x)
    soft = torch.empty((b, 2), dtype=torch.float32, device=x.device)
    _lib.check_soft(_lib.load_soft().cough_mix_batch(x.data_ptr(), labels.data_ptr(), perm.data_ptr(), coef.data_ptr(), b,
                                                     x.numel() // b, out.data_ptr(), soft.data_ptr(),
                                                     torch.cuda.current_stream(x.device).cuda_stream), "cough_mix_batch")
    return out, soft


class MixUp:
    def __init__(self, alpha: float = 0.2):
        self.alpha = alpha
        self.last_lam: Optional[np.ndarray] = None

    def __call__(self, x1: torch.Tensor, y1: torch.Tensor, x2: torch.Tensor,
                 y2: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """The reference's pair call (:353-369): one ``lam = np.random.beta(alpha, alpha)``, x and y mixed with it."""
        lam = np.random.beta(self.alpha, self.alpha)
        self.last_lam = np.array([lam])
        if x1.shape != x2.shape or y1.shape != y2.shape:
            raise ValueError(f"MixUp: shapes differ: {tuple(x1.shape)} / {tuple(x2.shape)}, {tuple(y1.shape)} / {tuple(y2.shape)}")
        return _mix(x1, x2, self.last_lam, None, "MixUp"), _mix(y1, y2, self.last_lam, None, "MixUp")

    def mix_batch(self, x: torch.Tensor, y: torch.Tensor,
                  perm: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """MixUp of a batch with a permutation of itself, one λ per row (``np.random.beta(alpha, alpha, size=B)``):
        x[b] <- lam[b] x[b] + (1 - lam[b]) x[perm[b]], the same for the labels y (B, ...).  ``perm`` defaults to
        ``torch.randperm(B)``; the λ of the last call are ``last_lam``."""
        bsz = x.shape[0]
        if y.shape[0] != bsz:
            raise ValueError(f"MixUp.mix_batch: {bsz} inputs but {y.shape[0]} labels")
        perm = torch.randperm(bsz) if perm is None else torch.as_tensor(perm)
        perm = perm.detach().to("cpu", torch.int64).reshape(-1)
        if perm.numel() != bsz or (bsz and (int(perm.min()) < 0 or int(perm.max()) >= bsz)):
            raise ValueError(f"MixUp.mix_batch: perm must hold {bsz} row indices in 0..{bsz - 1}")
        lam = np.random.beta(self.alpha, self.alpha, size=bsz)
        self.last_lam = lam
        if bsz == 0:
            return x, y
        return _mix(x, x, lam, perm, "MixUp.mix_batch"), _mix(y, y, lam, perm, "MixUp.mix_batch")


def create_augmentation_pipeline(sample_rate: int = 16000, noise_dir: Optional[str] = None, p_augment: float = 0.5,
                                 use_spec_augment: bool = True, speed: bool = False,
                                 speed_range: Tuple[float, float] = (0.9, 1.1), pitch: bool = False,
                                 pitch_range: Tuple[int, int] = (-2, 2),
                                 phase_lock: bool = False, reverb=None, channel=None, p_clip: float = 0.3,
                                 clip_range: Tuple[float, float] = (0.25, 1.0)) -> Tuple[AudioAugmentor, Optional[SpecAugment]]:
    """(AudioAugmentor, SpecAugment or None), reference :372-398; ``speed`` / ``speed_range`` / ``pitch`` /
    ``pitch_range`` / ``phase_lock`` / ``reverb`` / ``channel`` / ``p_clip`` / ``clip_range`` go to the augmentor."""
    audio_aug = AudioAugmentor(sample_rate=sample_rate, noise_dir=noise_dir, p_augment=p_augment, speed=speed,
                               speed_range=speed_range, pitch=pitch, pitch_range=pitch_range, phase_lock=phase_lock,
                               reverb=reverb, channel=channel, p_clip=p_clip, clip_range=clip_range)
    spec_aug = SpecAugment(p=p_augment) if use_spec_augment else None
    return audio_aug, spec_aug
