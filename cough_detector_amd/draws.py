"""A training batch's random draws on the MI355X (``csrc/draws.hip``, ``include/cough_amd_draws.h``).

* ``draw_batch``: the per-clip records of ``AudioAugmentor.augment`` (``cough_aug_clip``: shift, gain, the two noise
  steps' coins, SNRs, bank entry and crop start) and SpecAugment's coin and masks per image, written by one launch of
  ``cough_draw_batch`` into device memory -- one thread per row, a seeded Philox4x32-10 stream per batch.
* ``augment_rows_drawn``: ``cough_augment_waveforms``' augmentation with those records, the rows and the noise bank's
  tables all read from device memory; the rows are read in place from the packed clip bank.

The draw contract (which word of which Philox block makes which draw, and the float64 arithmetic on it) is stated in
``include/cough_amd_draws.h`` and restated in numpy in ``tests/draws_ref.py``.  Every draw has the reference's
distribution (``/root/reference/src/augmentation.py``); none of them is the reference's random stream, which comes from
Python's ``random`` and ``torch.rand``: a seeded run repeats itself, not a ``num_workers=0`` reference loader.  The
reference draws its masks in float32 (``torch.rand(1)``); here they are drawn in float64.
"""
from __future__ import annotations

import ctypes as C
from typing import TYPE_CHECKING, Optional, Tuple

import torch

from . import _lib
from ._native import _on_gpu, _stream

if TYPE_CHECKING:                                # the augmentors run the chain, which launches through this module
    from .augmentation import AudioAugmentor, SpecAugment

CLIP_BYTES = C.sizeof(_lib.CoughAugClip)        # 40: one cough_aug_clip


def mask_counts(spec: SpecAugment) -> Tuple[int, int]:
    """(frequency masks, time masks) that ``spec`` draws: an axis whose ``mask_param`` is < 1 draws none."""
    return (spec.n_freq_masks if spec.freq_mask_param >= 1 else 0, spec.n_time_masks if spec.time_mask_param >= 1 else 0)


def draw_batch(seed: int, lengths_dev: torch.Tensor, audio_augmentor: Optional[AudioAugmentor],
               spec_augmentor: Optional[SpecAugment], feature_shape: Tuple[int, int]
               ) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """The draws of one batch, on the device: ``(clips, masks)``.

    ``lengths_dev``: the rows' lengths, int32 (B,) on the GPU.  ``clips``: (B, 40) uint8, one ``cough_aug_clip`` per row
    (what ``augment_rows_drawn`` reads), or None without ``audio_augmentor``.  ``masks``: int32 (3, B, n_masks) -- axis,
    start, end as ``cough_mask_images`` reads them, frequency masks first -- or None when ``spec_augmentor`` is None or
    draws no mask; an image whose coin did not fire has (0, 0, 0) in every mask.  ``feature_shape`` is the images'
    (height, width).  The same ``seed`` (64-bit) gives the same draws; the draws have the reference's distributions, not
    its random stream, and the masks are drawn in float64 where the reference uses float32."""
    dev = _on_gpu("draw_batch", lengths_dev=(lengths_dev, torch.int32))
    b = lengths_dev.numel()
    height, width = int(feature_shape[0]), int(feature_shape[1])
    clips = masks = None
    p_aug, n_bank, bank_lengths = -1.0, 0, None
    if audio_augmentor is not None:
        p_aug = float(audio_augmentor.p_augment)
        if p_aug < 0:
            raise ValueError(f"draw_batch: p_augment = {p_aug} must not be negative")
        n_bank = len(audio_augmentor._bank_lengths)
        if n_bank:
            bank_lengths = audio_augmentor._bank_tables_device(dev)[1]
        clips = torch.empty((b, CLIP_BYTES), dtype=torch.uint8, device=dev)
    spec_p, n_f, n_t, f_param, t_param = -1.0, 0, 0, 0, 0
    if spec_augmentor is not None:
        n_f, n_t = mask_counts(spec_augmentor)
        f_param, t_param = int(spec_augmentor.freq_mask_param), int(spec_augmentor.time_mask_param)
        if n_f + n_t:
            spec_p = float(spec_augmentor.p)
            if spec_p < 0:
                raise ValueError(f"draw_batch: SpecAugment's p = {spec_p} must not be negative")
            masks = torch.empty((3, b, n_f + n_t), dtype=torch.int32, device=dev)
    if b == 0:
        return clips, masks
    ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    m = masks if masks is not None else (None, None, None)
    _lib.check_draws(_lib.load_draws().cough_draw_batch(
        int(seed) & (2**64 - 1), b, lengths_dev.data_ptr(), p_aug, n_bank, ptr(bank_lengths), spec_p, n_f, f_param, n_t,
        t_param, height, width, ptr(clips), ptr(m[0]), ptr(m[1]), ptr(m[2]), _stream(dev)), "cough_draw_batch")
    return clips, masks


def augment_rows_drawn(bank_data: torch.Tensor, row_offsets_dev: torch.Tensor, lengths_dev: torch.Tensor, n_samples: int,
                       clips_dev: torch.Tensor, audio_augmentor: AudioAugmentor, seed: int) -> torch.Tensor:
    """``AudioAugmentor.augment`` of B rows of the packed float32 buffer ``bank_data`` with the device records
    ``clips_dev`` (``draw_batch``'s, (B, 40) uint8): row b is the ``lengths_dev[b]`` samples at ``row_offsets_dev[b]``
    (int64), read in place.  Returns (B, n_samples) float32, each row's tail written as 0; ``n_samples`` is at least the
    longest row.  The gaussian noise comes from the counter-based generator keyed by ``seed``, as with
    ``augment_batch(noise="device")``.  The noise bank's offsets and lengths are uploaded once per augmentor.  A record
    the kernel cannot use (see ``include/cough_amd_draws.h``) loses the step in question instead of raising: the host
    never sees the records."""
    dev = _on_gpu("augment_rows_drawn", bank_data=(bank_data, torch.float32), row_offsets_dev=(row_offsets_dev, torch.int64),
                  lengths_dev=(lengths_dev, torch.int32), clips_dev=(clips_dev, torch.uint8))
    b = lengths_dev.numel()
    if row_offsets_dev.numel() != b or clips_dev.numel() != b * CLIP_BYTES:
        raise ValueError(f"augment_rows_drawn: need {b} row offsets and {b} records of {CLIP_BYTES} bytes")
    lib = _lib.load_draws()
    out = torch.empty((b, int(n_samples)), dtype=torch.float32, device=dev)
    n_bank = len(audio_augmentor._bank_lengths)
    bank = offs = lens = None
    if n_bank:
        bank = audio_augmentor._bank_device(dev)
        offs, lens = audio_augmentor._bank_tables_device(dev)
    if b == 0:
        return out
    ws = torch.empty(max(int(lib.cough_augment_rows_drawn_workspace_bytes(b)), 1), dtype=torch.uint8, device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    _lib.check_draws(lib.cough_augment_rows_drawn(
        bank_data.data_ptr(), row_offsets_dev.data_ptr(), lengths_dev.data_ptr(), b, int(n_samples), clips_dev.data_ptr(),
        ptr(bank), bank.numel() if bank is not None else 0, ptr(offs), ptr(lens), n_bank, int(seed) & (2**64 - 1),
        out.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)), "cough_augment_rows_drawn")
    return out
