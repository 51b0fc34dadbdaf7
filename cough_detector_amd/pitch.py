"""Pitch shift on the MI355X (``csrc/pitch.hip``, ``include/cough_amd_pitch.h``).

A pitch shift by ``n_steps`` semitones is a time stretch by ``rate = 2 ** (-n_steps / 12)`` that keeps the pitch,
followed by a resampling from ``int(sample_rate / rate)`` to ``sample_rate`` that brings the clip back to its length
and moves the pitch (``torchaudio.functional.pitch_shift``).

* ``stretch_rows``: every row of a batch stretched by a rate of its own in one launch of ``cough_stretch_rows`` -- a
  float64 phase vocoder (n_fft 512, hop 128, Hann) with a magnitude floor, one workgroup per row; the spectra stay in
  LDS.  The rows are read in place from a packed buffer and the time shift of the waveform chain is fused into the read.
  A row whose plan carries the mode ``PHASE_LOCK`` is stretched with identity phase locking, which keeps a steady
  tone's level (the plain vocoder returns a 440 Hz tone at 0.6 of it); mode 0, the default everywhere, is the plain
  vocoder.
* ``pitch_shift_rows``: ``stretch_rows``, then ``warp_rows`` (``cough_detector_amd/warp.py``) on the stretched rows.
* ``draw_pitch``: the per-row plans of both launches for a ``draws="device"`` batch, one launch of ``cough_draw_pitch``
  -- a seeded Philox4x32-10 stream per batch.
* ``pitch_rate`` / ``pitch_rate_pair`` / ``stretched_length``: the host's side of the same arithmetic.

The arithmetic and the draw contract are stated in ``include/cough_amd_pitch.h`` and restated in numpy in
``tests/pitch_ref.py`` (the locked mode in ``tests/pitch_lock_ref.py``).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from . import warp as _warp
from ._native import _on_gpu, _stream

PLAN_BYTES = C.sizeof(_lib.CoughStretchPlan)       # 16: int32 shift, int32 reserved, float64 rate
MAX_LENGTH = _lib.PITCH_MAX_LENGTH
MIN_STRETCH_LENGTH = 257                           # the reflect padding of the first and last frame needs 257 samples
PHASE_LOCK = 1                                     # COUGH_STRETCH_PHASE_LOCK: the mode bit of a plan's `reserved` word
_PLAN_DTYPE = np.dtype([("shift", np.int32), ("reserved", np.int32), ("rate", np.float64)])
_STEP_DTYPE = np.dtype([("rate", np.float64), ("orig", np.int32), ("reserved", np.int32)])


def pitch_rate(n_steps: int) -> float:
    """The stretch rate of a shift by ``n_steps`` semitones: ``2 ** (-n_steps / 12)`` (up: below 1, the clip gets longer
    before the resampler shortens it again)."""
    return 2.0 ** (-n_steps / 12)


def pitch_rate_pair(n_steps: int, sample_rate: int) -> Tuple[int, int]:
    """(orig, new) of the resampling that follows the stretch: ``(int(sample_rate / rate), sample_rate)``."""
    return int(sample_rate / pitch_rate(n_steps)), int(sample_rate)


def stretches(rate: float, n: int) -> bool:
    """Whether ``cough_stretch_rows`` stretches a row of ``n`` samples at this rate (it copies the row otherwise)."""
    return bool(0.5 <= rate <= 2.0 and rate != 1.0 and n >= MIN_STRETCH_LENGTH)


def stretched_length(n: int, rate: float) -> int:
    """``rint(n / rate)``, half to even: the length ``cough_stretch_rows`` gives a row of ``n`` samples (``n`` itself
    for a row it copies)."""
    n = max(0, min(int(n), MAX_LENGTH))
    return int(np.rint(n / rate)) if stretches(rate, n) else n


def check_pitch_range(pitch_range: Sequence[int], who: str) -> Tuple[int, int]:
    lo, hi = pitch_range[0], pitch_range[1]
    if int(lo) != lo or int(hi) != hi or not (-_lib.PITCH_MAX_STEPS <= lo <= hi <= _lib.PITCH_MAX_STEPS):
        raise ValueError(f"{who}: pitch_range {tuple(pitch_range)} must be whole semitones with -12 <= lo <= hi <= 12")
    return int(lo), int(hi)


def plan_array(plans: Sequence[Sequence]) -> np.ndarray:
    """(B, 16) uint8: ``(shift, rate)`` or ``(shift, rate, mode)`` per row in the layout of ``cough_stretch_plan``.  The
    mode (0 when left out) goes into the field ``reserved``: ``PHASE_LOCK`` stretches the row with identity phase locking,
    0 with the plain vocoder; the kernel reads bit 0 only."""
    arr = np.zeros(len(plans), dtype=_PLAN_DTYPE)
    for k, plan in enumerate(plans):
        shift, rate, mode = plan if len(plan) == 3 else tuple(plan) + (0,)
        arr[k] = (max(-2**31, min(2**31 - 1, int(shift))), int(mode), float(rate))
    return arr.view(np.uint8).reshape(len(plans), PLAN_BYTES)


def step_table(pitch_range: Sequence[int], sample_rate: int, phase_lock: bool = False) -> np.ndarray:
    """(hi - lo + 1, 16) uint8: per ``n_steps`` in ``lo..hi`` the rate and the resampler's ``orig``, the layout of
    ``cough_pitch_step`` -- computed here so that no device ``pow`` enters the draw.  With ``phase_lock`` every entry
    carries the mode ``PHASE_LOCK`` in its ``reserved`` word, and ``cough_draw_pitch`` hands it to the rows that draw
    semitones other than 0."""
    lo, hi = check_pitch_range(pitch_range, "step_table")
    arr = np.zeros(hi - lo + 1, dtype=_STEP_DTYPE)
    for k, s in enumerate(range(lo, hi + 1)):
        arr[k] = (pitch_rate(s), pitch_rate_pair(s, sample_rate)[0], PHASE_LOCK if phase_lock else 0)
    return arr.view(np.uint8).reshape(hi - lo + 1, PLAN_BYTES)


def stretch_rows(src: torch.Tensor, row_offsets_dev: torch.Tensor, lengths_dev: torch.Tensor, plans_dev: torch.Tensor,
                 n_samples: int, return_lengths: bool = False):
    """B rows of the packed float32 buffer ``src`` stretched in one launch: row b is the ``lengths_dev[b]`` samples at
    ``row_offsets_dev[b]`` (int64), read in place; ``plans_dev`` is uint8 (B, 16), per row a ``cough_stretch_plan``
    (``plan_array``).  Returns (B, n_samples) float32: row b holds its ``n_s = rint(n / rate)`` samples (cut at
    ``n_samples``) and zeros behind them; with ``return_lengths`` also the int32 (B,) new lengths, on the device.  A
    rate of 1, a rate the kernel cannot use (outside [1/2, 2], NaN) and a row shorter than 257 samples give a bit-exact
    (shifted) copy instead of raising: the host never sees the plans."""
    dev = _on_gpu("stretch_rows", src=(src, torch.float32), row_offsets_dev=(row_offsets_dev, torch.int64),
                  lengths_dev=(lengths_dev, torch.int32), plans_dev=(plans_dev, torch.uint8))
    b = lengths_dev.numel()
    if row_offsets_dev.numel() != b or plans_dev.numel() != b * PLAN_BYTES:
        raise ValueError(f"stretch_rows: need {b} row offsets and {b} plans of {PLAN_BYTES} bytes")
    out = torch.empty((b, int(n_samples)), dtype=torch.float32, device=dev)
    new_lengths = torch.empty(b, dtype=torch.int32, device=dev) if return_lengths else None
    _lib.check_pitch(_lib.load_pitch().cough_stretch_rows(
        src.data_ptr(), row_offsets_dev.data_ptr(), lengths_dev.data_ptr(), b, plans_dev.data_ptr(), out.data_ptr(),
        int(n_samples), new_lengths.data_ptr() if return_lengths else None, _stream(dev)), "cough_stretch_rows")
    return (out, new_lengths) if return_lengths else out


def pitch_shift_rows(src: torch.Tensor, row_offsets_dev: torch.Tensor, lengths_dev: torch.Tensor,
                     stretch_plans_dev: torch.Tensor, warp_plans_dev: torch.Tensor, n_samples: int,
                     stretch_width: Optional[int] = None) -> torch.Tensor:
    """The pitch shift of B packed rows in two launches: ``stretch_rows`` into a (B, stretch_width) matrix, then
    ``warp_rows`` on its rows with ``warp_plans_dev`` (int32 (B, 3): ``(0, orig, new)`` per row; the time shift belongs
    in the stretch plan) into (B, n_samples).  With ``n_samples`` the width of the input, the resampler's cut and zero
    fill are torchaudio's crop or pad back to the original length: a row keeps its length ``n``.  (A row shorter than
    ``n_samples`` may carry the few samples by which ``ceil(n_s * new / orig)`` exceeds ``n`` behind its end; the
    chain's next kernel reads ``n`` samples per row.)  ``stretch_width`` must hold the longest stretched row
    (``stretched_length``; a row is cut there otherwise) and defaults to ``2 * n_samples``, which holds any row of up
    to ``n_samples`` samples at any rate."""
    if stretch_width is None:
        stretch_width = min(2 * int(n_samples), _lib.PITCH_MAX_SAMPLES)
    stretched, n_s = stretch_rows(src, row_offsets_dev, lengths_dev, stretch_plans_dev, stretch_width, return_lengths=True)
    b = lengths_dev.numel()
    offs = torch.arange(b, dtype=torch.int64, device=src.device) * int(stretch_width)
    return _warp.warp_rows(stretched.reshape(-1), offs, n_s, warp_plans_dev, n_samples)


def draw_pitch(seed: int, lengths_dev: torch.Tensor, p_augment: float, pitch_range: Sequence[int],
               sample_rate: int, table_dev: Optional[torch.Tensor] = None,
               phase_lock: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The pitch draws of one batch, on the device: ``(stretch plans uint8 (B, 16), warp plans int32 (B, 3), stretched
    lengths int32 (B,))``.  Row b's coin fires with probability ``p_augment``; it then draws ``n_steps`` uniformly
    from ``pitch_range`` (inclusive, as ``random.randint``) and gets the rate ``pitch_rate(n_steps)`` and the pair
    ``pitch_rate_pair(n_steps, sample_rate)``; otherwise, and for 0 semitones, rate 1 and ``(sample_rate,
    sample_rate)``.  ``table_dev``: ``step_table(pitch_range, sample_rate, phase_lock)`` already on the device (uploaded
    here otherwise; ``phase_lock`` is not looked at when the caller brings a table).  A row that draws semitones other
    than 0 gets the mode of its table entry (``PHASE_LOCK`` or 0), every other row mode 0.  The same ``seed`` gives the
    same draws, whatever the mode."""
    lo, hi = check_pitch_range(pitch_range, "draw_pitch")
    if not 1 <= int(sample_rate) <= _lib.WARP_MAX_RATE:
        raise ValueError(f"draw_pitch: sample_rate {sample_rate} must lie in 1..2^20")
    dev = _on_gpu("draw_pitch", lengths_dev=(lengths_dev, torch.int32))
    if table_dev is None:
        table_dev = torch.from_numpy(step_table((lo, hi), sample_rate, phase_lock)).to(dev)
    _on_gpu("draw_pitch", lengths_dev=(lengths_dev, torch.int32), table_dev=(table_dev, torch.uint8))
    if table_dev.numel() != (hi - lo + 1) * PLAN_BYTES:
        raise ValueError(f"draw_pitch: table_dev must hold {hi - lo + 1} entries of {PLAN_BYTES} bytes")
    b = lengths_dev.numel()
    stretch_plans = torch.empty((b, PLAN_BYTES), dtype=torch.uint8, device=dev)
    warp_plans = torch.empty((b, _warp.PLAN_WORDS), dtype=torch.int32, device=dev)
    n_s = torch.empty(b, dtype=torch.int32, device=dev)
    _lib.check_pitch(_lib.load_pitch().cough_draw_pitch(int(seed) & (2**64 - 1), b, lengths_dev.data_ptr(), float(p_augment),
                                                        lo, hi, table_dev.data_ptr(), int(sample_rate),
                                                        stretch_plans.data_ptr(), warp_plans.data_ptr(), n_s.data_ptr(),
                                                        _stream(dev)), "cough_draw_pitch")
    return stretch_plans, warp_plans, n_s


def drawn_width(row_len: int, pitch_range: Sequence[int]) -> int:
    """The width that holds every stretched row of a ``draw_pitch`` batch whose longest row has ``row_len`` samples:
    the length at the largest number of semitones (the smallest rate), and ``row_len`` itself for a row whose coin did
    not fire -- computed on the host (the draws are never read back)."""
    if row_len <= 0:
        return 0
    return max(int(row_len), max(stretched_length(row_len, pitch_rate(s)) for s in range(pitch_range[0], pitch_range[1] + 1)))
