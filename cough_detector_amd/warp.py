"""Speed perturbation on the MI355X (``csrc/warp.hip``, ``include/cough_amd_warp.h``).

* ``warp_rows``: every row of a batch resampled by a rate pair of its own in one launch of ``cough_warp_rows`` -- a
  windowed-sinc filter (torchaudio's ``sinc_interp_hann``, width 6, rolloff 0.99) whose coefficients are evaluated per
  tap on the device, so there is no polyphase table.  The rows are read in place from a packed buffer and the time
  shift of the waveform chain is fused into the read, because the chain shifts before it changes the speed.
* ``draw_speed``: the per-row plans (shift, rate pair) and new lengths of a ``draws="device"`` batch, one launch of
  ``cough_draw_speed`` -- a seeded Philox4x32-10 stream per batch.
* ``speed_rate_pair``: ``torchaudio.functional.speed``'s rule, ``(int(factor * sample_rate), sample_rate)``.

The arithmetic and the draw contract are stated in ``include/cough_amd_warp.h`` and restated in numpy in
``tests/warp_ref.py``.  Pitch shift (``cough_detector_amd/pitch.py``) runs ``warp_rows`` behind its time stretch.
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._native import _on_gpu, _stream

PLAN_WORDS = C.sizeof(_lib.CoughWarpPlan) // 4     # 3 int32: shift, orig, new
MAX_LENGTH = 1 << 30


def speed_rate_pair(factor: float, sample_rate: int) -> Tuple[int, int]:
    """(orig, new) of ``torchaudio.functional.speed(waveform, sample_rate, factor)``: the clip is taken to have rate
    ``int(factor * sample_rate)`` and resampled to ``sample_rate``, so a factor above 1 shortens it."""
    return int(factor * sample_rate), int(sample_rate)


def usable_pair(orig: int, new: int) -> bool:
    """Whether ``cough_warp_rows`` resamples by this pair (it copies the row otherwise)."""
    return (1 <= orig <= _lib.WARP_MAX_RATE and 1 <= new <= _lib.WARP_MAX_RATE and orig <= _lib.WARP_MAX_RATIO * new
            and new <= _lib.WARP_MAX_RATIO * orig)


def warped_length(n: int, orig: int, new: int) -> int:
    """``ceil(n * new / orig)`` in exact integer arithmetic: the length ``cough_warp_rows`` gives a row of ``n`` samples
    (``n`` itself for a pair it cannot use)."""
    n = max(0, min(int(n), MAX_LENGTH))
    if not usable_pair(orig, new):
        return n
    return (n * int(new) + int(orig) - 1) // int(orig)


def check_speed_range(speed_range: Sequence[float], sample_rate: int, who: str) -> Tuple[float, float]:
    lo, hi = float(speed_range[0]), float(speed_range[1])
    if not (0.25 <= lo <= hi <= 4.0):
        raise ValueError(f"{who}: speed_range {tuple(speed_range)} must satisfy 1/4 <= lo <= hi <= 4")
    if not (1 <= int(sample_rate) <= _lib.WARP_MAX_RATE and 4 * int(lo * sample_rate) >= sample_rate
            and (hi <= 1.0 or int(hi * sample_rate) < _lib.WARP_MAX_RATE)):
        raise ValueError(f"{who}: sample_rate {sample_rate} with speed_range {tuple(speed_range)} gives a rate pair the "
                         "resampler does not take")
    return lo, hi


def plan_array(plans: Sequence[Tuple[int, int, int]]) -> np.ndarray:
    """(B, 3) int32 ``(shift, orig, new)``: the layout of ``cough_warp_plan``."""
    arr = np.asarray(plans, dtype=np.int64).reshape(-1, PLAN_WORDS)
    return np.clip(arr, -2**31, 2**31 - 1).astype(np.int32)


def warp_rows(src: torch.Tensor, row_offsets_dev: torch.Tensor, lengths_dev: torch.Tensor, plans_dev: torch.Tensor,
              n_samples: int, return_lengths: bool = False):
    """B rows of the packed float32 buffer ``src`` resampled in one launch: row b is the ``lengths_dev[b]`` samples at
    ``row_offsets_dev[b]`` (int64), read in place; ``plans_dev`` is int32 (B, 3), per row ``(shift, orig, new)``.
    Returns (B, n_samples) float32: row b holds its ``n' = ceil(n * new / orig)`` samples (cut at ``n_samples``) and
    zeros behind them; with ``return_lengths`` also the int32 (B,) new lengths, on the device.  ``orig == new`` is a
    bit-exact (shifted) copy.  A plan the kernel cannot use (a rate outside 1..2^20, a ratio beyond 4) counts as
    ``orig == new`` instead of raising: the host never sees the plans."""
    dev = _on_gpu("warp_rows", src=(src, torch.float32), row_offsets_dev=(row_offsets_dev, torch.int64),
                  lengths_dev=(lengths_dev, torch.int32), plans_dev=(plans_dev, torch.int32))
    b = lengths_dev.numel()
    if row_offsets_dev.numel() != b or plans_dev.numel() != b * PLAN_WORDS:
        raise ValueError(f"warp_rows: need {b} row offsets and {b} plans of {PLAN_WORDS} int32")
    out = torch.empty((b, int(n_samples)), dtype=torch.float32, device=dev)
    new_lengths = torch.empty(b, dtype=torch.int32, device=dev) if return_lengths else None
    _lib.check_warp(_lib.load_warp().cough_warp_rows(
        src.data_ptr(), row_offsets_dev.data_ptr(), lengths_dev.data_ptr(), b, plans_dev.data_ptr(), out.data_ptr(),
        int(n_samples), new_lengths.data_ptr() if return_lengths else None, _stream(dev)), "cough_warp_rows")
    return (out, new_lengths) if return_lengths else out


def draw_speed(seed: int, lengths_dev: torch.Tensor, p_augment: float, speed_range: Sequence[float],
               sample_rate: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The speed draws of one batch, on the device: ``(plans int32 (B, 3), new lengths int32 (B,))``.  Row b gets the
    time shift the batch's record would carry (slot 0 of ``include/cough_amd_draws.h``, drawn for its original length)
    and, when its coin fires with probability ``p_augment``, the pair ``speed_rate_pair(uniform(*speed_range),
    sample_rate)``; otherwise ``(sample_rate, sample_rate)``.  The same ``seed`` gives the same draws."""
    lo, hi = check_speed_range(speed_range, sample_rate, "draw_speed")
    dev = _on_gpu("draw_speed", lengths_dev=(lengths_dev, torch.int32))
    b = lengths_dev.numel()
    plans = torch.empty((b, PLAN_WORDS), dtype=torch.int32, device=dev)
    new_lengths = torch.empty(b, dtype=torch.int32, device=dev)
    _lib.check_warp(_lib.load_warp().cough_draw_speed(int(seed) & (2**64 - 1), b, lengths_dev.data_ptr(), float(p_augment),
                                                      lo, hi, int(sample_rate), plans.data_ptr(), new_lengths.data_ptr(),
                                                      _stream(dev)), "cough_draw_speed")
    return plans, new_lengths


def clear_shifts(clips_dev: torch.Tensor) -> None:
    """Zero the shift of device records (``draw_batch``'s (B, 40) uint8) whose rows the resampler has already shifted."""
    dev = _on_gpu("clear_shifts", clips_dev=(clips_dev, torch.uint8))
    size = C.sizeof(_lib.CoughAugClip)
    if clips_dev.numel() % size:
        raise ValueError(f"clear_shifts: expected records of {size} bytes")
    _lib.check_warp(_lib.load_warp().cough_clear_shifts(clips_dev.data_ptr(), clips_dev.numel() // size, _stream(dev)),
                    "cough_clear_shifts")


def drawn_width(row_len: int, speed_range: Sequence[float], sample_rate: int) -> int:
    """The output width that holds every row of a ``draw_speed`` batch whose longest row has ``row_len`` samples:
    ``ceil(row_len * sample_rate / int(lo * sample_rate))`` (``row_len`` itself when ``lo`` is above 1: a row whose
    coin did not fire keeps its length), computed on the host (the draws are never read back)."""
    if row_len <= 0:
        return 0
    return max(int(row_len), warped_length(row_len, int(float(speed_range[0]) * sample_rate), int(sample_rate)))
