"""Room reverberation on the MI355X (``csrc/reverb.hip``, ``include/cough_amd_reverb.h``).

Every clip the project trains on is close-mic and dry; the detector sits in a room.  Convolving a clip with a room
impulse response (RIR) is the standard far-field augmentation, and the one step of the waveform chain that does not keep
a dry clip dry.  One response per clip: no moving sources, no microphone response.

* ``RirBank``: a bank of responses -- host float32 taps, the packed device taps and, prepared lazily and once per device,
  the spectra ``cough_reverb_rows`` multiplies with (``cough_reverb_prepare``).  ``RirBank.from_directory`` reads
  measured responses from WAVE files; ``synth_rirs`` makes synthetic ones (exponentially decaying noise behind a direct
  path).
* ``reverb_rows``: every row of a batch convolved with a response of its own in one launch -- FFT overlap-save, a
  16384-point complex transform held in the LDS of one workgroup per 16384 outputs.  The rows are read in place from a
  packed buffer and the time shift of the waveform chain is fused into the read.
* ``draw_reverb``: the per-row plans of a ``draws="device"`` batch, one launch of ``cough_draw_reverb``.
* ``reverberate_bank``: a ``DeviceClipBank`` convolved clip by clip, tails kept -- far-field coughs and far-field speech
  for ``draw_scene_plan`` / ``compose_scenes``.

The arithmetic, the rules for non-finite and silent input, the error bound and the draw contract are stated in
``include/cough_amd_reverb.h`` and restated in numpy in ``tests/reverb_ref.py``.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._native import _on_gpu, _stream, cuda_device

FFT = 16384                       # COUGH_REVERB_FFT: the outputs of one span
MAX_TAPS = 8193                   # COUGH_REVERB_MAX_TAPS
MAX_LENGTH = 1 << 30              # COUGH_REVERB_MAX_LENGTH
PLAN_WORDS = 4                    # cough_reverb_plan: int32 shift, rir, out_len, reserved
BOUND_K = 160                     # COUGH_REVERB_BOUND_K


class RirBank:
    """A bank of room impulse responses.  ``responses``: 1-D float arrays of 1 .. 8193 finite taps each (a longer one is
    refused: cut it first, as ``from_directory`` does).  ``taps`` are the host float32 copies, ``lengths`` (int32) and
    ``offsets`` (int64) place them in the packed buffer ``packed``.  ``device_taps(dev)`` and ``workspace(dev)`` upload
    and prepare on first use and keep the result per device."""

    def __init__(self, responses: Sequence):
        taps = []
        for k, h in enumerate(responses):
            a = np.ascontiguousarray(h.detach().cpu().numpy() if isinstance(h, torch.Tensor) else np.asarray(h)).astype(np.float32)
            if a.ndim != 1 or a.size < 1:
                raise ValueError(f"RirBank: response {k} has shape {a.shape}; expected (L,) with L >= 1")
            if a.size > MAX_TAPS:
                raise ValueError(f"RirBank: response {k} has {a.size} taps, at most {MAX_TAPS} fit (cut it)")
            if not np.isfinite(a).all():
                raise ValueError(f"RirBank: response {k} holds a NaN or an Inf")
            taps.append(a)
        if not taps:
            raise ValueError("RirBank: no responses")
        self.taps: List[np.ndarray] = taps
        self.lengths = np.array([a.size for a in taps], dtype=np.int32)
        self.offsets = np.concatenate([[0], np.cumsum(self.lengths[:-1], dtype=np.int64)]).astype(np.int64)
        self.packed = np.concatenate(taps)
        self._taps_dev: Dict[torch.device, torch.Tensor] = {}
        self._workspace: Dict[torch.device, tuple] = {}      # device -> (workspace, ready event, the preparing stream)

    def __len__(self) -> int:
        return len(self.taps)

    @property
    def max_taps(self) -> int:
        return int(self.lengths.max())

    def device_taps(self, dev: Optional[torch.device] = None) -> torch.Tensor:
        dev = torch.device(dev) if dev is not None else cuda_device()
        if dev not in self._taps_dev:
            self._taps_dev[dev] = torch.from_numpy(self.packed).to(dev)
        return self._taps_dev[dev]

    def workspace(self, dev: Optional[torch.device] = None) -> torch.Tensor:
        """The prepared bank on ``dev`` (uint8, ``cough_reverb_bank_bytes`` long): the twiddle table and one spectrum per
        response.  Prepared on the first call, on the stream that is current then; an event recorded behind the
        preparation is waited for by the stream that is current at every later call, so a caller on another stream never
        reads spectra that are still being written (a stream-side wait: the host does not block)."""
        dev = torch.device(dev) if dev is not None else cuda_device()
        if dev not in self._workspace:
            ws = torch.empty(bank_bytes(len(self)), dtype=torch.uint8, device=dev)
            prepare(self.device_taps(dev), self.offsets, self.lengths, ws)
            ready = torch.cuda.Event()
            ready.record(torch.cuda.current_stream(dev))
            self._workspace[dev] = (ws, ready, torch.cuda.current_stream(dev))
        ws, ready, first = self._workspace[dev]
        if torch.cuda.current_stream(dev) != first:
            torch.cuda.current_stream(dev).wait_event(ready)
        return ws

    @staticmethod
    def conditioned(h) -> np.ndarray:
        """A measured response made ready for the bank, in float64: it starts at its largest ``|h|`` (what lies in front
        of the direct path is the recording's lead-in), is cut to 8193 taps and scaled to unit L2 norm, so a reverberated
        clip keeps roughly its power."""
        a = np.asarray(h, dtype=np.float64).reshape(-1)
        if a.size < 1 or not np.isfinite(a).all() or not a.any():
            raise ValueError("RirBank: a response must hold finite samples that are not all zero")
        a = a[int(np.argmax(np.abs(a))):][:MAX_TAPS]
        return a / math.sqrt(float((a * a).sum()))

    @classmethod
    def from_directory(cls, directory, preprocessor) -> "RirBank":
        """The WAVE files of ``directory`` (sorted by name) as a bank: loaded, resampled to the preprocessor's rate and
        mixed to mono through ``preprocessor.load_audio`` / ``resample`` / ``to_mono``, then ``conditioned``."""
        from pathlib import Path
        responses = []
        for f in sorted(Path(directory).iterdir()):
            if f.suffix.lower() == ".wav":
                w, sr = preprocessor.load_audio(str(f))
                mono = preprocessor.to_mono(preprocessor.resample(w, sr)).detach().cpu().numpy().reshape(-1)
                responses.append(cls.conditioned(mono).astype(np.float32))
        if not responses:
            raise ValueError(f"{directory}: no WAVE files")
        return cls(responses)


def synth_rir_taps(n: int, sample_rate: int = 16000, rt60_range: Tuple[float, float] = (0.15, 0.5),
                   drr_db_range: Tuple[float, float] = (0.0, 15.0), seed: int = 0) -> Tuple[List[np.ndarray], np.ndarray]:
    """``synth_rirs`` before the rounding: the float64 taps of every response and the table of the draws."""
    if n < 1 or sample_rate < 1:
        raise ValueError(f"synth_rirs: n = {n}, sample_rate = {sample_rate}")
    (r_lo, r_hi), (d_lo, d_hi) = rt60_range, drr_db_range
    if not (0.0 < r_lo <= r_hi) or not (d_lo <= d_hi) or not all(map(math.isfinite, (r_lo, r_hi, d_lo, d_hi))):
        raise ValueError(f"synth_rirs: rt60_range {tuple(rt60_range)} must be positive and both ranges ordered and finite")
    rng = np.random.Generator(np.random.Philox(int(seed)))
    gap = int(0.002 * sample_rate)                   # taps 1 .. gap-1 are zero: the first reflection is 2 ms away
    taps, table = [], np.zeros((n, 3), dtype=np.float64)
    for r in range(n):
        rt60 = float(rng.uniform(r_lo, r_hi))
        drr_db = float(rng.uniform(d_lo, d_hi))
        L = min(MAX_TAPS, int(math.ceil(rt60 * sample_rate)))
        h = np.zeros(max(L, 1), dtype=np.float64)
        h[0] = 1.0
        if L > max(gap, 1):
            k = np.arange(max(gap, 1), L, dtype=np.float64)
            tail = rng.standard_normal(k.size) * np.exp(-3.0 * math.log(10.0) * k / (rt60 * sample_rate))
            energy = float((tail * tail).sum())
            if energy > 0.0:                         # direct-to-reverberant ratio: 1 / sum(tail^2) = 10^(drr_db / 10)
                h[max(gap, 1):] = tail * math.sqrt(10.0 ** (-drr_db / 10.0) / energy)
        h /= math.sqrt(float((h * h).sum()))
        taps.append(h)
        table[r] = (rt60, drr_db, h.size)
    return taps, table


def synth_rirs(n: int, sample_rate: int = 16000, rt60_range: Tuple[float, float] = (0.15, 0.5),
               drr_db_range: Tuple[float, float] = (0.0, 15.0), seed: int = 0) -> Tuple[RirBank, np.ndarray]:
    """``n`` synthetic responses and the (n, 3) float64 table of what was drawn for each: ``(rt60, drr_db, L)``.

    The draws come from ``numpy.random.Generator(numpy.random.Philox(seed))``, response by response in this order:
    ``rt60 = uniform(*rt60_range)``, ``drr_db = uniform(*drr_db_range)``, then the tail's ``standard_normal(L - gap)``
    in one call.  ``L = min(8193, ceil(rt60 * sample_rate))``; ``h[0] = 1`` is the direct path; taps ``1 .. gap - 1``
    with ``gap = int(0.002 * sample_rate)`` are zero; from tap ``gap`` on the tail is ``g[k] * exp(-3 ln10 * k / (rt60 *
    sample_rate))`` -- 60 dB down after ``rt60`` seconds -- scaled in float64 so that the direct-to-reverberant ratio
    ``10 log10(h[0]^2 / sum(tail^2))`` is exactly ``drr_db``.  The whole response is then scaled to unit L2 norm and
    rounded once to float32.  Host work: a bank is about 100 x 8193 floats, built once."""
    taps, table = synth_rir_taps(n, sample_rate, rt60_range, drr_db_range, seed)
    return RirBank([h.astype(np.float32) for h in taps]), table


# ------------------------------------------------------------------------------------------------ the C ABI
def bank_bytes(n_rirs: int) -> int:
    """``cough_reverb_bank_bytes``: the workspace of a prepared bank."""
    got = int(_lib.load_reverb().cough_reverb_bank_bytes(int(n_rirs)))
    if got == 0:
        raise ValueError(f"bank_bytes: n_rirs = {n_rirs}")
    return got


def prepare(taps_dev: torch.Tensor, offsets: np.ndarray, lengths: np.ndarray, workspace: torch.Tensor) -> None:
    """``cough_reverb_prepare``: the spectra of the packed responses ``taps_dev`` (float32, on the device; response r is
    ``lengths[r]`` taps at ``offsets[r]``, host arrays) into ``workspace`` (uint8, on the device)."""
    dev = _on_gpu("prepare", taps_dev=(taps_dev, torch.float32), workspace=(workspace, torch.uint8))
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    lengths = np.ascontiguousarray(lengths, dtype=np.int32)
    if offsets.size != lengths.size:
        raise ValueError(f"prepare: {offsets.size} offsets but {lengths.size} lengths")
    if lengths.size and int((offsets + lengths).max()) > taps_dev.numel():
        raise ValueError("prepare: a response ends behind the packed taps")
    _lib.check_reverb(_lib.load_reverb().cough_reverb_prepare(
        taps_dev.data_ptr(), offsets.ctypes.data_as(C.POINTER(C.c_longlong)), lengths.ctypes.data_as(C.POINTER(C.c_int)),
        int(lengths.size), workspace.data_ptr(), workspace.numel(), _stream(dev)), "cough_reverb_prepare")


def plan_array(plans: Sequence[Sequence[int]], n_rirs: Optional[int] = None, width: Optional[int] = None) -> np.ndarray:
    """(B, 4) int32: ``(shift, rir, out_len)`` per row in the layout of ``cough_reverb_plan`` (``rir = -1``: the row is
    copied).  With ``n_rirs`` / ``width`` the plans are checked as the host must check them, before anything is launched:
    ``rir >= n_rirs``, ``rir < -1``, ``out_len < 0`` and ``out_len > width`` raise ValueError."""
    wide = np.zeros((len(plans), PLAN_WORDS), dtype=np.int64)
    for k, (shift, rir, out_len) in enumerate(plans):
        wide[k, :3] = (max(-2**31, min(2**31 - 1, int(shift))), max(-2**31, min(2**31 - 1, int(rir))), min(2**31, int(out_len)))
    return check_plans(wide, n_rirs, 2**31 - 1 if width is None else width, "plan_array")


def check_plans(plans: np.ndarray, n_rirs: Optional[int], width: int, who: str = "reverb_rows") -> np.ndarray:
    """The one place that refuses host plans ((B, 4) integers): ``rir < -1``, ``rir >= n_rirs`` (when ``n_rirs`` is
    given), ``out_len < 0`` and ``out_len > width`` raise ValueError.  Returns them as contiguous int32."""
    arr = np.asarray(plans)
    if arr.ndim != 2 or arr.shape[1] != PLAN_WORDS or arr.dtype.kind not in "iu":
        raise ValueError(f"{who}: host plans must be (B, {PLAN_WORDS}) integers, got {arr.dtype} {arr.shape}")
    bad = (arr[:, 1] < -1) | (arr[:, 2] < 0) | (arr[:, 2] > width)
    if n_rirs is not None:
        bad |= arr[:, 1] >= n_rirs
    if bad.any():
        k = int(np.nonzero(bad)[0][0])
        raise ValueError(f"{who}: row {k} has rir = {int(arr[k, 1])}" + (f" (bank of {n_rirs})" if n_rirs is not None else "")
                         + f" and out_len = {int(arr[k, 2])} (width {width})")
    return np.ascontiguousarray(arr, dtype=np.int32)


def reverb_rows(src: torch.Tensor, row_offsets_dev: torch.Tensor, lengths_dev: torch.Tensor,
                plans: Union[np.ndarray, torch.Tensor], width: int, bank: RirBank) -> torch.Tensor:
    """B rows of the packed float32 buffer ``src`` convolved in one launch: row b is the ``lengths_dev[b]`` samples at
    ``row_offsets_dev[b]`` (int64), read in place.  ``plans``: per row a ``cough_reverb_plan`` -- a host array
    (``plan_array``), which is checked against the bank and ``width`` before anything is launched and then uploaded, or
    an int32 (B, 4) tensor on the device (``draw_reverb``), whose entries the kernel makes harmless instead (a response
    that does not exist copies the row, ``out_len`` is clamped to ``0 .. width``).  Returns (B, width) float32: row b
    holds ``y[0 .. out_len-1]`` and ``+0.0`` behind; a row with ``rir = -1`` holds its shifted copy."""
    dev = _on_gpu("reverb_rows", src=(src, torch.float32), row_offsets_dev=(row_offsets_dev, torch.int64),
                  lengths_dev=(lengths_dev, torch.int32))
    b, width = lengths_dev.numel(), int(width)
    if not 1 <= width <= MAX_LENGTH:
        raise ValueError(f"reverb_rows: width = {width} must lie in 1..2^30")
    if not isinstance(plans, torch.Tensor):
        plans = torch.from_numpy(check_plans(plans, len(bank), width)).to(dev)
    _on_gpu("reverb_rows", src=(src, torch.float32), plans=(plans, torch.int32))
    if row_offsets_dev.numel() != b or plans.numel() != b * PLAN_WORDS:
        raise ValueError(f"reverb_rows: need {b} row offsets and {b} plans of {PLAN_WORDS} words")
    ws = bank.workspace(dev)
    out = torch.empty((b, max(width, 0)), dtype=torch.float32, device=dev)
    _lib.check_reverb(_lib.load_reverb().cough_reverb_rows(
        src.data_ptr(), row_offsets_dev.data_ptr(), lengths_dev.data_ptr(), b, plans.data_ptr(), ws.data_ptr(), len(bank),
        out.data_ptr(), width, _stream(dev)), "cough_reverb_rows")
    return out


def draw_reverb(seed: int, lengths_dev: torch.Tensor, p_augment: float, bank: Union[RirBank, int]) -> torch.Tensor:
    """The reverb draws of one batch, on the device: int32 (B, 4) plans.  Row b's coin fires with probability
    ``p_augment``; it then draws a response uniformly from the bank (as ``random.randrange``), otherwise ``-1``.
    ``out_len`` is the row's length: the step keeps it.  The same ``seed`` gives the same draws."""
    dev = _on_gpu("draw_reverb", lengths_dev=(lengths_dev, torch.int32))
    b = lengths_dev.numel()
    plans = torch.empty((b, PLAN_WORDS), dtype=torch.int32, device=dev)
    _lib.check_reverb(_lib.load_reverb().cough_draw_reverb(
        int(seed) & (2**64 - 1), b, lengths_dev.data_ptr(), float(p_augment), bank if isinstance(bank, int) else len(bank),
        plans.data_ptr(), _stream(dev)), "cough_draw_reverb")
    return plans


def reverberate_bank(bank, rirs: RirBank, index: Sequence[int], keep_tail: bool = True, max_elements: int = 1 << 26):
    """A ``DeviceClipBank`` whose clip ``i`` is clip ``i`` of ``bank`` convolved with response ``index[i]`` of ``rirs``
    (``-1``: the clip as it is); the labels stay.  With ``keep_tail`` a convolved clip is ``n + L - 1`` samples long, the
    full convolution; without, ``n``.  Far-field coughs and far-field speech for ``draw_scene_plan`` / ``compose_scenes``:
    the SNR drawn there is then that of the reverberant cough.  The rows are convolved in groups whose dense matrix holds
    at most ``max_elements`` floats, one launch and one cut per group."""
    from .data import DeviceClipBank
    index = np.asarray(index, dtype=np.int64).reshape(-1)
    if index.size != len(bank):
        raise ValueError(f"reverberate_bank: {len(bank)} clips but {index.size} response indices")
    if index.size and (index.min() < -1 or index.max() >= len(rirs)):
        raise ValueError(f"reverberate_bank: response indices must lie in -1 .. {len(rirs) - 1}")
    n = bank.lengths.numpy().astype(np.int64)
    taps = np.where(index >= 0, rirs.lengths[np.maximum(index, 0)].astype(np.int64), 1)
    out_len = n + taps - 1 if keep_tail else n
    if index.size and out_len.max() > MAX_LENGTH:
        raise ValueError("reverberate_bank: a clip is longer than 2^30 samples")
    dev, parts, at = bank.device, [], 0
    while at < index.size:
        end, width = at + 1, int(out_len[at])
        while end < index.size and max(width, int(out_len[end])) * (end + 1 - at) <= max_elements:
            width, end = max(width, int(out_len[end])), end + 1
        rows, width = slice(at, end), max(width, 1)        # a group of empty clips still is one column wide
        plans = plan_array([(0, int(r), int(m)) for r, m in zip(index[rows], out_len[rows])], len(rirs), width)
        dense = reverb_rows(bank.data, bank.offsets_dev[rows].contiguous(), bank.lengths_dev[rows].contiguous(), plans, width, rirs)
        k = end - at
        matrix = DeviceClipBank.from_packed(dense.reshape(-1), [width] * k, [0] * k)
        kept = np.nonzero(out_len[rows] > 0)[0]            # an empty clip stays empty: nothing of it is cut out
        if kept.size:
            parts.append(matrix.cut(kept, np.zeros(kept.size, dtype=np.int32), out_len[rows][kept]).data)
        at = end
    data = torch.cat(parts) if parts else torch.zeros(0, dtype=torch.float32, device=dev)
    return DeviceClipBank.from_packed(data, out_len, bank.labels.numpy())
