"""The capture channel on the MI355X (``csrc/channel.hip``, ``include/cough_amd_channel.h``).

The corpus's two classes come through different recording devices; a classifier that can tell the devices apart needs
to hear neither a cough nor speech.  This is the step of the waveform chain for the device that records: a microphone
response -- a short cascade of second-order IIR sections out of a bank -- and the converter's ceiling, a hard clip
relative to the clip's own peak.  It is drawn per clip, independently of the label, and runs on the matrix the
augmentation kernel wrote: a microphone hears the room and the noise.

* ``ChannelBank``: a bank of cascades of 1 .. 4 sections in scipy's ``sos`` layout (``scipy.signal.butter(...,
  output="sos")``, or a fit to a measured microphone); the prepared blob per device (``cough_channel_prepare``).
* ``synth_channels``: synthetic microphones -- a high-pass, a low-pass and 0 .. 2 peaking sections per entry, from the
  RBJ cookbook formulas.
* ``channel_rows``: every row of a batch filtered and clipped in one launch, one workgroup per row; the serial
  recurrence runs block-parallel, 256 chunks of 64 samples joined by a scan over the workgroup.
* ``draw_channel``: the per-row plans of a ``draws="device"`` batch, one launch of ``cough_draw_channel``.
* ``channel_report``: the long-term average mel spectrum of a bank per label and their difference -- the figure that
  tells whether the classes differ by channel, and whether ``synth_channels``' ranges cover the gap.

The arithmetic, the rules for non-finite and silent input, the blob and the draw contract are stated in
``include/cough_amd_channel.h`` and restated in numpy in ``tests/channel_ref.py``.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._native import _on_gpu, _stream, cuda_device

MAX_SECTIONS = 4                  # COUGH_CHANNEL_MAX_SECTIONS
CHUNK, THREADS = 64, 256          # COUGH_CHANNEL_CHUNK / COUGH_CHANNEL_THREADS
ENTRY_WORDS = 160                 # COUGH_CHANNEL_ENTRY_WORDS
MAX_LENGTH = 1 << 30              # COUGH_CHANNEL_MAX_LENGTH
PLAN_DTYPE = np.dtype([("filter", "<i4"), ("clip_ratio", "<f4")])      # cough_channel_plan, 8 bytes


def check_sos(sos, who: str = "ChannelBank", k: int = 0) -> np.ndarray:
    """One cascade as contiguous float64 (S, 6), refused as ``cough_channel_prepare`` refuses it: a shape other than
    (1 .. 4, 6), a coefficient that is not finite, ``a0 = 0`` and a section outside the stability triangle
    ``|a2| < 1``, ``|a1| < 1 + a2`` (after the division by ``a0``)."""
    a = np.ascontiguousarray(sos.detach().cpu().numpy() if isinstance(sos, torch.Tensor) else np.asarray(sos), dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 6 or not 1 <= a.shape[0] <= MAX_SECTIONS:
        raise ValueError(f"{who}: entry {k} has shape {a.shape}; expected (S, 6) with S in 1..{MAX_SECTIONS}")
    if not np.isfinite(a).all():
        raise ValueError(f"{who}: entry {k} holds a NaN or an Inf")
    if (a[:, 3] == 0.0).any():
        raise ValueError(f"{who}: entry {k} has a section with a0 = 0")
    a1, a2 = a[:, 4] / a[:, 3], a[:, 5] / a[:, 3]
    if not (np.isfinite(a[:, [0, 1, 2, 4, 5]] / a[:, 3:4]).all() and (np.abs(a2) < 1.0).all() and (np.abs(a1) < 1.0 + a2).all()):
        raise ValueError(f"{who}: entry {k} has a section that is not stable (|a2| < 1 and |a1| < 1 + a2 must hold)")
    return a


class ChannelBank:
    """A bank of microphone responses, each a cascade of 1 .. 4 second-order sections in scipy's layout ``(b0, b1, b2,
    a0, a1, a2)``.  ``sos`` are the host float64 copies; ``blob(dev)`` prepares on first use and keeps the result per
    device."""

    def __init__(self, cascades: Sequence, device=None):
        self.sos: List[np.ndarray] = [check_sos(s, "ChannelBank", k) for k, s in enumerate(cascades)]
        if not self.sos:
            raise ValueError("ChannelBank: no entries")
        self.n_sections = np.array([s.shape[0] for s in self.sos], dtype=np.int32)
        self._blob: Dict[torch.device, torch.Tensor] = {}
        if device is not None:
            self.blob(device)

    @classmethod
    def from_sos(cls, cascades: Sequence, device=None) -> "ChannelBank":
        """The bank of a list of (S, 6) arrays; with ``device`` it is prepared there at once."""
        return cls(cascades, device)

    def __len__(self) -> int:
        return len(self.sos)

    def blob(self, dev: Optional[torch.device] = None) -> torch.Tensor:
        """The prepared bank on ``dev`` (uint8, ``cough_channel_bank_bytes`` long).  ``cough_channel_prepare`` returns
        after its copy has completed, so every stream may read the blob afterwards."""
        dev = torch.device(dev) if dev is not None else cuda_device()
        if dev.index is None and dev.type == "cuda":
            dev = torch.device("cuda", torch.cuda.current_device())
        if dev not in self._blob:
            with torch.cuda.device(dev):
                blob = torch.empty(bank_bytes(len(self)), dtype=torch.uint8, device=dev)
                prepare(np.concatenate(self.sos), self.n_sections, blob)
            self._blob[dev] = blob
        return self._blob[dev]


# ------------------------------------------------------------------------------------------------ synthetic microphones
def rbj_section(kind: str, f0: float, sample_rate: float, q: float, gain_db: float = 0.0) -> np.ndarray:
    """One section of the RBJ audio-EQ cookbook as a scipy-layout row, in float64: ``kind`` is ``"highpass"``,
    ``"lowpass"`` or ``"peak"`` (``gain_db`` at ``f0``, bandwidth by ``q``)."""
    w0 = 2.0 * math.pi * float(f0) / float(sample_rate)
    cs, alpha = math.cos(w0), math.sin(w0) / (2.0 * float(q))
    if kind == "lowpass":
        return np.array([(1.0 - cs) / 2.0, 1.0 - cs, (1.0 - cs) / 2.0, 1.0 + alpha, -2.0 * cs, 1.0 - alpha])
    if kind == "highpass":
        return np.array([(1.0 + cs) / 2.0, -(1.0 + cs), (1.0 + cs) / 2.0, 1.0 + alpha, -2.0 * cs, 1.0 - alpha])
    if kind == "peak":
        a = 10.0 ** (float(gain_db) / 40.0)
        return np.array([1.0 + alpha * a, -2.0 * cs, 1.0 - alpha * a, 1.0 + alpha / a, -2.0 * cs, 1.0 - alpha / a])
    raise ValueError(f"rbj_section: kind {kind!r}")


def synth_channel_sos(n: int, sample_rate: int = 16000, highpass_hz=(20, 400), lowpass_hz=(3000, 7800), peaks=(0, 2),
                      peak_hz=(200, 6000), peak_gain_db=(-12, 12), peak_q=(0.5, 4), seed: int = 0) -> Tuple[List[np.ndarray], np.ndarray]:
    """``synth_channels`` before the bank: the (S, 6) float64 cascade of every entry and the table of the draws."""
    ranges = dict(highpass_hz=highpass_hz, lowpass_hz=lowpass_hz, peak_hz=peak_hz, peak_q=peak_q)
    if n < 1 or sample_rate < 1:
        raise ValueError(f"synth_channels: n = {n}, sample_rate = {sample_rate}")
    for name, (lo, hi) in ranges.items():
        if not (math.isfinite(lo) and math.isfinite(hi) and 0.0 < lo <= hi):
            raise ValueError(f"synth_channels: {name} = {(lo, hi)} must be positive, finite and ordered")
        if name.endswith("_hz") and hi >= sample_rate / 2.0:
            raise ValueError(f"synth_channels: {name} = {(lo, hi)} must lie below half the sample rate")
    (g_lo, g_hi), (p_lo, p_hi) = peak_gain_db, peaks
    if not (math.isfinite(g_lo) and math.isfinite(g_hi) and g_lo <= g_hi):
        raise ValueError(f"synth_channels: peak_gain_db = {(g_lo, g_hi)} must be finite and ordered")
    if not 0 <= int(p_lo) <= int(p_hi) <= MAX_SECTIONS - 2:
        raise ValueError(f"synth_channels: peaks = {(p_lo, p_hi)} must lie in 0..{MAX_SECTIONS - 2} and be ordered")
    rng = np.random.Generator(np.random.Philox(int(seed)))
    log_uniform = lambda lo, hi: float(math.exp(rng.uniform(math.log(lo), math.log(hi))))     # noqa: E731
    butter_q = 1.0 / math.sqrt(2.0)
    cascades, table = [], np.full((n, 3 + 3 * int(p_hi)), np.nan, dtype=np.float64)
    for r in range(n):
        hp, lp = log_uniform(*highpass_hz), log_uniform(*lowpass_hz)
        k = int(rng.integers(int(p_lo), int(p_hi) + 1))
        rows = [rbj_section("highpass", hp, sample_rate, butter_q), rbj_section("lowpass", lp, sample_rate, butter_q)]
        table[r, :3] = (hp, lp, k)
        for j in range(k):
            f0, gain, q = log_uniform(*peak_hz), float(rng.uniform(g_lo, g_hi)), float(rng.uniform(*peak_q))
            rows.append(rbj_section("peak", f0, sample_rate, q, gain))
            table[r, 3 + 3 * j:6 + 3 * j] = (f0, gain, q)
        cascades.append(np.stack(rows))
    return cascades, table


def synth_channels(n: int, sample_rate: int = 16000, highpass_hz=(20, 400), lowpass_hz=(3000, 7800), peaks=(0, 2),
                   peak_hz=(200, 6000), peak_gain_db=(-12, 12), peak_q=(0.5, 4), seed: int = 0) -> Tuple[ChannelBank, np.ndarray]:
    """``n`` synthetic microphones and the float64 table of what was drawn for each: ``(highpass_hz, lowpass_hz, n_peaks,
    then per peak f0, gain_db, q)``, NaN where an entry has fewer peaks than ``peaks[1]``.

    The draws come from ``numpy.random.Generator(numpy.random.Philox(seed))``, entry by entry in this order: the
    high-pass corner and the low-pass corner, log-uniform; ``integers(peaks[0], peaks[1] + 1)`` peaks; per peak its
    centre (log-uniform), its gain in dB (uniform) and its Q (uniform).  Every section is the RBJ cookbook's, evaluated
    in float64 on the host: a high-pass and a low-pass with the Butterworth Q ``1 / sqrt(2)`` -- 12 dB per octave each,
    3 dB down at the corner -- and ``peakingEQ`` sections.  The default ranges are a design choice (a small electret
    capsule's low cut, an anti-aliasing roll-off below Nyquist, a few mild resonances); nothing was tuned on measured
    microphones."""
    cascades, table = synth_channel_sos(n, sample_rate, highpass_hz, lowpass_hz, peaks, peak_hz, peak_gain_db, peak_q, seed)
    return ChannelBank(cascades), table


# ------------------------------------------------------------------------------------------------ the C ABI
def bank_bytes(n_bank: int) -> int:
    """``cough_channel_bank_bytes``: the blob of a prepared bank."""
    got = int(_lib.load_channel().cough_channel_bank_bytes(int(n_bank)))
    if got == 0:
        raise ValueError(f"bank_bytes: n_bank = {n_bank}")
    return got


def prepare(sos: np.ndarray, n_sections: np.ndarray, blob: torch.Tensor) -> None:
    """``cough_channel_prepare``: the packed scipy-layout rows ``sos`` (float64 (sum S, 6), host; entry r has
    ``n_sections[r]`` of them) into ``blob`` (uint8, on the device)."""
    dev = _on_gpu("prepare", blob=(blob, torch.uint8))
    sos = np.ascontiguousarray(sos, dtype=np.float64).reshape(-1, 6)
    n_sections = np.ascontiguousarray(n_sections, dtype=np.int32)
    if int(np.clip(n_sections, 0, None).sum()) > sos.shape[0]:
        raise ValueError(f"prepare: {sos.shape[0]} sections but the entries need {int(n_sections.sum())}")
    _lib.check_channel(_lib.load_channel().cough_channel_prepare(
        sos.ctypes.data_as(C.POINTER(C.c_double)), n_sections.ctypes.data_as(C.POINTER(C.c_int)), int(n_sections.size),
        blob.data_ptr(), blob.numel(), _stream(dev)), "cough_channel_prepare")


def plan_array(plans: Sequence[Tuple[int, float]], n_bank: Optional[int] = None) -> np.ndarray:
    """(B,) ``PLAN_DTYPE``: ``(filter, clip_ratio)`` per row in the layout of ``cough_channel_plan`` (``filter = -1``: no
    filter; a ratio outside ``[0, 1)`` or NaN: no clip).  With ``n_bank`` the plans are checked as the host must check
    them, before anything is launched: ``filter >= n_bank`` and ``filter < -1`` raise ValueError."""
    arr = np.zeros(len(plans), dtype=PLAN_DTYPE)
    wide = np.array([max(-2**31, min(2**31 - 1, int(f))) for f, _ in plans], dtype=np.int64)
    arr["clip_ratio"] = np.array([float(r) for _, r in plans], dtype=np.float64).astype(np.float32)
    bad = wide < -1
    if n_bank is not None:
        bad |= wide >= n_bank
    if bad.any():
        k = int(np.nonzero(bad)[0][0])
        raise ValueError(f"plan_array: row {k} has filter = {int(wide[k])}" + (f" (bank of {n_bank})" if n_bank is not None else ""))
    arr["filter"] = wide
    return arr


def check_plans(plans: np.ndarray, n_bank: int, who: str = "channel_rows") -> np.ndarray:
    """Host plans ((B,) ``PLAN_DTYPE``) against a bank: ``filter < -1`` and ``filter >= n_bank`` raise ValueError."""
    arr = np.asarray(plans)
    if arr.dtype != PLAN_DTYPE or arr.ndim != 1:
        raise ValueError(f"{who}: host plans must be a (B,) array of plan_array's dtype, got {arr.dtype} {arr.shape}")
    bad = (arr["filter"] < -1) | (arr["filter"] >= n_bank)
    if bad.any():
        k = int(np.nonzero(bad)[0][0])
        raise ValueError(f"{who}: row {k} has filter = {int(arr['filter'][k])} (bank of {n_bank})")
    return np.ascontiguousarray(arr)


def plans_to_device(plans: np.ndarray, dev: torch.device) -> torch.Tensor:
    """Host plans as the int32 (B, 2) device tensor ``channel_rows`` takes (the ratio's bits in the second word)."""
    return torch.from_numpy(np.ascontiguousarray(plans).view(np.int32).reshape(-1, 2).copy()).to(dev)


def channel_rows(packed: torch.Tensor, offsets: torch.Tensor, lengths: torch.Tensor, plans: Union[np.ndarray, torch.Tensor],
                 width: int, bank: Optional[ChannelBank], out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """B rows of the packed float32 buffer ``packed`` filtered and clipped in one launch: row b is the ``lengths[b]``
    (int32) samples at ``offsets[b]`` (int64), read in place.  ``plans``: per row a ``cough_channel_plan`` -- a host array
    (``plan_array``), which is checked against the bank before anything is launched and then uploaded, or an int32 (B, 2)
    tensor on the device (``draw_channel``), whose entries the kernel makes harmless instead (a filter the bank does not
    have filters nothing).  ``bank=None`` is a bank without entries: the ceiling alone.  Returns (B, width) float32: row b
    holds its first ``min(n, width)`` samples through its filter and its ceiling and ``+0.0`` behind.  ``out`` may be
    given, and may be ``packed`` itself when that is the dense (B, width) matrix with ``offsets[b] = b * width``."""
    dev = _on_gpu("channel_rows", packed=(packed, torch.float32), offsets=(offsets, torch.int64), lengths=(lengths, torch.int32))
    b, width, n_bank = lengths.numel(), int(width), 0 if bank is None else len(bank)
    if not 1 <= width <= MAX_LENGTH:
        raise ValueError(f"channel_rows: width = {width} must lie in 1..2^30")
    if not isinstance(plans, torch.Tensor):
        plans = plans_to_device(check_plans(plans, n_bank), dev)
    _on_gpu("channel_rows", packed=(packed, torch.float32), plans=(plans, torch.int32))
    if offsets.numel() != b or plans.numel() != 2 * b:
        raise ValueError(f"channel_rows: need {b} row offsets and {b} plans of 2 words")
    if out is None:
        out = torch.empty((b, width), dtype=torch.float32, device=dev)
    else:
        _on_gpu("channel_rows", packed=(packed, torch.float32), out=(out, torch.float32))
        if out.numel() != b * width:
            raise ValueError(f"channel_rows: out must hold {b} x {width} values")
    blob = bank.blob(dev) if n_bank else None
    _lib.check_channel(_lib.load_channel().cough_channel_rows(
        packed.data_ptr(), offsets.data_ptr(), lengths.data_ptr(), b, plans.data_ptr(), blob.data_ptr() if blob is not None else None,
        n_bank, out.data_ptr(), width, _stream(dev)), "cough_channel_rows")
    return out.view(b, width)


def draw_channel(seed: int, b: int, p_augment: float, bank: Union[ChannelBank, int, None], p_clip: float = 0.3,
                 clip_range: Tuple[float, float] = (0.25, 1.0), device=None) -> torch.Tensor:
    """The channel draws of a batch of ``b`` rows, on the device: int32 (B, 2) plans.  Row b's coin fires with
    probability ``p_augment``; it then draws a filter uniformly from the bank (as ``random.randrange``) and, with
    probability ``p_clip``, a clip ratio uniform in ``clip_range``; otherwise ``(-1, 1.0)``.  The same ``seed`` gives the
    same draws.  Nothing is read back."""
    dev = torch.device(device) if device is not None else cuda_device()
    n_bank = 0 if bank is None else bank if isinstance(bank, int) else len(bank)
    plans = torch.empty((int(b), 2), dtype=torch.int32, device=dev)
    _lib.check_channel(_lib.load_channel().cough_draw_channel(
        int(seed) & (2**64 - 1), int(b), float(p_augment), n_bank, float(p_clip), float(clip_range[0]), float(clip_range[1]),
        plans.data_ptr(), _stream(dev)), "cough_draw_channel")
    return plans


def check_clip(p_clip: float, clip_range: Tuple[float, float], who: str) -> Tuple[float, Tuple[float, float]]:
    """``p_clip`` in [0, 1] and a finite, ordered ``clip_range`` inside [0, 1] (a ratio of 1 does not clip)."""
    p, (lo, hi) = float(p_clip), (float(clip_range[0]), float(clip_range[1]))
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"{who}: p_clip = {p_clip} must lie in 0..1")
    if not (math.isfinite(lo) and math.isfinite(hi) and 0.0 <= lo <= hi <= 1.0):
        raise ValueError(f"{who}: clip_range = {tuple(clip_range)} must be ordered and lie in 0..1")
    return p, (lo, hi)


# ------------------------------------------------------------------------------------------------ the report
def channel_report(bank, preprocessor, batch: int = 256, headroom_db: float = 40.0) -> Dict[str, np.ndarray]:
    """The long-term average spectrum of a ``DeviceClipBank`` per label, as the featuriser sees it: ``{"labels":
    (n_labels,) int64, "mel_db": (n_labels, n_mels), "difference_db": (n_mels,)}`` -- per label the mean over its clips
    and frames of the log-mel rows in dB, and, for a bank of two labels, the second's minus the first's (NaN otherwise).
    Classes whose difference is a smooth curve of several dB differ by their recording channel, whatever else they
    differ by; ``synth_channels``' ranges should cover that curve.  Every clip is prepared as the loader prepares it
    (``cough_prepare_rows``: centre crop or zero pad, peak 1), so a constant offset between the classes is their crest
    factor, not their channel: read the curve's shape.  The mel rows are ``clamp((dB + 80) / 80, 0, 1)`` with 0 dB at a
    mel power of 1, which a full-scale clip exceeds in most bands, so the clips are featurised ``headroom_db`` below full
    scale; the 80 dB window then reaches from the loudest cell down, and the rows are read back as ``80 row - 80``.  Torch
    ops on the featuriser's output only, one host read."""
    if not (0.0 <= float(headroom_db) <= 80.0):
        raise ValueError(f"channel_report: headroom_db = {headroom_db} must lie in 0..80")
    dev, n_mels, scale = bank.device, int(preprocessor.n_mels), 10.0 ** (-float(headroom_db) / 20.0)
    labels = bank.labels_dev
    kinds = torch.unique(labels)
    onehot = (labels.reshape(-1, 1) == kinds.reshape(1, -1)).to(torch.float64)           # (n, n_labels)
    sums = torch.zeros((kinds.numel(), n_mels), dtype=torch.float64, device=dev)
    for at in range(0, len(bank), int(batch)):
        rows = slice(at, min(at + int(batch), len(bank)))
        b = rows.stop - rows.start
        seg = torch.empty((b, preprocessor.segment_samples), dtype=torch.float32, device=dev)
        _lib.check_data(_lib.load_data().cough_prepare_rows(
            bank.data.data_ptr(), bank.offsets_dev[rows].contiguous().data_ptr(), bank.lengths_dev[rows].contiguous().data_ptr(), b,
            seg.data_ptr(), preprocessor.segment_samples, _lib.PREP_NORMALIZE, _stream(dev)), "cough_prepare_rows")
        feats = preprocessor.featurize_batch(seg * scale, normalize=False)               # (b, F, T); rows 0 .. n_mels-1 are the mel rows
        mel_db = (80.0 * feats[:, :n_mels, :].to(torch.float64) - 80.0).mean(dim=2)      # (b, n_mels)
        sums += onehot[rows].t() @ mel_db
    mean = sums / onehot.sum(dim=0).reshape(-1, 1)
    host = torch.cat([mean, kinds.to(torch.float64).reshape(-1, 1)], dim=1).cpu().numpy()       # the one host read
    mel_db = host[:, :n_mels]
    return {"labels": host[:, n_mels].astype(np.int64), "mel_db": mel_db,
            "difference_db": mel_db[1] - mel_db[0] if mel_db.shape[0] == 2 else np.full(n_mels, np.nan)}
