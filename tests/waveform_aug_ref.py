"""CPU restatement of the reference's waveform augmentation and MixUp (TEST INFRASTRUCTURE, not product).

Follows ``/root/reference/src/augmentation.py`` -- ``AudioAugmentor`` (:19-268) and ``MixUp`` (:334-369) -- with torch
ops on the CPU, in the reference's order of random draws: Python ``random`` for every coin and uniform, the CPU torch
generator for ``randn_like``.  The reference module imports torchaudio at the top and so cannot be executed here; the
noise bank is passed in as a list of (1, L) tensors instead of being loaded by torchaudio.

Every draw is appended to ``log`` as ``(step, values...)`` so a test can compare the host draw sequence of the product.
"""
from __future__ import annotations

import random
from typing import List, Optional, Tuple

import numpy as np
import torch


class AudioAugmentorRef:
    def __init__(self, p_augment: float = 0.5, noise_samples: Optional[List[torch.Tensor]] = None):
        self.p_augment = p_augment
        self.noise_samples = list(noise_samples or [])
        self.log: List[tuple] = []

    def time_shift(self, waveform: torch.Tensor, shift_limit: float = 0.2) -> torch.Tensor:
        """:77-105 -- s = int(N * uniform(-limit, limit)); right: zeros on the left, left: zeros on the right."""
        if random.random() > self.p_augment:
            return waveform
        s = int(waveform.shape[1] * random.uniform(-shift_limit, shift_limit))
        if s != 0:
            self.log.append(("shift", s))
        if s > 0:
            waveform = torch.nn.functional.pad(waveform, (s, 0))[:, :-s]
        elif s < 0:
            waveform = torch.nn.functional.pad(waveform, (0, -s))[:, -s:]
        return waveform

    def speed_perturbation(self, waveform: torch.Tensor) -> torch.Tensor:
        """:107-117 -- the identity."""
        return waveform

    def add_noise(self, waveform: torch.Tensor, snr_range: Tuple[float, float] = (5, 20)) -> torch.Tensor:
        """:119-163 -- choice, repeat to (N // L + 1) * L when shorter, randint crop start, SNR; skipped on a silent crop."""
        if random.random() > self.p_augment or len(self.noise_samples) == 0:
            return waveform
        k = random.choice(range(len(self.noise_samples)))     # the same draw as random.choice(noise_samples)
        noise = self.noise_samples[k].clone()
        n = waveform.shape[1]
        if noise.shape[1] < n:
            noise = noise.repeat(1, n // noise.shape[1] + 1)
        start = random.randint(0, noise.shape[1] - n)
        noise = noise[:, start:start + n]
        snr_db = random.uniform(*snr_range)
        self.log.append(("bank", k, start, snr_db))
        signal_power = waveform.pow(2).mean()
        noise_power = noise.pow(2).mean()
        if noise_power > 0:
            scale = torch.sqrt(signal_power / (10 ** (snr_db / 10) * noise_power))
            waveform = waveform + scale * noise
        return waveform

    def add_gaussian_noise(self, waveform: torch.Tensor, snr_range: Tuple[float, float] = (10, 30)) -> torch.Tensor:
        """:165-192 -- Pz is the power of the noise actually drawn."""
        if random.random() > self.p_augment:
            return waveform
        snr_db = random.uniform(*snr_range)
        self.log.append(("gauss", snr_db))
        signal_power = waveform.pow(2).mean()
        noise = torch.randn_like(waveform)
        noise_power = noise.pow(2).mean()
        scale = torch.sqrt(signal_power / (10 ** (snr_db / 10) * noise_power))
        return waveform + scale * noise

    def volume_perturbation(self, waveform: torch.Tensor, gain_range: Tuple[float, float] = (0.7, 1.3)) -> torch.Tensor:
        """:194-213"""
        if random.random() > self.p_augment:
            return waveform
        gain = random.uniform(*gain_range)
        self.log.append(("gain", gain))
        return waveform * gain

    def pitch_shift(self, waveform: torch.Tensor, shift_range: Tuple[int, int] = (-2, 2)) -> torch.Tensor:
        """:215-247 without sox: coin, semitones, the input unchanged."""
        if random.random() > self.p_augment:
            return waveform
        random.randint(*shift_range)
        return waveform

    def augment(self, waveform: torch.Tensor) -> torch.Tensor:
        """:249-268"""
        waveform = self.time_shift(waveform)
        waveform = self.speed_perturbation(waveform)
        waveform = self.volume_perturbation(waveform)
        waveform = self.add_gaussian_noise(waveform)
        if len(self.noise_samples) > 0:
            waveform = self.add_noise(waveform)
        return waveform


def clip_log(c) -> List[tuple]:
    """The draws one product ``CoughAugClip`` records, in the restatement's ``log`` form."""
    out = []
    if c.shift != 0:
        out.append(("shift", c.shift))
    if c.gain != 1.0:
        out.append(("gain", c.gain))
    if c.gaussian:
        out.append(("gauss", c.gaussian_snr_db))
    if c.bank_index >= 0:
        out.append(("bank", c.bank_index, c.bank_start, c.bank_snr_db))
    return out


def mixup(x1, y1, x2, y2, alpha: float = 0.2):
    """:353-369 -- one lam = np.random.beta(alpha, alpha)."""
    lam = np.random.beta(alpha, alpha)
    return lam * x1 + (1 - lam) * x2, lam * y1 + (1 - lam) * y2
