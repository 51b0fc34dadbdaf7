"""The native entry points one batch of the loader calls, in order, for every way the waveform chain can run.

A thin proxy sits in each ``_lib.LIBRARIES[name].handle`` while one ``launch_batch`` or ``launch_batch_drawn`` runs and
writes down the name of every entry point called through it (version, last-error and workspace-size queries aside).  The
expected sequences are literals, never produced by the code under test: they pin which launches a batch makes and in
which order, and that a launch with nothing to do (no pair fired, no semitones fired, semitones of 0) is
skipped.  The last test compares a batch of one with its row of the batch of six, bit for bit.
"""
import contextlib

import numpy as np
import pytest
import torch

import cough_detector_amd as cda
from cough_detector_amd import _lib
from cough_detector_amd import warp as cwarp
from cough_detector_amd.data import BatchPlan

pytestmark = pytest.mark.gpu
SHIPPED = dict(use_pcen=False, use_pre_emphasis=False, use_delta_delta=False, use_spectral_contrast=False)
LENGTHS = [1, 2, 257, 700, 4097, 9000]
SHIFTS = [0, 0, -40, 100, -700, 1500]
INDICES = [0, 1, 2, 3, 4, 5]
_SKIPPED = ("_abi_version", "_last_error", "_workspace_bytes")


class _Recording:
    def __init__(self, real, log):
        self._real, self._log = real, log

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if any(s in name for s in _SKIPPED):
            return fn

        def call(*args):
            self._log.append(name)
            return fn(*args)
        return call


@contextlib.contextmanager
def recorded():
    """The ordered names of the native entry points called while the block runs."""
    log, real = [], {}
    for name, library in _lib.LIBRARIES.items():
        real[name] = library.load()
        library.handle = _Recording(real[name], log)
    try:
        yield log
    finally:
        for name, library in _lib.LIBRARIES.items():
            library.handle = real[name]


def _augmentor(speed=True, pitch=True, p=0.5):
    g = torch.Generator().manual_seed(11)
    aug = cda.AudioAugmentor(p_augment=p, speed=speed, pitch=pitch)
    aug.noise_samples = [torch.randn((1, n), generator=g) * 0.3 for n in (700, 9000)]
    aug._pack_bank()
    return aug


@pytest.fixture(scope="module")
def setup():
    g = torch.Generator().manual_seed(23)
    bank = cda.DeviceClipBank([(torch.rand(n, generator=g) - 0.5) * 0.8 for n in LENGTHS], [0, 1, 0, 0, 1, 0])
    pre = cda.AudioPreprocessor(device="cuda", **SHIPPED)
    pre.featurize_batch(torch.zeros((1, pre.segment_samples), device="cuda"), normalize=False)   # the handle exists
    return bank, pre


def _loader(setup, aug, draws="host"):
    bank, pre = setup
    return cda.DeviceDataLoader(bank, pre, batch_size=6, audio_augmentor=aug, spec_augmentor=cda.SpecAugment(p=1.0),
                                mixup=cda.MixUp(0.4), draws=draws, generator=torch.Generator().manual_seed(1))


PAIRS = [None, None, (15000, 16000), None, (17000, 16000), None]
STEPS = [None, None, None, 2, None, -1]
HOST_CASES = {"nothing": ([None] * 6, [None] * 6), "pairs": (PAIRS, [None] * 6), "steps": ([None] * 6, STEPS),
              "both": (PAIRS, STEPS), "zero steps": ([None] * 6, [None, None, None, 0, None, 0])}


def _plan(pairs, steps, rows=INDICES, mix=True, host_noise=False):
    new = [LENGTHS[i] if pairs[i] is None else cwarp.warped_length(LENGTHS[i], *pairs[i]) for i in rows]
    clips = [_lib.CoughAugClip(shift=SHIFTS[i], gain=0.8 + 0.1 * i, gaussian=1, bank_index=i % 2, gaussian_snr_db=20.0,
                               bank_snr_db=10.0, bank_start=0) for i in rows]
    masks = [[(0, 3 + i, 9 + i), (0, 40, 41), (1, 5 * i, 5 * i + 12), (1, 90, 95)] for i in rows]
    plan = BatchPlan(clips=clips, seed=5, masks=masks, pairs=[pairs[i] for i in rows], new_lengths=new,
                     steps=[steps[i] for i in rows])
    if mix:
        plan.perm, plan.lam = torch.tensor([3, 0, 5, 1, 2, 4]), np.array([0.9, 0.5, 0.25, 1.0, 0.0, 0.7])
    if host_noise:
        g = torch.Generator().manual_seed(77)
        noise = torch.randn((6, max(LENGTHS) + 1000), generator=g)
        plan.gaussian = noise[rows].contiguous()
    return plan


_TAIL = ["cough_prepare_rows", "cough_featurize_any", "cough_mask_images", "cough_mix_batch"]
_PITCH = ["cough_stretch_rows", "cough_warp_rows"]
EXPECTED_HOST = {
    "nothing": ["cough_gather_rows", "cough_augment_waveforms"] + _TAIL,
    "pairs": ["cough_warp_rows", "cough_augment_waveforms"] + _TAIL,
    "steps": _PITCH + ["cough_augment_waveforms"] + _TAIL,
    "both": ["cough_warp_rows"] + _PITCH + ["cough_augment_waveforms"] + _TAIL,
    "zero steps": ["cough_gather_rows", "cough_augment_waveforms"] + _TAIL,
}
EXPECTED_DEVICE = {
    (True, True): ["cough_draw_speed", "cough_draw_pitch", "cough_draw_batch", "cough_warp_rows", "cough_clear_shifts"]
                  + _PITCH + ["cough_augment_rows_drawn"] + _TAIL,
    (True, False): ["cough_draw_speed", "cough_draw_batch", "cough_warp_rows", "cough_clear_shifts",
                    "cough_augment_rows_drawn"] + _TAIL,
    (False, True): ["cough_draw_pitch", "cough_draw_batch", "cough_clear_shifts"] + _PITCH + ["cough_augment_rows_drawn"]
                   + _TAIL,
    (False, False): ["cough_draw_batch", "cough_augment_rows_drawn"] + _TAIL,
}


@pytest.mark.parametrize("case", list(HOST_CASES))
def test_launch_batch_calls_what_it_called(setup, case):
    loader = _loader(setup, _augmentor())
    plan = _plan(*HOST_CASES[case])
    with recorded() as log:
        feats, soft = loader.launch_batch(INDICES, plan)
    assert tuple(feats.shape) == (6, 1, 90, 101) and tuple(soft.shape) == (6, 2)
    assert log == EXPECTED_HOST[case]


@pytest.mark.parametrize("speed,pitch", [(True, True), (True, False), (False, True), (False, False)])
def test_launch_batch_drawn_calls_what_it_called(setup, speed, pitch):
    loader = _loader(setup, _augmentor(speed, pitch), draws="device")
    with recorded() as log:
        feats, soft = loader.launch_batch_drawn(INDICES, 12345)
    assert tuple(feats.shape) == (6, 1, 90, 101) and tuple(soft.shape) == (6, 2)
    assert log == EXPECTED_DEVICE[speed, pitch]


def test_a_batch_of_one_is_its_row_of_the_batch_of_six(setup):
    loader = _loader(setup, _augmentor())
    feats, targets = loader.launch_batch(INDICES, _plan(*HOST_CASES["both"], mix=False, host_noise=True))
    assert tuple(feats.shape) == (6, 1, 90, 101) and torch.isfinite(feats).all()
    for i in INDICES:
        f, t = loader.launch_batch([i], _plan(*HOST_CASES["both"], rows=[i], mix=False, host_noise=True))
        assert torch.equal(f[0], feats[i]) and torch.equal(t[0], targets[i]), i
