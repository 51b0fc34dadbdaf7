"""Where every step of the waveform chain sits in a batch's native calls, the capture channel included.

``tests/test_gpu_chain.py`` pins the order for the speed and the pitch step.  This file does it for all four optional
steps (speed, pitch, reverb, channel), with the recording proxy in every library's handle -- ``_lib.LIBRARIES``,
``_lib.LATER`` and ``_lib.OPEN`` -- so the reverb's and the channel's entry points are seen too.  Public entry points
only.  The expected sequences are literals, never produced by the code under test.  The last test records one
``augment_batch`` link by link (``chain_trace.recording(channel=True)``): the channel step reads, bit for bit, what the
augmentation kernel wrote, and what it writes is what the caller gets.
"""
import contextlib
import random

import numpy as np
import pytest
import torch

import cough_detector_amd as cda
from cough_detector_amd import _lib
from cough_detector_amd import warp as cwarp
from cough_detector_amd.data import BatchPlan
from chain_trace import recording

pytestmark = pytest.mark.gpu
SHIPPED = dict(use_pcen=False, use_pre_emphasis=False, use_delta_delta=False, use_spectral_contrast=False)
LENGTHS = [1, 2, 257, 700, 4097, 9000]
SHIFTS = [0, 0, -40, 100, -700, 1500]
INDICES = [0, 1, 2, 3, 4, 5]
_SKIPPED = ("_abi_version", "_last_error", "_workspace_bytes", "_bank_bytes")


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
    """The ordered names of the native entry points called, through any library, while the block runs."""
    log, real = [], {}
    tables = (_lib.LIBRARIES, _lib.LATER, _lib.OPEN)
    for table in tables:
        for name, library in table.items():
            real[name] = library.load()
            library.handle = _Recording(real[name], log)
    try:
        yield log
    finally:
        for table in tables:
            for name, library in table.items():
                library.handle = real[name]


@pytest.fixture(scope="module")
def setup():
    g = torch.Generator().manual_seed(23)
    bank = cda.DeviceClipBank([(torch.rand(n, generator=g) - 0.5) * 0.8 for n in LENGTHS], [0, 1, 0, 0, 1, 0])
    pre = cda.AudioPreprocessor(device="cuda", **SHIPPED)
    pre.featurize_batch(torch.zeros((1, pre.segment_samples), device="cuda"), normalize=False)   # the handle exists
    rirs, mics = cda.synth_rirs(3, seed=3)[0], cda.synth_channels(3, seed=3)[0]
    rirs.workspace(bank.device)                          # both banks are prepared here: no *_prepare call lands in a log
    mics.blob(bank.device)
    return bank, pre, rirs, mics


def _augmentor(setup, speed=True, pitch=True, reverb=True, channel=True, p=0.5):
    _, _, rirs, mics = setup
    g = torch.Generator().manual_seed(11)
    aug = cda.AudioAugmentor(p_augment=p, speed=speed, pitch=pitch, reverb=rirs if reverb else None,
                             channel=mics if channel else None)
    aug.noise_samples = [torch.randn((1, n), generator=g) * 0.3 for n in (700, 9000)]
    aug._pack_bank()
    return aug


def _loader(setup, aug, draws="host"):
    bank, pre = setup[:2]
    return cda.DeviceDataLoader(bank, pre, batch_size=6, audio_augmentor=aug, spec_augmentor=cda.SpecAugment(p=1.0),
                                mixup=cda.MixUp(0.4), draws=draws, generator=torch.Generator().manual_seed(1))


NONE = [None] * 6
PAIRS = [None, None, (15000, 16000), None, (17000, 16000), None]
STEPS = [None, None, None, 2, None, -1]
RIRS = [None, 0, None, 2, 1, None]
MICS = [(0, 1.0), None, (2, 0.5), None, None, (1, 0.3)]
HOST_CASES = {"nothing": (NONE, NONE, NONE, NONE), "channel": (NONE, NONE, NONE, MICS), "reverb": (NONE, NONE, RIRS, NONE),
              "all four": (PAIRS, STEPS, RIRS, MICS)}


def _plan(pairs, steps, rirs, mics):
    new = [n if p is None else cwarp.warped_length(n, *p) for n, p in zip(LENGTHS, pairs)]
    clips = [_lib.CoughAugClip(shift=SHIFTS[i], gain=0.8 + 0.1 * i, gaussian=1, bank_index=i % 2, gaussian_snr_db=20.0,
                               bank_snr_db=10.0, bank_start=0) for i in INDICES]
    masks = [[(0, 3 + i, 9 + i), (0, 40, 41), (1, 5 * i, 5 * i + 12), (1, 90, 95)] for i in INDICES]
    return BatchPlan(clips=clips, seed=5, masks=masks, perm=torch.tensor([3, 0, 5, 1, 2, 4]),
                     lam=np.array([0.9, 0.5, 0.25, 1.0, 0.0, 0.7]), pairs=list(pairs), new_lengths=new, steps=list(steps),
                     rirs=list(rirs), channels=list(mics))


_TAIL = ["cough_prepare_rows", "cough_featurize_any", "cough_mask_images", "cough_mix_batch"]
EXPECTED_HOST = {
    "nothing": ["cough_gather_rows", "cough_augment_waveforms"] + _TAIL,
    "channel": ["cough_gather_rows", "cough_augment_waveforms", "cough_channel_rows"] + _TAIL,
    "reverb": ["cough_reverb_rows", "cough_augment_waveforms"] + _TAIL,
    "all four": ["cough_warp_rows", "cough_stretch_rows", "cough_warp_rows", "cough_reverb_rows", "cough_augment_waveforms",
                 "cough_channel_rows"] + _TAIL,
}
# (speed, pitch, reverb, channel) -> the calls in front of the tail
EXPECTED_DEVICE = {
    (False, False, False, False): ["cough_draw_batch", "cough_augment_rows_drawn"],
    (False, False, False, True): ["cough_draw_batch", "cough_augment_rows_drawn", "cough_draw_channel", "cough_channel_rows"],
    (False, False, True, False): ["cough_draw_reverb", "cough_draw_batch", "cough_clear_shifts", "cough_reverb_rows",
                                  "cough_augment_rows_drawn"],
    (False, False, True, True): ["cough_draw_reverb", "cough_draw_batch", "cough_clear_shifts", "cough_reverb_rows",
                                 "cough_augment_rows_drawn", "cough_draw_channel", "cough_channel_rows"],
    (False, True, False, False): ["cough_draw_pitch", "cough_draw_batch", "cough_clear_shifts", "cough_stretch_rows",
                                  "cough_warp_rows", "cough_augment_rows_drawn"],
    (False, True, False, True): ["cough_draw_pitch", "cough_draw_batch", "cough_clear_shifts", "cough_stretch_rows",
                                 "cough_warp_rows", "cough_augment_rows_drawn", "cough_draw_channel", "cough_channel_rows"],
    (False, True, True, False): ["cough_draw_pitch", "cough_draw_reverb", "cough_draw_batch", "cough_clear_shifts",
                                 "cough_stretch_rows", "cough_warp_rows", "cough_reverb_rows", "cough_augment_rows_drawn"],
    (False, True, True, True): ["cough_draw_pitch", "cough_draw_reverb", "cough_draw_batch", "cough_clear_shifts",
                                "cough_stretch_rows", "cough_warp_rows", "cough_reverb_rows", "cough_augment_rows_drawn",
                                "cough_draw_channel", "cough_channel_rows"],
    (True, False, False, False): ["cough_draw_speed", "cough_draw_batch", "cough_warp_rows", "cough_clear_shifts",
                                  "cough_augment_rows_drawn"],
    (True, False, False, True): ["cough_draw_speed", "cough_draw_batch", "cough_warp_rows", "cough_clear_shifts",
                                 "cough_augment_rows_drawn", "cough_draw_channel", "cough_channel_rows"],
    (True, False, True, False): ["cough_draw_speed", "cough_draw_reverb", "cough_draw_batch", "cough_warp_rows",
                                 "cough_clear_shifts", "cough_reverb_rows", "cough_augment_rows_drawn"],
    (True, False, True, True): ["cough_draw_speed", "cough_draw_reverb", "cough_draw_batch", "cough_warp_rows",
                                "cough_clear_shifts", "cough_reverb_rows", "cough_augment_rows_drawn", "cough_draw_channel",
                                "cough_channel_rows"],
    (True, True, False, False): ["cough_draw_speed", "cough_draw_pitch", "cough_draw_batch", "cough_warp_rows",
                                 "cough_clear_shifts", "cough_stretch_rows", "cough_warp_rows", "cough_augment_rows_drawn"],
    (True, True, False, True): ["cough_draw_speed", "cough_draw_pitch", "cough_draw_batch", "cough_warp_rows",
                                "cough_clear_shifts", "cough_stretch_rows", "cough_warp_rows", "cough_augment_rows_drawn",
                                "cough_draw_channel", "cough_channel_rows"],
    (True, True, True, False): ["cough_draw_speed", "cough_draw_pitch", "cough_draw_reverb", "cough_draw_batch",
                                "cough_warp_rows", "cough_clear_shifts", "cough_stretch_rows", "cough_warp_rows",
                                "cough_reverb_rows", "cough_augment_rows_drawn"],
    (True, True, True, True): ["cough_draw_speed", "cough_draw_pitch", "cough_draw_reverb", "cough_draw_batch",
                               "cough_warp_rows", "cough_clear_shifts", "cough_stretch_rows", "cough_warp_rows",
                               "cough_reverb_rows", "cough_augment_rows_drawn", "cough_draw_channel", "cough_channel_rows"],
}


@pytest.mark.parametrize("case", list(HOST_CASES))
def test_launch_batch_calls_every_step_in_its_place(setup, case):
    loader = _loader(setup, _augmentor(setup))
    plan = _plan(*HOST_CASES[case])
    with recorded() as log:
        feats, soft = loader.launch_batch(INDICES, plan)
    assert tuple(feats.shape) == (6, 1, 90, 101) and tuple(soft.shape) == (6, 2)
    assert log == EXPECTED_HOST[case]


@pytest.mark.parametrize("on", list(EXPECTED_DEVICE), ids=["".join(str(int(v)) for v in on) for on in EXPECTED_DEVICE])
def test_launch_batch_drawn_calls_every_step_in_its_place(setup, on):
    loader = _loader(setup, _augmentor(setup, *on), draws="device")
    with recorded() as log:
        feats, soft = loader.launch_batch_drawn(INDICES, 12345)
    assert tuple(feats.shape) == (6, 1, 90, 101) and tuple(soft.shape) == (6, 2)
    assert log == EXPECTED_DEVICE[on] + _TAIL


def test_the_channel_link_reads_what_the_kernel_wrote(setup):
    bank = setup[0]
    aug = _augmentor(setup, p=1.0)
    x = torch.zeros((6, max(LENGTHS)), device=bank.device)
    for r in INDICES:
        x[r, :LENGTHS[r]] = bank.clip(r)[0]
    random.seed(41)
    with recording(channel=True) as trace:
        out, lens = aug.augment_batch(x, lengths=LENGTHS, noise="device", seed=9, return_lengths=True)
    torch.cuda.synchronize()
    assert [link["kind"] for link in trace] == ["warp", "stretch", "back", "reverb", "augment", "channel"]
    assert trace[0]["shift"].any() and not any(link["shift"].any() for link in trace[1:])
    kernel, mic = trace[-2], trace[-1]
    assert mic["lengths"].tolist() == lens.tolist() and all(f >= 0 for f, _ in mic["param"])
    for r, n in enumerate(lens.tolist()):
        assert mic["rows"][r].size == n and (mic["rows"][r].view(np.uint32) == kernel["out"][r, :n].view(np.uint32)).all(), r
    assert tuple(out.shape) == mic["out"].shape and (out.cpu().numpy().view(np.uint32) == mic["out"].view(np.uint32)).all()
    assert not (mic["out"] == kernel["out"]).all()       # the step did something
