"""``channel_report`` on a synthetic bank whose class 1 went through a fixed low-pass with ``channel_rows``: the difference
of the two long-term average mel spectra must show the cascade's roll-off.

THE TOLERANCE.  The reference project's featuriser restated on the CPU (oracle/featurizer.py: ``normalize``, the clip
40 dB below full scale, ``extract_mel_spectrogram``, ``80 row - 80`` averaged over frames and clips) on these very clips
-- class 1 filtered with ``scipy.signal.sosfilt`` -- gives a difference that, once its mean deviation over the bands
below 500 Hz (the passband; the offset is the peak normalisation's) is taken off, stays within 0.358 dB of the cascade's
``sosfreqz`` magnitude at the 64 mel centres (100 Hz .. 4 kHz, down to -27 dB), and is strictly decreasing above the
cutoff.  What is left is the noise of 16 one-second clips per class and the width of the mel filters.  The device's
features agree with that restatement to 1e-5 of a row's unit, 1e-3 dB, so the test allows 0.5 dB.
"""
import numpy as np
import pytest
import torch
from scipy import signal

import cough_detector_amd as cda
from cough_detector_amd import channel as cch

pytestmark = pytest.mark.gpu
SHIPPED = dict(use_pcen=False, use_pre_emphasis=False, use_delta_delta=False, use_spectral_contrast=False)
TOLERANCE_DB, CUTOFF = 0.5, 1000.0


def test_the_report_shows_a_low_pass_between_the_classes():
    rng = np.random.default_rng(0)
    sos = signal.butter(2, CUTOFF / 8000.0, output="sos")
    clips = [(0.1 * rng.standard_normal(16000)).astype(np.float32) for _ in range(32)]
    wet_src = torch.from_numpy(np.concatenate(clips[16:])).cuda()
    offs = (torch.arange(16, dtype=torch.int64) * 16000).cuda()
    lens = torch.full((16,), 16000, dtype=torch.int32).cuda()
    wet = cda.channel_rows(wet_src, offs, lens, cch.plan_array([(0, 1.0)] * 16, 1), 16000, cda.ChannelBank.from_sos([sos]))
    bank = cda.DeviceClipBank([torch.from_numpy(x) for x in clips[:16]] + [row.cpu() for row in wet], [0] * 16 + [1] * 16)
    pre = cda.AudioPreprocessor(device="cuda", **SHIPPED)
    report = cda.channel.channel_report(bank, pre, batch=10)                # ragged batches: 10, 10, 10, 2
    assert report["labels"].tolist() == [0, 1] and report["mel_db"].shape == (2, 64) and report["difference_db"].shape == (64,)
    assert np.isfinite(report["mel_db"]).all() and (report["mel_db"] > -79).all() and (report["mel_db"] < -1).all()    # off both clamps
    mel = lambda f: 2595.0 * np.log10(1.0 + f / 700.0)                      # noqa: E731
    centres = 700.0 * (10.0 ** (np.linspace(mel(pre.f_min), mel(pre.f_max), 66)[1:-1] / 2595.0) - 1.0)
    _, h = signal.sosfreqz(sos, worN=centres, fs=16000)
    want = 20.0 * np.log10(np.abs(h))
    d = report["difference_db"]
    dev = d - np.mean((d - want)[centres < 500.0]) - want
    print(f"largest deviation from sosfreqz at the mel centres: {np.abs(dev).max():.3f} dB (the CPU restatement: 0.358); deepest band {want.min():.1f} dB")
    assert np.abs(dev).max() <= TOLERANCE_DB
    assert (np.diff(d[centres > CUTOFF]) < 0).all() and (centres > CUTOFF).sum() >= 30
    # one label only: no difference to report; the same call twice: the same figures
    one = cda.channel.channel_report(cda.DeviceClipBank([torch.from_numpy(x) for x in clips[:3]], [1, 1, 1]), pre)
    assert one["labels"].tolist() == [1] and np.isnan(one["difference_db"]).all()
    again = cda.channel.channel_report(bank, pre, batch=10)
    assert again["mel_db"].tobytes() == report["mel_db"].tobytes()
    with pytest.raises(ValueError):
        cda.channel.channel_report(bank, pre, headroom_db=-1.0)
