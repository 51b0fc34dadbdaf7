"""The fused normalise takes the clip's peak from each sample once: frame 0 scans every sample it loads, every later frame only
the samples that are new to it.  A spike that no frame scans leaves the peak at the noise level, 40 dB below the truth, which
shifts every dB value of the clip -- so one spike at each edge of the frames' "new samples" ranges and of the reflected zones,
checked against the CPU oracle, shows that the union of the ranges is the whole clip."""
import numpy as np
import pytest
import torch

import cough_detector_amd as cda
from oracle import featurizer as ofeat
from parity import FEAT_TOL, SHIPPED, feature_errors

pytestmark = pytest.mark.gpu

# first / last sample, the ends of the reflected zone of the first frames, the edges of a frame's new-sample range (a hop of 160:
# 40, 200, 360 and their neighbours), the middle of the clip, the last frames' ranges and the reflected zone at the clip's end
SPIKES = (0, 1, 39, 40, 199, 200, 201, 359, 360, 7999, 8039, 8040, 15839, 15840, 15998, 15999)
NEGATIVE = (0, 223, 224, 15999)   # further clips whose spike is -1.0: the peak is of |x|


@pytest.fixture(scope="module")
def clips():
    rng = np.random.default_rng(91)
    w = rng.uniform(-0.01, 0.01, size=(len(SPIKES) + len(NEGATIVE), 16000)).astype(np.float32)
    for i, s in enumerate(SPIKES):
        w[i, s] = 1.0
    for i, s in enumerate(NEGATIVE):
        w[len(SPIKES) + i, s] = -1.0
    return torch.from_numpy(w)


@pytest.mark.parametrize("pre_emphasis", [False, True], ids=["plain", "pre_emphasis"])
def test_a_spike_anywhere_in_the_clip_sets_the_peak(clips, pre_emphasis):
    flags = {**SHIPPED, "use_pre_emphasis": pre_emphasis}
    pre = cda.AudioPreprocessor(device="cuda", **flags)
    got = pre.featurize_batch(clips.cuda(), normalize=True).cpu()
    ref = ofeat.extract_features_batch(clips, normalize_first=True, use_pre_emphasis=pre_emphasis)
    assert torch.isfinite(got).all()
    for i, s in enumerate(SPIKES + NEGATIVE):
        mel, rel = feature_errors(got[i], ref[i])
        print(f"spike at {s:5d}: mel abs {mel:.2e}, mfcc/delta rel {rel:.2e}")
        assert mel < FEAT_TOL and rel < FEAT_TOL, s
    # the peak is found wherever the spike sits: scaling the clip leaves the peak-normalised features where they are
    scaled = pre.featurize_batch((clips * 0.25).cuda(), normalize=True).cpu()
    mel, rel = feature_errors(scaled, got)
    assert mel < FEAT_TOL and rel < FEAT_TOL


@pytest.mark.parametrize("pre_emphasis", [False, True], ids=["plain", "pre_emphasis"])
def test_silence_and_a_nan_in_the_last_sample(clips, pre_emphasis):
    flags = {**SHIPPED, "use_pre_emphasis": pre_emphasis}
    pre = cda.AudioPreprocessor(device="cuda", **flags)
    w = clips[:3].clone()
    w[0] = 0.0                       # digital silence: normalize is a silent no-op
    w[1, 15999] = float("nan")       # seen by the last two frames only, through the reflection too
    got = pre.featurize_batch(w.cuda(), normalize=True).cpu()
    ref = ofeat.extract_features_batch(w, normalize_first=True, use_pre_emphasis=pre_emphasis)
    assert torch.isnan(ref[1]).all() and torch.isnan(got[1]).all()
    assert torch.all(got[0, :64] == 0)
    for i in (0, 2):                 # the NaN clip leaves its neighbours alone
        mel, rel = feature_errors(got[i], ref[i])
        assert mel < FEAT_TOL and rel < FEAT_TOL, i
