"""The fused stem's feature image at its first and last columns: frame 0 lands in the odd image column 3 (beside the border
column 2) and frame 100 in column 103, the last one written.  Clips whose energy sits in the first or the last 100 samples put
their signal into exactly these columns; the pipeline's logits (image built in LDS, stem fused) must be bit-equal to the
classifier run on the materialised features."""
import numpy as np
import pytest
import torch

import cough_detector_amd as cda
from parity import SHIPPED, synth_batch

pytestmark = pytest.mark.gpu


def edge_energy_clips() -> torch.Tensor:
    rng = np.random.default_rng(404)
    w = np.zeros((8, 16000), dtype=np.float32)
    burst = lambda: rng.uniform(-0.5, 0.5, size=100).astype(np.float32)
    for i in range(8):
        if i % 3 != 1:
            w[i, :100] = burst()          # first 100 samples: frames 0 and 1
        if i % 3 != 0:
            w[i, -100:] = burst()         # last 100 samples: frames 99 and 100
    w[6, :100] *= 1e-3                    # a quiet start beside a loud end, and the other way round
    w[7, -100:] *= 1e-3
    return torch.cat([torch.from_numpy(w), synth_batch(820, 2, peak_normalize=False) * 0.4])


@pytest.mark.parametrize("normalize", [False, True])
def test_pipeline_is_bit_equal_to_two_steps_on_the_edge_columns(resnet_golden, normalize):
    sd, _ = resnet_golden
    w = edge_energy_clips().cuda()
    pre = cda.AudioPreprocessor(device="cuda", **SHIPPED)
    model = cda.create_model("residual", n_mels=90, num_classes=2, in_channels=1, compute_dtype="bf16x3")
    model.load_state_dict(sd)
    model.cuda()
    feats = pre.featurize_batch(w, normalize=normalize)
    assert torch.isfinite(feats).all()
    # the signal is where the test says it is: the edge clips' mel rows peak in the first or last frames
    mel = feats[:8, :64].amax(dim=1)                                     # (8, 101): loudest band per frame
    assert all(int(mel[i].argmax()) in (0, 1, 2, 98, 99, 100) for i in range(8))
    want = model(feats.unsqueeze(1))
    got = cda.CoughPipeline(pre, model)(w, normalize=normalize)
    assert torch.isfinite(got).all() and torch.equal(got, want)
    assert float((want[:, 1] - want[:, 0]).std()) > 0                    # the clips do not all score alike
