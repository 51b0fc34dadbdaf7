"""The fused split-bf16 stem against the stand-alone one, bit for bit, at the batch sizes where a layout mistake would show.

The fused stem keeps its bf16 images at a pitch of its own (112 bf16 for the shipped instantiations, 106 for the full-band ones)
and addresses a tile's fragments from one register per (plane, k-step pair).  None of that touches the arithmetic: same MFMA sequence, same k order, same max / bias / ReLU as ``stem_bf16_kernel``.  So

* the fused pipeline's logits equal featurise -> ``model(features)`` bit for bit, and
* the fused kernel's stem output ``a1`` equals the stand-alone stem's on the same features bit for bit -- including pooled
  positions 544..549, which come from the partial 69th tile; the clip with the NaN sample is the one exception, it leaves the
  kernel before the stem and its ``a1`` is never written --

for the shipped flags, pre-emphasis and delta-delta (the 103-row stem in two halves), at B = 1, 2 and 5, on random clips, an
all-zero clip, a clip with one NaN sample and a clip that is an impulse in its first and in its last frame.
"""
import pytest
import torch

import cough_detector_amd as cda
from cough_detector_amd import _lib
from cough_detector_amd._native import cuda_device
from parity import SHIPPED, synth_batch

pytestmark = pytest.mark.gpu

FLAGS = {"shipped": {}, "preemph": {"use_pre_emphasis": True}, "delta_delta": {"use_delta_delta": True}}
RANDOM0, ZERO, NAN, IMPULSE, RANDOM1 = range(5)


@pytest.fixture(scope="module")
def clips():
    w = synth_batch(4100, 5, peak_normalize=False) * 0.5
    w[ZERO] = 0.0
    w[NAN, 7777] = float("nan")
    w[IMPULSE] = 0.0
    w[IMPULSE, 0] = 0.8            # frame 0 ...
    w[IMPULSE, 15999] = -0.6       # ... and frame 100
    return w


@pytest.fixture(scope="module")
def pipes(resnet_golden, resnet_heights_golden):
    out = {}
    for name, flags in FLAGS.items():
        rows = 103 if flags.get("use_delta_delta") else 90
        sd = resnet_heights_golden["h103"][0] if rows == 103 else resnet_golden[0]
        pre = cda.AudioPreprocessor(device="cuda", **{**SHIPPED, **flags})
        model = cda.create_model("residual", n_mels=rows, num_classes=2, in_channels=1, compute_dtype="bf16x3")
        model.load_state_dict(sd)
        model.cuda().eval()
        out[name] = (pre, model, cda.CoughPipeline(pre, model), rows)
    return out


def _fused_a1(pipe, model, b, rows):
    """The stem output the featurise kernel left in the pipeline's workspace (NCHW f32), through the model's parity tap."""
    dev = cuda_device()
    ws, _ = pipe._ws.lookup(dev)
    out = torch.empty((b, 32, ((rows - 1) // 2 + 1) // 2, 25), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().cough_resnet_read_activation(model._native(), ws.data_ptr(), b, rows, 101, 1, out.data_ptr(),
                                                        torch.cuda.current_stream(dev).cuda_stream),
               "cough_resnet_read_activation")
    return out


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("b", [1, 2, 5])
@pytest.mark.parametrize("name", list(FLAGS))
def test_fused_stem_equals_the_standalone_stem_bit_for_bit(pipes, clips, name, b):
    pre, model, pipe, rows = pipes[name]
    # B = 1: every kind of clip alone; B = 2: pairs that put every kind first and second; B = 5: all of them
    picks = {1: [[RANDOM0], [ZERO], [NAN], [IMPULSE]], 2: [[RANDOM0, ZERO], [NAN, IMPULSE], [IMPULSE, RANDOM1], [ZERO, NAN]],
             5: [[RANDOM0, ZERO, NAN, IMPULSE, RANDOM1]]}[b]
    for pick in picks:
        w = clips[pick].cuda()
        logits = pipe(w, normalize=True)
        a1 = _fused_a1(pipe, model, b, rows)
        feats = pre.featurize_batch(w, normalize=True)
        want = model(feats[:, None])
        a1_want = model.read_activation(1)
        assert feats.shape == (b, rows, 101) and a1.shape == a1_want.shape
        assert torch.equal(_bits(logits), _bits(want)), (name, pick)
        # a clip with a non-finite sample leaves the featurise kernel before the stem (its flag alone makes the logits NaN), so
        # its slice of a1 is never written: every other clip's a1 is compared, next to that clip as well
        keep = [i for i, kind in enumerate(pick) if kind != NAN]
        assert torch.equal(_bits(a1[keep]), _bits(a1_want[keep])), (name, pick)
        flat, flat_want = a1[keep].flatten(2), a1_want[keep].flatten(2)    # [clips, 32, pooled position]
        assert torch.equal(_bits(flat[:, :, 544:550]), _bits(flat_want[:, :, 544:550]))
        for i, kind in enumerate(pick):
            if kind == NAN:
                assert torch.isnan(logits[i]).all()
            else:
                assert torch.isfinite(logits[i]).all() and torch.isfinite(a1[i]).all()
        if RANDOM0 in pick:                                                # the stem output is not trivially zero
            assert a1[pick.index(RANDOM0)].abs().max() > 0
