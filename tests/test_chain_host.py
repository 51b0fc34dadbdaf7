"""The waveform chain's host rules, without a GPU: who carries the time shift, how wide the output is, and what a batch
in which nothing fired runs.

The device calls are replaced by recorders that return zeros of the right shape (``warp_rows``, ``pitch_shift_rows``,
``AudioAugmentor._run``; ``cuda_device`` gives the CPU), and a seeded ``augment_batch`` / ``augment`` is driven through
them.  The expected tables below are literals, never produced by the code under test: per configuration the ordered
calls, the shift in each warp and stretch plan, the shifts of the records that reach ``_run``, the lengths handed on, the
output and stretch widths, the shape of the gaussian matrix, and the returned shape and lengths.  Row 2 is 200 samples
long: below the 257 samples the stretch needs, so the length arithmetic has to hand it through untouched.
"""
import random

import numpy as np
import pytest
import torch

import cough_detector_amd as cda
from cough_detector_amd import augmentation as caug
from cough_detector_amd import pitch as cpitch
from cough_detector_amd import warp as cwarp

LENGTHS = [300, 5000, 200]
WIDTH = 5000
_STRETCH = np.dtype([("shift", np.int32), ("reserved", np.int32), ("rate", np.float64)])


def _trace(monkeypatch, speed, pitch, p, single=False, seed=17):
    """The recorded calls of one seeded ``augment_batch`` (or, with ``single``, ``augment`` of row 1) and what it
    returned: ``(calls, returned shape, returned lengths)``."""
    calls = []
    cpu = torch.device("cpu")

    def warp_rows(src, offsets, lens, plans, n_samples, return_lengths=False):
        assert not return_lengths and all(t.device == cpu for t in (src, offsets, lens, plans))
        calls.append(("warp_rows", dict(offsets=offsets.tolist(), lengths=lens.tolist(), plans=plans.tolist(),
                                        width=int(n_samples))))
        return torch.zeros((lens.numel(), int(n_samples)), dtype=torch.float32)

    def pitch_shift_rows(src, offsets, lens, stretch, back, n_samples, stretch_width=None):
        plans = stretch.numpy().reshape(-1).view(_STRETCH)
        calls.append(("pitch_shift_rows", dict(offsets=offsets.tolist(), lengths=lens.tolist(),
                                               stretch_shifts=plans["shift"].tolist(),
                                               stretch_rates=[round(float(r), 6) for r in plans["rate"]],
                                               back=back.tolist(), width=int(n_samples), stretch_width=stretch_width)))
        return torch.zeros((lens.numel(), int(n_samples)), dtype=torch.float32)

    def run(self, x, clips, lengths, gaussian, seed):
        calls.append(("_run", dict(shape=tuple(x.shape), shifts=[c.shift for c in clips],
                                   lengths=None if lengths is None else [int(v) for v in lengths],
                                   gaussian=None if gaussian is None else tuple(gaussian.shape))))
        return torch.zeros(tuple(x.shape), dtype=torch.float32)

    monkeypatch.setattr(caug, "cuda_device", lambda: cpu)
    monkeypatch.setattr(cwarp, "warp_rows", warp_rows)
    monkeypatch.setattr(cpitch, "pitch_shift_rows", pitch_shift_rows)
    monkeypatch.setattr(cda.AudioAugmentor, "_run", run)
    aug = cda.AudioAugmentor(p_augment=p, speed=speed, pitch=pitch)
    random.seed(seed)
    torch.manual_seed(seed)
    if single:
        out = aug.augment(torch.ones((1, WIDTH)))
        return calls, tuple(out.shape), None
    out, lens = aug.augment_batch(torch.ones((len(LENGTHS), WIDTH)), lengths=LENGTHS, noise="host", return_lengths=True)
    assert lens.dtype == torch.int32
    return calls, tuple(out.shape), lens.tolist()


def _run_call(width, shifts, lengths):
    return ("_run", dict(shape=(len(shifts), width), shifts=shifts, lengths=lengths, gaussian=(len(shifts), width)))


_NOTHING = ([_run_call(5000, [0, 0, 0], LENGTHS)], (3, 5000), LENGTHS)
EXPECTED = {
    # the warp carries the shift; the stretch and the record carry none; everything is max n' wide
    (True, True, 1.0): ([
        ("warp_rows", dict(offsets=[0, 5000, 10000], lengths=[300, 5000, 200],
                           plans=[[36, 15326, 16000], [-495, 15415, 16000], [30, 16965, 16000]], width=5190)),
        ("pitch_shift_rows", dict(offsets=[0, 5190, 10380], lengths=[314, 5190, 189], stretch_shifts=[0, 0, 0],
                                  stretch_rates=[0.890899, 0.943874, 1.0],
                                  back=[[0, 17959, 16000], [0, 16951, 16000], [0, 1, 1]], width=5190, stretch_width=5499)),
        _run_call(5190, [0, 0, 0], [314, 5190, 189])], (3, 5190), [314, 5190, 189]),
    (True, False, 1.0): ([
        ("warp_rows", dict(offsets=[0, 5000, 10000], lengths=[300, 5000, 200],
                           plans=[[36, 15326, 16000], [-231, 15207, 16000], [39, 17000, 16000]], width=5261)),
        _run_call(5261, [0, 0, 0], [314, 5261, 189])], (3, 5261), [314, 5261, 189]),
    # no speed step: the stretch carries the shift, and the output is N wide; the 200-sample row keeps its length
    (False, True, 1.0): ([
        ("pitch_shift_rows", dict(offsets=[0, 5000, 10000], lengths=[300, 5000, 200], stretch_shifts=[36, -502, -7],
                                  stretch_rates=[1.0, 0.943874, 1.122462],
                                  back=[[0, 1, 1], [0, 16951, 16000], [0, 14254, 16000]], width=5000, stretch_width=5297)),
        _run_call(5000, [0, 0, 0], LENGTHS)], (3, 5000), LENGTHS),
    # neither: the record carries the shift
    (False, False, 1.0): ([_run_call(5000, [36, -779, -14], LENGTHS)], (3, 5000), LENGTHS),
    # no coin fired: one launch, whatever is switched on
    (True, True, 0.0): _NOTHING, (True, False, 0.0): _NOTHING, (False, True, 0.0): _NOTHING, (False, False, 0.0): _NOTHING,
    "single": ([
        ("pitch_shift_rows", dict(offsets=[0], lengths=[5000], stretch_shifts=[569], stretch_rates=[0.890899],
                                  back=[[0, 17959, 16000]], width=5000, stretch_width=5612)),
        _run_call(5000, [0], [5000])], (1, 5000), None),
}


@pytest.mark.parametrize("speed,pitch,p", [(s, q, p) for p in (1.0, 0.0) for s in (True, False) for q in (True, False)])
def test_augment_batch_runs_the_chain_it_ran_before(monkeypatch, speed, pitch, p):
    assert _trace(monkeypatch, speed, pitch, p) == EXPECTED[speed, pitch, p]


def test_augment_of_one_clip_with_a_pitch_step(monkeypatch):
    assert _trace(monkeypatch, False, True, 1.0, single=True, seed=19) == EXPECTED["single"]
