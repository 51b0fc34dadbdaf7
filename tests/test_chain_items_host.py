"""One record per item, and the channel step in ``chain.host_plans``, without a GPU.

For every on/off combination of the four optional steps: ``draw_item_channel`` returns a ``chain.ItemDraw`` whose first
3, 4 and 5 fields are what ``draw_item``, ``draw_item_pitched`` and ``draw_item_reverb`` return from the same ``random``
state, and all four leave that state where the others leave it.  ``host_plans(..., channel=...)`` puts the channel's
plans last, as ``channel.plan_array``'s words, and changes no other array; a batch in which the channel alone fired has no
other plan, so nothing carries a shift and the loader gathers its rows.
"""
import itertools
import random

import numpy as np
import pytest

import cough_detector_amd as cda
from cough_detector_amd import chain as cchain
from cough_detector_amd import channel as cch

COMBINATIONS = list(itertools.product((False, True), repeat=4))
LENGTHS = [16000, 9000, 700, 257, 2, 1]


def _augmentor(speed, pitch, reverb, channel):
    rirs, mics = cda.synth_rirs(3, seed=2)[0], cda.synth_channels(5, seed=2)[0]
    return cda.AudioAugmentor(p_augment=0.6, speed=speed, pitch=pitch, reverb=rirs if reverb else None,
                              channel=mics if channel else None, p_clip=0.5, clip_range=(0.3, 0.9))


@pytest.mark.parametrize("on", COMBINATIONS, ids=["".join(str(int(v)) for v in on) for on in COMBINATIONS])
def test_the_older_draw_methods_are_prefixes_of_the_item(on):
    aug = _augmentor(*on)
    random.seed(1000 + sum(int(v) << k for k, v in enumerate(on)))
    seen = {name: 0 for name in cchain.ItemDraw._fields[1:]}
    for n in LENGTHS * 4:
        state = random.getstate()
        item = aug.draw_item_channel(n)
        end = random.getstate()
        assert type(item) is cchain.ItemDraw and cchain.ItemDraw._fields == ("record", "pair", "length", "steps", "rir", "channel")
        for method, k in (("draw_item", 3), ("draw_item_pitched", 4), ("draw_item_reverb", 5)):
            random.setstate(state)
            got = getattr(aug, method)(n)
            assert random.getstate() == end, method
            assert type(got) is tuple and len(got) == k, method
            assert bytes(got[0]) == bytes(item.record) and got[1:] == item[1:k], method
        for name, step_on in zip(("pair", "steps", "rir", "channel"), on):
            assert step_on or getattr(item, name) is None, name
            seen[name] += getattr(item, name) is not None
        assert item.length == (n if item.pair is None else cda.warp.warped_length(n, *item.pair))
        seen["length"] += 1
    assert [seen[name] > 0 for name in ("pair", "steps", "rir", "channel")] == list(on)      # every step that is on fired


SHIFTS = [5, -3, 0, 40]
ROWS = [1000, 2000, 300, 1500]
PAIRS = [None, (15000, 16000), None, (17000, 16000)]
STEPS = [2, None, 0, -1]
RIRS = [None, 1, 0, None]
MICS = [(0, 1.0), None, (4, 0.5), (2, 0.25)]


@pytest.mark.parametrize("pairs,steps,rirs", list(itertools.product((None, PAIRS), (None, STEPS), (None, RIRS))))
def test_host_plans_put_the_channel_last_and_leave_the_rest(pairs, steps, rirs):
    without = cchain.host_plans(SHIFTS, pairs, steps, ROWS, 16000, 2000, reverb=rirs)
    plans = cchain.host_plans(SHIFTS, pairs, steps, ROWS, 16000, 2000, reverb=rirs, channel=MICS, n_channels=5)
    assert list(plans.arrays) == list(without.arrays) + ["channel"]
    want = cch.plan_array([m if m is not None else (-1, 1.0) for m in MICS]).view(np.int32)
    got = plans.arrays["channel"]
    assert got.dtype == np.int32 and got.shape == (4, 2) and got.tobytes() == want.tobytes()
    for name, array in without.arrays.items():
        assert plans.arrays[name].dtype == array.dtype and plans.arrays[name].shape == array.shape
        assert plans.arrays[name].tobytes() == array.tobytes(), name
    assert plans[1:] == without[1:]
    # switched off, or no coin fired: the call without the keyword
    for off in (dict(channel=None), dict(channel=[None] * 4, n_channels=5)):
        same = cchain.host_plans(SHIFTS, pairs, steps, ROWS, 16000, 2000, reverb=rirs, **off)
        assert list(same.arrays) == list(without.arrays) and same[1:] == without[1:]
    with pytest.raises(ValueError):
        cchain.host_plans(SHIFTS, pairs, steps, ROWS, 16000, 2000, reverb=rirs, channel=MICS, n_channels=4)


def test_a_batch_in_which_only_the_channel_fired_gathers_its_rows():
    for pairs, steps, rirs in ((None, None, None), ([None] * 4, [None, 0, None, 0], [None] * 4)):
        plans = cchain.host_plans(SHIFTS, pairs, steps, ROWS, 16000, 2000, reverb=rirs, channel=MICS, n_channels=5)
        assert list(plans.arrays) == ["channel"] and plans.new_lengths == ROWS and plans.stretch_width == 0
        assert plans.width == (2000 if pairs is None else max(ROWS))
        asked = []
        go = cchain.launches(plans, lambda name: asked.append(name) or name, None, keep=True)
        # no launch in front of the kernel: the records keep their shifts and the loader takes cough_gather_rows
        assert go.speed is None and go.pitch is None and go.reverb is None and go.front == 0 and not go.chained
        assert go.channel == "channel" and asked == ["channel"]
    assert cchain.launches(None, None, None) == (None, None, None, None, 0, False)
