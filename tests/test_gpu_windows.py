"""Composed windows on the MI355X (cough_detector_amd/windows.py, csrc/windows.hip) against tests/windows_ref.py, against
the kernels of the scenes whose arithmetic they fuse, and through the loader.

One ragged batch (``windows_ref.batch_rows``) runs at seven widths: a single sample, one short of / exactly / one past the
256 samples of a stretch, one past a multiple of it, the shipped second, and one past the 16384 samples up to which the
kernel keeps the background in registers (the path that reads it twice).

Tolerances.  None, but for one: the output, the gains and the background power are compared bit for bit (NaNs of any
payload count as equal: the contract does not fix a payload) with the restatement, which sums the power in the kernel's
order and evaluates the gain on the device's own powers, and with ``span_power`` / ``compose_scenes``.  The power is also
held against numpy's float64 sum within ``2 * n * 2^-53`` relative, tests/test_gpu_scenes.py's bound for span powers:
every term is exact and non-negative, so any order of n of them is within ``(n - 1) * 2^-53`` of the exact sum.
"""
import random

import numpy as np
import pytest
import torch

import cough_detector_amd as cda
from cough_detector_amd import scenes as cscenes
from cough_detector_amd import windows as cwin
import scenes_ref as R
import windows_ref as W

pytestmark = pytest.mark.gpu
SHIPPED = dict(use_pcen=False, use_pre_emphasis=False, use_delta_delta=False, use_spectral_contrast=False)
WIDTHS = [1, 255, 256, 257, 4097, 16000, 16385]
SR = 16000


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32 if x.dtype == np.float32 else np.uint64)


def _same(a, b):
    """Bit for bit, NaNs of any payload counting as equal."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.array_equal(_bits(a[~np.isnan(a)]), _bits(b[~np.isnan(b)]))


def _bank(clips, labels=0):
    labels = [labels] * len(clips) if isinstance(labels, int) else labels
    return cda.DeviceClipBank([torch.from_numpy(c) for c in clips], labels, device="cuda")


@pytest.fixture(scope="module")
def banks():
    bgs, evs = W.banks()
    bg_bank, ev_bank = _bank(bgs), _bank(evs, 1)
    assert {int(o) % 4 for o in bg_bank.offsets} == {int(o) % 4 for o in ev_bank.offsets} == {0, 1, 2, 3}
    return bgs, evs, bg_bank, ev_bank, cwin.event_powers(ev_bank)


@pytest.fixture(scope="module", params=WIDTHS)
def case(request, banks):
    width = request.param
    bgs, evs, bg_bank, ev_bank, p_ev = banks
    rows = W.batch_rows(width)
    plan = cda.WindowPlan(*W.plan_arrays(rows))
    out, p_bg, gains = cda.compose_windows(bg_bank, ev_bank, plan, width, event_power=p_ev, return_diagnostics=True)
    assert out.shape == (len(rows), width) and out.dtype == torch.float32 and p_bg.dtype == torch.float64
    return dict(width=width, rows=rows, plan=plan, out=out.cpu().numpy(), p_bg=p_bg.cpu().numpy(), gains=gains.cpu().numpy(),
                p_ev=p_ev.cpu().numpy(), snr_linear=10.0 ** (plan.snr_db / 10.0))


# ------------------------------------------------------------------------------------------------ against the restatement
def test_output_gains_and_power_equal_the_restatement(case, banks):
    bgs, evs = banks[:2]
    c, width = case, case["width"]
    for r, row in enumerate(c["rows"]):
        bg = None if row[0] < 0 else bgs[row[0]]
        events = W.row_events(row, evs, c["snr_linear"][r])
        p_ev = [c["p_ev"][e[0]] for e in row[3]]
        want, _, gains = W.compose_slices(bg, row[1], row[2], width, events, p_ev=p_ev, p_bg=c["p_bg"][r])
        assert _same(c["out"][r], want), (width, r, row)
        assert _same(c["gains"][r], np.array(list(gains) + [0.0] * (4 - len(gains)), np.float32)), (width, r, c["gains"][r], gains)
        # the power itself, summed on the host in the kernel's order
        p_bg = 0.0 if bg is None else W.power_order(R.span_ref(bg, row[1], width))
        assert _same(np.float64(c["p_bg"][r]), np.float64(p_bg)), (width, r, c["p_bg"][r], p_bg)
        if width <= 257:                                                   # and sample by sample where that is quick
            assert _same(c["out"][r], W.compose_loop(bg, row[1], row[2], width, events, p_ev=p_ev, p_bg=c["p_bg"][r])[0]), (width, r)
    for e in range(len(evs)):                                              # the event powers are whole-clip powers in that order too
        assert _same(np.float64(c["p_ev"][e]), np.float64(W.power_order(evs[e]))), e


def test_the_batch_holds_what_it_is_meant_to_hold(case):
    c, width, rows = case, case["width"], case["rows"]
    by_bg = {b: [r for r, row in enumerate(rows) if row[0] == b] for b in (-1, W.BG_SILENT, W.BG_NAN, W.BG_INF)}
    for r in by_bg[-1] + by_bg[W.BG_SILENT]:                               # silence: P_bg 0, every gain 1
        assert c["p_bg"][r] == 0.0 and (c["gains"][r][:len(rows[r][3])] == 1.0).all()
    if width > 100:
        assert all(np.isnan(c["p_bg"][r]) and np.isnan(c["out"][r]).any() for r in by_bg[W.BG_NAN])
        assert all(c["p_bg"][r] == np.inf and c["gains"][r][0] == 1.0 for r in by_bg[W.BG_INF])
    zero = [r for r, row in enumerate(rows) if row[3] and row[3][0][0] == W.EV_ZERO][0]
    assert c["gains"][zero][0] == 1.0 and c["gains"][zero][1] not in (0.0, 1.0)
    empty = [r for r, row in enumerate(rows) if not row[3] and row[0] >= 0][0]
    assert (c["gains"][empty] == 0.0).all() and c["p_bg"][empty] > 0
    assert not np.isnan(np.delete(c["out"], by_bg[W.BG_NAN] + by_bg[W.BG_INF], axis=0)).any()
    if width >= 255:                                                       # events reach across both edges and over each other
        spans = [[(on, on + W.EV_LENGTHS[cl]) for cl, on, _ in row[3]] for row in rows]
        assert any(a < 0 < b for s in spans for a, b in s) and any(a < width < b for s in spans for a, b in s)
        assert any(a < 0 and b > width for s in spans for a, b in s) and any(b <= 0 or a >= width for s in spans for a, b in s)
        assert any(len(s) == 4 and max(a for a, _ in s) < min(b for _, b in s) for s in spans)


def test_the_background_power_is_span_powers(case, banks):
    bgs, _, bg_bank = banks[:3]
    c, width = case, case["width"]
    real = [r for r, row in enumerate(c["rows"]) if row[0] >= 0]
    clips, starts = [c["rows"][r][0] for r in real], [c["rows"][r][1] for r in real]
    spans = cscenes.span_power(bg_bank, clips, starts, [width] * len(real)).cpu().numpy()
    assert _same(c["p_bg"][real], spans)
    for r, b, s in zip(real, clips, starts):
        want = R.power_ref(bgs[b], s, width)
        if np.isfinite(want):
            assert abs(c["p_bg"][r] - want) <= 2 * width * 2.0 ** -53 * want, (width, r, c["p_bg"][r], want)


def test_rows_inside_and_apart_equal_compose_scenes(case, banks):
    _, evs, bg_bank, ev_bank = banks[:4]
    c, width = case, case["width"]
    fit = [r for r, row in enumerate(c["rows"]) if W.inside_and_apart(row, width)]
    assert len(fit) >= 5 and any(len(c["rows"][r][3]) >= (2 if width >= 255 else 1) for r in fit)
    scene, clip, onset, snr, slot = [], [], [], [], []
    for s, r in enumerate(fit):
        for e in sorted(range(len(c["rows"][r][3])), key=lambda e: c["rows"][r][3][e][1]):
            cl, on, db = c["rows"][r][3][e]
            scene.append(s), clip.append(cl), onset.append(on), snr.append(db), slot.append((r, e))
    plan = cda.ScenePlan(np.array([c["rows"][r][0] for r in fit]), np.array([c["rows"][r][1] for r in fit]),
                         np.array([c["rows"][r][2] for r in fit], np.float32), np.full(len(fit), width), np.array(scene, np.int64),
                         np.array(clip, np.int64), np.array(onset, np.int64), np.array(snr))
    scenes, truth = cda.compose_scenes(bg_bank, ev_bank, plan)
    assert _same(scenes.data.cpu().numpy().reshape(len(fit), width), c["out"][fit])
    gains = truth.gain.cpu().numpy()
    assert _same(gains, np.array([c["gains"][r][e] for r, e in slot], np.float32))


def test_a_row_alone_and_a_repeated_call_give_the_same_bits(case, banks):
    bg_bank, ev_bank, p_ev = banks[2:]
    c, width, plan = case, case["width"], case["plan"]
    again = cda.compose_windows(bg_bank, ev_bank, plan, width, return_diagnostics=True)     # the event powers worked out anew
    assert np.array_equal(_bits(again[0].cpu().numpy()), _bits(c["out"])) and np.array_equal(_bits(again[1].cpu().numpy()), _bits(c["p_bg"]))
    assert np.array_equal(_bits(again[2].cpu().numpy()), _bits(c["gains"]))
    n = len(plan)
    for r in (0, 7, 21, n - 12, n - 10, n - 8, n - 5, n - 1):
        one = cda.WindowPlan(*(getattr(plan, f)[r:r + 1] for f in ("background", "bg_start", "bg_gain", "n_events", "event_clip", "onset", "snr_db")))
        out = torch.full((width,), -7.0, dtype=torch.float32, device="cuda")
        got = cda.compose_windows(bg_bank, ev_bank, one, width, event_power=p_ev, out=out)
        assert got.data_ptr() == out.data_ptr() and np.array_equal(_bits(out.cpu().numpy()), _bits(c["out"][r])), (width, r)


# ------------------------------------------------------------------------------------------------ the Python front
def test_host_held_bad_plans_raise_and_empty_plans_launch_nothing(banks):
    bg_bank, ev_bank, p_ev = banks[2:]
    good = cda.WindowPlan(*W.plan_arrays(W.batch_rows(300)))
    for field, value, match in (("background", np.full(len(good), len(bg_bank)), "background indices"),
                                ("bg_start", np.full(len(good), 50000), "bg_start"), ("n_events", np.full(len(good), 5), "n_events"),
                                ("event_clip", np.full((len(good), 4), len(ev_bank)), "event clips")):
        bad = cda.WindowPlan(**{**{f: getattr(good, f) for f in ("background", "bg_start", "bg_gain", "n_events", "event_clip",
                                                                  "onset", "snr_db")}, field: value})
        if field == "event_clip":
            bad.n_events = np.full(len(good), 1)
        with pytest.raises(ValueError, match=match):
            cda.compose_windows(bg_bank, ev_bank, bad, 300)
    with pytest.raises(ValueError, match="width"):
        cda.compose_windows(bg_bank, ev_bank, good, 2**20 + 1)
    with pytest.raises(ValueError, match="out must be"):
        cda.compose_windows(bg_bank, ev_bank, good, 300, out=torch.zeros(300, device="cuda"))
    with pytest.raises(ValueError, match="overlaps a bank"):              # the C ABI's own check: composing into a bank
        cda.compose_windows(bg_bank, ev_bank, cda.WindowPlan(*(getattr(good, f)[:1] for f in (
            "background", "bg_start", "bg_gain", "n_events", "event_clip", "onset", "snr_db"))), 300, out=bg_bank.data[1000:1300])
    empty = cda.WindowPlan(*W.plan_arrays([]))
    out, p_bg, gains = cda.compose_windows(bg_bank, ev_bank, empty, 300, return_diagnostics=True)
    assert out.shape == (0, 300) and p_bg.numel() == 0 and gains.shape == (0, 4)
    nothing = cda.DeviceClipBank([], [], device="cuda")                    # empty banks: silence, and events there are none of
    rows = cda.compose_windows(nothing, nothing, cda.WindowPlan(np.array([-1, -1]), np.zeros(2, int), np.ones(2, np.float32),
                                                               np.zeros(2, int), np.full((2, 4), -1), np.zeros((2, 4), int), np.zeros((2, 4))), 7)
    assert rows.cpu().tolist() == [[0.0] * 7] * 2


# ------------------------------------------------------------------------------------------------ the loader
@pytest.fixture(scope="module")
def corpus():
    rng = np.random.default_rng(9)
    backgrounds = _bank([(rng.standard_normal(n) * 0.05).astype(np.float32) for n in (30000, 48001, 7000, 900)])
    lengths, labels = (6000, 9001, 3000, 12000, 5000, 2500), [1, 1, 1, 1, 0, 0]
    events = _bank([(rng.standard_normal(n) * np.hanning(n)).astype(np.float32) for n in lengths], labels)
    return backgrounds, events, cda.AudioPreprocessor(device="cuda", **SHIPPED)


def _seed_everything(k):
    random.seed(k)
    np.random.seed(k)
    torch.manual_seed(k)


@pytest.mark.parametrize("mix", [False, True])
@pytest.mark.parametrize("draws", ["host", "device"])
def test_a_batch_equals_its_parts(corpus, draws, mix):
    """``ComposedWindowLoader`` against the plan restated on the host (``windows_ref.draw_ref``), ``compose_windows`` of it
    into a fresh bank and a plain ``DeviceDataLoader`` over that bank, under the same seeds: bit for bit."""
    backgrounds, events, pre = corpus
    b, width = 8, int(pre.segment_samples)
    make = lambda: (cda.AudioAugmentor(sample_rate=SR, speed=True), cda.SpecAugment(), cda.MixUp(0.4) if mix else None)
    aug, spec, mixup = make()
    loader = cda.ComposedWindowLoader(backgrounds, events, pre, batch_size=b, batches_per_epoch=2, seed=5, audio_augmentor=aug,
                                      spec_augmentor=spec, mixup=mixup, draws=draws, snr_range=(3, 12))
    assert len(loader) == 2 and loader.margin == cda.edge_margin(aug, width) > int(0.2 * width)
    _seed_everything(3)
    got, plans = [], []
    for feats, targets in loader:
        got.append((feats.cpu(), targets.cpu()))
        plans.append(loader.last_plan)
    assert len(got) == 2 and got[0][0].shape[:2] == (b, 1) and got[0][0].shape[2:] == loader.inner.feature_shape()

    aug, spec, mixup = make()
    bl, el, lab = backgrounds.lengths.numpy(), events.lengths.numpy(), events.labels.numpy()
    _seed_everything(3)
    for k in range(2):
        drawn = W.draw_ref(bl, el, lab, b, width, SR, 5 + k, snr_range=(3, 12), margin=cda.edge_margin(aug, width),
                           rho_min=cwin.speed_ratios(aug)[0])
        plan = cda.WindowPlan(*(drawn[f] for f in ("background", "bg_start", "bg_gain", "n_events", "event_clip", "onset", "snr_db")))
        for f in ("background", "bg_start", "bg_gain", "n_events", "event_clip", "onset", "snr_db"):
            assert getattr(plans[k], f).tolist() == getattr(plan, f).tolist(), (k, f)
        labels = plan.labels(lab)
        rows = cda.compose_windows(backgrounds, events, plan, width)
        bank = cda.DeviceClipBank.from_packed(rows.reshape(-1), [width] * b, labels)
        plain = cda.DeviceDataLoader(bank, pre, batch_size=b, audio_augmentor=aug, spec_augmentor=spec, is_training=True,
                                     use_weighted_sampler=False, draws=draws, mixup=mixup)
        if draws == "device":
            feats, targets = plain.launch_batch_drawn(range(b), 5 + k)
        else:
            feats, targets = plain.launch_batch(range(b), plain.draw_batch(range(b)))
        assert torch.equal(got[k][0].view(torch.int32), feats.cpu().view(torch.int32)), (draws, mix, k)
        if mix:
            assert got[k][1].shape == (b, 2) and torch.equal(got[k][1], targets.cpu())
        else:
            assert got[k][1].tolist() == labels.tolist() == targets.cpu().tolist()
    assert not mix or any(0.0 < float(v) < 1.0 for v in got[0][1].reshape(-1))


def test_two_epochs_repeat_themselves_under_one_seed(corpus):
    backgrounds, events, pre = corpus
    runs = []
    for _ in range(2):
        loader = cda.ComposedWindowLoader(backgrounds, events, pre, batch_size=8, batches_per_epoch=2, seed=21,
                                          audio_augmentor=cda.AudioAugmentor(sample_rate=SR), draws="device", p_cough=0.5)
        _seed_everything(4)
        runs.append([[(f.cpu(), t.cpu()) for f, t in loader] for _ in range(2)])
    for e in range(2):
        for k in range(2):
            assert torch.equal(runs[0][e][k][0].view(torch.int32), runs[1][e][k][0].view(torch.int32)), (e, k)
            assert torch.equal(runs[0][e][k][1], runs[1][e][k][1])
    assert not torch.equal(runs[0][0][0][0], runs[0][1][0][0])            # epoch 1 is not epoch 0 again
    assert loader.epoch == 2 and loader.batch_seed(1, 1) == 21 + 2 + 1
    targets = torch.cat([t for epoch in runs[0] for _, t in epoch])
    assert set(targets.tolist()) == {0, 1}


def test_a_training_step_on_a_composed_batch(corpus):
    backgrounds, events, pre = corpus
    torch.manual_seed(0)
    model = cda.create_model("small", n_mels=90, num_classes=2, in_channels=1)
    trainer = cda.SmallTrainer(model, lr=1e-3, weight_decay=0.01, seed=0)
    loader = cda.ComposedWindowLoader(backgrounds, events, pre, batch_size=8, batches_per_epoch=1, seed=1)
    feats, targets = next(iter(loader))
    loss, outputs = trainer.step(feats, targets)
    assert np.isfinite(float(loss)) and outputs.shape == (8, 2) and torch.isfinite(outputs).all()
    soft = cda.ComposedWindowLoader(backgrounds, events, pre, batch_size=8, batches_per_epoch=1, seed=1, mixup=cda.MixUp(0.4))
    result = cda.train_epoch_async(trainer, soft, 0)
    assert np.isfinite(result["loss"])


# ------------------------------------------------------------------------------------------------ the validation bank
def test_scene_window_bank_cuts_the_unambiguous_windows(corpus):
    backgrounds, events, pre = corpus
    coughs = events.subset([0, 1, 2])
    plan = cda.draw_scene_plan(backgrounds, coughs, 4, 5.0, events_per_scene=(1, 3), min_gap_seconds=0.3, seed=2)
    scenes, truth = cda.compose_scenes(backgrounds, coughs, plan)
    bank, table = cda.scene_window_bank(scenes, truth, pre)
    window, hop = int(pre.segment_samples), 4000
    every = cda.window_labels(truth, scenes.lengths.numpy(), window, hop, SR)
    assert len(every) == 4 * 17 and set(every.label.tolist()) == {1, 0, -1}
    keep = every.label >= 0
    assert len(bank) == len(table) == int(keep.sum()) and (table.label >= 0).all()
    assert table.recording.tolist() == every.recording[keep].tolist() and table.window.tolist() == every.window[keep].tolist()
    assert bank.labels.tolist() == table.label.tolist() == every.label[keep].tolist() and table.overlap.tolist() == every.overlap[keep].tolist()
    assert bank.lengths.tolist() == [window] * len(bank)
    cut = scenes.cut(table.recording, table.window * hop, np.full(len(table), window))
    assert torch.equal(bank.data.view(torch.int32), cut.data.view(torch.int32))
    data, source = bank.data.cpu().numpy(), scenes.data.cpu().numpy()
    for j in (0, len(table) // 2, len(table) - 1):
        o = int(scenes.offsets[table.recording[j]]) + int(table.window[j]) * hop
        assert np.array_equal(data[j * window:(j + 1) * window], source[o:o + window])
    feats, targets = next(iter(cda.DeviceDataLoader(bank, pre, batch_size=len(bank), is_training=False)))
    assert feats.shape[0] == len(bank) and targets.cpu().tolist() == table.label.tolist()
