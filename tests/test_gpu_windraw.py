"""The window plans drawn on the MI355X (``cough_draw_window_plans``) against the numpy restatement of the draw contract
(tests/windraw_ref.py), bit for bit; the composer on device-held records against the composer on the same records
uploaded; and ``ComposedWindowLoader(plan_draws="device")`` against its parts.  Every batch is a few hundred rows at
most: the kernel is one thread per row, so what can go wrong does so at the workgroup's edges (T - 1, T, T + 1, 2T + 1
rows), at the ends of the integer ranges and in the slot bookkeeping, none of which needs size."""
import random

import numpy as np
import pytest
import torch

import cough_detector_amd as cda
from cough_detector_amd import windows as cwin
import windraw_ref as D

pytestmark = pytest.mark.gpu
SHIPPED = dict(use_pcen=False, use_pre_emphasis=False, use_delta_delta=False, use_spectral_contrast=False)
SR, T = 16000, D.THREADS
SIZES = (1, T - 1, T, T + 1, 2 * T + 1)
BG = (48000, 7, 20000)
# shorter than m = 1600, exactly m, longer than a row of 16000; two distractors
EV, LAB = (1600, 3000, 800, 1, 5000, 2400, 40000), (1, 1, 1, 1, 0, 0, 1)
_SPEED = cda.AudioAugmentor(sample_rate=SR, speed=True)
CHAIN = dict(margin=cda.edge_margin(_SPEED, 16000), rho_min=cwin.speed_ratios(_SPEED)[0])
CASES = {
    "defaults": dict(),
    "seed 2^32 - 1": dict(seed=2**32 - 1),
    "seed 2^64 - 1": dict(seed=2**64 - 1, p_distractor=0.7, bg_gain_range=(0.25, 2.0)),
    "no backgrounds": dict(bg=()),
    "a background of one sample": dict(bg=(1,)),
    "no distractors": dict(ev=EV[:4], lab=LAB[:4]),
    "p_cough 0": dict(p_cough=0.0, p_distractor=1.0),
    "p_cough 1": dict(p_cough=1.0),
    "one cough": dict(coughs_per_window=(1, 1), p_cough=0.9, p_distractor=1.0),
    "one or two coughs": dict(coughs_per_window=(1, 2), p_cough=0.9, p_distractor=1.0),
    "four coughs": dict(coughs_per_window=(4, 4), p_cough=0.9, p_distractor=1.0),
    "up to four and the chain's margin": dict(coughs_per_window=(1, 4), p_cough=0.8, p_distractor=0.9, snr_range=(0, 3), **CHAIN),
    "margin 0 explicitly": dict(margin=0, rho_min=1.0, coughs_per_window=(2, 3)),
    "width 1": dict(width=1, m=1),
    "width 257": dict(width=257, m=16, p_distractor=0.8),
}


def _bank(lengths, labels):
    rng = np.random.default_rng(len(lengths))
    return cda.DeviceClipBank([torch.from_numpy((rng.standard_normal(n) * 0.1).astype(np.float32)) for n in lengths], list(labels))


@pytest.fixture(scope="module", params=list(CASES))
def case(request):
    kw = dict(CASES[request.param])
    bg, ev, lab = kw.pop("bg", BG), kw.pop("ev", EV), kw.pop("lab", LAB)
    width, m, seed = kw.pop("width", 16000), kw.pop("m", 1600), kw.pop("seed", 0)
    backgrounds, events = _bank(bg, [0] * len(bg)), _bank(ev, lab)
    want = D.draw_batch(seed, SIZES[-1], D.arguments(bg, ev, lab, width, m=m, **kw))
    # sample_rate 1 and min_overlap_seconds m: m samples exactly
    draw = lambda b: cda.draw_window_records(backgrounds, events, b, width, seed, sample_rate=1, min_overlap_seconds=float(m), **kw)
    return request.param, backgrounds, events, width, draw, want


def test_records_and_labels_equal_the_restatement_bit_for_bit(case):
    name, _, _, _, draw, (want, want_labels) = case
    for b in SIZES:
        records, labels = draw(b)
        assert records.shape == (b, 80) and records.dtype == torch.uint8 and labels.shape == (b,) and labels.dtype == torch.int64
        got = cwin.read_window_records(records)
        for f in D.PLAN_DTYPE.names:                                     # name the first field that differs
            assert got[f].tobytes() == want[f][:b].tobytes(), (name, b, f, got[f][:4], want[f][:4])
        assert D.same_records(got, want[:b]) and labels.cpu().tolist() == want_labels[:b].tolist(), (name, b)


def test_a_repeated_call_and_a_larger_batch_give_the_same_rows(case):
    name, _, _, _, draw, _ = case
    (r1, l1), (r2, l2), (r3, l3) = draw(2 * T + 1), draw(2 * T + 1), draw(T + 1)
    assert torch.equal(r1, r2) and torch.equal(l1, l2), name
    assert torch.equal(r1[:T + 1], r3) and torch.equal(l1[:T + 1], l3), name


def test_composing_from_device_records_equals_composing_the_same_records_uploaded(case):
    name, backgrounds, events, width, draw, (want, _) = case
    b = T + 1
    records, _ = draw(b)
    got = cda.compose_window_records(backgrounds, events, records, width, return_diagnostics=True)
    rec = want[:b]
    used = np.arange(4)[None, :] < rec["n_events"][:, None]
    # the same records as a host plan: snr_db is only carried, the launch below uploads rec itself
    plan = cda.WindowPlan(rec["background"], rec["bg_start"], rec["bg_gain"], rec["n_events"], rec["clip"], rec["onset"],
                          np.zeros((b, 4))).checked(backgrounds.lengths.numpy(), events.lengths.numpy(), width)
    assert plan.records()["clip"].tolist() == rec["clip"].tolist() and plan.records()["onset"].tolist() == rec["onset"].tolist()
    uploaded = torch.from_numpy(rec.view(np.uint8).reshape(b, 80).copy()).cuda()
    out = torch.empty((b, width), dtype=torch.float32, device="cuda")
    p_bg, gains = torch.empty(b, dtype=torch.float64, device="cuda"), torch.empty((b, 4), dtype=torch.float32, device="cuda")
    cwin._launch_records(backgrounds, events, uploaded, b, width, cwin.event_powers(events), out, p_bg, gains)
    assert torch.equal(got[0].view(torch.int32), out.view(torch.int32)), name
    assert torch.equal(got[1].view(torch.int64), p_bg.view(torch.int64)) and torch.equal(got[2].view(torch.int32), gains.view(torch.int32)), name
    assert torch.isfinite(got[0]).all() and (got[2].cpu().numpy()[~used] == 0.0).all()
    if used.any() and width > 1:
        assert (got[2].cpu().numpy()[used] > 0).all()
    again = torch.full((b * width,), float("nan"), device="cuda")
    assert cda.compose_window_records(backgrounds, events, records, width, event_power=cwin.event_powers(events), out=again).data_ptr() == again.data_ptr()
    assert torch.equal(again.view(b, width).view(torch.int32), out.view(torch.int32))


def test_tables_are_kept_and_checked():
    backgrounds, events = _bank(BG, [0] * 3), _bank(EV, LAB)
    tables = cwin.WindowDrawTables.build(events, (5, 20))
    assert tables.coughs.cpu().tolist() == [0, 1, 2, 3, 6] and tables.distractors.cpu().tolist() == [4, 5]
    assert tables.snr.cpu().numpy().tobytes() == D.snr_levels(5, 20).tobytes()
    a, b = cda.draw_window_records(backgrounds, events, 9, 16000, 4, tables=tables), cda.draw_window_records(backgrounds, events, 9, 16000, 4)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(ValueError, match="tables must be"):
        cda.draw_window_records(backgrounds, events, 9, 16000, 4, snr_range=(0, 3), tables=tables)
    with pytest.raises(ValueError, match="tables must be"):
        cda.draw_window_records(backgrounds, events.subset([0, 4]), 9, 16000, 4, tables=tables)
    empty = cda.draw_window_records(backgrounds, events, 0, 16000, 4)
    assert empty[0].shape == (0, 80) and empty[1].shape == (0,)
    assert cda.compose_window_records(backgrounds, events, empty[0], 16000).shape == (0, 16000)


# ------------------------------------------------------------------------------------------------ the loader
@pytest.fixture(scope="module")
def corpus():
    rng = np.random.default_rng(9)
    bgs = [(rng.standard_normal(n) * 0.05).astype(np.float32) for n in (30000, 48001, 7000, 900)]
    lengths, labels = (6000, 9001, 3000, 12000, 5000, 2500), [1, 1, 1, 1, 0, 0]
    evs = [(rng.standard_normal(n) * np.hanning(n)).astype(np.float32) for n in lengths]
    return (cda.DeviceClipBank([torch.from_numpy(x) for x in bgs], [0] * 4), cda.DeviceClipBank([torch.from_numpy(x) for x in evs], labels),
            cda.AudioPreprocessor(device="cuda", **SHIPPED))


def _seed_everything(k):
    random.seed(k)
    np.random.seed(k)
    torch.manual_seed(k)


@pytest.mark.parametrize("mix", [False, True])
@pytest.mark.parametrize("draws", ["host", "device"])
def test_a_device_drawn_batch_equals_its_parts(corpus, draws, mix):
    """``ComposedWindowLoader(plan_draws="device")`` against the records restated on the host, composed
    (``compose_window_records`` of their upload) into a fresh bank that carries the restated labels, and a plain
    ``DeviceDataLoader`` over that bank, under the same seeds: features and targets bit for bit."""
    backgrounds, events, pre = corpus
    b, width = 8, int(pre.segment_samples)
    make = lambda: (cda.AudioAugmentor(sample_rate=SR, speed=True), cda.SpecAugment(), cda.MixUp(0.4) if mix else None)
    aug, spec, mixup = make()
    loader = cda.ComposedWindowLoader(backgrounds, events, pre, batch_size=b, batches_per_epoch=2, seed=5, audio_augmentor=aug,
                                      spec_augmentor=spec, mixup=mixup, draws=draws, snr_range=(3, 12), plan_draws="device")
    _seed_everything(3)
    got = []
    for feats, targets in loader:
        assert loader.last_plan is None and loader.last_records.shape == (b, 80) and loader.last_labels.shape == (b,)
        got.append((feats.cpu(), targets.cpu(), cwin.read_window_records(loader.last_records), loader.last_labels.cpu()))
    assert len(got) == 2 and got[0][0].shape[:2] == (b, 1) and got[0][0].shape[2:] == loader.inner.feature_shape()

    aug, spec, mixup = make()
    a = D.arguments(backgrounds.lengths.numpy(), events.lengths.numpy(), events.labels.numpy(), width, snr_range=(3, 12),
                    margin=cda.edge_margin(aug, width), rho_min=cwin.speed_ratios(aug)[0])
    _seed_everything(3)
    for k in range(2):
        rec, labels = D.draw_batch(5 + k, b, a)
        assert D.same_records(got[k][2], rec) and got[k][3].tolist() == labels.tolist(), k
        rows = cda.compose_window_records(backgrounds, events, torch.from_numpy(rec.view(np.uint8).reshape(b, 80).copy()).cuda(), width)
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
    # (under draws="host" batch 0's permutation happens to pair every row with one of its own label: look at both)
    assert not mix or any(0.0 < float(v) < 1.0 for g in got for v in g[1].reshape(-1))
    assert set(np.concatenate([g[3].numpy() for g in got]).tolist()) == {0, 1}


def test_the_host_drawn_loader_is_what_it_was(corpus):
    """``plan_draws`` left alone: the batch of ``draw_window_plan``'s plan, ``last_plan`` set, no device records."""
    backgrounds, events, pre = corpus
    loader = cda.ComposedWindowLoader(backgrounds, events, pre, batch_size=8, batches_per_epoch=1, seed=5)
    feats, targets = next(iter(loader))
    plan = cda.draw_window_plan(backgrounds, events, 8, int(pre.segment_samples), SR, 5)
    assert loader.last_records is None and loader.last_plan.onset.tolist() == plan.onset.tolist()
    assert targets.cpu().tolist() == plan.labels(events.labels).tolist()
    with pytest.raises(ValueError, match="targets must be"):
        loader.inner.launch_batch(range(8), loader.inner.draw_batch(range(8)), targets=torch.zeros(8, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="targets must be"):
        loader.inner.launch_batch(range(8), loader.inner.draw_batch(range(8)), targets=torch.zeros(7, dtype=torch.int64, device="cuda"))


def test_two_device_drawn_epochs_repeat_themselves_under_one_seed(corpus):
    backgrounds, events, pre = corpus
    runs = []
    for _ in range(2):
        loader = cda.ComposedWindowLoader(backgrounds, events, pre, batch_size=8, batches_per_epoch=2, seed=21,
                                          audio_augmentor=cda.AudioAugmentor(sample_rate=SR), draws="device", plan_draws="device")
        runs.append([[(f.cpu(), t.cpu()) for f, t in loader] for _ in range(2)])
    for e in range(2):
        for k in range(2):
            assert torch.equal(runs[0][e][k][0].view(torch.int32), runs[1][e][k][0].view(torch.int32)), (e, k)
            assert torch.equal(runs[0][e][k][1], runs[1][e][k][1])
    assert not torch.equal(runs[0][0][0][0], runs[0][1][0][0])            # epoch 1 is not epoch 0 again
    assert set(torch.cat([t for epoch in runs[0] for _, t in epoch]).tolist()) == {0, 1}


def test_a_training_step_on_a_device_drawn_batch(corpus):
    backgrounds, events, pre = corpus
    torch.manual_seed(0)
    model = cda.create_model("small", n_mels=90, num_classes=2, in_channels=1)
    trainer = cda.SmallTrainer(model, lr=1e-3, weight_decay=0.01, seed=0)
    loader = cda.ComposedWindowLoader(backgrounds, events, pre, batch_size=8, batches_per_epoch=1, seed=1, plan_draws="device")
    feats, targets = next(iter(loader))
    loss, outputs = trainer.step(feats, targets)
    assert np.isfinite(float(loss)) and outputs.shape == (8, 2) and torch.isfinite(outputs).all()
    soft = cda.ComposedWindowLoader(backgrounds, events, pre, batch_size=8, batches_per_epoch=1, seed=1, mixup=cda.MixUp(0.4),
                                    plan_draws="device", draws="device")
    assert np.isfinite(cda.train_epoch_async(trainer, soft, 0)["loss"])
