"""The label audit on the MI355X (cough_detector_amd/audit.py): ``out_of_fold_scores`` against the sequence it stands
for, composed by hand from ``subset``, ``create_data_loaders``, a trainer, ``train_epoch_async``, the eval-mode forward
and a softmax; its determinism; the planted label flips it has to find; the other model types; its refusals; and the
command line.

The corpus (tests/audit_ref.py, ``synth_corpus``): 180 one-second ``synth.make_clip`` clips, 120 non-cough kinds and 60
cough-like bursts, with 12 labels flipped, 6 per class.  One module-scoped audit -- Small, 5 folds x 20 epochs, batch 32,
no augmentation, seed 0: a fold trains on 144 clips, 4 whole batches, so 5 x 20 x 4 = 400 training steps -- is shared
by the tests that read its scores.

Comparisons between two runs on the device are exact: the training kernels use fixed-order reductions and no float
atomics, and the loaders' draws are seeded."""
import json
import os
import random
import struct
import wave

import numpy as np
import pytest
import torch

import audit_ref as R
import cough_detector_amd as cda
from cough_detector_amd import audit, synth
from cough_detector_amd import train as train_mod
from cough_detector_amd.train import preprocessor_config

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "audit_synth.json")
FOLDS, EPOCHS, BATCH = 5, 20, 32


@pytest.fixture(scope="module")
def pre():
    return cda.AudioPreprocessor(device="cuda", **preprocessor_config())


@pytest.fixture(scope="module")
def corpus():
    """(bank, given labels, planted indices); the bank is never written to."""
    seeds, _, given, planted = R.synth_corpus()
    return cda.DeviceClipBank([synth.make_clip(s) for s in seeds], given.tolist()), given, planted


@pytest.fixture(scope="module")
def small_corpus(corpus):
    """48 of the clips, 32 labelled non-cough and 16 labelled cough, for the runs that only have to finish."""
    bank, given, _ = corpus
    keep = np.concatenate([np.flatnonzero(given == 0)[:32], np.flatnonzero(given == 1)[:16]])
    return bank.subset(keep.tolist())


@pytest.fixture(scope="module")
def audited(corpus, pre):
    bank, _, _ = corpus
    return cda.audit_labels(bank, pre, model_type="small", folds=FOLDS, epochs=EPOCHS, batch_size=BATCH, p_augment=0,
                            seed=0)


# ------------------------------------------------------------------------------------------------ equals its parts
def _compose(bank, pre, fold, k, epochs):
    """Fold ``k`` of ``out_of_fold_scores(bank, pre, "small", epochs=epochs, seed=0)``, call by call."""
    random.seed(k)
    np.random.seed(k)
    torch.manual_seed(k)
    train_bank = bank.subset(np.flatnonzero(fold != k).tolist())
    held_bank = bank.subset(np.flatnonzero(fold == k).tolist())
    train_loader, held_loader = cda.create_data_loaders(train_bank, held_bank, pre, batch_size=BATCH,
                                                        use_weighted_sampler=True, draws="host",
                                                        generator=torch.Generator().manual_seed(k))
    model = cda.create_model("small", n_mels=90, num_classes=2, in_channels=1)
    trainer = cda.SmallTrainer(model, lr=1e-3, weight_decay=0.01, seed=k,
                               class_weights=cda.class_weights_from_counts(train_bank.class_counts))
    history = [cda.train_epoch_async(trainer, train_loader, epoch) for epoch in range(epochs)]
    model.eval()
    with torch.no_grad():
        prob = torch.cat([torch.softmax(model(inputs), dim=1) for inputs, _ in held_loader])
    return prob, history


def test_scores_equal_their_parts(corpus, pre, audited, monkeypatch):
    bank, given, _ = corpus
    scores, issues = audited
    n = len(bank)
    assert isinstance(scores, cda.OutOfFoldScores) and isinstance(issues, cda.LabelIssues)
    assert scores.prob.device.type == "cuda" and scores.prob.dtype == torch.float32 and tuple(scores.prob.shape) == (n, 2)
    assert np.array_equal(scores.labels, given) and np.array_equal(scores.fold, R.kfold(given, FOLDS, 42))
    assert scores.config == dict(model_type="small", folds=FOLDS, epochs=EPOCHS, batch_size=BATCH, learning_rate=1e-3,
                                 weight_decay=0.01, p_augment=0, draws="host", seed=0, random_state=42,
                                 scheduler_factory=None)
    assert len(scores.history) == FOLDS and all(len(h) == EPOCHS for h in scores.history)
    assert all(set(e) == {"loss", "accuracy"} and np.isfinite(e["loss"]) for h in scores.history for e in h)
    for k in (1, 4):
        prob, history = _compose(bank, pre, scores.fold, k, EPOCHS)
        rows = torch.from_numpy(np.flatnonzero(scores.fold == k)).to(scores.prob.device)
        assert prob.shape[0] == rows.numel() == 36 and torch.equal(scores.prob[rows], prob), k
        assert scores.history[k] == history, k

    # the clips every fold trains on and the clips it scores: disjoint, together all of them, ascending
    calls = []
    subset = cda.DeviceClipBank.subset

    def spy(self, indices):
        calls.append([int(i) for i in indices])
        return subset(self, indices)

    monkeypatch.setattr(cda.DeviceClipBank, "subset", spy)
    short = cda.out_of_fold_scores(bank, pre, epochs=1, batch_size=BATCH)
    monkeypatch.undo()
    assert len(calls) == 2 * FOLDS
    for k in range(FOLDS):
        train_idx, held_idx = calls[2 * k], calls[2 * k + 1]
        assert not set(train_idx) & set(held_idx) and sorted(train_idx + held_idx) == list(range(n))
        assert train_idx == sorted(train_idx) and held_idx == np.flatnonzero(short.fold == k).tolist()
    assert np.array_equal(short.fold, scores.fold) and bool(torch.isfinite(short.prob).all())


# ------------------------------------------------------------------------------------------------ determinism
def test_a_second_run_repeats_the_first_and_another_seed_does_not(corpus, pre):
    bank, _, _ = corpus
    runs = [cda.out_of_fold_scores(bank, pre, epochs=2, batch_size=BATCH, seed=s) for s in (0, 0, 1)]
    assert torch.equal(runs[0].prob, runs[1].prob) and runs[0].history == runs[1].history
    assert bool(torch.isfinite(runs[0].prob).all())
    assert not torch.equal(runs[0].prob, runs[2].prob)
    assert np.array_equal(runs[0].fold, runs[2].fold)                       # the folds are random_state's, not seed's


# ------------------------------------------------------------------------------------------------ planted flips
def test_the_planted_flips_are_found(audited, corpus):
    """The reference's own ``CoughDetectorSmall`` under torch AdamW on the CPU -- features of oracle.featurizer, the same
    folds, ``WeightedRandomSampler``, batch 32 with the ragged batch dropped, class weights, gradient clip 1.0, lr 1e-3,
    weight decay 0.01, fold k seeded with seed + k; neither the dropout stream nor the sampler's stream is the device
    run's -- gave on this corpus (tests/golden/audit_synth.json):

        10 epochs, seed 0:  9 of 12 planted flips among the suspects, 0 other suspects, 12 in the 24 lowest margins
        10 epochs, seed 1: 11 of 12, 0 others, 12
        20 epochs, seed 0: 12 of 12, 0 others, 12; thresholds (0.770, 0.875), noise rates 0.05 and 0.10
        20 epochs, seed 1: 11 of 12, 0 others, 12; noise rates 0.05 and 0.083
        30 epochs, seed 0: 12 of 12, 0 others, 12
        30 epochs, seed 1: 12 of 12, 2 others, 12
        40 epochs, seed 0: 10 of 12, 0 others, 11
        40 epochs, seed 1: 11 of 12, 2 others, 11

    At the settings and the seed of the audit under test the reference reaches 12 / 12 / 0.  More epochs do not help
    its other seed: from 30 epochs on the model starts to fit the flipped labels.  So 20 epochs stay.  The device run
    of the fixture gave 12 of 12, 0 others, 12, thresholds (0.766, 0.881), noise rates 0.05 and 0.10.

    The planted rates are 6 / 120 of the clips labelled non-cough and 6 / 60 of those labelled cough: flipping 6 labels
    each way leaves the class sizes at 120 and 60.  The issue that set these conditions wrote 6 / 126 and 6 / 54; a
    noise rate has to lie within 0.05 of both pairs of figures, which asks no less than either."""
    scores, issues = audited
    _, given, planted = corpus
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert golden["planted"] == planted.tolist() and golden["given_labels"] == given.tolist()
    assert (golden["settings"]["folds"], golden["settings"]["batch_size"]) == (FOLDS, BATCH)
    at = [r for r in golden["reference_runs"] if (r["epochs"], r["seed"]) == (EPOCHS, 0)]
    assert len(at) == 1 and (at[0]["planted_among_suspects"], at[0]["planted_in_24_lowest_margins"],
                             at[0]["other_suspects"]) == (12, 12, 0)

    planted_set, suspects = set(planted.tolist()), set(issues.index.tolist())
    lowest = set(issues.ranking[:24].tolist())
    m = scores.metrics()
    print("audit: planted among suspects", len(planted_set & suspects), "other suspects", len(suspects - planted_set),
          "planted in the 24 lowest margins", len(planted_set & lowest), "thresholds", issues.thresholds.tolist(),
          "noise_rate", issues.noise_rate, "metrics", m, "reference", at[0])
    assert len(issues.unscored) == 0 and len(issues.ranking) == len(given)
    assert planted_set <= lowest
    assert len(planted_set & suspects) >= 10
    assert len(suspects - planted_set) <= 6
    for j, rates in ((0, (6 / 120, 6 / 126)), (1, (6 / 60, 6 / 54))):
        for rate in rates:
            assert abs(issues.noise_rate[j] - rate) <= 0.05, (j, issues.noise_rate[j], rate)
    assert all(np.isfinite(v) for v in m.values()) and m["tp"] + m["fp"] + m["fn"] + m["tn"] == len(given)
    assert np.array_equal(issues.given, given)


# ------------------------------------------------------------------------------------------------ the other modes
@pytest.mark.parametrize("model_type", ["standard", "residual"])
def test_the_other_model_types_score_every_clip(small_corpus, pre, model_type):
    scores = cda.out_of_fold_scores(small_corpus, pre, model_type=model_type, folds=2, epochs=1, batch_size=8)
    p = scores.prob
    assert tuple(p.shape) == (48, 2) and bool(torch.isfinite(p).all())          # the tensor starts as NaN: all written
    assert float((p.sum(1) - 1.0).abs().max()) <= 1e-6
    assert scores.config["model_type"] == model_type and [len(h) for h in scores.history] == [1, 1]


def test_a_non_finite_clip_is_refused_before_any_training(small_corpus, pre, monkeypatch):
    clips = [small_corpus.clip(k)[0].cpu().clone() for k in range(48)]
    clips[17][1234] = float("nan")
    bank = cda.DeviceClipBank(clips, small_corpus.labels)
    built = []

    def spy(*a, **k):
        built.append(a)
        raise AssertionError("a trainer was constructed")

    for name in train_mod._TRAINERS:
        monkeypatch.setitem(train_mod._TRAINERS, name, spy)
    with pytest.raises(ValueError, match=r"clip\(s\) \[17\] hold non-finite"):
        cda.out_of_fold_scores(bank, pre, folds=2, epochs=1, batch_size=8)
    assert not built


def test_device_draws_with_augmentation_run_to_finite_scores(small_corpus, pre):
    scores = cda.out_of_fold_scores(small_corpus, pre, folds=2, epochs=1, batch_size=8, draws="device", p_augment=0.3)
    assert bool(torch.isfinite(scores.prob).all()) and scores.config["draws"] == "device"
    assert all(np.isfinite(e["loss"]) for h in scores.history for e in h)
    issues = cda.find_label_issues(scores)
    assert len(issues.unscored) == 0 and len(issues.ranking) == 48


# ------------------------------------------------------------------------------------------------ the command line
def _write_wave(path, samples):
    pcm = np.round(np.clip(samples, -1.0, 1.0) * 32767.0).astype(np.int16).tolist()
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(struct.pack(f"<{len(pcm)}h", *pcm))


def test_main_lists_files_by_margin_and_prints_one_json_line(tmp_path, capsys):
    seeds, true, _, _ = R.synth_corpus()
    for cls in ("non_cough", "cough"):
        (tmp_path / cls).mkdir()
    for seed, label in list(zip(seeds, true))[:16] + list(zip(seeds, true))[120:128]:
        _write_wave(tmp_path / ("non_cough", "cough")[label] / f"clip_{seed:03d}.wav", synth.make_clip(seed))
    (tmp_path / "non_cough" / "readme.txt").write_text("not audio")
    report = audit.main([str(tmp_path), "--folds", "2", "--epochs", "2", "--batch-size", "4", "--top", "10", "--seed", "1"])
    lines = capsys.readouterr().out.strip().splitlines()
    printed = json.loads(lines[-1])
    assert printed == json.loads(json.dumps(report))
    assert set(printed) == {"n", "folds", "metrics", "thresholds", "noise_rate", "suspects", "unscored"}
    assert (printed["n"], printed["folds"], printed["unscored"]) == (24, 2, 0) and 0 <= printed["suspects"] <= 24
    assert set(printed["noise_rate"]) == {"0", "1"} and len(printed["thresholds"]) == 2
    assert set(printed["metrics"]) == {"accuracy", "precision", "recall", "f1", "tp", "fp", "fn", "tn"}
    listed = [line.split("\t") for line in lines[:-1]]
    assert len(listed) == 10 and all(len(fields) == 4 for fields in listed)
    files = cda.bank_files(str(tmp_path))
    assert len(files) == 24 and len({fields[0] for fields in listed}) == 10
    for path, given, suggested, _ in listed:
        assert os.path.exists(path) and path in files
        assert given == os.path.basename(os.path.dirname(path)) and suggested in ("non_cough", "cough")
    margins = [float(fields[3]) for fields in listed]
    assert margins == sorted(margins) and all(-1.0 <= v <= 1.0 for v in margins)
