"""``train_windows`` on the MI355X: synthetic banks made here (6 backgrounds of 3 s, 12 bursts labelled 1, 6 labelled 0),
two epochs of four batches of eight on Small, four held-out scenes of 5 s.  What is checked: the files it writes, that
the checkpoint loads, that a seeded run repeats itself bit for bit and equals the same sequence composed by hand, and the
command line on directories of WAVE files."""
import json
import os
import random

import numpy as np
import pytest
import torch

import cough_detector_amd as cda
from cough_detector_amd import windows as cwin
from cough_detector_amd.train import preprocessor_config

pytestmark = pytest.mark.gpu
SR = 16000
RUN = dict(model_type="small", epochs=2, batch_size=8, batches_per_epoch=4, val_scenes=4, scene_seconds=5.0)


def _clips():
    rng = np.random.default_rng(31)
    t = np.arange(int(0.3 * SR)) / SR
    backgrounds = [(rng.standard_normal(3 * SR) * 0.02).astype(np.float32) for _ in range(6)]
    coughs = [(rng.standard_normal(t.size) * np.hanning(t.size) * 0.5).astype(np.float32) for _ in range(12)]       # noise bursts
    others = [(np.sin(2 * np.pi * (300 + 90 * k) * t) * np.hanning(t.size) * 0.5).astype(np.float32) for k in range(6)]    # tone bursts
    return backgrounds, coughs, others


@pytest.fixture(scope="module")
def banks():
    backgrounds, coughs, others = _clips()
    return (cda.DeviceClipBank([torch.from_numpy(x) for x in backgrounds], [0] * 6),
            cda.DeviceClipBank([torch.from_numpy(x) for x in coughs + others], [1] * 12 + [0] * 6))


@pytest.fixture(scope="module")
def first_run(banks, tmp_path_factory):
    out = tmp_path_factory.mktemp("windows_a")
    best = cda.train_windows(banks[0], banks[1], str(out), **RUN)
    return out, best


def _weights(path):
    return torch.load(path, map_location="cpu", weights_only=False)["model_state_dict"]


def test_it_writes_its_files_and_the_checkpoint_loads(first_run):
    out, best = first_run
    assert best == str(out / "best_model.pt")
    for f in ("config.json", "latest_model.pt", "history.json"):
        assert (out / f).exists(), f
    config, history = json.load(open(out / "config.json")), json.load(open(out / "history.json"))
    assert config["model_type"] == "small" and all(config[k] == v for k, v in preprocessor_config().items())
    assert config["windows"]["plan_draws"] == config["windows"]["draws"] == "device" and config["windows"]["batches_per_epoch"] == 4
    assert config["windows"]["seed"] == 0 and config["windows"]["p_cough"] == 0.5 and config["batch_size"] == 8
    assert [h["epoch"] for h in history] == [0, 1] and all(np.isfinite(h["train"]["loss"]) and np.isfinite(h["val"]["loss"]) for h in history)
    reached = max(h["val"]["f1"] for h in history) > 0
    assert (out / "best_model.pt").exists() == reached == (out / "events.json").exists()
    engine = cda.CoughDetectorInference(str(out / ("best_model.pt" if reached else "latest_model.pt")), verbose=False)
    assert engine.config["windows"]["val_scenes"] == 4
    if reached:
        report = json.load(open(out / "events.json"))
        assert set(report["pick"]) == {"threshold", "index", "recall", "false_alarms_per_minute", "meets_recall"}
        assert len(report["thresholds"]) == 101 and report["recordings"] == 4 and 12 <= report["truth_events"] <= 24


def test_a_second_run_repeats_the_first_bit_for_bit(banks, first_run, tmp_path):
    out, _ = first_run
    cda.train_windows(banks[0], banks[1], str(tmp_path), **RUN)
    assert json.load(open(tmp_path / "history.json")) == json.load(open(out / "history.json"))
    a, b = _weights(out / "latest_model.pt"), _weights(tmp_path / "latest_model.pt")
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    other = tmp_path / "other"
    cda.train_windows(banks[0], banks[1], str(other), seed=1, **RUN)
    assert json.load(open(other / "history.json")) != json.load(open(out / "history.json"))


def test_the_sequence_composed_by_hand_gives_the_same_history(banks, first_run, tmp_path):
    out, _ = first_run
    pre = cda.AudioPreprocessor(device="cuda", **preprocessor_config())
    train_bg, train_ev, held_bg, held_coughs = cwin.window_split(banks[0], banks[1], 0.2, 42)
    assert (len(train_bg), len(held_bg), len(held_coughs)) == (4, 2, 3) and train_ev.labels.tolist().count(1) == 9
    random.seed(0)
    np.random.seed(0)
    torch.manual_seed(0)
    loader = cda.ComposedWindowLoader(train_bg, train_ev, pre, batch_size=8, batches_per_epoch=4, seed=0,
                                      audio_augmentor=cda.AudioAugmentor(sample_rate=SR, p_augment=0.3),
                                      spec_augmentor=cda.SpecAugment(8, 15, 2, 2, 0.3), draws="device", plan_draws="device")
    plan = cda.draw_scene_plan(held_bg, held_coughs, 4, 5.0, events_per_scene=(3, 6), snr_range=(5, 20), seed=1, sample_rate=SR)
    scenes, truth = cda.compose_scenes(held_bg, held_coughs, plan)
    val_bank, _ = cda.scene_window_bank(scenes, truth, pre)
    val_loader = cda.DeviceDataLoader(val_bank, pre, batch_size=8, is_training=False)
    model = cda.create_model("small", n_mels=pre.get_num_features(), num_classes=2, in_channels=1)
    trainer = cda.SmallTrainer(model, lr=1e-3, weight_decay=0.01, class_weights=cda.class_weights_from_counts({0: 16, 1: 16}), seed=0)
    result = cda.fit(trainer, loader, val_loader, str(tmp_path), epochs=2, patience=15,
                     config=dict(model_type="small", **preprocessor_config()))
    assert json.loads(json.dumps(result["history"])) == json.load(open(out / "history.json"))
    a, b = _weights(out / "latest_model.pt"), _weights(tmp_path / "latest_model.pt")
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_the_command_line_trains_from_directories(tmp_path, capsys):
    backgrounds, coughs, others = _clips()
    bank = lambda clips, label: cda.DeviceClipBank([torch.from_numpy(x) for x in clips], [label] * len(clips))
    cda.write_clips(bank(backgrounds, 0), str(tmp_path / "bg"), [f"bg_{k}" for k in range(6)], sample_rate=SR)
    cda.write_clips(bank(coughs, 1), str(tmp_path / "ev"), [f"c_{k}" for k in range(12)], sample_rate=SR)
    cda.write_clips(bank(others, 0), str(tmp_path / "ev"), [f"o_{k}" for k in range(6)], sample_rate=SR)
    out = tmp_path / "out"
    report = cwin.main([str(tmp_path / "bg" / "non_cough"), str(tmp_path / "ev"), "--output-dir", str(out), "--model-type", "small",
                        "--epochs", "2", "--batch-size", "8", "--batches-per-epoch", "4", "--val-scenes", "4", "--seconds", "5"])
    last = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert last == report and set(last) == {"best_model", "best_f1", "epochs_run", "pick"} and last["epochs_run"] == 2
    assert last["best_model"] == str(out / "best_model.pt") and (last["pick"] is not None) == os.path.exists(last["best_model"])
    for f in ("config.json", "latest_model.pt", "history.json"):
        assert (out / f).exists(), f
    assert json.load(open(out / "config.json"))["windows"]["events_per_scene"] == [3, 6]
    # an event directory without non_cough/ trains too (no distractors), one without a cough does not
    os.rename(tmp_path / "ev" / "non_cough", tmp_path / "elsewhere")
    best = cda.train_windows(str(tmp_path / "bg" / "non_cough"), str(tmp_path / "ev"), str(tmp_path / "out2"), **dict(RUN, epochs=1))
    assert os.path.exists(tmp_path / "out2" / "latest_model.pt") and best.endswith("best_model.pt")


def test_a_side_without_a_cough_raises(banks, tmp_path):
    backgrounds, events = banks
    with pytest.raises(ValueError, match="held-out side without a cough"):
        cda.train_windows(backgrounds, events.subset(range(12, 18)), str(tmp_path), **RUN)
    with pytest.raises(ValueError, match="training side without a cough"):
        cda.train_windows(backgrounds, events.subset([0, 12, 13]), str(tmp_path), **RUN)
    with pytest.raises(ValueError, match="without a background"):
        cda.train_windows(backgrounds.subset([0]), events, str(tmp_path), **RUN)
    assert not list(tmp_path.iterdir())
