"""The training entry point on the MI355X (cough_detector_amd/train.py): ``train()`` against the sequence it stands for,
composed by hand from ``from_directory``, ``stratified_split``, ``from_esc50``, ``concat``, ``create_data_loaders``, a
trainer and ``fit``; and the bank helpers it adds (``concat``, ``from_esc50``, ``prepare_dataset_split``) against the
per-file calls.

Every comparison is exact.  The banks hold copies of what ``load_audio`` / ``resample`` / ``to_mono`` return, and the
training kernels are deterministic (fixed-order reductions, no float atomics), so two runs with the same seed, or a run
and its hand-composed twin, agree in every weight, every optimizer moment and every metric to the last bit.

The corpus is written by the test: 14 non-cough and 10 cough clips at 16 kHz (0.4-1.6 s) and an ESC-50-shaped tree of
ten 1 s clips at 44.1 kHz over folds 1-5, three of them "coughing".  The split keeps 5 of the 24 for validation, fold
5 adds 2, so training sees 19 + 8 = 27 clips (3 batches of 8) and validation 7, both classes on both sides: the
smallest set that exercises every branch of ``train``."""
import json
import math
import random
import wave

import numpy as np
import pytest
import torch

import cough_detector_amd as cda
from cough_detector_amd import data as cdata
from cough_detector_amd.train import main, preprocessor_config, train

pytestmark = pytest.mark.gpu
SEED = 3
# (filename, fold, target): two files per fold; fold 5 (validation) holds one cough and one negative
ESC_ROWS = [("1-100-A-24.wav", 1, 24), ("1-101-A-0.wav", 1, 0), ("2-102-A-20.wav", 2, 20), ("2-103-A-24.wav", 2, 24),
            ("3-104-A-38.wav", 3, 38), ("3-105-A-0.wav", 3, 0), ("4-106-A-21.wav", 4, 21), ("4-107-A-10.wav", 4, 10),
            ("5-108-A-24.wav", 5, 24), ("5-109-A-5.wav", 5, 5)]


def _clip(g, n, cough):
    """Seeded noise; a cough clip carries three decaying bursts."""
    x = g.normal(0.0, 0.05, n)
    if cough:
        for start in g.randint(0, max(n - 800, 1), 3):
            m = min(800, n - start)
            x[start:start + m] += g.normal(0.0, 0.5, m) * np.exp(-np.arange(m) / 200.0)
    return np.clip(x, -0.99, 0.99)


def _write_wave(path, samples, rate):
    pcm = np.round(samples * 32767.0).astype("<i2")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1 if pcm.ndim == 1 else pcm.shape[1])
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(pcm.tobytes())


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    root = tmp_path_factory.mktemp("train_entry")
    g = np.random.RandomState(11)
    for cls, count in (("non_cough", 14), ("cough", 10)):
        (root / "data" / cls).mkdir(parents=True)
        for k in range(count):
            n = int(g.randint(6400, 25601))                                    # 0.4-1.6 s
            _write_wave(root / "data" / cls / f"{cls}_{k:02d}.wav", _clip(g, n, cls == "cough"), 16000)
    esc = root / "datasets" / "ESC-50-master"
    (esc / "meta").mkdir(parents=True)
    (esc / "audio").mkdir()
    lines = ["filename,fold,target,category,esc10,src_file,take"]
    for k, (name, fold, target) in enumerate(ESC_ROWS):
        lines.append(f"{name},{fold},{target},class{target},False,{100 + k},A")
        x = _clip(g, 44100, target == 24)
        if k == 2:                                                             # one stereo file: to_mono has work to do
            x = np.stack([x, _clip(g, 44100, False)], axis=1)
        _write_wave(esc / "audio" / name, x, 44100)
    (esc / "meta" / "esc50.csv").write_text("\n".join(lines) + "\n")
    return root


@pytest.fixture(scope="module")
def pre():
    return cda.AudioPreprocessor(device="cuda", **preprocessor_config())


def _same_bank(a, b):
    for name in ("data", "lengths", "offsets", "labels", "offsets_dev", "lengths_dev", "labels_dev"):
        u, v = getattr(a, name), getattr(b, name)
        assert u.dtype == v.dtype and u.device == v.device and torch.equal(u, v), name


def _run(corpus, out, **kw):
    kw.setdefault("model_type", "small")
    kw.setdefault("epochs", 2)
    return train(str(corpus / "data"), str(out), batch_size=8, use_esc50=True,
                 esc50_dir=str(corpus / "datasets" / "ESC-50-master"), seed=SEED, **kw)


@pytest.fixture(scope="module")
def trained(corpus):
    """One seeded ``train()`` of two epochs, shared by the tests that read its outputs."""
    out = corpus / "out1"
    best = _run(corpus, out, learning_rate=2e-3, weight_decay=0.05, patience=4)
    return out, best


def _checkpoint(path):
    return torch.load(str(path), map_location="cpu", weights_only=False)


def _same_checkpoint(a, b):
    assert a["epoch"] == b["epoch"] and a["metrics"] == b["metrics"] and a["config"] == b["config"]
    assert a["trainer_state"] == b["trainer_state"]
    assert list(a["model_state_dict"]) == list(b["model_state_dict"])
    for k, v in a["model_state_dict"].items():
        assert torch.equal(v, b["model_state_dict"][k]), k
    sa, sb = a["optimizer_state_dict"], b["optimizer_state_dict"]
    assert sa["param_groups"] == sb["param_groups"] and sorted(sa["state"]) == sorted(sb["state"]) and sa["state"]
    for i, entry in sa["state"].items():
        assert set(entry) == set(sb["state"][i]) == {"step", "exp_avg", "exp_avg_sq"}
        for k, v in entry.items():
            assert torch.equal(torch.as_tensor(v), torch.as_tensor(sb["state"][i][k])), (i, k)


# ------------------------------------------------------------------------------------------------ the banks
def test_from_esc50_equals_the_per_file_calls(corpus, pre):
    esc = corpus / "datasets" / "ESC-50-master"
    for key in ((True, 5, True), (False, 5, True), (True, None, False)):
        rows = cdata.esc50_rows(esc / "meta" / "esc50.csv", *key)
        bank = cda.DeviceClipBank.from_esc50(str(esc), pre, *key)
        assert bank.data.device.type == "cuda" and bank.labels.tolist() == [v for _, v in rows]
        assert bank.lengths.tolist() == [math.ceil(44100 * 160 / 441)] * len(rows) == [16000] * len(rows)
        for k, (name, _) in enumerate(rows):
            waveform, sr = pre.load_audio(str(esc / "audio" / name))
            assert sr == 44100 and waveform.shape == ((2 if name == ESC_ROWS[2][0] else 1), 44100)
            want = pre.to_mono(pre.resample(waveform, sr))
            assert tuple(want.shape) == (1, 16000) and torch.equal(bank.clip(k), want.to(bank.device)), name
    train_rows = cdata.esc50_rows(esc / "meta" / "esc50.csv", True, 5, True)
    assert [n for n, _ in train_rows] == [r[0] for r in ESC_ROWS[:8]] and sum(v for _, v in train_rows) == 2
    assert cdata.esc50_rows(esc / "meta" / "esc50.csv", False, 5, True) == [(ESC_ROWS[8][0], 1), (ESC_ROWS[9][0], 0)]
    assert len(cdata.esc50_rows(esc / "meta" / "esc50.csv", True, None, False)) == 6   # targets 0, 10 and 5 are dropped


def test_concat_equals_a_bank_of_the_concatenated_clips():
    g = torch.Generator().manual_seed(4)
    groups = [([5, 1, 16001], [0, 1, 0]), ([7], [1]), ([], []), ([3, 40001, 16000], [1, 1, 0])]
    clips = [[torch.randn(n, generator=g) for n in lengths] for lengths, _ in groups]
    banks = [cda.DeviceClipBank(c, labels) for c, (_, labels) in zip(clips, groups)]
    got = cda.DeviceClipBank.concat(banks)
    want = cda.DeviceClipBank([c for part in clips for c in part], [v for _, labels in groups for v in labels])
    _same_bank(got, want)
    assert got.data.device.type == "cuda" and got.device == banks[0].device and len(got) == 7
    assert got.class_counts == {k: sum(b.class_counts[k] for b in banks) for k in (0, 1)} == {0: 3, 1: 4}
    for k in range(7):
        assert torch.equal(got.clip(k), want.clip(k))
    assert len(cda.DeviceClipBank.concat([])) == 0 and cda.DeviceClipBank.concat([]).data.device.type == "cuda"
    with pytest.raises(ValueError, match="share one device"):
        cda.DeviceClipBank.concat([banks[0], cda.DeviceClipBank(clips[1], [1], device="cpu")])


def test_prepare_dataset_split_equals_subset_of_the_split(corpus, pre):
    bank = cda.DeviceClipBank.from_directory(str(corpus / "data"), pre)
    assert len(bank) == 24 and bank.class_counts == {0: 14, 1: 10} and bank.data.device.type == "cuda"
    assert 6400 <= min(bank.lengths.tolist()) and max(bank.lengths.tolist()) <= 25600
    train_idx, val_idx = cda.stratified_split(bank.labels)
    assert len(train_idx) == 19 and len(val_idx) == 5
    for source in (str(corpus / "data"), bank):
        train_bank, val_bank = cda.prepare_dataset_split(source, pre)
        _same_bank(train_bank, bank.subset(train_idx))
        _same_bank(val_bank, bank.subset(val_idx))
        assert min(train_bank.class_counts.values()) >= 1 and min(val_bank.class_counts.values()) >= 1
    other, _ = cda.prepare_dataset_split(bank, val_split=0.25, random_state=7)
    _same_bank(other, bank.subset(cda.stratified_split(bank.labels, 0.25, 7)[0]))


# ------------------------------------------------------------------------------------------------ train() and its parts
def _compose(corpus, out, lr, weight_decay, patience, epochs=2):
    """What ``train(data, out, "small", epochs, 8, lr, weight_decay, patience, seed=SEED)`` stands for, call by call."""
    cfg = preprocessor_config()
    pre = cda.AudioPreprocessor(device="cuda", **cfg)
    audio = cda.AudioAugmentor(sample_rate=16000, p_augment=0.3)
    spec = cda.SpecAugment(freq_mask_param=8, time_mask_param=15, n_freq_masks=2, n_time_masks=2, p=0.3)
    bank = cda.DeviceClipBank.from_directory(str(corpus / "data"), pre)
    train_idx, val_idx = cda.stratified_split(bank.labels, val_split=0.2, random_state=42)
    esc = str(corpus / "datasets" / "ESC-50-master")
    esc_train = cda.DeviceClipBank.from_esc50(esc, pre, is_training=True, fold=5)
    esc_val = cda.DeviceClipBank.from_esc50(esc, pre, is_training=False, fold=5)
    train_bank = cda.DeviceClipBank.concat([bank.subset(train_idx), esc_train])
    val_bank = cda.DeviceClipBank.concat([bank.subset(val_idx), esc_val])
    random.seed(SEED)
    np.random.seed(SEED)
    torch.manual_seed(SEED)
    train_loader, val_loader = cda.create_data_loaders(train_bank, val_bank, pre, batch_size=8, use_weighted_sampler=True,
                                                       audio_augmentor=audio, spec_augmentor=spec, draws="host",
                                                       generator=torch.Generator().manual_seed(SEED))
    model = cda.create_model("small", n_mels=90, num_classes=2, in_channels=1)
    trainer = cda.SmallTrainer(model, lr=lr, weight_decay=weight_decay, seed=SEED,
                               class_weights=cda.class_weights_from_counts(train_bank.class_counts))
    config = dict(model_type="small", **cfg, batch_size=8, learning_rate=lr, weight_decay=weight_decay, epochs=epochs,
                  patience=patience)
    return (len(train_bank), len(val_bank), train_bank.class_counts), cda.fit(
        trainer, train_loader, val_loader, str(out), epochs=epochs, patience=patience, config=config)


def test_train_equals_its_parts(corpus, trained):
    out1, best = trained
    assert best == str(out1 / "best_model.pt")
    sizes, res = _compose(corpus, corpus / "parts", lr=2e-3, weight_decay=0.05, patience=4)
    assert sizes == (27, 7, {0: 17, 1: 10})                  # 11 + 8 of the 24 and 6 + 2 of folds 1-4
    history = json.loads((out1 / "history.json").read_text())
    print("train() history:", json.dumps(history))
    assert history == res["history"] and len(history) == res["epochs_run"] == 2
    for h in history:
        assert np.isfinite(h["train"]["loss"]) and np.isfinite(h["val"]["loss"])
        assert h["val"]["tp"] + h["val"]["fp"] + h["val"]["fn"] + h["val"]["tn"] == 7
    assert history[0] != history[1]
    _same_checkpoint(_checkpoint(out1 / "latest_model.pt"), _checkpoint(corpus / "parts" / "latest_model.pt"))
    assert json.loads((out1 / "config.json").read_text()) == json.loads((corpus / "parts" / "config.json").read_text())
    assert (out1 / "best_model.pt").exists() == (corpus / "parts" / "best_model.pt").exists() == (res["best_f1"] > 0)


def test_a_second_seeded_run_repeats_the_first(corpus, trained):
    out1, _ = trained
    out2 = corpus / "out2"
    _run(corpus, out2, learning_rate=2e-3, weight_decay=0.05, patience=4)
    assert json.loads((out2 / "history.json").read_text()) == json.loads((out1 / "history.json").read_text())
    _same_checkpoint(_checkpoint(out1 / "latest_model.pt"), _checkpoint(out2 / "latest_model.pt"))
    ck = _checkpoint(out2 / "latest_model.pt")
    assert ck["epoch"] == 1 and ck["trainer_state"] == {"seed": SEED, "draws": 6}     # 3 batches of 8 per epoch


def test_outputs_hold_what_was_passed(trained):
    out1, _ = trained
    config = json.loads((out1 / "config.json").read_text())
    assert config == dict(model_type="small", **preprocessor_config(), batch_size=8, learning_rate=2e-3, weight_decay=0.05,
                          epochs=2, patience=4)
    assert _checkpoint(out1 / "latest_model.pt")["config"] == config
    history = json.loads((out1 / "history.json").read_text())
    assert [h["epoch"] for h in history] == [0, 1] and all(set(h) == {"epoch", "train", "val"} for h in history)


def test_resume_runs_exactly_the_epochs_that_are_left(corpus, trained):
    out1, _ = trained
    out3 = corpus / "out3"
    _run(corpus, out3, epochs=3, resume=str(out1 / "latest_model.pt"), learning_rate=2e-3, weight_decay=0.05, patience=4)
    history = json.loads((out3 / "history.json").read_text())
    assert [h["epoch"] for h in history] == [2]
    ck = _checkpoint(out3 / "latest_model.pt")
    assert ck["epoch"] == 2 and ck["trainer_state"] == {"seed": SEED, "draws": 9}
    assert ck["optimizer_state_dict"]["state"][0]["step"].item() == 9
    assert json.loads((out3 / "config.json").read_text())["epochs"] == 3


# ------------------------------------------------------------------------------------------------ the other modes
def _scores_a_window(path, model_type):
    engine = cda.CoughDetectorInference(str(path), verbose=False)
    assert engine.config["model_type"] == model_type and type(engine.model).__name__ == \
        {"small": "CoughDetectorSmall", "standard": "CoughDetector", "residual": "CoughDetectorResidual"}[model_type]
    window = torch.from_numpy(_clip(np.random.RandomState(2), 16000, True).astype(np.float32)).cuda().unsqueeze(0)
    feats = engine.preprocessor.featurize_batch(window, normalize=True)
    assert tuple(feats.shape) == (1, 90, 101)
    is_cough, confidence = engine.predict(feats)
    assert 0.0 <= confidence <= 1.0 and is_cough == (confidence > 0.5)


def test_device_draws_run_to_a_finite_loss(corpus):
    out = corpus / "out_drawn"
    _run(corpus, out, draws="device")
    history = json.loads((out / "history.json").read_text())
    assert len(history) == 2
    assert all(np.isfinite(h["train"]["loss"]) and np.isfinite(h["val"]["loss"]) for h in history)
    _scores_a_window(out / "latest_model.pt", "small")


@pytest.mark.parametrize("model_type", ["standard", "residual"])
def test_the_other_model_types_train_and_load(corpus, model_type):
    out = corpus / f"out_{model_type}"
    best = _run(corpus, out, model_type=model_type, epochs=1)
    assert best == str(out / "best_model.pt")
    assert json.loads((out / "config.json").read_text())["model_type"] == model_type
    history = json.loads((out / "history.json").read_text())
    assert len(history) == 1 and np.isfinite(history[0]["train"]["loss"]) and np.isfinite(history[0]["val"]["loss"])
    ck = _checkpoint(out / "latest_model.pt")
    assert ck["config"]["model_type"] == model_type and ck["epoch"] == 0
    _scores_a_window(out / "latest_model.pt", model_type)


def test_refusals_on_the_device(corpus, tmp_path):
    with pytest.raises(FileNotFoundError, match="esc50.csv"):                  # nothing is downloaded
        train(str(corpus / "data"), str(tmp_path / "o"), epochs=1, batch_size=8, esc50_dir=str(tmp_path / "no-esc50"))
    with pytest.raises(ValueError, match="draws"):
        train(str(corpus / "data"), str(tmp_path / "o"), epochs=1, batch_size=8, use_esc50=False, draws="gpu")


# ------------------------------------------------------------------------------------------------ the command line
def test_main_prints_one_json_line(corpus, capsys):
    out = corpus / "out_cli"
    report = main(["--data-dir", str(corpus / "data"), "--output-dir", str(out), "--epochs", "1", "--batch-size", "8",
                   "--seed", str(SEED), "--no-esc50", "--num-workers", "0"])
    line = capsys.readouterr().out.strip().splitlines()[-1]
    printed = json.loads(line)
    assert printed == report and set(printed) == {"best_model", "best_f1", "epochs_run"}
    assert printed["epochs_run"] == 1 and 0.0 <= printed["best_f1"] <= 1.0
    best = printed["best_model"]
    assert best == str(out / "best_model.pt") and (out / "latest_model.pt").exists() and (out / "history.json").exists()
    config = json.loads((out / "config.json").read_text())
    assert (config["epochs"], config["batch_size"], config["learning_rate"], config["patience"]) == (1, 8, 0.001, 15)
    assert _checkpoint(out / "latest_model.pt")["trainer_state"] == {"seed": SEED, "draws": 2}    # 19 clips: 2 batches of 8
