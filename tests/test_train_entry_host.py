"""The training entry point without a GPU (cough_detector_amd/train.py and the split / ESC-50 / concat additions of
cough_detector_amd/data.py): ``stratified_split`` against results recorded from scikit-learn's ``train_test_split``
(tests/golden/stratified_split.json) and, where scikit-learn is installed, against it live; the ESC-50 row selection
against hand-written expectations; the command line's defaults; what ``train`` refuses before it touches a device; and
the bank-level helpers on CPU banks."""
import inspect
import json
import math
import os
import wave

import numpy as np
import pytest
import torch

import cough_detector_amd as cda
from cough_detector_amd import data as cdata

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stratified_split.json")
SHIPPED = dict(use_pcen=False, use_pre_emphasis=False, use_delta_delta=False, use_spectral_contrast=False)


def _cases():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


# ------------------------------------------------------------------------------------------------ stratified_split
def test_golden_file_covers_the_sizes_and_stays_small():
    cases = _cases()
    assert os.path.getsize(GOLDEN) < 100 * 1024
    assert {c["n"] for c in cases} == {5, 10, 11, 37, 100, 333}
    assert {c["val_split"] for c in cases} == {0.1, 0.2, 0.25, 0.33} and {c["random_state"] for c in cases} == {0, 7, 42}
    assert sum("refused" not in c for c in cases) >= 40 and any("refused" in c for c in cases)


@pytest.mark.parametrize("k", range(len(_cases())))
def test_stratified_split_equals_the_recorded_sklearn_result(k):
    c = _cases()[k]
    if "refused" in c:
        with pytest.raises(ValueError):
            cda.stratified_split(c["labels"], c["val_split"], c["random_state"])
        return
    train, val = cda.stratified_split(c["labels"], val_split=c["val_split"], random_state=c["random_state"])
    assert train == c["train"] and val == c["val"], (c["n"], c["mix"], c["val_split"], c["random_state"])
    assert all(type(i) is int for i in train + val)
    # a label tensor (what a bank holds) gives the same lists
    assert cda.stratified_split(torch.tensor(c["labels"]), c["val_split"], c["random_state"]) == (train, val)


def test_stratified_split_equals_sklearn_live():
    sk = pytest.importorskip("sklearn.model_selection")
    checked = 0
    for n in (5, 8, 13, 50, 257, 1000, 8220):
        for share in (0.1, 0.37, 0.5):
            k = max(1, int(round(share * n)))
            labels = [0] * (n - k) + [1] * k
            for split in (0.1, 0.2, 0.25, 0.33):
                for seed in (0, 7, 42):
                    try:
                        want = sk.train_test_split(list(range(n)), test_size=split, random_state=seed, stratify=labels)
                    except ValueError:
                        with pytest.raises(ValueError):
                            cda.stratified_split(labels, split, seed)
                        continue
                    assert cda.stratified_split(labels, split, seed) == (list(want[0]), list(want[1])), (n, share, split, seed)
                    checked += 1
    assert checked > 150


@pytest.mark.parametrize("n,k,split", [(10, 3, 0.2), (11, 4, 0.25), (24, 10, 0.2), (37, 5, 0.33), (333, 111, 0.1),
                                       (1000, 101, 0.2)])
def test_stratified_split_properties(n, k, split):
    labels = np.array([0] * (n - k) + [1] * k)
    for seed in (0, 42):
        train, val = cda.stratified_split(labels, split, seed)
        assert not set(train) & set(val)
        assert sorted(train + val) == list(range(n))
        assert len(val) == math.ceil(split * n) and len(train) == n - len(val)
        for cls, count in ((0, n - k), (1, k)):
            for side in (train, val):
                assert abs(int((labels[side] == cls).sum()) - count * len(side) / n) <= 1.0, (seed, cls)
        assert (train, val) == cda.stratified_split(labels, split, seed)               # no hidden state
    assert cda.stratified_split(labels, split, 0) != cda.stratified_split(labels, split, 42)


def test_stratified_split_defaults_are_the_references():
    p = inspect.signature(cda.stratified_split).parameters
    assert p["val_split"].default == 0.2 and p["random_state"].default == 42
    labels = [0] * 14 + [1] * 10
    assert cda.stratified_split(labels) == cda.stratified_split(labels, 0.2, 42)


def test_stratified_split_refuses_what_sklearn_refuses():
    with pytest.raises(ValueError, match="single member"):
        cda.stratified_split([0, 0, 0, 0, 1], 0.4)
    with pytest.raises(ValueError, match="validation side"):                   # ceil(0.2 * 5) = 1 clip for 2 classes
        cda.stratified_split([0, 0, 0, 1, 1], 0.2)
    with pytest.raises(ValueError, match="training side"):                     # 10 - ceil(0.95 * 10) = 0
        cda.stratified_split([0] * 5 + [1] * 5, 0.95)
    with pytest.raises(ValueError, match="training side"):                     # 1 clip for 2 classes
        cda.stratified_split([0] * 5 + [1] * 5, 0.9)
    for bad in (0.0, 1.0, -0.2, 1.5, 2, None):
        with pytest.raises(ValueError, match="val_split"):
            cda.stratified_split([0] * 5 + [1] * 5, bad)
    with pytest.raises(ValueError):
        cda.stratified_split([], 0.2)
    with pytest.raises(ValueError, match="one-dimensional"):
        cda.stratified_split([[0, 1], [1, 0]], 0.5)


# ------------------------------------------------------------------------------------------------ ESC-50 rows
ESC_ROWS = [("a.wav", 1, 24), ("b.wav", 1, 0), ("c.wav", 2, 20), ("d.wav", 2, 24), ("e.wav", 3, 38), ("f.wav", 3, 0),
            ("g.wav", 4, 24), ("h.wav", 4, 20), ("i.wav", 5, 24), ("j.wav", 5, 0), ("k.wav", 5, 38), ("l.wav", 5, 20)]
MISSING = "g.wav"
# (is_training, fold, include_all_negatives) -> "<name><label>" in csv order; without a fold is_training changes nothing
ESC_WANT = {
    (True, None, True): "a1 b0 c0 d1 e0 f0 h0 i1 j0 k0 l0", (False, None, True): "a1 b0 c0 d1 e0 f0 h0 i1 j0 k0 l0",
    (True, None, False): "a1 c0 d1 e0 h0 i1 k0 l0", (False, None, False): "a1 c0 d1 e0 h0 i1 k0 l0",
    (True, 5, True): "a1 b0 c0 d1 e0 f0 h0", (True, 5, False): "a1 c0 d1 e0 h0",
    (False, 5, True): "i1 j0 k0 l0", (False, 5, False): "i1 k0 l0",
    (True, 2, True): "a1 b0 e0 f0 h0 i1 j0 k0 l0", (False, 2, False): "c0 d1",
}


def _write_wave(path, samples, rate=16000, channels=1):
    """16-bit PCM; ``samples`` float in [-1, 1): (n,) or (n, channels)."""
    pcm = np.clip(np.round(np.asarray(samples) * 32768.0), -32768, 32767).astype("<i2")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(pcm.tobytes())
    return pcm.astype(np.float32) / 32768.0


def _esc_tree(root, audio=None):
    """An ESC-50-shaped checkout of ``ESC_ROWS`` with the real csv's columns; ``audio(name)`` gives a file's samples
    (default: a few bytes that are no audio -- row selection only looks at whether the file exists)."""
    (root / "meta").mkdir(parents=True)
    (root / "audio").mkdir()
    lines = ["filename,fold,target,category,esc10,src_file,take"]
    lines += [f"{name},{fold},{target},cat{target},False,{100 + k},A" for k, (name, fold, target) in enumerate(ESC_ROWS)]
    (root / "meta" / "esc50.csv").write_text("\n".join(lines) + "\n")
    kept = {}
    for name, _, _ in ESC_ROWS:
        if name == MISSING:
            continue
        if audio is None:
            (root / "audio" / name).write_bytes(b"RIFF")
        else:
            kept[name] = _write_wave(root / "audio" / name, audio(name))
    return root / "meta" / "esc50.csv", kept


@pytest.mark.parametrize("key", sorted(ESC_WANT, key=str))
def test_esc50_rows_follow_the_reference_rule(key, tmp_path):
    csv_path, _ = _esc_tree(tmp_path / "esc")
    is_training, fold, include_all = key
    want = [(w[0] + ".wav", int(w[1])) for w in ESC_WANT[key].split()]
    assert cdata.esc50_rows(csv_path, is_training, fold, include_all) == want
    assert cdata.esc50_rows(str(csv_path), is_training=is_training, fold=fold, include_all_negatives=include_all) == want
    assert all(name != MISSING for name, _ in want)


def test_esc50_constants_and_missing_csv(tmp_path):
    assert cdata.ESC50_NEGATIVE_CLASSES == (20, 21, 22, 23, 25, 26, 38) and cdata.ESC50_COUGH_CLASS == 24
    p = inspect.signature(cdata.esc50_rows).parameters
    assert (p["is_training"].default, p["fold"].default, p["include_all_negatives"].default) == (True, None, True)
    missing = tmp_path / "nowhere" / "meta" / "esc50.csv"
    with pytest.raises(FileNotFoundError) as e:
        cdata.esc50_rows(missing)
    assert str(missing) in str(e.value) and "ESC-50" in str(e.value)
    with pytest.raises(FileNotFoundError, match="esc50.csv"):
        cda.DeviceClipBank.from_esc50(str(tmp_path / "nowhere"), cda.AudioPreprocessor(**SHIPPED), device="cpu")
    assert not hasattr(cdata, "download_esc50")


def test_from_esc50_on_a_cpu_bank_at_the_native_rate(tmp_path):
    """16 kHz mono files need neither ``cough_resample`` nor the mono kernel: the bank's bookkeeping without a GPU."""
    g = np.random.RandomState(3)
    _, kept = _esc_tree(tmp_path / "esc", audio=lambda name: g.uniform(-0.5, 0.5, 200 + 37 * (ord(name[0]) - 96)))
    pre = cda.AudioPreprocessor(**SHIPPED)
    for key in ((True, 5, True), (False, 5, True), (True, None, False)):
        bank = cda.DeviceClipBank.from_esc50(str(tmp_path / "esc"), pre, *key, device="cpu")
        want = [(w[0] + ".wav", int(w[1])) for w in ESC_WANT[key].split()]
        assert bank.labels.tolist() == [v for _, v in want] and bank.lengths.tolist() == [len(kept[n]) for n, _ in want]
        for k, (name, _) in enumerate(want):
            assert torch.equal(bank.clip(k)[0], torch.from_numpy(kept[name])), name


# ------------------------------------------------------------------------------------------------ concat, split of a bank
def _cpu_bank(lengths, labels, seed):
    g = torch.Generator().manual_seed(seed)
    clips = [torch.randn(n, generator=g) for n in lengths]
    return cda.DeviceClipBank(clips, labels, device="cpu"), clips


def test_concat_equals_a_bank_of_the_concatenated_lists():
    a, ca = _cpu_bank([5, 1, 16001], [0, 1, 0], 1)
    b, cb = _cpu_bank([7], [1], 2)
    e, _ = _cpu_bank([], [], 3)
    c, cc = _cpu_bank([3, 40001], [1, 1], 4)
    got = cda.DeviceClipBank.concat([a, b, e, c])
    want = cda.DeviceClipBank(ca + cb + cc, [0, 1, 0, 1, 1, 1], device="cpu")
    for name in ("data", "lengths", "offsets", "labels", "offsets_dev", "lengths_dev", "labels_dev"):
        assert torch.equal(getattr(got, name), getattr(want, name)) and getattr(got, name).dtype == getattr(want, name).dtype
    assert got.device == a.device and len(got) == 6
    assert got.class_counts == {0: 2, 1: 4} == {k: a.class_counts[k] + b.class_counts[k] + c.class_counts[k] for k in (0, 1)}
    assert torch.equal(got.sample_weights, want.sample_weights)
    one = cda.DeviceClipBank.concat([a])
    assert torch.equal(one.data, a.data) and one.labels.tolist() == a.labels.tolist()
    assert a.lengths.tolist() == [5, 1, 16001] and len(b) == 1                     # the parts are left as they were


def test_prepare_dataset_split_of_a_bank_is_subset_of_the_split():
    lengths = [10 + 3 * k for k in range(24)]
    labels = [0] * 14 + [1] * 10
    bank, _ = _cpu_bank(lengths, labels, 5)
    train_idx, val_idx = cda.stratified_split(bank.labels)
    assert len(val_idx) == 5 and len(train_idx) == 19
    for kw, idx in ((dict(), (train_idx, val_idx)),
                    (dict(val_split=0.25, random_state=7), cda.stratified_split(labels, 0.25, 7))):
        got = cda.prepare_dataset_split(bank, **kw)
        for g, i in zip(got, idx):
            want = bank.subset(i)
            assert torch.equal(g.data, want.data) and g.lengths.tolist() == want.lengths.tolist()
            assert g.labels.tolist() == [labels[j] for j in i] and min(g.class_counts.values()) >= 1
    p = inspect.signature(cda.prepare_dataset_split).parameters
    assert list(p) == ["data_dir_or_bank", "preprocessor", "val_split", "random_state", "device"]
    assert (p["val_split"].default, p["random_state"].default) == (0.2, 42)
    with pytest.raises(ValueError, match="preprocessor"):
        cda.prepare_dataset_split("some/dir")


def test_prepare_dataset_split_reads_a_directory(tmp_path):
    g = np.random.RandomState(8)
    for cls, count in (("non_cough", 6), ("cough", 4)):
        (tmp_path / cls).mkdir()
        for k in range(count):
            _write_wave(tmp_path / cls / f"{k}.wav", g.uniform(-0.4, 0.4, 100 + 11 * k))
    pre = cda.AudioPreprocessor(**SHIPPED)
    bank = cda.DeviceClipBank.from_directory(str(tmp_path), pre, device="cpu")
    train, val = cda.prepare_dataset_split(str(tmp_path), pre, device="cpu")
    train_idx, val_idx = cda.stratified_split(bank.labels)
    assert len(train) == 8 and len(val) == 2 and val.class_counts == {0: 1, 1: 1}
    assert torch.equal(train.data, bank.subset(train_idx).data) and torch.equal(val.data, bank.subset(val_idx).data)


# ------------------------------------------------------------------------------------------------ the command line
def test_cli_defaults_are_the_references():
    import cough_detector_amd.train as m
    kw = m.train_kwargs(m.build_parser().parse_args([]))
    assert kw == dict(data_dir=None, output_dir="./checkpoints", model_type="small", epochs=100, batch_size=32,
                      learning_rate=1e-3, weight_decay=0.01, patience=15, device="auto", num_workers=4, resume=None,
                      use_esc50=True, esc50_dir=None, val_split=0.2, draws="host", seed=None)
    sig = inspect.signature(m.train).parameters
    assert list(sig)[:13] == ["data_dir", "output_dir", "model_type", "epochs", "batch_size", "learning_rate",
                              "weight_decay", "patience", "device", "num_workers", "resume", "use_esc50", "esc50_dir"]
    for name, value in kw.items():
        if name not in ("data_dir", "output_dir"):
            assert sig[name].default == value, name
    assert {n for n, p in sig.items() if p.kind is p.KEYWORD_ONLY} == {"val_split", "random_state", "p_augment", "draws", "seed"}
    assert (sig["random_state"].default, sig["p_augment"].default) == (42, 0.3)


def test_cli_flags_map_to_train_arguments(capsys):
    import cough_detector_amd.train as m
    kw = m.train_kwargs(m.build_parser().parse_args(
        ["--data-dir", "d", "--output-dir", "o", "--model-type", "standard", "--epochs", "3", "--batch-size", "8", "--lr",
         "0.01", "--weight-decay", "0.1", "--patience", "2", "--device", "cuda", "--num-workers", "0", "--resume", "r.pt",
         "--no-esc50", "--esc50-dir", "e", "--seed", "3", "--draws", "device", "--val-split", "0.25"]))
    assert kw == dict(data_dir="d", output_dir="o", model_type="standard", epochs=3, batch_size=8, learning_rate=0.01,
                      weight_decay=0.1, patience=2, device="cuda", num_workers=0, resume="r.pt", use_esc50=False,
                      esc50_dir="e", val_split=0.25, draws="device", seed=3)
    for choice in ("standard", "small", "residual"):
        assert m.build_parser().parse_args(["--model-type", choice]).model_type == choice
    for bad in (["--model-type", "tiny"], ["--draws", "gpu"]):
        with pytest.raises(SystemExit):
            m.build_parser().parse_args(bad)
    with pytest.raises(SystemExit):
        m.main(["--model-type", "tiny"])
    capsys.readouterr()


# ------------------------------------------------------------------------------------------------ train()'s refusals
def test_train_refuses_before_it_touches_a_device(tmp_path, monkeypatch):
    from cough_detector_amd.train import train
    import cough_detector_amd.train as m

    def touched(*a, **k):
        raise AssertionError("train() went past its argument checks")

    for name in ("AudioPreprocessor", "prepare_dataset_split", "create_model", "fit"):
        monkeypatch.setattr(m, name, touched)
    out = tmp_path / "out"
    for device in ("cpu", "mps", "cuda:0", None):
        with pytest.raises(ValueError, match="no CPU fallback"):
            train(str(tmp_path), str(out), device=device)
    with pytest.raises(ValueError, match="No training data"):
        train(None, str(out), use_esc50=False)
    with pytest.raises(ValueError, match="No training data"):
        train(str(tmp_path / "missing"), str(out), use_esc50=False)
    with pytest.raises(ValueError, match="model type"):
        train(str(tmp_path), str(out), model_type="tiny", use_esc50=False)
    with pytest.raises(ValueError, match="No training data"):
        m.main(["--output-dir", str(out), "--no-esc50"])
    assert not out.exists()


def test_preprocessor_config_is_the_references_block():
    import cough_detector_amd.train as m
    cfg = m.preprocessor_config()
    assert cfg == dict(sample_rate=16000, n_mels=64, n_fft=512, hop_length=160, win_length=400, f_min=100.0, f_max=4000.0,
                       segment_duration=1.0, n_mfcc=13, use_mfcc=True, use_pcen=False, use_pre_emphasis=False,
                       pre_emphasis_coef=0.97, use_delta_delta=False, use_spectral_contrast=False, n_contrast_bands=6)
    pre = cda.AudioPreprocessor(**cfg)
    assert pre.get_num_features() == 90 and pre.segment_samples == 16000
    from cough_detector_amd.inference import num_features_from_config
    assert num_features_from_config(cfg) == 90
    assert m._TRAINERS == {"small": cda.SmallTrainer, "residual": cda.ResidualTrainer, "standard": cda.StandardTrainer}


# ------------------------------------------------------------------------------------------------ exports
def test_exports():
    for name in ("prepare_dataset_split", "stratified_split"):
        assert name in cda.__all__ and getattr(cda, name) is getattr(cdata, name), name
    assert "train" not in cda.__all__ and len(set(cda.__all__)) == len(cda.__all__)
    import cough_detector_amd.train as m
    assert callable(m.train) and callable(m.main) and cda.train is m             # the submodule, not a function
    assert hasattr(cda.DeviceClipBank, "concat") and hasattr(cda.DeviceClipBank, "from_esc50")
