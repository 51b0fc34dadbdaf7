"""The label audit without a GPU (cough_detector_amd/audit.py): the fold assignment and the confident-learning rule
against their restatement in plain loops (tests/audit_ref.py) and against hand-worked tables, ``bank_files`` against
``DeviceClipBank.from_directory`` on a CPU bank, the command line's defaults, the refusals that need no device and the
exports.

The NaN choice that ``find_label_issues`` documents is the one checked here: a row with a NaN probability is left out of
the threshold means (so it cannot move them), is never a suspect, is not ranked and is listed in ``unscored``; it still
counts in the denominator of its label's ``noise_rate``."""
import inspect
import wave

import numpy as np
import pytest
import torch

import audit_ref as R
import cough_detector_amd as cda
from cough_detector_amd import _lib, audit

SHIPPED = dict(use_pcen=False, use_pre_emphasis=False, use_delta_delta=False, use_spectral_contrast=False)
NAMES = ("stratified_kfold", "out_of_fold_scores", "OutOfFoldScores", "find_label_issues", "LabelIssues", "audit_labels",
         "bank_files")


def _labels(n, share, seed):
    k = max(int(round(share * n)), 0)
    y = np.array([0] * (n - k) + [1] * k)
    return np.random.RandomState(seed).permutation(y)


# ------------------------------------------------------------------------------------------------ stratified_kfold
@pytest.mark.parametrize("n,share,folds", [(10, 0.5, 2), (10, 0.5, 5), (11, 0.36, 3), (37, 0.3, 5), (100, 0.1, 10),
                                           (180, 1 / 3, 5), (333, 0.5, 7), (1000, 0.07, 5), (2000, 0.25, 4)])
def test_kfold_is_a_stratified_partition_and_equals_the_restatement(n, share, folds):
    for seed in (0, 42):
        y = _labels(n, share, seed + n)
        fold = cda.stratified_kfold(y, folds, seed)
        assert fold.dtype == np.int64 and fold.shape == (n,)
        assert fold.min() == 0 and fold.max() == folds - 1                      # a partition into exactly `folds` parts
        sizes = np.bincount(fold, minlength=folds)
        assert sizes.sum() == n and sizes.max() - sizes.min() <= 1
        for c in (0, 1):
            per_class = np.bincount(fold[y == c], minlength=folds)
            assert per_class.sum() == (y == c).sum() and per_class.max() - per_class.min() <= 1, c
        assert np.array_equal(fold, R.kfold(y, folds, seed))
        assert np.array_equal(fold, cda.stratified_kfold(y, folds, seed))       # no hidden state
        assert np.array_equal(fold, cda.stratified_kfold(torch.tensor(y), folds=folds, random_state=seed))
        assert np.array_equal(fold, cda.stratified_kfold(y.tolist(), folds, seed))
    assert not np.array_equal(cda.stratified_kfold(y, folds, 0), cda.stratified_kfold(y, folds, 1))


def test_kfold_defaults_and_a_worked_case():
    p = inspect.signature(cda.stratified_kfold).parameters
    assert list(p) == ["labels", "folds", "random_state"] and (p["folds"].default, p["random_state"].default) == (5, 42)
    y = [0] * 7 + [1] * 5
    assert np.array_equal(cda.stratified_kfold(y), cda.stratified_kfold(y, 5, 42))
    # 7 clips of class 0 fill folds 0 1 2 3 4 0 1; class 1 goes on at fold 2: 2 3 4 0 1 -> sizes 3 3 2 2 2
    fold = cda.stratified_kfold(y, 5, 3)
    assert np.bincount(fold[:7]).tolist() == [2, 2, 1, 1, 1] and np.bincount(fold[7:]).tolist() == [1, 1, 1, 1, 1]
    rng = np.random.RandomState(3)
    first = rng.permutation(np.arange(7))
    assert [int(fold[i]) for i in first] == [0, 1, 2, 3, 4, 0, 1]
    second = rng.permutation(np.arange(7, 12))
    assert [int(fold[i]) for i in second] == [2, 3, 4, 0, 1]


def test_kfold_refusals():
    y = [0] * 6 + [1] * 4
    for bad in (1, 0, -3, 2.0, True, None):
        with pytest.raises(ValueError, match="folds"):
            cda.stratified_kfold(y, bad)
    with pytest.raises(ValueError, match="0 .non_cough. or 1"):
        cda.stratified_kfold([0, 1, 2, 0, 1, 1], 2)
    with pytest.raises(ValueError, match="0 .non_cough. or 1"):
        cda.stratified_kfold([0, 1, -1, 0, 1, 1], 2)
    with pytest.raises(ValueError, match="class 1 has 4 member"):
        cda.stratified_kfold(y, 5)
    with pytest.raises(ValueError, match="class 0 has 0 member"):
        cda.stratified_kfold([1] * 8, 2)
    with pytest.raises(ValueError, match="one-dimensional"):
        cda.stratified_kfold([[0, 1], [1, 0]], 2)
    assert cda.stratified_kfold(y, 4).shape == (10,)                            # exactly `folds` members is enough


# ------------------------------------------------------------------------------------------------ find_label_issues
def _same_as_ref(got, prob, labels):
    want = R.label_issues(prob, labels)
    assert got.thresholds.dtype == np.float64 and np.array_equal(got.thresholds, np.array(want["thresholds"]), equal_nan=True)
    assert got.index.tolist() == want["suspects"] and got.ranking.tolist() == want["ranking"]
    assert got.unscored.tolist() == want["unscored"]
    assert got.given.tolist() == [int(v) for v in labels] and got.suggested.tolist() == want["suggested"]
    assert np.array_equal(got.margin, np.array(want["margin"]), equal_nan=True)
    assert np.array_equal(got.self_confidence, np.array(want["self_confidence"]), equal_nan=True)
    assert set(got.noise_rate) == {0, 1}
    for j in (0, 1):
        assert got.noise_rate[j] == want["noise_rate"][j] or (np.isnan(got.noise_rate[j]) and np.isnan(want["noise_rate"][j]))
    for a in (got.index, got.ranking, got.unscored, got.given, got.suggested):
        assert a.dtype == np.int64
    assert len(got) == len(want["suspects"])


@pytest.mark.parametrize("n,share,seed", [(10, 0.5, 0), (57, 0.3, 1), (180, 1 / 3, 2), (1000, 0.1, 3), (2000, 0.5, 4)])
def test_label_issues_equal_the_restatement_on_random_probabilities(n, share, seed):
    g = np.random.RandomState(seed)
    y = _labels(n, share, seed)
    # scores that mostly agree with the label, a tenth that do not
    agree = g.uniform(0.5, 1.0, n)
    p_given = np.where(g.uniform(size=n) < 0.1, 1.0 - agree, agree).astype(np.float32)
    p = np.empty((n, 2), dtype=np.float32)
    p[np.arange(n), y] = p_given
    p[np.arange(n), 1 - y] = np.float32(1.0) - p_given
    got = cda.find_label_issues(p, y)
    _same_as_ref(got, p, y)
    assert 0 < len(got) < n and len(got.ranking) == n and len(got.unscored) == 0
    assert np.all(np.diff(got.margin[got.ranking]) >= 0) and np.all(np.diff(got.margin[got.index]) >= 0)
    # coarse probabilities: many equal margins and rows that sit exactly on a threshold
    q = np.round(p * 8) / 8
    _same_as_ref(cda.find_label_issues(q, y), q, y)
    # a tensor and a list of labels give the same
    again = cda.find_label_issues(torch.from_numpy(p), y.tolist())
    assert again.index.tolist() == got.index.tolist() and np.array_equal(again.margin, got.margin)
    # rows need not sum to 1
    r = g.uniform(0, 1, (n, 2))
    _same_as_ref(cda.find_label_issues(r, y), r, y)


# (p0, p1), given label.  Every value is a multiple of 1/8, so the means below are exact in float64.
#   t0 = mean of p0 over rows 0-5 = (7/8 + 3/4 + 3/8 + 1/2 + 0 + 1/2) / 6 = 3 / 6 = 0.5
#   t1 = mean of p1 over rows 6-9 = (1 + 3/4 + 1/4 + 1/2) / 4 = 2.5 / 4 = 0.625
#   row 0  p0 7/8 >= t0, p1 1/8 <  t1   C = {0}   stays 0      margin  3/4
#   row 1  p0 3/4 >= t0, p1 1/4 <  t1   C = {0}   stays 0      margin  1/2
#   row 2  p0 3/8 <  t0, p1 5/8 == t1   C = {1}   SUSPECT -> 1 margin -1/4   (p == t counts as >=)
#   row 3  p0 1/2 == t0, p1 1/2 <  t1   C = {0}   stays 0      margin  0
#   row 4  p0 0   <  t0, p1 1   >= t1   C = {1}   SUSPECT -> 1 margin -1
#   row 5  as row 3                                             margin  0
#   row 6  p0 0   <  t0, p1 1   >= t1   C = {1}   stays 1      margin  1
#   row 7  p0 1/4 <  t0, p1 3/4 >= t1   C = {1}   stays 1      margin  1/2
#   row 8  p0 3/4 >= t0, p1 1/4 <  t1   C = {0}   SUSPECT -> 0 margin -1/2
#   row 9  p0 1/2 == t0, p1 1/2 <  t1   C = {0}   SUSPECT -> 0 margin  0     (p == t counts as >=)
# suspects by ascending margin: 4, 8, 2, 9; noise rates 2/6 of the clips labelled 0 and 2/4 of those labelled 1
TABLE = [((7 / 8, 1 / 8), 0), ((3 / 4, 1 / 4), 0), ((3 / 8, 5 / 8), 0), ((1 / 2, 1 / 2), 0), ((0.0, 1.0), 0),
         ((1 / 2, 1 / 2), 0), ((0.0, 1.0), 1), ((1 / 4, 3 / 4), 1), ((3 / 4, 1 / 4), 1), ((1 / 2, 1 / 2), 1)]


def test_label_issues_on_a_hand_worked_table():
    p = np.array([row for row, _ in TABLE])
    y = np.array([label for _, label in TABLE])
    got = cda.find_label_issues(p, y)
    assert isinstance(got, cda.LabelIssues)
    assert got.thresholds.tolist() == [0.5, 0.625]
    assert got.index.tolist() == [4, 8, 2, 9] and len(got) == 4
    assert got.suggested.tolist() == [0, 0, 1, 0, 1, 0, 1, 1, 0, 0] and got.given.tolist() == y.tolist()
    assert got.suggested[got.index].tolist() == [1, 0, 1, 0] and got.given[got.index].tolist() == [0, 1, 0, 1]
    assert got.margin.tolist() == [0.75, 0.5, -0.25, 0.0, -1.0, 0.0, 1.0, 0.5, -0.5, 0.0]
    assert got.self_confidence.tolist() == [0.875, 0.75, 0.375, 0.5, 0.0, 0.5, 1.0, 0.75, 0.25, 0.5]
    assert got.ranking.tolist() == [4, 8, 2, 3, 5, 9, 1, 7, 0, 6]              # equal margins in index order
    assert got.noise_rate == {0: 2 / 6, 1: 2 / 4} and got.unscored.tolist() == []
    _same_as_ref(got, p, y)
    # float32 probabilities (what the device holds) are widened, not rounded again
    _same_as_ref(cda.find_label_issues(torch.tensor(p, dtype=torch.float32), torch.tensor(y)), p, y)


def test_ties_keep_the_given_label():
    # t0 = t1 = 0.5 and every row has both classes in C_i with equal probabilities: nothing moves
    p = np.full((4, 2), 0.5)
    got = cda.find_label_issues(p, [0, 1, 0, 1])
    assert got.thresholds.tolist() == [0.5, 0.5] and len(got) == 0 and got.suggested.tolist() == [0, 1, 0, 1]
    assert got.ranking.tolist() == [0, 1, 2, 3] and got.noise_rate == {0: 0.0, 1: 0.0}
    # both classes in C_i, the other one strictly larger: it wins.  t0 = (0.5 + 0.5) / 2, t1 = (0.5 + 0.5) / 2
    p = np.array([[0.5, 0.5], [0.5, 0.75], [0.5, 0.5], [0.5, 0.5]])
    y = [0, 0, 1, 1]
    got = cda.find_label_issues(p, y)
    assert got.thresholds.tolist() == [0.5, 0.5]
    assert got.suggested.tolist() == [0, 1, 1, 1] and got.index.tolist() == [1]    # rows 0, 2, 3 tie and keep theirs
    _same_as_ref(got, p, y)


def test_nan_rows_are_unscored_and_do_not_move_the_thresholds():
    p = np.array([row for row, _ in TABLE] + [(np.nan, 0.3), (0.2, np.nan), (np.nan, np.nan)])
    y = np.array([label for _, label in TABLE] + [0, 1, 1])
    got = cda.find_label_issues(p, y)
    assert got.thresholds.tolist() == [0.5, 0.625]                                 # those of the table alone
    assert got.unscored.tolist() == [10, 11, 12] and got.index.tolist() == [4, 8, 2, 9]
    assert got.ranking.tolist() == [4, 8, 2, 3, 5, 9, 1, 7, 0, 6]
    assert got.suggested[10:].tolist() == [0, 1, 1] and np.isnan(got.margin[10:]).all()
    assert np.isnan(got.self_confidence[10:]).all() and not np.isnan(got.margin[:10]).any()
    assert got.noise_rate == {0: 2 / 7, 1: 2 / 6}                                  # of all clips with that label
    _same_as_ref(got, p, y)
    # a label whose clips are all unscored has no threshold and is never suggested
    got = cda.find_label_issues(np.array([[0.9, 0.1], [0.1, 0.9], [np.nan, 0.5]]), [0, 0, 1])
    assert got.thresholds[0] == 0.5 and np.isnan(got.thresholds[1]) and len(got) == 0 and got.unscored.tolist() == [2]


def test_confident_input_has_no_suspects():
    y = _labels(60, 0.4, 9)
    p = np.where(y[:, None] == np.arange(2)[None, :], 0.97, 0.03)
    got = cda.find_label_issues(p, y)
    assert len(got) == 0 and got.index.dtype == np.int64 and got.noise_rate == {0: 0.0, 1: 0.0}
    assert got.suggested.tolist() == y.tolist() and got.ranking.tolist() == list(range(60))
    assert np.allclose(got.thresholds, 0.97) and np.allclose(got.margin, 0.94)


def test_label_issues_refusals_and_the_scores_object():
    with pytest.raises(ValueError, match="need their labels"):
        cda.find_label_issues(np.zeros((3, 2)))
    with pytest.raises(ValueError, match=r"\(n, 2\)"):
        cda.find_label_issues(np.zeros((3, 3)), [0, 1, 0])
    with pytest.raises(ValueError, match="labels of shape"):
        cda.find_label_issues(np.zeros((3, 2)), [0, 1])
    with pytest.raises(ValueError, match="0 .non_cough. or 1"):
        cda.find_label_issues(np.zeros((3, 2)), [0, 1, 2])
    p = np.array([row for row, _ in TABLE], dtype=np.float32)
    y = np.array([label for _, label in TABLE])
    scores = cda.OutOfFoldScores(torch.from_numpy(p), np.zeros(10, np.int64), y, [], {})
    assert cda.find_label_issues(scores).index.tolist() == [4, 8, 2, 9] and len(scores) == 10
    # argmax with a tie as class 0: predictions 0 0 1 0 1 0 | 1 1 0 0 -> tp 2, fp 2, fn 2, tn 4
    m = scores.metrics()
    assert (m["tp"], m["fp"], m["fn"], m["tn"]) == (2, 2, 2, 4)
    assert m["accuracy"] == 60.0 and m["precision"] == 0.5 and m["recall"] == 0.5 and m["f1"] == 0.5
    assert set(m) == {"accuracy", "precision", "recall", "f1", "tp", "fp", "fn", "tn"}
    none = cda.OutOfFoldScores(torch.tensor([[0.9, 0.1]] * 4), np.zeros(4, np.int64), np.array([0, 0, 1, 1]), [], {})
    assert none.metrics() == dict(accuracy=50.0, precision=0.0, recall=0.0, f1=0.0, tp=0, fp=0, fn=2, tn=2)


# ------------------------------------------------------------------------------------------------ bank_files
def _write_wave(path, n):
    pcm = (np.arange(n) % 100 * 50).astype("<i2")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(pcm.tobytes())


def test_bank_files_are_in_the_banks_order(tmp_path):
    """Every WAVE file has its own length, so the bank's ``lengths`` identify which file became which clip."""
    n = 200
    for cls, names in (("non_cough", ["b.wav", "a.WAV", "zz.wav", "c.wav", "m.wav"]), ("cough", ["y.wav", "x.wav", "k.Wav"])):
        (tmp_path / cls).mkdir()
        for name in names:
            _write_wave(tmp_path / cls / name, n)
            n += 37
    (tmp_path / "non_cough" / "song.mp3").write_bytes(b"ID3")                   # an audio suffix that is not decoded
    (tmp_path / "non_cough" / "notes.txt").write_text("not audio")
    (tmp_path / "cough" / "sub.wav.bak").write_text("not audio")
    (tmp_path / "other").mkdir()
    _write_wave(tmp_path / "other" / "o.wav", 5000)
    pre = cda.AudioPreprocessor(**SHIPPED)
    with pytest.warns(UserWarning, match="skipped 1 audio file"):
        bank = cda.DeviceClipBank.from_directory(str(tmp_path), pre, device="cpu")
    files = cda.bank_files(str(tmp_path))
    assert len(files) == len(bank) == 8 and all(type(f) is str for f in files)
    lengths = []
    for f in files:
        with wave.open(f, "rb") as w:
            lengths.append(w.getnframes())
    assert lengths == bank.lengths.tolist() and len(set(lengths)) == 8
    assert [f.split("/")[-2] for f in files] == ["non_cough"] * 5 + ["cough"] * 3
    assert bank.labels.tolist() == [0] * 5 + [1] * 3
    assert cda.bank_files(tmp_path) == files                                      # a Path is taken too
    # a missing class directory contributes nothing, as in from_directory
    (tmp_path / "only").mkdir()
    (tmp_path / "only" / "cough").mkdir()
    _write_wave(tmp_path / "only" / "cough" / "q.wav", 300)
    assert cda.bank_files(str(tmp_path / "only")) == [str(tmp_path / "only" / "cough" / "q.wav")]


# ------------------------------------------------------------------------------------------------ the call surface
def test_signatures_and_cli_defaults():
    p = inspect.signature(cda.out_of_fold_scores).parameters
    assert list(p) == ["bank", "preprocessor", "model_type", "folds", "epochs", "batch_size", "learning_rate",
                       "weight_decay", "p_augment", "draws", "seed", "random_state", "scheduler_factory"]
    assert [p[k].default for k in list(p)[2:]] == ["small", 5, 20, 32, 1e-3, 0.01, 0.0, "host", 0, 42, None]
    assert list(inspect.signature(cda.audit_labels).parameters) == ["data_dir_or_bank", "preprocessor", "kw"]
    assert list(inspect.signature(cda.find_label_issues).parameters) == ["scores_or_prob", "labels"]
    args = audit.build_parser().parse_args(["some/dir"])
    assert vars(args) == dict(data_dir="some/dir", model_type="small", folds=5, epochs=20, batch_size=32, seed=0, top=50,
                              draws="host", p_augment=0.0)
    args = audit.build_parser().parse_args(["d", "--model-type", "residual", "--folds", "3", "--epochs", "2", "--batch-size",
                                            "8", "--seed", "4", "--top", "7", "--draws", "device", "--p-augment", "0.3"])
    assert vars(args) == dict(data_dir="d", model_type="residual", folds=3, epochs=2, batch_size=8, seed=4, top=7,
                              draws="device", p_augment=0.3)
    for bad in (["d", "--model-type", "tiny"], ["d", "--draws", "gpu"], []):
        with pytest.raises(SystemExit):
            audit.build_parser().parse_args(bad)


def test_refusals_that_need_no_device(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("out_of_fold_scores went past its argument checks")

    for name in ("create_model", "create_data_loaders", "train_epoch_async"):
        monkeypatch.setattr(audit, name, touched)
    g = torch.Generator().manual_seed(0)
    bank = cda.DeviceClipBank([torch.randn(50, generator=g) for _ in range(12)], [0] * 8 + [1] * 4, device="cpu")
    with pytest.raises(ValueError, match="model type"):
        cda.out_of_fold_scores(bank, None, model_type="tiny")
    with pytest.raises(ValueError, match="class 1 has 4 member"):
        cda.out_of_fold_scores(bank, None, folds=5)
    with pytest.raises(ValueError, match="folds"):
        cda.out_of_fold_scores(bank, None, folds=1)
    clips = [torch.randn(50 + k, generator=g) for k in range(12)]
    clips[3][7] = float("nan")
    clips[10][0] = float("inf")
    clips[11][-1] = float("-inf")
    bad = cda.DeviceClipBank(clips, [0] * 8 + [1] * 4, device="cpu")
    with pytest.raises(ValueError, match=r"clip\(s\) \[3, 10, 11\] hold non-finite"):
        cda.out_of_fold_scores(bad, None, folds=2)


def test_exports():
    for name in NAMES:
        assert name in cda.__all__ and getattr(cda, name) is getattr(audit, name), name
    assert "train" not in cda.__all__ and len(set(cda.__all__)) == len(cda.__all__)
    assert callable(audit.main) and cda.audit is audit
    assert len(_lib.LIBRARIES) == 9
