"""The label audit of the reference's improvement plan (its step 1.3, an ``audit_dataset`` stub: estimate the mislabel
rate of a source, discard the source above 5 %), assembled from what this package already runs on the MI355X.

``out_of_fold_scores`` splits a ``DeviceClipBank`` into stratified folds (``stratified_kfold``), trains one model per
fold on the other folds -- ``create_data_loaders``, a HIP trainer and ``train_epoch_async``, exactly the pieces of
``train()`` -- and scores the held-out fold with the eval-mode forward, so every clip gets the probability of a model
that never saw it.  ``find_label_issues`` applies the confident-learning rule (Northcutt, Jiang and Chuang, "Confident
Learning: Estimating Uncertainty in Dataset Labels", JAIR 2021) for two classes to those probabilities: the clips whose
out-of-fold score is confidently the other class, the share of each class they make up, and all clips ranked by margin
("listen to these first").  ``audit_labels`` is the two in sequence; ``bank_files`` names the clips of a directory.

Nothing here launches a kernel of its own.  A batch costs what it costs in ``train_epoch_async`` and in ``validate``: no
per-clip Python, no host read; the probabilities are scattered into one ``(n, 2)`` device tensor and stay there until
``metrics()`` or ``find_label_issues`` reads it, once.  Per fold the host does read the trained weights once, when the
eval-mode handle is built from them.

The audit judges each clip as the loader sees it: ``cough_prepare_rows`` keeps the centre ``segment_duration`` of a
longer clip, so long recordings go through ``extract_segments`` first.  Copies of one clip on both sides of a fold make
these scores optimistic: ``cough_detector_amd.duplicates`` finds them (and copies filed under both labels) beforehand.

    python -m cough_detector_amd.audit data --model-type small --folds 5 --epochs 20 --top 50
"""
from __future__ import annotations

import json
import random
from pathlib import Path
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import train as _train
from .augmentation import AudioAugmentor, SpecAugment
from .data import _AUDIO_EXTENSIONS, CLASSES, DeviceClipBank, create_data_loaders
from .loop import class_weights_from_counts, train_epoch_async
from .model import create_model
from .preprocessing import AudioPreprocessor


# ------------------------------------------------------------------------------------------------ folds
def stratified_kfold(labels, folds: int = 5, random_state: int = 42) -> np.ndarray:
    """``(n,)`` int64: the fold (``0..folds-1``) of every clip, stratified by ``labels`` (0 / 1).  The contract is this
    package's own (no scikit-learn): with ``rng = np.random.RandomState(random_state)`` and ``start = 0``, for class
    ``c`` in ``(0, 1)`` in that order::

        idx = rng.permutation(np.flatnonzero(labels == c))
        fold[idx[m]] = (m + start) % folds            # for every m
        start = (start + len(idx)) % folds

    Class 1 goes on dealing where class 0 stopped, so the fold sizes differ by at most 1 overall and by at most 1 per
    class.  ``ValueError``: ``folds < 2``, labels that are not one-dimensional, a label outside {0, 1}, a class with
    fewer than ``folds`` members."""
    y = np.asarray(labels.tolist() if isinstance(labels, torch.Tensor) else labels)
    if y.ndim != 1:
        raise ValueError(f"stratified_kfold: labels must be one-dimensional, got shape {y.shape}")
    if isinstance(folds, bool) or not isinstance(folds, (int, np.integer)) or folds < 2:
        raise ValueError(f"stratified_kfold: folds={folds!r} must be an integer >= 2")
    if not np.isin(y, (0, 1)).all():
        raise ValueError("stratified_kfold: labels are 0 (non_cough) or 1 (cough)")
    folds = int(folds)
    fold = np.empty(y.shape[0], dtype=np.int64)
    rng = np.random.RandomState(random_state)
    start = 0
    for c in (0, 1):
        members = np.flatnonzero(y == c)
        if len(members) < folds:
            raise ValueError(f"stratified_kfold: class {c} has {len(members)} member(s); {folds} folds need at least "
                             f"{folds} of every class")
        idx = rng.permutation(members)
        fold[idx] = (np.arange(len(idx), dtype=np.int64) + start) % folds
        start = (start + len(idx)) % folds
    return fold


# ------------------------------------------------------------------------------------------------ out-of-fold scores
class OutOfFoldScores:
    """What ``out_of_fold_scores`` returns.  ``prob``: ``(n, 2)`` float32 on the device, row i the softmax of the logits
    that the model of fold ``fold[i]`` -- trained without that fold -- gives clip i.  ``fold`` (n,) int64 and ``labels``
    (n,) int64: numpy arrays.  ``history``: per fold the list of per-epoch ``{'loss', 'accuracy'}`` of
    ``train_epoch_async``.  ``config``: every argument of the call."""

    def __init__(self, prob: torch.Tensor, fold: np.ndarray, labels: np.ndarray, history: List[List[Dict[str, float]]],
                 config: Dict):
        self.prob, self.fold, self.labels, self.history, self.config = prob, fold, labels, history, config

    def __len__(self) -> int:
        return int(self.labels.shape[0])

    def metrics(self) -> Dict[str, float]:
        """``{'accuracy', 'precision', 'recall', 'f1', 'tp', 'fp', 'fn', 'tn'}`` of the out-of-fold argmax (a tie is
        class 0) against the given labels over all clips, by ``validate``'s formulas: accuracy in percent, precision /
        recall / F1 of the cough class (1), 0.0 where a denominator is 0.  One read of ``prob``."""
        p = self.prob.cpu().numpy()
        pred, y = p[:, 1] > p[:, 0], self.labels == 1
        tp, fp = int((pred & y).sum()), int((pred & ~y).sum())
        fn, tn = int((~pred & y).sum()), int((~pred & ~y).sum())
        precision = tp / (tp + fp) if (tp + fp) > 0 else 0.0
        recall = tp / (tp + fn) if (tp + fn) > 0 else 0.0
        f1 = 2 * precision * recall / (precision + recall) if (precision + recall) > 0 else 0.0
        return {"accuracy": 100.0 * (tp + tn) / max(len(self), 1), "precision": precision, "recall": recall, "f1": f1,
                "tp": tp, "fp": fp, "fn": fn, "tn": tn}


def _nonfinite_clips(bank: DeviceClipBank) -> List[int]:
    """The clips of ``bank`` that hold a NaN or an infinity: one prefix sum where the bank lives, one read of n counts."""
    if not len(bank):
        return []
    bad = torch.cumsum(~torch.isfinite(bank.data), 0, dtype=torch.int64)
    bad = torch.cat([bad.new_zeros(1), bad])
    per_clip = bad[bank.offsets_dev + bank.lengths_dev] - bad[bank.offsets_dev]
    return np.flatnonzero(per_clip.cpu().numpy()).tolist()


def out_of_fold_scores(bank: DeviceClipBank, preprocessor, model_type: str = "small", folds: int = 5, epochs: int = 20,
                       batch_size: int = 32, learning_rate: float = 1e-3, weight_decay: float = 0.01,
                       p_augment: float = 0.0, draws: str = "host", seed: int = 0, random_state: int = 42,
                       scheduler_factory: Optional[Callable] = None) -> OutOfFoldScores:
    """Every clip of ``bank`` scored by a model that was trained without it.

    The clips are dealt into ``stratified_kfold(bank.labels, folds, random_state)``.  For fold k, ``random``, ``numpy``
    and ``torch`` are seeded with ``seed + k`` and a ``model_type`` model is built; it trains on
    ``bank.subset(clips of the other folds, ascending)`` through ``create_data_loaders(..., use_weighted_sampler=True,
    draws=draws, generator=torch.Generator().manual_seed(seed + k))`` and the model type's HIP trainer (``lr``,
    ``weight_decay``, the class weights of the training clips' counts, ``seed=seed + k``) for ``epochs`` times
    ``train_epoch_async``: no early stopping, no checkpoint, no look at the held-out fold.  ``p_augment``: 0 trains on
    the clips as they are; otherwise the ``AudioAugmentor`` and ``SpecAugment`` of ``train()`` at that probability.
    ``scheduler_factory(optimizer)``, when given, returns a scheduler that is stepped once per epoch; the default is a
    constant learning rate.  The model then scores ``bank.subset(clips of fold k, ascending)`` in eval mode, batch by
    batch in order, and the softmax of its logits goes to those clips' rows of ``prob`` on the device.

    Refused before anything is trained (``ValueError``): an unknown ``model_type``, what ``stratified_kfold`` refuses,
    and a bank that holds a non-finite sample, with the clips' indices -- one NaN clip in a training fold turns that
    fold's parameters, and with them every score the fold produces, into NaN.

    The trainers and loaders are deterministic: the same arguments give the same ``prob`` bit for bit."""
    if model_type not in _train._TRAINERS:
        raise ValueError(f"out_of_fold_scores: unknown model type {model_type!r}; choose from {list(_train.MODEL_TYPES)}")
    if epochs < 0:
        raise ValueError(f"out_of_fold_scores: epochs={epochs} must not be negative")
    labels = bank.labels.numpy().copy()
    fold = stratified_kfold(labels, folds, random_state)
    bad = _nonfinite_clips(bank)
    if bad:
        raise ValueError(f"out_of_fold_scores: clip(s) {bad} hold non-finite samples; one of them in a training fold "
                         "makes every score of that fold NaN")
    config = dict(model_type=model_type, folds=int(folds), epochs=epochs, batch_size=batch_size,
                  learning_rate=learning_rate, weight_decay=weight_decay, p_augment=p_augment, draws=draws, seed=seed,
                  random_state=random_state,
                  scheduler_factory=None if scheduler_factory is None else getattr(scheduler_factory, "__name__",
                                                                                   repr(scheduler_factory)))
    audio_augmentor = spec_augmentor = None
    if p_augment != 0:
        audio_augmentor = AudioAugmentor(sample_rate=preprocessor.sample_rate, p_augment=p_augment)
        spec_augmentor = SpecAugment(freq_mask_param=8, time_mask_param=15, n_freq_masks=2, n_time_masks=2, p=p_augment)

    dev = bank.device
    prob = torch.full((len(bank), 2), float("nan"), dtype=torch.float32, device=dev)
    history = []
    for k in range(int(folds)):
        random.seed(seed + k)
        np.random.seed(seed + k)
        torch.manual_seed(seed + k)
        held = np.flatnonzero(fold == k)
        train_bank, held_bank = bank.subset(np.flatnonzero(fold != k).tolist()), bank.subset(held.tolist())
        train_loader, held_loader = create_data_loaders(
            train_bank, held_bank, preprocessor, batch_size=batch_size, use_weighted_sampler=True,
            audio_augmentor=audio_augmentor, spec_augmentor=spec_augmentor, draws=draws,
            generator=torch.Generator().manual_seed(seed + k))
        model = create_model(model_type, n_mels=preprocessor.get_num_features(), num_classes=2, in_channels=1)
        trainer = _train._TRAINERS[model_type](model, lr=learning_rate, weight_decay=weight_decay,
                                               class_weights=class_weights_from_counts(train_bank.class_counts),
                                               seed=seed + k)
        scheduler = scheduler_factory(trainer.optimizer) if scheduler_factory is not None else None
        epochs_run = []
        for epoch in range(epochs):
            epochs_run.append(train_epoch_async(trainer, train_loader, epoch))
            if scheduler is not None:
                scheduler.step()
        history.append(epochs_run)

        model.eval()
        rows = torch.from_numpy(held).to(dev)
        at = 0
        with torch.no_grad():
            for inputs, _ in held_loader:
                p = torch.softmax(model(inputs), dim=1)
                prob.index_copy_(0, rows[at:at + p.shape[0]], p)
                at += p.shape[0]
    return OutOfFoldScores(prob, fold, labels, history, config)


# ------------------------------------------------------------------------------------------------ confident learning
class LabelIssues:
    """What ``find_label_issues`` returns, for n clips.

    Per clip, (n,) numpy arrays: ``given`` (int64, the labels as passed), ``suggested`` (int64, the rule's label; the
    given one where the rule has nothing to say), ``self_confidence`` (float64, ``p[i][given[i]]``) and ``margin``
    (float64, ``p[i][given[i]] - p[i][1 - given[i]]``); both floats are NaN for an unscored clip.
    ``index``: int64, the suspects (``suggested != given``) by ascending margin, ties by index; ``given[index]``,
    ``suggested[index]``, ``margin[index]`` are theirs.  ``ranking``: int64, all scored clips in that order.
    ``unscored``: int64, the clips with a NaN probability, ascending; never suspects, absent from ``ranking``.
    ``thresholds``: (2,) float64, ``t[j]``.  ``noise_rate``: ``{0: share of the clips labelled 0 that are suspects, 1:
    the same for the clips labelled 1}`` (of all clips with that label, unscored ones included; NaN for a label nobody
    carries): the figure the plan's 5 % bar is compared with."""

    def __init__(self, index, given, suggested, self_confidence, margin, thresholds, noise_rate, unscored, ranking):
        self.index, self.given, self.suggested = index, given, suggested
        self.self_confidence, self.margin, self.thresholds = self_confidence, margin, thresholds
        self.noise_rate, self.unscored, self.ranking = noise_rate, unscored, ranking

    def __len__(self) -> int:
        return int(self.index.shape[0])


def find_label_issues(scores_or_prob, labels=None) -> LabelIssues:
    """The confident-learning rule for two classes on out-of-fold probabilities: an ``OutOfFoldScores``, or ``(n, 2)``
    probabilities (tensor or array) with their ``labels``.  Computed in float64 on the host after one read.

    ``t[j]`` is the mean of ``p[i][j]`` over the scored clips labelled j (a row with a NaN is unscored: it is left out
    of the means, is never a suspect and is listed in ``unscored``).  ``C_i = {j : p[i][j] >= t[j]}``; ``suggested[i]``
    is the j in ``C_i`` with the largest ``p[i][j]``, the given label when the two are equal, and the given label when
    ``C_i`` is empty.  Clip i is a suspect iff ``suggested[i] != labels[i]``.  A label without a scored clip has a NaN
    threshold and is never suggested."""
    if isinstance(scores_or_prob, OutOfFoldScores):
        prob = scores_or_prob.prob
        labels = scores_or_prob.labels if labels is None else labels
    else:
        prob = scores_or_prob
    if labels is None:
        raise ValueError("find_label_issues: probabilities need their labels")
    if isinstance(prob, torch.Tensor):
        prob = prob.detach().cpu().numpy()
    p = np.asarray(prob, dtype=np.float64)
    y = np.asarray(labels.tolist() if isinstance(labels, torch.Tensor) else labels).astype(np.int64)
    if p.ndim != 2 or p.shape[1] != 2:
        raise ValueError(f"find_label_issues: expected probabilities (n, 2), got {p.shape}")
    if y.shape != (p.shape[0],):
        raise ValueError(f"find_label_issues: {p.shape[0]} rows of probabilities but labels of shape {y.shape}")
    if not np.isin(y, (0, 1)).all():
        raise ValueError("find_label_issues: labels are 0 (non_cough) or 1 (cough)")
    n = p.shape[0]
    index = np.arange(n, dtype=np.int64)
    scored = ~np.isnan(p).any(axis=1)
    thresholds = np.array([p[scored & (y == j), j].mean() if (scored & (y == j)).any() else np.nan for j in (0, 1)])
    with np.errstate(invalid="ignore"):
        confident = (p >= thresholds) & scored[:, None]                   # C_i, one column per class
        other_wins = confident[index, 1 - y] & (~confident[index, y] | (p[index, 1 - y] > p[index, y]))
    suggested = np.where(other_wins, 1 - y, y)
    self_confidence = p[index, y]
    margin = p[index, y] - p[index, 1 - y]
    self_confidence[~scored] = np.nan
    margin[~scored] = np.nan
    ranking = index[scored]
    ranking = ranking[np.lexsort((ranking, margin[ranking]))]
    suspects = ranking[suggested[ranking] != y[ranking]]
    noise_rate = {j: float((y[suspects] == j).sum() / (y == j).sum()) if (y == j).any() else float("nan")
                  for j in (0, 1)}
    return LabelIssues(suspects, y, suggested, self_confidence, margin, thresholds, noise_rate, index[~scored], ranking)


# ------------------------------------------------------------------------------------------------ the audit in one call
def bank_files(data_dir: str) -> List[str]:
    """The paths of the files that ``DeviceClipBank.from_directory(data_dir, ...)`` reads, in the bank's order:
    ``data_dir/non_cough`` then ``data_dir/cough``, the files of each in directory order, WAVE files only; a missing
    class directory contributes nothing.  Clip k of the bank is ``bank_files(data_dir)[k]`` as long as the directory
    has not changed in between."""
    files = []
    for class_name in CLASSES:
        class_dir = Path(data_dir) / class_name
        if not class_dir.exists():
            continue
        for audio_file in class_dir.iterdir():
            suffix = audio_file.suffix.lower()
            if suffix in _AUDIO_EXTENSIONS and suffix == ".wav":
                files.append(str(audio_file))
    return files


def audit_labels(data_dir_or_bank, preprocessor=None, **kw) -> Tuple[OutOfFoldScores, LabelIssues]:
    """``(scores, issues)``: ``out_of_fold_scores(bank, preprocessor, **kw)`` and ``find_label_issues(scores)``.  A
    directory is read with ``DeviceClipBank.from_directory``; without a ``preprocessor`` the one of ``train()``
    (``preprocessor_config()``) is built on the GPU."""
    if preprocessor is None:
        preprocessor = AudioPreprocessor(device="cuda", **_train.preprocessor_config())
    bank = data_dir_or_bank
    if not isinstance(bank, DeviceClipBank):
        bank = DeviceClipBank.from_directory(str(bank), preprocessor)
    scores = out_of_fold_scores(bank, preprocessor, **kw)
    return scores, find_label_issues(scores)


# ------------------------------------------------------------------------------------------------ CLI
def build_parser():
    import argparse
    parser = argparse.ArgumentParser(prog="python -m cough_detector_amd.audit",
                                     description="Audit the labels of DATA_DIR/non_cough and DATA_DIR/cough with "
                                                 "out-of-fold scores (MI355X path)")
    parser.add_argument("data_dir", help="directory with non_cough/ and cough/ WAVE files")
    parser.add_argument("--model-type", type=str, default="small", choices=list(_train.MODEL_TYPES),
                        help="Model architecture")
    parser.add_argument("--folds", type=int, default=5, help="Number of stratified folds")
    parser.add_argument("--epochs", type=int, default=20, help="Training epochs per fold")
    parser.add_argument("--batch-size", type=int, default=32, help="Batch size")
    parser.add_argument("--seed", type=int, default=0, help="Fold k is seeded with seed + k")
    parser.add_argument("--top", type=int, default=50, help="How many of the lowest-margin files to list")
    parser.add_argument("--draws", type=str, default="host", choices=["host", "device"],
                        help="Where the training loaders make their per-item draws")
    parser.add_argument("--p-augment", type=float, default=0.0, help="Probability of the training augmentations")
    return parser


def main(argv: Optional[Sequence[str]] = None) -> dict:
    """Prints the ``--top`` lowest-margin files, one per line as ``path <tab> given <tab> suggested <tab> margin``, then
    one JSON object: ``n``, ``folds``, ``metrics``, ``thresholds``, ``noise_rate``, ``suspects`` (their number) and
    ``unscored`` (their number)."""
    args = build_parser().parse_args(argv)
    preprocessor = AudioPreprocessor(device="cuda", **_train.preprocessor_config())
    files = bank_files(args.data_dir)
    bank = DeviceClipBank.from_directory(args.data_dir, preprocessor)
    if len(files) != len(bank):
        raise RuntimeError(f"audit: {args.data_dir} changed while it was read ({len(files)} files, {len(bank)} clips)")
    scores, issues = audit_labels(bank, preprocessor, model_type=args.model_type, folds=args.folds, epochs=args.epochs,
                                  batch_size=args.batch_size, seed=args.seed, draws=args.draws, p_augment=args.p_augment)
    for i in issues.ranking[:max(args.top, 0)]:
        print(f"{files[i]}\t{CLASSES[issues.given[i]]}\t{CLASSES[issues.suggested[i]]}\t{issues.margin[i]:.6f}")
    report = {"n": len(bank), "folds": args.folds, "metrics": scores.metrics(),
              "thresholds": issues.thresholds.tolist(), "noise_rate": {str(j): v for j, v in issues.noise_rate.items()},
              "suspects": len(issues), "unscored": int(issues.unscored.shape[0])}
    print(json.dumps(report))
    return report


if __name__ == "__main__":
    main()
