"""The epoch loop around the HIP training step: what the reference's ``src/train.py`` does outside one optimisation step.

``EarlyStopping`` (:31-52), ``validate`` (:114-180), ``save_checkpoint`` / ``load_checkpoint`` (:183-212), the class-weight
rule (:429-436) and the loop of ``train`` (:458-518, ``fit``), for a ``ResidualTrainer``, ``SmallTrainer`` or
``StandardTrainer`` that the caller has built.  The per-batch metric arithmetic of ``train_epoch`` and ``validate``
(``loss.item()``, ``outputs.max(1)``, ``predicted.eq(targets).sum().item()``, the predictions' copy to the host) runs in
one small kernel, ``cough_epoch_meter_update`` of ``libcough_amd_loop.so`` (``include/cough_amd_loop.h``), which
accumulates into 64 bytes of device memory: an epoch synchronises with the device once, when it reads them.

The checkpoints are the reference's (``epoch``, ``model_state_dict``, ``optimizer_state_dict``, ``metrics``, ``config``),
so ``CoughDetectorInference`` and the reference's own loader read them; with a trainer they also carry ``trainer_state``
(the dropout generator's seed and draw count), which makes a resumed run continue bit for bit.
"""
from __future__ import annotations

import json
import os
from typing import Dict, Iterable, Mapping, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._native import cuda_device
from .model import CoughDetector, CoughDetectorResidual, CoughDetectorSmall
from .training import soft_class

CHECKPOINT_KEYS = ("epoch", "model_state_dict", "optimizer_state_dict", "metrics", "config")
_METER_FIELDS = ("n_batches", "total", "correct", "tp", "fp", "fn", "tn")
_MODEL_TYPES = ((CoughDetectorResidual, "residual"), (CoughDetectorSmall, "small"), (CoughDetector, "standard"))


class EarlyStopping:
    """The reference's ``EarlyStopping`` (``src/train.py:31-52``): ``self(val_loss)`` returns True once ``patience`` calls
    in a row have failed to bring the loss more than ``min_delta`` below the best one."""

    def __init__(self, patience: int = 10, min_delta: float = 0.001):
        self.patience = patience
        self.min_delta = min_delta
        self.counter = 0
        self.best_loss = None
        self.early_stop = False

    def __call__(self, val_loss: float) -> bool:
        if self.best_loss is None:
            self.best_loss = val_loss
        elif val_loss > self.best_loss - self.min_delta:
            self.counter += 1
            if self.counter >= self.patience:
                self.early_stop = True
        else:
            self.best_loss = val_loss
            self.counter = 0
        return self.early_stop


def class_weights_from_counts(counts, max_ratio: float = 20.0) -> torch.Tensor:
    """The reference's class weights (``src/train.py:429-436``) from ``counts`` (a mapping ``{0: n, 1: n}`` or a pair):
    ``total / (2 * count)`` per class, a class that is missing counted as 1, the cough weight capped at ``max_ratio``
    times the other.  A float32 CPU tensor ``[weight_0, weight_1]``."""
    if not isinstance(counts, Mapping):
        counts = dict(enumerate(counts))
    total = counts.get(0, 1) + counts.get(1, 1)
    weight_0 = total / (2 * max(counts.get(0, 1), 1))
    weight_1 = total / (2 * max(counts.get(1, 1), 1))
    if weight_1 / weight_0 > max_ratio:
        weight_1 = weight_0 * max_ratio
    return torch.tensor([weight_0, weight_1])


class EpochMeter:
    """An epoch's running loss and prediction counts in device memory (``cough_epoch_meter``).  ``update`` is one
    stream-ordered launch and reads nothing back; ``result()`` is the only synchronisation."""

    def __init__(self, device=None):
        self.device = torch.device(device) if device is not None else cuda_device()
        if self.device.type != "cuda":
            raise ValueError(f"EpochMeter: device={device!r}; the meter lives on the GPU")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        _lib.load_loop()
        self._buf = torch.zeros(_lib.EPOCH_METER_BYTES // 8, dtype=torch.int64, device=self.device)

    def reset(self) -> None:
        self._buf.zero_()

    def update(self, logits: torch.Tensor, targets: torch.Tensor, class_weights: Optional[torch.Tensor] = None,
               batch_loss: Optional[torch.Tensor] = None, preds_out: Optional[torch.Tensor] = None) -> None:
        """One batch: ``logits`` (B, 2), ``targets`` (B,) class indices.  ``batch_loss`` (a 1-element float32 device
        tensor, e.g. the loss a trainer's ``step`` returned) is added as it is; without it the batch's
        ``CrossEntropyLoss(weight=class_weights)`` is computed by the kernel.  ``preds_out`` (B,) int64 device tensor,
        optional, receives the predictions.  Soft ``targets`` (B, 2) floating are accepted with a ``batch_loss``: the
        class index counted is their argmax (first of equal values), taken on the device.  Without a ``batch_loss``
        they are refused: the meter's own loss is the class-index loss."""
        dev = self.device
        z = logits.detach().to(device=dev, dtype=torch.float32).contiguous()
        if z.dim() != 2 or z.shape[1] != 2 or z.shape[0] < 1:
            raise ValueError(f"EpochMeter.update: expected logits (B, 2) with B >= 1, got {tuple(logits.shape)}")
        t = torch.as_tensor(targets).detach()
        if t.dim() == 2 and t.dtype.is_floating_point:
            if tuple(t.shape) != (z.shape[0], 2):
                raise ValueError(f"EpochMeter.update: soft targets {tuple(t.shape)} for {z.shape[0]} clips")
            if batch_loss is None:
                raise ValueError("EpochMeter.update: soft targets need the step's batch_loss (the meter computes the "
                                 "class-index loss only)")
            t = soft_class(t.to(dev))
        t = t.to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
        if t.numel() != z.shape[0]:
            raise ValueError(f"EpochMeter.update: {t.numel()} targets for {z.shape[0]} clips")
        cw = loss = None
        if class_weights is not None:
            cw = torch.as_tensor(class_weights).detach().to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
            if cw.numel() != 2:
                raise ValueError("EpochMeter.update: class_weights needs one weight per class (2)")
        if batch_loss is not None:
            loss = batch_loss.detach().to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
            if loss.numel() != 1:
                raise ValueError("EpochMeter.update: batch_loss must hold one value")
        if preds_out is not None and not (preds_out.device == dev and preds_out.dtype == torch.int64
                                          and preds_out.is_contiguous() and preds_out.numel() == z.shape[0]):
            raise ValueError(f"EpochMeter.update: preds_out must be a contiguous int64 tensor of {z.shape[0]} on {dev}")
        ptr = lambda a: None if a is None else a.data_ptr()     # noqa: E731
        _lib.check_loop(_lib.load_loop().cough_epoch_meter_update(
            z.data_ptr(), t.data_ptr(), z.shape[0], ptr(cw), ptr(loss), self._buf.data_ptr(), ptr(preds_out),
            torch.cuda.current_stream(dev).cuda_stream), "cough_epoch_meter_update")

    def result(self) -> Dict[str, float]:
        """``{'loss_sum', 'n_batches', 'total', 'correct', 'tp', 'fp', 'fn', 'tn'}`` (one device-to-host copy)."""
        raw = self._buf.cpu().numpy()
        out = {"loss_sum": float(raw[:1].view(np.float64)[0])}
        out.update({k: int(v) for k, v in zip(_METER_FIELDS, raw[1:])})
        return out


def train_epoch_async(trainer, train_loader: Iterable, epoch: int) -> Dict[str, float]:
    """``training.train_epoch`` without its two host reads per batch: every step is followed by one meter update that
    takes the step's loss buffer and train-mode logits, and the host reads the meter at the end of the epoch.  The
    same ``{'loss', 'accuracy'}``, to the last bit."""
    trainer.model.train()
    dev = trainer.device
    meter = EpochMeter(dev)
    for inputs, targets in train_loader:
        inputs = inputs.to(dev)
        targets = torch.as_tensor(targets).to(dev)
        loss, outputs = trainer.step(inputs, targets)
        meter.update(outputs, targets, batch_loss=loss)
    r = meter.result()
    return {"loss": r["loss_sum"] / max(r["n_batches"], 1), "accuracy": 100.0 * r["correct"] / max(r["total"], 1)}


def _device_of(model) -> torch.device:
    p = next(model.parameters(), None)
    return p.device if p is not None and p.device.type == "cuda" else cuda_device()


@torch.no_grad()
def validate(model, val_loader: Iterable, class_weights=None, device=None) -> Dict[str, float]:
    """The reference's ``validate`` (``src/train.py:114-180``) on the eval-mode kernels: ``{'loss', 'accuracy',
    'precision', 'recall', 'f1', 'tp', 'fp', 'fn', 'tn'}``, precision / recall / F1 of the cough class (1).  ``loss`` is
    the mean over the batches of ``CrossEntropyLoss(weight=class_weights)``.  The logits never leave the device: one
    meter update per batch, one read per epoch.  The model stays in eval mode, as the reference leaves it."""
    dev = torch.device(device) if device is not None else _device_of(model)
    model.eval()
    meter = EpochMeter(dev)
    cw = None
    if class_weights is not None:
        cw = torch.as_tensor(class_weights).detach().to(device=meter.device, dtype=torch.float32).reshape(-1).contiguous()
    for inputs, targets in val_loader:
        outputs = model(inputs.to(meter.device))
        meter.update(outputs, targets, class_weights=cw)
    r = meter.result()
    tp, fp, fn, tn = r["tp"], r["fp"], r["fn"], r["tn"]
    precision = tp / (tp + fp) if (tp + fp) > 0 else 0.0
    recall = tp / (tp + fn) if (tp + fn) > 0 else 0.0
    f1 = 2 * precision * recall / (precision + recall) if (precision + recall) > 0 else 0.0
    return {"loss": r["loss_sum"] / max(r["n_batches"], 1), "accuracy": 100.0 * r["correct"] / max(r["total"], 1),
            "precision": precision, "recall": recall, "f1": f1, "tp": tp, "fp": fp, "fn": fn, "tn": tn}


def _to_cpu(obj):
    """``obj`` with every tensor inside copied to the host, compact (a view of a flat buffer would drag the buffer in)."""
    if isinstance(obj, torch.Tensor):
        return obj.detach().to("cpu").clone()
    if isinstance(obj, dict):
        return {k: _to_cpu(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(_to_cpu(v) for v in obj)
    return obj


def save_checkpoint(model, optimizer, epoch: int, metrics: Dict, path: str, config: Dict, trainer=None) -> None:
    """The reference's ``save_checkpoint`` (``src/train.py:183-199``): its five keys, tensors on the host.  With
    ``trainer``, ``trainer_state = {'seed', 'draws'}`` (the device dropout generator) is stored as well; loaders that do
    not know the key ignore it."""
    checkpoint = {"epoch": epoch, "model_state_dict": _to_cpu(model.state_dict()),
                  "optimizer_state_dict": _to_cpu(optimizer.state_dict()), "metrics": metrics, "config": config}
    if trainer is not None:
        checkpoint["trainer_state"] = {"seed": int(trainer.seed), "draws": int(trainer._draws)}
    torch.save(checkpoint, path)


def load_checkpoint(path: str, model, optimizer=None, trainer=None) -> Tuple[int, Dict]:
    """The reference's ``load_checkpoint`` (``src/train.py:202-212``) -> ``(epoch, metrics)``.  The state is copied into
    the model's own tensors, so a model bound to a trainer keeps its flat views, and the model's inference handles are
    dropped.  With ``trainer``, a stored ``trainer_state`` is restored."""
    checkpoint = torch.load(path, map_location="cpu", weights_only=False)
    model.load_state_dict(checkpoint["model_state_dict"])
    if hasattr(model, "invalidate"):
        model.invalidate()
    if optimizer is not None:
        optimizer.load_state_dict(checkpoint["optimizer_state_dict"])
    if trainer is not None and "trainer_state" in checkpoint:
        trainer.seed = int(checkpoint["trainer_state"]["seed"])
        trainer._draws = int(checkpoint["trainer_state"]["draws"])
    return checkpoint["epoch"], checkpoint["metrics"]


def _model_type(model) -> str:
    for cls, name in _MODEL_TYPES:
        if isinstance(model, cls):
            return name
    raise TypeError(f"fit: no model_type for {type(model).__name__}")


def fit(trainer, train_loader: Iterable, val_loader: Iterable, output_dir: str, epochs: int = 100, patience: int = 15,
        config: Optional[Dict] = None, scheduler=None, resume: Optional[str] = None) -> Dict:
    """The loop of the reference's ``train`` (``src/train.py:458-518``) on a trainer: per epoch ``train_epoch_async``,
    ``validate`` with the trainer's class weights and ``scheduler.step()``; ``best_model.pt`` on a strictly better F1,
    ``latest_model.pt`` every epoch, early stopping on the validation loss.  ``config`` goes into ``config.json`` and
    into every checkpoint: besides ``model_type`` (filled in from the model when absent) it needs the preprocessor keys
    that ``CoughDetectorInference`` reads (``n_mels``, ``n_mfcc``, ``use_mfcc``, ``use_pcen``, ...), since the engine's
    defaults are not the shipped training set-up.  ``resume``: a checkpoint to continue from, at its epoch + 1, with the
    best F1 so far taken from its metrics; the scheduler starts anew, as the reference's does.
    Returns ``{'best_model', 'best_f1', 'epochs_run', 'history'}``; ``history`` holds ``{'epoch', 'train', 'val'}`` per
    epoch run."""
    model, optimizer = trainer.model, trainer.optimizer
    config = dict(config or {})
    config.setdefault("model_type", _model_type(model))
    if config["model_type"] != _model_type(model):
        raise ValueError(f"fit: config['model_type']={config['model_type']!r} but the trainer's model is "
                         f"{_model_type(model)!r}")
    os.makedirs(output_dir, exist_ok=True)
    with open(os.path.join(output_dir, "config.json"), "w") as f:
        json.dump(config, f, indent=2)
    if scheduler is None:
        scheduler = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(optimizer, T_0=10, T_mult=2, eta_min=1e-6)
    early_stopping = EarlyStopping(patience=patience)
    best_path, latest_path = os.path.join(output_dir, "best_model.pt"), os.path.join(output_dir, "latest_model.pt")
    start_epoch, best_f1 = 0, 0.0
    if resume and os.path.exists(resume):
        start_epoch, metrics = load_checkpoint(resume, model, optimizer, trainer)
        best_f1 = metrics.get("f1", 0.0)
        start_epoch += 1
    history = []
    for epoch in range(start_epoch, epochs):
        train_metrics = train_epoch_async(trainer, train_loader, epoch)
        val_metrics = validate(model, val_loader, class_weights=trainer.class_weights, device=trainer.device)
        scheduler.step()
        history.append({"epoch": epoch, "train": train_metrics, "val": val_metrics})
        if val_metrics["f1"] > best_f1:
            best_f1 = val_metrics["f1"]
            save_checkpoint(model, optimizer, epoch, val_metrics, best_path, config, trainer)
        save_checkpoint(model, optimizer, epoch, val_metrics, latest_path, config, trainer)
        if early_stopping(val_metrics["loss"]):
            break
    return {"best_model": best_path, "best_f1": best_f1, "epochs_run": len(history), "history": history}
