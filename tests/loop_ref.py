"""Float64 CPU restatement of the reference's epoch loop (TEST INFRASTRUCTURE, not product).

What ``src/train.py`` does around one optimisation step, restated so that the tests have expected values: the
early-stopping rule (:31-52), the per-batch loss and prediction of ``train_epoch`` / ``validate`` (:97-100, :146-155),
the epoch's metrics (:161-180) and the class-weight rule (:429-436).  Everything is computed in float64 from logits
that the caller supplies; the only float32 step is the one the reference itself takes, ``loss.item()`` of a float32
loss (``item32=True``).
"""
from __future__ import annotations

from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

CHECKPOINT_KEYS = {"epoch", "model_state_dict", "optimizer_state_dict", "metrics", "config"}
METRIC_KEYS = {"loss", "accuracy", "precision", "recall", "f1", "tp", "fp", "fn", "tn"}


class EarlyStopping:
    """State after every call: ``counter``, ``best_loss``, and the returned flag (sticky once set)."""

    def __init__(self, patience: int = 10, min_delta: float = 0.001):
        self.patience, self.min_delta = patience, min_delta
        self.counter, self.best_loss, self.early_stop = 0, None, False

    def __call__(self, val_loss: float) -> bool:
        improved = self.best_loss is None or not (val_loss > self.best_loss - self.min_delta)
        if improved:
            if self.best_loss is not None:
                self.counter = 0
            self.best_loss = val_loss
        else:
            self.counter += 1
            self.early_stop = self.early_stop or self.counter >= self.patience
        return self.early_stop


def early_stop_epoch(losses: Sequence[float], patience: int, min_delta: float = 0.001) -> Optional[int]:
    """Index of the first loss at which the rule stops, or None."""
    es = EarlyStopping(patience, min_delta)
    for i, v in enumerate(losses):
        if es(v):
            return i
    return None


def class_weights(counts: Dict[int, int], max_ratio: float = 20.0) -> Tuple[float, float]:
    n0, n1 = counts.get(0, 1), counts.get(1, 1)
    total = n0 + n1
    w0, w1 = total / (2 * max(n0, 1)), total / (2 * max(n1, 1))
    if w1 / w0 > max_ratio:
        w1 = w0 * max_ratio
    return w0, w1


def predict(logits: torch.Tensor) -> torch.Tensor:
    """``outputs.max(1)[1]``: torch's own rule (the first NaN wins, otherwise the first of the largest)."""
    return logits.max(1)[1]


def batch_loss(logits: torch.Tensor, targets: torch.Tensor, weight=None) -> float:
    """float64 ``CrossEntropyLoss(weight)``; NaN for a target outside {0, 1} (torch raises there)."""
    t = torch.as_tensor(targets).long()
    if bool(((t < 0) | (t > 1)).any()):
        return float("nan")
    w = None if weight is None else torch.as_tensor(weight, dtype=torch.float64)
    return float(F.cross_entropy(logits.double(), t, weight=w))


def counts(preds: torch.Tensor, targets: torch.Tensor) -> Dict[str, int]:
    p, t = preds.numpy(), torch.as_tensor(targets).numpy()
    return {"total": int(t.shape[0]), "correct": int((p == t).sum()),
            "tp": int(((p == 1) & (t == 1)).sum()), "fp": int(((p == 1) & (t == 0)).sum()),
            "fn": int(((p == 0) & (t == 1)).sum()), "tn": int(((p == 0) & (t == 0)).sum())}


def epoch_metrics(batches: Iterable[Tuple[torch.Tensor, torch.Tensor]], weight=None, item32: bool = False) -> Dict:
    """``validate`` on (logits, targets) batches.  ``item32`` rounds every batch loss to float32 before it is summed,
    as ``loss.item()`` of a float32 loss does."""
    running, n_batches = 0.0, 0
    preds: List[torch.Tensor] = []
    tgts: List[torch.Tensor] = []
    for z, t in batches:
        loss = batch_loss(z, t, weight)
        running += float(np.float32(loss)) if item32 else loss
        n_batches += 1
        preds.append(predict(z))
        tgts.append(torch.as_tensor(t).long())
    c = counts(torch.cat(preds), torch.cat(tgts))
    tp, fp, fn, tn = c["tp"], c["fp"], c["fn"], c["tn"]
    precision = tp / (tp + fp) if (tp + fp) > 0 else 0
    recall = tp / (tp + fn) if (tp + fn) > 0 else 0
    f1 = 2 * precision * recall / (precision + recall) if (precision + recall) > 0 else 0
    return {"loss": running / n_batches, "accuracy": 100.0 * c["correct"] / c["total"], "precision": precision,
            "recall": recall, "f1": f1, "tp": tp, "fp": fp, "fn": fn, "tn": tn}
