"""Time a whole epoch of the loop around the HIP training step, old against new, on one GPU.

Per configuration (``--configs small:32,standard:256``), with ``--steps`` device-resident batches per epoch:
  train     ``training.train_epoch`` (two host reads per batch) against ``loop.train_epoch_async`` (one per epoch), on two
            trainers that start from the same state and seed, so both compute the same epochs (checked: equal results)
  validate  the reference's validate loop composed from torch ops on the same eval-mode kernels (``loss.item()``,
            ``predicted.eq(targets).sum().item()`` and the predictions' and targets' ``.cpu()`` per batch) against
            ``loop.validate`` (checked: equal counts, loss within 1e-4 relative)
The two sides alternate, ``--rounds`` times after one warm-up epoch each; an epoch is timed with the host clock around a
call that ends in a device synchronise.  Prints one JSON line per (configuration, loop): the median, the fastest and the
slowest epoch in ms of each side, and the ratio of the medians.
Usage: python tools/bench_epoch.py [--configs small:32,standard:256] [--steps 200] [--rounds 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cough_detector_amd as cda                      # noqa: E402
from cough_detector_amd.training import ResidualTrainer, SmallTrainer, StandardTrainer, train_epoch   # noqa: E402

H, W = 90, 101
TRAINERS = {"small": SmallTrainer, "standard": StandardTrainer, "residual": ResidualTrainer}
DISTINCT = 8            # distinct batches in device memory, cycled to --steps


@torch.no_grad()
def torch_validate(model, val_loader, class_weights, device):
    """The reference's validate (src/train.py:114-180) as it is written there, on this project's eval-mode forward."""
    model.eval()
    running_loss, correct, total = 0.0, 0, 0
    all_preds, all_targets = [], []
    n_batches = 0
    for inputs, targets in val_loader:
        inputs, targets = inputs.to(device), targets.to(device)
        outputs = model(inputs)
        loss = F.cross_entropy(outputs, targets, weight=class_weights)
        running_loss += loss.item()
        _, predicted = outputs.max(1)
        total += targets.size(0)
        correct += predicted.eq(targets).sum().item()
        all_preds.extend(predicted.cpu().numpy())
        all_targets.extend(targets.cpu().numpy())
        n_batches += 1
    all_preds, all_targets = np.array(all_preds), np.array(all_targets)
    tp = int(((all_preds == 1) & (all_targets == 1)).sum())
    fp = int(((all_preds == 1) & (all_targets == 0)).sum())
    fn = int(((all_preds == 0) & (all_targets == 1)).sum())
    tn = int(((all_preds == 0) & (all_targets == 0)).sum())
    return {"loss": running_loss / n_batches, "accuracy": 100.0 * correct / total, "tp": tp, "fp": fp, "fn": fn, "tn": tn}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def summary(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "epochs_ms": [round(v, 3) for v in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="small:32,standard:256")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_epoch.py needs the MI355X; there is nothing to time without it")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    for cfg in a.configs.split(","):
        kind, b = cfg.split(":")
        b = int(b)
        g = torch.Generator().manual_seed(b)
        pool = [(torch.randn(b, 1, H, W, generator=g).to(dev), torch.randint(0, 2, (b,), generator=g).to(dev))
                for _ in range(DISTINCT)]
        loader = [pool[i % DISTINCT] for i in range(a.steps)]
        cw = torch.tensor([1.0, 2.5], device=dev)

        def trainer():
            torch.manual_seed(0)
            return TRAINERS[kind](cda.create_model(kind, n_mels=H), class_weights=cw, seed=1)

        old, new = trainer(), trainer()
        t_old, t_new = [], []
        for r in range(a.rounds + 1):
            ms_o, res_o = timed(lambda: train_epoch(old, loader, r))
            ms_n, res_n = timed(lambda: cda.train_epoch_async(new, loader, r))
            assert all(np.array_equal(res_o[k], res_n[k], equal_nan=True) for k in res_o), (res_o, res_n)
            if r > 0:                       # round 0 warms both up
                t_old.append(ms_o)
                t_new.append(ms_n)
        so, sn = summary(t_old), summary(t_new)
        emit({"loop": "train", "model": kind, "batch": b, "steps": a.steps, "rounds": a.rounds,
              "train_epoch": so, "train_epoch_async": sn, "new_over_old": round(sn["median_ms"] / so["median_ms"], 4),
              "results_equal": True})

        model = new.model
        v_old, v_new = [], []
        for r in range(a.rounds + 1):
            ms_o, res_o = timed(lambda: torch_validate(model, loader, cw, dev))
            ms_n, res_n = timed(lambda: cda.validate(model, loader, class_weights=cw, device=dev))
            assert all(res_o[k] == res_n[k] for k in ("tp", "fp", "fn", "tn", "accuracy")), (res_o, res_n)
            assert abs(res_o["loss"] - res_n["loss"]) <= 1e-4 * max(1.0, abs(res_o["loss"])), (res_o, res_n)
            if r > 0:
                v_old.append(ms_o)
                v_new.append(ms_n)
        so, sn = summary(v_old), summary(v_new)
        emit({"loop": "validate", "model": kind, "batch": b, "steps": a.steps, "rounds": a.rounds,
              "torch_ops_validate": so, "validate": sn, "new_over_old": round(sn["median_ms"] / so["median_ms"], 4),
              "results_equal": True})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
