"""Time a whole label audit (``cough_detector_amd.audit.audit_labels``) on one GPU, beside the parts it is made of.

Per bank -- the 180-clip synthetic corpus of tests/test_gpu_audit.py, and ``--clips`` one-second clips generated on the
device by ``synth.device_clips`` (seed % 6 == 0 is the cough-like kind) -- and per mode (``p_augment`` 0; ``--p-augment``
with ``draws="host"`` and with ``draws="device"``):
  audit   ``audit_labels(bank, pre, model_type, folds, epochs, batch)`` from the call to the ``LabelIssues``, ``--rounds``
          times after one warm-up audit of a single epoch per fold
  parts   on the loaders and the trainer of fold 0: one ``train_epoch_async`` epoch, and one eval-mode pass over the held-out
          fold with the softmax and the ``index_copy_``; the median of ``--rounds`` after one warm-up each
``parts_sum_ms`` is ``folds * (epochs * epoch + held-out pass)``: what the audit would cost if it were nothing but its
batches; the rest is per fold set-up (``subset``, the model, the trainer, the eval-mode handle) and the final read.
Times are host-clock milliseconds around work that ends in a device synchronise.  One JSON line per (bank, mode).
Usage: python tools/bench_audit.py [--clips 4096] [--model-type small] [--folds 5] [--epochs 20] [--batch-size 32]
                                   [--p-augment 0.3] [--rounds 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import audit_ref                                       # noqa: E402  (the test corpus' seeds and flips)
import cough_detector_amd as cda                      # noqa: E402
from cough_detector_amd import synth                  # noqa: E402
from cough_detector_amd import train as train_mod     # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def summary(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def test_corpus():
    seeds, _, given, _ = audit_ref.synth_corpus()
    return cda.DeviceClipBank([synth.make_clip(s) for s in seeds], given.tolist())


def device_corpus(count):
    """``count`` clips of 16000 samples generated where they stay, seeds 0 .. count - 1."""
    clips = synth.device_clips(0, count)
    return cda.DeviceClipBank.from_packed(clips.reshape(-1), [synth.N] * count, [int(s % 6 == 0) for s in range(count)])


def parts(bank, pre, a, p_augment, draws, rounds):
    """Fold 0 of the audit, built as ``out_of_fold_scores`` builds it: (epoch summary, held-out pass summary, steps)."""
    fold = cda.stratified_kfold(bank.labels, a.folds)
    held = np.flatnonzero(fold == 0)
    train_bank, held_bank = bank.subset(np.flatnonzero(fold != 0).tolist()), bank.subset(held.tolist())
    audio = spec = None
    if p_augment:
        audio = cda.AudioAugmentor(sample_rate=pre.sample_rate, p_augment=p_augment)
        spec = cda.SpecAugment(freq_mask_param=8, time_mask_param=15, n_freq_masks=2, n_time_masks=2, p=p_augment)
    train_loader, held_loader = cda.create_data_loaders(train_bank, held_bank, pre, batch_size=a.batch_size,
                                                        use_weighted_sampler=True, audio_augmentor=audio, spec_augmentor=spec,
                                                        draws=draws, generator=torch.Generator().manual_seed(0))
    torch.manual_seed(0)
    model = cda.create_model(a.model_type, n_mels=pre.get_num_features(), num_classes=2, in_channels=1)
    trainer = train_mod._TRAINERS[a.model_type](model, class_weights=cda.class_weights_from_counts(train_bank.class_counts))
    epoch_ms = [timed(lambda: cda.train_epoch_async(trainer, train_loader, r))[0] for r in range(rounds + 1)][1:]
    prob = torch.empty((len(bank), 2), dtype=torch.float32, device=bank.device)
    rows = torch.from_numpy(held).to(bank.device)

    @torch.no_grad()
    def held_pass():
        model.eval()
        at = 0
        for inputs, _ in held_loader:
            p = torch.softmax(model(inputs), dim=1)
            prob.index_copy_(0, rows[at:at + p.shape[0]], p)
            at += p.shape[0]

    held_ms = [timed(held_pass)[0] for _ in range(rounds + 1)][1:]
    return summary(epoch_ms), summary(held_ms), len(train_loader)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=4096)
    ap.add_argument("--model-type", default="small")
    ap.add_argument("--folds", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--p-augment", type=float, default=0.3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_audit.py needs the MI355X; there is nothing to time without it")
    torch.cuda.set_device(0)
    pre = cda.AudioPreprocessor(device="cuda", **train_mod.preprocessor_config())
    lines = []
    for name, bank in (("test_corpus_180", test_corpus()), (f"device_clips_{a.clips}", device_corpus(a.clips))):
        for p_augment, draws in ((0.0, "host"), (a.p_augment, "host"), (a.p_augment, "device")):
            kw = dict(model_type=a.model_type, folds=a.folds, batch_size=a.batch_size, p_augment=p_augment, draws=draws)
            cda.audit_labels(bank, pre, epochs=1, **kw)                           # warm-up: code objects, workspaces
            audit_ms, results = [], []
            for _ in range(a.rounds):
                ms, (scores, issues) = timed(lambda: cda.audit_labels(bank, pre, epochs=a.epochs, **kw))
                audit_ms.append(ms)
                results.append(scores.prob)
            assert all(torch.equal(results[0], r) for r in results[1:]), "an audit did not repeat itself"
            epoch, held, steps = parts(bank, pre, a, p_augment, draws, a.rounds)
            rec = {"bank": name, "clips": len(bank), "model": a.model_type, "folds": a.folds, "epochs": a.epochs,
                   "batch": a.batch_size, "p_augment": p_augment, "draws": draws, "steps_per_epoch": steps,
                   "training_steps": a.folds * a.epochs * steps, "rounds": a.rounds, "audit": summary(audit_ms),
                   "train_epoch_async": epoch, "held_out_pass": held,
                   "parts_sum_ms": round(a.folds * (a.epochs * epoch["median_ms"] + held["median_ms"]), 3),
                   "suspects": len(issues), "noise_rate": issues.noise_rate, "runs_equal": True}
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
