"""The reference's training entry point (``src/train.py:215-572``): ``train(data_dir, output_dir, model_type, ...)`` and
its ``main()`` command line, assembled from what this package already runs on the MI355X.

``train`` builds the preprocessor and the augmentors of the reference's config block, reads the clips into
``DeviceClipBank``s (``prepare_dataset_split`` for the custom directory, ``DeviceClipBank.from_esc50`` with fold 5 held
out, ``DeviceClipBank.concat`` for both), wraps them in ``create_data_loaders``, builds the model and its HIP trainer and
hands all of it to ``fit``.  Nothing here launches a kernel of its own: the epoch loop is ``fit``'s.

    python -m cough_detector_amd.train --data-dir data --output-dir checkpoints --model-type small
"""
from __future__ import annotations

import json
import random
from pathlib import Path
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from .augmentation import AudioAugmentor, SpecAugment
from .data import DeviceClipBank, create_data_loaders, prepare_dataset_split
from .loop import class_weights_from_counts, fit
from .model import create_model
from .preprocessing import AudioPreprocessor
from .training import ResidualTrainer, SmallTrainer, StandardTrainer

MODEL_TYPES = ("standard", "small", "residual")                       # the reference's --model-type choices, in its order
_TRAINERS = {"small": SmallTrainer, "residual": ResidualTrainer, "standard": StandardTrainer}
_ESC50_VAL_FOLD = 5                                                   # src/train.py:357-374


def preprocessor_config() -> Dict:
    """The preprocessor keys of the reference's config block (``src/train.py:266-281``): what ``AudioPreprocessor``
    takes and ``CoughDetectorInference`` reads back from a checkpoint."""
    return dict(sample_rate=16000, n_mels=64, n_fft=512, hop_length=160, win_length=400, f_min=100.0, f_max=4000.0,
                segment_duration=1.0, n_mfcc=13, use_mfcc=True, use_pcen=False, use_pre_emphasis=False,
                pre_emphasis_coef=0.97, use_delta_delta=False, use_spectral_contrast=False, n_contrast_bands=6)


def train(data_dir: Optional[str], output_dir: str, model_type: str = "small", epochs: int = 100, batch_size: int = 32,
          learning_rate: float = 0.001, weight_decay: float = 0.01, patience: int = 15, device: str = "auto",
          num_workers: int = 4, resume: Optional[str] = None, use_esc50: bool = True, esc50_dir: Optional[str] = None, *,
          val_split: float = 0.2, random_state: int = 42, p_augment: float = 0.3, draws: str = "host",
          seed: Optional[int] = None) -> str:
    """The reference's ``train`` (``src/train.py:215-518``); the positional parameters are its own, in its order.

    ``data_dir``: a directory with ``non_cough/`` and ``cough/`` WAVE files, split 80 / 20 by ``prepare_dataset_split``
    (``val_split``, ``random_state``); skipped when it is None or does not exist.  ``use_esc50``: add the ESC-50 checkout
    at ``esc50_dir`` (default ``<data_dir>/../datasets/ESC-50-master``, or ``./datasets/ESC-50-master`` without a
    ``data_dir``), fold 5 for validation and the other folds for training, every non-cough class a negative.  Nothing is
    downloaded: a missing checkout raises ``FileNotFoundError``.  With both sources each side is the custom bank followed
    by the ESC-50 bank.  ``device``: ``"auto"`` or ``"cuda"``; there is no CPU fallback.  ``num_workers`` is accepted and
    ignored: the loader runs on the device.  ``p_augment``: the probability of ``AudioAugmentor`` and of ``SpecAugment``
    (the reference's 0.3).  ``draws``: the training loader's (``"host"`` or ``"device"``).  ``seed``: seeds ``random``,
    ``numpy`` and ``torch`` before the model is built, the sampler's generator and the trainer's dropout generator, so
    a run repeats itself bit for bit.

    Writes ``config.json``, ``latest_model.pt`` and ``best_model.pt`` (``fit``) and ``history.json`` (``fit``'s
    ``history``) into ``output_dir`` and returns ``str(Path(output_dir) / "best_model.pt")``; as in the reference, that
    file exists only once some epoch reached F1 > 0.

    Deviations from the reference.  Its ``CombinedDataset`` has neither ``sample_weights`` nor ``.samples``, so with both
    sources the reference falls back to shuffling and then fails when it counts the classes; here the combined bank is a
    bank, and gets the weighted sampler and its class counts like any other.  The reference writes the literals
    ``learning_rate`` 0.0005, ``epochs`` 150 and ``patience`` 20 into its config whatever was passed; that bug is not
    reproduced: the config holds the values actually used."""
    _train(data_dir, output_dir, model_type, epochs, batch_size, learning_rate, weight_decay, patience, device, resume,
           use_esc50, esc50_dir, val_split, random_state, p_augment, draws, seed)
    return str(Path(output_dir) / "best_model.pt")


def _train(data_dir, output_dir, model_type, epochs, batch_size, learning_rate, weight_decay, patience, device, resume,
           use_esc50, esc50_dir, val_split=0.2, random_state=42, p_augment=0.3, draws="host", seed=None,
           num_workers=None) -> Dict:
    """``train``'s work; returns ``fit``'s result (``main`` prints from it)."""
    if device not in ("auto", "cuda"):
        raise ValueError(f"train: device={device!r}; this build trains on the GPU only ('auto' or 'cuda'), there is no "
                         "CPU fallback")
    if model_type not in _TRAINERS:
        raise ValueError(f"train: unknown model type {model_type!r}; choose from {list(MODEL_TYPES)}")
    custom = bool(data_dir) and Path(data_dir).exists()
    if not custom and not use_esc50:
        raise ValueError("No training data found! Please provide data_dir or enable use_esc50")

    pre_config = preprocessor_config()
    config = dict(model_type=model_type, **pre_config, batch_size=batch_size, learning_rate=learning_rate,
                  weight_decay=weight_decay, epochs=epochs, patience=patience)
    preprocessor = AudioPreprocessor(device="cuda", **pre_config)
    audio_augmentor = AudioAugmentor(sample_rate=config["sample_rate"], p_augment=p_augment)
    spec_augmentor = SpecAugment(freq_mask_param=8, time_mask_param=15, n_freq_masks=2, n_time_masks=2, p=p_augment)

    train_banks, val_banks = [], []
    if custom:
        train_bank, val_bank = prepare_dataset_split(data_dir, preprocessor, val_split=val_split, random_state=random_state)
        train_banks.append(train_bank)
        val_banks.append(val_bank)
    if use_esc50:
        if esc50_dir is None:
            esc50_dir = str((Path(data_dir).parent if data_dir else Path(".")) / "datasets" / "ESC-50-master")
        for banks, is_training in ((train_banks, True), (val_banks, False)):
            banks.append(DeviceClipBank.from_esc50(esc50_dir, preprocessor, is_training=is_training, fold=_ESC50_VAL_FOLD,
                                                   include_all_negatives=True))
    train_bank = train_banks[0] if len(train_banks) == 1 else DeviceClipBank.concat(train_banks)
    val_bank = val_banks[0] if len(val_banks) == 1 else DeviceClipBank.concat(val_banks)

    generator = None
    if seed is not None:
        random.seed(seed)
        np.random.seed(seed)
        torch.manual_seed(seed)
        generator = torch.Generator().manual_seed(seed)
    train_loader, val_loader = create_data_loaders(train_bank, val_bank, preprocessor, batch_size=batch_size,
                                                   use_weighted_sampler=True, audio_augmentor=audio_augmentor,
                                                   spec_augmentor=spec_augmentor, draws=draws, generator=generator)
    model = create_model(model_type, n_mels=preprocessor.get_num_features(), num_classes=2, in_channels=1)
    trainer = _TRAINERS[model_type](model, lr=learning_rate, weight_decay=weight_decay,
                                    class_weights=class_weights_from_counts(train_bank.class_counts),
                                    seed=0 if seed is None else seed)
    result = fit(trainer, train_loader, val_loader, str(output_dir), epochs=epochs, patience=patience, config=config,
                 resume=resume)
    with open(Path(output_dir) / "history.json", "w") as f:
        json.dump(result["history"], f, indent=2)
    return result


def build_parser():
    import argparse
    parser = argparse.ArgumentParser(prog="python -m cough_detector_amd.train",
                                     description="Train cough detection model (MI355X path)")
    parser.add_argument("--data-dir", type=str, default=None, help="Directory with cough/non_cough subdirectories")
    parser.add_argument("--output-dir", type=str, default="./checkpoints", help="Directory to save checkpoints")
    parser.add_argument("--model-type", type=str, default="small", choices=list(MODEL_TYPES), help="Model architecture")
    parser.add_argument("--epochs", type=int, default=100, help="Maximum training epochs")
    parser.add_argument("--batch-size", type=int, default=32, help="Batch size")
    parser.add_argument("--lr", type=float, default=0.001, help="Learning rate")
    parser.add_argument("--weight-decay", type=float, default=0.01, help="Weight decay")
    parser.add_argument("--patience", type=int, default=15, help="Early stopping patience")
    parser.add_argument("--device", type=str, default="auto", help="Device (auto, cuda)")
    parser.add_argument("--num-workers", type=int, default=4, help="Accepted and ignored: the loader runs on the device")
    parser.add_argument("--resume", type=str, default=None, help="Resume from checkpoint")
    parser.add_argument("--no-esc50", action="store_true", help="Disable ESC-50 dataset")
    parser.add_argument("--esc50-dir", type=str, default=None, help="ESC-50 dataset directory (never downloaded)")
    parser.add_argument("--seed", type=int, default=None, help="Seed of initialisation, sampler, draws and dropout")
    parser.add_argument("--draws", type=str, default="host", choices=["host", "device"],
                        help="Where the training loader makes its per-item draws")
    parser.add_argument("--val-split", type=float, default=0.2, help="Share of the custom clips held out for validation")
    return parser


def train_kwargs(args) -> Dict:
    """The keyword arguments of ``train`` for parsed command-line ``args``."""
    return dict(data_dir=args.data_dir, output_dir=args.output_dir, model_type=args.model_type, epochs=args.epochs,
                batch_size=args.batch_size, learning_rate=args.lr, weight_decay=args.weight_decay, patience=args.patience,
                device=args.device, num_workers=args.num_workers, resume=args.resume, use_esc50=not args.no_esc50,
                esc50_dir=args.esc50_dir, val_split=args.val_split, draws=args.draws, seed=args.seed)


def main(argv: Optional[Sequence[str]] = None) -> dict:
    result = _train(**train_kwargs(build_parser().parse_args(argv)))
    report = {"best_model": result["best_model"], "best_f1": result["best_f1"], "epochs_run": result["epochs_run"]}
    print(json.dumps(report))
    return report


if __name__ == "__main__":
    main()
