"""Times the device-resident batch loader (cough_detector_amd/data.py) on the MI355X; writes profiles/data_loader_bench.txt.

One epoch is ``--batches`` batches of B clips over a synthetic bank (``cough_synth_clips`` audio cut into clips of
0.5-3 s), both augmentors at p = 0.5, the shipped featuriser flags.  Per batch size:

  (a)  the loader alone: iterate one epoch, synchronise once at the end
  (b)  the loader feeding ``train_epoch_async`` on a SmallTrainer
  (b0) ``train_epoch_async`` on the same number of pre-made device batches (what (b) would cost with a free loader)
  (c)  the per-clip public path producing such batches: ``augment -> normalize -> pad_or_trim -> extract_features ->
       SpecAugment`` per item, stacked; timed over ``--per-clip-batches`` batches and scaled to the epoch

Every figure is a host clock around work that ends in a device synchronise, after a warm-up epoch; the median of
``--repeats`` epochs with the smallest and largest next to it.  Usage: python bench_data_loader.py [--out FILE]
"""
from __future__ import annotations

import argparse
import os
import random
import statistics
import time

import numpy as np
import torch

import cough_detector_amd as cda
from cough_detector_amd import synth
from cough_detector_amd.hostcpu import bound_torch_threads
from cough_detector_amd.training import SmallTrainer

SHIPPED = dict(use_pcen=False, use_pre_emphasis=False, use_delta_delta=False, use_spectral_contrast=False)


def synthetic_bank(n_clips: int, seed: int) -> cda.DeviceClipBank:
    """``n_clips`` clips of 8000..48000 samples cut from one run of device-generated synthetic audio."""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(8000, 48001, size=n_clips).tolist()
    labels = (rng.random(n_clips) < 0.25).astype(int).tolist()
    total = sum(lengths)
    audio = synth.device_clips(seed, (total + synth.N - 1) // synth.N).reshape(-1)[:total]
    bank = object.__new__(cda.DeviceClipBank)
    bank.device = audio.device
    bank._set(audio, lengths, labels)
    return bank


def timed(fn, repeats: int):
    fn()                                    # warm-up: code objects, allocator, workspaces
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def fmt(name: str, times, batches: int, scale: float = 1.0) -> str:
    ms = sorted(t * 1e3 * scale for t in times)
    med = statistics.median(ms)
    return (f"  {name:<58} median {med:9.1f} ms  min {ms[0]:9.1f}  max {ms[-1]:9.1f}  "
            f"({med / batches:7.3f} ms per batch)")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "data_loader_bench.txt"))
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch-sizes", type=int, nargs="+", default=[32, 256])
    ap.add_argument("--per-clip-batches", type=int, nargs="+", default=[20, 3])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_data_loader.py needs the MI355X; there is no CPU fallback")
    bound_torch_threads()
    pre = cda.AudioPreprocessor(device="cuda", **SHIPPED)
    lines = [f"device-resident loader, {args.batches} batches per epoch, median of {args.repeats} epochs after one warm-up "
             f"epoch; {torch.cuda.get_device_name(0)}",
             "clips of 0.5-3 s (8000..48000 samples), AudioAugmentor(p_augment=0.5) + SpecAugment(p=0.5), noise='device'"]
    for b, n_c in zip(args.batch_sizes, args.per_clip_batches):
        bank = synthetic_bank(args.batches * b, seed=1000 + b)
        aug, spec = cda.AudioAugmentor(p_augment=0.5), cda.SpecAugment(p=0.5)
        loader = cda.DeviceDataLoader(bank, pre, batch_size=b, audio_augmentor=aug, spec_augmentor=spec,
                                      generator=torch.Generator().manual_seed(b))
        assert len(loader) == args.batches
        random.seed(b); torch.manual_seed(b)

        def loader_alone():
            for _ in loader:
                pass

        torch.manual_seed(0)
        model = cda.create_model("small", n_mels=90, num_classes=2, in_channels=1, compute_dtype="fp32")
        trainer = SmallTrainer(model, class_weights=cda.class_weights_from_counts(bank.class_counts), seed=1)
        premade = [(f.clone(), t.clone()) for f, t in loader]

        def per_clip():
            order = loader.epoch_indices()
            for k in range(n_c):
                feats = []
                for i in order[k * b:(k + 1) * b]:
                    w = pre.pad_or_trim(pre.normalize(aug.augment(bank.clip(i))))
                    feats.append(spec(pre.extract_features(w)))
                torch.stack(feats)

        a = timed(loader_alone, args.repeats)
        b1 = timed(lambda: cda.train_epoch_async(trainer, loader, 0), args.repeats)
        b0 = timed(lambda: cda.train_epoch_async(trainer, premade, 0), args.repeats)
        c = timed(per_clip, max(2, args.repeats // 2))
        med = lambda t: statistics.median(t)      # noqa: E731
        lines += [f"B = {b}  (bank: {len(bank)} clips, {bank.data.numel() * 4 / 2**30:.2f} GiB)",
                  fmt("(a)  loader alone", a, args.batches),
                  fmt("(b)  loader -> train_epoch_async (Small)", b1, args.batches),
                  fmt("(b0) pre-made device batches -> train_epoch_async (Small)", b0, args.batches),
                  fmt(f"(c)  per-clip public path ({n_c} batches timed, scaled to the epoch)", c, args.batches,
                      scale=args.batches / n_c),
                  f"  (c) / (a) = {med(c) * args.batches / n_c / med(a):.1f}x    (b) / (b0) = {med(b1) / med(b0):.3f}    "
                  f"(b0) spread max / min = {max(b0) / min(b0):.3f}"]
        del premade, bank, loader
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
