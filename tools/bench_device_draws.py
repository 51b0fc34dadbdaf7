"""Times the batch loader with its draws on the host against its draws on the device (``DeviceDataLoader(draws=...)``) on
the MI355X; writes profiles/device_draws_bench.txt.

The setup is bench_data_loader.py's: one epoch is ``--batches`` batches of B clips over a synthetic bank (clips of 0.5-3 s),
both augmentors at p = 0.5, the shipped featuriser flags.  Per batch size, for ``draws="host"`` and ``draws="device"``:

  (a)  the loader alone: iterate one epoch, synchronise once at the end
  (b)  the loader feeding ``train_epoch_async`` on a SmallTrainer
  (b0) ``train_epoch_async`` on the same number of pre-made device batches: the floor of (b)

Both modes run in the same process and alternate epoch by epoch (host, device, host, ...), so that whatever else the
machine is doing falls on both; every figure is a host clock around work that ends in a device synchronise, after a
warm-up epoch of each, and the median of ``--repeats`` epochs with the smallest and largest next to it.  The last
section splits the host time of ``launch_batch_drawn`` (enqueueing only: nothing in it waits for the device) over its
steps.  Usage: python tools/bench_device_draws.py [--out FILE]
"""
from __future__ import annotations

import argparse
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import cough_detector_amd as cda                                   # noqa: E402
from cough_detector_amd import data as cdata, draws as cdraws, synth          # noqa: E402
from cough_detector_amd.hostcpu import bound_torch_threads         # noqa: E402
from cough_detector_amd.training import SmallTrainer               # noqa: E402

SHIPPED = dict(use_pcen=False, use_pre_emphasis=False, use_delta_delta=False, use_spectral_contrast=False)


def synthetic_bank(n_clips: int, seed: int) -> cda.DeviceClipBank:
    """``n_clips`` clips of 8000..48000 samples cut from one run of device-generated synthetic audio."""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(8000, 48001, size=n_clips).tolist()
    labels = (rng.random(n_clips) < 0.25).astype(int).tolist()
    total = sum(lengths)
    audio = synth.device_clips(seed, (total + synth.N - 1) // synth.N).reshape(-1)[:total]
    return cda.DeviceClipBank.from_packed(audio, lengths, labels)


def once(fn) -> float:
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def fmt(name: str, times, batches: int) -> str:
    ms = sorted(t * 1e3 for t in times)
    med = statistics.median(ms)
    return (f"  {name:<58} median {med:9.1f} ms  min {ms[0]:9.1f}  max {ms[-1]:9.1f}  "
            f"({med / batches:7.3f} ms per batch)")


def host_split(loader, batches: int):
    """Host seconds per batch inside ``launch_batch_drawn`` by step, over one epoch (the device is not waited for)."""
    spent = {}

    def timed(owner, name, label):
        inner = getattr(owner, name)

        def wrapper(*a, **kw):
            t0 = time.perf_counter()
            out = inner(*a, **kw)
            spent[label] = spent.get(label, 0.0) + time.perf_counter() - t0
            return out
        setattr(owner, name, wrapper)
        return lambda: setattr(owner, name, inner)

    undo = [timed(cdata, "_upload", "index arithmetic's upload (_upload)"),
            timed(cdraws, "draw_batch", "draw_batch"), timed(cdraws, "augment_rows_drawn", "augment_rows_drawn"),
            timed(loader.preprocessor, "featurize_batch", "featurize_batch"), timed(cdata, "mask_images", "mask_images")]
    inner = loader.launch_batch_drawn

    def whole(*a, **kw):
        t0 = time.perf_counter()
        out = inner(*a, **kw)
        spent["launch_batch_drawn, all of it"] = spent.get("launch_batch_drawn, all of it", 0.0) + time.perf_counter() - t0
        return out
    loader.launch_batch_drawn = whole
    try:
        t0 = time.perf_counter()
        for _ in loader:
            pass
        spent["the epoch's iteration (sampler and seed included)"] = time.perf_counter() - t0
        torch.cuda.synchronize()
    finally:
        del loader.launch_batch_drawn
        for u in undo:
            u()
    return {k: v / batches for k, v in spent.items()}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_draws_bench.txt"))
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch-sizes", type=int, nargs="+", default=[32, 256])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_device_draws.py needs the MI355X; there is no CPU fallback")
    if args.repeats < 5:
        raise SystemExit("bench_device_draws.py: medians of fewer than 5 epochs are not reported")
    bound_torch_threads()
    pre = cda.AudioPreprocessor(device="cuda", **SHIPPED)
    lines = [f"batch loader, draws on the host against draws on the device; {args.batches} batches per epoch, the two modes "
             f"alternating, median of {args.repeats} epochs each after one warm-up epoch each; {torch.cuda.get_device_name(0)}",
             "clips of 0.5-3 s (8000..48000 samples), AudioAugmentor(p_augment=0.5) + SpecAugment(p=0.5), noise='device'"]
    for b in args.batch_sizes:
        bank = synthetic_bank(args.batches * b, seed=1000 + b)
        aug, spec = cda.AudioAugmentor(p_augment=0.5), cda.SpecAugment(p=0.5)
        loaders = {mode: cda.DeviceDataLoader(bank, pre, batch_size=b, audio_augmentor=aug, spec_augmentor=spec, draws=mode,
                                              generator=torch.Generator().manual_seed(b)) for mode in ("host", "device")}
        assert all(len(ld) == args.batches for ld in loaders.values())
        random.seed(b); torch.manual_seed(b)
        torch.manual_seed(0)
        model = cda.create_model("small", n_mels=90, num_classes=2, in_channels=1, compute_dtype="fp32")
        trainer = SmallTrainer(model, class_weights=cda.class_weights_from_counts(bank.class_counts), seed=1)
        premade = [(f.clone(), t.clone()) for f, t in loaders["device"]]

        def alone(mode):
            for _ in loaders[mode]:
                pass

        runs = {("a", "host"): lambda: alone("host"), ("a", "device"): lambda: alone("device"),
                ("b", "host"): lambda: cda.train_epoch_async(trainer, loaders["host"], 0),
                ("b", "device"): lambda: cda.train_epoch_async(trainer, loaders["device"], 0),
                ("b0", ""): lambda: cda.train_epoch_async(trainer, premade, 0)}
        for fn in runs.values():                                   # warm-up: code objects, allocator, workspaces
            once(fn)
        times = {k: [] for k in runs}
        for _ in range(args.repeats):                              # host, device, host, device, floor; then again
            for k, fn in runs.items():
                times[k].append(once(fn))
        med = {k: statistics.median(v) for k, v in times.items()}
        lines += [f"B = {b}  (bank: {len(bank)} clips, {bank.data.numel() * 4 / 2**30:.2f} GiB)",
                  fmt("(a)  loader alone, draws='host'", times["a", "host"], args.batches),
                  fmt("(a)  loader alone, draws='device'", times["a", "device"], args.batches),
                  fmt("(b)  loader -> train_epoch_async (Small), draws='host'", times["b", "host"], args.batches),
                  fmt("(b)  loader -> train_epoch_async (Small), draws='device'", times["b", "device"], args.batches),
                  fmt("(b0) pre-made device batches -> train_epoch_async (Small)", times["b0", ""], args.batches),
                  f"  host / device: (a) {med['a', 'host'] / med['a', 'device']:.2f}x   (b) {med['b', 'host'] / med['b', 'device']:.2f}x"
                  f"    (b) / (b0): host {med['b', 'host'] / med['b0', '']:.3f}  device {med['b', 'device'] / med['b0', '']:.3f}"
                  f"    (b0) spread max / min = {max(times['b0', '']) / min(times['b0', '']):.3f}"]
        split = host_split(loaders["device"], args.batches)
        lines.append(f"  host time inside launch_batch_drawn per batch at B = {b} (enqueueing; one epoch, the device not waited for):")
        lines += [f"    {k:<52} {v * 1e3:7.3f} ms" for k, v in split.items()]
        del premade, bank, loaders
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
