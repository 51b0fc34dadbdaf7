"""Times soft-target training on the MI355X; writes profiles/mixup_bench.txt.

Everything runs in one process, the two sides of a comparison alternating run by run so that both see the same box at the
same time; medians of ``--repeats`` runs after ``--warmup`` warm-up runs each are reported.

  steps   each trainer's soft step (``cough_train*_forward_backward_soft`` + AdamW) against its hard step at B = 32 and
          256 on 90 x 101 images, device events around one ``trainer.step``.  The hard step is timed twice per round
          (hard, soft, hard): the ratio of the two hard medians and the hard runs' own spread are the noise floor the
          soft / hard ratio is to be judged against.
  mix     ``cough_mix_batch`` (one launch, coefficients already on the device) against ``MixUp.mix_batch`` (two
          ``cough_mix_rows`` calls and two pageable coefficient copies) at B = 256, a host clock to a device synchronise.
  loader  an epoch of ``train_epoch_async`` (SmallTrainer) fed by a ``DeviceDataLoader`` with and without ``mixup``,
          ``--clips`` synthetic 1 s clips at batch 32, in both draw modes, a host clock around the epoch.

Run it under a time limit, e.g. ``timeout -k 10 400 python tools/bench_mixup.py``.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import cough_detector_amd as cda                                  # noqa: E402
from cough_detector_amd import synth                              # noqa: E402
from cough_detector_amd.augmentation import mix_batch_rows, mix_coefficients   # noqa: E402
from cough_detector_amd.hostcpu import bound_torch_threads        # noqa: E402
from cough_detector_amd.training import ResidualTrainer, SmallTrainer, StandardTrainer   # noqa: E402

SHIPPED = dict(use_pcen=False, use_pre_emphasis=False, use_delta_delta=False, use_spectral_contrast=False)
TRAINERS = (("residual", ResidualTrainer), ("small", SmallTrainer), ("standard", StandardTrainer))


def host_time(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def device_time(fn) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def fmt(name: str, times) -> str:
    ms = sorted(t * 1e3 for t in times)
    med = statistics.median(ms)
    return (f"  {name:<58} median {med:9.3f} ms  min {ms[0]:9.3f}  max {ms[-1]:9.3f}  "
            f"spread (max - min) / median {100 * (ms[-1] - ms[0]) / med:5.1f} %")


def bench_steps(args, lines) -> None:
    lines.append(f"  steps: one trainer.step (forward, backward, clip + AdamW), device events; per round hard, soft, hard; "
                 f"{args.repeats} rounds after {args.warmup} warm-up rounds")
    for name, cls in TRAINERS:
        for b in (32, 256):
            torch.manual_seed(1)
            model = cda.create_model(name, n_mels=90, num_classes=2, in_channels=1, compute_dtype="fp32")
            tr = cls(model, class_weights=[1.0, 2.5], seed=3, lr=1e-5)
            g = torch.Generator().manual_seed(b)
            x = torch.randn(b, 1, 90, 101, generator=g).cuda()
            t = torch.randint(0, 2, (b,), generator=g).cuda()
            lam = torch.from_numpy(np.random.RandomState(b).beta(0.2, 0.2, size=b)).float()
            y = torch.stack([lam, 1 - lam], dim=1).cuda().contiguous()
            hard, soft = (lambda: tr.step(x, t)), (lambda: tr.step(x, y))
            for _ in range(args.warmup):
                hard(); soft()
            t_h1, t_s, t_h2 = [], [], []
            for _ in range(args.repeats):
                t_h1.append(device_time(hard))
                t_s.append(device_time(soft))
                t_h2.append(device_time(hard))
            m1, ms, m2 = (statistics.median(v) for v in (t_h1, t_s, t_h2))
            mh = statistics.median(t_h1 + t_h2)
            lines += [fmt(f"{name} B={b} hard step (first of the round)", t_h1), fmt(f"{name} B={b} soft step", t_s),
                      fmt(f"{name} B={b} hard step (last of the round)", t_h2),
                      f"    soft / hard = {ms / mh:.4f}; hard (last) / hard (first) = {m2 / m1:.4f}: the soft step differs from the "
                      f"hard step by {100 * (ms / mh - 1):+.2f} %, two hard medians from each other by {100 * (m2 / m1 - 1):+.2f} %"]


def bench_mix(args, lines) -> None:
    b = 256
    g = torch.Generator().manual_seed(7)
    x = torch.randn(b, 1, 90, 101, generator=g).cuda()
    labels = torch.randint(0, 2, (b,), generator=g).cuda()
    onehot = torch.nn.functional.one_hot(labels, 2).float()
    perm = torch.randperm(b, generator=g)
    dperm = perm.to(torch.int32).cuda()
    mix = cda.MixUp(alpha=0.2)
    np.random.seed(0)
    coef = torch.from_numpy(mix_coefficients(np.random.beta(0.2, 0.2, size=b))).cuda()
    two_call = lambda: mix.mix_batch(x, onehot, perm)                 # noqa: E731
    one_launch = lambda: mix_batch_rows(x, labels, dperm, coef)         # noqa: E731
    for _ in range(args.warmup):
        two_call(); one_launch()
    t_two, t_one, t_dev = [], [], []
    for _ in range(args.repeats):
        t_two.append(host_time(two_call))
        t_one.append(host_time(one_launch))
        t_dev.append(device_time(one_launch))
    mbytes = 3 * x.numel() * 4 / 1e6
    lines += [f"  mix: B = {b} images of 90 x 101 ({mbytes:.1f} MB moved), host clock to a device synchronise",
              fmt("MixUp.mix_batch (2 cough_mix_rows calls, pageable copies)", t_two),
              fmt("cough_mix_batch (1 launch, device coefficients)", t_one),
              fmt("cough_mix_batch, device events", t_dev),
              f"    two calls / one launch = {statistics.median(t_two) / statistics.median(t_one):.2f}; the launch moves "
              f"{mbytes / 1e3 / statistics.median(t_dev):.0f} GB/s by the device events"]


def bench_loader(args, lines) -> None:
    pre = cda.AudioPreprocessor(device="cuda", **SHIPPED)
    audio = synth.device_clips(4100, args.clips).reshape(-1)
    bank = cda.DeviceClipBank.from_packed(audio, [synth.N] * args.clips, [k % 2 for k in range(args.clips)])
    lines.append(f"  loader: an epoch of train_epoch_async (SmallTrainer) over {args.clips} clips of {synth.N} samples at batch 32, "
                 "waveform augmentation and SpecAugment at p = 0.5, host clock around the epoch")
    for draws in ("host", "device"):
        torch.manual_seed(1)
        tr = SmallTrainer(cda.create_model("small", n_mels=90, num_classes=2, in_channels=1, compute_dtype="fp32"), seed=3, lr=1e-5)

        def loader(mixup):
            return cda.DeviceDataLoader(bank, pre, batch_size=32, audio_augmentor=cda.AudioAugmentor(p_augment=0.5),
                                        spec_augmentor=cda.SpecAugment(p=0.5), draws=draws,
                                        generator=torch.Generator().manual_seed(2), mixup=mixup)

        plain, mixing = loader(None), loader(cda.MixUp(alpha=0.2))
        run = lambda ld: (lambda: cda.train_epoch_async(tr, ld, 0))    # noqa: E731
        for _ in range(max(1, args.warmup // 2)):
            run(plain)(); run(mixing)()
        t_plain, t_mix = [], []
        for _ in range(args.loader_repeats):
            t_plain.append(host_time(run(plain)))
            t_mix.append(host_time(run(mixing)))
        ratio = statistics.median(t_mix) / statistics.median(t_plain)
        lines += [fmt(f"draws={draws}: loader without mixup", t_plain), fmt(f"draws={draws}: loader with mixup", t_mix),
                  f"    with / without = {ratio:.4f} ({100 * (ratio - 1):+.2f} %), {len(plain)} batches per epoch"]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "mixup_bench.txt"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--loader-repeats", type=int, default=7)
    ap.add_argument("--clips", type=int, default=512)
    ap.add_argument("--steps", nargs="+", default=["steps", "mix", "loader"], choices=["steps", "mix", "loader"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mixup.py needs the MI355X; there is no CPU fallback")
    bound_torch_threads()
    lines = [f"soft-target training and batch MixUp; {torch.cuda.get_device_name(0)}"]
    for step, fn in (("steps", bench_steps), ("mix", bench_mix), ("loader", bench_loader)):
        if step in args.steps:
            fn(args, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
