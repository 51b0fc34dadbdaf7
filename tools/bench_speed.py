"""Times speed perturbation on the MI355X; writes profiles/speed_perturbation_bench.txt.

Everything runs in one process, the two sides of a comparison alternating run by run so that both see the same box at the
same time; medians of ``--repeats`` runs after ``--warmup`` warm-up runs each are reported.

  kernel  ``cough_warp_rows`` on ``--rows`` rows of 16000 samples with factors drawn by ``cough_draw_speed`` (p = 1,
          the default range), device events around the launch, and the bytes it moves (each row read once, the output
          matrix written once) against the 8 TB/s peak.  Beside it ``cough_resample`` on the same rows at the fixed pair
          (9, 10) -- the one existing kernel that computes the same thing, from a table -- and ``cough_warp_rows`` at that
          same fixed pair.
  loader  an epoch of a ``DeviceDataLoader`` alone, then the same epoch feeding ``train_epoch_async`` (SmallTrainer),
          each with and without ``speed`` on the augmentor, in both draw modes, ``--clips`` synthetic 1 s clips at batch
          32, a host clock around the epoch.  The baseline is the same tree with ``speed=False``.

Run it under a time limit, e.g. ``timeout -k 10 400 python tools/bench_speed.py``.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import cough_detector_amd as cda                                  # noqa: E402
from cough_detector_amd import _lib, _tables, synth               # noqa: E402
from cough_detector_amd import warp as cwarp                      # noqa: E402
from cough_detector_amd.hostcpu import bound_torch_threads        # noqa: E402
from cough_detector_amd.training import SmallTrainer              # noqa: E402

SHIPPED = dict(use_pcen=False, use_pre_emphasis=False, use_delta_delta=False, use_spectral_contrast=False)
PEAK = 8.0e12


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


def bench_kernel(args, lines) -> None:
    b, n, sr = args.rows, 16000, 16000
    x = ((torch.rand((b, n), generator=torch.Generator().manual_seed(1)) - 0.5) * 0.8).cuda()
    offs = (torch.arange(b, dtype=torch.int64) * n).cuda()
    lens = torch.full((b,), n, dtype=torch.int32).cuda()
    plans, new_lens = cwarp.draw_speed(7, lens, 1.0, (0.9, 1.1), sr)
    width = cwarp.drawn_width(n, (0.9, 1.1), sr)
    fixed = torch.tensor([[0, 9, 10]] * b, dtype=torch.int32).cuda()
    n_fixed = cwarp.warped_length(n, 9, 10)
    kern, w, o, m = _tables.sinc_resample_kernel(9, 10)
    table = kern.cuda()
    out_r = torch.empty((b, n_fixed), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    lib = _lib.load()
    drawn = lambda: cwarp.warp_rows(x, offs, lens, plans, width)                 # noqa: E731
    same = lambda: cwarp.warp_rows(x, offs, lens, fixed, n_fixed)                # noqa: E731
    table_run = lambda: _lib.check(lib.cough_resample(x.data_ptr(), n, b, n, table.data_ptr(), o, m, w, out_r.data_ptr(),   # noqa: E731
                                                      n_fixed, n_fixed, stream), "cough_resample")
    for _ in range(args.warmup):
        drawn(); same(); table_run()
    t_d, t_s, t_t = [], [], []
    for _ in range(args.repeats):
        t_d.append(device_time(drawn))
        t_s.append(device_time(same))
        t_t.append(device_time(table_run))
    moved_d = 4 * (b * n + b * width)
    moved_s = 4 * (b * n + b * n_fixed)
    md, ms_, mt = (statistics.median(v) for v in (t_d, t_s, t_t))
    taps = 2 * 7 + 2
    lines += [f"  kernel: {b} rows of {n} samples, device events around one launch (the output allocation included for "
              f"cough_warp_rows); new lengths {int(new_lens.min())} .. {int(new_lens.max())}, output width {width}",
              fmt("cough_warp_rows, drawn factors in (0.9, 1.1)", t_d),
              fmt("cough_warp_rows, every row (9, 10)", t_s),
              fmt("cough_resample, table of (9, 10)", t_t),
              f"    drawn factors: {moved_d / 1e6:.0f} MB read + written, {moved_d / md / 1e9:.0f} GB/s = "
              f"{100 * moved_d / md / PEAK:.2f} % of the 8 TB/s peak; {b * float(new_lens.float().mean()) * taps / md / 1e9:.1f} G "
              f"coefficients/s ({taps} taps per output, each evaluated in float64)",
              f"    fixed (9, 10): warp {moved_s / ms_ / 1e9:.0f} GB/s, table {moved_s / mt / 1e9:.0f} GB/s; warp / table = "
              f"{ms_ / mt:.2f}"]


def bench_loader(args, lines) -> None:
    pre = cda.AudioPreprocessor(device="cuda", **SHIPPED)
    audio = synth.device_clips(4100, args.clips).reshape(-1)
    bank = cda.DeviceClipBank.from_packed(audio, [synth.N] * args.clips, [k % 2 for k in range(args.clips)])
    lines.append(f"  loader: an epoch over {args.clips} clips of {synth.N} samples at batch 32, waveform augmentation and SpecAugment "
                 "at p = 0.5, host clock around the epoch; 'alone' iterates the loader, 'training' feeds train_epoch_async "
                 "(SmallTrainer)")
    for draws in ("host", "device"):
        torch.manual_seed(1)
        tr = SmallTrainer(cda.create_model("small", n_mels=90, num_classes=2, in_channels=1, compute_dtype="fp32"), seed=3, lr=1e-5)

        def loader(speed):
            return cda.DeviceDataLoader(bank, pre, batch_size=32, audio_augmentor=cda.AudioAugmentor(p_augment=0.5, speed=speed),
                                        spec_augmentor=cda.SpecAugment(p=0.5), draws=draws,
                                        generator=torch.Generator().manual_seed(2))

        def alone(ld):
            def run():
                for _ in ld:
                    pass
            return run

        plain, sped = loader(False), loader(True)
        train = lambda ld: (lambda: cda.train_epoch_async(tr, ld, 0))    # noqa: E731
        for kind, run in (("alone", alone), ("training", train)):
            for _ in range(max(1, args.warmup // 2)):
                run(plain)(); run(sped)()
            t_plain, t_sped = [], []
            for _ in range(args.loader_repeats):
                t_plain.append(host_time(run(plain)))
                t_sped.append(host_time(run(sped)))
            ratio = statistics.median(t_sped) / statistics.median(t_plain)
            lines += [fmt(f"draws={draws}, {kind}: speed=False", t_plain), fmt(f"draws={draws}, {kind}: speed=True", t_sped),
                      f"    with / without = {ratio:.4f} ({100 * (ratio - 1):+.2f} %), {len(plain)} batches per epoch"]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "speed_perturbation_bench.txt"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--loader-repeats", type=int, default=7)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--clips", type=int, default=512)
    ap.add_argument("--steps", nargs="+", default=["kernel", "loader"], choices=["kernel", "loader"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_speed.py needs the MI355X; there is no CPU fallback")
    bound_torch_threads()
    lines = [f"speed perturbation: the tableless per-row sinc resampler; {torch.cuda.get_device_name(0)}"]
    for step, fn in (("kernel", bench_kernel), ("loader", bench_loader)):
        if step in args.steps:
            fn(args, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
