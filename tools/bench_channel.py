"""Times the capture-channel step on the MI355X; writes profiles/channel_bench.txt (and, with ``--steps precision``,
profiles/channel_precision.txt).

Everything of a step runs in one process, the two sides of a comparison alternating run by run so that both see the same
box at the same time; medians of ``--repeats`` runs after ``--warmup`` warm-up runs each are reported.  No time here is a
pass/fail bar.  Every step is a run of its own under its own time limit, e.g.

    timeout -k 10 300 python tools/bench_channel.py --steps kernel
    timeout -k 10 600 python tools/bench_channel.py --steps loader --append
    timeout -k 10 300 python tools/bench_channel.py --steps precision

  kernel     ``cough_channel_rows`` on ``--rows`` rows of 16000 samples and on 32 rows (the latency a loader batch
             sees), 4-section entries drawn by ``cough_draw_channel`` (p = 1, p_clip = 0.3) from a synthetic bank, device
             events around the launch, the output allocation included.  Beside it the obvious alternative: the same
             cascades' impulse responses cut to 8193 taps in a ``RirBank`` through ``cough_reverb_rows`` (no ceiling there).
  loader     a 32-row ``launch_batch`` / ``launch_batch_drawn`` and an epoch of a ``DeviceDataLoader``, each with and without
             ``channel`` on the augmentor, in both draw modes, ``--clips`` synthetic 1 s clips at batch 32, a host clock.
  precision  the rows of the test batch (tests/channel_ref.py): per row the device's and the float64 emulation's largest
             error against the long-double recurrence in units of 2^-53 G peak(x), beside the bound's K.
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
sys.path.insert(0, ROOT)

import cough_detector_amd as cda                                  # noqa: E402
from cough_detector_amd import channel as cch                     # noqa: E402
from cough_detector_amd import reverb as crev                     # noqa: E402
from cough_detector_amd import synth                              # noqa: E402
from cough_detector_amd.hostcpu import bound_torch_threads        # noqa: E402

SHIPPED = dict(use_pcen=False, use_pre_emphasis=False, use_delta_delta=False, use_spectral_contrast=False)
HBM_PEAK = 8.0e12                                                 # bytes/s


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


def four_section_bank(n: int) -> cda.ChannelBank:
    """``synth_channels`` with exactly two peaks per entry: every cascade has 4 sections."""
    return cda.synth_channels(n, peaks=(2, 2), seed=1)[0]


def bench_kernel(args, lines) -> None:
    from scipy import signal
    n = 16000
    bank = four_section_bank(args.bank)
    impulse = np.zeros(crev.MAX_TAPS)
    impulse[0] = 1.0
    responses = [signal.sosfilt(s / s[:, 3:4], impulse).astype(np.float32) for s in bank.sos]
    left_out = max(float(np.abs(signal.sosfilt(s / s[:, 3:4], np.concatenate([impulse, np.zeros(65536)]))[crev.MAX_TAPS:]).max())
                   for s in bank.sos)
    rirs = cda.RirBank(responses)
    bank.blob()
    rirs.workspace()
    lines.append(f"  kernel: rows of {n} samples, 4-section entries drawn (p = 1, p_clip = 0.3) from a synthetic bank of {len(bank)}; device "
                 "events around the launches, output allocations included.  'reverb' is the same cascades' impulse responses cut to "
                 f"{crev.MAX_TAPS} taps in a RirBank through cough_reverb_rows: no ceiling, and the largest tap it drops is {left_out:.1e}")
    for b in (args.rows, 32):
        x = ((torch.rand((b, n), generator=torch.Generator().manual_seed(1)) - 0.5) * 0.8).cuda()
        flat = x.reshape(-1)
        offs = (torch.arange(b, dtype=torch.int64) * n).cuda()
        lens = torch.full((b,), n, dtype=torch.int32).cuda()
        plans = cda.draw_channel(7, b, 1.0, bank, 0.3, (0.25, 1.0))
        unclipped = plans.clone()
        unclipped[:, 1] = torch.tensor([1.0]).view(torch.int32).item()
        room = torch.zeros((b, 4), dtype=torch.int32, device="cuda")
        room[:, 1], room[:, 2] = plans[:, 0], n
        ours = lambda: cch.channel_rows(flat, offs, lens, plans, n, bank)                               # noqa: E731
        theirs = lambda: crev.reverb_rows(flat, offs, lens, room, n, rirs)                              # noqa: E731
        err = (cch.channel_rows(flat, offs, lens, unclipped, n, bank) - theirs()).abs().max().item()
        for _ in range(args.warmup):
            ours(); theirs()
        t_o, t_t = [], []
        for _ in range(args.repeats):
            t_o.append(device_time(ours))
            t_t.append(device_time(theirs))
        med = statistics.median(t_o)
        clipped = int((plans[:, 1].view(torch.float32) < 1.0).sum())
        traffic = 4 * b * n * (3 + 2 * clipped / b)              # the row in twice and out once; in and out again when it clips
        lines += [f"  {b} rows ({clipped} of them clip); max |unclipped kernel - reverb| = {err:.2e}",
                  fmt(f"cough_channel_rows, {b} rows", t_o), fmt(f"cough_reverb_rows, {b} rows", t_t),
                  f"    reverb / channel = {statistics.median(t_t) / med:.2f};  {med / b * 1e6:.2f} us per row;  algorithmic traffic "
                  f"{traffic / 1e9:.3f} GB = {traffic / med / 1e12:.2f} TB/s at the median ({traffic / HBM_PEAK * 1e3:.3f} ms at the 8 TB/s peak)"]
    lines.append("    not measured: one lane per row (the estimate behind the block-parallel design), LDS bank conflicts and occupancy "
                 "(no counters were collected), rows of several spans, measured microphones")


def bench_loader(args, lines) -> None:
    pre = cda.AudioPreprocessor(device="cuda", **SHIPPED)
    audio = synth.device_clips(4100, args.clips).reshape(-1)
    bank = cda.DeviceClipBank.from_packed(audio, [synth.N] * args.clips, [k % 2 for k in range(args.clips)])
    mics = four_section_bank(args.bank)
    mics.blob(bank.device)
    lines.append(f"  loader: {args.clips} clips of {synth.N} samples at batch 32, waveform augmentation and SpecAugment at p = 0.5, "
                 f"p_clip = 0.3, a synthetic bank of {len(mics)} 4-section entries, host clock; 'batch' is one 32-row launch_batch / "
                 "launch_batch_drawn (draws included), 'alone' iterates the loader for an epoch")
    for draws in ("host", "device"):
        def loader(channel):
            return cda.DeviceDataLoader(bank, pre, batch_size=32, audio_augmentor=cda.AudioAugmentor(p_augment=0.5, channel=channel),
                                        spec_augmentor=cda.SpecAugment(p=0.5), draws=draws,
                                        generator=torch.Generator().manual_seed(2))

        def one_batch(ld):
            indices = list(range(32))
            if draws == "device":
                return lambda: ld.launch_batch_drawn(indices, 5)
            return lambda: ld.launch_batch(indices, ld.draw_batch(indices))

        def alone(ld):
            def run():
                for _ in ld:
                    pass
            return run

        dry, wet = loader(None), loader(mics)
        for kind, run, repeats in (("batch", one_batch, args.repeats), ("alone", alone, args.loader_repeats)):
            random.seed(1)
            for _ in range(max(1, args.warmup // 2)):
                run(dry)(); run(wet)()
            t_dry, t_wet = [], []
            for _ in range(repeats):
                t_dry.append(host_time(run(dry)))
                t_wet.append(host_time(run(wet)))
            ratio = statistics.median(t_wet) / statistics.median(t_dry)
            lines += [fmt(f"draws={draws}, {kind}: channel=None", t_dry), fmt(f"draws={draws}, {kind}: channel=bank", t_wet),
                      f"    with / without = {ratio:.4f} ({100 * (ratio - 1):+.2f} %)"
                      + (f", {len(dry)} batches per epoch" if kind != "batch" else "")]
    lines.append("    not measured: the loader feeding a trainer, noise='host', banks of measured microphones")


def bench_precision(args) -> str:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import channel_ref as R
    cascades, rows = R.batch()
    bank = cda.ChannelBank.from_sos(cascades)
    data = torch.from_numpy(np.concatenate([r["x"] for r in rows])).cuda()
    sizes = [r["x"].size for r in rows]
    offs = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)).cuda()
    lens = torch.tensor(sizes, dtype=torch.int32).cuda()
    y = cch.channel_rows(data, offs, lens, cch.plans_to_device(R.plans_of(rows, False), data.device), R.WIDTH, bank).cpu().numpy()
    lines = [f"channel precision: the rows of tests/channel_ref.py on {torch.cuda.get_device_name(0)}, every ratio set to 1; per filtered "
             "row the largest error against the long-double recurrence beyond 2^-24 |y_ref|, in units of 2^-53 G peak(x), of the device "
             "(fma allowed), of the float64 numpy emulation of the same chunked scan (no fma) and of scipy.signal.sosfilt; "
             f"the bound's K = 16 x {R.EMULATE_UNITS:g} = {R.BOUND_K:g}",
             f"  {'row':<42} {'sections':>8} {'G':>8} {'device':>11} {'emulation':>11} {'sosfilt':>11} {'device / K':>11}"]
    worst_dev = worst_emu = 0.0
    from scipy import signal
    for r, row in enumerate(rows):
        if row["rule"] is not None or not row["x"].size:
            continue
        dev = R.units(y[r, :row["x"].size], row["ref"], row["g"], row["peak"])
        emu = R.units(R.emulate(row["x"], row["sos"]), row["ref"], row["g"], row["peak"])
        sos = R.units(signal.sosfilt(R.scipy_sos(row["sos"]), row["x"].astype(np.float64)), row["ref"], row["g"], row["peak"])
        worst_dev, worst_emu = max(worst_dev, dev), max(worst_emu, emu)
        lines.append(f"  {row['name']:<42} {len(row['sos']):8d} {row['g']:8.3g} {dev:11.4g} {emu:11.4g} {sos:11.4g} {dev / R.BOUND_K:11.2e}")
    lines.append(f"  largest: device {worst_dev:.4g}, emulation {worst_emu:.4g} units; K / device = {R.BOUND_K / max(worst_dev, 1e-300):.1f}")
    return "\n".join(lines) + "\n"


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "channel_bench.txt"))
    ap.add_argument("--precision-out", default=os.path.join("profiles", "channel_precision.txt"))
    ap.add_argument("--append", action="store_true", help="append to --out instead of starting it anew")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--loader-repeats", type=int, default=5)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--bank", type=int, default=100)
    ap.add_argument("--clips", type=int, default=512)
    ap.add_argument("--steps", nargs="+", default=["kernel", "loader"], choices=["kernel", "loader", "precision"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_channel.py needs the MI355X; there is no CPU fallback")
    bound_torch_threads()
    if "precision" in args.steps:
        text = bench_precision(args)
        print(text, end="")
        os.makedirs(os.path.dirname(os.path.abspath(args.precision_out)), exist_ok=True)
        with open(args.precision_out, "w") as f:
            f.write(text)
    lines = [] if args.append else [f"capture channel: biquad cascades run block-parallel by a scan over the workgroup, and the hard clip; "
                                    f"{torch.cuda.get_device_name(0)}"]
    for step, fn in (("kernel", bench_kernel), ("loader", bench_loader)):
        if step in args.steps:
            fn(args, lines)
    if lines != [] and (args.append or len(lines) > 1):
        text = "\n".join(lines) + "\n"
        print(text, end="")
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if args.append else "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
