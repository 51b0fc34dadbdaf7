"""Times room reverberation on the MI355X; writes profiles/reverb_bench.txt (and, with ``--steps precision``,
profiles/reverb_precision.txt).

Everything of a step runs in one process, the two sides of a comparison alternating run by run so that both see the same
box at the same time; medians of ``--repeats`` runs after ``--warmup`` warm-up runs each are reported.  Every step is a
run of its own under its own time limit, e.g.

    timeout -k 10 300 python tools/bench_reverb.py --steps kernel
    timeout -k 10 300 python tools/bench_reverb.py --steps prepare --append
    timeout -k 10 600 python tools/bench_reverb.py --steps loader --append
    timeout -k 10 300 python tools/bench_reverb.py --steps precision

  kernel     ``cough_reverb_rows`` on ``--rows`` rows of 16000 samples, ``out_len`` 16000, responses drawn by
             ``cough_draw_reverb`` (p = 1) from a 100-entry synthetic bank, device events around the launch, the output
             allocation included.  Beside it the same convolution from torch ops on the same GPU: ``torch.fft.rfft`` of the
             rows at 32768 points, the rows' spectra gathered from a bank of ``rfft`` spectra computed ahead of the
             clock, the product, ``torch.fft.irfft`` and the cut to 16000 columns.  The torch side therefore includes the
             zero padding inside rfft, the gather of 4096 x 16385 complex64, and every intermediate's allocation; it
             excludes the bank's own transform, as the kernel's side excludes ``cough_reverb_prepare``.
  prepare    ``cough_reverb_prepare`` for the 100-entry bank (one launch per response), host clock to synchronize.
  loader     a 32-row ``launch_batch`` / ``launch_batch_drawn``, an epoch of a ``DeviceDataLoader`` alone and the same epoch
             feeding ``train_epoch_async`` (SmallTrainer), each with and without ``reverb`` on the augmentor, in both draw
             modes, ``--clips`` synthetic 1 s clips at batch 32, a host clock around each.
  precision  the rows of the test batch (tests/reverb_ref.py): per row the RMS error against float64 of the device and of
             the float32 emulation computed here, both over the worst-case bound and over each other.
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
from cough_detector_amd import reverb as crev                     # noqa: E402
from cough_detector_amd import synth                              # noqa: E402
from cough_detector_amd.hostcpu import bound_torch_threads        # noqa: E402
from cough_detector_amd.training import SmallTrainer              # noqa: E402

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


def bench_kernel(args, lines) -> None:
    b, n = args.rows, 16000
    bank, table = cda.synth_rirs(args.bank, seed=1)
    x = ((torch.rand((b, n), generator=torch.Generator().manual_seed(1)) - 0.5) * 0.8).cuda()
    flat = x.reshape(-1)
    offs = (torch.arange(b, dtype=torch.int64) * n).cuda()
    lens = torch.full((b,), n, dtype=torch.int32).cuda()
    plans = cda.draw_reverb(7, lens, 1.0, bank)
    index = plans[:, 1].long()
    bank.workspace(x.device)
    padded = torch.zeros((len(bank), 32768), dtype=torch.float32, device="cuda")
    for k, h in enumerate(bank.taps):
        padded[k, :h.size] = torch.from_numpy(h).cuda()
    spectra = torch.fft.rfft(padded)                              # ahead of the clock, as cough_reverb_prepare is

    ours = lambda: crev.reverb_rows(flat, offs, lens, plans, n, bank)                                  # noqa: E731
    theirs = lambda: torch.fft.irfft(torch.fft.rfft(x, 32768) * spectra[index], 32768)[:, :n].contiguous()  # noqa: E731
    err = (ours() - theirs()).abs().max().item()
    for _ in range(args.warmup):
        ours(); theirs()
    t_o, t_t = [], []
    for _ in range(args.repeats):
        t_o.append(device_time(ours))
        t_t.append(device_time(theirs))
    used = int(torch.unique(index).numel())
    traffic = 4 * 2 * b * n + b * 131072                         # rows in and out, one spectrum per row
    hbm_floor = (4 * 2 * b * n + used * 131072) / HBM_PEAK
    med = statistics.median(t_o)
    lines += [f"  kernel: {b} rows of {n} samples, out_len {n}, responses drawn (p = 1) from a synthetic bank of {len(bank)} "
              f"({used} in use, {int(table[:, 2].min())} .. {int(table[:, 2].max())} taps); device events around the launches, "
              f"output allocations included; max |kernel - torch| = {err:.2e}",
              fmt("cough_reverb_rows", t_o),
              fmt("torch: rfft(32768), gathered spectra, product, irfft, cut", t_t),
              f"    torch / kernel = {statistics.median(t_t) / med:.2f}",
              f"    algorithmic traffic {traffic / 1e9:.3f} GB (rows in, rows out, one 128 KiB spectrum per row) = "
              f"{traffic / med / 1e12:.2f} TB/s at the median; from HBM at most the rows and the {used} spectra once, "
              f"{(4 * 2 * b * n + used * 131072) / 1e9:.3f} GB = {hbm_floor * 1e3:.3f} ms at the 8 TB/s peak: the kernel takes "
              f"{med / hbm_floor:.1f} x that, so it is bound by its LDS passes and barriers, not by HBM",
              f"    the {used} spectra are {used * 131072 / 1e6:.1f} MB, read {b / used:.0f} times each on average: they can only "
              "have come from L2 / the Infinity Cache (no counters were collected to confirm it)",
              "    not measured: measured RIRs, banks too large for the cache, long recordings (several spans per row)"]


def bench_prepare(args, lines) -> None:
    bank, _ = cda.synth_rirs(args.bank, seed=1)
    dev = torch.device("cuda", torch.cuda.current_device())
    taps = bank.device_taps(dev)
    ws = torch.empty(crev.bank_bytes(len(bank)), dtype=torch.uint8, device=dev)
    run = lambda: crev.prepare(taps, bank.offsets, bank.lengths, ws)                                   # noqa: E731
    for _ in range(args.warmup):
        run()
    times = [host_time(run) for _ in range(args.repeats)]
    lines += [f"  prepare: cough_reverb_prepare for {len(bank)} responses ({ws.numel() / 1e6:.1f} MB of workspace), one launch per "
              "response and the twiddle table's copy, host clock to synchronize", fmt("cough_reverb_prepare", times)]


def bench_loader(args, lines) -> None:
    pre = cda.AudioPreprocessor(device="cuda", **SHIPPED)
    audio = synth.device_clips(4100, args.clips).reshape(-1)
    bank = cda.DeviceClipBank.from_packed(audio, [synth.N] * args.clips, [k % 2 for k in range(args.clips)])
    room, _ = cda.synth_rirs(args.bank, seed=1)
    room.workspace(bank.device)
    lines.append(f"  loader: {args.clips} clips of {synth.N} samples at batch 32, waveform augmentation and SpecAugment at p = 0.5, "
                 f"a synthetic bank of {len(room)} responses, host clock; 'batch' is one 32-row launch_batch / launch_batch_drawn "
                 "(draws included), 'alone' iterates the loader for an epoch, 'training' feeds train_epoch_async (SmallTrainer)")
    for draws in ("host", "device"):
        torch.manual_seed(1)
        tr = SmallTrainer(cda.create_model("small", n_mels=90, num_classes=2, in_channels=1, compute_dtype="fp32"), seed=3, lr=1e-5)

        def loader(reverb):
            return cda.DeviceDataLoader(bank, pre, batch_size=32, audio_augmentor=cda.AudioAugmentor(p_augment=0.5, reverb=reverb),
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

        dry, wet = loader(None), loader(room)
        train = lambda ld: (lambda: cda.train_epoch_async(tr, ld, 0))    # noqa: E731
        for kind, run, repeats in (("batch", one_batch, args.repeats), ("alone", alone, args.loader_repeats),
                                   ("training", train, args.loader_repeats)):
            random.seed(1)
            for _ in range(max(1, args.warmup // 2)):
                run(dry)(); run(wet)()
            t_dry, t_wet = [], []
            for _ in range(repeats):
                t_dry.append(host_time(run(dry)))
                t_wet.append(host_time(run(wet)))
            ratio = statistics.median(t_wet) / statistics.median(t_dry)
            lines += [fmt(f"draws={draws}, {kind}: reverb=None", t_dry), fmt(f"draws={draws}, {kind}: reverb=bank", t_wet),
                      f"    with / without = {ratio:.4f} ({100 * (ratio - 1):+.2f} %)"
                      + (f", {len(dry)} batches per epoch" if kind != "batch" else "")]


def bench_precision(args) -> str:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import reverb_ref as R
    bank_h, rows, width, exp = R.expected()
    bank = cda.RirBank(bank_h)
    data = torch.from_numpy(np.concatenate([r["x"] for r in rows])).cuda()
    sizes = [r["x"].size for r in rows]
    offs = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)).cuda()
    lens = torch.tensor(sizes, dtype=torch.int32).cuda()
    y = crev.reverb_rows(data, offs, lens, crev.plan_array([(r["shift"], r["rir"], r["out_len"]) for r in rows], len(bank), width),
                         width, bank).cpu().numpy()
    lines = [f"reverb precision: the rows of tests/reverb_ref.py on {torch.cuda.get_device_name(0)}; per row the RMS error against the "
             "float64 convolution of the device (fma allowed) and of the float32 numpy emulation of the same algorithm (no fma), "
             f"the worst |error| / bound (K = {R.BOUND_K}) of both, and device RMS / emulation RMS (the test allows {R.RMS_FACTOR:g})",
             f"  {'row':<52} {'device RMS':>11} {'emul. RMS':>11} {'dev/bound':>10} {'emu/bound':>10} {'dev/emu':>8}"]
    worst = 0.0
    for r, (row, e) in enumerate(zip(rows, exp)):
        if row["rir"] < 0 or not row["out_len"]:
            continue
        dev, emu = R.rms_errors(y[r], row, e)
        if not emu:
            continue
        ok = np.isfinite(y[r][:row["out_len"]]) & np.isfinite(e["emu"]) & (e["bound"] > 0)
        over = lambda v: float((np.abs(v[:row["out_len"]][ok] - e["ref"][ok]) / e["bound"][ok]).max())   # noqa: E731
        lines.append(f"  {row['name']:<52} {dev:11.3e} {emu:11.3e} {over(y[r]):10.2e} {over(e['emu']):10.2e} {dev / emu:8.3f}")
        worst = max(worst, dev / emu)
    lines.append(f"  worst device RMS / emulation RMS: {worst:.3f}")
    return "\n".join(lines) + "\n"


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "reverb_bench.txt"))
    ap.add_argument("--precision-out", default=os.path.join("profiles", "reverb_precision.txt"))
    ap.add_argument("--append", action="store_true", help="append to --out instead of starting it anew")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--loader-repeats", type=int, default=5)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--bank", type=int, default=100)
    ap.add_argument("--clips", type=int, default=512)
    ap.add_argument("--steps", nargs="+", default=["kernel", "prepare", "loader"], choices=["kernel", "prepare", "loader", "precision"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_reverb.py needs the MI355X; there is no CPU fallback")
    bound_torch_threads()
    if "precision" in args.steps:
        text = bench_precision(args)
        print(text, end="")
        os.makedirs(os.path.dirname(os.path.abspath(args.precision_out)), exist_ok=True)
        with open(args.precision_out, "w") as f:
            f.write(text)
    lines = [] if args.append else [f"room reverberation: FFT overlap-save in LDS with a prepared bank; {torch.cuda.get_device_name(0)}"]
    for step, fn in (("kernel", bench_kernel), ("prepare", bench_prepare), ("loader", bench_loader)):
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
