"""Times pitch shift on the MI355X; writes profiles/pitch_shift_bench.txt (``--steps lock``: profiles/pitch_lock_bench.txt).

Everything runs in one process, the two sides of a comparison alternating run by run so that both see the same box at the
same time; medians of ``--repeats`` runs after ``--warmup`` warm-up runs each are reported.

  kernel  ``cough_stretch_rows`` and ``pitch_shift_rows`` on ``--rows`` rows of 16000 samples with semitones drawn by
          ``cough_draw_pitch`` (p = 1, the default range), device events around the launches.  Beside them the same
          chain composed from torch ops on the same GPU: ``torch.stft`` in float64, torchaudio's phase vocoder
          (``angle`` / ``cumsum``, no magnitude floor), ``torch.istft``, then ``warp_rows``.  torch has one rate per
          call, so the rows are grouped by their semitones and each group is one batched call; a baseline that cannot
          run is reported as such.
  loader  an epoch of a ``DeviceDataLoader`` alone, then the same epoch feeding ``train_epoch_async`` (SmallTrainer),
          each with and without ``pitch`` on the augmentor, in both draw modes, ``--clips`` synthetic 1 s clips at batch
          32, a host clock around the epoch.  The baseline is the same tree with ``pitch=False``.
  lock    identity phase locking (the mode bit of the stretch plans) against the plain stretch of the same build, same
          rows and semitones: ``cough_stretch_rows``, ``pitch_shift_rows`` and one 32-row ``launch_batch_drawn`` of a
          ``DeviceDataLoader`` whose every row draws a pitch coin.  With ``--parent-lib`` (another build of
          ``libcough_amd_pitch.so``, e.g. the parent commit's) the plain stretch of that library runs as a third side,
          its outputs are compared bit for bit with this build's plain rows, and its own spread is the yardstick.

Run it under a time limit, e.g. ``timeout -k 10 400 python tools/bench_pitch.py``.
"""
from __future__ import annotations

import argparse
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import cough_detector_amd as cda                                  # noqa: E402
from cough_detector_amd import _lib                               # noqa: E402
from cough_detector_amd import synth                              # noqa: E402
from cough_detector_amd import pitch as cpitch                    # noqa: E402
from cough_detector_amd import warp as cwarp                      # noqa: E402
from cough_detector_amd.hostcpu import bound_torch_threads        # noqa: E402
from cough_detector_amd.training import SmallTrainer              # noqa: E402

SHIPPED = dict(use_pcen=False, use_pre_emphasis=False, use_delta_delta=False, use_spectral_contrast=False)
RANGE = (-2, 2)


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


def torch_stretch(x64: torch.Tensor, rate: float, n_s: int, window: torch.Tensor) -> torch.Tensor:
    """torchaudio's phase_vocoder between torch.stft and torch.istft, float64: (b, n) -> (b, n_s)."""
    spec = torch.stft(x64, 512, 128, 512, window, center=True, pad_mode="reflect", return_complex=True)
    frames = spec.shape[-1]
    steps = torch.arange(0, frames, rate, device=x64.device, dtype=torch.float64)
    advance = torch.linspace(0, math.pi * 128, 257, device=x64.device, dtype=torch.float64)[:, None]
    phase_0 = spec[..., :1].angle()
    spec = torch.nn.functional.pad(spec, [0, 2])
    i0 = steps.long()
    alphas = steps - i0
    s0, s1 = spec.index_select(-1, i0), spec.index_select(-1, i0 + 1)
    phase = s1.angle() - s0.angle() - advance
    phase = phase - 2 * math.pi * torch.round(phase / (2 * math.pi))
    phase = torch.cat([phase_0, (phase + advance)[..., :-1]], dim=-1)
    mag = alphas * s1.abs() + (1 - alphas) * s0.abs()
    return torch.istft(torch.polar(mag, torch.cumsum(phase, dim=-1)), 512, 128, 512, window, length=n_s).float()


def bench_kernel(args, lines) -> None:
    b, n, sr = args.rows, 16000, 16000
    x = ((torch.rand((b, n), generator=torch.Generator().manual_seed(1)) - 0.5) * 0.8).cuda()
    flat = x.reshape(-1)
    offs = (torch.arange(b, dtype=torch.int64) * n).cuda()
    lens = torch.full((b,), n, dtype=torch.int32).cuda()
    stretch, back, n_s = cpitch.draw_pitch(7, lens, 1.0, RANGE, sr)
    width = cpitch.drawn_width(n, RANGE)
    rates = torch.from_numpy(stretch.cpu().numpy().view(cpitch._PLAN_DTYPE)["rate"].reshape(-1).copy())
    groups = [(float(r), torch.nonzero(rates == r).reshape(-1).cuda()) for r in sorted(set(rates.tolist()))]
    window = torch.hann_window(512, periodic=True, dtype=torch.float64, device="cuda")
    wide_offs = (torch.arange(b, dtype=torch.int64) * width).cuda()

    def torch_stretch_all():
        out = torch.zeros((b, width), dtype=torch.float32, device="cuda")
        for rate, rows in groups:
            if rate == 1.0:
                out[rows, :n] = x[rows]
            else:
                y = torch_stretch(x[rows].double(), rate, cpitch.stretched_length(n, rate), window)
                out[rows, :y.shape[1]] = y
        return out

    ours_stretch = lambda: cpitch.stretch_rows(flat, offs, lens, stretch, width)                      # noqa: E731
    ours_chain = lambda: cpitch.pitch_shift_rows(flat, offs, lens, stretch, back, n, width)           # noqa: E731
    torch_chain = lambda: cwarp.warp_rows(torch_stretch_all().reshape(-1), wide_offs, n_s, back, n)   # noqa: E731
    frames_out = sum(math.ceil((1 + n // 128) / r) * int(rows.numel()) for r, rows in groups if r != 1.0)
    lines += [f"  kernel: {b} rows of {n} samples, semitones drawn in {RANGE} (p = 1): "
              + ", ".join(f"{int(rows.numel())} rows at rate {r:.4f}" for r, rows in groups)
              + f"; stretched lengths {int(n_s.min())} .. {int(n_s.max())}, width {width}; device events around the "
              "launches, output allocations included"]
    baseline = None
    try:
        torch_chain()
        torch.cuda.synchronize()
        baseline = True
    except Exception as e:                                        # noqa: BLE001 -- reported, not hidden
        lines.append(f"  the torch baseline (torch.stft float64 -> vocoder -> torch.istft -> warp_rows) could not run here: "
                     f"{type(e).__name__}: {str(e).splitlines()[0] if str(e) else ''}")
    for _ in range(args.warmup):
        ours_stretch(); ours_chain()
        if baseline:
            torch_stretch_all(); torch_chain()
    t_s, t_c, t_ts, t_tc = [], [], [], []
    for _ in range(args.repeats):
        t_s.append(device_time(ours_stretch))
        t_c.append(device_time(ours_chain))
        if baseline:
            t_ts.append(device_time(torch_stretch_all))
            t_tc.append(device_time(torch_chain))
    med = statistics.median(t_s)
    lines += [fmt("cough_stretch_rows", t_s), fmt("pitch_shift_rows (stretch + warp)", t_c),
              f"    stretch: {frames_out / med / 1e6:.2f} M output frames/s, {med / b * 1e6:.2f} us per row of 1 s; "
              f"{4 * (b * n + b * width) / med / 1e9:.0f} GB/s read + written (the kernel is bound by its chain of float64 FFTs)"]
    if baseline:
        lines += [fmt("torch: stft, vocoder, istft (float64, grouped by rate)", t_ts),
                  fmt("torch: the same, then warp_rows", t_tc),
                  f"    stretch: torch / kernel = {statistics.median(t_ts) / med:.2f}; chain: torch / kernel = "
                  f"{statistics.median(t_tc) / statistics.median(t_c):.2f}  (the torch chain has no magnitude floor; it is timed, "
                  "not compared)"]


def bench_lock(args, lines) -> None:
    b, n, sr = args.rows, 16000, 16000
    x = ((torch.rand((b, n), generator=torch.Generator().manual_seed(1)) - 0.5) * 0.8).cuda()
    flat = x.reshape(-1)
    offs = (torch.arange(b, dtype=torch.int64) * n).cuda()
    lens = torch.full((b,), n, dtype=torch.int32).cuda()
    plain, back, _ = cpitch.draw_pitch(7, lens, 1.0, RANGE, sr)
    locked = cpitch.draw_pitch(7, lens, 1.0, RANGE, sr, phase_lock=True)[0]
    modes = locked.cpu().numpy().view(cpitch._PLAN_DTYPE)["reserved"].reshape(-1)
    width = cpitch.drawn_width(n, RANGE)
    lines += [f"  lock: {b} rows of {n} samples, semitones drawn in {RANGE} (p = 1), {int(modes.sum())} rows with semitones "
              f"(locked on the locked side), width {width}; device events around the launches, sides alternating"]
    sides = {"plain": lambda: cpitch.stretch_rows(flat, offs, lens, plain, width),
             "locked": lambda: cpitch.stretch_rows(flat, offs, lens, locked, width)}
    parent = None
    if args.parent_lib:
        parent = _lib.Library("pitch", _lib.LIBRARIES["pitch"].abi, _lib.LIBRARIES["pitch"].prototypes)
        parent.path = os.path.abspath(args.parent_lib)

        def stretch_parent():                                     # allocates its output, as stretch_rows does
            out = torch.empty((b, width), dtype=torch.float32, device="cuda")
            parent.check(parent.load().cough_stretch_rows(flat.data_ptr(), offs.data_ptr(), lens.data_ptr(), b, plain.data_ptr(),
                                                          out.data_ptr(), width, None, torch.cuda.current_stream().cuda_stream),
                         "cough_stretch_rows")
            return out
        sides = {"parent": stretch_parent, **sides}
        same = torch.equal(stretch_parent(), sides["plain"]())
        lines.append(f"  plain rows of this build against {args.parent_lib}: {'bit-identical' if same else 'NOT bit-identical'} on these {b} rows")
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        try:
            import pitch_lock_ref as L
            import pitch_ref as P
            cases = L.lock_cases()
            packed, offsets = P.pack(cases)
            t_src, t_offs = torch.from_numpy(packed).cuda(), torch.from_numpy(offsets).cuda()
            t_lens = torch.tensor([c[1].size for c in cases], dtype=torch.int32).cuda()
            t_plans = torch.from_numpy(cpitch.plan_array([(c[2], c[3]) for c in cases])).cuda()
            t_width = max(cpitch.stretched_length(c[1].size, c[3]) for c in cases)
            ours = cpitch.stretch_rows(t_src, t_offs, t_lens, t_plans, t_width)
            theirs = torch.empty_like(ours)
            parent.check(parent.load().cough_stretch_rows(t_src.data_ptr(), t_offs.data_ptr(), t_lens.data_ptr(), len(cases),
                                                          t_plans.data_ptr(), theirs.data_ptr(), t_width, None,
                                                          torch.cuda.current_stream().cuda_stream),
                         "cough_stretch_rows")
            same = bool((ours.view(torch.int32) == theirs.view(torch.int32)).all())
            lines.append(f"  the same on the {len(cases)} rows of the test batch (tests/pitch_lock_ref.py, NaN rows included): "
                         f"{'bit-identical' if same else 'NOT bit-identical'}")
        except ImportError as e:
            lines.append(f"  the test batch could not be loaded: {e}")
    sides["pitch_shift_rows, plain"] = lambda: cpitch.pitch_shift_rows(flat, offs, lens, plain, back, n, width)
    sides["pitch_shift_rows, locked"] = lambda: cpitch.pitch_shift_rows(flat, offs, lens, locked, back, n, width)
    for _ in range(args.warmup):
        for fn in sides.values():
            fn()
    times = {name: [] for name in sides}
    for _ in range(args.repeats):
        for name, fn in sides.items():
            times[name].append(device_time(fn))
    med = {name: statistics.median(t) for name, t in times.items()}
    spread = lambda t: (max(t) - min(t)) / statistics.median(t)                                        # noqa: E731
    for name, t in times.items():
        lines.append(fmt(name if "rows" in name else f"cough_stretch_rows, {name}", t))
    if parent is not None:
        lines.append(f"    plain / parent = {med['plain'] / med['parent']:.4f}; the parent's own spread (max - min) / median over "
                     f"{args.repeats} rounds: {100 * spread(times['parent']):.1f} %")
    lines.append(f"    cough_stretch_rows: locked / plain = {med['locked'] / med['plain']:.4f}; pitch_shift_rows: locked / plain = "
                 f"{med['pitch_shift_rows, locked'] / med['pitch_shift_rows, plain']:.4f}; the plain side's spread "
                 f"{100 * spread(times['plain']):.1f} %")
    # one 32-row batch of the loader, device draws, every row with a pitch coin
    pre = cda.AudioPreprocessor(device="cuda", **SHIPPED)
    audio = synth.device_clips(4100, 64).reshape(-1)
    bank = cda.DeviceClipBank.from_packed(audio, [synth.N] * 64, [k % 2 for k in range(64)])
    loaders = {lock: cda.DeviceDataLoader(bank, pre, batch_size=32, draws="device", generator=torch.Generator().manual_seed(2),
                                          audio_augmentor=cda.AudioAugmentor(p_augment=1.0, pitch=True, phase_lock=lock),
                                          spec_augmentor=cda.SpecAugment(p=0.5)) for lock in (False, True)}
    indices = list(range(32))
    for _ in range(args.warmup):
        for ld in loaders.values():
            ld.launch_batch_drawn(indices, 5)
    t_batch = {lock: [] for lock in loaders}
    for k in range(args.repeats):
        for lock, ld in loaders.items():
            t_batch[lock].append(host_time(lambda: ld.launch_batch_drawn(indices, 100 + k)))
    lines += [fmt("loader batch of 32 (launch_batch_drawn, p = 1), plain", t_batch[False]),
              fmt("loader batch of 32 (launch_batch_drawn, p = 1), locked", t_batch[True]),
              f"    loader batch: locked / plain = {statistics.median(t_batch[True]) / statistics.median(t_batch[False]):.4f} "
              "(host clock, launch to synchronize; 4 of 5 rows draw semitones)"]


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

        def loader(pitch):
            return cda.DeviceDataLoader(bank, pre, batch_size=32, audio_augmentor=cda.AudioAugmentor(p_augment=0.5, pitch=pitch),
                                        spec_augmentor=cda.SpecAugment(p=0.5), draws=draws,
                                        generator=torch.Generator().manual_seed(2))

        def alone(ld):
            def run():
                for _ in ld:
                    pass
            return run

        plain, pitched = loader(False), loader(True)
        train = lambda ld: (lambda: cda.train_epoch_async(tr, ld, 0))    # noqa: E731
        for kind, run in (("alone", alone), ("training", train)):
            for _ in range(max(1, args.warmup // 2)):
                run(plain)(); run(pitched)()
            t_plain, t_pitched = [], []
            for _ in range(args.loader_repeats):
                t_plain.append(host_time(run(plain)))
                t_pitched.append(host_time(run(pitched)))
            ratio = statistics.median(t_pitched) / statistics.median(t_plain)
            lines += [fmt(f"draws={draws}, {kind}: pitch=False", t_plain), fmt(f"draws={draws}, {kind}: pitch=True", t_pitched),
                      f"    with / without = {ratio:.4f} ({100 * (ratio - 1):+.2f} %), {len(plain)} batches per epoch"]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="profiles/pitch_shift_bench.txt, or profiles/pitch_lock_bench.txt for --steps lock")
    ap.add_argument("--parent-lib", default=None, help="another build of libcough_amd_pitch.so for the lock step's third side")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--loader-repeats", type=int, default=7)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--clips", type=int, default=512)
    ap.add_argument("--steps", nargs="+", default=["kernel", "loader"], choices=["kernel", "loader", "lock"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pitch.py needs the MI355X; there is no CPU fallback")
    bound_torch_threads()
    lines = [f"pitch shift: the per-row float64 phase vocoder and the resampler behind it; {torch.cuda.get_device_name(0)}"]
    if args.out is None:
        args.out = os.path.join("profiles", "pitch_lock_bench.txt" if args.steps == ["lock"] else "pitch_shift_bench.txt")
    for step, fn in (("kernel", bench_kernel), ("loader", bench_loader), ("lock", bench_lock)):
        if step in args.steps:
            fn(args, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
