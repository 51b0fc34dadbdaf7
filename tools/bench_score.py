"""Times the offline scorer (cough_detector_amd/score.py) on the MI355X; writes profiles/score_bench.txt.

Workload: ``--clips`` (2048) recordings of ``--seconds`` (10) s of device-generated synthetic audio
(``synth.device_clips``) in one ``DeviceClipBank``: 37 windows each at a 0.25 s hop, 75,776 in all.  The classifier is
the residual net with random weights in ``bf16x3`` arithmetic, as ``bench.py`` runs it (kernel time does not depend on the weights).
Steps (``--steps``):

  score   (a) ``score_bank`` (window table, uploads, gather + pipeline per 4096 windows, smoothing), against the bare
          pipeline run over the same number of windows as pre-made contiguous (4096, 16000) batches.  The two are timed
          alternately, a host clock around work that ends in a device synchronise, ``--repeats`` times after
          ``--warmup`` warm-up runs each; the ratio of the medians is what gather, copies and smoothing cost.
  sweep   (c) ``sweep_thresholds`` at 101 thresholds (device events), against the host restatement
          (``tests/score_ref.py``: Python over the same smoothed values, decisions only) timed once.
  trace   (b) one ``score_bank`` + sweep + event list after a warm-up, for a run of the whole script under
          ``rocprofv3 --kernel-trace --stats`` (no counters in that run); ``--stats-csv`` then adds each kernel's share
          of the device time to the report.

Run it under a time limit, e.g. ``timeout -k 10 400 python tools/bench_score.py``.
"""
from __future__ import annotations

import argparse
import csv
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cough_detector_amd as cda                                  # noqa: E402
from cough_detector_amd import synth                              # noqa: E402
from cough_detector_amd.hostcpu import bound_torch_threads        # noqa: E402

SHIPPED = dict(use_pcen=False, use_pre_emphasis=False, use_delta_delta=False, use_spectral_contrast=False)
BATCH = 4096


def synthetic_bank(n_clips: int, samples: int, seed: int) -> cda.DeviceClipBank:
    total = n_clips * samples
    audio = synth.device_clips(seed, (total + synth.N - 1) // synth.N).reshape(-1)[:total]
    return cda.DeviceClipBank.from_packed(audio, [samples] * n_clips, [k % 2 for k in range(n_clips)])


def host_time(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def device_times(fn, warmup: int, repeats: int):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e-3)
    return out


def fmt(name: str, times) -> str:
    ms = sorted(t * 1e3 for t in times)
    return f"  {name:<72} median {statistics.median(ms):9.3f} ms  min {ms[0]:9.3f}  max {ms[-1]:9.3f}"


def kernel_shares(path: str):
    rows = list(csv.DictReader(open(path)))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    out = [f"  (b) kernel shares of {total / 1e6:.3f} ms device time in the traced pass ({os.path.basename(path)}):"]
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"]))[:12]:
        name = r["Name"].replace("cough::(anonymous namespace)::", "").replace("cough::", "")
        name = name.split("(")[0][:66]
        out.append(f"    {name:<66} calls {int(r['Calls']):5d}  {float(r['TotalDurationNs']) / 1e6:9.3f} ms  "
                   f"{100 * float(r['TotalDurationNs']) / total:5.1f} %")
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "score_bench.txt"))
    ap.add_argument("--clips", type=int, default=2048)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--steps", nargs="+", default=["score", "sweep"], choices=["score", "sweep", "trace"])
    ap.add_argument("--stats-csv", default=None, help="kernel_stats.csv of a traced run: append the shares to the report")
    ap.add_argument("--append", action="store_true", help="append to --out instead of replacing it")
    args = ap.parse_args()
    lines = []
    if args.steps and not (args.stats_csv and args.steps == ["trace"]):
        if not torch.cuda.is_available():
            raise SystemExit("bench_score.py needs the MI355X; there is no CPU fallback")
        bound_torch_threads()
        pre = cda.AudioPreprocessor(device="cuda", **SHIPPED)
        model = cda.create_model("residual", n_mels=90, num_classes=2, in_channels=1, compute_dtype="bf16x3")
        model.load_state_dict(synth.random_state_dict(seed=5))
        pipe = cda.CoughPipeline(pre, model.cuda().eval())
        samples = int(round(args.seconds * pre.sample_rate))
        bank = synthetic_bank(args.clips, samples, seed=4100)
        scores = cda.score_bank(bank, pipe, batch=BATCH)
        n = int(scores.prob.numel())
        lines.append(f"offline scoring, {len(bank)} recordings of {samples} samples ({bank.data.numel() * 4 / 2**30:.2f} GiB), "
                     f"window {scores.window_samples} / hop {scores.hop_samples}: {n} windows, {BATCH} per pass; "
                     f"{torch.cuda.get_device_name(0)}")
    if "score" in args.steps:
        sizes = [min(BATCH, n - lo) for lo in range(0, n, BATCH)]
        batches = [synth.device_clips(5000 + k, b) for k, b in enumerate(sizes)]
        assert all(b.shape == (s, pre.segment_samples) and b.is_contiguous() for b, s in zip(batches, sizes))
        sink = torch.empty(n, dtype=torch.float32, device="cuda")

        def bare():
            lo = 0
            for b in batches:
                sink[lo:lo + b.shape[0]] = pipe.predict(b, normalize=True)[1][:, 1]
                lo += b.shape[0]

        def scored():
            cda.score_bank(bank, pipe, batch=BATCH)

        for _ in range(args.warmup):
            bare()
            scored()
        t_bare, t_score = [], []
        for _ in range(args.repeats):                                      # alternately: both see the same box at the same time
            t_bare.append(host_time(bare))
            t_score.append(host_time(scored))
        mb, ms = statistics.median(t_bare), statistics.median(t_score)
        ratio = ms / mb
        lines += [f"  (a) median of {args.repeats} alternating runs after {args.warmup} warm-up runs each, host clock to a device synchronise",
                  fmt(f"bare pipeline, {len(batches)} contiguous batches ({n} windows)", t_bare),
                  f"    {n / mb / 1e6:.2f} M windows/s",
                  fmt("score_bank (table, uploads, gather + pipeline per pass, smoothing)", t_score),
                  f"    {n / ms / 1e6:.2f} M windows/s; score_bank / bare pipeline = {ratio:.3f} "
                  f"({100 * (ratio - 1):+.1f} % for gather, copies and smoothing)"]
    if "sweep" in args.steps:
        import score_ref as R
        thresholds = np.linspace(0.0, 1.0, 101)
        t = device_times(lambda: cda.sweep_thresholds(scores, thresholds, debounce_seconds=0.5), args.warmup, args.repeats)
        sweep = cda.sweep_thresholds(scores, thresholds, debounce_seconds=0.5)
        t_events = device_times(lambda: cda.detect_events(scores, 0.5, debounce_seconds=0.5), args.warmup, args.repeats)
        smoothed = np.split(scores.smoothed.cpu().numpy(), scores.window_offsets.numpy()[1:-1])
        t0 = time.perf_counter()
        ref = R.sweep_ref(smoothed, thresholds.tolist(), sweep.gap)
        t_host = time.perf_counter() - t0
        same = sweep.counts.tolist() == ref["counts"] and sweep.first_window.tolist() == ref["first_window"]
        med = statistics.median(t)
        lines += [f"  (c) decisions for {n} windows at {thresholds.size} thresholds, debounce 0.5 s (gap {sweep.gap})",
                  fmt("sweep_thresholds, whole call (device events)", t),
                  fmt("detect_events at 0.5, whole call incl. the read of the counts", t_events),
                  f"    host restatement (tests/score_ref.py sweep_ref, one run): {t_host * 1e3:.1f} ms = {t_host / med:.0f} x the "
                  f"device call; counts and first windows equal: {same}; events fired over all thresholds: "
                  f"{int(sweep.counts.sum())}"]
    if "trace" in args.steps and not args.stats_csv:
        torch.cuda.synchronize()
        traced = cda.score_bank(bank, pipe, batch=BATCH)
        cda.sweep_thresholds(traced, np.linspace(0.0, 1.0, 101))
        cda.detect_events(traced, 0.5)
        torch.cuda.synchronize()
    if args.stats_csv:
        lines += kernel_shares(args.stats_csv)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
