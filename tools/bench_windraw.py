"""Times where ``ComposedWindowLoader`` draws its window plans (``plan_draws="host"`` against ``"device"``) on the MI355X;
writes profiles/windraw_bench.txt.

Banks as in tools/bench_windows.py: 64 synthetic backgrounds of 30 s and 256 synthetic coughs of 0.3..0.8 s.  The two
sides of every comparison run alternately, round by round, in one process; medians of ``--rounds`` (15) rounds after
``--warmup`` rounds, min..max beside them.  ``plan_draws="host"`` is the path the loader had before the device draw
existed, so the figures to hold the new path against are measured in the same run.  At B = 32 and B = 256, under both
inner ``draws`` modes, with ``AudioAugmentor(p_augment=0.5)`` and ``SpecAugment()`` behind the composer:

  alone     an epoch of 16 batches iterated alone (host clock, one synchronise at the end)
  feeding   the same epoch feeding ``train_epoch_async`` of a Small trainer

and per batch size the plan alone: ``draw_window_plan`` with its record packing (host clock) against the
``cough_draw_window_plans`` launch (device events, and the host clock of the call with its synchronise).

No time here is a pass/fail bar.  Run it under a time limit, e.g. ``timeout -k 10 400 python tools/bench_windraw.py``.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import cough_detector_amd as cda                                  # noqa: E402
from cough_detector_amd import windows as cwin                    # noqa: E402
from cough_detector_amd.hostcpu import bound_torch_threads        # noqa: E402
from bench_windows import SHIPPED, SR, WIDTH, alternate, flat_bank, fmt, host_time, timed   # noqa: E402

BATCHES = 16


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "windraw_bench.txt"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=15)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_windraw.py needs the MI355X; there is no CPU fallback")
    bound_torch_threads()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(7)
    rng = np.random.default_rng(7)
    bg_lengths = [30 * SR] * 64
    ev_lengths = rng.integers(SR * 3 // 10, SR * 8 // 10 + 1, 256).tolist()
    backgrounds = flat_bank(torch.randn(sum(bg_lengths), device=dev, generator=gen) * 0.05, bg_lengths, 0)
    shape = torch.cat([torch.hann_window(n, periodic=False, device=dev) for n in ev_lengths])
    coughs = flat_bank(torch.randn(sum(ev_lengths), device=dev, generator=gen) * shape, ev_lengths, 1)
    lines = [f"banks: {len(bg_lengths)} backgrounds and {len(ev_lengths)} coughs; rows of {WIDTH} samples; "
             f"{torch.cuda.get_device_name(0)}; medians of {args.rounds} alternating rounds after {args.warmup} warm-up rounds; "
             "plan_draws='host' is the loader's path before the device draw existed"]
    pre = cda.AudioPreprocessor(device="cuda", **SHIPPED)
    torch.manual_seed(0)
    trainer = cda.SmallTrainer(cda.create_model("small", n_mels=90, num_classes=2, in_channels=1), lr=1e-3, weight_decay=0.01, seed=0)
    per = lambda t, name: statistics.median(t[name]) / BATCHES * 1e3

    for b in (32, 256):
        tables = cwin.WindowDrawTables.build(coughs, (5, 20))
        margin = cda.edge_margin(cda.AudioAugmentor(sample_rate=SR), WIDTH)
        on_host = lambda: cda.draw_window_plan(backgrounds, coughs, b, WIDTH, SR, 3, margin=margin).records()
        on_device = lambda: cda.draw_window_records(backgrounds, coughs, b, WIDTH, 3, margin=margin, tables=tables)
        t = alternate([("host", host_time, on_host), ("device host clock", host_time, on_device), ("device", timed, on_device)],
                      args.rounds, args.warmup)
        lines += [f"B = {b}: the plan of one batch alone",
                  fmt("draw_window_plan and its records (numpy; host clock, nothing uploaded yet)", t["host"]),
                  fmt("draw_window_records, whole call (argument checks, one launch, a synchronise; host clock)", t["device host clock"]),
                  fmt("draw_window_records, device events around the call", t["device"])]
        for draws in ("host", "device"):
            make = lambda mode: cda.ComposedWindowLoader(backgrounds, coughs, pre, batch_size=b, batches_per_epoch=BATCHES, seed=3,
                                                         audio_augmentor=cda.AudioAugmentor(sample_rate=SR),
                                                         spec_augmentor=cda.SpecAugment(), draws=draws, plan_draws=mode)
            host, device = make("host"), make("device")
            alone = lambda loader: (lambda: [None for _ in loader])
            feeding = lambda loader: (lambda: cda.train_epoch_async(trainer, loader, 0))
            t = alternate([("host", host_time, alone(host)), ("device", host_time, alone(device)),
                           ("host+train", host_time, feeding(host)), ("device+train", host_time, feeding(device))],
                          args.rounds, args.warmup)
            lines += [f"B = {b}: an epoch of {BATCHES} batches, draws={draws!r}, AudioAugmentor(p_augment=0.5) and SpecAugment() (host clock)",
                      fmt("plan_draws='host', iterated alone", t["host"]),
                      fmt("plan_draws='device', iterated alone", t["device"]),
                      fmt("plan_draws='host' feeding train_epoch_async (Small)", t["host+train"]),
                      fmt("plan_draws='device' feeding train_epoch_async (Small)", t["device+train"]),
                      f"    per batch: {per(t, 'device'):.3f} against {per(t, 'host'):.3f} ms alone "
                      f"({per(t, 'device') - per(t, 'host'):+.3f}), {per(t, 'device+train'):.3f} against "
                      f"{per(t, 'host+train'):.3f} ms feeding the trainer ({per(t, 'device+train') - per(t, 'host+train'):+.3f})"]

    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
