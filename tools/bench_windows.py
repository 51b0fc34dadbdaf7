"""Times the composed windows (cough_detector_amd/windows.py) on the MI355X; writes profiles/windows_bench.txt.

Banks: 64 synthetic backgrounds of 30 s and 256 synthetic coughs of 0.3..0.8 s, so that a cough fits inside a row
(gaussian noise, the coughs under a Hann window; kernel time does not depend on the samples).  The two sides of every comparison run
alternately, round by round, in one process; medians of ``--rounds`` (15) rounds after ``--warmup`` rounds.  Steps
(``--steps``):

  compose  ``compose_windows`` at B = 32 and B = 4096 rows of 16000 samples, every second row holding one cough that lies
           inside the row, against ``compose_scenes`` on the equivalent ``ScenePlan`` (two ``cough_span_power``,
           ``cough_scene_gains``, ``cough_mix_scenes`` and their uploads).  Per side: the whole call by the host clock (it
           ends in a synchronise) and by device events around it (the first kernel's start to the last one's end, host
           gaps between launches included); for the new kernel also the launch alone on plans that are on the device
           already.  The algorithmic bytes -- the row's background in, the row out, the visible event samples in -- per
           second of the launch alone, against the 8 TB/s HBM peak.
  epoch    16 batches of 32 from ``ComposedWindowLoader`` against a ``DeviceDataLoader`` over a bank made beforehand of the
           same 512 rows, both with ``AudioAugmentor(p_augment=0.5)`` and ``SpecAugment()``, in both ``draws`` modes:
           iterated alone (host clock, one synchronise at the end) and feeding ``train_epoch_async`` of a Small trainer.

Run it under a time limit, e.g. ``timeout -k 10 400 python tools/bench_windows.py``.
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
from cough_detector_amd import _lib                               # noqa: E402
from cough_detector_amd import windows as cwin                    # noqa: E402
from cough_detector_amd.hostcpu import bound_torch_threads        # noqa: E402

SR, WIDTH, HBM_PEAK, L3 = 16000, 16000, 8.0e12, 256 * 2**20
SHIPPED = dict(use_pcen=False, use_pre_emphasis=False, use_delta_delta=False, use_spectral_contrast=False)


def flat_bank(data: torch.Tensor, lengths, label: int) -> cda.DeviceClipBank:
    return cda.DeviceClipBank.from_packed(data, lengths, [label] * len(lengths))


def timed(fn) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def host_time(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def fmt(name: str, times) -> str:
    ms = sorted(t * 1e3 for t in times)
    return f"  {name:<84} median {statistics.median(ms):8.3f} ms  min {ms[0]:8.3f}  max {ms[-1]:8.3f}"


def alternate(sides, rounds: int, warmup: int):
    """``sides``: ``[(name, clock, fn)]``; every round runs each side once, in order.  Returns ``{name: [seconds]}``."""
    times = {name: [] for name, _, _ in sides}
    for k in range(warmup + rounds):
        for name, clock, fn in sides:
            t = clock(fn)
            if k >= warmup:
                times[name].append(t)
    return times


def in_window_plans(backgrounds, coughs, b: int, seed: int):
    """``(WindowPlan, ScenePlan)`` of the same ``b`` rows: every second row one cough inside the row."""
    rng = np.random.default_rng(seed)
    bl, el = backgrounds.lengths.numpy().astype(np.int64), coughs.lengths.numpy().astype(np.int64)
    background = rng.integers(0, bl.size, b)
    start = rng.integers(0, bl[background])
    positive = np.arange(b) % 2 == 0
    clip = rng.integers(0, el.size, b)
    onset = rng.integers(0, WIDTH - el[clip] + 1)
    snr = rng.uniform(5, 20, b)
    slots = lambda v, fill: np.concatenate([np.where(positive, v, fill)[:, None], np.full((b, 3), fill, dtype=v.dtype)], axis=1)
    window = cda.WindowPlan(background, start, np.ones(b, np.float32), positive.astype(np.int64), slots(clip, -1), slots(onset, 0),
                            slots(snr, 0.0))
    rows = np.flatnonzero(positive)
    scene = cda.ScenePlan(background, start, np.ones(b, np.float32), np.full(b, WIDTH), rows, clip[rows], onset[rows], snr[rows])
    return window, scene, int(el[clip[rows]].sum())


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "windows_bench.txt"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--steps", nargs="+", default=["compose", "epoch"], choices=["compose", "epoch"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_windows.py needs the MI355X; there is no CPU fallback")
    bound_torch_threads()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(7)
    rng = np.random.default_rng(7)
    bg_lengths = [30 * SR] * 64
    ev_lengths = rng.integers(SR * 3 // 10, SR * 8 // 10 + 1, 256).tolist()
    backgrounds = flat_bank(torch.randn(sum(bg_lengths), device=dev, generator=gen) * 0.05, bg_lengths, 0)
    shape = torch.cat([torch.hann_window(n, periodic=False, device=dev) for n in ev_lengths])
    coughs = flat_bank(torch.randn(sum(ev_lengths), device=dev, generator=gen) * shape, ev_lengths, 1)
    bank_bytes = 4 * (backgrounds.data.numel() + coughs.data.numel())
    lines = [f"banks: {len(bg_lengths)} backgrounds and {len(ev_lengths)} coughs, {bank_bytes / 2**20:.0f} MiB together; rows of "
             f"{WIDTH} samples; {torch.cuda.get_device_name(0)}; medians of {args.rounds} alternating rounds after "
             f"{args.warmup} warm-up rounds"]

    if "compose" in args.steps:
        p_ev = cwin.event_powers(coughs)
        lib = _lib.load_windows()
        for b in (32, 4096):
            window, scene, ev_samples = in_window_plans(backgrounds, coughs, b, seed=b)
            out = torch.empty((b, WIDTH), dtype=torch.float32, device=dev)
            records = torch.from_numpy(window.records().view(np.int64).reshape(-1).copy()).to(dev)

            def launch():
                _lib.check_windows(lib.cough_compose_windows(
                    backgrounds.data.data_ptr(), backgrounds.data.numel(), backgrounds.offsets_dev.data_ptr(),
                    backgrounds.lengths_dev.data_ptr(), len(backgrounds), coughs.data.data_ptr(), coughs.data.numel(),
                    coughs.offsets_dev.data_ptr(), coughs.lengths_dev.data_ptr(), p_ev.data_ptr(), len(coughs), records.data_ptr(),
                    b, WIDTH, out.data_ptr(), None, None, None), "cough_compose_windows")

            new = lambda: cda.compose_windows(backgrounds, coughs, window, WIDTH, event_power=p_ev, out=out)
            old = lambda: cda.compose_scenes(backgrounds, coughs, scene)
            same = torch.equal(new().view(-1).view(torch.int32), old()[0].data.view(torch.int32))
            t = alternate([("new host", host_time, new), ("old host", host_time, old), ("new device", timed, new),
                           ("old device", timed, old), ("launch", timed, launch)], args.rounds, args.warmup)
            moved = 4 * (2 * b * WIDTH + ev_samples)
            m = statistics.median(t["launch"])
            touched = 4 * b * WIDTH + bank_bytes
            lines += [f"B = {b}: {b // 2} rows with one cough inside the row; both sides give the same bits: {same}",
                      fmt("compose_windows, whole call (plan check, one upload, one launch; host clock)", t["new host"]),
                      fmt("compose_scenes, whole call (plan check, uploads, four launches, a new bank; host clock)", t["old host"]),
                      fmt("compose_windows, device events around the call", t["new device"]),
                      fmt("compose_scenes, device events around the call", t["old device"]),
                      fmt("cough_compose_windows, the launch alone (plans on the device)", t["launch"]),
                      f"    host clock: compose_scenes / compose_windows = "
                      f"{statistics.median(t['old host']) / statistics.median(t['new host']):.2f}; device events: "
                      f"{statistics.median(t['old device']) / statistics.median(t['new device']):.2f}",
                      f"    algorithmic bytes {moved / 2**20:.1f} MiB (background in, row out, visible event samples in): "
                      f"{moved / m / 1e12:.3f} TB/s of the launch alone, {100 * moved / m / HBM_PEAK:.1f} % of the "
                      f"{HBM_PEAK / 1e12:.0f} TB/s peak",
                      f"    the banks and the rows written are {touched / 2**20:.0f} MiB together: "
                      + ("they fit the 256 MiB Infinity Cache, and the same call is repeated, so none of this is HBM traffic"
                         if touched <= L3 else
                         f"the {bank_bytes / 2**20:.0f} MiB of banks fit the 256 MiB Infinity Cache and are read from there once "
                         f"warm; the {4 * b * WIDTH / 2**20:.0f} MiB written go past it")]

    if "epoch" in args.steps:
        pre = cda.AudioPreprocessor(device="cuda", **SHIPPED)
        batches, b = 16, 32
        torch.manual_seed(0)
        trainer = cda.SmallTrainer(cda.create_model("small", n_mels=90, num_classes=2, in_channels=1), lr=1e-3, weight_decay=0.01, seed=0)
        for draws in ("host", "device"):
            make = lambda: dict(audio_augmentor=cda.AudioAugmentor(sample_rate=SR), spec_augmentor=cda.SpecAugment(), draws=draws)
            composed = cda.ComposedWindowLoader(backgrounds, coughs, pre, batch_size=b, batches_per_epoch=batches, seed=3, **make())
            plan = cda.draw_window_plan(backgrounds, coughs, batches * b, WIDTH, SR, 3, margin=composed.margin)
            rows = cda.compose_windows(backgrounds, coughs, plan, WIDTH)
            ready = cda.DeviceDataLoader(cda.DeviceClipBank.from_packed(rows.reshape(-1), [WIDTH] * (batches * b),
                                                                        plan.labels(coughs.labels)), pre, batch_size=b,
                                         is_training=True, use_weighted_sampler=False, **make())

            def alone(loader):
                return lambda: [None for _ in loader]

            def feeding(loader):
                return lambda: cda.train_epoch_async(trainer, loader, 0)

            t = alternate([("composed", host_time, alone(composed)), ("ready", host_time, alone(ready)),
                           ("composed+train", host_time, feeding(composed)), ("ready+train", host_time, feeding(ready))],
                          args.rounds, args.warmup)
            per = lambda name: statistics.median(t[name]) / batches * 1e3
            lines += [f"an epoch of {batches} batches of {b}, draws={draws!r}, AudioAugmentor(p_augment=0.5) and SpecAugment() (host clock)",
                      fmt("ComposedWindowLoader, iterated alone", t["composed"]),
                      fmt("DeviceDataLoader over a bank of the same rows, iterated alone", t["ready"]),
                      fmt("ComposedWindowLoader feeding train_epoch_async (Small)", t["composed+train"]),
                      fmt("DeviceDataLoader feeding train_epoch_async (Small)", t["ready+train"]),
                      f"    per batch: {per('composed'):.3f} against {per('ready'):.3f} ms alone "
                      f"(+{per('composed') - per('ready'):.3f}), {per('composed+train'):.3f} against {per('ready+train'):.3f} ms "
                      f"feeding the trainer (+{per('composed+train') - per('ready+train'):.3f})"]

    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
