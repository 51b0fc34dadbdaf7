"""Times the scenes (cough_detector_amd/scenes.py) on the MI355X; writes profiles/scenes_bench.txt.

Workload: ``--scenes`` (2048) scenes of ``--seconds`` (10) s with 4 coughs each at 5..20 dB, drawn by ``draw_scene_plan``
from 64 synthetic backgrounds of 30 s and 256 synthetic coughs of 1.0..1.5 s (gaussian noise under a Hann window; kernel
time does not depend on the samples).  Steps (``--steps``):

  mix     ``cough_mix_scenes`` alone (the launch, device events) against the same mix composed from torch ops on the GPU
          (a gather with computed cyclic indices, then one ``index_add_`` of the scaled event samples), timed
          alternately in one process, medians.  That composition is the plain one, not a tuned one: it builds an int64
          index for every output sample (2.4 GiB at the default size) and the events' index arrays inside the timed
          region, as a caller who holds only the plan would; bytes moved (scene samples in and out, event samples in) per second
          against the 8 TB/s HBM peak.  Also the whole of ``compose_scenes`` (uploads, four launches) by the host clock.
  power   ``cough_span_power`` over the scenes' background spans (device events), bytes read per second.
  match   ``match_events`` at 101 thresholds on planted probabilities (device events) against the Python restatement
          (``tests/scenes_ref.py`` ``match_ref``) timed once.

Run it under a time limit, e.g. ``timeout -k 10 400 python tools/bench_scenes.py``.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cough_detector_amd as cda                                  # noqa: E402
from cough_detector_amd import _lib                               # noqa: E402
from cough_detector_amd import scenes as cscenes                  # noqa: E402
from cough_detector_amd.hostcpu import bound_torch_threads        # noqa: E402

SR, HBM_PEAK = 16000, 8.0e12


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
    return f"  {name:<72} median {statistics.median(ms):9.3f} ms  min {ms[0]:9.3f}  max {ms[-1]:9.3f}"


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "scenes_bench.txt"))
    ap.add_argument("--scenes", type=int, default=2048)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--steps", nargs="+", default=["mix", "power", "match"], choices=["mix", "power", "match"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_scenes.py needs the MI355X; there is no CPU fallback")
    bound_torch_threads()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(7)
    rng = np.random.default_rng(7)
    bg_lengths = [30 * SR] * 64
    ev_lengths = rng.integers(SR, SR * 3 // 2 + 1, 256).tolist()
    backgrounds = flat_bank(torch.randn(sum(bg_lengths), device=dev, generator=gen) * 0.05, bg_lengths, 0)
    shape = torch.cat([torch.hann_window(n, periodic=False, device=dev) for n in ev_lengths])
    coughs = flat_bank(torch.randn(sum(ev_lengths), device=dev, generator=gen) * shape, ev_lengths, 1)
    plan = cda.draw_scene_plan(backgrounds, coughs, args.scenes, args.seconds, events_per_scene=(4, 4), seed=1)
    scenes, truth = cda.compose_scenes(backgrounds, coughs, plan)
    n, m, total = len(plan), len(truth), int(plan.length.sum())
    ev_samples = int((truth.offset - truth.onset).sum())
    lines = [f"scenes: {n} of {int(plan.length[0])} samples with {m} events ({ev_samples} event samples), "
             f"{scenes.data.numel() * 4 / 2**30:.2f} GiB out; {torch.cuda.get_device_name(0)}; medians of {args.repeats} "
             f"alternating runs after {args.warmup} warm-up runs"]

    if "mix" in args.steps:
        el, bl = coughs.lengths.numpy().astype(np.int64), backgrounds.lengths.numpy().astype(np.int64)
        tiles = cscenes.scene_tiles(plan.length)
        up = lambda a, t: torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(t))).to(dev)
        d = dict(bg_off=up(backgrounds.offsets.numpy()[plan.background], np.int64), bg_len=up(bl[plan.background], np.int32),
                 bg_start=up(plan.bg_start, np.int32), bg_gain=up(plan.bg_gain, np.float32), length=up(plan.length, np.int32),
                 out_off=up(scenes.offsets.numpy(), np.int64), ev_off=up(truth.offsets, np.int64),
                 src_off=up(coughs.offsets.numpy()[plan.event_clip], np.int64), src_len=up(el[plan.event_clip], np.int32),
                 onset=up(plan.onset, np.int32), tiles=up(tiles.reshape(-1), np.int32))
        out = torch.empty_like(scenes.data)
        lib = _lib.load_scenes()

        def kernel():
            _lib.check_scenes(lib.cough_mix_scenes(
                backgrounds.data.data_ptr(), backgrounds.data.numel(), d["bg_off"].data_ptr(), d["bg_len"].data_ptr(),
                d["bg_start"].data_ptr(), d["bg_gain"].data_ptr(), d["length"].data_ptr(), d["out_off"].data_ptr(),
                d["ev_off"].data_ptr(), n, coughs.data.data_ptr(), coughs.data.numel(), d["src_off"].data_ptr(),
                d["src_len"].data_ptr(), d["onset"].data_ptr(), truth.gain.data_ptr(), m, d["tiles"].data_ptr(),
                int(tiles.shape[0]), out.data_ptr(), out.numel(), None), "cough_mix_scenes")

        L = int(plan.length[0])
        ev_scene, ev_len = up(plan.event_scene, np.int64), d["src_len"].to(torch.int64)

        def composed():
            ar = torch.arange(L, device=dev)
            idx = (d["bg_start"].to(torch.int64)[:, None] + ar[None, :]) % d["bg_len"].to(torch.int64)[:, None] + d["bg_off"][:, None]
            mixed = backgrounds.data[idx] * d["bg_gain"][:, None]
            event = torch.repeat_interleave(torch.arange(m, device=dev), ev_len, output_size=ev_samples)
            within = torch.arange(ev_samples, device=dev) - (torch.cumsum(ev_len, 0) - ev_len)[event]
            mixed.view(-1).index_add_(0, ev_scene[event] * L + d["onset"].to(torch.int64)[event] + within,
                                      coughs.data[d["src_off"][event] + within] * truth.gain[event])
            return mixed

        kernel()
        close = torch.allclose(composed().view(-1), out, rtol=1e-5, atol=1e-6)
        for _ in range(args.warmup):
            kernel()
            composed()
        t_k, t_t = [], []
        for _ in range(args.repeats):
            t_k.append(timed(kernel))
            t_t.append(timed(composed))
        t_c = [host_time(lambda: cda.compose_scenes(backgrounds, coughs, plan)) for _ in range(args.repeats)]
        moved = 4 * (2 * total + ev_samples)
        mk, mt = statistics.median(t_k), statistics.median(t_t)
        lines += [fmt("cough_mix_scenes, the launch alone", t_k),
                  f"    {moved / 2**30:.2f} GiB moved (scene samples in and out, event samples in): {moved / mk / 1e12:.2f} TB/s, "
                  f"{100 * moved / mk / HBM_PEAK:.1f} % of the {HBM_PEAK / 1e12:.0f} TB/s peak",
                  f"    the two input banks hold {(backgrounds.data.numel() + coughs.data.numel()) * 4 / 2**20:.0f} MiB and are read "
                  f"many times over: they fit the 256 MiB Infinity Cache, so the reads are not HBM traffic; the "
                  f"{4 * total / 2**30:.2f} GiB written alone are {4 * total / mk / 1e12:.2f} TB/s",
                  fmt("the same mix from torch ops, untuned (cyclic gather, index_add_, indices built)", t_t),
                  f"    torch / kernel = {mt / mk:.1f}; results agree to 1e-5: {close}",
                  fmt("compose_scenes, whole call (plan check, uploads, four launches; host clock)", t_c)]

    if "power" in args.steps:
        t_p = [timed(lambda: cscenes.span_power(backgrounds, plan.background, plan.bg_start, plan.length))
               for _ in range(args.warmup + args.repeats)][args.warmup:]
        mp = statistics.median(t_p)
        lines += [fmt(f"span_power, {n} spans of {int(plan.length[0])} samples, whole call", t_p),
                  f"    {4 * total / 2**30:.2f} GiB read: {4 * total / mp / 1e12:.2f} TB/s"]

    if "match" in args.steps:
        import scenes_ref as R
        import score_ref as S
        hop, window = SR // 4, SR
        per = [int(v) for v in cda.score.windows_per_clip(plan.length, window, hop)]
        prob = np.clip(0.5 + 0.5 * np.sin(np.arange(sum(per)) / 6.0) + rng.normal(0, 0.15, sum(per)), 0, 1).astype(np.float32)
        scores = cda.WindowScores.from_probabilities(prob, per, hop, window, SR, 3)
        thresholds = np.linspace(0.0, 1.0, 101)
        t_m = [timed(lambda: cda.match_events(scores, truth, thresholds)) for _ in range(args.warmup + args.repeats)][args.warmup:]
        sweep = cda.match_events(scores, truth, thresholds)
        smoothed = np.split(scores.smoothed.cpu().numpy(), scores.window_offsets.numpy()[1:-1])
        t0 = time.perf_counter()
        ref = R.match_ref(smoothed, thresholds.tolist(), sweep.gap, truth.offsets, sweep.k_lo, sweep.k_hi, truth.onset, hop,
                          window, S.events_ref)
        t_host = time.perf_counter() - t0
        same = all(np.array_equal(getattr(sweep, a).cpu().numpy(), ref[b]) for a, b in
                   (("hits", "hits"), ("false_alarms", "false_alarms"), ("repeats", "repeats"), ("latency_samples", "latency")))
        lines += [fmt(f"match_events, {sum(per)} windows, {m} truth events, 101 thresholds, whole call", t_m),
                  f"    Python restatement (tests/scenes_ref.py match_ref, one run): {t_host * 1e3:.0f} ms = "
                  f"{t_host / statistics.median(t_m):.0f} x the device call; all four outputs equal: {same}; hits over all "
                  f"thresholds: {int(sweep.hits.sum())}"]

    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
