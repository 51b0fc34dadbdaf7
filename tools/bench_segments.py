"""Times corpus curation (cough_detector_amd/segments.py) on the MI355X; writes profiles/segments_bench.txt.

Workload: ``--clips`` (2048) recordings of ``--seconds`` (10) s, each ten consecutive clips of device-generated synthetic
audio (``synth.device_clips``), packed into one ``DeviceClipBank``.  Steps (``--steps``, each timed on its own):

  kernel  ``cough_frame_energy`` alone, tile table and offsets already on the device: device events around ``--inner``
          launches back to back (the bank is larger than the Infinity Cache, so every launch reads it from HBM).
          Reported as bytes over time against the 8 TB/s HBM peak; bytes = the bank read once + the energies written.
  find    the whole of ``find_segments`` (tile table, upload, both kernels, the read of the counts, the table): a host
          clock around the call, which ends in that read.
  torch   the same energies composed from torch ops on the same GPU: the bank viewed as a (clips, samples) matrix,
          ``unfold`` into frames, float64 square and mean, ``--torch-chunk`` clips at a time (the float64 frames of the
          whole bank would not fit); device events around the loop.  Its result is compared with the kernel's.

Every figure is the median of ``--repeats`` runs after ``--warmup`` warm-up runs, the smallest and largest next to it.
Run it under a time limit, e.g. ``timeout -k 10 300 python tools/bench_segments.py``.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import cough_detector_amd as cda                                  # noqa: E402
from cough_detector_amd import _lib, segments as cseg, synth     # noqa: E402
from cough_detector_amd.data import _ragged, _stream, _upload     # noqa: E402
from cough_detector_amd.hostcpu import bound_torch_threads        # noqa: E402

SHIPPED = dict(use_pcen=False, use_pre_emphasis=False, use_delta_delta=False, use_spectral_contrast=False)
HBM_PEAK = 8.0e12
FRAME, HOP = 400, 160


def synthetic_bank(n_clips: int, samples: int, seed: int) -> cda.DeviceClipBank:
    total = n_clips * samples
    audio = synth.device_clips(seed, (total + synth.N - 1) // synth.N).reshape(-1)[:total]
    return cda.DeviceClipBank.from_packed(audio, [samples] * n_clips, [k % 2 for k in range(n_clips)])


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


def host_times(fn, warmup: int, repeats: int):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def fmt(name: str, times) -> str:
    ms = sorted(t * 1e3 for t in times)
    return f"  {name:<72} median {statistics.median(ms):9.3f} ms  min {ms[0]:9.3f}  max {ms[-1]:9.3f}"


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "segments_bench.txt"))
    ap.add_argument("--clips", type=int, default=2048)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--inner", type=int, default=50, help="launches of the kernel per timed window")
    ap.add_argument("--torch-chunk", type=int, default=128)
    ap.add_argument("--steps", nargs="+", default=["kernel", "find", "torch"], choices=["kernel", "find", "torch"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_segments.py needs the MI355X; there is no CPU fallback")
    bound_torch_threads()
    pre = cda.AudioPreprocessor(device="cuda", **SHIPPED)
    samples = int(round(args.seconds * pre.sample_rate))
    bank = synthetic_bank(args.clips, samples, seed=4000)
    dev, n = bank.device, len(bank)
    frames = cseg.frame_counts(bank.lengths.numpy(), FRAME, HOP)
    total_frames = int(frames.sum())
    lines = [f"corpus curation, {n} clips of {samples} samples ({bank.data.numel() * 4 / 2**30:.2f} GiB), frame {FRAME} / hop "
             f"{HOP}: {total_frames} frames; median of {args.repeats} after {args.warmup} warm-up runs; "
             f"{torch.cuda.get_device_name(0)}"]
    energy = None
    if "kernel" in args.steps or "torch" in args.steps:
        energy, frame_offsets, offs_dev = cseg._frame_energy(bank, FRAME, HOP)      # also the comparison's left side
    if "kernel" in args.steps:
        lib = _lib.load_segments()
        tile_frames = lib.cough_frame_energy_tile_frames(FRAME, HOP)
        _, tile_clip, tile_rank = _ragged((frames + tile_frames - 1) // tile_frames)
        tiles = np.stack([tile_clip, tile_rank * tile_frames], axis=1).astype(np.int32)
        _, tiles_dev = _upload(dev, np.zeros(0, np.int64), tiles.reshape(-1))
        out = torch.empty_like(energy)

        def kernel():
            _lib.check_segments(lib.cough_frame_energy(bank.data.data_ptr(), bank.offsets_dev.data_ptr(),
                                                       bank.lengths_dev.data_ptr(), offs_dev.data_ptr(), n,
                                                       tiles_dev.data_ptr(), tiles.shape[0], FRAME, HOP, out.data_ptr(),
                                                       _stream(dev)), "cough_frame_energy")

        def launches():
            for _ in range(args.inner):
                kernel()

        t = [v / args.inner for v in device_times(launches, args.warmup, args.repeats)]
        assert torch.equal(out, energy)
        nbytes = bank.data.numel() * 4 + total_frames * 8
        med = statistics.median(t)
        lines += [fmt(f"cough_frame_energy ({tiles.shape[0]} tiles of {tile_frames} frames), per launch of {args.inner}", t),
                  f"    {nbytes / 2**30:.3f} GiB (bank read once + energies written) / median = {nbytes / med / 1e12:.2f} TB/s "
                  f"= {100 * nbytes / med / HBM_PEAK:.1f} % of the 8 TB/s HBM peak"]
    if "find" in args.steps:
        table = cda.find_segments(bank, pre)
        t = host_times(lambda: cda.find_segments(bank, pre), args.warmup, args.repeats)
        lines += [fmt("find_segments, whole call", t),
                  f"    {len(table)} segments in {int((table.counts > 0).sum())} of {n} clips"]
    if "torch" in args.steps:
        matrix = bank.data.view(n, samples)
        ref = torch.empty_like(energy).view(n, -1)

        def composed():
            for lo in range(0, n, args.torch_chunk):
                x = matrix[lo:lo + args.torch_chunk].unfold(1, FRAME, HOP)
                ref[lo:lo + args.torch_chunk] = x.double().square().mean(-1)

        t = device_times(composed, max(1, args.warmup // 2), max(3, args.repeats // 2))
        rel = float(((ref.view(-1) - energy).abs() / ref.view(-1).clamp_min(1e-300)).max())
        lines += [fmt(f"torch: unfold, float64 square, mean ({args.torch_chunk} clips at a time)", t),
                  f"    worst relative difference from cough_frame_energy: {rel:.2e}"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
