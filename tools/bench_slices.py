"""Times slicing recordings into active clips (cough_detector_amd/slices.py) on the MI355X; writes
profiles/slices_bench.txt.

Workload: the setup of tools/bench_segments.py -- ``--clips`` (2048) recordings of ``--seconds`` (10) s of device-generated
synthetic audio in one ``DeviceClipBank`` -- sliced at stride = the window length and at a quarter of it, with
``--max-per-clip`` (8) windows kept per recording at the most.  Sides, per stride:

  find    the whole of ``find_windows`` (the frame energies, uploads, both kernels, the read of the counts, the table);
  kernels ``cough_window_activity``, the read of the counts, ``cough_list_windows``: the decision alone, from energies
          and offsets that are on the device already -- what the torch side is the counterpart of;
  slice   the whole of ``slice_bank`` (``find_windows`` and the copy of the kept windows);
  torch   the same decisions composed from torch ops on the same GPU, from the same energies: the finite gate and the
          largest energy per clip, the activity, ``cumsum``, the windows' counts as differences of the cumulated
          activity at their first and last frame, the share test, and ``topk`` for the cap; it ends in the same read of
          the counts.  ``topk`` does not promise the earlier window on a tie, so its counts are compared with the
          kernels', not its choice among equals;
  numpy   the restatement of tests/slices_ref.py on the host, from energies that are already there (no transfer timed).

The sides alternate in one process, round by round, so that a drift of the machine lands on all of them; every figure
is the median of ``--repeats`` rounds after ``--warmup`` warm-up rounds, the smallest and largest next to it (a host
clock around each call; each call ends in a host read or a synchronize).  No time is a pass / fail bar.
Run it under a time limit, e.g. ``timeout -k 10 300 python tools/bench_slices.py``.
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
from cough_detector_amd import _lib, segments as cseg, slices as cslices   # noqa: E402
from cough_detector_amd.data import _offsets, _stream, _upload    # noqa: E402
from cough_detector_amd.hostcpu import bound_torch_threads        # noqa: E402
import slices_ref                                                 # noqa: E402
from bench_segments import SHIPPED, synthetic_bank                # noqa: E402

FRAME, HOP = 400, 160


def composed(energy: torch.Tensor, samples: int, seg_len: int, stride: int, ratio: float, floor: float, min_active: float,
             cap: int):
    """-> (keep (n, W) bool on the device, counts on the host) for a bank of equal lengths ``samples`` >= seg_len."""
    dev = energy.device
    w = torch.arange(1 + (samples - seg_len) // stride, device=dev, dtype=torch.int64)
    first = (w * stride + HOP - 1) // HOP
    last = torch.clamp((w * stride + seg_len - FRAME) // HOP, max=energy.shape[1] - 1)
    cnt = torch.clamp(last - first + 1, min=0)
    finite = torch.isfinite(energy).all(dim=1)
    e_max = energy.max(dim=1).values
    thr = torch.clamp(e_max * ratio, min=floor)
    active = (energy >= thr[:, None]) & (finite & (e_max >= floor))[:, None]
    below = torch.nn.functional.pad(active.to(torch.int32).cumsum(dim=1), (1, 0))
    m = torch.where(cnt > 0, below[:, last + 1] - below[:, first], 0)
    q = (m >= 1) & (m.double() >= min_active * cnt.double())
    if cap < q.shape[1]:
        key = torch.where(q, m, -1)
        top = key.topk(cap, dim=1)
        keep = torch.zeros_like(q).scatter_(1, top.indices, top.values >= 1)
    else:
        keep = q
    return keep, keep.sum(dim=1).cpu()


def kernels(bank, energy, offs_dev, seg_len: int, stride: int, ratio: float, floor: float, min_active: float, cap: int):
    """Both kernels and the read between them, as ``find_windows`` runs them -> counts on the host."""
    lib, dev, n = _lib.load_slices(), bank.device, len(bank)
    per_clip = cslices.window_counts(bank.lengths.numpy(), seg_len, stride)
    woffs, _ = _upload(dev, _offsets(per_clip), np.zeros(0, np.int32))
    i32 = dict(dtype=torch.int32, device=dev)
    total = int(per_clip.sum())
    peak, clip_active, counts_dev = torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, **i32), torch.empty(n, **i32)
    active, keep = torch.empty(total, **i32), torch.empty(total, **i32)
    _lib.check_slices(lib.cough_window_activity(
        energy.data_ptr(), offs_dev.data_ptr(), bank.lengths_dev.data_ptr(), woffs.data_ptr(), n, FRAME, HOP, seg_len, stride,
        cap, ratio, floor, min_active, peak.data_ptr(), clip_active.data_ptr(), active.data_ptr(), keep.data_ptr(),
        counts_dev.data_ptr(), _stream(dev)), "cough_window_activity")
    counts = counts_dev.cpu()
    rows = int(counts.sum())
    roffs, _ = _upload(dev, _offsets(counts), np.zeros(0, np.int32))
    clip = torch.empty(rows, dtype=torch.int64, device=dev)
    start, length, row_active = torch.empty(rows, **i32), torch.empty(rows, **i32), torch.empty(rows, **i32)
    if rows:
        _lib.check_slices(lib.cough_list_windows(
            keep.data_ptr(), active.data_ptr(), bank.lengths_dev.data_ptr(), woffs.data_ptr(), roffs.data_ptr(), n, seg_len,
            stride, clip.data_ptr(), start.data_ptr(), length.data_ptr(), row_active.data_ptr(), _stream(dev)),
            "cough_list_windows")
    return counts


def fmt(name: str, times) -> str:
    ms = sorted(t * 1e3 for t in times)
    return f"  {name:<60} median {statistics.median(ms):9.3f} ms  min {ms[0]:9.3f}  max {ms[-1]:9.3f}"


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "slices_bench.txt"))
    ap.add_argument("--clips", type=int, default=2048)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--max-per-clip", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=9)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_slices.py needs the MI355X; there is no CPU fallback")
    bound_torch_threads()
    pre = cda.AudioPreprocessor(device="cuda", **SHIPPED)
    seg_len, samples = int(pre.segment_samples), int(round(args.seconds * pre.sample_rate))
    bank = synthetic_bank(args.clips, samples, seed=4000)
    n, cap = len(bank), args.max_per_clip
    ratio, floor = slices_ref.levels()
    energy, frame_offsets, offs_dev = cseg._frame_energy(bank, FRAME, HOP)
    matrix = energy.view(n, -1)
    host = energy.cpu().numpy()
    energies = [host[a:b] for a, b in zip(frame_offsets[:-1], frame_offsets[1:])]
    lengths = bank.lengths.tolist()
    lines = [f"slicing into active clips, {n} clips of {samples} samples ({bank.data.numel() * 4 / 2**30:.2f} GiB), frame "
             f"{FRAME} / hop {HOP}, window {seg_len}, at most {cap} per clip; sides alternating, median of {args.repeats} "
             f"after {args.warmup} warm-up rounds; {torch.cuda.get_device_name(0)}"]
    for stride in (seg_len, seg_len // 4):
        params = dict(stride=stride, max_per_clip=cap)
        sides = {
            "find_windows, whole call": lambda: cda.find_windows(bank, pre, **params),
            "slice_bank, whole call": lambda: cda.slice_bank(bank, pre, **params),
            "both kernels and the read of the counts, from the energies":
                lambda: kernels(bank, energy, offs_dev, seg_len, stride, ratio, floor, 0.5, cap),
            "torch ops from the energies (cumsum, differences, topk)":
                lambda: composed(matrix, samples, seg_len, stride, ratio, floor, 0.5, cap),
            "numpy restatement on the host, from the energies":
                lambda: slices_ref.table_ref(energies, lengths, seg_len, stride, FRAME, HOP, cap=cap),
        }
        times = {name: [] for name in sides}
        for r in range(args.warmup + args.repeats):
            for name, fn in sides.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if r >= args.warmup:
                    times[name].append(time.perf_counter() - t0)
        table = cda.find_windows(bank, pre, **params)
        ref = slices_ref.table_ref(energies, lengths, seg_len, stride, FRAME, HOP, cap=cap)
        _, counts = composed(matrix, samples, seg_len, stride, ratio, floor, 0.5, cap)
        same = table.counts.tolist() == ref["counts"] and table.start.tolist() == ref["start"]
        lines.append(f" stride {stride}: {int(table.windows.sum())} windows, {len(table)} kept in "
                     f"{int((table.counts > 0).sum())} of {n} clips; equal to the restatement: {same}; torch's counts equal: "
                     f"{counts.tolist() == ref['counts']}")
        lines += [fmt(name, t) for name, t in times.items()]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
