"""Times the duplicate search (cough_detector_amd/duplicates.py) on the MI355X; writes profiles/dups_bench.txt.

Workload: one-second clips in one ``DeviceClipBank``, generated on the device from a seed: three bursts of band-limited
noise (low-passed noise on a random carrier under a Hann window, random place, length and level) on a noise floor 54 dB
down, so that clips are unrelated; every 16th clip is then replaced by its predecessor at gain 0.3, so the corpus holds
copies and the histogram shows both the copies and the bulk.  Sides:

  fingerprint   the whole of ``fingerprint_bank`` (``cough_prepare_rows``, the featuriser, the fingerprint kernel) on
                4096 and 16384 clips;
  count         ``cough_count_matches`` alone (the match kernel, the scan) at n = 1024, 4096, 8192 and 16384, L = 8,
                Tw = 86, from words that are on the device;
  find          the whole of ``find_duplicates`` (count, the read of the counts, the list pass, the reads of the list);
  torch         the same decisions composed from torch ops on the same GPU at n = 1024: per lag and per chunk of rows an
                XOR, a popcount by a byte lookup table, sums, the live count, and the integer best-lag rule; its counts
                are compared with the kernels';
  numpy         the restatement of tests/dups_ref.py on the host at n = 256 (3 rounds: it takes seconds); what it would
                take at a larger n is EXTRAPOLATED by the number of pairs and marked so.

A step is one XOR + popcount of two words: pairs * sum over the lags of the frames that meet.  The sides alternate in
one process, round by round; every figure is the median of ``--repeats`` (11) rounds after ``--warmup`` warm-up rounds,
the smallest and largest next to it (a host clock around each call; each call ends in a host read or a synchronize).
No time is a pass / fail bar.  ``--profile N`` runs ``cough_count_matches`` three times at n = N and nothing else, for a
counter run of its own.  Run it under a time limit, e.g. ``timeout -k 10 500 python tools/bench_dups.py``.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import cough_detector_amd as cda                                  # noqa: E402
from cough_detector_amd import _lib                               # noqa: E402
from cough_detector_amd.data import _stream                       # noqa: E402
from cough_detector_amd.hostcpu import bound_torch_threads        # noqa: E402
import dups_ref                                                   # noqa: E402
from bench_segments import SHIPPED                                # noqa: E402

L, THR, MIN_LIVE = 8, 256, 16


def burst_bank(n_clips: int, samples: int, seed: int, chunk: int = 2048) -> cda.DeviceClipBank:
    """Unrelated clips (module docstring), made with torch ops on the GPU."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.arange(samples, device="cuda", dtype=torch.float32)
    parts = []
    for lo in range(0, n_clips, chunk):
        b = min(chunk, n_clips - lo)
        x = torch.randn((b, samples), generator=g, device="cuda") * 10.0 ** (-54.0 / 20.0)
        for _ in range(3):
            u = torch.rand((5, b, 1), generator=g, device="cuda")
            length, freq, level = 1200.0 + 2800.0 * u[0], 300.0 + 3200.0 * u[1], 0.3 + 0.7 * u[2]
            start = u[3] * (samples - length)
            smooth = 4 + 2 * int(16 * float(u[4].mean()))         # the low-pass: a moving average of 4..36 samples
            noise = torch.nn.functional.avg_pool1d(torch.randn((b, 1, samples + smooth - 1), generator=g, device="cuda"), smooth, 1)[:, 0]
            phase = ((t[None, :] - start) / length).clamp(0.0, 1.0)
            x += level * noise * torch.cos(2.0 * np.pi * freq / 16000.0 * t[None, :]) * torch.sin(np.pi * phase) ** 2
        parts.append(x / x.abs().amax(dim=1, keepdim=True) * 0.8)
    return cda.DeviceClipBank.from_packed(torch.cat(parts).reshape(-1), [samples] * n_clips, [k % 2 for k in range(n_clips)])


def steps_per_pair(tw: int, lags: int) -> int:
    return sum(max(tw - abs(lag), 0) for lag in dups_ref.lag_order(lags))


def count_only(words: torch.Tensor, live: torch.Tensor, ws: torch.Tensor, counts: torch.Tensor, hist: torch.Tensor) -> None:
    n, tw = words.shape
    _lib.check_dups(_lib.load_dups().cough_count_matches(
        words.data_ptr(), live.data_ptr(), n, tw, L, THR, MIN_LIVE, counts.data_ptr(), hist.data_ptr(), ws.data_ptr(),
        ws.numel() * 4, _stream(words.device)), "cough_count_matches")


def composed(words: torch.Tensor, chunk: int = 32) -> torch.Tensor:
    """The matcher's counts from torch ops: -> (n,) int64 on the host."""
    n, tw = words.shape
    lut = torch.tensor([bin(v).count("1") for v in range(256)], dtype=torch.int32, device=words.device)
    alive = (words != 0).any(dim=1)
    index = torch.arange(n, device=words.device)
    counts = torch.zeros(n, dtype=torch.int64, device=words.device)
    for lo in range(0, n, chunk):
        hi = min(lo + chunk, n)
        valid = (index[lo:hi, None] < index[None, :]) & alive[lo:hi, None] & alive[None, :]
        b_err = torch.zeros((hi - lo, n), dtype=torch.int64, device=words.device)
        b_bits = torch.zeros_like(b_err)
        for lag in dups_ref.lag_order(L):
            t0, t1 = max(0, -lag), min(tw, tw - lag)
            if t1 <= t0:
                continue
            a, b = words[lo:hi, None, t0:t1], words[None, :, t0 + lag:t1 + lag]
            x = (a ^ b).contiguous()
            err = lut[x.view(torch.uint8).long()].view(hi - lo, n, -1).sum(dim=-1, dtype=torch.int64)
            bits = 32 * ((a | b) != 0).sum(dim=-1, dtype=torch.int64)
            take = valid & (bits >= 32 * MIN_LIVE) & ((b_bits == 0) | (err * b_bits < b_err * bits))
            b_err, b_bits = torch.where(take, err, b_err), torch.where(take, bits, b_bits)
        counts[lo:hi] = ((b_bits > 0) & (b_err * 1024 <= THR * b_bits)).sum(dim=1)
    return counts.cpu()


def fmt(name: str, times, extra: str = "") -> str:
    ms = sorted(t * 1e3 for t in times)
    return f"  {name:<58} median {statistics.median(ms):10.3f} ms  min {ms[0]:10.3f}  max {ms[-1]:10.3f}{extra}"


def rates(n: int, tw: int, seconds: float) -> str:
    pairs = n * (n - 1) // 2
    return f"  {pairs / seconds:9.3e} pairs/s  {pairs * steps_per_pair(tw, L) / seconds:9.3e} steps/s"


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "dups_bench.txt"))
    ap.add_argument("--clips", type=int, default=16384)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--profile", type=int, default=0, help="run cough_count_matches three times at this n and stop")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dups.py needs the MI355X; there is no CPU fallback")
    bound_torch_threads()
    pre = cda.AudioPreprocessor(device="cuda", **SHIPPED)
    samples = int(pre.segment_samples)
    n_all = max(args.clips, args.profile, 1024)
    bank = burst_bank(n_all, samples, seed=5000)
    rows = bank.data.view(n_all, samples)
    rows[1::16] = rows[0::16][:rows[1::16].shape[0]] * 0.3        # the planted copies
    fp = cda.fingerprint_bank(bank, pre)
    tw = int(fp.words.shape[1])
    lib, dev = _lib.load_dups(), bank.device

    def buffers(n):
        return (fp.words[:n].contiguous(), fp.live[:n].contiguous(),
                torch.empty(lib.cough_match_workspace_bytes(n, tw) // 4, dtype=torch.int32, device=dev),
                torch.empty(n, dtype=torch.int32, device=dev), torch.empty(65, dtype=torch.int64, device=dev))
    if args.profile:
        buf = buffers(args.profile)
        for _ in range(3):
            count_only(*buf)
        torch.cuda.synchronize()
        print(f"count at n = {args.profile}: {int(buf[3].sum())} matches")
        return

    sizes = [n for n in (1024, 4096, 8192, 16384) if n <= n_all]
    sides, note = {}, {}
    for n in (4096, 16384):
        if n <= n_all:
            sub = bank if n == n_all else bank.subset(range(n))
            sides[f"fingerprint_bank, {n} clips"] = lambda sub=sub: cda.fingerprint_bank(sub, pre)
    for n in sizes:
        buf = buffers(n)
        part = cda.Fingerprints(buf[0], buf[1], fp.window, fp.delta, fp.rows)
        sides[f"cough_count_matches, n = {n}"] = lambda buf=buf: count_only(*buf)
        sides[f"find_duplicates, whole call, n = {n}"] = lambda part=part: cda.find_duplicates(part)
        note[f"cough_count_matches, n = {n}"] = note[f"find_duplicates, whole call, n = {n}"] = n
    small = fp.words[:1024].contiguous()
    sides["torch ops (XOR, byte-table popcount, sums), n = 1024"] = lambda: composed(small)
    note["torch ops (XOR, byte-table popcount, sums), n = 1024"] = 1024
    host = fp.words[:256].cpu().numpy().view(np.uint32)
    slow = {"numpy restatement on the host, n = 256": lambda: dups_ref.match_words(host, L, THR, MIN_LIVE)}
    note["numpy restatement on the host, n = 256"] = 256

    times = {name: [] for name in (*sides, *slow)}
    for r in range(args.warmup + args.repeats):
        for name, fn in (*sides.items(), *(slow.items() if r < 3 else ())):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= args.warmup or name in slow:
                times[name].append(time.perf_counter() - t0)

    table = cda.find_duplicates(cda.Fingerprints(fp.words[:1024].contiguous(), fp.live[:1024].contiguous(), fp.window, fp.delta, fp.rows))
    ref = dups_ref.match_words(host, L, THR, MIN_LIVE)
    first = cda.find_duplicates(cda.Fingerprints(fp.words[:256].contiguous(), fp.live[:256].contiguous(), fp.window, fp.delta, fp.rows))
    equal = all(getattr(first, f).tolist() == ref[k].tolist() for f, k in (("a", "a"), ("b", "b"), ("lag", "lag"), ("errors", "err"),
                                                                           ("bits", "bits"), ("counts", "counts"), ("histogram", "hist")))
    whole = cda.find_duplicates(fp) if n_all <= 65536 else None
    lines = [f"duplicate search, one-second synthetic clips, every 16th a copy of its predecessor at gain 0.3; Tw = {tw}, L = {L}, "
             f"max_err_1024 = {THR}, min_live = {MIN_LIVE}; {steps_per_pair(tw, L)} steps per pair; sides alternating, median of "
             f"{args.repeats} after {args.warmup} warm-up rounds (numpy: 3 rounds); {torch.cuda.get_device_name(0)}",
             f" n = 256 equal to the numpy restatement (list, counts, histogram): {equal}; torch's counts at n = 1024 equal the "
             f"kernels': {composed(small).tolist() == table.counts.tolist()}"]
    for name, t in times.items():
        extra = rates(note[name], tw, statistics.median(t)) if name in note else ""
        lines.append(fmt(name, t, extra))
    per_pair = statistics.median(times["numpy restatement on the host, n = 256"]) / (256 * 255 // 2)
    lines.append(" numpy EXTRAPOLATED by pairs from n = 256 (not measured): "
                 + ", ".join(f"n = {n}: {per_pair * (n * (n - 1) // 2):.0f} s" for n in sizes[1:]))
    if whole is not None:
        lines.append(f" n = {n_all}: {len(whole)} pairs, {int((np.bincount(cda.duplicate_groups(whole)) > 1).sum())} groups, "
                     f"{whole.flat.size} flat clips; histogram of the best rate of every pair, bins of 1/64:")
        lines.append("  " + " ".join(str(v) for v in whole.histogram.tolist()))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
