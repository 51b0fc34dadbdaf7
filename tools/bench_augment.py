"""Throughput of AudioAugmentor.augment_batch (cough_augment_waveforms) on the MI355X.

4096 clips x 1 s (16 kHz) with a 100-entry noise bank (entries of 0.25 .. 3 s), p_augment = 0.5 (the reference's default)
and 1.0 (every step fires).  Reports, per configuration:
  * kernel time (device events around repeated launches with the draws made once) as clips/s and as effective HBM
    bandwidth over the algorithmic bytes: read the clip + read the bank crop (clips whose add_noise fired) + write the
    clip (+ read the gaussian buffer of clips whose add_gaussian_noise fired, host-noise mode);
  * the whole augment_batch call (host draws + launch) in device-noise mode;
  * a vectorised torch-on-GPU composition of the same chain (gather for the shift, torch reductions, torch.randn);
  * augment + featurise (AudioPreprocessor.extract_features, shipped flags) against featurise alone.
Prints human-readable lines and one JSON line.  Usage: python tools/bench_augment.py [--clips 4096] [--iters 50]
"""
import argparse
import json
import os
import random
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cough_detector_amd as cda                                   # noqa: E402
from cough_detector_amd import _lib                                # noqa: E402

SR, N = 16000, 16000


def timed(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def algorithmic_bytes(clips, host_noise):
    b = 0
    for c in clips:
        b += 4 * N * 2                                            # read the clip, write the clip
        if c.bank_index >= 0:
            b += 4 * N
        if host_noise and c.gaussian:
            b += 4 * N
    return b


def torch_chain(x, clips, bank, offsets, lengths):
    """The same chain composed from torch ops on the GPU, vectorised over the batch (per-clip parameters as tensors)."""
    dev = x.device
    bsz = x.shape[0]
    shift = torch.tensor([c.shift for c in clips], device=dev)
    gain = torch.tensor([c.gain for c in clips], device=dev)
    g_on = torch.tensor([c.gaussian for c in clips], device=dev, dtype=torch.bool)
    g_snr = torch.tensor([10 ** (c.gaussian_snr_db / 10) for c in clips], device=dev)
    k = torch.tensor([max(c.bank_index, 0) for c in clips], device=dev)
    b_on = torch.tensor([c.bank_index >= 0 for c in clips], device=dev)
    b_start = torch.tensor([c.bank_start for c in clips], device=dev)
    b_snr = torch.tensor([10 ** (c.bank_snr_db / 10) for c in clips], device=dev)
    i = torch.arange(N, device=dev)
    j = i[None, :] - shift[:, None]
    valid = (j >= 0) & (j < N)
    y = torch.where(valid, torch.gather(x, 1, j.clamp(0, N - 1)), torch.zeros((), device=dev)) * gain[:, None]
    p = y.pow(2).mean(dim=1)
    z = torch.randn((bsz, N), device=dev)
    pz = z.pow(2).mean(dim=1)
    y = torch.where(g_on[:, None], y + torch.sqrt(p / (g_snr * pz))[:, None] * z, y)
    p = y.pow(2).mean(dim=1)
    idx = offsets[k][:, None] + (b_start[:, None] + i[None, :]) % lengths[k][:, None]
    n = bank[idx]
    pn = n.pow(2).mean(dim=1)
    add = b_on & (pn > 0)
    return torch.where(add[:, None], y + torch.sqrt(p / (b_snr * pn))[:, None] * n, y)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    g = torch.Generator().manual_seed(0)
    x = ((torch.rand((args.clips, N), generator=g) - 0.5) * 0.8).to(dev)
    pre = cda.AudioPreprocessor(use_pcen=False, use_pre_emphasis=False, use_delta_delta=False, use_spectral_contrast=False,
                                device="cuda")
    results = {"clips": args.clips, "samples": N, "bank_entries": 100, "iters": args.iters}
    feat_ms = timed(lambda: pre.extract_features(x), args.iters)
    results["featurise_ms"] = feat_ms
    print(f"featurise alone: {feat_ms:.3f} ms  ({args.clips / feat_ms * 1e3 / 1e6:.2f} M clips/s)", flush=True)
    for p in (0.5, 1.0):
        aug = cda.AudioAugmentor(sample_rate=SR, p_augment=p)
        aug.noise_samples = [torch.randn((1, int(torch.randint(4000, 48001, (1,), generator=g))), generator=g) * 0.2
                             for _ in range(100)]
        aug._pack_bank()
        random.seed(1)
        clips = aug.draw_batch([N] * args.clips)
        gbuf = torch.randn((args.clips, N), generator=g).to(dev)
        bank = aug._bank_device(dev)
        offs = torch.tensor(aug._bank_offsets, device=dev)
        lens = torch.tensor(aug._bank_lengths, device=dev)
        tag = f"p={p}"
        dev_ms = timed(lambda: aug._run(x, clips, None, None, 7), args.iters)
        host_ms = timed(lambda: aug._run(x, clips, None, gbuf, 7), args.iters)
        bd, bh = algorithmic_bytes(clips, False), algorithmic_bytes(clips, True)
        t0 = time.perf_counter()
        for _ in range(5):
            aug.augment_batch(x)
        torch.cuda.synchronize()
        call_ms = (time.perf_counter() - t0) / 5 * 1e3
        torch_ms = timed(lambda: torch_chain(x, clips, bank, offs, lens), max(5, args.iters // 5), warmup=2)
        both_ms = timed(lambda: pre.extract_features(aug._run(x, clips, None, None, 7)), args.iters)
        r = {"kernel_device_noise_ms": dev_ms, "kernel_host_noise_ms": host_ms,
             "clips_per_s_device_noise": args.clips / dev_ms * 1e3, "clips_per_s_host_noise": args.clips / host_ms * 1e3,
             "eff_GBps_device_noise": bd / dev_ms / 1e6, "eff_GBps_host_noise": bh / host_ms / 1e6,
             "augment_batch_call_ms": call_ms, "torch_gpu_chain_ms": torch_ms, "augment_plus_featurise_ms": both_ms,
             "fired": {"shift": sum(c.shift != 0 for c in clips), "gain": sum(c.gain != 1.0 for c in clips),
                       "gaussian": sum(c.gaussian for c in clips), "bank": sum(c.bank_index >= 0 for c in clips)}}
        results[tag] = r
        print(f"{tag}: kernel (device noise) {dev_ms:.3f} ms = {r['clips_per_s_device_noise'] / 1e6:.2f} M clips/s, "
              f"{r['eff_GBps_device_noise']:.0f} GB/s effective; (host noise) {host_ms:.3f} ms = "
              f"{r['clips_per_s_host_noise'] / 1e6:.2f} M clips/s, {r['eff_GBps_host_noise']:.0f} GB/s effective", flush=True)
        print(f"{tag}: augment_batch call (host draws + launch) {call_ms:.2f} ms; torch-on-GPU chain {torch_ms:.3f} ms "
              f"({torch_ms / dev_ms:.1f}x the kernel); augment + featurise {both_ms:.3f} ms vs featurise alone "
              f"{feat_ms:.3f} ms; fired {r['fired']}", flush=True)
    print(json.dumps(results))


if __name__ == "__main__":
    main()
