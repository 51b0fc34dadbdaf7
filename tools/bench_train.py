"""Time one training step (forward, backward, clip, AdamW) of CoughDetectorResidual (``--model residual``, the default),
CoughDetectorSmall (``--model small``) or CoughDetector (``--model standard``): the HIP step of ResidualTrainer /
SmallTrainer / StandardTrainer against a torch-eager fp32 step on
the same GPU (a module of torch.nn layers with the reference's structure, torch.optim.AdamW, clip_grad_norm_).  The two paths alternate, `--rounds` times, each round timing `--steps` steps after
`--warmup` with device events.  Prints one line per batch size (median ms per step, clips/s, FLOP-based share of the
f32 MFMA peak).  For Standard, each line also carries the share of the peak of convs 1-3 alone (``--conv-ms``: their
kernels' time per step from a kernel trace).  For Small and Standard, each line also carries the HBM bytes per step that the HIP step's kernels must move at least (every stored
activation written once and read once per consumer, x read by each of its passes) and the achieved rate against it.
Usage: python tools/bench_train.py [--model residual|small|standard] [--batches 32,256,1024] [--steps 20] [--warmup 5] [--rounds 3]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cough_detector_amd as cda                      # noqa: E402
from cough_detector_amd.training import ResidualTrainer, SmallTrainer, StandardTrainer   # noqa: E402

F32_MFMA_PEAK = 157.3e12
H, W = 90, 101


def flops_per_clip(h=H, w=W):
    """2 * MACs of every conv, forward; a step is forward + wgrad (same) + dgrad (every conv but the stem)."""
    def o(n, k, s, p):
        return (n + 2 * p - k) // s + 1
    c1h, c1w = o(h, 7, 2, 3), o(w, 7, 2, 3)
    stem = 2 * c1h * c1w * 32 * 49
    ph, pw = c1h // 2, c1w // 2
    blocks = 0
    for cin, cout in ((32, 64), (64, 128)):
        oh, ow = o(ph, 3, 2, 1), o(pw, 3, 2, 1)
        blocks += 2 * oh * ow * cout * (9 * cin + 9 * cout + cin)
        ph, pw = oh, ow
    return stem, blocks, 2 * (stem + blocks) + blocks


class TorchResidual(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = nn.Sequential(nn.Conv2d(1, 32, 7, 2, 3), nn.BatchNorm2d(32), nn.ReLU(), nn.MaxPool2d(2))
        self.blocks = nn.ModuleList()
        for cin, cout in ((32, 64), (64, 128)):
            self.blocks.append(nn.ModuleDict(dict(
                conv1=nn.Conv2d(cin, cout, 3, 2, 1), bn1=nn.BatchNorm2d(cout), conv2=nn.Conv2d(cout, cout, 3, 1, 1),
                bn2=nn.BatchNorm2d(cout), skip=nn.Sequential(nn.Conv2d(cin, cout, 1, 2), nn.BatchNorm2d(cout)))))
        self.fc = nn.Sequential(nn.Flatten(), nn.Dropout(0.5), nn.Linear(128, 2))

    def forward(self, x):
        x = self.conv1(x)
        for b in self.blocks:
            idn = b["skip"](x)
            o = F.relu(b["bn1"](b["conv1"](x)))
            x = F.relu(b["bn2"](b["conv2"](o)) + idn)
        return self.fc(F.adaptive_avg_pool2d(x, 1))


def small_flops_per_clip(h=H, w=W):
    """2 * MACs of a step of CoughDetectorSmall: forward, wgrad (same) and dgrad of every conv but conv1."""
    conv1 = 2 * h * w * 16 * 9
    blocks, ph, pw = 0, h // 2, w // 2
    for cin, cout in ((16, 32), (32, 64), (64, 128)):
        blocks += 2 * ph * pw * (9 * cin + cin * cout)
        ph, pw = ph // 2, pw // 2
    return 2 * (conv1 + blocks) + blocks


def small_bytes_per_clip(h=H, w=W):
    """HBM bytes of one HIP step of Small per clip (csrc/train_small.hip): x read by its 5 passes; per block k the dw
    input p, dw output d and pw output z written once; read by the forward (z twice: statistics, pool / head; p, d once
    more by dw / pw); backward writes dz, dd, dp and reads z (twice), dp of the next block, dz (wgrad), d (wgrad), dd
    and p (dw backward), dp (BN partials and dz pass of the block before)."""
    total = 5 * h * w * 4
    ph, pw = h // 2, w // 2
    for cin, cout in ((16, 32), (32, 64), (64, 128)):
        n_in, n_out = ph * pw * cin * 4, ph * pw * cout * 4
        fwd = (n_in + n_in + n_out) + (n_in + n_out * 2)          # p, d, z written; p read by dw, z by stats + pool
        bwd = (n_out * 2 + n_out + n_in) + (n_out + n_in) + (n_in * 2 + n_in) + 2 * n_in
        total += fwd + bwd
        ph, pw = ph // 2, pw // 2
    return total


class TorchSmall(nn.Module):
    def __init__(self):
        super().__init__()
        self.features = nn.Sequential(
            nn.Conv2d(1, 16, 3, padding=1), nn.BatchNorm2d(16), nn.ReLU(), nn.MaxPool2d(2),
            nn.Conv2d(16, 16, 3, padding=1, groups=16), nn.Conv2d(16, 32, 1), nn.BatchNorm2d(32), nn.ReLU(), nn.MaxPool2d(2),
            nn.Conv2d(32, 32, 3, padding=1, groups=32), nn.Conv2d(32, 64, 1), nn.BatchNorm2d(64), nn.ReLU(), nn.MaxPool2d(2),
            nn.Conv2d(64, 64, 3, padding=1, groups=64), nn.Conv2d(64, 128, 1), nn.BatchNorm2d(128), nn.ReLU(),
            nn.AdaptiveAvgPool2d((1, 1)))
        self.classifier = nn.Sequential(nn.Flatten(), nn.Linear(128, 64), nn.ReLU(), nn.Dropout(0.3), nn.Linear(64, 2))

    def forward(self, x):
        return self.classifier(self.features(x))


STD_CHANNELS = (32, 64, 128, 256)


def std_flops_per_clip(h=H, w=W):
    """2 * MACs of a step of CoughDetector: (conv 0, convs 1-3 forward, step total).  A step is forward, wgrad (same)
    and dgrad of convs 1-3 (conv 0's input gradient is never needed)."""
    conv0 = 2 * h * w * 32 * 9
    blocks, ph, pw = 0, h // 2, w // 2
    for cin, cout in zip(STD_CHANNELS[:-1], STD_CHANNELS[1:]):
        blocks += 2 * ph * pw * cout * cin * 9
        ph, pw = ph // 2, pw // 2
    return conv0, blocks, 2 * (conv0 + blocks) + blocks


def std_bytes_per_clip(h=H, w=W):
    """HBM bytes of one HIP step of CoughDetector per clip (csrc/train_std.hip), counting each stored tensor once per
    write and once per reading pass: x read by conv 0 and its weight gradient; per block k the pre-BN output z (written;
    read by the two statistics passes, the BN-pool-dropout pass, the backward partial sums, and dz: 5 reads), the pooled
    output a (written; read by the next conv and its weight gradient), its gradient da (written by the dgrad; read by
    the backward partial sums and dz), the pool's argmax byte (written, read twice), and for k >= 1 dz (written; read by
    wgrad and dgrad)."""
    total = 2 * h * w * 4
    hh, ww = h, w
    for k, c in enumerate(STD_CHANNELS):
        z = hh * ww * c * 4
        ph, pw = hh // 2, ww // 2
        pooled = ph * pw * c
        total += 6 * z + 3 * pooled * 4 + 3 * pooled
        if k < 3:
            total += 3 * pooled * 4
        if k > 0:
            total += 3 * z
        hh, ww = ph, pw
    return total


class TorchStandard(nn.Module):
    def __init__(self):
        super().__init__()
        layers, cin = [], 1
        for c in STD_CHANNELS:
            layers += [nn.Conv2d(cin, c, 3, padding=1), nn.BatchNorm2d(c), nn.ReLU(), nn.MaxPool2d(2), nn.Dropout2d(0.1)]
            cin = c
        self.conv_layers = nn.Sequential(*layers)
        self.fc = nn.Sequential(nn.Linear(256, 128), nn.ReLU(), nn.Dropout(0.5), nn.Linear(128, 2))

    def forward(self, x):
        return self.fc(F.adaptive_avg_pool2d(self.conv_layers(x), 1).flatten(1))


def time_steps(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(steps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("residual", "small", "standard"), default="residual")
    ap.add_argument("--batches", default="32,256,1024")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only-hip", action="store_true", help="HIP step only (for a kernel trace)")
    ap.add_argument("--conv-ms", default="", help="standard: batch=ms,... of convs 1-3 per step (from a kernel trace)")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    small, std = a.model == "small", a.model == "standard"
    step_flops = small_flops_per_clip() if small else std_flops_per_clip()[2] if std else flops_per_clip()[2]
    conv_ms = {int(k): float(v) for k, v in (kv.split("=") for kv in a.conv_ms.split(",") if kv)}
    for b in [int(v) for v in a.batches.split(",")]:
        g = torch.Generator().manual_seed(b)
        x = torch.randn(b, 1, H, W, generator=g).to(dev)
        y = torch.randint(0, 2, (b,), generator=g).to(dev)
        cw = torch.tensor([1.0, 2.5], device=dev)
        if small:
            tr = SmallTrainer(cda.create_model("small", n_mels=H), class_weights=cw)
            tm = TorchSmall().to(dev).train()
        elif std:
            tr = StandardTrainer(cda.create_model("standard", n_mels=H), class_weights=cw)
            tm = TorchStandard().to(dev).train()
        else:
            tr = ResidualTrainer(cda.create_model("residual", n_mels=H), class_weights=cw)
            tm = TorchResidual().to(dev).train()
        opt = torch.optim.AdamW(tm.parameters(), lr=1e-3, weight_decay=0.01)
        crit = nn.CrossEntropyLoss(weight=cw)

        def hip_step():
            tr.step(x, y)

        def torch_step():
            opt.zero_grad()
            loss = crit(tm(x), y)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(tm.parameters(), max_norm=1.0)
            opt.step()

        hip, eager = [], []
        for _ in range(a.rounds):
            hip.append(time_steps(hip_step, a.steps, a.warmup))
            if not a.only_hip:
                eager.append(time_steps(torch_step, a.steps, a.warmup))
        med = lambda v: sorted(v)[len(v) // 2] if v else float("nan")   # noqa: E731
        h_ms, t_ms = med(hip), med(eager)
        extra = {}
        if small or std:
            nbytes = b * (small_bytes_per_clip() if small else std_bytes_per_clip())
            extra = {"step_hbm_bytes": nbytes, "hip_hbm_bytes_per_s": round(nbytes / (h_ms * 1e-3), 1)}
        if std and b in conv_ms:
            conv_flops = b * 3 * std_flops_per_clip()[1]
            extra["convs123_ms"] = conv_ms[b]
            extra["convs123_share_of_f32_mfma_peak"] = round(conv_flops / (conv_ms[b] * 1e-3) / F32_MFMA_PEAK, 4)
        print(json.dumps({"model": a.model, "batch": b, "image": [H, W], "hip_ms": round(h_ms, 4), "torch_eager_ms": round(t_ms, 4),
                          "hip_clips_per_s": round(b / h_ms * 1e3, 1), "eager_clips_per_s": round(b / t_ms * 1e3, 1),
                          "speedup": round(t_ms / h_ms, 3), "hip_rounds_ms": [round(v, 4) for v in hip],
                          "step_gflop": round(b * step_flops / 1e9, 3),
                          "hip_share_of_f32_mfma_peak": round(b * step_flops / (h_ms * 1e-3) / F32_MFMA_PEAK, 4), **extra}),
              flush=True)


if __name__ == "__main__":
    main()
