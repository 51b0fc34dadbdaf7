"""Split-bf16 classifier forwards at every image height block 0 (resblock_x3_kernel<32, 64, 1, R, 25>) is compiled for, from
resident random feature images: run under a kernel trace (tools/prof_stats.sh <outdir> tools/block0_heights.py [B]) for the
per-height kernel times.  Run on the GPU box."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cough_detector_amd as cda
from cough_detector_amd import synth
from cough_detector_amd.hostcpu import bound_torch_threads

bound_torch_threads()
B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
ROWS = {64: 16, 68: 17, 90: 22, 92: 23, 96: 24, 103: 26, 110: 27}   # image rows -> block-0 input rows (101 frames)
sd = synth.random_state_dict(seed=3)
for rows, r0 in ROWS.items():
    m = cda.create_model("residual", n_mels=rows, compute_dtype="bf16x3")
    m.load_state_dict(sd)
    m.cuda().eval()
    assert m.effective_dtype(rows, 101) == "bf16x3"
    xs = [torch.rand(B, 1, rows, 101, device="cuda") for _ in range(2)]
    for i in range(30):
        m(xs[i % 2])
    torch.cuda.synchronize()
    print(f"{rows} rows (block 0 at {r0}x25): done", flush=True)
