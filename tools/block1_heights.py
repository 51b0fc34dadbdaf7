"""Split-bf16 classifier forwards at every image height block 1 (resblock_x3_kernel<64, 128, G, R, 13>) is compiled for,
from resident random feature images: run under a kernel trace (tools/prof_stats.sh <outdir> tools/block1_heights.py [B])
for the per-height kernel times.  Run on the GPU box."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cough_detector_amd as cda
from cough_detector_amd import synth
from cough_detector_amd.hostcpu import bound_torch_threads

bound_torch_threads()
B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
ROWS = {64: 8, 68: 9, 90: 11, 92: 12, 103: 13, 110: 14}   # image rows -> block-1 input rows (101 frames)
sd = synth.random_state_dict(seed=3)
for rows, r1 in ROWS.items():
    m = cda.create_model("residual", n_mels=rows, compute_dtype="bf16x3")
    m.load_state_dict(sd)
    m.cuda().eval()
    assert m.effective_dtype(rows, 101) == "bf16x3"
    xs = [torch.rand(B, 1, rows, 101, device="cuda") for _ in range(2)]
    for i in range(30):
        m(xs[i % 2])
    torch.cuda.synchronize()
    print(f"{rows} rows (block 1 at {r1}x13): done", flush=True)
