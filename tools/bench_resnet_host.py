"""Host time per call of cough_resnet_forward where host dispatch is the largest share of a forward: one 90x101 clip, bf16x3.
2000 calls between two synchronisations, repeated; prints the per-call time of every repeat in microseconds."""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cough_detector_amd as cda                     # noqa: E402
from cough_detector_amd import _lib, synth           # noqa: E402

CALLS, REPEATS = 2000, int(sys.argv[1]) if len(sys.argv) > 1 else 5
m = cda.create_model("residual", n_mels=90, num_classes=2, in_channels=1, compute_dtype="bf16x3")
m.load_state_dict(synth.random_state_dict(seed=3))
m.cuda().eval()
x = torch.rand(1, 1, 90, 101, device="cuda")
m(x)
lib, h = _lib.load(), m._native()
ws = torch.empty(max(lib.cough_resnet_workspace_bytes(h, 1, 90, 101), 256), dtype=torch.uint8, device="cuda")
logits = torch.empty((1, 2), dtype=torch.float32, device="cuda")
args = (h, x.data_ptr(), 1, 90, 101, logits.data_ptr(), None, None, ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
for _ in range(200):
    lib.cough_resnet_forward(*args)
out = []
for _ in range(REPEATS):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(CALLS):
        lib.cough_resnet_forward(*args)
    t1 = time.perf_counter()          # every call has returned: host time of the launches
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    out.append((1e6 * (t1 - t0) / CALLS, 1e6 * (t2 - t0) / CALLS))
print("cough_resnet_forward B=1 90x101 bf16x3, us per call (host return / with the final synchronise):",
      " ".join(f"{a:.2f}/{b:.2f}" for a, b in out))
