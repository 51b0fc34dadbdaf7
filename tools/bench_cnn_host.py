"""Host time per call of cough_cnn_forward for the two shipped conv-stack nets at B = 1 (where host dispatch is the largest
share of a forward) and B = 32: 90x101 clips, bf16x3.  1000 calls between two synchronisations, repeated; prints the
per-call time of every repeat in microseconds."""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cough_detector_amd as cda                     # noqa: E402
from cough_detector_amd import _lib                  # noqa: E402

CALLS, REPEATS = 1000, int(sys.argv[1]) if len(sys.argv) > 1 else 5
for kind in ("standard", "small"):
    torch.manual_seed(3)
    m = cda.create_model(kind, n_mels=90, num_classes=2, in_channels=1, compute_dtype="bf16x3")
    m.cuda().eval()
    for batch in (1, 32):
        x = torch.rand(batch, 1, 90, 101, device="cuda")
        m(x)
        lib, h = _lib.load(), m._native()
        ws = torch.empty(max(lib.cough_cnn_workspace_bytes(h, batch, 90, 101), 256), dtype=torch.uint8, device="cuda")
        logits = torch.empty((batch, 2), dtype=torch.float32, device="cuda")
        args = (h, x.data_ptr(), batch, 90, 101, logits.data_ptr(), None, None, ws.data_ptr(), ws.numel(),
                torch.cuda.current_stream().cuda_stream)
        for _ in range(200):
            lib.cough_cnn_forward(*args)
        out = []
        for _ in range(REPEATS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(CALLS):
                lib.cough_cnn_forward(*args)
            t1 = time.perf_counter()          # every call has returned: host time of the launches
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            out.append((1e6 * (t1 - t0) / CALLS, 1e6 * (t2 - t0) / CALLS))
        print(f"cough_cnn_forward {kind} B={batch} 90x101 bf16x3, us per call (host return / with the final synchronise):",
              " ".join(f"{a:.2f}/{b:.2f}" for a, b in out))
