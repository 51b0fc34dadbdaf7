"""Workload for a kernel trace of the conv-stack classifiers' dispatch: every (case, dtype) of tests/cnn_layer_ref.CASES once
through forward, the 90x101 standard and small nets once through conv_output, and one CoughPipeline forward per dtype for
"standard".  Run it under `rocprofv3 --kernel-trace` for two builds and compare the traces with
tools/compare_kernel_traces.py: the (kernel, grid, workgroup, LDS) sequences must be equal."""
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import cough_detector_amd as cda                       # noqa: E402
import cnn_layer_ref as R                              # noqa: E402
from cough_detector_amd import synth                   # noqa: E402
from cough_detector_amd.pipeline import CoughPipeline  # noqa: E402
from test_gpu_cnn_layers import _StackNet              # noqa: E402

warnings.simplefilter("ignore")
torch.manual_seed(0)
g = np.load(os.path.join(ROOT, "tests", "golden", "cnn_golden.npz"))
GOLDEN = {kind: {k[len(kind) + 4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(kind + ".sd.")} for kind in R.BLOCKS}


def blocks_of(case):
    if case.net in R.BLOCKS:
        return R.BLOCKS[case.net](GOLDEN[case.net])
    return R.random_blocks(R.GENERIC[case.net], seed=sum(map(ord, case.net)))


OUT = {}                                               # COUGH_TRACE_OUT=<file>: the outputs, to compare two builds bit for bit
for case in R.CASES:
    x = R.case_image(case).cuda()
    for dtype in R.case_dtypes(case):
        m = _StackNet(blocks_of(case), dtype).cuda().eval()
        logits = m(x)
        torch.cuda.synchronize()
        OUT[f"{case.name}-{dtype}"] = logits.cpu()
        print(case.name, dtype, "finite" if bool(torch.isfinite(logits).all()) else "non-finite")
        if case.name in ("std_90x101", "small_90x101"):
            act = m.conv_output(x)
            torch.cuda.synchronize()
            OUT[f"{case.name}-{dtype}-conv_output"] = act.cpu()
wav = torch.from_numpy(synth.make_clips(0, 5)).cuda()
pre = cda.AudioPreprocessor(use_pcen=False, use_pre_emphasis=False, use_delta_delta=False, use_spectral_contrast=False, device="cuda")
for dtype in R.DTYPES:
    m = cda.create_model("standard", n_mels=90, num_classes=2, in_channels=1, compute_dtype=dtype)
    m.load_state_dict(GOLDEN["standard"])
    m.cuda().eval()
    logits = CoughPipeline(pre, m)(wav)
    torch.cuda.synchronize()
    OUT["pipeline-" + dtype] = logits.cpu()
    print("pipeline", dtype, [round(v, 4) for v in logits[0].tolist()])
if os.environ.get("COUGH_TRACE_OUT"):
    torch.save(OUT, os.environ["COUGH_TRACE_OUT"])
