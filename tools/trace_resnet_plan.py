"""Workload for a kernel trace of the residual net's dispatch: every model of tests/resnet_layer_ref.CASES once (batch 5),
one cough_pipeline_forward per dtype and one lone ResidualBlock.  Run it under `rocprofv3 --kernel-trace` for two builds and
compare the traces with tools/compare_kernel_traces.py: the (kernel, grid, workgroup, LDS) sequences must be equal."""
import os
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import cough_detector_amd as cda                     # noqa: E402
import resnet_layer_ref as R                         # noqa: E402
from cough_detector_amd import synth                 # noqa: E402
from cough_detector_amd.model import ResidualBlock   # noqa: E402
from cough_detector_amd.pipeline import CoughPipeline  # noqa: E402

warnings.simplefilter("ignore")
torch.manual_seed(0)
OUT = {}                                             # COUGH_TRACE_OUT=<file>: the logits, to compare two builds bit for bit
for case in R.CASES:
    m = cda.create_model("residual", n_mels=case.H, num_classes=2, in_channels=1, channels=case.channels, compute_dtype=case.dtype)
    m.load_state_dict(R.case_weights(case))
    m.cuda().eval()
    logits = m(R.case_image(case).cuda())
    torch.cuda.synchronize()
    OUT[R.case_id(case)] = logits.cpu()
    print(R.case_id(case), "finite" if bool(torch.isfinite(logits).all()) else "non-finite")
wav = torch.from_numpy(synth.make_clips(0, 5)).cuda()
pre = cda.AudioPreprocessor(use_pcen=False, use_pre_emphasis=False, use_delta_delta=False, use_spectral_contrast=False, device="cuda")
for dtype in R.DTYPES:
    m = cda.create_model("residual", n_mels=90, num_classes=2, in_channels=1, compute_dtype=dtype)
    m.load_state_dict(synth.random_state_dict(seed=3))
    m.cuda().eval()
    logits = CoughPipeline(pre, m)(wav)
    torch.cuda.synchronize()
    OUT["pipeline-" + dtype] = logits.cpu()
    print("pipeline", dtype, [round(v, 4) for v in logits[0].tolist()])
blk = ResidualBlock(32, 64).cuda()
y = blk(torch.randn(3, 32, 22, 25, generator=torch.Generator().manual_seed(1)).cuda())
torch.cuda.synchronize()
OUT["ResidualBlock"] = y.cpu()
print("ResidualBlock", tuple(y.shape))
if os.environ.get("COUGH_TRACE_OUT"):
    torch.save(OUT, os.environ["COUGH_TRACE_OUT"])
