"""Host tests of tests/resnet_layer_ref.py: the float64 stages against oracle/resnet.py, the dispatch restatement against
the plans csrc/resnet_plan.h itself computes (tests/resnet_plan_dump.cpp) and against the hand-written table, the derived per-pixel bounds against a CPU emulation of each
operand scheme over the whole GPU matrix, and planted defects that the per-pixel check must flag."""
import atexit
import functools
import os
import re
import shutil
import subprocess
import tempfile

import pytest
import torch

import resnet_layer_ref as R
from cough_detector_amd import build as cbuild
from cough_detector_amd import synth
from oracle import resnet as ores

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("channels,shape", [((32, 64, 128), (90, 101)), ((32, 64, 128), (3, 3)), ((5, 7, 9), (40, 33)),
                                            ((64, 32), (17, 30)), ((8, 16, 24, 40), (37, 50))])
def test_stages_are_the_oracle(channels, shape):
    sd = synth.random_state_dict(seed=3, channels=channels)
    sd64 = {k: v.double() for k, v in sd.items()}
    x = torch.randn(2, 1, *shape, generator=torch.Generator().manual_seed(4)).double() * 2
    logits, acts = ores.forward(x, sd64, return_intermediates=True)
    got = [R.stem_pool(x, sd)]
    for i in range(R.n_blocks(sd)):
        got.append(R.block(got[-1], sd, i))
    assert len(got) == len(acts) == len(channels)
    assert [tuple(a.shape[2:]) for a in got] == R.make_shapes(*shape, len(channels) - 1)
    for a, b in zip(got, acts):
        assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))
    assert float((R.head(got[-1], sd) - logits).abs().max()) <= 1e-12
    # the folded form the bounds are built on is the same function
    w, b = R.fold(sd, "conv1.0", "conv1.1")
    y = torch.nn.functional.max_pool2d(torch.relu(torch.nn.functional.conv2d(x, w, b, stride=2, padding=3)), 2)
    assert float((y - acts[0]).abs().max()) <= 1e-12 * max(1.0, float(acts[0].abs().max()))
    (w1, b1), (w2, b2), (ws, bs) = R.block_folds(sd, 0)
    h = torch.relu(torch.nn.functional.conv2d(y, w1, b1, stride=2, padding=1))
    z = torch.relu(torch.nn.functional.conv2d(h, w2, b2 + bs, padding=1) + torch.nn.functional.conv2d(y, ws, stride=2))
    assert float((z - acts[1]).abs().max()) <= 1e-12 * max(1.0, float(acts[1].abs().max()))


# ------------------------------------------------------------------------------------------ the C++ plan against plan()
CSRC = os.path.join(ROOT, "cough_detector_amd", "csrc")


@functools.lru_cache(maxsize=None)
def _dump_exe():
    """tests/resnet_plan_dump.cpp built once per session by a host compiler: csrc/resnet_plan.h includes no HIP header."""
    out = tempfile.mkdtemp(prefix="resnet_plan_dump_")
    atexit.register(shutil.rmtree, out, ignore_errors=True)
    exe = os.path.join(out, "resnet_plan_dump")
    cxx = [shutil.which("c++")] if shutil.which("c++") else [cbuild._hipcc(), "-x", "c++"]
    subprocess.run([*cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "resnet_plan_dump.cpp"),
                    "-o", exe], check=True)
    return exe


def _dump(queries):
    """(constants of the header, one plan line per (dtype, H, W, channels) query)."""
    text = "".join(f"{d} {'shipped' if tuple(ch) == R.SHIPPED else 'generic'} {len(ch) - 1} {h} {w}\n" for d, h, w, ch in queries)
    out = subprocess.run([_dump_exe()], input=text, capture_output=True, text=True, check=True).stdout
    head, _, body = out.partition("---\n")
    consts = {ln.split()[0]: tuple(int(v) for v in ln.split()[1:]) for ln in head.splitlines()}
    lines = body.splitlines()
    assert len(lines) == len(queries)
    return consts, lines


def _tail(p, pipeline):
    """The NaN rule and the a3 store as resnet.hip applies them: block 1's fused split-bf16 head takes the per-clip flag, every
    other plan ends with nan_rule_kernel; behind the featuriser's stem a fused block 1 does not store its output."""
    nan = "flag" if pipeline else p.nan
    by = "block1" if nan == "flag" and len(p.blocks) == 2 and p.blocks[1].kernel == "resblock_x3" else "nan_rule_kernel"
    return f"{nan} by={by} a3={'skip' if pipeline and p.head == 'fused' else 'store'}"


def _line(dtype, H, W, channels=R.SHIPPED):
    """The line resnet_plan_dump prints for a query, from plan() and the launch arithmetic of resnet_layer_ref."""
    p = R.plan(dtype, H, W, channels)
    if p is None:
        return "none"
    stem_lds = {"stem_bf16<bf16>": 1, "stem_bf16<x3>": 2}.get(p.stem.kernel, 0) * R.stem_lds(H, W)
    parts = [f"{p.stem.kernel} lds={stem_lds}"]
    for i, b in enumerate(p.blocks):
        lds = R.rb_lds_bytes(R.RB_CFG[i], *b.in_hw, *b.out_hw) if b.kernel.startswith("resblock_bf16") else 0
        parts.append(f"{b.kernel} {b.body} {b.clips} {R.stage_path(b)} {b.in_hw[0]}x{b.in_hw[1]}->{b.out_hw[0]}x{b.out_hw[1]} lds={lds}")
    parts += [p.head, _tail(p, False)]
    if tuple(channels) == R.SHIPPED and dtype != "fp32":
        parts.append(f"pipeline: featurize_kernel {p.head} " + _tail(p, True))
    return " | ".join(parts)


def _row(line):
    """plan_row of a dumped line."""
    f = line.split(" | ")
    if f[-1].startswith("pipeline: "):
        f.pop()
    blocks = [(k, body, int(clips)) for k, body, clips in (b.split()[:3] for b in f[1:-2])]
    return (f[0].split()[0], blocks, f[-2], f[-1].split()[0])


def test_cxx_plan_gives_the_hand_written_row_of_every_case():
    _, lines = _dump([(c.dtype, c.H, c.W, c.channels) for c in R.CASES])
    for c, line in zip(R.CASES, lines):
        assert _row(line) == R.EXPECT[R.case_id(c)], (R.case_id(c), line)
        assert line == _line(c.dtype, c.H, c.W, c.channels)


def test_cxx_plan_is_plan_over_the_sweep():
    """plan_resnet (csrc/resnet_plan.h, what resnet.hip executes) against plan(), field by field: stem and its LDS, each block's
    kernel, body, clips, instantiation name, shapes and LDS, the head, the NaN rule and who applies it, the a3 store, and the
    same for the forward behind the featuriser's stem.  Every dtype over H, W = 1..130 and the low, wide strips up to 1600
    columns, which hold the deciding cases of every limit (named below), plus the generic tuples of the matrix."""
    hw = [(h, w) for h in range(1, 131) for w in range(1, 131)] + [(h, w) for h in range(1, 41) for w in range(131, 1601)]
    queries = [(d, h, w, R.SHIPPED) for d in R.DTYPES for h, w in hw]
    assert len(queries) == 227100
    for d in R.DTYPES:
        queries += [(d, 40, 33, (5, 7, 9)), (d, 17, 30, (64, 32))]
    _, lines = _dump(queries)
    at = {q[:3]: ln for q, ln in zip(queries, lines) if q[3] == R.SHIPPED}
    bad = [(q, ln) for q, ln in zip(queries, lines) if ln != _line(*q)]
    assert not bad, (len(bad), bad[0], _line(*bad[0][0]))
    # the sweep reaches every kernel path of the matrix ...
    seen = set()
    for ln in lines:
        if ln != "none":
            f = ln.split(" | ")
            seen.add(f[0].split()[0])
            seen.update(b.split()[3] for b in f[1:] if "->" in b)
            seen.add(f[-3] if f[-1].startswith("pipeline: ") else f[-2])
    assert {"stem_mfma<float>", "stem_mfma<bf16>", "stem_bf16<x3>", "stem_bf16<bf16>",
            "conv_mfma<float,1>", "conv_mfma<float,2>", "conv_mfma<float,4>", "conv_gemm_bf16<2>", "conv_gemm_bf16<4>",
            "resblock_x3<25,16x16x32,G1>", "resblock_x3<25,32x32,G1>", "resblock_x3<13,16x16x32,G1>", "resblock_x3<13,16x16x32,G2>",
            "resblock_bf16:fixed<G1>", "resblock_bf16:fixed<G3>", "resblock_bf16:runtime<G1>", "resblock_bf16:runtime<G3>",
            "fused", "tail_kernel<float>", "tail_kernel<bf16>", "tail_generic_kernel"} <= seen
    # ... and the two sides of every limit: the stem's pixel count, its two-plane LDS, block 1's pixel tiles, 160 KB alone
    assert at["bf16x3", 110, 102].startswith("stem_bf16<x3> ") and at["bf16x3", 110, 103].startswith("stem_mfma<float> ")
    assert at["bf16x3", 8, 1400].startswith("stem_mfma<float> ") and at["bf16_approx", 8, 1400].startswith("stem_bf16<bf16> lds=39368 ")
    assert "resblock_bf16:runtime<G3> 12x13->6x7" in at["bf16_approx", 96, 101] and "conv_gemm_bf16<4> 13x13->7x7" in at["bf16_approx", 99, 101]
    assert "resblock_bf16:runtime<G1> 8x84->4x42" in at["bf16_approx", 32, 336] and "conv_gemm_bf16<4> 4x42->2x21" in at["bf16_approx", 32, 336]
    assert "conv_gemm_bf16<2> 2x384->1x192" in at["bf16_approx", 8, 1536]      # 192 pixels fit the tiles; 173 312 B do not (2 x 362: 163 456 B do)
    assert "resblock_bf16:runtime<G1> 2x362->1x181 lds=163456" in at["bf16_approx", 8, 1448] and "conv_gemm_bf16<2> 2x363->1x182" in at["bf16_approx", 8, 1452]


def test_plan_constants_are_the_header_s_and_defined_once():
    """plan() restates the dispatch with constants of its own; this ties them to the header the library is built from, so a
    retune of STEM_SB_MAXL, the RBX row lists, RBX_G_TALL, the RbCfg parameter lists, the fixed geometries or the two LDS
    limits fails here until plan(), EXPECT and the matrix have been revisited."""
    consts, _ = _dump([])
    assert consts == {"STEM_SB_MAXL": (R.STEM_SB_MAXL,), "RBX_BLOCK0_ROWS": R.RBX_BLOCK0_ROWS, "RBX_BLOCK1_ROWS": R.RBX_BLOCK1_ROWS,
                      "RBX_COLS": (25, 13), "RBX_G_TALL": (R.RBX_G_TALL,), "NET_CH": R.SHIPPED, "RB_CFG": R.RB_CFG[0] + R.RB_CFG[1],
                      "RB_FIXED": R.RB_FIXED[0] + R.RB_FIXED[1], "RB_MTMAX": tuple(R.rb_mtmax(c) for c in R.RB_CFG),
                      "RB_THREADS": tuple(c[4] * 64 for c in R.RB_CFG), "STEM_LDS_LIMIT": (R.STEM_LDS_LIMIT,),
                      "RB_LDS_LIMIT": (R.RB_LDS_LIMIT,), "PLAN_MAX_BLOCKS": (16,)}
    assert R.RB_FIXED == ((22, 25), (11, 13)) and R.STEM_LDS_LIMIT == 64 * 1024 and R.RB_LDS_LIMIT == 160 * 1024
    # one definition in csrc/: no second list or constant to drift to
    src = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC))}
    for name in ("STEM_SB_MAXL", "RBX_BLOCK0_ROWS", "RBX_BLOCK1_ROWS", "RBX_COLS", "RBX_G_TALL", "RB_CFG", "RB_FIXED", "STEM_LDS_LIMIT",
                 "RB_LDS_LIMIT", "NET_CH"):
        defs = [f for f, text in src.items() for _ in re.findall(rf"(?:#define\s+{name}\b|\b{name}(?:\[\d*\])*\s*=[^=])", text)]
        assert defs == ["resnet_plan.h"], (name, defs)
    for rows in (R.RBX_BLOCK0_ROWS, R.RBX_BLOCK1_ROWS):          # ... under any name or as an X-macro
        lists = [f for f, text in src.items() for _ in re.findall(r"\D{1,6}".join(rf"\b{r}\b" for r in rows), text)]
        assert lists == ["resnet_plan.h"], (rows, lists)
    for fn in ("make_shapes", "stem_lds", "rbx_compiled", "rbx_t16", "rbx_block1_clips", "rb_lds_bytes", "rb_mtmax", "plan_resnet"):
        defs = [f for f, text in src.items() for _ in re.findall(rf"^(?:constexpr|inline|static)[\w \*&:<>]*\b{fn}\(", text, flags=re.M)]
        assert defs == ["resnet_plan.h"], (fn, defs)
    # no build of the library overrides the tables from the command line
    build_py = open(os.path.join(ROOT, "cough_detector_amd", "build.py")).read()
    assert "RBX_BLOCK" not in build_py and "STEM_SB_MAXL" not in build_py and "RBX_G_TALL" not in build_py
    # the Python side names the same block-0 inputs
    from cough_detector_amd.model import CoughDetectorResidual
    assert CoughDetectorResidual.X3_BLOCK_INPUTS == tuple((r, 25) for r in R.RBX_BLOCK0_ROWS)


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_plan_gives_the_hand_written_row(case):
    p = R.plan(case.dtype, case.H, case.W, case.channels)
    assert p is not None and R.plan_row(p) == R.EXPECT[R.case_id(case)], R.plan_row(p)


def test_plan_edges():
    assert len(R.EXPECT) == len(R.CASES) == len({R.case_id(c) for c in R.CASES})
    assert R.plan("fp32", 2, 101) is None and R.plan("fp32", 101, 2) is None and R.plan("fp32", 3, 3) is not None
    # the pixel limit of the staged stems: 110 x 102 = 11 220 inside, 110 x 103 = 11 330 outside
    assert R.plan("bf16x3", 110, 102).stem.kernel == "stem_bf16<x3>" and R.plan("bf16x3", 110, 103).stem.kernel == "stem_mfma<float>"
    assert 8 * 1400 <= 2 * 256 * R.STEM_SB_MAXL and 2 * R.stem_lds(8, 1400) == 78736 > R.STEM_LDS_LIMIT
    assert R.plan("bf16_approx", 8, 1400).stem.kernel == "stem_bf16<bf16>"        # one plane: 39 368 B fits
    # every image of the windows the issue names lands on the mixed dispatch, flag and fused head included
    for rows in (71, 72, 73, 74, 83, 84, 85, 86, 99, 100, 101, 102):
        for frames in (99, 100, 101, 102):
            p = R.plan("bf16x3", rows, frames)
            assert (p.blocks[0].kernel, p.blocks[1].kernel, p.head, p.nan) == ("conv_mfma<float,2>", "resblock_x3", "fused", "flag")
    for frames in (103, 104, 105, 106):
        p = R.plan("bf16x3", 90, frames)
        assert (p.blocks[0].kernel, p.blocks[1].kernel, p.head) == ("conv_mfma<float,2>", "resblock_x3", "fused")
    # the single-bf16 block-1 pixel limit: 96 rows sit on it, 99 rows (25 -> 13 -> 7 rows: 3 * 49) are over
    p96, p99 = R.plan("bf16_approx", 96, 101), R.plan("bf16_approx", 99, 101)
    assert 3 * p96.blocks[1].out_hw[0] * p96.blocks[1].out_hw[1] == 126 and p96.blocks[1].kernel == "resblock_bf16:runtime"
    assert p99.blocks[1].out_hw == (7, 7) and p99.blocks[1].kernel == "conv_gemm_bf16<4>"
    # the case that the 160 KB limit alone decides
    p = R.plan("bf16_approx", 32, 336)
    (xh, xw), (oh, ow) = p.blocks[1].in_hw, p.blocks[1].out_hw
    assert (xh, xw, oh, ow) == (4, 42, 2, 21) and 3 * oh * ow <= R.rb_mtmax(R.RB_CFG[1]) * 32
    assert 3 * xh * xw * 8 <= 16 * 512 and R.rb_lds_bytes(R.RB_CFG[1], xh, xw, oh, ow) == 172032 > R.RB_LDS_LIMIT


def test_matrix_reaches_every_path_of_the_dispatch():
    """The paths the matrix exists for, read off plan(): a retune that empties one of them fails here instead of the coverage moving silently."""
    seen = set()
    for c in R.CASES:
        p = R.plan(c.dtype, c.H, c.W, c.channels)
        seen.add(p.stem.kernel)
        seen.update(R.stage_path(b) for b in p.blocks)
        seen.add((c.dtype, p.head))
        if c.nan:
            seen.add((c.dtype, "nan", p.nan))
    need = {"stem_mfma<float>", "stem_mfma<bf16>", "stem_bf16<x3>", "stem_bf16<bf16>",
            "conv_mfma<float,1>", "conv_mfma<float,2>", "conv_mfma<float,4>", "conv_gemm_bf16<2>", "conv_gemm_bf16<4>",
            "resblock_x3<25,16x16x32,G1>", "resblock_x3<25,32x32,G1>", "resblock_x3<13,16x16x32,G1>", "resblock_x3<13,16x16x32,G2>",
            "resblock_bf16:fixed<G1>", "resblock_bf16:fixed<G3>", "resblock_bf16:runtime<G1>", "resblock_bf16:runtime<G3>",
            ("fp32", "tail_kernel<float>"), ("fp32", "tail_generic_kernel"), ("bf16x3", "fused"), ("bf16x3", "tail_kernel<float>"),
            ("bf16_approx", "fused"), ("bf16_approx", "tail_kernel<bf16>"),
            ("bf16x3", "nan", "flag"), ("bf16x3", "nan", "rescan"), ("bf16_approx", "nan", "flag")}
    assert need <= seen, need - seen


def test_which_launch_limits_of_the_bf16_blocks_can_bind():
    """The statements of plan()'s docstring, by exhaustion over every block input up to 2048 pixels a side: the staging
    limit never decides a launch (the pixel limit has always tripped before it), the 160 KB limit does."""
    assert (R.rb_mtmax(R.RB_CFG[0]), R.rb_mtmax(R.RB_CFG[1])) == (6, 4)
    lds_alone = {0: [], 1: []}
    for i, cfg in enumerate(R.RB_CFG):
        cin, _, g, _, waves = cfg
        for xh in range(1, 2049):
            oh = (xh - 1) // 2 + 1
            for xw in range(1, 2049):
                ow = (xw - 1) // 2 + 1
                if g * oh * ow > R.rb_mtmax(cfg) * 32:
                    break                                                   # wider only adds pixels
                assert g * xh * xw * (cin // 8) <= 16 * waves * 64, (i, xh, xw)
                if R.rb_lds_bytes(cfg, xh, xw, oh, ow) > R.RB_LDS_LIMIT:
                    lds_alone[i].append((xh, xw))
    assert (2, 384) in lds_alone[0] and (4, 42) in lds_alone[1]
    # only strips: the shorter side of such an input is 2 pixels (block 0) or at most 4 (block 1)
    assert {min(s) for s in lds_alone[0]} == {2} and {min(s) for s in lds_alone[1]} == {1, 2, 4}


# ------------------------------------------------------------------------------------------ the emulation under the bound
@functools.lru_cache(maxsize=None)
def _setup(case, batch=2):
    sd = R.case_weights(case)
    return sd, R.case_image(case, batch), R.plan(case.dtype, case.H, case.W, case.channels)


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_clean_emulation_stays_within_the_bound_at_every_pixel(case):
    sd, x, p = _setup(case)
    acts = R.emulate_net(x, sd, p)
    worst = R.check_net(x, sd, p, lambda k: acts[k - 1])
    for w in worst:
        print(f"{R.case_id(case)} stage {w.stage} {w.kernel}: emulated / bound {w.ratio:.3f}")
    assert max(w.ratio for w in worst) <= 1.0, worst
    ref, e_l = R.head_bound(acts[-1], sd)               # the head in float32 arithmetic, torch's summation order
    got = torch.nn.functional.linear(acts[-1].float().mean(dim=(2, 3)), sd["fc.2.weight"], sd["fc.2.bias"]).double()
    assert float((R.head(acts[-1], sd) - ref).abs().max()) <= 1e-12 and float(((got - ref).abs() / e_l).max()) <= 1.0


# ------------------------------------------------------------------------------------------ planted defects
def _case(dtype, H, W):
    return [c for c in R.CASES if (c.dtype, c.H, c.W) == (dtype, H, W) and c.channels == R.SHIPPED][0]


# defect -> (matrix case that catches it, stage: "stem" or the block).  Ratios of the CPU emulation at the worst pixel are in
# profiles/resnet_layer_precision.txt.  The f32 convs (fp32 cases), the split-bf16 fused blocks with one and with two clips
# per workgroup (bf16x3 90x101 / 96x101 / 63x99; 103x101 and 110x102: the one-clip block 1 and the 32x32 body) and the
# single-bf16 fused and GEMM blocks (bf16_approx 64x101, 110x101) each catch what their budget can see:
# * the split-bf16 budget of a block is dominated by its float32 accumulation term (3 K u = 2.2e-4 at K = 1216 against
#   3 * 2^-18 = 1.1e-5), so a dropped lo*hi product (2^-9 per term, random signs) shows in block 0 (ratio 1.7) and in the
#   stem (K = 49), but reaches only 0.80 in block 1;
# * the single-bf16 budget is 2^-7 of sum |w x|: a wrapped border column (0.75), a neighbour clip's h (0.76) and a swapped
#   k-step (0.40) move a few of the K terms of a sum with random signs and stay under it; a wrong projection centre (5.3)
#   and a missing skip bias (4.2) do not.  Those three are caught by the fp32 and bf16x3 cases of the same shapes.
PLANTED = [
    ("drop_lo_hi", ("bf16x3", 63, 99), "stem"), ("drop_lo_hi", ("bf16x3", 90, 101), 0),
    ("border_wrap", ("fp32", 90, 101), 0), ("border_wrap", ("bf16x3", 90, 101), 1),
    ("proj_centre", ("fp32", 90, 101), 1), ("proj_centre", ("bf16x3", 103, 101), 0), ("proj_centre", ("bf16_approx", 110, 101), 1),
    ("clip_h", ("bf16x3", 90, 101), 1), ("clip_h", ("bf16x3", 96, 101), 1),
    ("bias_no_skip", ("fp32", 3, 3), 1), ("bias_no_skip", ("bf16x3", 110, 102), 0), ("bias_no_skip", ("bf16_approx", 64, 101), 1),
    ("kstep_swap", ("fp32", 17, 33), 0), ("kstep_swap", ("bf16x3", 63, 99), 1),
]


@pytest.mark.parametrize("defect,where,blk", PLANTED, ids=[f"{d}-{w[0]}-{w[1]}x{w[2]}-{b}" for d, w, b in PLANTED])
def test_planted_defect_exceeds_the_bound_at_some_pixel(defect, where, blk):
    case = _case(*where)
    sd, x, p = _setup(case, 3 if defect == "clip_h" else 2)
    clean = R.emulate_net(x, sd, p)
    assert max(w.ratio for w in R.check_net(x, sd, p, lambda k: clean[k - 1])) <= 1.0
    idx = 0 if blk == "stem" else blk + 1                   # position of the stage among the taps
    stage = p.stem if blk == "stem" else p.blocks[blk]
    if defect == "clip_h":
        assert stage.clips >= 2
    if defect == "border_wrap":
        assert stage.in_hw[1] % 2 == 1                      # a stride-2 conv reads the right border only of an odd width
    bad = R.emulate_net(x, sd, p, defect, blk)
    worst = R.check_net(x, sd, p, lambda k: bad[k - 1])
    at = worst[idx]
    print(f"PLANTED {defect} in {blk} of {R.case_id(case)} ({stage.kernel}): ratio {at.ratio:.3g} at clip {at.clip} "
          f"ch {at.channel} row {at.row} col {at.col}; the stages before it {max([w.ratio for w in worst[:idx]] + [0.0]):.3f}")
    assert at.ratio > 1.0
    assert all(w.ratio <= 1.0 for w in worst[:idx])         # the check names the stage: everything before it is clean
    if defect == "clip_h":                                  # ... and the clip: the first clip of a workgroup is clean
        first = R.check_stage(blk, "", bad[blk + 1][:1], R.block(bad[blk][:1], sd, blk),
                              R.stage_bound(blk, bad[blk][:1], sd, p.blocks[blk].scheme, p.stores_bf16))
        assert first.ratio <= 1.0 and at.clip % p.blocks[blk].clips == 1


def test_every_defect_is_caught_and_every_family_catches_one():
    by = {}
    for d, where, blk in PLANTED:
        c = _case(*where)
        p = R.plan(c.dtype, c.H, c.W)
        by.setdefault(d, set()).add((p.stem if blk == "stem" else p.blocks[blk]).scheme)
    assert set(by) == set(R.DEFECTS)
    assert by["drop_lo_hi"] == {"bf16x3"}                                    # the only scheme that has a lo operand
    assert set().union(*by.values()) == {"f32", "bf16x3", "bf16"}
    assert all({"f32", "bf16x3"} <= by[d] for d in ("border_wrap", "proj_centre", "bias_no_skip", "kstep_swap"))
