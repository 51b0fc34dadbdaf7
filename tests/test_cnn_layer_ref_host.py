"""Host tests of tests/cnn_layer_ref.py: the float64 block list against oracle/cnn.py, the dispatch restatement against a
hand-checked table and against the plans csrc/cnn_plan.h itself computes (tests/cnn_plan_dump.cpp), the derived per-pixel
bounds against a CPU emulation of each operand scheme over the whole GPU matrix (within HALF of the bound), and planted
defects that the per-pixel check flags while the logits stay within LOGIT_TOL."""
import atexit
import functools
import os
import re
import shutil
import subprocess
import tempfile

import pytest
import torch

import cnn_layer_ref as R
from cough_detector_amd import build as cbuild
from oracle import cnn as ocnn
from parity import LOGIT_TOL


def _f64(sd):
    return {k: v.double() for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def _case_blocks(net):
    return R.random_blocks(R.GENERIC[net], seed=sum(map(ord, net)))


def _blocks(case, cnn_golden):
    if case.net in R.BLOCKS:
        return R.BLOCKS[case.net](cnn_golden[case.net][0])
    return _case_blocks(case.net)


@pytest.mark.parametrize("kind", ["standard", "small"])
def test_block_list_is_the_oracle(cnn_golden, kind):
    sd, _ = cnn_golden[kind]
    x = torch.cat([cnn_golden["x"][:2].double(), R.case_image(R.Case("p", kind, 90, 101, 2, False)).double()])
    got = R.features(x, R.BLOCKS[kind](sd))[-1]
    want = ocnn.FEATURES[kind](x, _f64(sd))
    assert got.shape == want.shape and float((got - want).abs().max()) <= 1e-12
    # the folded form the bounds are built on is the same function
    y = x
    for b in R.BLOCKS[kind](sd):
        w, bias = R.fold(b)
        y = torch.relu(torch.nn.functional.conv2d(y, w, bias, padding=1))
        y = torch.nn.functional.max_pool2d(y, 2) if b.pool == 2 else y
    assert float((y - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


def test_plan_table():
    def t(dims, dtype, h, w):
        return [(s.kernel, s.band_rows, s.n_bands, s.fused_mean) for s in R.plan(dims, dtype, h, w)]
    F_, T_ = False, True
    assert t(R.STD_DIMS, "bf16x3", 90, 101) == [("first_x3", 0, 0, F_), ("lds_x3", 3, 8, F_), ("lds_x3", 4, 3, F_), ("lds_x3", 5, 1, T_)]
    assert t(R.SMALL_DIMS, "bf16x3", 90, 101) == [("first_x3", 0, 0, F_), ("lds_x3", 5, 5, F_), ("lds_x3", 6, 2, F_), ("lds_x3", 11, 1, T_)]
    # 64 x 47: first 32 x 23; Standard 16 x 11 (320 / 44 = 7 rows), 8 x 5 (192 / 20 = 9 -> 8), 4 x 2 (128 / 8 = 16 -> 4)
    assert t(R.STD_DIMS, "bf16x3", 64, 47) == [("first_x3", 0, 0, F_), ("lds_x3", 7, 3, F_), ("lds_x3", 8, 1, F_), ("lds_x3", 4, 1, T_)]
    # Small: 16 x 11 (512 / 44 = 11), 8 x 5 (320 / 20 = 16 -> 8), 8 x 5 unpooled (192 / 5 = 38 -> 8)
    assert t(R.SMALL_DIMS, "bf16x3", 64, 47) == [("first_x3", 0, 0, F_), ("lds_x3", 11, 2, F_), ("lds_x3", 8, 1, F_), ("lds_x3", 8, 1, T_)]
    assert t(R.STD_DIMS, "fp32", 90, 101) == [("first", 0, 0, F_)] + [("conv_f32", 0, 0, F_)] * 3
    assert [s.nt for s in R.plan(R.STD_DIMS, "fp32", 90, 101)] == [1, 2, 4, 4]
    # single bf16: 512 / 100 = 5 rows of 22; 256 / 48 = 5 rows of 11; 128 -> 256 has no LDS-image kernel
    assert t(R.STD_DIMS, "bf16_approx", 90, 101) == [("first", 0, 0, F_), ("lds_bf16", 5, 5, F_), ("lds_bf16", 5, 3, F_), ("gemm_bf16", 0, 0, F_)]
    assert t(R.SMALL_DIMS, "bf16_approx", 64, 47) == [("first", 0, 0, F_), ("lds_bf16", 11, 2, F_), ("lds_bf16", 8, 1, F_), ("lds_bf16", 8, 1, F_)]
    # odd H * W, the f32 first block above 11 264 pixels, the image that vanishes
    assert R.plan(R.STD_DIMS, "bf16x3", 91, 101)[0].odd_hw and not R.plan(R.STD_DIMS, "bf16x3", 90, 101)[0].odd_hw
    assert R.plan(R.STD_DIMS, "bf16x3", 128, 128)[0].kernel == "first" and R.plan(R.STD_DIMS, "bf16x3", 110, 101)[0].kernel == "first_x3"
    assert R.plan(R.STD_DIMS, "fp32", 15, 101) is None and R.plan(R.STD_DIMS, "fp32", 16, 16) is not None
    assert R.plan(R.SMALL_DIMS, "bf16x3", 7, 64) is None and R.plan(R.SMALL_DIMS, "bf16x3", 8, 8) is not None
    # the 32-channel layer at 150 columns needs 4 * 152 * 8 = 4864 pieces for ONE row: f32 between split-bf16 neighbours
    assert t(R.STD_DIMS, "bf16x3", 40, 300)[1:] == [("conv_f32", 0, 0, F_), ("lds_x3", 1, 5, F_), ("lds_x3", 1, 2, F_)]
    assert R.plan(R.STD_DIMS, "bf16_approx", 64, 400)[1].kernel == "unsupported"


# ------------------------------------------------------------------------------------------ the C++ plan against plan()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cough_detector_amd", "csrc")
ALL_DIMS = {"standard": R.STD_DIMS, "small": R.SMALL_DIMS, **{k: [(a, b, p) for a, b, p, _ in v] for k, v in R.GENERIC.items()}}


@functools.lru_cache(maxsize=None)
def _dump_exe():
    """tests/cnn_plan_dump.cpp built once per session by a host compiler: csrc/cnn_plan.h includes no HIP header."""
    out = tempfile.mkdtemp(prefix="cnn_plan_dump_")
    atexit.register(shutil.rmtree, out, ignore_errors=True)
    exe = os.path.join(out, "cnn_plan_dump")
    cxx = [shutil.which("c++")] if shutil.which("c++") else [cbuild._hipcc(), "-x", "c++"]
    subprocess.run([*cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cnn_plan_dump.cpp"),
                    "-o", exe], check=True)
    return exe


def _dump(queries):
    """(constants of the header, one line per query).  A query is a ready "forms ..." string or (dims, dtype, H, W, mode)."""
    text = "".join(q + "\n" if isinstance(q, str) else
                   f"{q[1]} {len(q[0])} {' '.join(f'{a} {b} {p}' for a, b, p in q[0])} {q[2]} {q[3]} {q[4]}\n" for q in queries)
    out = subprocess.run([_dump_exe()], input=text, capture_output=True, text=True, check=True).stdout
    head, _, body = out.partition("---\n")
    consts = {ln.split()[0]: tuple(int(v) for v in ln.split()[1:]) for ln in head.splitlines()}
    lines = body.splitlines()
    assert len(lines) == len(queries)
    return consts, lines


def _row(line):
    """(kernel, band_rows, n_bands, fused mean) per layer of a dumped line: the columns of R.EXPECT."""
    layers = [f.split() for f in line.split(" | ") if "->" in f]
    return [(f[0], int(f[2]), int(f[3]), f[6] == "1") for f in layers]


def test_cxx_plan_gives_the_hand_written_row_of_every_case():
    queries = [(R.case_dims(c), dt, c.H, c.W, "forward") for c in R.CASES for dt in R.case_dtypes(c)]
    names = [(c.name, dt) for c in R.CASES for dt in R.case_dtypes(c)]
    _, lines = _dump(queries)
    assert set(R.EXPECT) <= set(names)
    for name, q, line in zip(names, queries, lines):
        if name in R.EXPECT:
            assert _row(line) == R.EXPECT[name], (name, line)
        assert line == R.plan_line(*q), (name, line, R.plan_line(*q))


def test_cxx_plan_is_plan_over_the_sweep():
    """plan_cnn (csrc/cnn_plan.h, what cnn.hip executes) against plan(), field by field: each layer's kernel, tiles, band,
    bands per clip, dynamic LDS, grid, fused mean, odd pixel count and shapes, the ping-pong buffer, the head's HW and the
    single-bf16 refusal.  Both shipped nets and every generic net of the matrix, the three dtypes, both entry points, over
    H, W = 1..40 densely, the values around 90 / 101 / 110 / 128 and the wide and tall 300 and 400."""
    grid = list(range(1, 41)) + [47, 64, 72, 88, 89, 90, 91, 99, 100, 101, 102, 109, 110, 111, 112, 127, 128, 129, 300, 400]
    queries = [(dims, dt, h, w, mode) for dims in ALL_DIMS.values() for dt in R.DTYPES for mode in R.MODES for h in grid for w in grid]
    assert len(queries) == 7 * 3 * 2 * 60 * 60
    # low, wide strips through a two-block net: under 11 264 pixels, the two planes of the first block's image reach 64 KB
    strip = [(1, 16, 2), (16, 32, 2)]
    queries += [(strip, dt, h, w, mode) for dt in R.DTYPES for mode in R.MODES for h in (4, 8) for w in (1400, 2334, 2336)]
    _, lines = _dump(queries)
    bad = [(q, ln) for q, ln in zip(queries, lines) if ln != R.plan_line(*q)]
    assert not bad, (len(bad), bad[0], R.plan_line(*bad[0][0]))
    # the sweep reaches every kernel, the refusal, the vanishing image and both answers of the fused mean in each mode
    seen = {f.split()[0] for ln in lines for f in ln.split(" | ")[:-1]} | {ln for ln in lines if ln == "none"}
    assert {"first", "first_x3", "conv_f32", "lds_x3", "lds_bf16", "gemm_bf16", "conv_bf16", "unsupported", "none"} <= seen
    at = {(tuple(q[0]), *q[1:]): ln for q, ln in zip(queries, lines)}
    std = tuple(R.STD_DIMS)
    assert at[std, "bf16x3", 90, 101, "forward"].endswith("head_hw=1") and at[std, "bf16x3", 90, 101, "conv_output"].endswith("head_hw=30")
    assert at[std, "bf16x3", 110, 101, "forward"].endswith("head_hw=36")                # two bands: no fused mean
    assert at[std, "bf16_approx", 64, 400, "forward"].endswith("unsupported=1 32x200")
    # the two sides of the first block's limits: 110 x 102 = 11 220 pixels inside, 110 x 103 outside; 2 planes of 64 KB
    assert at[std, "bf16x3", 110, 102, "forward"].startswith("first_x3 ") and at[std, "bf16x3", 111, 102, "forward"].startswith("first ")
    assert at[std, "bf16x3", 27, 400, "forward"].startswith("first_x3 0 0 0 lds=48720 ") and at[std, "bf16x3", 1, 400, "forward"] == "none"
    assert at[tuple(strip), "bf16x3", 8, 1400, "forward"].startswith("first_x3 0 0 0 lds=61864 ")       # over 60 KB
    assert at[tuple(strip), "bf16x3", 4, 2334, "forward"].startswith("first_x3 0 0 0 lds=65520 ") and \
        at[tuple(strip), "bf16x3", 4, 2336, "forward"].startswith("first ")                               # 65 576 B do not fit


def test_capability_record_is_what_plan_assumes():
    """layer_forms (what cough_cnn_create packs and the forward reads) against the conditions plan() uses, over
    cin 8..256 step 8 x cout {32, 64, 96, 128, 256} x pool {1, 2}, every dtype, first and later layers."""
    combos = [(dt, i, cin, cout, pool) for dt in R.DTYPES for i in (0, 1) for cin in range(8, 257, 8) for cout in (32, 64, 96, 128, 256)
              for pool in (1, 2)]
    _, lines = _dump([f"forms {dt} {i} {cin} {cout} {pool}" for dt, i, cin, cout, pool in combos])
    for (dt, i, cin, cout, pool), line in zip(combos, lines):
        later, approx, x3 = i > 0, dt == "bf16_approx", dt == "bf16x3"
        gemm = later and approx and cin % 32 == 0 and cout % 64 == 0
        want = (later and approx, -(-9 * cin // 64) * 64 if gemm else 9 * cin, gemm,
                later and approx and (cin, cout) in ((16, 32), (32, 64), (64, 128)),
                later and x3 and cin in R.X3_CFG and (cout in (32, 64) or cout % 128 == 0),
                not later and x3 and pool == 2 and cout <= 32)
        assert tuple(int(v) for v in line.split()) == tuple(int(v) for v in want), (dt, i, cin, cout, pool, line)


def test_plan_constants_are_the_header_s_and_defined_once():
    """plan() restates the dispatch with constants of its own; this ties them to the header the library is built from, so a
    retune of CNN_X3_TABLE, CNN_FIRST_MAXL, CNN_LDS_UNP, the single-bf16 tile list or the first block's LDS limit fails
    here until plan(), the hand-checked tables and the matrix have been revisited."""
    consts, _ = _dump([])
    x3 = tuple(v for cin, (nt, mw, wm, wn, pieces) in R.X3_CFG.items() for v in (cin, nt, mw, wm, wn, pieces, int(cin == 32)))
    assert consts == {"CNN_FIRST_MAXL": (R.FIRST_MAXL,), "CNN_FIRST_LDS_LIMIT": (64 * 1024,), "CNN_LDS_UNP": (R.LDS_UNP,),
                      "CNN_LDS_CFG": (16, 1, 4, 32, 2, 4, 64, 4, 2), "CNN_X3_TABLE": x3,
                      "CNN_X3_THREADS": tuple(64 * c[2] * c[3] for c in R.X3_CFG.values()),
                      "CNN_X3_MAX_LDS": tuple(16 * c[4] + 64 for c in R.X3_CFG.values()), "PLAN_MAX_LAYERS": (16,)}
    assert (R.FIRST_MAXL, R.LDS_UNP) == (22, 12)
    # one definition in csrc/: no second list or constant to drift to
    src = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC))}
    for name in ("CNN_FIRST_MAXL", "CNN_FIRST_LDS_LIMIT", "CNN_LDS_UNP", "CNN_LDS_CFG", "CNN_X3_TABLE", "PLAN_MAX_LAYERS"):
        defs = [f for f, text in src.items() for _ in re.findall(rf"(?:#define\s+{name}\b|\b{name}(?:\[\d*\])*\s*=[^=])", text)]
        assert defs == ["cnn_plan.h"], (name, defs)
    for fn in ("first_lds", "layer_forms", "x3_band", "x3_lds_bytes", "lds_band", "lds_bytes", "conv_nt", "plan_cnn"):
        defs = [f for f, text in src.items() for _ in re.findall(rf"^(?:constexpr|inline|static)[\w \*&:<>]*\b{fn}\(", text, flags=re.M)]
        assert defs == ["cnn_plan.h"], (fn, defs)
    # the comma-list macros are gone, and no build of the library overrides the tile configurations from the command line
    build_py = open(os.path.join(ROOT, "cough_detector_amd", "build.py")).read()
    assert not [f for f, text in src.items() if "CNN_X3_CFG" in text] and "CNN_X3" not in build_py


def test_matrix_reaches_every_path_of_the_dispatch():
    rows = [(dt, R.plan(R.case_dims(c), dt, c.H, c.W)) for c in R.CASES for dt in R.case_dtypes(c)]
    assert all(steps is not None and all(s.kernel != "unsupported" for s in steps) for _, steps in rows)
    assert R.REQUIRED <= R.coverage(rows), R.REQUIRED - R.coverage(rows)
    assert all(c.batch <= 8 for c in R.CASES)


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_emulated_operands_stay_within_half_of_the_bound(cnn_golden, case):
    blocks = _blocks(case, cnn_golden)
    x = R.case_image(case, batch=1)
    for dtype in R.case_dtypes(case):
        steps = R.plan(blocks, dtype, case.H, case.W)
        taps = R.emulate(x.float(), blocks, steps, dtype)
        worst = R.check_taps(x.float(), blocks, steps, dtype, lambda d: taps[d])
        top = max(worst, key=lambda w: w.ratio)
        print(f"{case.name} {dtype}: worst emulated / bound {top.ratio:.3f} at depth {top.depth} ({top.kernel})")
        assert top.ratio <= 0.5, top


# ------------------------------------------------------------------------------------------ planted defects
def _logits(kind, sd, act):
    fc1, fc2 = ("fc.0", "fc.3") if kind == "standard" else ("classifier.1", "classifier.4")
    return R.head_ref(act, sd[fc1 + ".weight"], sd[fc1 + ".bias"], sd[fc2 + ".weight"], sd[fc2 + ".bias"])[0]


def _planted(cnn_golden, kind, H, depth, defect):
    """Run the bf16x3 emulation of ``kind`` on golden images cropped / padded to H rows with ``defect(x_in, clean_out,
    block, step) -> out`` replacing block ``depth``'s output.  -> (worst ratio at that depth, logit shift)."""
    sd, _ = cnn_golden[kind]
    blocks = R.BLOCKS[kind](sd)
    x = cnn_golden["x"][:4]
    if H > x.shape[2]:
        x = torch.cat([x, x[:, :, :H - x.shape[2]]], dim=2)
    x = x[:, :, :H].contiguous()
    steps = R.plan(blocks, "bf16x3", H, x.shape[3])
    clean = R.emulate(x, blocks, steps, "bf16x3")
    assert max(w.ratio for w in R.check_taps(x, blocks, steps, "bf16x3", lambda d: clean[d])) <= 0.5
    bad = list(clean)
    bad[depth] = defect(x.double() if depth == 0 else clean[depth - 1], clean[depth], blocks[depth], steps[depth])
    for d in range(depth + 1, len(blocks)):
        bad[d] = R.emulate_layer(bad[d - 1], blocks[d], *R.step_scheme(steps[d], "bf16x3"))
    worst = R.check_taps(x, blocks, steps, "bf16x3", lambda d: bad[d])
    at = [w for w in worst if w.depth == max(depth, 1)][0]     # block 0 is seen through block 1's tap
    shift = float((_logits(kind, sd, bad[-1]) - _logits(kind, sd, clean[-1])).abs().max())
    return at, shift, steps[depth]


def _halo_row_zeroed(band):
    def defect(x_in, clean_out, block, step):
        o0, rows = band * step.band_rows, step.band_rows
        halo = 2 * (o0 + rows)                       # the input row below the band's last conv row
        assert step.n_bands > band + 1 and halo < x_in.shape[2]
        x2 = x_in.clone()
        x2[:, :, halo] = 0
        out = clean_out.clone()
        out[:, :, o0:o0 + rows] = R.emulate_layer(x2, block, "bf16x3")[:, :, o0:o0 + rows]
        return out
    return defect


def _odd_last_row_as_padding(x_in, clean_out, block, step):
    assert x_in.shape[2] % 2 == 1                    # floor pooling: the last conv row reads it, nothing is centred on it
    x2 = x_in.clone()
    x2[:, :, -1] = 0
    return R.emulate_layer(x2, block, "bf16x3")


def _tile_tail_one_pixel_late(band, tile):
    def defect(x_in, clean_out, block, step):
        n, c, oh, ow = clean_out.shape
        first = band * step.band_rows * ow + tile * 8          # a 32-row tile of a pooled layer = 8 output pixels
        flat = clean_out.clone().reshape(n, c, oh * ow)
        src = clean_out.reshape(n, c, oh * ow)
        assert first + 9 <= oh * ow
        flat[:, :, first + 6:first + 9] = src[:, :, first + 5:first + 8]
        return flat.reshape(n, c, oh, ow)
    return defect


def _lo_hi_dropped(x_in, clean_out, block, step):
    return R.emulate_layer(x_in, block, "bf16x3", drop_lo_hi=True)


@pytest.mark.parametrize("name,kind,H,depth,defect", [
    ("last halo row of a band zeroed", "standard", 90, 1, _halo_row_zeroed(2)),
    ("odd last input row treated as padding", "standard", 90, 1, _odd_last_row_as_padding),
    ("one tile's tail written one pixel late", "standard", 90, 2, _tile_tail_one_pixel_late(1, 3)),
    ("lo*hi term dropped in one layer", "small", 90, 1, _lo_hi_dropped),
])
def test_planted_defect_is_flagged_per_pixel(cnn_golden, name, kind, H, depth, defect):
    at, shift, step = _planted(cnn_golden, kind, H, depth, defect)
    print(f"{name}: per-pixel ratio {at.ratio:.3g} at depth {at.depth} row {at.row} col {at.col} (band row {at.band_row}); "
          f"logit shift at the trained-scale head {shift:.2e}")
    assert step.kernel in ("lds_x3", "first_x3")
    assert at.ratio > 1.0


QUIET_ROW = 0.005     # the odd last row of the image at 0.5 % of a mel row's level: a band with next to no energy in it


@pytest.mark.parametrize("name,kind,H,depth,defect,last_row_scale", [
    ("one tile's tail written one pixel late", "small", 90, 0, _tile_tail_one_pixel_late(0, 3), 1.0),
    ("odd last input row treated as padding", "standard", 91, 0, _odd_last_row_as_padding, QUIET_ROW),
])
def test_geometric_defect_passes_the_logit_tolerance(cnn_golden, name, kind, H, depth, defect, last_row_scale):
    """The per-pixel check flags the defect AND the logits of the reference-generated, trained-scale goldens move by
    less than LOGIT_TOL, i.e. the assertions on logits alone pass with it.

    How far that goes, measured on the CPU emulation (ratio = |err| / bound at the worst pixel, shift = max |logit
    change| over 4 golden clips):

        tile tail one pixel late   Small, first block, tile 3            ratio 28     shift 5.3e-4   asserted here
                                   Standard, first block, tile 3         ratio 48     shift 3.8e-3
                                   Standard, block 2, band 1 tile 3      ratio 56     shift 1.6e-2
        odd last row as padding    Standard 91 rows, quiet last row      ratio 4.3    shift 3.9e-4   asserted here
                                   Standard 91 rows, last row = a mel row ratio 669   shift 2.0e-1
                                   Standard 90 rows, block 1             ratio 1422   shift 2.6e-1
        halo row of a band zeroed  Standard 90 rows, block 1 band 0      ratio 926    shift 3.0e-1
                                   Small 90 rows, block 1 band 0         ratio 1378   shift 6.1e-1

    A defect of a few pixels, or of a row that carries little energy, hides under the logit tolerance while the per-pixel
    ratio is well over 1.  One that costs a whole row of a map at full level moves the logits of these heads by 0.03 to 0.6
    (the head calibrated to a class-margin spread of 2.5 amplifies the feature error): the logit assertions see that one,
    but only at the image sizes they run, 90 x 101 and 64 x 47.  A zeroed halo row inside an activation map cannot be made
    quiet through the image (the folded BatchNorm bias keeps the row at O(1)), so it is asserted per pixel only."""
    golden = dict(cnn_golden)
    if last_row_scale != 1.0:
        x = cnn_golden["x"]
        x = torch.cat([x, x[:, :, :H - x.shape[2]]], dim=2).clone()
        x[:, :, -1] *= last_row_scale
        golden["x"] = x
    at, shift, _ = _planted(golden, kind, H, depth, defect)
    print(f"{name}: ratio {at.ratio:.3g}, logit shift {shift:.2e}")
    assert at.ratio > 1.0 and shift < LOGIT_TOL
