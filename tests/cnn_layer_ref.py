"""Float64 restatement of the conv-stack classifiers layer by layer, a Python restatement of the kernel dispatch of
``csrc/cnn_plan.h`` (``plan``), the per-pixel error budget of each kernel family (``layer_bound``), a CPU emulation of the
three operand schemes with plantable defects (``emulate_layer``) and the shape matrix the host and GPU tests share.

Blocks
------
A ``Block`` is what one ``cough_cnn_block`` carries: a dense 3x3 conv (``w`` (N, C, 3, 3)) or a depthwise 3x3
(``dw_w`` (C, 1, 3, 3), ``dw_b``) followed by a pointwise 1x1 (``w`` (N, C, 1, 1)), eval-mode BatchNorm, ReLU and an
optional 2x2 floor max-pool.  ``features`` runs them as ``oracle/cnn.py`` does (conv, ``F.batch_norm``, ReLU, pool) in
float64 and returns every block's output; ``tests/test_cnn_layer_ref_host.py`` pins it to ``oracle.cnn`` at 1e-12.

Dispatch (``plan``)
-------------------
A restatement, written independently, of ``plan_cnn`` in ``csrc/cnn_plan.h``, the one place the library decides what a
forward launches (``csrc/cnn.hip`` executes that plan).  The constants below (``X3_CFG``, ``FIRST_MAXL``, ``LDS_UNP``)
mirror ``CNN_X3_TABLE``, ``CNN_FIRST_MAXL`` and ``CNN_LDS_UNP``.  ``tests/test_cnn_layer_ref_host.py`` compiles the header
into ``tests/cnn_plan_dump.cpp`` and holds its constants, its capability record and its plans equal to this module's,
field by field (``plan_line``) over the matrix and a sweep of shapes, so a retune fails there; the GPU tests then assert
that every shape of the matrix lands on the path it was chosen for according to ``plan`` and the hand-written ``EXPECT``
rows, instead of the coverage moving silently.

Error budget (``layer_bound``)
------------------------------
u = 2^-24 is the unit roundoff of float32.  The library folds BatchNorm into the convolution in double
(``cough_cnn_create``): W = conv weight * gamma / sqrt(var + eps), b = (bias - mean) * gamma / sqrt(var + eps) + beta, a
depthwise / pointwise pair composed into the dense 3x3 it equals.  With x the layer's input exactly as the kernel
received it, K = 9 cin products per output and

    A = |W| * |x| + |b|                    (a float64 convolution with the absolute folded weights)

the budget of one conv output before ReLU is, per kernel family:

* f32 (``cnn_first_kernel``, ``cnn_conv_kernel<float>``): ``(K + C_F32) u A`` with C_F32 = 4.  A dot product of K terms
  in ANY summation order, fused or not, carries at most K roundings on any one term (its product and at most K - 1
  partial sums, none of which exceeds sum |w x|): K u A.  One more u for the float32 rounding of the folded weight, one
  for the float32 bias, one for the bias add: K + 3.  The fourth covers the second-order terms,
  (1 + u)^(K + 3) - 1 <= (K + 3) u (1 + 1e-4) for K <= 2304.
* split-bf16 (``cnn_first_x3_kernel``, ``cnn_conv_lds_x3_kernel``): an operand is held as hi + lo, hi = bf16(v),
  lo = bf16(v - hi).  bf16 has 8 significant bits, so |v - hi| <= 2^-9 |v| and |v - hi - lo| <= 2^-9 |v - hi| <= 2^-18 |v|:
  a 2^-18 relative representation error on each of x and w, and the dropped lo*lo product is at most
  (2^-9)^2 |x| |w| = 2^-18 |x| |w|: ``3 * 2^-18`` per product.  The three partial products hi*hi, lo*hi, hi*lo that ARE
  formed are exact in float32 (8 x 8 bits) and are accumulated in float32, 3 K terms whose absolute sum is at most
  (1 + 2^-8) sum |w x|: ``(3 K + C_F32) u (1 + 2^-7)``, the last factor also covering the cross terms of the first
  part.  Zero-weight k-slots (the 16-wide step of the first block holds 9 taps) add exact zeros.
* single bf16 (``cnn_conv_lds_kernel``, ``conv_gemm_bf16_kernel``, ``cnn_conv_kernel<bf16>``): ``2^-8`` on each operand
  (twice the unit roundoff of bf16: the folded weight is rounded to float32 first, then to bf16) and their product
  2^-16, then float32 accumulation of K exact products: ``2 * 2^-8 + 2^-16 + (K + C_F32) u``.  The first block of this
  mode computes in f32 (``cnn_first_kernel<bf16_t>``).  Every layer of this mode STORES bf16: ``2^-8 (|y| + e)`` is added
  after the pool, y the reference output.

ReLU and max are 1-Lipschitz, so the bound of a pooled output is the max of the bounds of its window's four conv
outputs and no kink needs handling.  An input that is itself only known to within E (depth 1: the first block's output
cannot be tapped, networks have at least two blocks) adds ``|W| * E`` before the pool.

Head (``head_bound``): the mean over HW non-negative activations in any order carries (HW + 2) u (HW - 1 adds, the
division, one spare); a GEMV of n terms plus bias (n + 2) u on sum |w v| + |b|; ReLU is 1-Lipschitz.  The second GEMV
is summed over 64 lanes and a 6-step wave reduction: any order, (HID + 2) u again.
"""
from __future__ import annotations

from collections import namedtuple
from typing import List, Optional

import torch
import torch.nn.functional as F

import emulate_precision as emu

EPS = 1e-5
U = 2.0 ** -24
C_F32 = 4
E_BF16 = 2.0 ** -8
E_SPLIT = 2.0 ** -18

Block = namedtuple("Block", "w b bn_w bn_b bn_mean bn_var dw_w dw_b pool")


# ------------------------------------------------------------------------------------------ blocks
def standard_blocks(sd) -> List[Block]:
    out, i = [], 0
    while f"conv_layers.{i}.conv.weight" in sd:
        p = f"conv_layers.{i}"
        out.append(Block(sd[p + ".conv.weight"], sd[p + ".conv.bias"], sd[p + ".bn.weight"], sd[p + ".bn.bias"],
                         sd[p + ".bn.running_mean"], sd[p + ".bn.running_var"], None, None, 2))
        i += 1
    return out


def small_blocks(sd) -> List[Block]:
    f = "features."
    out = []
    for conv, bn, dw, pool in ((0, 1, None, 2), (5, 6, 4, 2), (10, 11, 9, 2), (15, 16, 14, 1)):
        out.append(Block(sd[f"{f}{conv}.weight"], sd[f"{f}{conv}.bias"], sd[f"{f}{bn}.weight"], sd[f"{f}{bn}.bias"],
                         sd[f"{f}{bn}.running_mean"], sd[f"{f}{bn}.running_var"],
                         None if dw is None else sd[f"{f}{dw}.weight"], None if dw is None else sd[f"{f}{dw}.bias"], pool))
    return out


BLOCKS = {"standard": standard_blocks, "small": small_blocks}


def random_blocks(spec, seed: int) -> List[Block]:
    """Seeded blocks for ``spec`` = [(cin, cout, pool, separable)]: torch's default conv init, BatchNorm with
    non-trivial statistics (mean ~ N(0, 0.3), var ~ U(0.5, 1.5), weight ~ U(0.5, 1.5), bias ~ N(0, 0.1))."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for cin, cout, pool, sep in spec:
        def uni(shape, fan_in):
            k = 1.0 / fan_in ** 0.5
            return (torch.rand(shape, generator=g) * 2 - 1) * k
        if sep:
            dw_w, dw_b = uni((cin, 1, 3, 3), 9), uni((cin,), 9)
            w, b = uni((cout, cin, 1, 1), cin), uni((cout,), cin)
        else:
            dw_w = dw_b = None
            w, b = uni((cout, cin, 3, 3), 9 * cin), uni((cout,), 9 * cin)
        out.append(Block(w, b, torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1,
                         torch.randn(cout, generator=g) * 0.3, torch.rand(cout, generator=g) + 0.5, dw_w, dw_b, pool))
    return out


def layer_dims(blocks):
    """[(cin, cout, pool)] as ``cough_cnn_create`` sees the blocks."""
    return [(int(b.w.shape[1]) if b.dw_w is None else int(b.dw_w.shape[0]), int(b.w.shape[0]), int(b.pool)) for b in blocks]


def layer(x: torch.Tensor, b: Block) -> torch.Tensor:
    """One block in float64, written as ``oracle/cnn.py`` writes it."""
    x = x.double()
    if b.dw_w is not None:
        x = F.conv2d(x, b.dw_w.double(), b.dw_b.double(), padding=1, groups=b.dw_w.shape[0])
        x = F.conv2d(x, b.w.double(), b.b.double())
    else:
        x = F.conv2d(x, b.w.double(), b.b.double(), padding=1)
    x = F.relu(F.batch_norm(x, b.bn_mean.double(), b.bn_var.double(), b.bn_w.double(), b.bn_b.double(), training=False,
                            eps=EPS))
    return F.max_pool2d(x, 2) if b.pool == 2 else x


def features(x: torch.Tensor, blocks) -> List[torch.Tensor]:
    out = []
    for b in blocks:
        x = layer(x, b)
        out.append(x)
    return out


def fold(b: Block):
    """(W (N, C, 3, 3), bias (N,)) in float64, as ``cough_cnn_create`` folds them (before any rounding)."""
    w = b.w.double()
    bias = b.b.double()
    if b.dw_w is not None:
        pw = w[:, :, 0, 0]
        bias = bias + pw @ b.dw_b.double()
        w = pw[:, :, None, None] * b.dw_w.double()[:, 0][None]
    s = b.bn_w.double() / torch.sqrt(b.bn_var.double() + EPS)
    return w * s[:, None, None, None], (bias - b.bn_mean.double()) * s + b.bn_b.double()


# ------------------------------------------------------------------------------------------ dispatch
X3_CFG = {16: (1, 4, 4, 1, 6144), 32: (2, 5, 2, 2, 3328), 64: (4, 3, 2, 2, 5056), 128: (4, 2, 2, 4, 6144)}  # nt mw wm wn pieces
FIRST_MAXL = 22
LDS_UNP = 12
DTYPES = ("fp32", "bf16x3", "bf16_approx")

Step = namedtuple("Step", "kernel cin cout pool nt band_rows n_bands fused_mean odd_hw in_hw out_hw lds")
MODES = ("forward", "conv_output")


def shapes(dims, H, W):
    out, h, w = [], H, W
    for _, cout, pool in dims:
        if pool == 2:
            h, w = h // 2, w // 2
        if h < 1 or w < 1:
            return None
        out.append((h, w, cout))
    return out


def x3_band(cin, cout, pool, out_h, out_w, in_w) -> int:
    nt = 4 if cout >= 128 else cout // 32
    cfg = X3_CFG.get(cin)
    if cfg is None or cfg[0] != nt:
        return 0
    _, mw, wm, _, pieces = cfg
    band = min((wm * mw * 32) // ((4 if pool == 2 else 1) * out_w), out_h)
    while band >= 1 and ((2 if pool == 2 else 1) * band + 2) * (in_w + 2) * (cin // 4) > pieces:
        band -= 1
    return band


def plan(blocks_or_dims, dtype: str, H: int, W: int, mode: str = "forward") -> Optional[List[Step]]:
    """The kernel every layer of ``cough_cnn_forward`` (``mode`` "conv_output": of ``cough_cnn_conv_output``, which taps the
    last layer and wants no logits) launches for an (H, W) image, or None if the image vanishes.
    kernel: first | first_x3 | conv_f32 | lds_x3 | lds_bf16 | gemm_bf16 | conv_bf16 | unsupported (the launch is refused).
    lds: the dynamic LDS bytes of the launch."""
    assert dtype in DTYPES and mode in MODES
    dims = blocks_or_dims if isinstance(blocks_or_dims[0][0], int) else layer_dims(blocks_or_dims)
    shp = shapes(dims, H, W)
    if shp is None:
        return None
    out, ch, cw = [], H, W
    for i, ((cin, cout, pool), (sh, sw, _)) in enumerate(zip(dims, shp)):
        nt = 4 if cout >= 128 else cout // 32
        kernel, band, n_bands, fused, odd, lds = None, 0, 0, False, False, 0
        if i == 0:
            lds2 = 2 * (ch + 3) * ((cw + 7) & ~1) * 2
            if dtype == "bf16x3" and cout <= 32 and pool == 2 and ch * cw <= 2 * 256 * FIRST_MAXL and lds2 <= 64 * 1024:
                kernel, odd, lds = "first_x3", (ch * cw) % 2 == 1, lds2
            else:
                kernel = "first"
        elif dtype == "bf16_approx" and (cin, cout) in ((16, 32), (32, 64), (64, 128)):
            mw = 2 if cin == 64 else 4
            band = min((4 * mw * 32) // ((4 if pool == 2 else 1) * sw), sh)
            lds = ((2 if pool == 2 else 1) * band + 2) * (cw + 2) * cin * 2
            if band >= 1 and lds <= LDS_UNP * 256 * 16:
                kernel, n_bands = "lds_bf16", -(-sh // band)
            else:
                kernel, band, lds = "unsupported", 0, 0
        elif dtype == "bf16_approx":
            kernel = "gemm_bf16" if cin % 32 == 0 and cout % 64 == 0 else "conv_bf16"
        else:
            has_frag = dtype == "bf16x3" and cin in X3_CFG and (cout in (32, 64) or cout % 128 == 0)
            band = x3_band(cin, cout, pool, sh, sw, cw) if has_frag else 0
            if band >= 1:
                kernel, n_bands = "lds_x3", -(-sh // band)
                # two images (hi, lo), each rounded up to 16 bytes
                lds = -(-(((2 if pool == 2 else 1) * band + 2) * (cw + 2) * cin * 2) // 16) * 16 * 2
                fused = i + 1 == len(dims) and n_bands == 1 and mode == "forward"
            else:
                kernel = "conv_f32"
        out.append(Step(kernel, cin, cout, pool, nt, band, n_bands, fused, odd, (ch, cw), (sh, sw), lds))
        ch, cw = sh, sw
    return out


def plan_line(dims, dtype: str, H: int, W: int, mode: str = "forward") -> str:
    """The line tests/cnn_plan_dump.cpp prints for a query, built from ``plan`` and the launch arithmetic of csrc/cnn.hip:
    the grid (x per clip: workgroups of the one-workgroup-per-clip / per-band kernels, threads of the first block, GEMM
    rows of the rest; y: channel groups), one ping-pong buffer for 1 and for 3 clips, the tail kernel's HW."""
    steps = plan(dims, dtype, H, W, mode)
    if steps is None:
        return "none"
    parts = []
    for i, s in enumerate(steps):
        oh, ow = s.out_hw
        if s.kernel == "first":
            gx, gy = oh * ow, 1
        elif s.kernel == "first_x3":
            gx, gy = 1, 1
        elif s.kernel in ("lds_bf16", "unsupported"):
            gx, gy = s.n_bands, 1
        elif s.kernel == "lds_x3":
            gx, gy = s.n_bands, s.cout // (32 * s.nt)
        else:
            gx, gy = oh * ow * (4 if s.pool == 2 else 1), s.cout // (32 * s.nt)
        parts.append(f"{s.kernel} {s.nt if i else 0} {s.band_rows} {s.n_bands} lds={s.lds} grid={gx},{gy} {int(s.fused_mean)} "
                     f"{int(s.odd_hw)} {s.in_hw[0]}x{s.in_hw[1]}->{oh}x{ow}")
    act = max(s.out_hw[0] * s.out_hw[1] * s.cout for s in steps) * (2 if dtype == "bf16_approx" else 4)
    hw = 1 if steps[-1].fused_mean else steps[-1].out_hw[0] * steps[-1].out_hw[1]
    parts.append(f"buf={-(-act // 256) * 256},{-(-3 * act // 256) * 256} head_hw={hw}")
    bad = [i for i, s in enumerate(steps) if s.kernel == "unsupported"]
    if bad:
        parts.append(f"unsupported={bad[0]} {steps[bad[0]].in_hw[0]}x{steps[bad[0]].in_hw[1]}")
    return " | ".join(parts)


SCHEME = {"first": "f32", "conv_f32": "f32", "first_x3": "bf16x3", "lds_x3": "bf16x3", "lds_bf16": "bf16", "gemm_bf16": "bf16",
          "conv_bf16": "bf16"}


def step_scheme(step: Step, dtype: str):
    """(operand scheme, stores bf16) of a planned layer."""
    return SCHEME[step.kernel], dtype == "bf16_approx"


# ------------------------------------------------------------------------------------------ bounds
def _pool_max(e, pool):
    return F.max_pool2d(e, 2) if pool == 2 else e


def layer_bound(x: torch.Tensor, b: Block, scheme: str, stores_bf16: bool = False, e_in: Optional[torch.Tensor] = None,
                y_ref: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-element absolute bound of one block's output against ``layer(x, b)``; see the module docstring."""
    w, bias = fold(b)
    k = 9 * w.shape[1]
    a = F.conv2d(x.double().abs(), w.abs(), bias.abs(), padding=1)
    if scheme == "f32":
        rel = (k + C_F32) * U
    elif scheme == "bf16x3":
        rel = (3 * E_SPLIT + (3 * k + C_F32) * U) * (1 + 2.0 ** -7)
    elif scheme == "bf16":
        rel = 2 * E_BF16 + E_BF16 ** 2 + (k + C_F32) * U
    else:
        raise ValueError(scheme)
    e = rel * a
    if e_in is not None:
        e = e + F.conv2d(e_in.double(), w.abs(), padding=1)
    e = _pool_max(e, b.pool)
    if stores_bf16:
        y = layer(x, b) if y_ref is None else y_ref
        e = e + E_BF16 * (y.abs() + e)
    return e


def head_ref(act: torch.Tensor, w1, b1, w2, b2):
    """(logits, bound) of mean -> Linear -> ReLU -> Linear in float64 over the activation the kernels themselves
    produced, and the float32 budget of that head."""
    act, w1, b1, w2, b2 = (t.double() for t in (act, w1, b1, w2, b2))
    hw = act.shape[2] * act.shape[3]
    v = act.mean(dim=(2, 3))
    e_v = (hw + 2) * U * act.abs().mean(dim=(2, 3))
    pre = v @ w1.t() + b1
    e_h = e_v @ w1.abs().t() + (w1.shape[1] + 2) * U * (v.abs() @ w1.abs().t() + b1.abs())
    h = F.relu(pre)
    logits = h @ w2.t() + b2
    e_l = e_h @ w2.abs().t() + (w2.shape[1] + 2) * U * (h @ w2.abs().t() + b2.abs())
    return logits, e_l


# ------------------------------------------------------------------------------------------ emulation
def emulate_layer(x: torch.Tensor, b: Block, scheme: str, stores_bf16: bool = False, drop_lo_hi: bool = False) -> torch.Tensor:
    """One block under an operand scheme on the CPU (float64 tensors holding the rounded values): ``f32`` is a true float32
    ``F.conv2d`` over the float32 folded weights; ``bf16x3`` / ``bf16`` are ``emulate_precision._conv`` over them.
    ``drop_lo_hi``: planted defect, the lo*hi MFMA of the split scheme is missing."""
    w, bias = fold(b)
    w, bias = w.float(), bias.float()
    if scheme == "f32":
        y = F.conv2d(x.float(), w, padding=1).double()
    elif drop_lo_hi:
        xh, _ = emu.split(x.double())
        wh, wl = emu.split(w.double())
        y = F.conv2d(xh, wh, padding=1) + F.conv2d(xh, wl, padding=1)
    else:
        y = emu._conv(x.double(), w.double(), scheme, padding=1)
    y = (y.float() + bias[None, :, None, None]).double()
    y = _pool_max(F.relu(y), b.pool)
    return emu._store(y, "bf16") if stores_bf16 else y


def emulate(x: torch.Tensor, blocks, steps, dtype: str) -> List[torch.Tensor]:
    out = []
    x = x.double()
    for b, st in zip(blocks, steps):
        x = emulate_layer(x, b, *step_scheme(st, dtype))
        out.append(x)
    return out


# ------------------------------------------------------------------------------------------ the per-pixel check
Worst = namedtuple("Worst", "ratio depth kernel clip channel row col band_row err bound")


def check_taps(x: torch.Tensor, blocks, steps, dtype: str, tap) -> List[Worst]:
    """The per-pixel check both test files run.  ``tap(d)`` is the device's (or the emulation's) output of block d,
    d = 1 .. len(blocks) - 1 (a network has at least two blocks, so block 0 is never the end of one).  Depth 1 is
    compared with the reference of the image, the first block's bound propagated; depth d >= 2 with the reference of
    ``tap(d - 1)`` itself.  Returns the worst |err| / bound per depth with its coordinates."""
    x = x.double()
    out = []
    sch0, st0 = step_scheme(steps[0], dtype)
    y0 = layer(x, blocks[0])
    e0 = layer_bound(x, blocks[0], sch0, st0, y_ref=y0)
    prev = None
    for d in range(1, len(blocks)):
        sch, sto = step_scheme(steps[d], dtype)
        if d == 1:
            ref = layer(y0, blocks[1])
            bound = layer_bound(y0, blocks[1], sch, sto, e_in=e0, y_ref=ref)
        else:
            ref = layer(prev, blocks[d])
            bound = layer_bound(prev, blocks[d], sch, sto, y_ref=ref)
        got = tap(d).double().cpu()
        assert got.shape == ref.shape, (d, got.shape, ref.shape)
        assert torch.isfinite(got).all(), f"depth {d}: non-finite output"
        err = (got - ref).abs()
        ratio = err / bound.clamp(min=1e-300)
        ratio = torch.where((err == 0) & (bound == 0), torch.zeros_like(ratio), ratio)
        i = int(ratio.argmax())
        n, c, r, col = (int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape))
        band_row = r % steps[d].band_rows if steps[d].band_rows else -1
        out.append(Worst(float(ratio.flatten()[i]), d, steps[d].kernel, n, c, r, col, band_row, float(err.flatten()[i]),
                         float(bound.flatten()[i])))
        prev = got
    return out


# ------------------------------------------------------------------------------------------ the matrix
STD_DIMS = [(1, 32, 2), (32, 64, 2), (64, 128, 2), (128, 256, 2)]
SMALL_DIMS = [(1, 16, 2), (16, 32, 2), (32, 64, 2), (64, 128, 1)]

# generic stacks: [(cin, cout, pool, separable)]
GENERIC = {
    # every POOL = false instantiation of the split-bf16 kernel (cin 16, 32, 64, 128), the last one 128 -> 128
    "nopool": [(1, 16, 2, False), (16, 32, 1, False), (32, 64, 1, True), (64, 128, 1, False), (128, 128, 1, False)],
    # 8-wide first block; layers without a split-bf16 tile shape (8 -> 32, 32 -> 32, 64 -> 64) between ones that have one;
    # 128 -> 256 without a pool: grid.y = 2
    "mixed": [(1, 8, 2, False), (8, 32, 2, False), (32, 32, 1, False), (32, 64, 2, True), (64, 64, 1, False),
              (64, 128, 2, False), (128, 256, 1, False)],
    "first24": [(1, 24, 2, False), (24, 32, 1, False), (32, 64, 2, False)],
    # first block wider than one 32-channel tile and without a pool: cnn_first_kernel<T, false> in every mode
    "first64": [(1, 64, 1, False), (64, 64, 2, False), (64, 128, 2, True)],
    # the single-bf16 mode's three kernels in one network (16 -> 32, 32 -> 64, 64 -> 128 LDS image; 32 -> 32 direct;
    # 128 -> 128 LDS-staged GEMM)
    "approx": [(1, 16, 2, False), (16, 32, 2, False), (32, 32, 1, False), (32, 64, 2, True), (64, 128, 1, False),
               (128, 128, 2, False)],
}

Case = namedtuple("Case", "name net H W batch approx")
# net: "standard" | "small" | a GENERIC key.  approx: also run under bf16_approx (the rows marked with a dagger).
CASES = [
    Case("std_90x101", "standard", 90, 101, 3, True), Case("small_90x101", "small", 90, 101, 3, True),
    Case("std_110x101", "standard", 110, 101, 3, False), Case("std_111x101", "standard", 111, 101, 3, False),
    Case("small_110x101", "small", 110, 101, 3, False),
    Case("std_91x101", "standard", 91, 101, 3, True), Case("small_91x101", "small", 91, 101, 3, True),
    Case("std_89x99", "standard", 89, 99, 3, True), Case("small_89x99", "small", 89, 99, 3, True),
    Case("std_33x35", "standard", 33, 35, 3, True), Case("small_33x35", "small", 33, 35, 3, True),
    Case("std_17x17", "standard", 17, 17, 5, True), Case("small_17x17", "small", 17, 17, 5, True),
    Case("std_16x16", "standard", 16, 16, 3, False), Case("small_8x8", "small", 8, 8, 3, False),
    Case("std_128x128", "standard", 128, 128, 2, False), Case("small_128x128", "small", 128, 128, 2, False),
    Case("std_40x300", "standard", 40, 300, 2, False), Case("std_64x400", "standard", 64, 400, 2, False),
    Case("small_64x400", "small", 64, 400, 2, False),
    Case("std_300x40", "standard", 300, 40, 2, False), Case("small_9x200", "small", 9, 200, 3, False),
    Case("nopool_26x22", "nopool", 26, 22, 3, False), Case("mixed_72x88", "mixed", 72, 88, 3, False),
    Case("first24_31x37", "first24", 31, 37, 3, False), Case("first64_20x28", "first64", 20, 28, 3, False),
    Case("approx_48x56", "approx", 48, 56, 3, True),
]


# hand-checked (kernel, band_rows, n_bands, fused mean) of the cases that exist for one path of the dispatch
T_, F_ = True, False
EXPECT = {
    ("std_90x101", "bf16x3"): [("first_x3", 0, 0, F_), ("lds_x3", 3, 8, F_), ("lds_x3", 4, 3, F_), ("lds_x3", 5, 1, T_)],
    ("small_90x101", "bf16x3"): [("first_x3", 0, 0, F_), ("lds_x3", 5, 5, F_), ("lds_x3", 6, 2, F_), ("lds_x3", 11, 1, T_)],
    ("std_110x101", "bf16x3"): [("first_x3", 0, 0, F_), ("lds_x3", 3, 9, F_), ("lds_x3", 4, 4, F_), ("lds_x3", 5, 2, F_)],
    ("std_111x101", "bf16x3"): [("first_x3", 0, 0, F_), ("lds_x3", 3, 9, F_), ("lds_x3", 4, 4, F_), ("lds_x3", 5, 2, F_)],
    ("std_16x16", "bf16x3"): [("first_x3", 0, 0, F_), ("lds_x3", 4, 1, F_), ("lds_x3", 2, 1, F_), ("lds_x3", 1, 1, T_)],
    ("small_8x8", "bf16x3"): [("first_x3", 0, 0, F_), ("lds_x3", 2, 1, F_), ("lds_x3", 1, 1, F_), ("lds_x3", 1, 1, T_)],
    ("std_128x128", "bf16x3"): [("first", 0, 0, F_), ("lds_x3", 2, 16, F_), ("lds_x3", 3, 6, F_), ("lds_x3", 4, 2, F_)],
    ("small_128x128", "bf16x3"): [("first", 0, 0, F_), ("lds_x3", 4, 8, F_), ("lds_x3", 5, 4, F_), ("lds_x3", 12, 2, F_)],
    ("std_40x300", "bf16x3"): [("first", 0, 0, F_), ("conv_f32", 0, 0, F_), ("lds_x3", 1, 5, F_), ("lds_x3", 1, 2, F_)],
    ("std_64x400", "bf16x3"): [("first", 0, 0, F_)] + [("conv_f32", 0, 0, F_)] * 3,
    ("small_64x400", "bf16x3"): [("first", 0, 0, F_), ("lds_x3", 1, 16, F_), ("lds_x3", 1, 8, F_), ("lds_x3", 3, 3, F_)],
    ("std_300x40", "bf16x3"): [("first", 0, 0, F_), ("lds_x3", 8, 10, F_), ("lds_x3", 9, 5, F_), ("lds_x3", 12, 2, F_)],
    ("small_9x200", "bf16x3"): [("first_x3", 0, 0, F_), ("lds_x3", 2, 1, F_), ("lds_x3", 1, 1, F_), ("lds_x3", 1, 1, T_)],
    ("nopool_26x22", "bf16x3"): [("first_x3", 0, 0, F_), ("lds_x3", 13, 1, F_), ("lds_x3", 13, 1, F_), ("lds_x3", 13, 1, F_),
                                 ("lds_x3", 11, 2, F_)],
    ("mixed_72x88", "bf16x3"): [("first_x3", 0, 0, F_), ("conv_f32", 0, 0, F_), ("conv_f32", 0, 0, F_), ("lds_x3", 7, 2, F_),
                                ("conv_f32", 0, 0, F_), ("lds_x3", 4, 1, F_), ("lds_x3", 4, 1, T_)],
    ("first24_31x37", "bf16x3"): [("first_x3", 0, 0, F_), ("conv_f32", 0, 0, F_), ("lds_x3", 7, 1, T_)],
    ("first64_20x28", "bf16x3"): [("first", 0, 0, F_), ("conv_f32", 0, 0, F_), ("lds_x3", 5, 1, T_)],
    ("std_90x101", "bf16_approx"): [("first", 0, 0, F_), ("lds_bf16", 5, 5, F_), ("lds_bf16", 5, 3, F_), ("gemm_bf16", 0, 0, F_)],
    ("approx_48x56", "bf16_approx"): [("first", 0, 0, F_), ("lds_bf16", 9, 2, F_), ("conv_bf16", 0, 0, F_), ("lds_bf16", 6, 1, F_),
                                      ("lds_bf16", 6, 1, F_), ("gemm_bf16", 0, 0, F_)],
}


def case_dtypes(case: Case):
    return DTYPES if case.approx else DTYPES[:2]


def case_dims(case: Case):
    if case.net == "standard":
        return STD_DIMS
    if case.net == "small":
        return SMALL_DIMS
    return [(a, b, p) for a, b, p, _ in GENERIC[case.net]]


def case_image(case: Case, batch: Optional[int] = None) -> torch.Tensor:
    """Seeded images in the feature range of the shipped front end (mel rows in [0, 1], z-scored rows O(1))."""
    g = torch.Generator().manual_seed(1000 + case.H * 7 + case.W)
    n = case.batch if batch is None else batch
    x = torch.rand((n, 1, case.H, case.W), generator=g)
    x[:, :, case.H // 2:] = torch.randn((n, 1, case.H - case.H // 2, case.W), generator=g)
    return x


# What the matrix has to reach (asserted through ``plan`` in both test files): every path of the dispatch.
def coverage(rows):
    """rows: iterable of (dtype, [Step]).  -> set of coverage keys."""
    seen = set()
    for dtype, steps in rows:
        for st in steps:
            key = st.kernel
            if st.kernel == "first_x3":
                key += ":odd" if st.odd_hw else ":even"
            elif st.kernel == "lds_x3":
                key += f":{st.cin}:{'pool' if st.pool == 2 else 'nopool'}"
                seen.add("bands:" + ("1" if st.n_bands == 1 else "2" if st.n_bands == 2 else ">2"))
                if st.band_rows == 1:
                    seen.add("band_rows:1")
            elif st.kernel == "conv_f32":
                key += f":nt{st.nt}"
                if dtype == "bf16x3" and st.cin in X3_CFG and (st.cout in (32, 64) or st.cout % 128 == 0) and \
                        X3_CFG[st.cin][0] == st.nt:
                    seen.add("x3_band:0")
            seen.add(key)
        if dtype == "bf16x3":
            seen.add("head:fused" if steps[-1].fused_mean else "head:tail")
    return seen


REQUIRED = ({"first", "first_x3:even", "first_x3:odd", "conv_f32:nt1", "conv_f32:nt2", "conv_f32:nt4", "lds_bf16", "gemm_bf16",
             "conv_bf16", "head:fused", "head:tail", "bands:1", "bands:2", "bands:>2", "band_rows:1", "x3_band:0"} |
            {f"lds_x3:{c}:{p}" for c in (16, 32, 64, 128) for p in ("pool", "nopool")})
