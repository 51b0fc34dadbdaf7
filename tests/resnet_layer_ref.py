"""Float64 restatement of ``CoughDetectorResidual`` stage by stage, a Python restatement of the kernel dispatch of
``csrc/resnet_plan.h`` (``plan``), the per-pixel error budget of each kernel family (``stage_bound``), a CPU emulation of the
three operand schemes with plantable defects (``emulate_stage``) and the shape matrix the host and GPU tests share
(``CASES`` with the hand-written ``EXPECT``).  The conv-stack counterpart is ``cnn_layer_ref.py``; the constants U, C_F32,
E_BF16, E_SPLIT and the three bound families are the ones defined there.

Stages
------
``stem_pool`` (conv 7x7 s2 p3 -> BN -> ReLU -> max-pool 2), ``block`` (conv 3x3 s2 -> BN -> ReLU -> conv 3x3 -> BN, plus
the 1x1 s2 projection -> BN, ReLU of the sum) and ``head`` (global mean -> Linear) are written as ``oracle/resnet.py``
writes them, in float64, for any channel tuple; ``tests/test_resnet_layer_ref_host.py`` pins them to
``oracle.resnet.forward(..., return_intermediates=True)`` at 1e-12.

Dispatch (``plan``)
-------------------
Transcribed from ``csrc/resnet_plan.h``: ``make_shapes``, ``stem_lds``, ``rbx_compiled``, ``rbx_t16``,
``rbx_block1_clips``, ``rb_lds_bytes`` / ``rb_mtmax`` / ``rb_fits`` and ``plan_resnet``, which ``resnet.hip`` executes.  The
constants below mirror ``STEM_SB_MAXL``, ``RBX_BLOCK0_ROWS``, ``RBX_BLOCK1_ROWS``, ``RBX_G_TALL``, ``RB_CFG``, ``RB_FIXED`` and
the 64 KB / 160 KB limits.  ``tests/test_resnet_layer_ref_host.py`` builds ``tests/resnet_plan_dump.cpp`` over that header
and holds its constants and its plans of some 227 000 images equal to the ones here, so a retune fails there.

Error budget (``stage_bound``)
------------------------------
u = 2^-24.  The library folds BatchNorm in double and rounds to float32 (``fold`` in resnet.hip):
W = w * gamma / sqrt(var + eps), b = (bias - mean) * gamma / sqrt(var + eps) + beta.  With x the stage's input exactly
as the kernel received it and

    A = |W| * |x| + |b|                    (a float64 convolution with the absolute folded weights)

the budget of one dot product of K terms before ReLU is ``rel(K) * A`` with, per family (derived in cnn_layer_ref):

* f32 (``stem_mfma_kernel``, ``conv_mfma_kernel<float, NT>``):            rel = (K + C) u
* split-bf16 (``stem_bf16_kernel<true>``, ``resblock_x3_kernel``):        rel = (3 * 2^-18 + (3 K + C) u) (1 + 2^-7)
* single bf16 (``stem_bf16_kernel<false>``, ``resblock_bf16_kernel``,
  ``conv_gemm_bf16_kernel``):                                             rel = 2 * 2^-8 + 2^-16 + (K + C) u

(2^-18 is cnn_layer_ref's E_SPLIT, kept as it stands there.  It is the representation error of hi + lo away from the
powers of two; just above one, |v - hi| reaches 2^-8 |v| and |v - hi - lo| 2^-16 |v|.  The float32 accumulation term
beside it is 0.8 times as large at the stem's K = 49 and 4 to 19 times as large in the blocks; the measured ratios of the
split-bf16 stages stay under 0.35 at the stem and under 0.01 in the blocks.)

K = 49 for the stem, 9 cin for conv1 and 9 cout + cin for conv2 plus the projection, which every kernel computes as ONE
dot product (the projection is appended to conv2's K) with ONE bias, float32(b2) + float32(b_skip), summed in float32 at
create time.  C = C_F32 = 4 (weight rounding, bias rounding, bias add, second-order terms) for the stem and conv1; the
summed bias of conv2 carries one more rounding (the float32 add of the two biases), C = C_F32 + 1, and |b| = |b2| +
|b_skip| in A.  Zero k-slots (the stem's 49 taps in a 64-wide K, padded channels of the generic path) add exact zeros.

ReLU and max-pool are 1-Lipschitz: the bound of a pooled stem output is the max of its window's four conv bounds, and no
kink needs handling.

A block in two steps.  h = ReLU(conv1(x)) cannot be tapped, so its bound is carried: with h_ref the float64 h,

    e1 = rel(9 cin) * A1                                 A1 = |W1| * |x| + |b1|
    E  = e1 + s (h_ref + e1)                             s = 0 (f32: h is float32 in HBM), 2^-18 (split: h is kept as
                                                         hi + lo in LDS), 2^-8 (single bf16: h is bf16 in LDS or HBM)
    A2 = |W2| * (h_ref + E) + |Ws| * |x| + |b2| + |bs|   the operand roundings of conv2 act on the h the kernel HAS
    e  = rel(9 cout + cin) * A2 + |W2| * E

Every stage of ``bf16_approx`` STORES bf16: ``2^-8 (|y| + e)`` is added last, y the float64 output.

Head (``head_bound``): the mean over HW non-negative activations in any order carries (HW + 2) u (HW - 1 adds, the
division, one spare) on mean |a|; the GEMV of n channels plus bias (n + 2) u on sum |w v| + |b| (a wave reduction and two
cross-wave adds: any order).

Planted defects (``emulate_stage(..., defect=...)``): see ``DEFECTS``.
"""
from __future__ import annotations

from collections import namedtuple
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

import emulate_precision as emu
from cnn_layer_ref import C_F32, E_BF16, E_SPLIT, U

EPS = 1e-5
DTYPES = ("fp32", "bf16x3", "bf16_approx")
SHIPPED = (32, 64, 128)


# ------------------------------------------------------------------------------------------ float64 stages
def _d(sd, key):
    return sd[key].double()


def _bn(x, sd, p):
    return F.batch_norm(x, _d(sd, p + ".running_mean"), _d(sd, p + ".running_var"), _d(sd, p + ".weight"),
                        _d(sd, p + ".bias"), training=False, eps=EPS)


def stem_pool(x: torch.Tensor, sd) -> torch.Tensor:
    y = F.conv2d(x.double(), _d(sd, "conv1.0.weight"), _d(sd, "conv1.0.bias"), stride=2, padding=3)
    return F.max_pool2d(F.relu(_bn(y, sd, "conv1.1")), 2)


def block(a: torch.Tensor, sd, i: int) -> torch.Tensor:
    a, p = a.double(), f"res_blocks.{i}"
    identity = _bn(F.conv2d(a, _d(sd, p + ".skip.0.weight"), _d(sd, p + ".skip.0.bias"), stride=2), sd, p + ".skip.1")
    out = F.relu(_bn(F.conv2d(a, _d(sd, p + ".conv1.weight"), _d(sd, p + ".conv1.bias"), stride=2, padding=1), sd, p + ".bn1"))
    out = _bn(F.conv2d(out, _d(sd, p + ".conv2.weight"), _d(sd, p + ".conv2.bias"), padding=1), sd, p + ".bn2")
    return F.relu(out + identity)


def head(a3: torch.Tensor, sd) -> torch.Tensor:
    return F.linear(a3.double().mean(dim=(2, 3)), _d(sd, "fc.2.weight"), _d(sd, "fc.2.bias"))


def n_blocks(sd) -> int:
    i = 0
    while f"res_blocks.{i}.conv1.weight" in sd:
        i += 1
    return i


def fold(sd, conv: str, bn: str):
    """(W, b) in float64 as ``fold`` of resnet.hip computes them, BEFORE the rounding to float32."""
    s = _d(sd, bn + ".weight") / torch.sqrt(_d(sd, bn + ".running_var") + EPS)
    return _d(sd, conv + ".weight") * s[:, None, None, None], (_d(sd, conv + ".bias") - _d(sd, bn + ".running_mean")) * s + _d(sd, bn + ".bias")


def block_folds(sd, i: int):
    p = f"res_blocks.{i}"
    return fold(sd, p + ".conv1", p + ".bn1"), fold(sd, p + ".conv2", p + ".bn2"), fold(sd, p + ".skip.0", p + ".skip.1")


# ------------------------------------------------------------------------------------------ dispatch
STEM_SB_MAXL = 22                                  # 2 * 256 * 22 = 11 264 pixels
RBX_BLOCK0_ROWS = (16, 17, 22, 23, 24, 26, 27)     # block-0 inputs R x 25 the split-bf16 block kernel is compiled for
RBX_BLOCK1_ROWS = (8, 9, 11, 12, 13, 14)           # block-1 inputs R x 13
RBX_G_TALL = 1                                     # clips per workgroup of block 1 above 12 rows (2 up to 12)
RB_CFG = ((32, 64, 1, 3, 4), (64, 128, 3, 2, 8))   # RbCfg<CIN, COUT, G, MW, WAVES> of the single-bf16 blocks 0 and 1
RB_FIXED = ((22, 25), (11, 13))                    # ... and the input each has a compiled-geometry instantiation for
STEM_LDS_LIMIT = 64 * 1024
RB_LDS_LIMIT = 160 * 1024

Stage = namedtuple("Stage", "kernel body clips scheme in_hw out_hw")
Plan = namedtuple("Plan", "stem blocks head nan stores_bf16")


def make_shapes(H: int, W: int, blocks: int = 2) -> List[Tuple[int, int]]:
    """[(h, w)] after the stem + pool and after every block (``make_shapes`` / ``gen_shapes``)."""
    c1h, c1w = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    out = [(c1h // 2, c1w // 2)]
    for _ in range(blocks):
        h, w = out[-1]
        out.append(((h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1))
    return out


def stem_lds(H: int, W: int) -> int:
    (p1h, p1w), = make_shapes(H, W, 0)
    nrows = max(4 * p1h + 6, H + 3)
    pitch = (max(4 * p1w + 6, W + 3) + 1) & ~1
    return nrows * pitch * 2


def rbx_compiled(blk: int, xh: int, xw: int) -> bool:
    return (xw == 25 and xh in RBX_BLOCK0_ROWS) if blk == 0 else (xw == 13 and xh in RBX_BLOCK1_ROWS)


def rbx_t16(cin: int, cout: int, xh: int) -> bool:
    return (cin, cout) in ((32, 64), (64, 128)) and (cin == 64 or xh <= 26)


def rbx_block1_clips(xh: int) -> int:
    return 2 if xh <= 12 else RBX_G_TALL


def rb_mtmax(cfg) -> int:
    _, cout, _, mw, waves = cfg
    return waves // (cout // 32) * mw


def rb_lds_bytes(cfg, xh, xw, oh, ow) -> int:
    cin, cout, g, _, waves = cfg
    images = (g * (xh + 2) * (xw + 2) * cin + g * (oh + 2) * (ow + 2) * cout) * 2
    tile = rb_mtmax(cfg) * 32 * (cout + 8) * 2 + waves * 2 * 4
    return max(images, tile)


def plan(dtype: str, H: int, W: int, channels: Sequence[int] = SHIPPED) -> Optional[Plan]:
    """What ``cough_resnet_forward`` launches for an (H, W) image, or None if the image vanishes.

    stem     ``stem_mfma<float>`` | ``stem_mfma<bf16>`` | ``stem_bf16<x3>`` | ``stem_bf16<bf16>``
    blocks   ``resblock_x3`` (body ``32x32`` | ``16x16x32``, clips per workgroup) | ``resblock_bf16:fixed`` |
             ``resblock_bf16:runtime`` (body ``32x32``, 1 / 3 clips) | ``conv_mfma<float,NT>`` | ``conv_gemm_bf16<NT>``
    head     ``fused`` | ``tail_kernel<float>`` | ``tail_kernel<bf16>`` | ``tail_generic_kernel``
    nan      ``flag`` (the stem's staging loop looked at every pixel) | ``rescan`` (``nan_rule_kernel`` reads the image)

    A tuple other than (32, 64, 128) takes ``gen_forward``: f32, ``conv_mfma<float,1>``, whatever the dtype.

    The three launch conditions of a single-bf16 fused block are LDS <= 160 KB, G OH OW <= 32 MTMAX and
    G XH XW CIN / 8 <= 16 THREADS.  Which can bind:
    * the staging limit never does.  Block 0: XH XW <= (2 OH)(2 OW) <= 4 * 192 = 768 < 16 * 256 / 4 = 1024.  Block 1:
      3 XH XW * 8 <= 8192 asks XH XW <= 341, and XH XW <= 4 * 42 = 168.
    * the 160 KB limit does bind, for low and wide block inputs, where the zero border is a large part of the LDS image:
      block 1 at 4 x 42 -> 2 x 21 is inside the pixel limit (3 * 42 = 126 <= 128) and needs 3 * (6 * 44 * 64 +
      4 * 23 * 128) * 2 = 172 032 B > 163 840 B; block 0 at 2 x 384 -> 1 x 192 needs (4 * 386 * 32 + 3 * 194 * 64) * 2
      = 173 312 B.  ``bf16_approx`` 32 x 336 (8 x 84 -> 4 x 42 -> 2 x 21) is in the matrix for it: block 0 fused, block 1
      refused by the LDS limit alone.  ``test_which_launch_limits_of_the_bf16_blocks_can_bind`` searches every block
      input for both statements.
    """
    assert dtype in DTYPES
    channels = tuple(channels)
    nb = len(channels) - 1
    shp = make_shapes(H, W, nb)
    if any(h < 1 or w < 1 for h, w in shp):
        return None
    if channels != SHIPPED:
        blocks = [Stage("conv_mfma<float,1>", "32x32", 0, "f32", shp[i], shp[i + 1]) for i in range(nb)]
        return Plan(Stage("stem_mfma<float>", "32x32", 0, "f32", (H, W), shp[0]), blocks, "tail_generic_kernel", "rescan", False)
    fits = H * W <= 2 * 256 * STEM_SB_MAXL
    if dtype == "bf16_approx" and stem_lds(H, W) <= STEM_LDS_LIMIT and fits:
        stem, nan = Stage("stem_bf16<bf16>", "32x32", 1, "bf16", (H, W), shp[0]), "flag"
    elif dtype == "bf16x3" and 2 * stem_lds(H, W) <= STEM_LDS_LIMIT and fits:
        stem, nan = Stage("stem_bf16<x3>", "32x32", 1, "bf16x3", (H, W), shp[0]), "flag"
    else:
        stem, nan = Stage("stem_mfma<bf16>" if dtype == "bf16_approx" else "stem_mfma<float>", "32x32", 0, "f32", (H, W), shp[0]), "rescan"
    blocks, head_done = [], False
    for i in range(2):
        (xh, xw), (oh, ow) = shp[i], shp[i + 1]
        cin, cout = channels[i], channels[i + 1]
        if dtype == "bf16x3" and rbx_compiled(i, xh, xw):
            blocks.append(Stage("resblock_x3", "16x16x32" if rbx_t16(cin, cout, xh) else "32x32",
                                1 if i == 0 else rbx_block1_clips(xh), "bf16x3", (xh, xw), (oh, ow)))
            head_done = head_done or i == 1
            continue
        if dtype == "bf16_approx":
            cfg = RB_CFG[i]
            g, threads = cfg[2], cfg[4] * 64
            if rb_lds_bytes(cfg, xh, xw, oh, ow) <= RB_LDS_LIMIT and g * oh * ow <= rb_mtmax(cfg) * 32 and \
                    g * xh * xw * (cin // 8) <= 16 * threads:
                blocks.append(Stage("resblock_bf16:" + ("fixed" if (xh, xw) == RB_FIXED[i] else "runtime"), "32x32", g, "bf16",
                                    (xh, xw), (oh, ow)))
                head_done = head_done or i == 1
                continue
            blocks.append(Stage(f"conv_gemm_bf16<{2 if cout == 64 else 4}>", "32x32", 0, "bf16", (xh, xw), (oh, ow)))
            continue
        blocks.append(Stage(f"conv_mfma<float,{2 if cout == 64 else 4}>", "32x32", 0, "f32", (xh, xw), (oh, ow)))
    head_k = "fused" if head_done else ("tail_kernel<bf16>" if dtype == "bf16_approx" else "tail_kernel<float>")
    return Plan(stem, blocks, head_k, nan, dtype == "bf16_approx")


def plan_row(p: Plan):
    """The part of a plan the hand-written tables state."""
    return (p.stem.kernel, [(b.kernel, b.body, b.clips) for b in p.blocks], p.head, p.nan)


def stage_path(stage: Stage) -> str:
    """The name a stage's kernel instantiation is reported under (profiles/resnet_layer_precision.txt)."""
    if stage.kernel == "resblock_x3":
        return f"resblock_x3<{stage.in_hw[1]},{stage.body},G{stage.clips}>"
    if stage.kernel.startswith("resblock_bf16"):
        return f"{stage.kernel}<G{stage.clips}>"
    return stage.kernel


# ------------------------------------------------------------------------------------------ bounds
def rel_bound(scheme: str, k: int, c: int = C_F32) -> float:
    if scheme == "f32":
        return (k + c) * U
    if scheme == "bf16x3":
        return (3 * E_SPLIT + (3 * k + c) * U) * (1 + 2.0 ** -7)
    if scheme == "bf16":
        return 2 * E_BF16 + E_BF16 ** 2 + (k + c) * U
    raise ValueError(scheme)


H_STORE = {"f32": 0.0, "bf16x3": E_SPLIT, "bf16": E_BF16}


def stage_bound(stage, x: torch.Tensor, sd, scheme: str, stores_bf16: bool = False) -> torch.Tensor:
    """Per-element absolute bound of a stage's output against ``stem_pool(x, sd)`` (``stage == "stem"``) or
    ``block(x, sd, stage)`` (an int); see the module docstring."""
    x = x.double()
    if stage == "stem":
        w, b = fold(sd, "conv1.0", "conv1.1")
        a = F.conv2d(x.abs(), w.abs(), b.abs(), stride=2, padding=3)
        e = F.max_pool2d(rel_bound(scheme, 49) * a, 2)
        y = stem_pool(x, sd)
    else:
        (w1, b1), (w2, b2), (ws, bs) = block_folds(sd, stage)
        cin, cout = w1.shape[1], w1.shape[0]
        a1 = F.conv2d(x.abs(), w1.abs(), b1.abs(), stride=2, padding=1)
        e1 = rel_bound(scheme, 9 * cin) * a1
        h_ref = F.relu(F.conv2d(x, w1, b1, stride=2, padding=1))
        e_h = e1 + H_STORE[scheme] * (h_ref + e1)
        a2 = F.conv2d(h_ref + e_h, w2.abs(), b2.abs() + bs.abs(), padding=1) + F.conv2d(x.abs(), ws.abs(), stride=2)
        e = rel_bound(scheme, 9 * cout + cin, C_F32 + 1) * a2 + F.conv2d(e_h, w2.abs(), padding=1)
        y = block(x, sd, stage)
    if stores_bf16:
        e = e + E_BF16 * (y.abs() + e)
    return e


def head_bound(a3: torch.Tensor, sd):
    """(float64 logits over the activation the kernels themselves produced, their float32 budget)."""
    a3, w, b = a3.double(), _d(sd, "fc.2.weight"), _d(sd, "fc.2.bias")
    hw = a3.shape[2] * a3.shape[3]
    v = a3.mean(dim=(2, 3))
    e_v = (hw + 2) * U * a3.abs().mean(dim=(2, 3))
    logits = v @ w.t() + b
    e_l = e_v @ w.abs().t() + (w.shape[1] + 2) * U * (v.abs() @ w.abs().t() + b.abs())
    return logits, e_l


# ------------------------------------------------------------------------------------------ emulation
DEFECTS = {
    "drop_lo_hi": "split-bf16: the lo*hi product (activation lo, weight hi) of the stem, or of conv2 + projection, is missing",
    "border_wrap": "the zero border right of an input row is read as the first pixel of the next row (conv1's x image)",
    "proj_centre": "the projection reads x[2r + 1, 2c + 1] instead of the stride-2 centre x[2r, 2c]",
    "clip_h": "the second clip of a workgroup (clip index 1 mod G) runs conv2 over the first clip's h",
    "bias_no_skip": "b2 is added without the projection's bias",
    "kstep_swap": "conv2's weight fragments of k-steps 0 and 1 (channels 0..15 / 16..31 of tap (0, 0)) are swapped for the "
                  "first 32-channel tile",
}


def _f32(t):
    return t.float().double()


def _mm(x, w, scheme, defect=None, **kw):
    """conv2d of float64 tensors holding the values the kernel holds, under an operand scheme."""
    if scheme == "f32":
        return F.conv2d(x.float(), w.float(), **kw).double()            # a true float32 convolution
    if scheme == "bf16x3" and defect == "drop_lo_hi":
        xh, _ = emu.split(x)
        wh, wl = emu.split(w)
        return F.conv2d(xh, wh, **kw) + F.conv2d(xh, wl, **kw)
    return emu._conv(x, w, scheme, **kw)


def _keep(y, scheme):
    """h as the kernel keeps it between conv1 and conv2."""
    return _f32(y) if scheme == "f32" else emu._store(y, scheme)


def emulate_stage(stage, x: torch.Tensor, sd, scheme: str, stores_bf16: bool = False, defect: Optional[str] = None,
                  clips: int = 0) -> torch.Tensor:
    """A stage under an operand scheme on the CPU (float64 tensors holding the rounded values), float32 folded weights and
    biases as the library uploads them.  ``defect``: a key of ``DEFECTS`` (block stages; ``drop_lo_hi`` also in the stem); ``clips``: clips per workgroup,
    for ``clip_h``."""
    assert defect is None or defect in DEFECTS
    x = x.double()
    if stage == "stem":
        w, b = fold(sd, "conv1.0", "conv1.1")
        y = _mm(x, _f32(w), scheme, defect if defect == "drop_lo_hi" else None, stride=2, padding=3)
        y = F.max_pool2d(F.relu((y.float() + b.float()[None, :, None, None]).double()), 2)
    else:
        (w1, b1), (w2, b2), (ws, bs) = ((_f32(w), b.float()) for w, b in block_folds(sd, stage))
        if defect == "border_wrap":
            xp = F.pad(x, (1, 1, 1, 1))
            xp[:, :, 1:-2, -1] = x[:, :, 1:, 0]                 # border cell (r, W) <- pixel (r + 1, 0)
            c1 = _mm(xp, w1, scheme, stride=2)
        else:
            c1 = _mm(x, w1, scheme, stride=2, padding=1)
        h = _keep(F.relu((c1.float() + b1[None, :, None, None]).double()), scheme)
        if defect == "clip_h":
            assert clips >= 2 and x.shape[0] >= 2
            h = h.clone()
            for n in range(1, x.shape[0], clips):
                h[n] = h[n - 1]
        if defect == "kstep_swap":
            w2 = w2.clone()
            w2[:32, 0:16, 0, 0], w2[:32, 16:32, 0, 0] = w2[:32, 16:32, 0, 0].clone(), w2[:32, 0:16, 0, 0].clone()
        xs = F.pad(x, (0, 1, 0, 1))[:, :, 1:, 1:] if defect == "proj_centre" else x
        lo_hi = defect if defect == "drop_lo_hi" else None
        acc = _mm(h, w2, scheme, lo_hi, padding=1) + _mm(xs, ws, scheme, lo_hi, stride=2)
        bias = b2 if defect == "bias_no_skip" else b2 + bs                     # one float32 add, at create time
        y = F.relu((acc.float() + bias[None, :, None, None]).double())
    return emu.bf16(y) if stores_bf16 else y


# ------------------------------------------------------------------------------------------ the per-pixel check
Worst = namedtuple("Worst", "ratio stage kernel clip channel row col err bound")


def check_stage(stage, kernel: str, got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor) -> Worst:
    """The worst |got - ref| / bound over every pixel and channel, with its coordinates."""
    got = got.double().cpu()
    assert got.shape == ref.shape, (stage, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"stage {stage}: non-finite output"
    err = (got - ref).abs()
    ratio = err / bound.clamp(min=1e-300)
    ratio = torch.where((err == 0) & (bound == 0), torch.zeros_like(ratio), ratio)
    i = int(ratio.argmax())
    n, c, r, col = (int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape))
    return Worst(float(ratio.flatten()[i]), stage, kernel, n, c, r, col, float(err.flatten()[i]), float(bound.flatten()[i]))


def check_net(x: torch.Tensor, sd, p: Plan, tap) -> List[Worst]:
    """The per-pixel check both test files run.  ``tap(k)`` is the device's (or the emulation's) activation k = 1 (stem) ..
    n_blocks + 1.  The stem is held to its bound over x, block i to its bound over ``tap(i + 1)`` itself."""
    st = p.stores_bf16
    prev = tap(1)
    out = [check_stage("stem", p.stem.kernel, prev, stem_pool(x, sd), stage_bound("stem", x, sd, p.stem.scheme, st))]
    for i, b in enumerate(p.blocks):
        got = tap(i + 2)
        out.append(check_stage(i, b.kernel, got, block(prev, sd, i), stage_bound(i, prev, sd, b.scheme, st)))
        prev = got
    return out


def emulate_net(x: torch.Tensor, sd, p: Plan, defect: Optional[str] = None, at: Optional[int] = None) -> List[torch.Tensor]:
    """[a1, a2, ...] of the clean emulation, stage ``at`` ("stem" or a block index) with ``defect`` planted."""
    acts = [emulate_stage("stem", x, sd, p.stem.scheme, p.stores_bf16, defect if at == "stem" else None)]
    for i, b in enumerate(p.blocks):
        acts.append(emulate_stage(i, acts[-1], sd, b.scheme, p.stores_bf16, defect if i == at else None, b.clips))
    return acts


# ------------------------------------------------------------------------------------------ the matrix
Case = namedtuple("Case", "dtype H W channels nan")
BATCH = 5        # 3 + 2 for three-clip workgroups, 2 + 2 + 1 for two-clip ones


def _c(dtype, H, W, nan=False, channels=SHIPPED):
    return Case(dtype, H, W, channels, nan)


CASES = [
    _c("fp32", 3, 3), _c("fp32", 17, 33), _c("fp32", 90, 101),
    _c("bf16x3", 63, 99), _c("bf16x3", 110, 102),
    _c("bf16x3", 90, 101), _c("bf16x3", 96, 101), _c("bf16x3", 103, 101),
    _c("bf16x3", 74, 101, True), _c("bf16x3", 100, 101, True), _c("bf16x3", 90, 104, True),
    _c("bf16x3", 110, 103, True),
    _c("bf16x3", 40, 33), _c("bf16x3", 3, 3),
    _c("bf16x3", 8, 1400),
    _c("bf16_approx", 90, 101, True),
    _c("bf16_approx", 64, 101), _c("bf16_approx", 96, 101),
    _c("bf16_approx", 110, 101),
    _c("bf16_approx", 112, 112),
    _c("bf16_approx", 17, 33),
    _c("bf16_approx", 32, 336),
    _c("fp32", 40, 33, channels=(5, 7, 9)), _c("fp32", 17, 30, channels=(64, 32)),
]


def case_id(c: Case) -> str:
    return f"{c.dtype}-{c.H}x{c.W}" + ("" if c.channels == SHIPPED else "-ch" + "_".join(map(str, c.channels)))


# hand-written: (stem, [(block kernel, body, clips per workgroup; 0 = not clip-grouped)], head, NaN rule)
_X3, _T16, _B32 = "resblock_x3", "16x16x32", "32x32"
_F2, _F4, _F1 = ("conv_mfma<float,2>", _B32, 0), ("conv_mfma<float,4>", _B32, 0), ("conv_mfma<float,1>", _B32, 0)
_G2, _G4 = ("conv_gemm_bf16<2>", _B32, 0), ("conv_gemm_bf16<4>", _B32, 0)
_RT0, _RT1 = ("resblock_bf16:runtime", _B32, 1), ("resblock_bf16:runtime", _B32, 3)
EXPECT = {
    "fp32-3x3": ("stem_mfma<float>", [_F2, _F4], "tail_kernel<float>", "rescan"),
    "fp32-17x33": ("stem_mfma<float>", [_F2, _F4], "tail_kernel<float>", "rescan"),
    "fp32-90x101": ("stem_mfma<float>", [_F2, _F4], "tail_kernel<float>", "rescan"),
    # 63 x 99 -> 16 x 25 -> 8 x 13; 110 x 102 -> 27 x 25 (the 32x32 body: more than 26 rows) -> 14 x 13 (one clip)
    "bf16x3-63x99": ("stem_bf16<x3>", [(_X3, _T16, 1), (_X3, _T16, 2)], "fused", "flag"),
    "bf16x3-110x102": ("stem_bf16<x3>", [(_X3, _B32, 1), (_X3, _T16, 1)], "fused", "flag"),
    "bf16x3-90x101": ("stem_bf16<x3>", [(_X3, _T16, 1), (_X3, _T16, 2)], "fused", "flag"),        # 22 -> 11
    "bf16x3-96x101": ("stem_bf16<x3>", [(_X3, _T16, 1), (_X3, _T16, 2)], "fused", "flag"),        # 24 -> 12
    "bf16x3-103x101": ("stem_bf16<x3>", [(_X3, _T16, 1), (_X3, _T16, 1)], "fused", "flag"),       # 26 -> 13
    "bf16x3-74x101": ("stem_bf16<x3>", [_F2, (_X3, _T16, 2)], "fused", "flag"),                   # 18 x 25 -> 9 x 13
    "bf16x3-100x101": ("stem_bf16<x3>", [_F2, (_X3, _T16, 1)], "fused", "flag"),                  # 25 x 25 -> 13 x 13
    "bf16x3-90x104": ("stem_bf16<x3>", [_F2, (_X3, _T16, 2)], "fused", "flag"),                   # 22 x 26 -> 11 x 13
    "bf16x3-110x103": ("stem_mfma<float>", [_F2, (_X3, _T16, 1)], "fused", "rescan"),             # 27 x 26 -> 14 x 13
    "bf16x3-40x33": ("stem_bf16<x3>", [_F2, _F4], "tail_kernel<float>", "flag"),
    "bf16x3-3x3": ("stem_bf16<x3>", [_F2, _F4], "tail_kernel<float>", "flag"),
    "bf16x3-8x1400": ("stem_mfma<float>", [_F2, _F4], "tail_kernel<float>", "rescan"),
    "bf16_approx-90x101": ("stem_bf16<bf16>", [("resblock_bf16:fixed", _B32, 1), ("resblock_bf16:fixed", _B32, 3)], "fused", "flag"),
    "bf16_approx-64x101": ("stem_bf16<bf16>", [_RT0, _RT1], "fused", "flag"),
    "bf16_approx-96x101": ("stem_bf16<bf16>", [_RT0, _RT1], "fused", "flag"),                     # 3 * 6 * 7 = 126 <= 128
    "bf16_approx-110x101": ("stem_bf16<bf16>", [_RT0, _G4], "tail_kernel<bf16>", "flag"),         # 14 * 13 = 182; 3 * 49 > 128
    "bf16_approx-112x112": ("stem_mfma<bf16>", [_G2, _G4], "tail_kernel<bf16>", "rescan"),        # 12 544 px; 14 * 14 = 196
    "bf16_approx-17x33": ("stem_bf16<bf16>", [_RT0, _RT1], "fused", "flag"),
    # 8 x 84 -> 4 x 42 (168 <= 192 px) -> 2 x 21: 3 * 42 = 126 <= 128 px, but 172 032 B of LDS > 160 KB
    "bf16_approx-32x336": ("stem_bf16<bf16>", [_RT0, _G4], "tail_kernel<bf16>", "flag"),
    "fp32-40x33-ch5_7_9": ("stem_mfma<float>", [_F1, _F1], "tail_generic_kernel", "rescan"),
    "fp32-17x30-ch64_32": ("stem_mfma<float>", [_F1], "tail_generic_kernel", "rescan"),
}


def case_weights(c: Case) -> Dict[str, torch.Tensor]:
    from cough_detector_amd import synth
    return synth.random_state_dict(seed=100 + sum(c.channels), channels=c.channels)


def case_image(c: Case, batch: int = BATCH) -> torch.Tensor:
    """Seeded N(0, 2^2) images."""
    g = torch.Generator().manual_seed(2000 + 7 * c.H + c.W)
    return torch.randn((batch, 1, c.H, c.W), generator=g) * 2.0
