"""Host-side mirror of the reference classifier interface, backed by the HIP kernels K2-K5 (residual net) and
``csrc/cnn.hip`` (the two conv-stack nets).

Same names and constructor arguments as ``/root/reference/src/model.py``
(``ConvBlock`` :11-40, ``CoughDetector`` :43-141, ``CoughDetectorSmall`` :144-207,
``CoughDetectorResidual`` :210-265, ``ResidualBlock`` :268-293, ``create_model`` :296-316,
``count_parameters`` :319-321).  The modules below are *parameter containers* with the reference's
exact sub-module layout, so ``state_dict()`` / ``load_state_dict()`` use the reference's keys
(``conv1.0.weight`` ... ``fc.2.bias``); ``forward`` does not run them -- it hands the tensors to
``cough_resnet_forward`` (``csrc/resnet.hip``) through the C-ABI.  Inference (eval mode) only.
"""
from __future__ import annotations

import warnings
import ctypes as C
from typing import Dict, Tuple

import torch
import torch.nn as nn

from . import _lib
from ._native import NativeModule, conv_bn, cuda_device


class ResidualBlock(NativeModule):
    """The reference block (``src/model.py:268-293``): conv1/bn1 (3x3, stride s), conv2/bn2 (3x3, stride 1) and ``skip`` --
    a 1x1 stride-s conv + BN when ``stride != 1 or in_channels != out_channels``, ``nn.Identity()`` otherwise (:280-283).

    Inside ``CoughDetectorResidual`` the blocks run fused in the model's own kernels; called on its own
    (``block(x)``, x (B, in_channels, H, W)) a block runs through ``cough_resblock_forward`` on the exact-f32 MFMA
    conv kernels, eval-mode BatchNorm folded."""

    def __init__(self, in_channels: int, out_channels: int, stride: int = 2):
        super().__init__("cough_resblock_destroy")
        if not 1 <= int(stride) <= 4 or in_channels < 1 or out_channels < 1:
            raise ValueError(f"ResidualBlock: in_channels={in_channels}, out_channels={out_channels}, stride={stride}")
        self.in_channels, self.out_channels, self.stride = int(in_channels), int(out_channels), int(stride)
        self.conv1 = nn.Conv2d(in_channels, out_channels, 3, stride=stride, padding=1)
        self.bn1 = nn.BatchNorm2d(out_channels)
        self.conv2 = nn.Conv2d(out_channels, out_channels, 3, padding=1)
        self.bn2 = nn.BatchNorm2d(out_channels)
        self.skip = nn.Sequential(nn.Conv2d(in_channels, out_channels, 1, stride=stride),
                                  nn.BatchNorm2d(out_channels)) if in_channels != out_channels or stride != 1 else nn.Identity()
        self.eval()

    def _create(self) -> C.c_void_p:
        sd = self._host_weights()
        c1, c2 = conv_bn(sd, "conv1", "bn1"), conv_bn(sd, "conv2", "bn2")
        sk = conv_bn(sd, "skip.0", "skip.1") if isinstance(self.skip, nn.Sequential) else None
        h = C.c_void_p()
        _lib.check(_lib.load().cough_resblock_create(C.byref(h), self.in_channels, self.out_channels, self.stride,
                                                      C.byref(c1), C.byref(c2), C.byref(sk) if sk is not None else None,
                                                      float(self.bn1.eps)), "cough_resblock_create")
        return h

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        src_dev = x.device
        xf = self._gpu_input(x, self.in_channels)
        dev = xf.device
        b, _, hgt, wid = xf.shape
        lib, h = _lib.load(), self._native()
        oh, ow = C.c_int(), C.c_int()
        _lib.check(lib.cough_resblock_out_shape(h, hgt, wid, C.byref(oh), C.byref(ow)), "cough_resblock_out_shape")
        y = torch.empty((b, self.out_channels, oh.value, ow.value), dtype=torch.float32, device=dev)
        if b == 0:
            return y.to(src_dev)
        ws = self._ws.get(max(lib.cough_resblock_workspace_bytes(h, b, hgt, wid), 256), dev)
        _lib.check(lib.cough_resblock_forward(h, xf.data_ptr(), b, hgt, wid, y.data_ptr(), ws.data_ptr(), ws.numel(),
                                              torch.cuda.current_stream(dev).cuda_stream), "cough_resblock_forward")
        return y.to(src_dev)


class CoughDetectorResidual(NativeModule):
    """Residual CNN, (B, 1, F, T) float32 -> (B, 2) logits, executed by hand-written gfx950 kernels.

    ``compute_dtype``:

    * ``"fp32"``   exact-f32 MFMA (``v_mfma_f32_32x32x2_f32``): CPU-reference numerics, ~7x slower.
    * ``"bf16x3"`` split-bf16: every operand (feature image, activations, BN-folded weights) is a pair of bf16
      values hi + lo (16 significant bits) and every k-step is three bf16 MFMAs (hi*hi + hi*lo + lo*hi) into an
      f32 accumulator; activations are f32 in HBM.  Logits stay within 1e-3 of the f32 reference at a trained
      head's scale (measured 7e-5 on the goldens).  The throughput dtype of ``bench.py``.
    * ``"bf16_approx"`` single bf16 operands and bf16 activations (stem included), f32 accumulate: fastest, but
      APPROXIMATE -- logit error ~2 % of the class-margin spread (5.5e-2 on the goldens), outside the 1e-3
      tolerance.  ``"bf16"`` is a deprecated alias that emits a ``UserWarning`` saying so.
    """

    def __init__(self, n_mels: int = 64, num_classes: int = 2, in_channels: int = 1,
                 channels: Tuple[int, ...] = (32, 64, 128), dropout: float = 0.5, compute_dtype: str = "fp32"):
        super().__init__("cough_resnet_destroy")
        channels = tuple(int(c) for c in channels)
        if num_classes != 2 or in_channels != 1:
            raise ValueError("CoughDetectorResidual: the MI355X path implements num_classes=2, in_channels=1")
        if len(channels) < 2 or len(channels) > 17 or any(c < 1 or c > 1024 for c in channels):
            raise ValueError("CoughDetectorResidual: channels must be 2..17 values in 1..1024")
        self.channels = channels          # (32, 64, 128): the fused kernels; any other tuple: the exact-f32 kernels
        # what was asked for ('bf16' = deprecated alias of 'bf16_approx', warns); ``effective_dtype`` is what runs
        self.compute_dtype = _lib.normalize_dtype(compute_dtype, ("fp32", "bf16x3", "bf16_approx"))
        self._warned_fallback = set()
        self.conv1 = nn.Sequential(nn.Conv2d(in_channels, channels[0], 7, stride=2, padding=3),
                                   nn.BatchNorm2d(channels[0]), nn.ReLU(), nn.MaxPool2d(2))
        self.res_blocks = nn.ModuleList()
        in_ch = channels[0]
        for out_ch in channels[1:]:
            self.res_blocks.append(self._make_res_block(in_ch, out_ch))
            in_ch = out_ch
        self.global_pool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Sequential(nn.Flatten(), nn.Dropout(dropout), nn.Linear(channels[-1], num_classes))
        self.eval()

    def _make_res_block(self, in_ch: int, out_ch: int) -> nn.Module:
        return ResidualBlock(in_ch, out_ch)

    def _create(self) -> C.c_void_p:
        lib, sd = _lib.load(), self._host_weights()
        h = C.c_void_p()
        if self.channels == (32, 64, 128):
            w = _lib.ResNetWeights()
            w.stem = conv_bn(sd, "conv1.0", "conv1.1")
            for i in range(2):
                p = f"res_blocks.{i}"
                w.block[i].conv1 = conv_bn(sd, p + ".conv1", p + ".bn1")
                w.block[i].conv2 = conv_bn(sd, p + ".conv2", p + ".bn2")
                w.block[i].skip = conv_bn(sd, p + ".skip.0", p + ".skip.1")
            w.fc_w = _lib.fptr(sd["fc.2.weight"])
            w.fc_b = _lib.fptr(sd["fc.2.bias"])
            w.bn_eps = float(self.conv1[1].eps)
            _lib.check(lib.cough_resnet_create(C.byref(h), C.byref(w), _lib.DTYPES[self.compute_dtype]),
                       "cough_resnet_create")
        else:                                  # any other channel tuple (src/model.py:216-247): exact-f32 kernels
            nb = len(self.channels) - 1
            blocks = (_lib.ResBlockWeights * nb)()
            for i in range(nb):
                p = f"res_blocks.{i}"
                blocks[i].conv1 = conv_bn(sd, p + ".conv1", p + ".bn1")
                blocks[i].conv2 = conv_bn(sd, p + ".conv2", p + ".bn2")
                blocks[i].skip = conv_bn(sd, p + ".skip.0", p + ".skip.1")
            stem = conv_bn(sd, "conv1.0", "conv1.1")
            chans = (C.c_int * (nb + 1))(*self.channels)
            dtype = _lib.DTYPES[self.compute_dtype]
            _lib.check(lib.cough_resnet_create_ex(C.byref(h), nb, chans, C.byref(stem), blocks, _lib.fptr(sd["fc.2.weight"]),
                                                  _lib.fptr(sd["fc.2.bias"]), float(self.conv1[1].eps), dtype),
                       "cough_resnet_create_ex")
        return h

    # ------------------------------------------------------------------ forward
    def effective_dtype(self, height: int = 90, width: int = 101) -> str:
        """The accuracy class and throughput a ``(height, width)`` feature image gets: ``"bf16x3"`` / ``"bf16_approx"``
        when every stage runs the fused kernels of that mode, ``"fp32"`` when the f32 MFMA kernels carry block 0.  The
        fused reduced-precision kernels are compiled for the shipped ``channels=(32, 64, 128)``
        (``cough_resnet_create``); any other tuple goes through ``cough_resnet_create_ex`` onto the exact-f32 MFMA
        kernels, stem and head included.  The split-bf16 residual blocks are compiled for the images the reference's own
        flags produce at 101 frames -- 90 rows (shipped; block inputs 22x25 and 11x13), 103 rows (constructor defaults:
        delta-delta on; 26x25 / 13x13), 110 rows (+ contrast and centroid rows; 27x25 / 14x13), 91..98 rows (contrast
        rows on the shipped set) and 63..70 rows (use_mfcc=False, 64 rows + contrast rows).

        ``"fp32"`` for a ``bf16x3`` model with the shipped channels is NOT "every kernel in exact f32": the kernels are
        picked per stage (``csrc/resnet_plan.h: plan_resnet``; restated as ``plan()`` in ``tests/resnet_layer_ref.py``).
        The stem is the split-bf16 kernel whenever the image has at most 11 264 pixels and fits its LDS image, and
        block 1 is the fused split-bf16 kernel (with its head) whenever ITS input is one of the compiled 8..14 x 13
        shapes, whatever ran block 0 -- e.g. 71..74, 83..86 and 99..102 rows at 99..102 frames, or 103..106 frames at a
        compiled height.  What is guaranteed for such an image is split-bf16 accuracy or better at every stage (each
        within the per-pixel budget of its kernel family) and no more than the f32 path's time."""
        if self.compute_dtype == "fp32":
            return self.compute_dtype
        if self.channels != (32, 64, 128):
            return "fp32"
        if self.compute_dtype == "bf16x3":
            # the kernels are selected by the block-0 input (stem + pool output), csrc/resnet_plan.h: rbx_compiled() over
            # RBX_BLOCK0_ROWS x RBX_COLS[0], which X3_BLOCK_INPUTS below restates (tests/test_resnet_layer_ref_host.py):
            # 16x25 <- 63..66 rows, 17x25 <- 67..70, 22x25 <- 87..90, 23x25 <- 91..94, 24x25 <- 95..98, 26x25 <- 103..106,
            # 27x25 <- 107..110, each x 99..102 frames: every image the reference's flags produce at 1 s
            p1 = (((height - 1) // 2 + 1) // 2, ((width - 1) // 2 + 1) // 2)
            if p1 not in self.X3_BLOCK_INPUTS:
                return "fp32"
        return self.compute_dtype

    X3_BLOCK_INPUTS = ((16, 25), (17, 25), (22, 25), (23, 25), (24, 25), (26, 25), (27, 25))

    def _warn_fallback(self, height: int, width: int) -> None:
        eff = self.effective_dtype(height, width)
        if eff != self.compute_dtype and (height, width) not in self._warned_fallback:
            self._warned_fallback.add((height, width))
            why = (f"channels={self.channels}" if self.channels != (32, 64, 128) else f"a {height}x{width} feature image")
            how = ("running the exact-f32 MFMA kernels instead (same or better accuracy"
                   if self.channels != (32, 64, 128) else
                   "the f32 MFMA kernels run every stage that has no kernel of that mode for it (each stage at "
                   "split-bf16 accuracy or better")
            warnings.warn(f"CoughDetectorResidual: compute_dtype={self.compute_dtype!r} is not compiled for {why}; "
                          f"{how}, several times slower). See effective_dtype().", UserWarning, stacklevel=4)

    def _run(self, x: torch.Tensor, want_probs: bool):
        src_dev = x.device
        xf = self._gpu_input(x)
        dev = xf.device
        b, _, hgt, wid = xf.shape
        if b == 0:
            z = torch.empty((0, 2), dtype=torch.float32, device=src_dev)
            return (z, z.clone(), torch.empty((0,), dtype=torch.int32, device=src_dev)) if want_probs else z
        self._warn_fallback(hgt, wid)
        lib, h = _lib.load(), self._native()
        ws = self._ws.get(max(lib.cough_resnet_workspace_bytes(h, b, hgt, wid), 256), dev, note=(b, hgt, wid))
        logits = torch.empty((b, 2), dtype=torch.float32, device=dev)
        probs = torch.empty((b, 2), dtype=torch.float32, device=dev) if want_probs else None
        preds = torch.empty((b,), dtype=torch.int32, device=dev) if want_probs else None
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(lib.cough_resnet_forward(h, xf.data_ptr(), b, hgt, wid, logits.data_ptr(),
                                            probs.data_ptr() if want_probs else None,
                                            preds.data_ptr() if want_probs else None,
                                            ws.data_ptr(), ws.numel(), stream),
                   "cough_resnet_forward")
        if want_probs:
            return logits.to(src_dev), probs.to(src_dev), preds.to(src_dev)
        return logits.to(src_dev)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self._run(x, want_probs=False)

    def predict(self, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        _, probs, preds = self._run(x, want_probs=True)
        return preds.to(torch.int64), probs

    def read_activation(self, which: int) -> torch.Tensor:
        """Parity tap: activation after the stem (1), block 0 (2), block 1 (3), ... of the last forward on the current
        stream, NCHW f32."""
        if not 1 <= which <= len(self.channels):
            raise ValueError(f"which must be 1..{len(self.channels)}")
        dev = cuda_device()
        last = self._ws.lookup(dev)
        if last is None:
            raise RuntimeError("read_activation: no forward of this model has run on the current stream")
        ws, (b, hgt, wid) = last
        c = self.channels[which - 1]
        oh, ow = ((hgt - 1) // 2 + 1) // 2, ((wid - 1) // 2 + 1) // 2
        for _ in range(which - 1):
            oh, ow = (oh - 1) // 2 + 1, (ow - 1) // 2 + 1
        out = torch.empty((b, c, oh, ow), dtype=torch.float32, device=dev)
        _lib.check(_lib.load().cough_resnet_read_activation(self._native(), ws.data_ptr(), b, hgt, wid, which,
                                                            out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
                   "cough_resnet_read_activation")
        return out


class ConvBlock(nn.Module):
    """Parameter layout of the reference block (``src/model.py:11-40``): conv / bn (+ MaxPool2d, Dropout2d)."""

    def __init__(self, in_channels: int, out_channels: int, kernel_size: int = 3, stride: int = 1, padding: int = 1,
                 pool_size: int = 2):
        super().__init__()
        if (kernel_size, stride, padding) != (3, 1, 1) or pool_size not in (1, 2):
            raise ValueError("ConvBlock: the MI355X path implements kernel_size=3, stride=1, padding=1, pool_size 1 or 2")
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size=kernel_size, stride=stride, padding=padding)
        self.bn = nn.BatchNorm2d(out_channels)
        self.pool = nn.MaxPool2d(pool_size) if pool_size > 1 else nn.Identity()
        self.dropout = nn.Dropout2d(0.1)

    def forward(self, x):
        raise RuntimeError("ConvBlock is executed inside CoughDetector.forward on the MI355X path")


class _ConvStackNet(NativeModule):
    """Shared host side of the two conv-stack classifiers: builds the ``cough_cnn`` handle; subclasses describe their
    blocks (``_describe``) in terms of their own state_dict keys."""

    def __init__(self):
        super().__init__("cough_cnn_destroy")

    def _init_native(self, compute_dtype: str):
        # "fp32" (exact-f32 MFMA) and "bf16x3" (split-bf16: hi + lo operands, three MFMAs per k-step, f32 activations
        # in HBM) are the parity-grade modes; the single-bf16 mode is approximate and has to be asked for by that name
        # ('bf16' = deprecated alias, warns)
        self.compute_dtype = _lib.normalize_dtype(compute_dtype, ("fp32", "bf16x3", "bf16_approx"))
        self.eval()

    def _describe(self, sd: Dict[str, torch.Tensor]):
        """-> (blocks, fc1 prefix, fc2 prefix, bn eps); a block is (conv prefix, bn prefix, depthwise prefix | None,
        pool)."""
        raise NotImplementedError

    def _create(self) -> C.c_void_p:
        sd = self._host_weights()
        blocks, fc1, fc2, eps = self._describe(sd)
        arr = (_lib.CnnBlock * len(blocks))()
        for i, (conv, bn, dw, pool) in enumerate(blocks):
            w = sd[conv + ".weight"]
            arr[i].cin, arr[i].cout, arr[i].ksize, arr[i].pool = int(w.shape[1]), int(w.shape[0]), int(w.shape[2]), pool
            if dw is not None:
                arr[i].cin = int(sd[dw + ".weight"].shape[0])
                arr[i].dw_w, arr[i].dw_b = _lib.fptr(sd[dw + ".weight"]), _lib.fptr(sd[dw + ".bias"])
            arr[i].conv = conv_bn(sd, conv, bn)
        cw = _lib.CnnWeights(len(blocks), arr, int(sd[fc1 + ".weight"].shape[0]), _lib.fptr(sd[fc1 + ".weight"]),
                             _lib.fptr(sd[fc1 + ".bias"]), _lib.fptr(sd[fc2 + ".weight"]), _lib.fptr(sd[fc2 + ".bias"]),
                             float(eps))
        h = C.c_void_p()
        _lib.check(_lib.load().cough_cnn_create(C.byref(h), C.byref(cw), _lib.DTYPES[self.compute_dtype]),
                   "cough_cnn_create")
        return h

    def _prepare(self, x: torch.Tensor):
        """-> (lib, handle, x on the GPU, workspace or None for an empty batch)"""
        xf = self._gpu_input(x)
        b, _, hgt, wid = xf.shape
        lib, h = _lib.load(), self._native()
        if not b:
            return lib, h, xf, None
        need = lib.cough_cnn_workspace_bytes(h, b, hgt, wid)
        if need == 0:
            raise ValueError(f"input {hgt}x{wid} is too small for the network")
        return lib, h, xf, self._ws.get(max(need, 256), xf.device)

    def _run(self, x: torch.Tensor, want_probs: bool):
        src_dev = x.device
        lib, h, xf, ws = self._prepare(x)
        dev = xf.device
        b, _, hgt, wid = xf.shape
        logits = torch.empty((b, 2), dtype=torch.float32, device=dev)
        probs = torch.empty((b, 2), dtype=torch.float32, device=dev) if want_probs else None
        preds = torch.empty((b,), dtype=torch.int32, device=dev) if want_probs else None
        if b:
            _lib.check(lib.cough_cnn_forward(h, xf.data_ptr(), b, hgt, wid, logits.data_ptr(),
                                             probs.data_ptr() if want_probs else None,
                                             preds.data_ptr() if want_probs else None, ws.data_ptr(), ws.numel(),
                                             torch.cuda.current_stream(dev).cuda_stream),
                       "cough_cnn_forward")
        if want_probs:
            return logits.to(src_dev), probs.to(src_dev), preds.to(src_dev)
        return logits.to(src_dev)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self._run(x, want_probs=False)

    def predict(self, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        _, probs, preds = self._run(x, want_probs=True)
        return preds.to(torch.int64), probs

    def conv_output(self, x: torch.Tensor) -> torch.Tensor:
        """Parity tap: output of the conv stack before the global mean, (B, C, h, w) float32."""
        lib, h, xf, ws = self._prepare(x)
        dev = xf.device
        b, _, hgt, wid = xf.shape
        oh, ow = hgt, wid
        for _ in range(self._n_pools):
            oh, ow = oh // 2, ow // 2
        out = torch.empty((b, self._out_channels, oh, ow), dtype=torch.float32, device=dev)
        if b:
            _lib.check(lib.cough_cnn_conv_output(h, xf.data_ptr(), b, hgt, wid, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                                 torch.cuda.current_stream(dev).cuda_stream), "cough_cnn_conv_output")
        return out


class CoughDetector(_ConvStackNet):
    """The reference's "standard" CNN (``src/model.py:43-141``): ConvBlock x len(channels) -> global mean ->
    Linear -> ReLU -> Linear; (B, 1, F, T) float32 -> (B, 2) logits on hand-written gfx950 kernels."""

    def __init__(self, n_mels: int = 64, num_classes: int = 2, in_channels: int = 1,
                 channels: Tuple[int, ...] = (32, 64, 128, 256), fc_hidden: int = 128, dropout: float = 0.5,
                 compute_dtype: str = "fp32"):
        super().__init__()
        if num_classes != 2 or in_channels != 1:
            raise ValueError("CoughDetector: the MI355X path implements num_classes=2, in_channels=1")
        self.n_mels, self.num_classes = n_mels, num_classes
        layers, cur = [], in_channels
        for out_ch in channels:
            layers.append(ConvBlock(cur, out_ch))
            cur = out_ch
        self.conv_layers = nn.Sequential(*layers)
        self.global_pool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Sequential(nn.Linear(channels[-1], fc_hidden), nn.ReLU(), nn.Dropout(dropout),
                                nn.Linear(fc_hidden, num_classes))
        self._n_pools, self._out_channels = len(channels), channels[-1]
        self._init_native(compute_dtype)

    def _describe(self, sd):
        blocks = [(f"conv_layers.{i}.conv", f"conv_layers.{i}.bn", None, 2) for i in range(len(self.conv_layers))]
        return blocks, "fc.0", "fc.3", self.conv_layers[0].bn.eps


class CoughDetectorSmall(_ConvStackNet):
    """The reference's lightweight CNN (``src/model.py:144-207``): conv3x3 + three depthwise-separable blocks ->
    global mean -> Linear(128, 64) -> ReLU -> Linear(64, 2)."""

    def __init__(self, n_mels: int = 64, num_classes: int = 2, in_channels: int = 1, compute_dtype: str = "fp32"):
        super().__init__()
        if num_classes != 2 or in_channels != 1:
            raise ValueError("CoughDetectorSmall: the MI355X path implements num_classes=2, in_channels=1")
        self.features = nn.Sequential(
            nn.Conv2d(in_channels, 16, 3, padding=1), nn.BatchNorm2d(16), nn.ReLU(), nn.MaxPool2d(2),
            nn.Conv2d(16, 16, 3, padding=1, groups=16), nn.Conv2d(16, 32, 1), nn.BatchNorm2d(32), nn.ReLU(), nn.MaxPool2d(2),
            nn.Conv2d(32, 32, 3, padding=1, groups=32), nn.Conv2d(32, 64, 1), nn.BatchNorm2d(64), nn.ReLU(), nn.MaxPool2d(2),
            nn.Conv2d(64, 64, 3, padding=1, groups=64), nn.Conv2d(64, 128, 1), nn.BatchNorm2d(128), nn.ReLU(),
            nn.AdaptiveAvgPool2d((1, 1)))
        self.classifier = nn.Sequential(nn.Flatten(), nn.Linear(128, 64), nn.ReLU(), nn.Dropout(0.3),
                                        nn.Linear(64, num_classes))
        self._n_pools, self._out_channels = 3, 128
        self._init_native(compute_dtype)

    def _describe(self, sd):
        blocks = [("features.0", "features.1", None, 2), ("features.5", "features.6", "features.4", 2),
                  ("features.10", "features.11", "features.9", 2), ("features.15", "features.16", "features.14", 1)]
        return blocks, "classifier.1", "classifier.4", self.features[1].eps


def create_model(model_type: str = "standard", **kwargs) -> nn.Module:
    """Factory with the reference's signature (``src/model.py:296-316``)."""
    models = {"standard": CoughDetector, "small": CoughDetectorSmall, "residual": CoughDetectorResidual}
    if model_type not in models:
        raise ValueError(f"Unknown model type: {model_type}. Choose from {list(models.keys())}")
    return models[model_type](**kwargs)


def count_parameters(model: nn.Module) -> int:
    return sum(p.numel() for p in model.parameters() if p.requires_grad)
