"""Training of ``CoughDetectorResidual``, ``CoughDetectorSmall`` and ``CoughDetector`` on the MI355X: one optimisation step as the reference's ``train_epoch`` takes it
(``/root/reference/src/train.py:54-112``, built at :420-455)::

    optimizer.zero_grad(); outputs = model(inputs)            # train mode: batch-statistics BN, Dropout(p)
    loss = CrossEntropyLoss(weight=class_weights)(outputs, targets); loss.backward()
    clip_grad_norm_(model.parameters(), max_norm); AdamW(lr, betas, eps, weight_decay).step()

The forward, backward and optimizer arithmetic runs in ``csrc/train.hip`` (``cough_train_forward_backward``,
``cough_adamw_step``), ``csrc/train_small.hip`` (``cough_train_small_forward_backward``) and ``csrc/train_std.hip``
(``cough_train_std_forward_backward``); torch only allocates memory and supplies the stream.  The trainer makes the module's parameters,
gradients (``p.grad``) and BatchNorm buffers views of flat device buffers that the kernels update in place, so
``model.state_dict()`` holds the trained state after every step and ``model.eval()(x)`` runs the inference kernels on it.
``model.train()(x)`` still refuses: training goes through the trainer.

Targets come in two forms.  ``(B,)`` integer class indices take the entry points above.  ``(B, 2)`` floating class
probabilities -- ``MixUp``'s mixed one-hot labels, smoothed labels, a teacher's probabilities -- take the same steps'
``*_soft`` entry points of ``libcough_amd_soft.so`` (``include/cough_amd_soft.h``): the same kernels with the soft-target
loss of ``F.cross_entropy(outputs, probabilities, weight=class_weights)``, whose mean divides by the batch size B and not
by the sum of the clips' class weights as the class-index loss does.

Non-finite input gives a NaN loss; the step then leaves NaN gradients and parameters (as torch's own step does: the clip
coefficient of a NaN norm does not rescue them).  The residual net trains with its shipped channels ``(32, 64, 128)``
only, the standard net with ``channels=(32, 64, 128, 256)`` and ``fc_hidden=128``; ``create_trainer`` picks the trainer of a
Residual or Small model, and ``StandardTrainer(model)`` trains a ``CoughDetector``.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Iterable, Optional, Sequence

import torch
import torch.nn as nn

from . import _lib
from .model import CoughDetector, CoughDetectorResidual, CoughDetectorSmall

SHIPPED_CHANNELS = (32, 64, 128)
STANDARD_CHANNELS, STANDARD_FC_HIDDEN = (32, 64, 128, 256), 128


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


class HipAdamW(torch.optim.Optimizer):
    """``torch.optim.AdamW`` with the gradient clip of ``train_epoch`` fused in, on ``cough_adamw_step``.

    ``param_groups`` / ``state_dict()`` / ``load_state_dict()`` use ``torch.optim.AdamW``'s layout (per parameter index:
    ``step``, ``exp_avg``, ``exp_avg_sq``), so a state moves between the two and torch LR schedulers drive ``lr``.  One
    parameter group; its ``lr``, ``betas``, ``eps`` and ``weight_decay`` are read on every ``step()``.  The moments are
    views of two flat device buffers laid out like the parameters, and so is every ``p.grad`` (of ``flat_grads``)."""

    def __init__(self, params: Sequence[torch.nn.Parameter], flat_params: torch.Tensor, flat_grads: torch.Tensor,
                 lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.01, max_norm: float = 1.0):
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                        foreach=None, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=True)
        super().__init__(list(params), defaults)
        if len(self.param_groups) != 1:
            raise ValueError("HipAdamW: one parameter group")
        self._flat, self._flat_grads = flat_params, flat_grads
        self._exp_avg = torch.zeros_like(flat_params)
        self._exp_avg_sq = torch.zeros_like(flat_params)
        self._total_norm = torch.zeros(1, dtype=torch.float32, device=flat_params.device)
        self._n_steps = 0
        self.max_norm = float(max_norm)
        self._bind_state()
        self._grad_views = [flat_grads[off:off + n].view_as(p) for p, off, n in self._slices()]
        self.bind_grads()

    def _slices(self):
        off = 0
        for p in self.param_groups[0]["params"]:
            yield p, off, p.numel()
            off += p.numel()

    def _bind_state(self):
        for p, off, n in self._slices():
            self.state[p] = {"step": torch.tensor(float(self._n_steps)),
                             "exp_avg": self._exp_avg[off:off + n].view_as(p),
                             "exp_avg_sq": self._exp_avg_sq[off:off + n].view_as(p)}

    @property
    def total_norm(self) -> torch.Tensor:
        """The gradient norm of the last step (before clipping), a 1-element device tensor."""
        return self._total_norm

    def zero_grad(self, set_to_none: bool = True):
        """Zeroes the flat gradient buffer in place.  ``p.grad`` stays its view whatever ``set_to_none`` says: the kernels
        write the flat buffer, and a ``p.grad`` of ``None`` would hide every later gradient from the caller."""
        with torch.no_grad():
            self._flat_grads.zero_()
        self.bind_grads()

    def bind_grads(self):
        """Make every ``p.grad`` the view of the flat gradient buffer again (``Module.zero_grad()`` sets it to ``None``)."""
        for p, g in zip(self.param_groups[0]["params"], self._grad_views):
            if p.grad is not g:
                p.grad = g

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise ValueError("HipAdamW.step: closures are not supported")
        g = self.param_groups[0]
        beta1, beta2 = g["betas"]
        self._n_steps += 1
        # from the betas as the ABI carries them (C floats): the kernel forms 1 - beta from those, and bias corrections
        # of the double betas would make the step the AdamW of no beta at all (6.4e-6 relative at step 1 for 0.999)
        bc1 = 1.0 - C.c_float(float(beta1)).value ** self._n_steps
        bc2 = 1.0 - C.c_float(float(beta2)).value ** self._n_steps
        dev = self._flat.device
        _lib.check(_lib.load().cough_adamw_step(
            self._flat.data_ptr(), self._flat_grads.data_ptr(), self._exp_avg.data_ptr(), self._exp_avg_sq.data_ptr(),
            self._flat.numel(), float(g["lr"]), float(beta1), float(beta2), float(g["eps"]), float(g["weight_decay"]),
            self.max_norm, bc1, bc2, self._total_norm.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
            "cough_adamw_step")
        return None

    def state_dict(self):
        for p, _, _ in self._slices():
            self.state[p]["step"].fill_(float(self._n_steps))
        return super().state_dict()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        steps = set()
        with torch.no_grad():
            for p, off, n in self._slices():
                st = self.state.get(p, {})
                if "exp_avg" in st:
                    self._exp_avg[off:off + n].copy_(st["exp_avg"].reshape(-1))
                    self._exp_avg_sq[off:off + n].copy_(st["exp_avg_sq"].reshape(-1))
                    steps.add(int(float(st["step"])))
                else:
                    self._exp_avg[off:off + n].zero_()
                    self._exp_avg_sq[off:off + n].zero_()
                    steps.add(0)
        if len(steps) != 1:
            raise ValueError(f"HipAdamW.load_state_dict: parameters at different steps {sorted(steps)}")
        self._n_steps = steps.pop()
        self._bind_state()


class _FlatTrainer:
    """What the HIP trainers share: the module's parameters, gradients and BN buffers become views of flat device
    buffers, a ``HipAdamW`` over them, and one forward / backward entry point of the C-ABI per model.  Subclasses set
    the model class, the layout constants and the entry points, and check the model (``_check``)."""

    _model_cls = None
    _name = ""
    _n_tensors = _n_params = _n_running = _n_bns = _mask_width = 0
    _ws_fn = _fb_fn = _soft_fn = ""         # _soft_fn: the step's entry point for soft targets (libcough_amd_soft.so)

    def __init__(self, model, lr: float = 1e-3, weight_decay: float = 0.01, betas=(0.9, 0.999), eps: float = 1e-8,
                 class_weights=None, max_norm: float = 1.0, seed: int = 0):
        name = self._name
        if not isinstance(model, self._model_cls):
            raise TypeError(f"{name} trains a {self._model_cls.__name__}")
        self._check(model)
        if not torch.cuda.is_available():
            raise RuntimeError("cough_detector_amd needs an AMD GPU (gfx950); there is no CPU fallback")
        if max_norm <= 0:
            raise ValueError(f"{name}: max_norm must be > 0")
        bns = [m for m in model.modules() if isinstance(m, nn.BatchNorm2d)]
        if len(bns) != self._n_bns or any(b.momentum is None or not b.track_running_stats or not b.affine for b in bns):
            raise ValueError(f"{name}: every BatchNorm needs affine=True, track_running_stats=True and a momentum")
        if len({(float(b.momentum), float(b.eps)) for b in bns}) != 1:
            raise ValueError(f"{name}: all BatchNorm layers must share momentum and eps")
        self.model = model
        self.device = torch.device("cuda", torch.cuda.current_device())
        dev = self.device
        model.to(dev)
        params = list(model.parameters())
        n = sum(p.numel() for p in params)
        if len(params) != self._n_tensors or n != self._n_params:
            raise ValueError(f"{name}: {len(params)} parameter tensors / {n} values, expected {self._n_tensors} / "
                             f"{self._n_params}")
        self._params = torch.empty(n, dtype=torch.float32, device=dev)
        self._grads = torch.zeros(n, dtype=torch.float32, device=dev)
        self._running = torch.empty(self._n_running, dtype=torch.float32, device=dev)
        self._nbt = torch.empty(len(bns), dtype=torch.int64, device=dev)
        with torch.no_grad():
            off = 0
            for p in params:
                k = p.numel()
                self._params[off:off + k].copy_(p.detach().reshape(-1))
                p.data = self._params[off:off + k].view_as(p)
                off += k
            off = 0
            for i, bn in enumerate(bns):
                c = bn.num_features
                self._running[off:off + c].copy_(bn.running_mean)
                self._running[off + c:off + 2 * c].copy_(bn.running_var)
                self._nbt[i].copy_(bn.num_batches_tracked)
                bn.running_mean = self._running[off:off + c]
                bn.running_var = self._running[off + c:off + 2 * c]
                bn.num_batches_tracked = self._nbt[i]
                off += 2 * c
        model.invalidate()                   # the parameters and BN buffers are other tensors now
        self._momentum, self._bn_eps = float(bns[0].momentum), float(bns[0].eps)
        self.class_weights = None
        if class_weights is not None:
            cw = torch.as_tensor(class_weights, dtype=torch.float32).to(dev).reshape(-1).contiguous()
            if cw.numel() != 2:
                raise ValueError(f"{name}: class_weights needs one weight per class (2)")
            self.class_weights = cw
        self.optimizer = HipAdamW(params, self._params, self._grads, lr=lr, betas=betas, eps=eps,
                                  weight_decay=weight_decay, max_norm=max_norm)
        self.seed = int(seed) & ((1 << 64) - 1)
        self._draws = 0                      # device dropout draws so far: the Philox counter offset of the next one
        self._shape = None
        self._ws = self._loss = self._logits = None

    def _check(self, model) -> None:
        pass

    def _dropout_p(self) -> float:
        raise NotImplementedError

    def _dropout_args(self) -> tuple:
        """The dropout probabilities the forward / backward entry point takes, in its argument order."""
        return (self._dropout_p(),)

    # ------------------------------------------------------------------ step
    def _prepare(self, inputs: torch.Tensor, targets: torch.Tensor, dropout_mask):
        dev = self.device
        if inputs.dim() != 4 or inputs.shape[1] != 1:
            raise ValueError(f"expected inputs (B, 1, F, T), got {tuple(inputs.shape)}")
        x = inputs.detach().to(device=dev, dtype=torch.float32).contiguous()
        b, _, hgt, wid = x.shape
        t = torch.as_tensor(targets).detach()
        if t.dtype.is_floating_point:
            # class probabilities; a floating (B,) would be truncated to class indices, so it is refused
            if tuple(t.shape) != (b, 2):
                raise ValueError(f"targets: floating targets are class probabilities of shape ({b}, 2), got "
                                 f"{tuple(t.shape)}; class indices are integers of shape ({b},)")
            t = t.to(device=dev, dtype=torch.float32).contiguous()
        elif t.dtype.is_complex:
            raise ValueError(f"targets: {t.dtype} targets")
        else:
            t = t.to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
            if t.numel() != b:
                raise ValueError(f"targets: {t.numel()} values for a batch of {b}")
        mask = None
        if dropout_mask is not None:
            mask = torch.as_tensor(dropout_mask).detach().to(device=dev, dtype=torch.float32).contiguous()
            if tuple(mask.shape) != (b, self._mask_width):
                raise ValueError(f"dropout_mask must be ({b}, {self._mask_width}), got {tuple(mask.shape)}")
        if self._shape != (b, hgt, wid):
            need = getattr(_lib.load(), self._ws_fn)(b, hgt, wid)
            if need == 0:
                raise ValueError(f"{self._name}: a batch of {b} images of {hgt}x{wid} is not trainable (image too "
                                 "small for the network, or a BatchNorm would see one value per channel)")
            self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
            self._loss = torch.empty((), dtype=torch.float32, device=dev)
            self._logits = torch.empty((b, 2), dtype=torch.float32, device=dev)
            self._shape = (b, hgt, wid)
        return x, t, mask

    def forward_backward(self, inputs: torch.Tensor, targets: torch.Tensor, dropout_mask=None, mask_out=None):
        """The forward and backward half of ``step``: writes ``p.grad`` of every parameter (unclipped), the BN running
        statistics and counters; returns ``(loss, logits)``.  ``targets``: ``(B,)`` integer class indices, or ``(B, 2)``
        floating class probabilities (the soft-target step; anything else raises ``ValueError`` before any launch).
        ``mask_out`` (B, mask width) float32 device tensor, optional, receives the keep mask used."""
        x, t, mask = self._prepare(inputs, targets, dropout_mask)
        self.optimizer.bind_grads()          # after a torch-style zero_grad(set_to_none=True) on the module
        b, _, hgt, wid = x.shape
        ps = self._dropout_args()
        offset = self._draws
        if mask is None:
            self._draws += 1
        dev = self.device
        soft = t.dtype == torch.float32
        lib, check, fn = ((_lib.load_soft(), _lib.check_soft, self._soft_fn) if soft
                          else (_lib.load(), _lib.check, self._fb_fn))
        check(getattr(lib, fn)(
            x.data_ptr(), b, hgt, wid, t.data_ptr(), _ptr(self.class_weights), _ptr(mask), self.seed, offset, *ps,
            self._params.data_ptr(), self._grads.data_ptr(), self._running.data_ptr(), self._nbt.data_ptr(),
            self._momentum, self._bn_eps, self._loss.data_ptr(), self._logits.data_ptr(), _ptr(mask_out),
            self._ws.data_ptr(), self._ws.numel(), torch.cuda.current_stream(dev).cuda_stream),
            fn)
        # the kernels wrote the parameters / buffers behind torch's back (no _version bump): drop the inference handles
        # so the next eval-mode call re-reads them
        self.model.invalidate()
        return self._loss, self._logits

    def step(self, inputs: torch.Tensor, targets: torch.Tensor, dropout_mask=None):
        loss, logits = self.forward_backward(inputs, targets, dropout_mask)
        self.optimizer.step()
        self.model.invalidate()
        return loss, logits


class ResidualTrainer(_FlatTrainer):
    """Trains a ``CoughDetectorResidual`` (``channels=(32, 64, 128)``) with the reference's ``train_epoch`` step.

    ``step(inputs, targets, dropout_mask=None) -> (loss, logits)``: ``inputs`` (B, 1, F, T) float32, ``targets`` (B,)
    int64 class indices; ``dropout_mask`` (B, 128) of 0 / 1 keeps, or ``None`` for the device generator (Philox keyed by
    ``seed``, one new draw per step).  ``loss`` is a 0-d device tensor, ``logits`` the train-mode outputs; both are
    buffers of the trainer, overwritten by the next step at the same shape (read them, e.g. ``loss.item()``, first).
    No host synchronisation; no allocation after the first step at a given (B, F, T).

    Soft targets: ``targets`` (B, 2) floating class probabilities (cast to float32) run ``cough_train_forward_backward_soft``.
    Per clip ``l_b = -(w0 y_b0 lp_b0 + w1 y_b1 lp_b1)`` with ``lp = log_softmax(outputs)`` and ``w`` the class weights
    (1 without), and ``loss = sum(l_b) / B``: the mean over the batch, NOT over the summed class weights as with class
    indices, so with class weights a one-hot soft batch's loss is the class-index loss times ``sum(w_y) / B``.  Rows need
    not sum to 1, an all-zero row contributes nothing, values are not validated (no synchronisation) and a NaN in a row
    gives a NaN loss.  Without class weights, one-hot rows give the class-index step bit for bit."""

    _model_cls = CoughDetectorResidual
    _name = "ResidualTrainer"
    _n_tensors, _n_params, _n_running, _n_bns, _mask_width = 30, _lib.TRAIN_NUM_PARAMS, _lib.TRAIN_NUM_RUNNING, 7, 128
    _ws_fn, _fb_fn = "cough_train_workspace_bytes", "cough_train_forward_backward"
    _soft_fn = "cough_train_forward_backward_soft"

    def _check(self, model) -> None:
        if tuple(model.channels) != SHIPPED_CHANNELS:
            raise ValueError(f"ResidualTrainer: channels={tuple(model.channels)}; the training kernels are built for "
                             f"{SHIPPED_CHANNELS}")

    def _dropout_p(self) -> float:
        return float(self.model.fc[1].p)


class SmallTrainer(_FlatTrainer):
    """Trains a ``CoughDetectorSmall`` with the reference's ``train_epoch`` step (``csrc/train_small.hip``,
    ``cough_train_small_forward_backward``): the contract of ``ResidualTrainer``, with the dropout keep mask of the
    hidden layer (``classifier[3]``) ``(B, 64)``.  Trainable shapes: F, T >= 8 and B * (F // 8) * (T // 8) > 1.
    Soft targets (B, 2) floating run ``cough_train_small_forward_backward_soft`` under ``ResidualTrainer``'s soft contract:
    the loss is the sum of the clips' terms over B, not over the summed class weights."""

    _model_cls = CoughDetectorSmall
    _name = "SmallTrainer"
    _n_tensors, _n_params, _n_running, _n_bns, _mask_width = (26, _lib.TRAIN_SMALL_NUM_PARAMS,
                                                              _lib.TRAIN_SMALL_NUM_RUNNING, 4, 64)
    _ws_fn, _fb_fn = "cough_train_small_workspace_bytes", "cough_train_small_forward_backward"
    _soft_fn = "cough_train_small_forward_backward_soft"

    def _dropout_p(self) -> float:
        return float(self.model.classifier[3].p)


class StandardTrainer(_FlatTrainer):
    """Trains a ``CoughDetector`` ("standard": ``channels=(32, 64, 128, 256)``, ``fc_hidden=128``) with the reference's
    ``train_epoch`` step (``csrc/train_std.hip``, ``cough_train_std_forward_backward``): the contract of
    ``SmallTrainer``, with the dropout keep mask ``(B, 608)``: one Dropout2d keep per (clip, channel) of the four
    ConvBlocks (32 + 64 + 128 + 256 columns, in block order), then the 128 hidden units of ``fc[2]``.  The blocks'
    Dropout2d layers share one p, the head has its own.  Trainable shapes: F >= 16 and T >= 16.
    Soft targets (B, 2) floating run ``cough_train_std_forward_backward_soft`` under ``ResidualTrainer``'s soft contract:
    the loss is the sum of the clips' terms over B, not over the summed class weights."""

    _model_cls = CoughDetector
    _name = "StandardTrainer"
    _n_tensors, _n_params, _n_running, _n_bns, _mask_width = (20, _lib.TRAIN_STD_NUM_PARAMS, _lib.TRAIN_STD_NUM_RUNNING,
                                                              4, 608)
    _ws_fn, _fb_fn = "cough_train_std_workspace_bytes", "cough_train_std_forward_backward"
    _soft_fn = "cough_train_std_forward_backward_soft"

    def _check(self, model) -> None:
        chans = tuple(int(b.conv.out_channels) for b in model.conv_layers)
        if chans != STANDARD_CHANNELS:
            raise ValueError(f"StandardTrainer: channels={chans}; the training kernels are built for {STANDARD_CHANNELS}")
        if int(model.fc[0].out_features) != STANDARD_FC_HIDDEN:
            raise ValueError(f"StandardTrainer: fc_hidden={model.fc[0].out_features}; the training kernels are built for "
                             f"{STANDARD_FC_HIDDEN}")
        if len({float(b.dropout.p) for b in model.conv_layers}) != 1:
            raise ValueError("StandardTrainer: the ConvBlocks' Dropout2d layers must share one p")

    def _dropout_args(self) -> tuple:
        return float(self.model.conv_layers[0].dropout.p), float(self.model.fc[2].p)


def create_trainer(model, **kwargs):
    """The HIP trainer of ``model``: ``ResidualTrainer`` for a ``CoughDetectorResidual``, ``SmallTrainer`` for a
    ``CoughDetectorSmall`` (keyword arguments as theirs).  A ``CoughDetector`` ("standard") is trained by constructing
    ``StandardTrainer(model)``; this function does not route to it yet."""
    if isinstance(model, CoughDetectorResidual):
        return ResidualTrainer(model, **kwargs)
    if isinstance(model, CoughDetectorSmall):
        return SmallTrainer(model, **kwargs)
    if isinstance(model, CoughDetector):
        raise TypeError("CoughDetector ('standard') is not trainable yet through create_trainer: construct "
                        "StandardTrainer(model)")
    raise TypeError(f"no HIP trainer for {type(model).__name__}")


def soft_class(targets: torch.Tensor) -> torch.Tensor:
    """The class index of (B, 2) soft targets: ``targets.argmax(1)`` by torch's first-of-equals rule (a tie is class 0),
    computed where the targets live."""
    return (targets[:, 1] > targets[:, 0]).to(torch.int64)


def train_epoch(trainer: _FlatTrainer, train_loader: Iterable, epoch: int) -> Dict[str, float]:
    """The reference's ``train_epoch`` (``src/train.py:54-112``) on a ``ResidualTrainer``, a ``SmallTrainer``
    (``create_trainer``) or a ``StandardTrainer``: ``{'loss', 'accuracy'}``, the mean batch loss and the percentage of train-mode predictions equal to the target.
    The target of a soft (B, 2) floating row is its ``argmax(1)``: the first of equal values, so a tie counts as class 0."""
    trainer.model.train()
    running_loss, correct, total, n_batches = 0.0, 0, 0, 0
    for inputs, targets in train_loader:
        loss, outputs = trainer.step(inputs, targets)
        running_loss += loss.item()
        predicted = outputs.argmax(1)
        total += int(targets.shape[0])
        t = torch.as_tensor(targets).to(outputs.device)
        if t.dim() == 2 and t.dtype.is_floating_point:
            t = soft_class(t)
        correct += int(predicted.eq(t).sum().item())
        n_batches += 1
    return {"loss": running_loss / max(n_batches, 1), "accuracy": 100.0 * correct / max(total, 1)}
