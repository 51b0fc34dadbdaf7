"""Float64 CPU restatement of one training step of CoughDetectorSmall (TEST INFRASTRUCTURE, not product).

The step of the reference's ``train_epoch`` (/root/reference/src/train.py:54-112) on its CoughDetectorSmall
(src/model.py:144-207), written with torch functionals: F.conv2d (the depthwise ones with groups=C),
F.batch_norm(training=True) (batch mean, biased variance; running statistics with the unbiased one), ReLU, max-pool 2,
global average, Linear, ReLU, dropout with an explicit keep mask, Linear; CrossEntropyLoss(weight), autograd,
clip_grad_norm_ and torch.optim.AdamW.
"""
from __future__ import annotations

from typing import Dict, List

import torch
import torch.nn.functional as F

import pool_ties_ref

BNS = ["features.1", "features.6", "features.11", "features.16"]
DWS = ["features.4", "features.9", "features.14"]
PWS = ["features.5", "features.10", "features.15"]
PARAM_NAMES: List[str] = []
for _m in ["features.0", "features.1", "features.4", "features.5", "features.6", "features.9", "features.10",
           "features.11", "features.14", "features.15", "features.16", "classifier.1", "classifier.4"]:
    PARAM_NAMES += [_m + ".weight", _m + ".bias"]
# the conv biases that reach a BatchNorm (the dw ones through the pw conv): true gradient 0, the reference's is rounding
# noise -- bounded, never compared
BN_FED_BIASES = [f"features.{i}.bias" for i in (0, 4, 5, 9, 10, 14, 15)]
RELUS = ["stem", "b1", "b2", "b3", "fc"]      # the five ReLUs, in forward order
HIDDEN = 64


class _Relu(torch.autograd.Function):
    """ReLU whose backward mask is (input > 0) XOR ``flip`` (read when backward runs: see train_ref._Relu)."""

    @staticmethod
    def forward(ctx, v, flip):
        ctx.save_for_backward(v)
        ctx.flip = flip
        return v.clamp_min(0)

    @staticmethod
    def backward(ctx, g):
        v, = ctx.saved_tensors
        return g * ((v > 0) ^ ctx.flip), None


class RefStep:
    """Float64 parameters / BN buffers / an AdamW of a CoughDetectorSmall; ``step`` is one train_epoch iteration.
    ``pre`` / ``flip`` / ``regrad`` as in train_ref.RefStep."""

    def __init__(self, sd: Dict[str, torch.Tensor], lr=1e-3, weight_decay=0.01, betas=(0.9, 0.999), eps=1e-8,
                 max_norm=1.0, class_weights=None, momentum=0.1, bn_eps=1e-5, dtype=torch.float64):
        """``dtype``: float64 for the restatement; float32 gives torch's own f32 arithmetic of the same step."""
        self.dtype = dtype
        self.P = {n: sd[n].detach().to(dtype).clone().requires_grad_(True) for n in PARAM_NAMES}
        self.R = {}
        for b in BNS:
            self.R[b + ".running_mean"] = sd[b + ".running_mean"].detach().to(dtype).clone()
            self.R[b + ".running_var"] = sd[b + ".running_var"].detach().to(dtype).clone()
            self.R[b + ".num_batches_tracked"] = int(sd.get(b + ".num_batches_tracked", torch.tensor(0)))
        self.opt = torch.optim.AdamW([self.P[n] for n in PARAM_NAMES], lr=lr, betas=betas, eps=eps,
                                     weight_decay=weight_decay)
        self.max_norm, self.momentum, self.bn_eps = max_norm, momentum, bn_eps
        self.cw = None if class_weights is None else torch.as_tensor(class_weights, dtype=dtype)

    def _bn(self, z, b):
        self.R[b + ".num_batches_tracked"] += 1
        self.batch_var[b] = (z.shape[0] * z.shape[2] * z.shape[3], z.detach().var(dim=(0, 2, 3), unbiased=False))
        return F.batch_norm(z, self.R[b + ".running_mean"], self.R[b + ".running_var"], self.P[b + ".weight"],
                            self.P[b + ".bias"], training=True, momentum=self.momentum, eps=self.bn_eps)

    def _relu(self, v, name):
        self.pre[name] = v.detach()
        self.flip[name] = torch.zeros(v.shape, dtype=torch.bool)
        return _Relu.apply(v, self.flip[name])

    def forward(self, x, mask, p):
        P = self.P
        self.pre, self.flip, self.batch_var, self.pool_in, self.pick, self.pool_of = {}, {}, {}, {}, {}, {}
        h = F.conv2d(x, P["features.0.weight"], P["features.0.bias"], padding=1)
        h = pool_ties_ref.pool(self, self._relu(self._bn(h, BNS[0]), "stem"), "p0", relu="stem")
        for i in range(3):
            c = h.shape[1]
            h = F.conv2d(h, P[DWS[i] + ".weight"], P[DWS[i] + ".bias"], padding=1, groups=c)
            h = F.conv2d(h, P[PWS[i] + ".weight"], P[PWS[i] + ".bias"])
            h = self._relu(self._bn(h, BNS[i + 1]), f"b{i + 1}")
            if i < 2:
                h = pool_ties_ref.pool(self, h, f"p{i + 1}", relu=f"b{i + 1}")
        g = h.mean(dim=(2, 3))
        hid = self._relu(F.linear(g, P["classifier.1.weight"], P["classifier.1.bias"]), "fc")
        d = hid * (mask.to(self.dtype) * (1.0 / (1.0 - p))) if p < 1 else hid * 0.0
        return F.linear(d, P["classifier.4.weight"], P["classifier.4.bias"])

    def grads(self, x, y, mask, p):
        """Forward + backward: (loss, logits, {name: unclipped grad})."""
        self.opt.zero_grad()
        logits = self.forward(x.to(self.dtype), mask, p)
        loss = F.cross_entropy(logits, y, weight=self.cw)
        loss.backward(retain_graph=True)
        self._loss = loss
        return loss.detach(), logits.detach(), {n: self.P[n].grad.detach().clone() for n in PARAM_NAMES}

    def regrad(self):
        self.opt.zero_grad()
        self._loss.backward(retain_graph=True)
        return {n: self.P[n].grad.detach().clone() for n in PARAM_NAMES}

    def step(self, x, y, mask, p):
        """One train_epoch iteration: (loss, logits, unclipped grads, total norm)."""
        loss, logits, g = self.grads(x, y, mask, p)
        norm = torch.nn.utils.clip_grad_norm_([self.P[n] for n in PARAM_NAMES], max_norm=self.max_norm)
        self.opt.step()
        return loss, logits, g, float(norm)

    def state_dict(self):
        sd = {n: t.detach().clone() for n, t in self.P.items()}
        for k, v in self.R.items():
            sd[k] = torch.tensor(v) if isinstance(v, int) else v.clone()
        return sd


def running_names() -> List[str]:
    return [b + s for b in BNS for s in (".running_mean", ".running_var")]


def _worst(g, rgrads):
    return max((g[n] - rgrads[n]).abs().max().item() / max(rgrads[n].abs().max().item(), 1e-300)
               for n in PARAM_NAMES if n not in BN_FED_BIASES)


def resolve_kinks(g, ref, rgrads, kink=1e-6, limit=64, rtol=1e-4, ties=False):
    """train_ref.resolve_kinks for this network (pool_ties_ref.resolve): ReLU inputs within ``kink`` of 0 are flipped
    one at a time on ``ref`` (after ``grads``) and kept where that brings the restatement closer to ``g``.  With
    ``ties`` the pool windows with a positive maximum whose top two values differ by less than ``kink`` of it are
    candidates too (the runner-up takes the window), in one order of margin with the ReLU inputs; exact ties never are.
    A last pass undoes every kept change that the others made unnecessary.  Returns (gradients, kept changes); the
    gradients are ``rgrads`` itself when the plain comparison is within ``rtol``."""
    return pool_ties_ref.resolve(g, ref, rgrads, _worst, kink=kink, limit=limit, rtol=rtol, ties=ties)


def step_on_the_kernels_side(ref, g, x, y, mask, p, ties=False):
    """``ref.step`` for a check against a float32 step whose unclipped gradients are ``g``: the same train_epoch
    iteration, with the choices that are ambiguous in float32 (ReLU inputs within rounding of 0; with ``ties``,
    near-tied pool windows) taken as that step took them (``resolve_kinks``), as train_std_ref's.  Returns ``step``'s tuple and
    the kept changes."""
    loss, logits, rg = ref.grads(x, y, mask, p)
    rg, kept = resolve_kinks(g, ref, rg, ties=ties)
    for n in PARAM_NAMES:
        ref.P[n].grad = rg[n].clone()
    norm = torch.nn.utils.clip_grad_norm_([ref.P[n] for n in PARAM_NAMES], max_norm=ref.max_norm)
    ref.opt.step()
    return loss, logits, rg, float(norm), kept


def assert_step_matches(model, loss, logits, rloss, rlogits, rgrads, rsd, sd0, loss_on_logit_scale=False,
                        grad_rtol=1e-4) -> float:
    """train_ref.assert_step_matches for CoughDetectorSmall: loss within 1e-5 relative (or, with
    ``loss_on_logit_scale``, within the logits' bound), logits within 1e-5 of max(1, their largest), every gradient
    within ``grad_rtol`` of that tensor's largest reference gradient (the BN-fed conv biases bounded by ``grad_rtol`` of
    their weight's), running statistics rtol 1e-5, num_batches_tracked + 1.  Returns the largest gradient error as a
    fraction of its tensor's scale."""
    import numpy as np
    zscale = max(1.0, rlogits.abs().max().item())
    dl = abs(loss.item() - rloss.item())
    assert dl <= 1e-5 * abs(rloss.item()) or (loss_on_logit_scale and dl <= 1e-5 * zscale), (loss.item(), rloss.item())
    assert (logits.cpu().double() - rlogits).abs().max().item() <= 1e-5 * zscale
    g = {n: p.grad.detach().cpu().double() for n, p in model.named_parameters()}
    worst = 0.0
    for n in PARAM_NAMES:
        if n in BN_FED_BIASES:
            assert g[n].abs().max().item() <= grad_rtol * rgrads[n.replace(".bias", ".weight")].abs().max().item(), n
            continue
        scale = rgrads[n].abs().max().item()
        err = (g[n] - rgrads[n]).abs().max().item()
        assert err <= grad_rtol * scale, (n, err, scale)
        worst = max(worst, err / scale if scale > 0 else 0.0)
    msd = model.state_dict()
    for k in running_names():
        np.testing.assert_allclose(msd[k].cpu().double().numpy(), rsd[k].numpy(), rtol=1e-5, atol=1e-6, err_msg=k)
    for k in [n for n in msd if n.endswith("num_batches_tracked")]:
        assert int(msd[k]) == int(sd0[k]) + 1
    return worst
