"""Float64 CPU restatement of one training step of CoughDetectorResidual (TEST INFRASTRUCTURE, not product).

The step of the reference's ``train_epoch`` (/root/reference/src/train.py:54-112) written with torch functionals:
F.conv2d, F.batch_norm(training=True) (batch mean, biased variance; running statistics with the unbiased one),
ReLU, max-pool 2, the residual blocks of src/model.py:268-293, global average, dropout with an explicit keep mask,
Linear; CrossEntropyLoss(weight), autograd, clip_grad_norm_ and torch.optim.AdamW.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch
import torch.nn.functional as F

CONVS = ["conv1.0"] + [f"res_blocks.{i}.{c}" for i in range(2) for c in ("conv1", "conv2", "skip.0")]
BNS = ["conv1.1"] + [f"res_blocks.{i}.{c}" for i in range(2) for c in ("bn1", "bn2", "skip.1")]
PARAM_NAMES: List[str] = []
for _c, _b in zip(CONVS, BNS):
    PARAM_NAMES += [_c + ".weight", _c + ".bias", _b + ".weight", _b + ".bias"]
PARAM_NAMES += ["fc.2.weight", "fc.2.bias"]
# the order of model.parameters(): the stem conv/BN, then per block conv1, bn1, conv2, bn2, skip.0, skip.1, then fc
PARAM_NAMES = (PARAM_NAMES[:4] + [n for i in range(2) for n in PARAM_NAMES[4 + 12 * i:16 + 12 * i]] + PARAM_NAMES[-2:])
# the conv biases that feed a BatchNorm: true gradient 0, the reference's is rounding noise that AdamW turns into
# updates of up to lr per step -- bounded, never compared
BN_FED_BIASES = ["conv1.0.bias"] + [f"res_blocks.{i}.{c}.bias" for i in range(2) for c in ("conv1", "conv2", "skip.0")]


RELUS = ["stem", "b0.h", "b0.out", "b1.h", "b1.out"]      # the five ReLUs, in forward order


class _Relu(torch.autograd.Function):
    """ReLU whose backward mask is (input > 0) XOR ``flip``: ``flip`` is read when backward runs, so a caller may
    change it in place and run backward again on the retained graph (RefStep.regrad)."""

    @staticmethod
    def forward(ctx, v, flip):
        ctx.save_for_backward(v)
        ctx.flip = flip                  # not saved: changed in place between backward runs
        return v.clamp_min(0)

    @staticmethod
    def backward(ctx, g):
        v, = ctx.saved_tensors
        return g * ((v > 0) ^ ctx.flip), None


class RefStep:
    """Holds float64 parameters / BN buffers / an AdamW; ``step`` is one train_epoch iteration.

    After ``grads``, ``pre[name]`` holds the input of ReLU ``name`` (RELUS) and ``flip[name]`` a boolean mask of the
    same shape, all False: setting elements and calling ``regrad()`` gives the gradient with those ReLU derivatives
    taken from the other side of the kink (the forward pass does not change)."""

    def __init__(self, sd: Dict[str, torch.Tensor], lr=1e-3, weight_decay=0.01, betas=(0.9, 0.999), eps=1e-8,
                 max_norm=1.0, class_weights=None, momentum=0.1, bn_eps=1e-5):
        self.P = {n: sd[n].detach().to(torch.float64).clone().requires_grad_(True) for n in PARAM_NAMES}
        self.R = {}
        for b in BNS:
            self.R[b + ".running_mean"] = sd[b + ".running_mean"].detach().to(torch.float64).clone()
            self.R[b + ".running_var"] = sd[b + ".running_var"].detach().to(torch.float64).clone()
            self.R[b + ".num_batches_tracked"] = int(sd.get(b + ".num_batches_tracked", torch.tensor(0)))
        self.opt = torch.optim.AdamW([self.P[n] for n in PARAM_NAMES], lr=lr, betas=betas, eps=eps,
                                     weight_decay=weight_decay)
        self.max_norm, self.momentum, self.bn_eps = max_norm, momentum, bn_eps
        self.cw = None if class_weights is None else torch.as_tensor(class_weights, dtype=torch.float64)

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
        self.pre, self.flip, self.batch_var = {}, {}, {}
        h = F.conv2d(x, P["conv1.0.weight"], P["conv1.0.bias"], stride=2, padding=3)
        h = F.max_pool2d(self._relu(self._bn(h, "conv1.1"), "stem"), 2)
        for i in range(2):
            q = f"res_blocks.{i}."
            o = self._relu(self._bn(F.conv2d(h, P[q + "conv1.weight"], P[q + "conv1.bias"], stride=2, padding=1), q + "bn1"),
                           f"b{i}.h")
            o = self._bn(F.conv2d(o, P[q + "conv2.weight"], P[q + "conv2.bias"], padding=1), q + "bn2")
            idn = self._bn(F.conv2d(h, P[q + "skip.0.weight"], P[q + "skip.0.bias"], stride=2), q + "skip.1")
            h = self._relu(o + idn, f"b{i}.out")
        g = h.mean(dim=(2, 3))
        d = g * (mask.to(torch.float64) * (1.0 / (1.0 - p))) if p < 1 else g * 0.0
        return F.linear(d, P["fc.2.weight"], P["fc.2.bias"])

    def grads(self, x, y, mask, p):
        """Forward + backward: (loss, logits, {name: unclipped grad})."""
        self.opt.zero_grad()
        logits = self.forward(x.to(torch.float64), mask, p)
        loss = F.cross_entropy(logits, y, weight=self.cw)
        loss.backward(retain_graph=True)
        self._loss = loss
        return loss.detach(), logits.detach(), {n: self.P[n].grad.detach().clone() for n in PARAM_NAMES}

    def regrad(self):
        """The gradients of the last ``grads`` again, with the ReLU derivatives ``flip`` now selects."""
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


def golden_index(n: int):
    """The flattened elements of a per-parameter tensor of n values that train_step_golden.npz keeps
    (tools/make_train_golden.py): all of them up to 2047 values, otherwise every (n // 1024)-th."""
    import numpy as np
    return np.arange(0, n, max(1, n // 1024))


def golden_sample(t):
    """``t`` (torch tensor or array) reduced to the elements the golden keeps, as a numpy array."""
    import numpy as np
    a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    a = a.reshape(-1)
    return a[golden_index(a.size)]


def running_names() -> List[str]:
    return [b + s for b in BNS for s in (".running_mean", ".running_var")]


def _worst(g, rgrads):
    return max((g[n] - rgrads[n]).abs().max().item() / max(rgrads[n].abs().max().item(), 1e-300)
               for n in PARAM_NAMES if n not in BN_FED_BIASES)


def resolve_kinks(g, ref, rgrads, kink=1e-6, limit=64, rtol=1e-4):
    """The restatement's gradients with ReLU derivatives taken from the side the f32 step took, where that is ambiguous.

    A ReLU input within f32 rounding of 0 (|v| < ``kink``; BatchNorm-normalised, so O(1) in scale) may fall on the other
    side of 0 in the f32 step: the forward pass does not notice, but that element's gradient is passed in one run and
    blocked in the other, and everything upstream moves by a full term (measured: 1e-2 .. 5e-2 of a block's weight
    gradient scale from one element at 1.0e-7).  Such inputs (at most ``limit``, closest to 0 first) are flipped one at
    a time on ``ref`` (RefStep after ``grads``) and kept where that brings the reference closer to ``g``; the search
    stops once every gradient is within ``rtol`` of its scale (the 1e-4 rule).  Returns (gradients, [(relu, index, input value)] kept)."""
    if _worst(g, rgrads) <= rtol:
        return rgrads, []
    cand = []
    for name, v in ref.pre.items():
        for idx in (v.abs() < kink).nonzero().tolist():
            cand.append((abs(v[tuple(idx)].item()), name, tuple(idx)))
    cand.sort()
    kept, best = [], _worst(g, rgrads)
    for a, name, idx in cand[:limit]:
        ref.flip[name][idx] = True
        trial = ref.regrad()
        w = _worst(g, trial)
        if w < best:
            best, rgrads = w, trial
            kept.append((name, idx, ref.pre[name][idx].item()))
            if best <= rtol:
                break
        else:
            ref.flip[name][idx] = False
    return rgrads, kept


def step_on_the_kernels_side(ref, g, x, y, mask, p):
    """``ref.step`` for a check against a float32 step whose unclipped gradients are ``g``: the same train_epoch
    iteration, with the ReLU derivatives that are ambiguous in float32 taken as that step took them (``resolve_kinks``,
    the rule of every single-step check here).  Without it a ReLU input within rounding of 0 moves a whole block's
    gradients by 1e-2 of their scale, and with them the clip norm and every moment.  Returns ``step``'s tuple and the
    kept flips."""
    loss, logits, rg = ref.grads(x, y, mask, p)
    rg, kept = resolve_kinks(g, ref, rg)
    for n in PARAM_NAMES:
        ref.P[n].grad = rg[n].clone()
    norm = torch.nn.utils.clip_grad_norm_([ref.P[n] for n in PARAM_NAMES], max_norm=ref.max_norm)
    ref.opt.step()
    return loss, logits, rg, float(norm), kept


def assert_step_matches(model, loss, logits, rloss, rlogits, rgrads, rsd, sd0, loss_on_logit_scale=False,
                        grad_rtol=1e-4) -> float:
    """One HIP forward/backward (``model``'s ``p.grad`` and BN buffers after the step, its ``loss`` / ``logits``) against
    the float64 restatement's (``rloss``, ``rlogits``, ``rgrads``, ``rsd`` = ``RefStep.state_dict()``) from the state
    ``sd0``: loss within 1e-5 relative, logits within 1e-5 of max(1, their largest), every gradient within 1e-4 of that
    tensor's largest reference gradient (the BN-fed conv biases bounded by 1e-4 of their weight's), running statistics
    rtol 1e-5, num_batches_tracked + 1.  ``loss_on_logit_scale``: the loss also passes within the logits' bound;
    ``grad_rtol``: a wider gradient rule for ill-conditioned BatchNorms (both explained in test_gpu_train_shapes.py).  Returns the largest gradient error as a fraction of its tensor's scale."""
    import numpy as np
    zscale = max(1.0, rlogits.abs().max().item())
    dl = abs(loss.item() - rloss.item())
    assert dl <= 1e-5 * abs(rloss.item()) or (loss_on_logit_scale and dl <= 1e-5 * zscale), (loss.item(), rloss.item())
    assert (logits.cpu().double() - rlogits).abs().max().item() <= 1e-5 * zscale
    g = {n: p.grad.detach().cpu().double() for n, p in model.named_parameters()}
    worst = 0.0
    for n in PARAM_NAMES:
        if n in BN_FED_BIASES:
            # a sum of dz over B*H*W pixels that cancels exactly: f32 rounding far below the weight gradient's scale
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
