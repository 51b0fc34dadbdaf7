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


class RefStep:
    """Holds float64 parameters / BN buffers / an AdamW; ``step`` is one train_epoch iteration."""

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
        return F.batch_norm(z, self.R[b + ".running_mean"], self.R[b + ".running_var"], self.P[b + ".weight"],
                            self.P[b + ".bias"], training=True, momentum=self.momentum, eps=self.bn_eps)

    def forward(self, x, mask, p):
        P = self.P
        h = F.conv2d(x, P["conv1.0.weight"], P["conv1.0.bias"], stride=2, padding=3)
        h = F.max_pool2d(F.relu(self._bn(h, "conv1.1")), 2)
        for i in range(2):
            q = f"res_blocks.{i}."
            o = F.relu(self._bn(F.conv2d(h, P[q + "conv1.weight"], P[q + "conv1.bias"], stride=2, padding=1), q + "bn1"))
            o = self._bn(F.conv2d(o, P[q + "conv2.weight"], P[q + "conv2.bias"], padding=1), q + "bn2")
            idn = self._bn(F.conv2d(h, P[q + "skip.0.weight"], P[q + "skip.0.bias"], stride=2), q + "skip.1")
            h = F.relu(o + idn)
        g = h.mean(dim=(2, 3))
        d = g * (mask.to(torch.float64) * (1.0 / (1.0 - p))) if p < 1 else g * 0.0
        return F.linear(d, P["fc.2.weight"], P["fc.2.bias"])

    def grads(self, x, y, mask, p):
        """Forward + backward: (loss, logits, {name: unclipped grad})."""
        self.opt.zero_grad()
        logits = self.forward(x.to(torch.float64), mask, p)
        loss = F.cross_entropy(logits, y, weight=self.cw)
        loss.backward()
        return loss.detach(), logits.detach(), {n: self.P[n].grad.detach().clone() for n in PARAM_NAMES}

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
