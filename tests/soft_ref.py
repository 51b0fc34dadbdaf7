"""Restatements of the soft-target contract (include/cough_amd_soft.h) in numpy / torch float64: the loss and dlogits of
``F.cross_entropy(z, y, weight=w)`` for class-probability targets ``y`` (B, 2), ``cough_mix_batch``, the accuracy rule of
soft targets, and the target rows the GPU tests train on.  tests/test_soft_host.py checks the loss and dlogits against
``F.cross_entropy`` and autograd on the CPU: that is the link to torch's semantics."""
import numpy as np
import torch


def soft_loss_and_dlogits(z, y, w=None):
    """(loss, dlogits (B, 2), per-clip terms (B,)) in float64.  l_b = -(w0 y_b0 lp_b0 + w1 y_b1 lp_b1) with
    lp = log_softmax(z_b); loss = sum(l_b) / B (the batch size, not the summed weights); dz_bc = (softmax_bc S_b -
    w_c y_bc) / B with S_b = w0 y_b0 + w1 y_b1."""
    z = np.asarray(z, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    w = np.ones(2) if w is None else np.asarray(w, dtype=np.float64)
    b = z.shape[0]
    mx = z.max(axis=1, keepdims=True)
    lse = mx + np.log(np.exp(z - mx).sum(axis=1, keepdims=True))
    lp = z - lse
    wy = w[None, :] * y
    terms = -(wy * lp).sum(axis=1)
    s = wy.sum(axis=1, keepdims=True)
    return terms.sum() / b, (np.exp(lp) * s - wy) / b, terms


def hard_loss(z, t, w=None):
    """The class-index loss of the same logits: sum(w_t (lse - z_t)) / sum(w_t), float64."""
    z = np.asarray(z, dtype=np.float64)
    t = np.asarray(t, dtype=np.int64)
    w = np.ones(2) if w is None else np.asarray(w, dtype=np.float64)
    mx = z.max(axis=1)
    lse = mx + np.log(np.exp(z - mx[:, None]).sum(axis=1))
    wt = w[t]
    return (wt * (lse - z[np.arange(len(t)), t])).sum() / wt.sum()


def onehot(labels, dtype=np.float32):
    """(B, 2) one-hot rows; a label outside {0, 1} has the all-zero row (the kernel's rule)."""
    labels = np.asarray(labels).reshape(-1)
    return np.stack([labels == 0, labels == 1], axis=1).astype(dtype)


def mix_batch(x, labels, perm, coef):
    """``cough_mix_batch`` in float32 numpy, one IEEE operation per operator (numpy has no fused multiply-add):
    out[b] = a_b x[b] + c_b x[perm[b]], soft[b] = a_b onehot(y[b]) + c_b onehot(y[perm[b]]); a ``perm`` entry outside
    0..B-1 leaves the row as it is.  ``coef`` (B, 2) float32 (a, c)."""
    x = np.asarray(x, dtype=np.float32)
    b = x.shape[0]
    flat = x.reshape(b, -1)
    oh = onehot(labels)
    coef = np.asarray(coef, dtype=np.float32).reshape(b, 2)
    out, soft = np.empty_like(flat), np.empty((b, 2), dtype=np.float32)
    for r in range(b):
        p = int(perm[r])
        if 0 <= p < b:
            out[r] = coef[r, 0] * flat[r] + coef[r, 1] * flat[p]
            soft[r] = coef[r, 0] * oh[r] + coef[r, 1] * oh[p]
        else:
            out[r], soft[r] = flat[r], oh[r]
    return out.reshape(x.shape), soft


def soft_class(y):
    """The class a soft row counts as: ``argmax(1)`` by torch's first-of-equals rule, so a tie is class 0."""
    y = np.asarray(y)
    return (y[:, 1] > y[:, 0]).astype(np.int64)


def accuracy(logits, y):
    """Percentage of rows whose prediction (first of the largest logits) equals ``soft_class(y)``."""
    z = np.asarray(logits)
    pred = (z[:, 1] > z[:, 0]).astype(np.int64)
    return 100.0 * float((pred == soft_class(y)).sum()) / len(pred)


ROW_KINDS = ("mixture", "onehot1", "zeros", "onehot0", "tie", "unnormalised")


def target_rows(b, seed):
    """(B, 2) float32 soft targets for the step tests, row r of kind ROW_KINDS[r % 6]: a lam-mixture of the two one-hots
    with lam ~ Beta(0.2, 0.2) (formed as MixUp forms it: lam and 1 - lam in float64, then float32), exact one-hots of
    both classes, (0.5, 0.5), an all-zero row and the unnormalised (0.3, 0.3).  A batch of 6 or more holds every kind;
    no batch is all zeros."""
    rng = np.random.RandomState(seed)
    rows = np.zeros((b, 2), dtype=np.float32)
    for r in range(b):
        kind = ROW_KINDS[r % len(ROW_KINDS)]
        lam = rng.beta(0.2, 0.2)
        if kind == "mixture":
            pair = np.array([lam, 1.0 - lam]).astype(np.float32)
            rows[r] = pair if r % 12 < 6 else pair[::-1]
        elif kind == "onehot1":
            rows[r] = (0.0, 1.0)
        elif kind == "onehot0":
            rows[r] = (1.0, 0.0)
        elif kind == "tie":
            rows[r] = (0.5, 0.5)
        elif kind == "unnormalised":
            rows[r] = (0.3, 0.3)
    return torch.from_numpy(rows)
