"""Training step without a GPU: the float64 restatement (tests/train_ref.py) against the reference's own three steps
(tests/golden/train_step_golden.npz, tools/make_train_golden.py), the argument checks of the new entry points, and the
optimizer state layout shared with torch.optim.AdamW."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

from cough_detector_amd import _lib
from cough_detector_amd.training import HipAdamW
from train_ref import BN_FED_BIASES, PARAM_NAMES, RefStep, golden_sample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_train_golden():
    """(golden, initial state_dict): the golden as a dict plus the inputs ``x{s}`` of step s (images 8s .. 8s+7 of
    resnet_golden.npz, as tools/make_train_golden.py used them); per-parameter tensors hold train_ref.golden_index."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "train_step_golden.npz"))
    g = {k: z[k] for k in z.files}
    r = np.load(os.path.join(ROOT, "tests", "golden", "resnet_golden.npz"))
    for s in range(3):
        g[f"x{s}"] = np.ascontiguousarray(r["x"][8 * s:8 * s + 8])
    init = {k[3:]: torch.from_numpy(r[k]) for k in r.files if k.startswith("sd.")}
    return g, init


def test_restatement_reproduces_the_reference_steps():
    g, init = load_train_golden()
    ref = RefStep(init, lr=float(g["lr"]), weight_decay=float(g["weight_decay"]), class_weights=g["class_weights"])
    p = float(g["p"])
    for s in range(3):
        x, y, mask = torch.from_numpy(g[f"x{s}"]), torch.from_numpy(g[f"y{s}"]), torch.from_numpy(g[f"mask{s}"])
        loss, logits, grads, _ = ref.step(x, y, mask, p)
        # the golden is float32 arithmetic: ~1e-7 relative per operation over a few thousand-term sums at step 0; from
        # step 1 on the parameters themselves differ (float32 AdamW updates of near-zero gradients), 1.4e-5 measured
        tol = 1e-5 if s == 0 else 1e-4
        assert abs(loss.item() - float(g[f"loss{s}"])) <= tol * abs(float(g[f"loss{s}"]))
        np.testing.assert_allclose(logits.numpy(), g[f"logits{s}"], rtol=0, atol=10 * tol * np.abs(g[f"logits{s}"]).max())
        if s == 0:
            for n in PARAM_NAMES:
                got, want = golden_sample(ref.P[n].grad), g["grad1." + n]
                if n in BN_FED_BIASES:
                    assert np.abs(got).max() <= 1e-9 and np.abs(want).max() <= 1e-4
                    continue
                assert np.abs(got - want).max() <= 1e-4 * np.abs(want).max(), n
    sd = ref.state_dict()
    lr = float(g["lr"])
    for n in PARAM_NAMES:
        got, want = golden_sample(sd[n]), g["final." + n]
        if n in BN_FED_BIASES:
            # three AdamW steps of at most lr each (plus decay) on noise: both sides stay within 3 lr of the start
            assert np.abs(got - want).max() <= 6 * lr + 1e-6, n
            continue
        # |m / sqrt(v)| <= 1 per step for a steady gradient sign; parameters whose gradient is tiny against the f32
        # noise can flip it -- allow 2 lr per step over three steps for those, and check the bulk at 1e-5
        d = np.abs(got - want)
        assert d.max() <= 6 * lr, n
        assert np.median(d) <= 1e-5, n
    for b in ["conv1.1"] + [f"res_blocks.{i}.{c}" for i in range(2) for c in ("bn1", "bn2", "skip.1")]:
        # the batch means include the conv bias, which drifts by up to 2 lr per step on noise (above): momentum 0.1 x
        # 3 steps x 2 lr bounds what reaches running_mean; the variance does not see the bias
        np.testing.assert_allclose(sd[f"{b}.running_mean"].numpy(), g[f"final.{b}.running_mean"], rtol=0, atol=0.1 * 6 * lr)
        np.testing.assert_allclose(sd[f"{b}.running_var"].numpy(), g[f"final.{b}.running_var"], rtol=1e-4, atol=1e-6)
        assert int(sd[f"{b}.num_batches_tracked"]) == int(g[f"final.{b}.num_batches_tracked"])


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    lib = _lib.load()
    assert lib.cough_train_workspace_bytes(8, 90, 101) % 256 == 0 and lib.cough_train_workspace_bytes(8, 90, 101) > 0
    assert lib.cough_train_workspace_bytes(0, 90, 101) == 0
    assert lib.cough_train_workspace_bytes(8, 2, 101) == 0                  # too small for the network
    fake = 1 << 20
    wsb = lib.cough_train_workspace_bytes(8, 90, 101)

    def fb(x=fake, n=8, h=90, w=101, targets=fake, p=0.5, params=fake, grads=fake, running=fake, nbt=fake, mom=0.1,
           eps=1e-5, loss=fake, logits=fake, ws=1 << 24, ws_bytes=wsb):
        return lib.cough_train_forward_backward(x, n, h, w, targets, None, None, 0, 0, p, params, grads, running, nbt, mom,
                                                eps, loss, logits, None, ws, ws_bytes, None)

    E = _lib.EINVAL
    for kw in ("x", "targets", "params", "grads", "running", "nbt", "loss", "logits", "ws"):
        assert fb(**{kw: None}) == E, kw
        assert b"NULL" in lib.cough_amd_last_error()
    assert fb(n=0) == E and fb(n=-1) == E and fb(h=0) == E and fb(w=-3) == E
    assert fb(h=2) == E and b"too small" in lib.cough_amd_last_error()
    assert fb(n=1, h=8, w=8) == E and b"one value" in lib.cough_amd_last_error()   # 1x1 last block, batch of 1
    assert fb(p=1.5) == E and fb(p=-0.1) == E and fb(p=float("nan")) == E
    assert fb(mom=float("nan")) == E and fb(eps=-1.0) == E
    assert fb(ws=(1 << 24) + 8) == E
    assert fb(ws_bytes=wsb - 1) == _lib.EWORKSPACE

    def adam(p=fake, g=fake, m=fake, v=fake, n=100, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.01, mx=1.0, bc1=0.1,
             bc2=0.001, norm=fake):
        return lib.cough_adamw_step(p, g, m, v, n, lr, b1, b2, eps, wd, mx, bc1, bc2, norm, None)

    for kw in ("p", "g", "m", "v", "norm"):
        assert adam(**{kw: None}) == E, kw
    assert adam(n=0) == E and adam(lr=-1.0) == E and adam(b1=1.0) == E and adam(b2=-0.5) == E
    assert adam(mx=0.0) == E and adam(bc1=0.0) == E and adam(bc2=1.5) == E and adam(eps=float("inf")) == E
    with pytest.raises(ValueError, match="cough_adamw_step"):
        _lib.check(adam(n=0), "cough_adamw_step")


def test_optimizer_state_round_trips_through_torch_adamw():
    torch.manual_seed(0)
    shapes = [(4, 3), (5,), (2, 2, 3)]
    n = sum(int(np.prod(s)) for s in shapes)
    flat = torch.randn(n, dtype=torch.float32)
    params, off = [], 0
    for s in shapes:
        k = int(np.prod(s))
        params.append(torch.nn.Parameter(flat[off:off + k].view(s)))
        off += k
    opt = HipAdamW(params, flat, torch.zeros(n), lr=3e-4, betas=(0.8, 0.99), eps=1e-7, weight_decay=0.05)
    opt._exp_avg.copy_(torch.randn(n))
    opt._exp_avg_sq.copy_(torch.rand(n))
    opt._n_steps = 7
    sd = copy.deepcopy(opt.state_dict())
    assert set(sd["state"]) == {0, 1, 2} and all(set(v) == {"step", "exp_avg", "exp_avg_sq"} for v in sd["state"].values())
    assert float(sd["state"][1]["step"]) == 7.0 and sd["state"][2]["exp_avg"].shape == (2, 2, 3)
    tparams = [torch.nn.Parameter(p.detach().clone()) for p in params]
    topt = torch.optim.AdamW(tparams, lr=1.0)
    topt.load_state_dict(sd)
    assert topt.param_groups[0]["lr"] == 3e-4 and topt.param_groups[0]["betas"] == (0.8, 0.99)
    back = copy.deepcopy(topt.state_dict())
    flat2 = torch.zeros(n)
    params2 = [torch.nn.Parameter(flat2[o:o + int(np.prod(s))].view(s))
               for o, s in zip(np.cumsum([0] + [int(np.prod(s)) for s in shapes])[:-1], shapes)]
    opt2 = HipAdamW(params2, flat2, torch.zeros(n))
    opt2.load_state_dict(back)
    assert opt2._n_steps == 7 and opt2.param_groups[0]["weight_decay"] == 0.05
    assert torch.equal(opt2._exp_avg, opt._exp_avg) and torch.equal(opt2._exp_avg_sq, opt._exp_avg_sq)
    # the state entries stay views of the flat moments
    assert opt2.state[params2[1]]["exp_avg"].data_ptr() == opt2._exp_avg.data_ptr() + 12 * 4
    sched = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(opt2, T_0=10, T_mult=2, eta_min=1e-6)
    assert opt2.param_groups[0]["lr"] == opt2.param_groups[0]["initial_lr"]
    del sched


def test_training_exports():
    import cough_detector_amd as cda
    assert cda.ResidualTrainer is not None and callable(cda.train_epoch)
    for s in ("cough_train_workspace_bytes", "cough_train_forward_backward", "cough_adamw_step"):
        assert s in _lib.SYMBOLS


def test_trainable_shapes_are_the_ones_torch_accepts(resnet_golden):
    """cough_train_workspace_bytes / cough_train_forward_backward refuse exactly the (B, H, W) on which the reference's
    train-mode forward raises (an image too small for the pools, or a BatchNorm with one value per channel).  Only
    shapes that must be refused reach cough_train_forward_backward (fake pointers: an accepted call would launch)."""
    lib = _lib.load()
    sd, _ = resnet_golden
    ref = RefStep(sd)
    fake = 1 << 20
    seen = set()
    for b in (1, 2, 3):
        for h in range(1, 13):
            for w in range(1, 13):
                x = torch.zeros(b, 1, h, w)
                try:
                    with torch.no_grad():
                        ref.forward(x.double(), torch.ones(b, 128), 0.5)
                    torch_ok = True
                except (RuntimeError, ValueError):          # max_pool2d: RuntimeError, batch_norm: ValueError
                    torch_ok = False
                wsb = lib.cough_train_workspace_bytes(b, h, w)
                seen.add((torch_ok, wsb > 0))
                if torch_ok:
                    assert wsb > 0, (b, h, w)
                elif wsb > 0:
                    rc = lib.cough_train_forward_backward(fake, b, h, w, fake, None, None, 0, 0, 0.5, fake, fake, fake,
                                                          fake, 0.1, 1e-5, fake, fake, None, 1 << 24, wsb, None)
                    assert rc == _lib.EINVAL, (b, h, w)
    assert seen == {(True, True), (False, False), (False, True)}       # all three outcomes occur in this range


@pytest.mark.parametrize("set_to_none", [True, False])
def test_zero_grad_keeps_p_grad_a_view_of_the_flat_buffer(set_to_none):
    shapes = [(4, 3), (5,), (2, 2, 3)]
    n = sum(int(np.prod(s)) for s in shapes)
    flat, grads = torch.randn(n), torch.randn(n)
    params, off = [], 0
    for s in shapes:
        k = int(np.prod(s))
        params.append(torch.nn.Parameter(flat[off:off + k].view(s)))
        off += k
    opt = HipAdamW(params, flat, grads)
    for p in params:
        assert p.grad is not None and p.grad.untyped_storage().data_ptr() == grads.untyped_storage().data_ptr()
    opt.zero_grad(set_to_none=set_to_none)
    assert torch.count_nonzero(grads) == 0
    grads.fill_(2.0)
    for p in params:
        assert p.grad is not None and torch.equal(p.grad, torch.full(p.shape, 2.0))
    # Module.zero_grad(set_to_none=True) drops p.grad; the next forward_backward re-binds it (bind_grads)
    torch.nn.ParameterList(params).zero_grad()
    assert all(p.grad is None for p in params)
    opt.bind_grads()
    assert all(p.grad is not None and p.grad.data_ptr() == grads.data_ptr() + 4 * o
               for p, o in zip(params, np.cumsum([0] + [int(np.prod(s)) for s in shapes])[:-1]))
