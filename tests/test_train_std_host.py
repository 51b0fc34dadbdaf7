"""CoughDetector ("standard") training without a GPU: the float64 restatement (tests/train_std_ref.py) against the
reference's own three steps (tests/golden/train_std_step_golden.npz, tools/make_train_std_golden.py), the argument
checks and trainable shapes of the new entry points, the exported symbols, the optimizer state layout, StandardTrainer's
refusals and create_trainer."""
import copy
import os
import re

import numpy as np
import pytest
import torch

import cough_detector_amd as cda
from cough_detector_amd import _lib
from cough_detector_amd.training import HipAdamW, StandardTrainer, create_trainer
from train_std_ref import BN_FED_BIASES, BNS, MASK_WIDTH, PARAM_NAMES, RefStep, golden_sample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def std_sd():
    """the CoughDetector state of cnn_golden.npz (``standard.sd.*``)"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "cnn_golden.npz"))
    return {k[len("standard.sd."):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("standard.sd.")}


def load_std_golden():
    """(golden, initial state_dict): the golden as a dict plus the inputs ``x{s}`` of step s (images 8s .. 8s+7 of
    resnet_golden.npz, as tools/make_train_std_golden.py used them)."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "train_std_step_golden.npz"))
    g = {k: z[k] for k in z.files}
    r = np.load(os.path.join(ROOT, "tests", "golden", "resnet_golden.npz"))
    for s in range(3):
        g[f"x{s}"] = np.ascontiguousarray(r["x"][8 * s:8 * s + 8])
    return g, std_sd()


def golden_grad_rtol(name):
    """How close a gradient of the golden's step 0 is to the exact one, as a fraction of its tensor's largest value.
    The golden is the reference's float32 CPU step; conv 0's weight gradient is a sum over the 72,720 pixels of the batch
    of terms that cancel (dz leaves a BatchNorm), as for the Small net (test_train_small_host.golden_grad_rtol): 1e-3
    there, 1e-4 elsewhere."""
    return 1e-3 if name == "conv_layers.0.conv.weight" else 1e-4


def test_restatement_reproduces_the_reference_steps():
    g, init = load_std_golden()
    ref = RefStep(init, lr=float(g["lr"]), weight_decay=float(g["weight_decay"]), class_weights=g["class_weights"])
    pb, pf = float(g["p_block"]), float(g["p_fc"])
    for s in range(3):
        x, y, mask = torch.from_numpy(g[f"x{s}"]), torch.from_numpy(g[f"y{s}"]), torch.from_numpy(g[f"mask{s}"])
        assert tuple(mask.shape) == (8, MASK_WIDTH)
        loss, logits, grads, _ = ref.step(x, y, mask, pb, pf)
        # the golden is float32 arithmetic with logits in the hundreds: the loss and logits agree on that scale
        zscale = np.abs(g[f"logits{s}"]).max()
        tol = 1e-5 if s == 0 else 1e-4
        assert abs(loss.item() - float(g[f"loss{s}"])) <= tol * zscale
        np.testing.assert_allclose(logits.numpy(), g[f"logits{s}"], rtol=0, atol=tol * zscale)
        if s == 0:
            # p.grad of the golden is clipped (clip_grad_norm_ writes it back): compare directions, then the norm
            norm = float(torch.sqrt(sum((grads[n] ** 2).sum() for n in PARAM_NAMES)))
            coef = min(1.0 / (norm + 1e-6), 1.0)
            for n in PARAM_NAMES:
                got, want = golden_sample(grads[n]) * coef, g["grad1." + n]
                if n in BN_FED_BIASES:
                    # rounding noise of a sum that cancels exactly: bounded by the weight's rule
                    w = n.replace(".bias", ".weight")
                    assert np.abs(got).max() <= 1e-9 and np.abs(want).max() <= golden_grad_rtol(w) * np.abs(g["grad1." + w]).max()
                    continue
                assert np.abs(got - want).max() <= golden_grad_rtol(n) * np.abs(want).max(), n
    sd = ref.state_dict()
    lr = float(g["lr"])
    for n in PARAM_NAMES:
        d = np.abs(golden_sample(sd[n]) - g["final." + n])
        assert d.max() <= 6 * lr, n
        if n not in BN_FED_BIASES:
            assert np.median(d) <= 1e-5, n
    for b in BNS:
        np.testing.assert_allclose(sd[f"{b}.running_mean"].numpy(), g[f"final.{b}.running_mean"], rtol=1e-4,
                                   atol=0.1 * 6 * lr)
        np.testing.assert_allclose(sd[f"{b}.running_var"].numpy(), g[f"final.{b}.running_var"], rtol=1e-4, atol=1e-6)
        assert int(sd[f"{b}.num_batches_tracked"]) == int(g[f"final.{b}.num_batches_tracked"])


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    lib = _lib.load()
    wsb = lib.cough_train_std_workspace_bytes(8, 90, 101)
    assert wsb > 0 and wsb % 256 == 0
    assert lib.cough_train_std_workspace_bytes(0, 90, 101) == 0
    assert lib.cough_train_std_workspace_bytes(-1, 90, 101) == 0
    assert lib.cough_train_std_workspace_bytes(8, 15, 101) == 0
    assert lib.cough_train_std_workspace_bytes(8, 90, -5) == 0
    assert lib.cough_train_std_workspace_bytes(1, 16, 16) > 0
    fake = 1 << 20

    def fb(x=fake, n=8, h=90, w=101, targets=fake, pb=0.1, pf=0.5, params=fake, grads=fake, running=fake, nbt=fake,
           mom=0.1, eps=1e-5, loss=fake, logits=fake, ws=1 << 24, ws_bytes=wsb):
        return lib.cough_train_std_forward_backward(x, n, h, w, targets, None, None, 0, 0, pb, pf, params, grads,
                                                    running, nbt, mom, eps, loss, logits, None, ws, ws_bytes, None)

    E = _lib.EINVAL
    for kw in ("x", "targets", "params", "grads", "running", "nbt", "loss", "logits", "ws"):
        assert fb(**{kw: None}) == E, kw
        assert b"NULL" in lib.cough_amd_last_error()
    assert fb(n=0) == E and fb(n=-1) == E and fb(h=0) == E and fb(w=-3) == E
    assert fb(h=15) == E and b"too small" in lib.cough_amd_last_error()
    assert fb(w=15) == E and b"too small" in lib.cough_amd_last_error()
    for bad in (1.5, -0.1, float("nan")):
        assert fb(pb=bad) == E and fb(pf=bad) == E
    assert fb(mom=float("nan")) == E and fb(mom=2.0) == E and fb(eps=-1.0) == E
    assert fb(ws=(1 << 24) + 8) == E
    assert fb(ws_bytes=wsb - 1) == _lib.EWORKSPACE
    with pytest.raises(ValueError, match="cough_train_std_forward_backward"):
        _lib.check(fb(n=0), "cough_train_std_forward_backward")


def _torch_trainable(ref, b, h, w):
    x = torch.zeros(b, 1, h, w)
    try:
        with torch.no_grad():
            ref.forward(x.double(), torch.ones(b, MASK_WIDTH), 0.1, 0.5)
        return True
    except (RuntimeError, ValueError):                  # max_pool2d: RuntimeError, batch_norm: ValueError
        return False


def test_trainable_shapes_are_the_ones_torch_accepts():
    """cough_train_std_workspace_bytes accepts exactly the (B, H, W) on which the train-mode forward runs in torch, and
    cough_train_std_forward_backward refuses the others (fake pointers: an accepted call would launch)."""
    lib = _lib.load()
    ref = RefStep(std_sd())
    fake = 1 << 20
    seen = set()
    for b in (1, 2, 3):
        for h in range(1, 21):
            for w in range(1, 21):
                ok = _torch_trainable(ref, b, h, w)
                wsb = lib.cough_train_std_workspace_bytes(b, h, w)
                seen.add(ok)
                assert (wsb > 0) == ok, (b, h, w)
                assert ok == (h >= 16 and w >= 16)
                if not ok:
                    rc = lib.cough_train_std_forward_backward(fake, b, h, w, fake, None, None, 0, 0, 0.1, 0.5, fake,
                                                              fake, fake, fake, 0.1, 1e-5, fake, fake, None, 1 << 24,
                                                              1 << 40, None)
                    assert rc == _lib.EINVAL, (b, h, w)
    assert seen == {True, False}


def test_symbols_are_exported_and_the_counts_match_the_header():
    header = open(os.path.join(ROOT, "include", "cough_amd.h")).read()
    for s in ("cough_train_std_workspace_bytes", "cough_train_std_forward_backward"):
        assert s in _lib.SYMBOLS and s + "(" in header
        assert hasattr(_lib.load(), s)
    np_ = int(re.search(r"#define COUGH_TRAIN_STD_NUM_PARAMS (\d+)", header).group(1))
    nr = int(re.search(r"#define COUGH_TRAIN_STD_NUM_RUNNING (\d+)", header).group(1))
    assert (np_, nr) == (_lib.TRAIN_STD_NUM_PARAMS, _lib.TRAIN_STD_NUM_RUNNING) == (421954, 960)
    m = cda.create_model("standard", n_mels=90)
    params = list(m.parameters())
    assert len(params) == 20 and sum(p.numel() for p in params) == np_
    assert [n for n, _ in m.named_parameters()] == PARAM_NAMES
    assert sum(b.numel() for n, b in m.named_buffers() if not n.endswith("num_batches_tracked")) == nr
    assert cda.StandardTrainer is StandardTrainer and "StandardTrainer" in cda.__all__
    n_decl = int(re.search(r"exactly the (\d+) entry points declared in this header", header).group(1))
    assert n_decl == len(_lib.SYMBOLS) == 53


def test_optimizer_state_round_trips_through_torch_adamw():
    """HipAdamW over the standard model's parameter shapes: the state moves to torch.optim.AdamW and back."""
    torch.manual_seed(0)
    shapes = [tuple(p.shape) for p in cda.create_model("standard", n_mels=90).parameters()]
    n = sum(int(np.prod(s)) for s in shapes)
    assert n == _lib.TRAIN_STD_NUM_PARAMS

    def params_of(flat):
        out, off = [], 0
        for s in shapes:
            k = int(np.prod(s))
            out.append(torch.nn.Parameter(flat[off:off + k].view(s)))
            off += k
        return out

    flat = torch.randn(n)
    opt = HipAdamW(params_of(flat), flat, torch.zeros(n), lr=3e-4, betas=(0.8, 0.99), eps=1e-7, weight_decay=0.05)
    opt._exp_avg.copy_(torch.randn(n))
    opt._exp_avg_sq.copy_(torch.rand(n))
    opt._n_steps = 7
    sd = copy.deepcopy(opt.state_dict())
    assert set(sd["state"]) == set(range(20))
    tparams = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
    topt = torch.optim.AdamW(tparams, lr=1.0)
    topt.load_state_dict(sd)
    back = copy.deepcopy(topt.state_dict())
    flat2 = torch.zeros(n)
    opt2 = HipAdamW(params_of(flat2), flat2, torch.zeros(n))
    opt2.load_state_dict(back)
    assert opt2._n_steps == 7 and opt2.param_groups[0]["lr"] == 3e-4 and opt2.param_groups[0]["weight_decay"] == 0.05
    assert torch.equal(opt2._exp_avg, opt._exp_avg) and torch.equal(opt2._exp_avg_sq, opt._exp_avg_sq)


def test_standard_trainer_refusals_and_create_trainer():
    with pytest.raises(TypeError, match="not trainable yet"):
        create_trainer(cda.create_model("standard", n_mels=90))
    with pytest.raises(TypeError, match="StandardTrainer"):
        create_trainer(cda.create_model("standard", n_mels=90))
    with pytest.raises(TypeError, match="CoughDetector"):
        StandardTrainer(cda.create_model("small", n_mels=90))
    with pytest.raises(ValueError, match="channels"):
        StandardTrainer(cda.create_model("standard", n_mels=90, channels=(32, 64, 128)))
    with pytest.raises(ValueError, match="channels"):
        StandardTrainer(cda.create_model("standard", n_mels=90, channels=(16, 32, 64, 128)))
    with pytest.raises(ValueError, match="fc_hidden"):
        StandardTrainer(cda.create_model("standard", n_mels=90, fc_hidden=64))
    m = cda.create_model("standard", n_mels=90)
    m.conv_layers[2].dropout.p = 0.2
    with pytest.raises(ValueError, match="Dropout2d"):
        StandardTrainer(m)
    gpu = torch.cuda.is_available()
    # the head's own p may differ from the blocks' (the reference's defaults: 0.1 and 0.5); the BatchNorm refusals come
    # after the GPU check (as the other trainers')
    m = cda.create_model("standard", n_mels=90)
    m.conv_layers[1].bn.eps = 1e-3
    with pytest.raises(ValueError if gpu else RuntimeError, match="share momentum and eps" if gpu else "GPU"):
        StandardTrainer(m)
    if not gpu:
        with pytest.raises(RuntimeError, match="GPU"):
            StandardTrainer(cda.create_model("standard", n_mels=90, dropout=0.3))
