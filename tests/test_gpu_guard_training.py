"""The three training steps and their soft-target twins between guard zones, on poisoned workspaces (``tests/guarded.py``).

These steps have the largest workspace carves in the project.  Every run receives: the image batch, the parameters, the
class weights, the dropout keep mask and (soft step) the target probabilities as inputs held flush against a trailing
guard; the gradients, running statistics, counters, loss, logits and ``d_mask_out`` as guarded outputs, 4-byte aligned (the
int64 counters 8); class-index targets in an ordinary tensor; and a guarded 256-byte aligned workspace of exactly
``cough_train*_workspace_bytes`` under each fill -- zeros, all-ones bits, and what a step of another batch size with a NaN
clip left.  Loss, logits, keep mask, the whole flat gradient buffer, running statistics and counters must be bit-equal
across the fills and bit-equal to the trainer's own step (``forward_backward``), which the parity suites hold to the
float64 restatements.  ``cough_train_std_*`` refuses images below 16 x 16, so its smallest case is (2, 16, 16)."""
import pytest
import torch

import cough_detector_amd as cda
import guarded as G
from cough_detector_amd import _lib
from cough_detector_amd.training import ResidualTrainer, SmallTrainer, StandardTrainer
from guarded import Guarded

pytestmark = pytest.mark.gpu

CW = [1.0, 2.5]
KINDS = {
    "residual": ("residual", ResidualTrainer, [(2, 90, 101), (3, 37, 29)]),
    "small": ("small", SmallTrainer, [(2, 8, 8), (5, 37, 29)]),
    "std": ("standard", StandardTrainer, [(2, 16, 16), (5, 37, 29)]),
}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _trainer(kind, resnet_golden, cnn_golden):
    name, cls, _ = KINDS[kind]
    sd = resnet_golden[0] if kind == "residual" else cnn_golden[name][0]
    m = cda.create_model(name, n_mels=90, num_classes=2, in_channels=1, compute_dtype="fp32")
    m.load_state_dict(sd)
    return cls(m, class_weights=CW, seed=1234)


def _targets(b, soft, g):
    if soft:
        y = torch.rand(b, 2, generator=g)
        return y / y.sum(1, keepdim=True)
    return torch.randint(0, 2, (b,), generator=g)


def _launch(tr, soft, x_ptr, b, hgt, wid, t_ptr, cw_ptr, mask_ptr, offset, params, grads, running, nbt, loss, logits,
            mask_out, ws_ptr, ws_bytes):
    lib, check, fn = ((_lib.load_soft(), _lib.check_soft, tr._soft_fn) if soft else (_lib.load(), _lib.check, tr._fb_fn))
    check(getattr(lib, fn)(x_ptr, b, hgt, wid, t_ptr, cw_ptr, mask_ptr, tr.seed, offset, *tr._dropout_args(), params, grads,
                           running, nbt, tr._momentum, tr._bn_eps, loss, logits, mask_out, ws_ptr, ws_bytes, _stream()), fn)


@pytest.mark.parametrize("soft", [False, True], ids=["class_index", "soft"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_training_step(resnet_golden, cnn_golden, kind, soft):
    tr = _trainer(kind, resnet_golden, cnn_golden)
    ws_bytes = getattr(_lib.load(), tr._ws_fn)
    width = tr._mask_width
    assert (ws_bytes(2, 8, 8) == 0) == (kind == "std")          # the standard net has four pools: nothing below 16 x 16
    for case, (b, hgt, wid) in enumerate(KINDS[kind][2]):
        g = torch.Generator().manual_seed(100 * b + hgt)
        x = torch.randn(b, 1, hgt, wid, generator=g)
        t = _targets(b, soft, g)
        # the first shape with an explicit keep mask, the second with the device's draw (Philox: seed, offset)
        mask = (torch.rand(b, width, generator=g) >= 0.3).float() if case == 0 else None
        before = {k: v.clone() for k, v in (("params", tr._params), ("grads", tr._grads), ("running", tr._running),
                                            ("nbt", tr._nbt))}

        def restore():
            for k, buf in (("params", tr._params), ("grads", tr._grads), ("running", tr._running), ("nbt", tr._nbt)):
                buf.copy_(before[k])

        # the normal path
        offset = tr._draws
        mask_out = torch.empty((b, width), device="cuda")
        loss, logits = tr.forward_backward(x.cuda(), t.cuda(), dropout_mask=None if mask is None else mask.cuda(),
                                           mask_out=mask_out)
        torch.cuda.synchronize()
        want = {"loss": loss.reshape(1).clone(), "logits": logits.clone(), "mask_out": mask_out, "grads": tr._grads.clone(),
                "running": tr._running.clone(), "nbt": tr._nbt.clone()}
        assert torch.equal(tr._params, before["params"]) and bool(torch.isfinite(want["loss"]).all())
        assert bool((want["nbt"] == before["nbt"] + 1).all()) and not torch.equal(want["running"], before["running"])
        if mask is not None:
            assert torch.equal(mask_out.cpu(), mask)
        restore()

        need = ws_bytes(b, hgt, wid)
        nb = b + 1
        other_need = ws_bytes(nb, hgt, wid)
        assert need > 0 and other_need > 0
        other_x = torch.randn(nb, 1, hgt, wid, generator=g)
        other_x[-1, 0, hgt // 2, wid // 3] = float("nan")
        other_x = Guarded.holding(other_x.cuda(), 4)
        other_t = _targets(nb, soft, g).cuda()
        other = {k: v.clone() for k, v in before.items()}
        other_out = torch.empty(1 + nb * 2, device="cuda")

        def stale(ws):
            return G.run_other(ws, other_need, lambda p, n: _launch(
                tr, soft, other_x.ptr, nb, hgt, wid, other_t.data_ptr(), tr.class_weights.data_ptr(), None, 77,
                other["params"].data_ptr(), other["grads"].data_ptr(), other["running"].data_ptr(), other["nbt"].data_ptr(),
                other_out.data_ptr(), other_out[1:].data_ptr(), None, p, n))

        for fill, ws, more in G.workspaces(need, stale):
            ins = {"x": Guarded.holding(x.cuda(), 4, name="d_x"),
                   "params": Guarded.holding(before["params"], 4, name="d_params"),
                   "cw": Guarded.holding(tr.class_weights, 4, name="d_class_weights")}
            if mask is not None:
                ins["mask"] = Guarded.holding(mask.cuda(), 4, name="d_dropout_mask")
            if soft:
                ins["t"] = Guarded.holding(t.cuda(), 4, name="d_soft_targets")
                t_ptr = ins["t"].ptr
            else:
                t_dev = t.cuda()               # class indices stay in an ordinary tensor
                t_ptr = t_dev.data_ptr()
            outs = {k: G.output(want[k].shape, want[k].dtype, name="d_" + k) for k in want}
            outs["running"].float32.copy_(before["running"])       # in / out state
            outs["nbt"].int64.copy_(before["nbt"])
            _launch(tr, soft, ins["x"].ptr, b, hgt, wid, t_ptr, ins["cw"].ptr, ins["mask"].ptr if mask is not None else None,
                    offset, ins["params"].ptr, outs["grads"].ptr, outs["running"].ptr, outs["nbt"].ptr, outs["loss"].ptr,
                    outs["logits"].ptr, outs["mask_out"].ptr, ws.ptr, need)
            torch.cuda.synchronize()
            got = {k: o.view(want[k].dtype).view(want[k].shape) for k, o in outs.items()}
            G.check(list(ins.values()) + list(outs.values()) + [ws] + more, got, want,
                    f"{tr._soft_fn if soft else tr._fb_fn} {(b, hgt, wid)} workspace {fill}")
            assert torch.equal(ins["params"].float32, before["params"])
