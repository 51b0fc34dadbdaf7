"""Generate tests/golden/train_std_step_golden.npz from the reference's own training step of CoughDetector ("standard").

Runs the reference's ``train_epoch`` (src/train.py:54-112) three times, one batch each, on its CoughDetector
(src/model.py:11-141) built from the ``standard.sd.*`` weights of tests/golden/cnn_golden.npz, with the criterion and
optimizer its ``train()`` builds (:420-455): CrossEntropyLoss(weight=[1.0, 2.5]), AdamW(lr, weight_decay=0.01),
clip_grad_norm_(1.0).  B = 8 images of 90x101, float32 on the CPU: step k trains on images 8k .. 8k+7 of
resnet_golden.npz's ``x``, which are not copied here.  The reference package is imported by path, its audio / data
dependencies replaced by import-only stubs (tools/make_train_golden.py).

Recorded: per step k in 0..2 ``y{k}``, ``mask{k}`` (B, 608): the keep masks of the four Dropout2d layers (one per
(clip, channel); 1 where the input plane is all zero, whose gradient is zero either way) and of fc[2], captured by
forward hooks; ``loss{k}``, ``logits{k}``; ``grad1.<name>`` the clipped gradients left by step 0; ``final.<name>`` the
state_dict after step 2; ``adam.exp_avg.<name>``, ``adam.exp_avg_sq.<name>``, ``adam.step``; ``lr``, ``weight_decay``,
``class_weights``, ``p_block``, ``p_fc``.  Every per-parameter tensor keeps the elements of
make_train_golden.golden_index (all of a tensor up to 2047 values, else every (n // 1024)-th).

Usage: python tools/make_train_std_golden.py <reference checkout>   (only where the reference exists)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_train_golden import _StubFinder, sample   # noqa: E402


def main(ref_root: str, out: str) -> None:
    sys.meta_path.insert(0, _StubFinder())
    sys.path.insert(0, ref_root)
    from src import model as rmodel, train as rtrain          # noqa: E402  (the reference, by path)

    torch.manual_seed(0)
    c = np.load(os.path.join(ROOT, "tests", "golden", "cnn_golden.npz"))
    sd = {k[len("standard.sd."):]: torch.from_numpy(c[k]) for k in c.files if k.startswith("standard.sd.")}
    model = rmodel.create_model("standard", n_mels=90, num_classes=2, in_channels=1)
    model.load_state_dict(sd)
    lr, wd, cw = 1e-3, 0.01, torch.tensor([1.0, 2.5])
    criterion = torch.nn.CrossEntropyLoss(weight=cw)
    optimizer = torch.optim.AdamW(model.parameters(), lr=lr, weight_decay=wd)
    rec = {"lr": np.float64(lr), "weight_decay": np.float64(wd), "class_weights": cw.numpy(),
           "p_block": np.float64(model.conv_layers[0].dropout.p), "p_fc": np.float64(model.fc[2].p)}
    cap = {}

    def plane_hook(i):
        def hook(mod, inp, outp):
            x, y = inp[0], outp
            live = x.flatten(2).ne(0).any(dim=2)
            kept = y.flatten(2).ne(0).any(dim=2)
            cap[i] = torch.where(live, kept.to(x.dtype), torch.ones_like(live, dtype=x.dtype)).detach().clone()
        return hook

    def fc_hook(mod, inp, outp):
        x, y = inp[0], outp
        cap[4] = torch.where(x != 0, (y != 0).to(x.dtype), torch.ones_like(x)).detach().clone()

    def out_hook(mod, inp, outp):
        cap["logits"] = outp.detach().clone()

    for i, blk in enumerate(model.conv_layers):
        blk.dropout.register_forward_hook(plane_hook(i))
    model.fc[2].register_forward_hook(fc_hook)
    model.register_forward_hook(out_hook)
    images = torch.from_numpy(np.load(os.path.join(ROOT, "tests", "golden", "resnet_golden.npz"))["x"])
    for step in range(3):
        x = images[8 * step:8 * step + 8].clone()
        y = torch.tensor([0, 1, 1, 0, 1, 0, 0, 1]) if step != 1 else torch.tensor([1, 1, 0, 0, 0, 1, 1, 1])
        res = rtrain.train_epoch(model, [(x, y)], criterion, optimizer, torch.device("cpu"), step)
        rec[f"y{step}"] = y.numpy()
        rec[f"mask{step}"] = torch.cat([cap[i] for i in range(5)], dim=1).numpy()
        rec[f"logits{step}"] = cap["logits"].numpy()
        rec[f"loss{step}"] = np.float64(res["loss"])
        if step == 0:
            for name, p in model.named_parameters():
                rec["grad1." + name] = sample(p.grad)
    for k, v in model.state_dict().items():
        rec["final." + k] = sample(v) if v.dim() else v.detach().numpy().copy()
    st = optimizer.state_dict()["state"]
    for i, (name, _) in enumerate(model.named_parameters()):
        rec["adam.exp_avg." + name] = sample(st[i]["exp_avg"])
        rec["adam.exp_avg_sq." + name] = sample(st[i]["exp_avg_sq"])
    rec["adam.step"] = np.float64(float(st[0]["step"]))
    np.savez_compressed(out, **rec)
    print(f"wrote {out}: losses {[float(rec[f'loss{s}']) for s in range(3)]}")


if __name__ == "__main__":
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("COUGH_REFERENCE", "")
    if not ref or not os.path.isdir(os.path.join(ref, "src")):
        sys.exit("usage: make_train_std_golden.py <reference checkout>")
    main(ref, os.path.join(ROOT, "tests", "golden", "train_std_step_golden.npz"))
