"""Generate tests/golden/train_step_golden.npz from the reference's own training step.

Runs the reference's ``train_epoch`` (src/train.py:54-112) three times, one batch each, on its CoughDetectorResidual
(src/model.py:210-293) built from the weights of tests/golden/resnet_golden.npz, with the criterion and optimizer its
``train()`` builds (:420-455): CrossEntropyLoss(weight=[1.0, 2.5]), AdamW(lr, weight_decay=0.01), clip_grad_norm_(1.0).
B = 8 images of 90x101, float32 on the CPU: step k trains on images 8k .. 8k+7 of resnet_golden.npz's ``x`` (feature
images of the reference's featuriser, at the scale the golden weights were calibrated for), which are not copied here.  The reference package is imported by path; its
audio / data dependencies are replaced by import-only stubs (nothing of them runs in a training step).

Recorded: per step k in 0..2 ``y{k}``, ``mask{k}`` (the dropout keep mask of fc[1], captured by a forward hook),
``loss{k}``, ``logits{k}``; ``grad1.<name>`` the clipped gradients left by step 0 (``p.grad`` after the step);
``final.<name>`` the state_dict after step 2 (parameters, BN buffers);
``adam.exp_avg.<name>``, ``adam.exp_avg_sq.<name>``, ``adam.step``; ``lr``, ``weight_decay``, ``class_weights``, ``p``.
Per-parameter tensors (grad1, final parameters, AdamW moments) keep the elements ``golden_index(numel)`` of their
flattened values -- every element of a tensor of up to 2047 values, otherwise every (numel // 1024)-th -- which keeps the
file small; BN buffers are stored whole.

Usage: python tools/make_train_golden.py <reference checkout>   (only where the reference exists)
"""
import importlib.abc
import importlib.machinery
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUBS = ("torchaudio", "pandas", "sklearn", "soundfile", "librosa")


class _Stub(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Stub(f"{self.__name__}.{name}")

    def __call__(self, *a, **k):
        return _Stub(self.__name__ + "()")


class _StubFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def find_spec(self, name, path, target=None):
        if name.split(".")[0] in STUBS:
            return importlib.machinery.ModuleSpec(name, self, is_package=True)
        return None

    def create_module(self, spec):
        m = _Stub(spec.name)
        m.__path__ = []
        return m

    def exec_module(self, module):
        pass


def golden_index(n: int) -> np.ndarray:
    """The flattened elements a per-parameter tensor of n values keeps (tests/train_ref.py has the same rule)."""
    return np.arange(0, n, max(1, n // 1024))


def sample(t: torch.Tensor) -> np.ndarray:
    a = t.detach().numpy().reshape(-1)
    return a[golden_index(a.size)].copy()


def main(ref_root: str, out: str) -> None:
    sys.meta_path.insert(0, _StubFinder())
    sys.path.insert(0, ref_root)
    from src import model as rmodel, train as rtrain          # noqa: E402  (the reference, by path)

    torch.manual_seed(0)
    g = np.load(os.path.join(ROOT, "tests", "golden", "resnet_golden.npz"))
    sd = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd.")}
    model = rmodel.create_model("residual", n_mels=90, num_classes=2, in_channels=1)
    model.load_state_dict(sd)
    lr, wd, cw = 1e-3, 0.01, torch.tensor([1.0, 2.5])
    criterion = torch.nn.CrossEntropyLoss(weight=cw)
    optimizer = torch.optim.AdamW(model.parameters(), lr=lr, weight_decay=wd)
    rec = {"lr": np.float64(lr), "weight_decay": np.float64(wd), "class_weights": cw.numpy(),
           "p": np.float64(model.fc[1].p)}
    cap = {}

    def mask_hook(mod, inp, outp):
        x, y = inp[0], outp
        cap["mask"] = torch.where(x != 0, (y != 0).to(x.dtype), torch.ones_like(x)).detach().clone()

    def out_hook(mod, inp, outp):
        cap["logits"] = outp.detach().clone()

    model.fc[1].register_forward_hook(mask_hook)
    model.register_forward_hook(out_hook)
    images = torch.from_numpy(g["x"])
    for step in range(3):
        x = images[8 * step:8 * step + 8].clone()
        y = torch.tensor([0, 1, 1, 0, 1, 0, 0, 1]) if step != 1 else torch.tensor([1, 1, 0, 0, 0, 1, 1, 1])
        res = rtrain.train_epoch(model, [(x, y)], criterion, optimizer, torch.device("cpu"), step)
        rec[f"y{step}"] = y.numpy()
        rec[f"mask{step}"] = cap["mask"].numpy()
        rec[f"logits{step}"] = cap["logits"].numpy()
        rec[f"loss{step}"] = np.float64(res["loss"])
        if step == 0:
            for name, p in model.named_parameters():
                rec["grad1." + name] = sample(p.grad)
    params = dict(model.named_parameters())
    for k, v in model.state_dict().items():
        rec["final." + k] = sample(v) if k in params else v.numpy().copy()
    st = optimizer.state_dict()["state"]
    names = [n for n, _ in model.named_parameters()]
    for i, name in enumerate(names):
        rec["adam.exp_avg." + name] = sample(st[i]["exp_avg"])
        rec["adam.exp_avg_sq." + name] = sample(st[i]["exp_avg_sq"])
    rec["adam.step"] = np.float64(float(st[0]["step"]))
    np.savez_compressed(out, **rec)
    print(f"wrote {out}: losses {[float(rec[f'loss{s}']) for s in range(3)]}")


if __name__ == "__main__":
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("COUGH_REFERENCE", "")
    if not ref or not os.path.isdir(os.path.join(ref, "src")):
        sys.exit("usage: make_train_golden.py <reference checkout>")
    main(ref, os.path.join(ROOT, "tests", "golden", "train_step_golden.npz"))
