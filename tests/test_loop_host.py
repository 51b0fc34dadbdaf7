"""The epoch loop without a GPU: the companion library's symbols and argument checks, EarlyStopping and the class-weight
rule against the restatement (tests/loop_ref.py), and the checkpoint schema."""
import os
import re
import shutil
import subprocess
import types

import pytest
import torch

import cough_detector_amd as cda
import loop_ref
from cough_detector_amd import _lib
from cough_detector_amd import build as cbuild
from cough_detector_amd import loop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cough_amd_loop.h")


def _declared():
    return set(re.findall(r"\b(cough_[a-z_0-9]+)\s*\(", open(HEADER).read()))


def test_companion_library_exports_exactly_its_header():
    declared = _declared()
    assert declared == set(_lib.LOOP_SYMBOLS), declared ^ set(_lib.LOOP_SYMBOLS)
    lib = _lib.load_loop()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.cough_loop_abi_version() == 1
    assert "#define COUGH_LOOP_ABI_VERSION 1" in open(HEADER).read()
    # binutils' nm, or the llvm-nm that ships next to hipcc
    nm = shutil.which("nm") or os.path.join(os.path.dirname(os.path.realpath(cbuild._hipcc())), "..", "lib", "llvm", "bin", "llvm-nm")
    out = subprocess.run([nm, "-D", "--defined-only", _lib.LOOP_LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert exported == declared, sorted(exported ^ declared)


def test_the_main_library_is_untouched_by_the_companion():
    assert not set(_lib.LOOP_SYMBOLS) & set(_lib.SYMBOLS)
    assert len(_lib.SYMBOLS) == 53 and _lib.load().cough_amd_abi_version() == 5
    main_header = open(os.path.join(ROOT, "include", "cough_amd.h")).read()
    for s in _lib.LOOP_SYMBOLS:
        assert s not in main_header


def test_meter_update_refuses_bad_arguments_without_a_gpu():
    lib = _lib.load_loop()
    fake = 1 << 20

    def upd(logits=fake, targets=fake, n=32, cw=None, loss=None, meter=fake, preds=None):
        return lib.cough_epoch_meter_update(logits, targets, n, cw, loss, meter, preds, None)

    E = _lib.EINVAL
    for kw in ("logits", "targets", "meter"):
        assert upd(**{kw: None}) == E, kw
        assert b"NULL" in lib.cough_loop_last_error() and b"cough_epoch_meter_update" in lib.cough_loop_last_error()
    assert upd(n=0) == E and b"n_clips" in lib.cough_loop_last_error()
    assert upd(n=-1) == E and b"n_clips" in lib.cough_loop_last_error()
    assert upd(n=-2 ** 31) == E
    for kw in ("logits", "cw", "loss"):
        assert upd(**{kw: fake + 2}) == E and b"4-byte" in lib.cough_loop_last_error(), kw
    for kw in ("targets", "meter", "preds"):
        assert upd(**{kw: fake + 4}) == E and b"8-byte" in lib.cough_loop_last_error(), kw
    with pytest.raises(ValueError, match="cough_epoch_meter_update: .*n_clips"):
        _lib.check_loop(upd(n=0), "cough_epoch_meter_update")
    # the two libraries keep their messages apart
    assert b"n_clips" not in _lib.load().cough_amd_last_error()


def test_the_package_exports_the_loop():
    for name in ("EpochMeter", "EarlyStopping", "train_epoch_async", "validate", "save_checkpoint", "load_checkpoint",
                 "class_weights_from_counts", "fit"):
        assert name in cda.__all__ and getattr(cda, name) is getattr(loop, name), name


SEQUENCES = [
    ([1.0, 0.9, 0.8, 0.7, 0.6], 3, 0.001),
    ([1.0, 1.0, 1.0, 1.0, 1.0], 3, 0.001),
    ([1.0, 0.9995, 0.9991, 0.5, 0.6, 0.7, 0.8], 3, 0.001),
    ([1.0, 0.75, 0.5, 0.5001, 0.25], 2, 0.25),               # 0.75 == best - min_delta: an improvement, not a miss
    ([1.0, 0.7500001, 0.75, 0.5], 2, 0.25),                   # a hair above the edge misses
    ([0.5, 0.6, 0.4, 0.41], 1, 0.001),                        # patience 1: the first miss stops
    ([0.5, 0.4, 0.3, 0.31, 0.1, 0.2], 1, 0.0),                # the flag stays set after a later improvement
    ([2.0, float("nan"), 1.0, 3.0, 3.0], 2, 0.001),
    ([0.3], 1, 0.001),
]


@pytest.mark.parametrize("losses,patience,min_delta", SEQUENCES)
def test_early_stopping_follows_the_restatement(losses, patience, min_delta):
    got, want = cda.EarlyStopping(patience=patience, min_delta=min_delta), loop_ref.EarlyStopping(patience, min_delta)
    assert (got.counter, got.best_loss, got.early_stop) == (0, None, False)
    for i, v in enumerate(losses):
        fg, fw = got(v), want(v)
        assert fg is fw, (i, v)
        assert got.counter == want.counter, (i, v)
        same = got.best_loss == want.best_loss or (got.best_loss != got.best_loss and want.best_loss != want.best_loss)
        assert same, (i, v, got.best_loss, want.best_loss)
        assert got.early_stop is fg


def test_early_stopping_edges_by_hand():
    es = cda.EarlyStopping(patience=2, min_delta=0.25)
    assert [es(v) for v in (1.0, 0.75)] == [False, False] and es.best_loss == 0.75 and es.counter == 0
    assert es(0.75) is False and es.counter == 1 and es.best_loss == 0.75
    assert es(0.6) is True and es.counter == 2
    one = cda.EarlyStopping(patience=1)
    assert one(1.0) is False and one(1.0) is True
    d = cda.EarlyStopping()
    assert (d.patience, d.min_delta) == (10, 0.001)


@pytest.mark.parametrize("counts,want", [
    ({0: 500, 1: 500}, (1.0, 1.0)),
    ({0: 500, 1: 100}, (0.6, 3.0)),
    ({0: 10000, 1: 100}, (0.505, 10.1)),                       # 1 : 100 -> 50.5 capped at 20 x 0.505
    ({0: 40}, (41 / 80, 20 * 41 / 80)),                        # a missing class counts as 1: 20.5, capped
    ({1: 7}, (4.0, 8 / 14)),
    ({0: 100, 1: 0}, (0.5, 10.0)),                             # a present class with no clip: total 100, divisor 1, capped
])
def test_class_weights_from_counts(counts, want):
    w = cda.class_weights_from_counts(counts)
    assert isinstance(w, torch.Tensor) and w.dtype == torch.float32 and tuple(w.shape) == (2,)
    ref = loop_ref.class_weights(counts)
    assert ref == pytest.approx(want, rel=1e-12)
    assert w.tolist() == torch.tensor(list(ref)).tolist()
    assert w[1] / w[0] <= 20.0 * (1 + 1e-6)


def test_class_weights_cap_and_sequence_input():
    assert cda.class_weights_from_counts([500, 100]).tolist() == cda.class_weights_from_counts({0: 500, 1: 100}).tolist()
    w = cda.class_weights_from_counts({0: 10000, 1: 100}, max_ratio=5.0)
    assert w.tolist() == torch.tensor([0.505, 0.505 * 5.0]).tolist()
    assert cda.class_weights_from_counts({0: 10000, 1: 100}, max_ratio=1000.0).tolist() == torch.tensor([0.505, 50.5]).tolist()


def _small():
    torch.manual_seed(3)
    return cda.create_model("small", n_mels=90)


def _stepped_adamw(model):
    opt = torch.optim.AdamW(model.parameters(), lr=2e-3, weight_decay=0.05)
    for p in model.parameters():
        p.grad = torch.full_like(p, 0.01)
    opt.step()
    return opt


def test_checkpoint_schema_and_round_trip(tmp_path):
    model = _small()
    opt = _stepped_adamw(model)
    metrics = {"loss": 0.4, "f1": 0.8, "tp": 4}
    config = {"model_type": "small", "n_mels": 64}
    path = str(tmp_path / "ck.pt")
    cda.save_checkpoint(model, opt, 7, metrics, path, config)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert set(ck) == loop_ref.CHECKPOINT_KEYS == set(loop.CHECKPOINT_KEYS)
    assert ck["epoch"] == 7 and ck["metrics"] == metrics and ck["config"] == config
    assert set(ck["model_state_dict"]) == set(model.state_dict())
    assert set(ck["optimizer_state_dict"]) == {"state", "param_groups"}

    fake_trainer = types.SimpleNamespace(seed=1234, _draws=17)
    cda.save_checkpoint(model, opt, 8, metrics, path, config, trainer=fake_trainer)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert set(ck) == loop_ref.CHECKPOINT_KEYS | {"trainer_state"}
    assert ck["trainer_state"] == {"seed": 1234, "draws": 17}

    fresh = cda.create_model("small", n_mels=90)
    fopt = torch.optim.AdamW(fresh.parameters())
    other = types.SimpleNamespace(seed=0, _draws=0)
    params_before = [p for p in fresh.parameters()]
    ptrs = [p.data_ptr() for p in params_before]
    epoch, got = cda.load_checkpoint(path, fresh, fopt, trainer=other)
    assert (epoch, got) == (8, metrics) and (other.seed, other._draws) == (1234, 17)
    assert [p.data_ptr() for p in fresh.parameters()] == ptrs           # copied in place
    for (k, a), b in zip(model.state_dict().items(), fresh.state_dict().values()):
        assert torch.equal(a, b), k
    assert fopt.param_groups[0]["lr"] == 2e-3 and fopt.param_groups[0]["weight_decay"] == 0.05
    for a, b in zip(opt.state_dict()["state"].values(), fopt.state_dict()["state"].values()):
        assert torch.equal(a["exp_avg"], b["exp_avg"]) and float(a["step"]) == float(b["step"]) == 1.0
    # without an optimizer / trainer only the model is touched
    again = cda.create_model("small", n_mels=90)
    assert cda.load_checkpoint(path, again) == (8, metrics)


def test_a_checkpoint_in_the_reference_schema_loads(tmp_path):
    """what the reference's save_checkpoint writes: plain torch.save of its five keys"""
    model = _small()
    opt = _stepped_adamw(model)
    path = str(tmp_path / "ref.pt")
    torch.save({"epoch": 3, "model_state_dict": model.state_dict(), "optimizer_state_dict": opt.state_dict(),
                "metrics": {"f1": 0.5}, "config": {"model_type": "small"}}, path)
    fresh = cda.create_model("small", n_mels=90)
    fopt = torch.optim.AdamW(fresh.parameters())
    trainer = types.SimpleNamespace(seed=5, _draws=9)
    assert cda.load_checkpoint(path, fresh, fopt, trainer=trainer) == (3, {"f1": 0.5})
    assert (trainer.seed, trainer._draws) == (5, 9)                      # no trainer_state in the file: left alone
    for (k, a), b in zip(model.state_dict().items(), fresh.state_dict().values()):
        assert torch.equal(a, b), k


def test_restated_metrics_on_a_hand_case():
    z = torch.tensor([[0.0, 1.0], [2.0, 1.0], [0.5, 0.5], [float("nan"), 0.0], [0.0, float("nan")], [-1.0, 3.0]])
    t = torch.tensor([1, 1, 0, 1, 0, 0])
    assert loop_ref.predict(z).tolist() == [1, 0, 0, 0, 1, 1]
    m = loop_ref.epoch_metrics([(z[:3], t[:3]), (z[3:], t[3:])])
    assert set(m) == loop_ref.METRIC_KEYS
    assert (m["tp"], m["fp"], m["fn"], m["tn"]) == (1, 2, 2, 1) and m["accuracy"] == pytest.approx(100 * 2 / 6)
    assert m["precision"] == pytest.approx(1 / 3) and m["recall"] == pytest.approx(1 / 3) and m["loss"] != m["loss"]
    assert loop_ref.batch_loss(z[:3], torch.tensor([0, 2, 1])) != loop_ref.batch_loss(z[:3], torch.tensor([0, 2, 1]))
    assert loop_ref.early_stop_epoch([1.0, 1.0, 1.0], patience=2) == 2 and loop_ref.early_stop_epoch([3.0, 2.0, 1.0], 1) is None
