"""The epoch loop on the MI355X (cough_detector_amd/loop.py, csrc/loop.hip) against the float64 restatement
(tests/loop_ref.py), the reference-generated logits under tests/golden/ and the existing ``train_epoch``.

Bounds.  A batch loss of the meter is within ``1e-6 * max(1, max|z|)`` of float64 ``CrossEntropyLoss(weight)`` on the same
float32 logits: the per-clip term is a float32 exp / log / add / subtract chain at a few ulp of max|z| (2^-24 max|z| each),
the sums run in double, and a weighted mean of terms cannot be further off than the worst of them.  ``validate`` against
the golden logits: the kernels' logits are within the project's 1e-3 of the reference's, which moves a clip's CE by at
most 2e-3 (|d lse| <= max|dz| and |d z_y| <= max|dz|), hence the mean by at most 2e-3; every clip used has a golden margin
|z1 - z0| > 1e-2 (asserted), ten times the logit tolerance, so every prediction and with it every count, accuracy,
precision, recall and F1 is exact.  ``train_epoch_async`` sums the same float32 losses in the same order in double as
``train_epoch`` and counts the same predictions, so the two agree to the last bit.
"""
import json

import numpy as np
import pytest
import torch

import cough_detector_amd as cda
import loop_ref
from cough_detector_amd.training import ResidualTrainer, SmallTrainer, train_epoch
from test_train_small_host import small_sd

pytestmark = pytest.mark.gpu
CW = [0.6, 3.0]
SHIPPED = dict(use_pcen=False, use_pre_emphasis=False, use_delta_delta=False, use_spectral_contrast=False)
CONFIG = dict(model_type="small", sample_rate=16000, n_mels=64, n_fft=512, hop_length=160, win_length=400, f_min=100.0,
              f_max=4000.0, segment_duration=1.0, n_mfcc=13, use_mfcc=True, pre_emphasis_coef=0.97, n_contrast_bands=6,
              **SHIPPED)


# ------------------------------------------------------------------------------------------------ the meter
def _one_update(z, t, cw=None, preds=False, batch_loss=None):
    meter = cda.EpochMeter("cuda")
    p = torch.full((z.shape[0],), -7, dtype=torch.int64, device="cuda") if preds else None
    meter.update(z.cuda(), t.cuda(), class_weights=cw, batch_loss=batch_loss, preds_out=p)
    return meter.result(), meter._buf.cpu().clone(), (None if p is None else p.cpu())


@pytest.mark.parametrize("scale", [1.0, 10.0, 50.0])
@pytest.mark.parametrize("b", [1, 7, 32, 257, 4096])
def test_meter_matches_float64(scale, b):
    g = torch.Generator().manual_seed(int(scale) * 10007 + b)
    z = torch.randn(b, 2, generator=g) * scale
    t = torch.randint(0, 2, (b,), generator=g)
    if b >= 7:
        z[3] = z[3, 0]                                   # a tie predicts class 0
    bound = 1e-6 * max(1.0, z.abs().max().item())
    want_counts = loop_ref.counts(loop_ref.predict(z), t)
    for cw in (None, CW):
        r, raw, preds = _one_update(z, t, cw, preds=True)
        want = loop_ref.batch_loss(z, t, cw)
        print(f"scale {scale} B {b} weights {cw}: loss {r['loss_sum']!r} float64 {want!r} "
              f"diff {abs(r['loss_sum'] - want):.3e} bound {bound:.3e}")
        assert r["n_batches"] == 1
        assert {k: r[k] for k in want_counts} == want_counts
        assert torch.equal(preds, loop_ref.predict(z))
        assert r["loss_sum"] == float(np.float32(r["loss_sum"]))          # a float32 value, as loss.item()
        assert abs(r["loss_sum"] - want) <= bound
        r2, raw2, preds2 = _one_update(z, t, cw, preds=True)
        assert torch.equal(raw, raw2) and torch.equal(preds, preds2)
        r3, raw3, _ = _one_update(z, t, cw, preds=False)
        assert torch.equal(raw, raw3)


def test_meter_nan_logits_and_out_of_range_targets():
    nan = float("nan")
    z = torch.tensor([[0.5, 1.5], [nan, 1.0], [1.0, nan], [nan, nan], [2.0, -1.0], [0.25, 0.25], [-3.0, 4.0]])
    t = torch.tensor([1, 1, 0, 1, 0, 1, 0])
    r, _, preds = _one_update(z, t, CW, preds=True)
    assert preds.tolist() == loop_ref.predict(z).tolist() == [1, 0, 1, 0, 0, 0, 1]
    assert r["loss_sum"] != r["loss_sum"] and loop_ref.batch_loss(z, t, CW) != loop_ref.batch_loss(z, t, CW)
    want = loop_ref.counts(preds, t)
    assert {k: r[k] for k in want} == want
    assert (r["tp"], r["fp"], r["fn"], r["tn"], r["correct"], r["total"]) == (1, 2, 3, 1, 2, 7)
    # a NaN in one clip only: the other clips' counts are untouched, the loss is NaN with or without weights
    for cw in (None, CW):
        assert np.isnan(_one_update(z[:2], t[:2], cw)[0]["loss_sum"])
        assert np.isfinite(_one_update(z[4:], t[4:], cw)[0]["loss_sum"])
    # targets outside {0, 1}: NaN loss, the clip enters `total` only
    g = torch.Generator().manual_seed(5)
    z = torch.randn(40, 2, generator=g)
    t = torch.randint(0, 2, (40,), generator=g)
    ok, _, _ = _one_update(z, t, CW)
    for bad in (2, -1, 1 << 40):
        tb = t.clone()
        tb[11] = bad
        r, _, preds = _one_update(z, tb, CW, preds=True)
        assert np.isnan(r["loss_sum"]) and np.isnan(loop_ref.batch_loss(z, tb, CW))
        want = loop_ref.counts(preds, tb)
        assert {k: r[k] for k in want} == want and r["total"] == 40
        assert r["tp"] + r["fp"] + r["fn"] + r["tn"] == 39
        assert torch.equal(preds, loop_ref.predict(z))
    assert np.isfinite(ok["loss_sum"])


def test_meter_accumulates_and_takes_a_given_batch_loss():
    g = torch.Generator().manual_seed(9)
    meter = cda.EpochMeter("cuda")
    batches, given = [], [0.625, 1.0e-3, 3.1415927, 17.5]
    for i, b in enumerate((32, 32, 5, 300)):
        z, t = torch.randn(b, 2, generator=g) * 3, torch.randint(0, 2, (b,), generator=g)
        batches.append((z, t))
        meter.update(z.cuda(), t.cuda(), batch_loss=torch.tensor(given[i], dtype=torch.float32, device="cuda"))
    r = meter.result()
    total = 0.0
    for v in given:
        total += float(np.float32(v))
    assert r["loss_sum"] == total and r["n_batches"] == 4 and r["total"] == 369
    want = loop_ref.counts(torch.cat([loop_ref.predict(z) for z, _ in batches]), torch.cat([t for _, t in batches]))
    assert {k: r[k] for k in want} == want
    # computed losses: the sum of the float32 batch losses, in order, in double
    meter.reset()
    assert meter.result() == dict(loss_sum=0.0, n_batches=0, total=0, correct=0, tp=0, fp=0, fn=0, tn=0)
    singles = 0.0
    for z, t in batches:
        meter.update(z.cuda(), t.cuda(), class_weights=CW)
        singles += _one_update(z, t, CW)[0]["loss_sum"]
    assert meter.result()["loss_sum"] == singles
    with pytest.raises(ValueError):
        meter.update(torch.zeros(4, 3).cuda(), torch.zeros(4, dtype=torch.int64).cuda())
    with pytest.raises(ValueError):
        meter.update(torch.zeros(4, 2).cuda(), torch.zeros(3, dtype=torch.int64).cuda())
    with pytest.raises(ValueError):
        meter.update(torch.zeros(0, 2).cuda(), torch.zeros(0, dtype=torch.int64).cuda())


# ------------------------------------------------------------------------------------------------ validate
def _golden_case(name, resnet_golden, cnn_golden, resnet_heights_golden):
    if name == "resnet":
        sd, vec = resnet_golden
        return "residual", sd, vec["x"], vec["logits"]
    if name in ("standard", "small"):
        sd, vec = cnn_golden[name]
        return name, sd, cnn_golden["x"], vec["logits"]
    sd, vec = resnet_heights_golden[name]
    return "residual", sd, vec["x"], vec["logits"]


def _batches_of(x, y, n):
    return [(x[i:i + n], y[i:i + n]) for i in range(0, x.shape[0], n)]


@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
@pytest.mark.parametrize("name", ["resnet", "standard", "small", "h103", "h64"])
def test_validate_against_the_reference_logits(name, dtype, resnet_golden, cnn_golden, resnet_heights_golden):
    kind, sd, x, zref = _golden_case(name, resnet_golden, cnn_golden, resnet_heights_golden)
    n = x.shape[0]
    assert n % 5 != 0                                                      # the last batch is ragged
    margin = (zref[:, 1] - zref[:, 0]).abs().min().item()
    assert margin > 1e-2, margin
    y = torch.randint(0, 2, (n,), generator=torch.Generator().manual_seed(1234 + n))
    model = cda.create_model(kind, n_mels=90, num_classes=2, in_channels=1, compute_dtype=dtype)
    model.load_state_dict(sd)
    for cw in (None, CW):
        want = loop_ref.epoch_metrics(_batches_of(zref, y, 5), cw, item32=True)
        got = cda.validate(model, _batches_of(x, y, 5), class_weights=cw)
        print(f"{name} {dtype} weights {cw}: loss {got['loss']!r} expected {want['loss']!r} "
              f"diff {abs(got['loss'] - want['loss']):.3e}; margin {margin:.3f}; counts "
              f"{[got[k] for k in ('tp', 'fp', 'fn', 'tn')]}")
        assert set(got) == loop_ref.METRIC_KEYS
        for k in ("tp", "fp", "fn", "tn", "accuracy", "precision", "recall", "f1"):
            assert got[k] == want[k], k
        assert got["tp"] + got["fp"] + got["fn"] + got["tn"] == n          # no clip is left out
        assert abs(got["loss"] - want["loss"]) <= 2e-3
        assert not model.training
        # inputs already on the device, targets on the host: the same numbers
        dev = cda.validate(model.cuda(), [(a.cuda(), b) for a, b in _batches_of(x, y, 5)], class_weights=cw, device="cuda")
        assert dev == got


# ------------------------------------------------------------------------------------------------ training epochs
class _Masked:
    """A trainer whose ``step`` takes the next of a list of explicit dropout masks (what ``train_epoch`` needs of a
    trainer: ``model``, ``device`` and ``step``)."""

    def __init__(self, trainer, masks):
        self.trainer, self.masks, self.i = trainer, masks, 0
        self.model, self.device = trainer.model, trainer.device

    def step(self, inputs, targets):
        mask = self.masks[self.i]
        self.i += 1
        return self.trainer.step(inputs, targets, dropout_mask=mask)


def _small_state():
    sd = dict(small_sd())
    sd["classifier.4.weight"] = sd["classifier.4.weight"] / 100           # logits of a few units (test_gpu_train_small.py)
    sd["classifier.4.bias"] = sd["classifier.4.bias"] / 100
    return sd


def _make_trainer(kind, sd, **kw):
    m = cda.create_model(kind, n_mels=90, num_classes=2, in_channels=1, compute_dtype="fp32")
    m.load_state_dict(sd)
    return (SmallTrainer if kind == "small" else ResidualTrainer)(m, class_weights=CW, **kw)


def _epoch_data(width, seed, sizes=(8, 8, 5)):
    g = torch.Generator().manual_seed(seed)
    data, masks = [], []
    for b in sizes:
        data.append((torch.randn(b, 1, 90, 101, generator=g), torch.randint(0, 2, (b,), generator=g)))
        masks.append((torch.rand(b, width, generator=g) >= 0.4).float())
    return data, masks


@pytest.mark.parametrize("kind", ["small", "residual"])
def test_train_epoch_async_equals_train_epoch(kind, resnet_golden):
    sd = _small_state() if kind == "small" else resnet_golden[0]
    data, masks = _epoch_data(64 if kind == "small" else 128, seed=21)
    a, b = _make_trainer(kind, sd), _make_trainer(kind, sd)
    want = [train_epoch(_Masked(a, masks), data, e) for e in range(2)]
    got = [cda.train_epoch_async(_Masked(b, masks), data, e) for e in range(2)]
    print(f"{kind}: train_epoch {want} train_epoch_async {got}")
    assert got == want and set(got[0]) == {"loss", "accuracy"}
    assert np.isfinite(got[0]["loss"]) and got[0] != got[1]
    assert torch.equal(a._params, b._params) and torch.equal(a._running, b._running) and torch.equal(a._nbt, b._nbt)
    assert torch.equal(a.optimizer._exp_avg, b.optimizer._exp_avg)
    assert b.model.training
    # device-resident batches and the device dropout generator: the same again
    c, d = _make_trainer(kind, sd, seed=3), _make_trainer(kind, sd, seed=3)
    on_dev = [(x.cuda(), y.cuda()) for x, y in data]
    assert cda.train_epoch_async(d, on_dev, 0) == train_epoch(c, data, 0)
    assert torch.equal(c._params, d._params)


def test_validate_on_a_trainer_bound_model():
    sd = _small_state()
    tr = _make_trainer("small", sd, seed=1)
    data, _ = _epoch_data(64, seed=33)
    val = _batches_of(torch.randn(13, 1, 90, 101, generator=torch.Generator().manual_seed(2)),
                      torch.randint(0, 2, (13,), generator=torch.Generator().manual_seed(3)), 5)
    before = cda.validate(tr.model, val, class_weights=tr.class_weights)
    cda.train_epoch_async(tr, data, 0)
    after = cda.validate(tr.model, val, class_weights=tr.class_weights)
    plain = cda.create_model("small", n_mels=90, compute_dtype="fp32")
    plain.load_state_dict({k: v.cpu() for k, v in tr.model.state_dict().items()})
    assert after == cda.validate(plain, val, class_weights=CW)
    assert after["loss"] != before["loss"]
    # the logits behind the numbers: the restatement on the model's own eval-mode outputs
    with torch.no_grad():
        zs = [(tr.model(x.cuda()).cpu(), y) for x, y in val]
    want = loop_ref.epoch_metrics(zs, CW, item32=True)
    assert {k: after[k] for k in ("tp", "fp", "fn", "tn", "accuracy", "f1")} == \
           {k: want[k] for k in ("tp", "fp", "fn", "tn", "accuracy", "f1")}
    assert abs(after["loss"] - want["loss"]) <= 1e-6 * max(1.0, max(z.abs().max().item() for z, _ in zs))


def test_resume_continues_bit_for_bit(tmp_path):
    sd = _small_state()
    data, _ = _epoch_data(64, seed=41, sizes=(8, 8, 8, 8))
    path = str(tmp_path / "ck.pt")
    a = _make_trainer("small", sd, seed=77, lr=2e-3)
    for x, y in data[:2]:
        a.step(x, y)                                                       # dropout_mask=None: the device generator
    cda.save_checkpoint(a.model, a.optimizer, 4, {"f1": 0.25}, path, dict(CONFIG), trainer=a)
    for x, y in data[2:]:
        a.step(x, y)
    torch.manual_seed(0)
    fresh = cda.create_model("small", n_mels=90, num_classes=2, in_channels=1, compute_dtype="fp32")
    b = SmallTrainer(fresh, class_weights=CW, seed=1, lr=5e-4)
    flat = b._params.data_ptr()
    assert cda.load_checkpoint(path, fresh, b.optimizer, trainer=b) == (4, {"f1": 0.25})
    assert b._params.data_ptr() == flat and next(fresh.parameters()).data_ptr() == flat     # the flat views survive
    assert (b.seed, b._draws, b.optimizer._n_steps) == (77, 2, 2) and b.optimizer.param_groups[0]["lr"] == 2e-3
    for x, y in data[2:]:
        b.step(x, y)
    assert torch.equal(a._params, b._params)
    assert torch.equal(a.optimizer._exp_avg, b.optimizer._exp_avg)
    assert torch.equal(a.optimizer._exp_avg_sq, b.optimizer._exp_avg_sq)
    assert a.optimizer._n_steps == b.optimizer._n_steps == 4
    assert torch.equal(a._running, b._running) and torch.equal(a._nbt, b._nbt)
    for (k, u), v in zip(a.model.state_dict().items(), b.model.state_dict().values()):
        assert torch.equal(u, v), k
    ma, mb = torch.empty(8, 64, device="cuda"), torch.empty(8, 64, device="cuda")
    a.forward_backward(*data[0], mask_out=ma)
    b.forward_backward(*data[0], mask_out=mb)
    assert torch.equal(ma, mb) and a._draws == b._draws == 5
    # without trainer_state the generator would start over: the stored draw count matters
    c = _make_trainer("small", sd, seed=77, lr=2e-3)
    mc = torch.empty(8, 64, device="cuda")
    c.forward_backward(*data[0], mask_out=mc)
    assert not torch.equal(mc, ma)


# ------------------------------------------------------------------------------------------------ fit
def _fit_once(out_dir, feats, labels):
    torch.manual_seed(0)
    model = cda.create_model("small", n_mels=90, num_classes=2, in_channels=1, compute_dtype="fp32")
    counts = {0: int((labels[:32] == 0).sum()), 1: int((labels[:32] == 1).sum())}
    tr = SmallTrainer(model, class_weights=cda.class_weights_from_counts(counts), seed=5)
    train = _batches_of(feats[:32], labels[:32], 8)
    val = _batches_of(feats[32:], labels[32:], 5)
    return tr, cda.fit(tr, train, val, str(out_dir), epochs=3, patience=1, config=dict(CONFIG))


def test_fit_end_to_end(tmp_path):
    from cough_detector_amd import synth
    wav = torch.from_numpy(synth.make_clips(0, 48)).cuda()
    pre = cda.AudioPreprocessor(device="cuda", **SHIPPED)
    feats = pre.extract_features(wav).unsqueeze(1).contiguous()
    assert tuple(feats.shape) == (48, 1, 90, 101)
    labels = torch.randint(0, 2, (48,), generator=torch.Generator().manual_seed(7))
    tr, res = _fit_once(tmp_path / "a", feats, labels)
    _, res2 = _fit_once(tmp_path / "b", feats, labels)
    assert set(res) == {"best_model", "best_f1", "epochs_run", "history"}
    hist = res["history"]
    print("fit history:", json.dumps(hist))
    assert res["epochs_run"] == len(hist) and 1 <= len(hist) <= 3
    assert [h["epoch"] for h in hist] == list(range(len(hist)))
    for h in hist:
        assert set(h["train"]) == {"loss", "accuracy"} and set(h["val"]) == loop_ref.METRIC_KEYS
        assert np.isfinite(h["train"]["loss"]) and np.isfinite(h["val"]["loss"])
        assert h["val"]["tp"] + h["val"]["fp"] + h["val"]["fn"] + h["val"]["tn"] == 16
    losses = [h["val"]["loss"] for h in hist]
    stop = loop_ref.early_stop_epoch(losses, patience=1)
    assert (stop is None and len(hist) == 3) or stop == len(hist) - 1
    assert res2["history"] == hist and res2["best_f1"] == res["best_f1"]
    out = tmp_path / "a"
    assert json.load(open(out / "config.json")) == CONFIG
    assert (out / "latest_model.pt").exists()
    best = max(h["val"]["f1"] for h in hist)
    assert res["best_f1"] == best and res["best_model"] == str(out / "best_model.pt")
    assert (out / "best_model.pt").exists() == (best > 0)
    ck = torch.load(str(out / "latest_model.pt"), map_location="cpu", weights_only=False)
    assert set(ck) == loop_ref.CHECKPOINT_KEYS | {"trainer_state"}
    assert ck["epoch"] == len(hist) - 1 and ck["metrics"] == hist[-1]["val"] and ck["config"] == CONFIG
    assert ck["trainer_state"] == {"seed": 5, "draws": 4 * len(hist)}
    if best > 0:
        bk = torch.load(str(out / "best_model.pt"), map_location="cpu", weights_only=False)
        first_best = next(h for h in hist if h["val"]["f1"] == best)
        assert bk["epoch"] == first_best["epoch"] and bk["metrics"] == first_best["val"]
    # the engine loads what fit wrote and computes what the trained model computes
    eng = cda.CoughDetectorInference(str(out / "latest_model.pt"), verbose=False, compute_dtype="fp32")
    assert eng.config == CONFIG and type(eng.model) is type(tr.model)
    tr.model.eval()
    with torch.no_grad():
        want = tr.model(feats[40:41])
        got = eng.model(feats[40:41])
    assert torch.equal(got, want)
    probs = eng.predict_batch(feats[40:41])
    assert abs(probs[0].item() - torch.softmax(want, 1)[0, 1].item()) <= 1e-6
    # resume: continues at the stored epoch + 1, with the best F1 so far
    torch.manual_seed(0)
    model = cda.create_model("small", n_mels=90, num_classes=2, in_channels=1, compute_dtype="fp32")
    tr3 = SmallTrainer(model, class_weights=tr.class_weights, seed=0)
    res3 = cda.fit(tr3, _batches_of(feats[:32], labels[:32], 8), _batches_of(feats[32:], labels[32:], 5),
                   str(tmp_path / "c"), epochs=len(hist) + 1, patience=1, config=dict(CONFIG),
                   resume=str(out / "latest_model.pt"))
    assert [h["epoch"] for h in res3["history"]] == [len(hist)] and res3["best_f1"] >= hist[-1]["val"]["f1"]
    assert tr3.seed == 5 and tr3._draws == 4 * (len(hist) + 1)
