"""Room reverberation on the MI355X (cough_detector_amd/reverb.py, csrc/reverb.hip) against tests/reverb_ref.py.

One ragged batch (``reverb_ref.cases``) covers the edges; every row goes through ``reverb_ref.check_row``: the header's
bound per sample, the span rule and the silence rule exactly, copies and padding columns bit for bit, and the RMS error
against float64 at most 4 x the float32 emulation's (tests/test_reverb_host.py shows that these checks see the planted
defects).  Everything that composes kernels compared elsewhere (the chain, the loaders, the bank) is compared bit for bit.
"""
import random

import numpy as np
import pytest
import torch

import cough_detector_amd as cda
from cough_detector_amd import _lib
from cough_detector_amd import reverb as crev
from cough_detector_amd.data import BatchPlan
import draws_ref as D
import pitch_ref as P
import reverb_ref as R
import warp_ref as W

pytestmark = pytest.mark.gpu
SHIPPED = dict(use_pcen=False, use_pre_emphasis=False, use_delta_delta=False, use_spectral_contrast=False)
NOISE_BANK = [700, 9000, 20000]


def _pack(xs):
    """Rows packed at offsets of every phase modulo 4, NaN between them: a read outside a row shows."""
    pieces, offsets, at = [np.full(1, np.nan, dtype=np.float32)], [], 1
    for r, x in enumerate(xs):
        offsets.append(at)
        gap = 1 + (r + x.size) % 4
        pieces += [np.asarray(x, dtype=np.float32), np.full(gap, np.nan, dtype=np.float32)]
        at += x.size + gap
    return np.concatenate(pieces), np.asarray(offsets, dtype=np.int64)


@pytest.fixture(scope="module")
def rirs():
    return cda.RirBank(R.expected()[0])


@pytest.fixture(scope="module")
def batch(rirs):
    """The ragged batch of tests/reverb_ref.py, convolved once."""
    _, rows, width, exp = R.expected()
    packed, offsets = _pack([r["x"] for r in rows])
    assert len({int(o) % 4 for o in offsets}) == 4
    data, offs = torch.from_numpy(packed).cuda(), torch.from_numpy(offsets).cuda()
    lens = torch.tensor([r["x"].size for r in rows], dtype=torch.int32).cuda()
    plans = crev.plan_array([(r["shift"], r["rir"], r["out_len"]) for r in rows], len(rirs), width)
    y = crev.reverb_rows(data, offs, lens, plans, width, rirs)
    torch.cuda.synchronize()
    return dict(rows=rows, exp=exp, width=width, data=data, offs=offs, lens=lens, plans=plans, y=y, y_host=y.cpu().numpy())


# ------------------------------------------------------------------------------------------------ 1. the convolution
def test_every_row_is_inside_the_contract(batch):
    assert tuple(batch["y"].shape) == (len(batch["rows"]), batch["width"]) and batch["y"].dtype == torch.float32
    ratios = []
    for r, (row, e) in enumerate(zip(batch["rows"], batch["exp"])):
        dev, emu = R.rms_errors(batch["y_host"][r], row, e)
        if emu:
            ratios.append(dev / emu)
            print(f"{row['name']}: device RMS error {dev:.3e}, emulation {emu:.3e}, ratio {dev / emu:.2f}")
        R.check_row(batch["y_host"][r], row, e, batch["width"])
    assert len(ratios) >= 20 and max(ratios) <= R.RMS_FACTOR


def test_a_non_finite_sample_spoils_its_spans_and_nothing_else(batch):
    seen = 0
    for r, (row, e) in enumerate(zip(batch["rows"], batch["exp"])):
        if row["twin"] is None:
            continue
        y, twin = batch["y_host"][r], batch["y_host"][row["twin"]]
        assert any(e["bad"]) and not all(e["bad"])
        for w, bad in enumerate(e["bad"]):
            span = slice(R.N * w, min(R.N * (w + 1), row["out_len"]))
            if bad:
                assert np.isnan(y[span]).all() and np.isfinite(twin[span]).all()
            else:                                          # bit for bit what it is without that sample
                assert y[span].view(np.uint32).tolist() == twin[span].view(np.uint32).tolist(), (row["name"], w)
        seen += 1
    assert seen == 4


def test_an_impulse_response_delays_the_row(batch, rirs):
    rng = np.random.default_rng(12)
    x = rng.standard_normal(40000).astype(np.float32)
    data = torch.from_numpy(x).cuda()
    offs, lens = torch.zeros(4, dtype=torch.int64).cuda(), torch.full((4,), 40000, dtype=torch.int32).cuda()
    width = 40000 + 8192
    y = crev.reverb_rows(data, offs, lens, crev.plan_array([(0, k, width) for k in (5, 6, 7, 8)]), width, rirs).cpu().numpy()
    for k, at in enumerate((0, 1, 8191, 8192)):
        want = np.zeros(width)
        want[at:at + 40000] = x
        assert np.abs(y[k] - want).max() <= 1e-5, at                    # far inside the bound (2e-3); an off-by-one would be ~1


def test_a_row_alone_and_a_call_repeated(batch, rirs):
    again = crev.reverb_rows(batch["data"], batch["offs"], batch["lens"], batch["plans"], batch["width"], rirs)
    assert torch.equal(again.view(torch.int32), batch["y"].view(torch.int32))
    for r in (5, 13, 24, 27, 30, len(batch["rows"]) - 1):
        row = batch["rows"][r]
        width = max(row["out_len"], 1)
        alone = crev.reverb_rows(torch.from_numpy(row["x"]).cuda() if row["x"].size else torch.zeros(1).cuda(),
                                 torch.zeros(1, dtype=torch.int64).cuda(), torch.tensor([row["x"].size], dtype=torch.int32).cuda(),
                                 crev.plan_array([(row["shift"], row["rir"], row["out_len"])]), width, rirs)
        assert torch.equal(alone[0, :row["out_len"]].view(torch.int32), batch["y"][r, :row["out_len"]].view(torch.int32)), row["name"]


def test_the_prepared_bank(rirs):
    ws = rirs.workspace(torch.device("cuda", torch.cuda.current_device()))
    assert ws.numel() == crev.bank_bytes(len(rirs)) == 131072 * (len(rirs) + 1)
    table = ws.view(torch.float32).view(len(rirs) + 1, R.N, 2).cpu().numpy()
    assert np.abs(table[0, :, 0] - R.TW_R).max() <= 2.0 ** -24 and np.abs(table[0, :, 1] - R.TW_I).max() <= 2.0 ** -24
    assert (table[0, :, 0] == R.TW_R).mean() > 0.999 and (table[0, :, 1] == R.TW_I).mean() > 0.999
    for k, h in enumerate(rirs.taps):
        hr, hi = R.spectrum(h)
        scale = float(np.abs(h).sum()) / R.N                                 # max |H| <= ||h||_1 / N
        assert np.abs(table[k + 1, :, 0] - hr).max() <= 1e-5 * scale and np.abs(table[k + 1, :, 1] - hi).max() <= 1e-5 * scale
    assert rirs.workspace(ws.device) is ws                                   # prepared once per device


# ------------------------------------------------------------------------------------------------ 2. refusals
def test_refusals(batch, rirs):
    data, offs, lens = batch["data"], batch["offs"][:2].contiguous(), batch["lens"][:2].contiguous()
    for bad in ((0, len(rirs), 4), (0, -2, 4), (0, 0, -1), (0, 0, 101)):
        with pytest.raises(ValueError):
            crev.reverb_rows(data, offs, lens, np.array([[0, 0, 4, 0], list(bad) + [0]], dtype=np.int32), 100, rirs)
    plans = torch.zeros((2, 4), dtype=torch.int32).cuda()
    for width in (0, -5, 2**30 + 1):
        with pytest.raises(ValueError):
            crev.reverb_rows(data, offs, lens, plans, width, rirs)
    with pytest.raises(ValueError):
        crev.reverb_rows(data, offs, lens[:1].contiguous(), plans, 100, rirs)
    with pytest.raises(ValueError):
        crev.reverb_rows(data.double(), offs, lens, plans, 100, rirs)
    with pytest.raises(RuntimeError):
        crev.reverb_rows(data.cpu(), offs.cpu(), lens.cpu(), plans.cpu(), 100, rirs)
    lib, st = _lib.load_reverb(), torch.cuda.current_stream().cuda_stream
    ws, out = rirs.workspace(data.device), torch.empty((2, 100), dtype=torch.float32).cuda()
    args = lambda **kw: [kw.get("src", data.data_ptr()), offs.data_ptr(), lens.data_ptr(), kw.get("rows", 2), plans.data_ptr(),  # noqa: E731
                         kw.get("ws", ws.data_ptr()), kw.get("n_rirs", len(rirs)), kw.get("out", out.data_ptr()), kw.get("width", 100), st]
    assert lib.cough_reverb_rows(*args()) == _lib.OK
    for kw in (dict(rows=-1), dict(n_rirs=-1), dict(src=None), dict(ws=None), dict(out=data.data_ptr()), dict(ws=ws.data_ptr() + 4),
               dict(out=out.data_ptr() + 2), dict(width=0)):
        assert lib.cough_reverb_rows(*args(**kw)) == _lib.EINVAL, kw
        assert lib.cough_reverb_last_error().decode().startswith("cough_reverb_rows:")
    assert lib.cough_reverb_rows(*args(width=2**30 + 1)) == _lib.EUNSUPPORTED        # refused before anything is launched
    assert lib.cough_reverb_rows(*args(rows=0, src=None)) == _lib.OK
    # the bank: a response of 8194 taps, a workspace that is too small
    taps = torch.ones(8194, dtype=torch.float32).cuda()
    big = torch.empty(crev.bank_bytes(1), dtype=torch.uint8).cuda()
    with pytest.raises(ValueError, match="8193"):
        crev.prepare(taps, np.array([0]), np.array([8194]), big)
    with pytest.raises(ValueError):
        crev.prepare(taps, np.array([0]), np.array([0]), big)
    with pytest.raises(RuntimeError, match="workspace"):
        crev.prepare(taps, np.array([0]), np.array([8193]), big[:131072 * 2 - 256])
    crev.prepare(taps, np.array([1]), np.array([8193]), big)
    assert crev.bank_bytes(0) == 131072 and lib.cough_reverb_bank_bytes(-1) == 0
    with pytest.raises(ValueError):
        cda.draw_reverb(1, lens, 1.5, rirs)
    torch.cuda.synchronize()


def test_device_plans_are_made_harmless(batch, rirs):
    rows = [5, 7, 24, 27]
    offs, lens = batch["offs"][rows].contiguous(), batch["lens"][rows].contiguous()
    width = 20000
    wild = np.array([[0, 99, 20000, 7], [3, -5, 2**31 - 1, -1], [0, 3, -4, 0], [-2**31, 4, 20001, 0]], dtype=np.int32)
    tame = np.array([[0, -1, 20000, 0], [3, -1, 20000, 0], [0, 3, 0, 0], [-2**31, 4, 20000, 0]], dtype=np.int32)
    got = crev.reverb_rows(batch["data"], offs, lens, torch.from_numpy(wild).cuda(), width, rirs)
    want = crev.reverb_rows(batch["data"], offs, lens, torch.from_numpy(tame).cuda(), width, rirs)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and torch.isfinite(got).all()
    assert not got[2].any() and not got[3].any()                            # out_len 0; a shift that empties the row


# ------------------------------------------------------------------------------------------------ 3. the draws
@pytest.mark.parametrize("b", [1, 63, 64, 257])                            # one thread; a block less one; a block; several
def test_reverb_draws_equal_the_restatement(b):
    pool = [0, 1, 256, 16000, 16385, 48000, 2**31 - 1, -3]
    lengths = [pool[(5 * i + b) % len(pool)] for i in range(b)]
    lens = torch.tensor(lengths, dtype=torch.int32).cuda()
    case, mixed = 0, False
    for p in (0.0, 0.5, 1.0):
        for n_rirs in (1, 9, 100, 0):
            case += 1
            seed = (case * 0x9E3779B97F4A7C15 + b) & (2**64 - 1)           # both key words in use
            got = cda.draw_reverb(seed, lens, p, n_rirs).cpu().numpy()
            want = R.draw_reverb_ref(seed, lengths, p, n_rirs)
            assert got.dtype == np.int32 and got.shape == (b, 4) and (got == want).all(), (p, n_rirs)
            mixed |= bool((want[:, 1] >= 0).any() and (want[:, 1] < 0).any())
    assert mixed or b == 1
    bank = cda.RirBank([np.ones(3)] * 9)
    assert torch.equal(cda.draw_reverb(5, lens, 0.5, bank), cda.draw_reverb(5, lens, 0.5, 9))


# ------------------------------------------------------------------------------------------------ 4. the chain
def _rows(lengths, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(n, generator=g) - 0.5) * 0.8 for n in lengths]


@pytest.fixture(scope="module")
def room():
    return cda.synth_rirs(7, seed=3)[0]


def _augmentor(p, room, speed=False, pitch=False, n_bank=3):
    g = torch.Generator().manual_seed(11)
    aug = cda.AudioAugmentor(p_augment=p, speed=speed, pitch=pitch, reverb=room)
    aug.noise_samples = [torch.randn((1, n), generator=g) * 0.3 for n in NOISE_BANK[:n_bank]]
    aug._pack_bank()
    return aug


CHAIN_LENGTHS = [1, 2, 257, 4097, 16000, 9000, 16385, 700]


@pytest.mark.parametrize("p,speed,pitch", [(1.0, False, False), (0.5, False, False), (0.6, True, False), (0.6, False, True),
                                           (0.7, True, True)])
def test_augment_batch_equals_augment_clip_by_clip(room, p, speed, pitch):
    rows = _rows(CHAIN_LENGTHS, seed=5)
    n = max(CHAIN_LENGTHS)
    x = torch.zeros((len(rows), n))
    for r, row in enumerate(rows):
        x[r, :row.numel()] = row
    aug = _augmentor(p, room, speed=speed, pitch=pitch)
    random.seed(31)
    torch.manual_seed(31)
    got, got_lens = aug.augment_batch(x.cuda(), lengths=CHAIN_LENGTHS, noise="host", return_lengths=True)
    random.seed(31)
    torch.manual_seed(31)
    singles = [aug.augment(row[None].cuda()) for row in rows]
    random.seed(31)
    items = [aug.draw_item_reverb(v) for v in CHAIN_LENGTHS]
    assert sum(it[4] is not None for it in items) >= 2 and (p == 1.0 or any(it[4] is None for it in items))
    assert got_lens.tolist() == [s.shape[1] for s in singles] == [it[2] for it in items]
    assert tuple(got.shape) == (len(rows), max(got_lens.tolist()) if speed else n) and got.is_cuda
    for r, s in enumerate(singles):
        assert torch.equal(got[r, :s.shape[1]], s[0]), r
        assert not got[r, s.shape[1]:].any(), r
    if not speed:
        assert got_lens.tolist() == CHAIN_LENGTHS                          # the reverb step keeps the lengths


def test_the_reverb_step_alone_is_the_convolution(room):
    """No other step fires: the chain's output is the shifted row convolved with the drawn response, tail dropped."""
    aug = cda.AudioAugmentor(p_augment=1.0, reverb=room)
    x = _rows([16000], seed=9)[0]
    random.seed(4)
    c, pair, n_new, steps, rir = aug.draw_item_reverb(16000)
    assert rir is not None and pair is None and steps is None and n_new == 16000
    c.gain, c.gaussian, c.bank_index = 1.0, 0, -1
    got = aug._run_chain(x[None], [c], None, None, None, None, 0, rirs=[rir])[0].numpy()
    want = R.reverb_ref(x.numpy(), c.shift, room.taps[rir], 16000)
    assert c.shift != 0 and np.abs(got - want).max() <= R.bound(x.numpy(), c.shift, room.taps[rir], 16000).max()
    assert np.abs(got - want).max() <= 1e-5


def test_reverb_off_is_todays_output(room):
    rows = _rows(CHAIN_LENGTHS, seed=5)
    n = max(CHAIN_LENGTHS)
    x = torch.zeros((len(rows), n))
    for r, row in enumerate(rows):
        x[r, :row.numel()] = row
    aug = _augmentor(0.7, None)
    random.seed(12)
    got = aug.augment_batch(x.cuda(), lengths=CHAIN_LENGTHS, noise="device", seed=99)
    random.seed(12)
    want = aug._run(x.cuda(), aug.draw_batch(CHAIN_LENGTHS), CHAIN_LENGTHS, None, 99)
    assert torch.equal(got, want) and tuple(got.shape) == (len(rows), n)
    # a batch in which no reverb coin fired runs the launches it ran before: reverb_rows is not called
    wet = _augmentor(0.7, room)
    called = []
    original = crev.reverb_rows
    crev.reverb_rows = lambda *a, **k: called.append(1) or original(*a, **k)
    try:
        clips = aug.draw_batch(CHAIN_LENGTHS)
        out = wet._run_chain(x.cuda(), clips, CHAIN_LENGTHS, None, None, None, 99, rirs=[None] * len(rows))
        assert not called and torch.equal(out, aug._run(x.cuda(), clips, CHAIN_LENGTHS, None, 99))
        wet._run_chain(x.cuda(), clips, CHAIN_LENGTHS, None, None, None, 99, rirs=[0] + [None] * (len(rows) - 1))
        assert called == [1]
    finally:
        crev.reverb_rows = original


# ------------------------------------------------------------------------------------------------ 5. the loader
@pytest.fixture(scope="module")
def pre():
    return cda.AudioPreprocessor(device="cuda", **SHIPPED)


@pytest.fixture(scope="module")
def clip_bank():
    rng = np.random.default_rng(5)
    lengths = rng.integers(8000, 30001, size=24).tolist()
    labels = [int(i % 3 == 0) for i in range(24)]
    return cda.DeviceClipBank(_rows(lengths, seed=23), labels), lengths


@pytest.mark.parametrize("speed,pitch", [(False, False), (True, True)])
def test_a_host_drawn_batch_equals_its_items_one_at_a_time(clip_bank, pre, room, speed, pitch):
    bank, lengths = clip_bank
    loader = cda.DeviceDataLoader(bank, pre, batch_size=6, audio_augmentor=_augmentor(0.6, room, speed=speed, pitch=pitch),
                                  spec_augmentor=cda.SpecAugment(p=0.5), noise="host", generator=torch.Generator().manual_seed(1))
    wet = 0
    for k in range(2):
        indices = [(7 * k + 5 * i) % 24 for i in range(6)]
        random.seed(100 + k)
        torch.manual_seed(100 + k)
        plan = loader.draw_batch(indices)
        feats, targets = loader.launch_batch(indices, plan)
        assert tuple(feats.shape) == (6, 1, 90, 101) and torch.isfinite(feats).all()
        wet += plan.reverbs()
        for r, i in enumerate(indices):
            one = BatchPlan(clips=[plan.clips[r]], gaussian=plan.gaussian[r:r + 1].contiguous(), seed=plan.seed,
                            masks=[plan.masks[r]], pairs=[plan.pairs[r]] if speed else None,
                            new_lengths=[plan.new_lengths[r]] if speed else None, steps=[plan.steps[r]] if pitch else None,
                            rirs=[plan.rirs[r]])
            f, t = loader.launch_batch([i], one)
            assert torch.equal(f[0], feats[r]) and torch.equal(t[0], targets[r]), (k, r)
    assert wet >= 1
    # the reverb step changes the features where it fired, and only there
    fired = [r is not None for r in plan.rirs]
    plan.rirs = [None] * 6
    plain, _ = loader.launch_batch(indices, plan)
    assert any(fired) and [not torch.equal(feats[r], plain[r]) for r in range(6)] == fired


def _restated_plan(seed, lengths, aug, spec, shape):
    """The BatchPlan that holds the restated device draws of ``seed``: speed and pitch if the augmentor has them, reverb."""
    sr = aug.sample_rate
    if aug.speed:
        plans, new_lens, _ = W.draw_speed_ref(seed, lengths, aug.p_augment, aug.speed_range[0], aug.speed_range[1], sr)
    else:
        new_lens = np.asarray(lengths, dtype=np.int32)
    n_f, n_t = (spec.n_freq_masks, spec.n_time_masks) if spec is not None else (0, 0)
    clips, masks, f = D.draw_ref(seed, new_lens, aug.p_augment, aug._bank_lengths, spec.p if spec is not None else None, n_f,
                                 spec.freq_mask_param if spec else 0, n_t, spec.time_mask_param if spec else 0, *shape)
    plan = BatchPlan(seed=seed)
    if aug.pitch:
        _, _, _, steps, fired = P.draw_pitch_ref(seed, new_lens, aug.p_augment, aug.pitch_range[0], aug.pitch_range[1], sr)
        plan.steps = [int(s) if fi else None for s, fi in zip(steps, fired)]
    rev = R.draw_reverb_ref(seed, new_lens, aug.p_augment, len(aug.reverb))
    assert (rev[:, 2] == new_lens).all()                                   # out_len is the row's current length
    plan.rirs = [int(r) if r >= 0 else None for r in rev[:, 1]]
    if aug.speed:
        clips["shift"] = plans[:, 0]                                       # drawn for the original length
        plan.pairs, plan.new_lengths = [(int(o), int(m)) for _, o, m in plans], [int(v) for v in new_lens]
    plan.clips = [_lib.CoughAugClip(shift=int(r["shift"]), gain=float(r["gain"]), gaussian=int(r["gaussian"]),
                                    bank_index=int(r["bank_index"]), gaussian_snr_db=float(r["gaussian_snr_db"]),
                                    bank_snr_db=float(r["bank_snr_db"]), bank_start=int(r["bank_start"])) for r in clips]
    if masks is not None:
        plan.masks = [[tuple(int(v) for v in masks[:, r, m]) for m in range(n_f + n_t)] if f["spec"][r] else []
                      for r in range(len(lengths))]
    return plan


@pytest.mark.parametrize("speed,pitch", [(False, False), (True, False), (False, True), (True, True)])
def test_launch_batch_drawn_equals_launch_batch_on_the_restated_plan(clip_bank, pre, room, monkeypatch, speed, pitch):
    bank, lengths = clip_bank
    aug, spec = _augmentor(0.5, room, speed=speed, pitch=pitch), cda.SpecAugment(p=0.5)
    loader = cda.DeviceDataLoader(bank, pre, batch_size=8, audio_augmentor=aug, spec_augmentor=spec, draws="device",
                                  generator=torch.Generator().manual_seed(1))
    wet = 0
    for k, seed in enumerate((7, 2**63 + 12345)):
        indices = [(11 * k + 3 * i) % 24 for i in range(8)]
        feats, targets = loader.launch_batch_drawn(indices, seed)
        plan = _restated_plan(seed, [lengths[i] for i in indices], aug, spec, loader.feature_shape())
        want, want_targets = loader.launch_batch(indices, plan)
        assert tuple(feats.shape) == (8, 1, 90, 101) and feats.is_cuda
        assert torch.equal(feats, want) and torch.equal(targets, want_targets), (k, seed)
        wet += sum(r is not None for r in plan.rirs)
    assert 0 < wet < 16                                                    # rows with and without a reverb step
    monkeypatch.setattr(cda.DeviceDataLoader, "draw_batch", lambda *a: pytest.fail("draw_batch was called"))
    assert len(list(loader)) == 3 == len(loader)


# ------------------------------------------------------------------------------------------------ 6. the bank
@pytest.mark.parametrize("keep_tail", [True, False])
def test_reverberate_bank_equals_per_row_calls(room, keep_tail):
    lengths = [1, 300, 16000, 9000, 20000, 16385]
    bank = cda.DeviceClipBank(_rows(lengths, seed=41), [1, 0, 1, 1, 0, 1])
    index = [2, -1, 0, 6, 3, -1]
    wet = cda.reverberate_bank(bank, room, index, keep_tail=keep_tail, max_elements=60000)     # several groups
    assert isinstance(wet, cda.DeviceClipBank) and wet.labels.tolist() == bank.labels.tolist() and wet.device == bank.device
    want_lens = [n + (int(room.lengths[k]) - 1 if keep_tail and k >= 0 else 0) for n, k in zip(lengths, index)]
    assert wet.lengths.tolist() == want_lens and wet.data.numel() == sum(want_lens)
    for i, (n, k) in enumerate(zip(lengths, index)):
        one = crev.reverb_rows(bank.data, bank.offsets_dev[i:i + 1].contiguous(), bank.lengths_dev[i:i + 1].contiguous(),
                               crev.plan_array([(0, k, want_lens[i])]), want_lens[i], room)
        assert torch.equal(wet.clip(i)[0].view(torch.int32), one[0].view(torch.int32)), i
        if k < 0:
            assert torch.equal(wet.clip(i), bank.clip(i))
    assert torch.equal(cda.reverberate_bank(bank, room, index, keep_tail=keep_tail).data, wet.data)    # one group
    with pytest.raises(ValueError):
        cda.reverberate_bank(bank, room, index[:-1])
    with pytest.raises(ValueError):
        cda.reverberate_bank(bank, room, [7] * 6)
    # an empty clip, copied or convolved with one tap, stays empty -- alone in its group and beside another clip
    one_tap = cda.RirBank([np.array([0.5], dtype=np.float32)])
    holed = cda.DeviceClipBank.from_packed(bank.data[:5].clone(), [0, 5, 0], [0, 1, 0])
    for idx, groups in (([-1, 0, 0], 1), ([0, -1, -1], 1), ([0, 0, -1], 1 << 26)):
        out = cda.reverberate_bank(holed, one_tap, idx, keep_tail=keep_tail, max_elements=groups)
        assert out.lengths.tolist() == [0, 5, 0] and out.data.numel() == 5
        if idx[1] < 0:
            assert torch.equal(out.data, holed.data)
        else:
            assert torch.allclose(out.data, holed.data * 0.5, rtol=0, atol=1e-6)
    # far-field events go into the scenes as any bank does
    plan = cda.draw_scene_plan(bank, wet.subset([0, 2, 3]), 2, 8.0, events_per_scene=(1, 2), seed=1)
    scenes, truth = cda.compose_scenes(bank, wet.subset([0, 2, 3]), plan)
    assert len(scenes) == 2 and torch.isfinite(scenes.data).all()
