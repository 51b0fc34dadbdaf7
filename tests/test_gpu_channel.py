"""The capture channel on the MI355X (cough_detector_amd/channel.py, csrc/channel.hip) against tests/channel_ref.py.

One ragged batch (``channel_ref.batch``) covers the chunk and span edges, cascades of 1 to 4 sections, every kind of
ratio and the signals that hurt: it runs twice, once with every ratio set to 1 -- the filter alone, held to the bound
``|y - y_ref| <= 2^-24 |y_ref| + K 2^-53 G peak(x)`` against the long-double recurrence -- and once as it is; the clipped
run must be, bit for bit, the reference clip of the device's own unclipped rows.  Copies, padding columns, the NaN and
silence rules, a row alone, a repeated call, the call in place, the draws and everything that composes kernels compared
elsewhere (the augmentor, the loaders) are compared bit for bit.  tests/test_channel_host.py shows that the bound sees
the planted defects.
"""
import random

import numpy as np
import pytest
import torch

import cough_detector_amd as cda
from cough_detector_amd import _lib
from cough_detector_amd import channel as cch
from cough_detector_amd.data import BatchPlan
import channel_ref as R
import draws_ref as D

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


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def mics():
    return cda.ChannelBank.from_sos(R.batch()[0])


@pytest.fixture(scope="module")
def batch(mics):
    """The ragged batch of tests/channel_ref.py, run once without and once with its ceilings."""
    _, rows = R.batch()
    packed, offsets = _pack([r["x"] for r in rows])
    assert len({int(o) % 4 for o in offsets}) == 4
    data, offs = torch.from_numpy(packed).cuda(), torch.from_numpy(offsets).cuda()
    lens = torch.tensor([r["x"].size for r in rows], dtype=torch.int32).cuda()
    # device plans: one filter is beyond the bank on purpose, which the host check would refuse
    plain_plans, clip_plans = (cch.plans_to_device(R.plans_of(rows, c), data.device) for c in (False, True))
    plain = cch.channel_rows(data, offs, lens, plain_plans, R.WIDTH, mics)
    clipped = cch.channel_rows(data, offs, lens, clip_plans, R.WIDTH, mics)
    torch.cuda.synchronize()
    return dict(rows=rows, data=data, offs=offs, lens=lens, plain_plans=plain_plans, clip_plans=clip_plans, plain=plain,
                clipped=clipped, plain_host=plain.cpu().numpy(), clipped_host=clipped.cpu().numpy())


# ------------------------------------------------------------------------------------------------ 1. the filter
def test_every_filtered_row_is_inside_the_bound(batch):
    worst = {}
    for r, row in enumerate(batch["rows"]):
        if row["rule"] is not None:
            continue
        y = batch["plain_host"][r, :row["x"].size]
        err = np.abs(y.astype(np.longdouble) - row["ref"])
        u = R.units(y, row["ref"], row["g"], row["peak"])
        worst[row["filter"]] = max(worst.get(row["filter"], 0.0), u)
        print(f"{row['name']:42s} filter {row['filter']}: {u:10.4g} units of 2^-53 G peak beyond 2^-24 |y_ref|")
        assert np.isfinite(y).all() and (err <= R.bound(row["ref"], row["g"], row["peak"])).all(), (row["name"], u, R.BOUND_K)
    print("largest per filter:", {k: f"{v:.4g}" for k, v in sorted(worst.items())}, "K =", R.BOUND_K)
    assert set(worst) == {0, 1, 2, 3, 4}


def test_copies_rules_and_padding_bit_for_bit(batch):
    seen = set()
    for clipped in (False, True):
        got = batch["clipped_host" if clipped else "plain_host"]
        for r, row in enumerate(batch["rows"]):
            n = row["x"].size
            assert not _bits(got[r, n:]).any(), (row["name"], "padding columns are +0.0")
            want = R.expect_exact(row, clipped)
            if want is not None:
                seen.add(row["rule_clipped" if clipped else "rule"])
                assert np.array_equal(_bits(got[r, :n]), _bits(want)), (row["name"], clipped)
    assert seen == {"copy", "nan", "zero"}


def test_the_ceiling_is_the_reference_clip_of_the_unclipped_rows(batch):
    clips = 0
    for r, row in enumerate(batch["rows"]):
        n = row["x"].size
        if row["rule_clipped"] is not None:
            continue
        base = batch["plain_host"][r, :n]                        # the device's own unclipped output (a copy without a filter)
        want = R.clip_ref(base, row["ratio"])
        got = batch["clipped_host"][r, :n]
        assert np.array_equal(_bits(got), _bits(want)), row["name"]
        ratio = np.float32(row["ratio"])
        if ratio >= 0 and ratio < 1 and n:
            clips += 1
            c = np.float32(ratio * np.abs(base).max())
            assert np.array_equal(got, np.clip(base, -c, c)) and np.abs(got).max() == c
        else:
            assert np.array_equal(_bits(got), _bits(base))
    assert clips >= 8


def test_a_row_alone_a_call_repeated_and_in_place(batch, mics):
    rows, width = batch["rows"], R.WIDTH
    again = cch.channel_rows(batch["data"], batch["offs"], batch["lens"], batch["clip_plans"], width, mics)
    assert torch.equal(again.view(torch.int32), batch["clipped"].view(torch.int32))
    for r in [k for k, row in enumerate(rows) if row["x"].size in (65, 16385, 32769, 48000)][:6] + [len(rows) - 1]:
        alone = cch.channel_rows(batch["data"], batch["offs"][r:r + 1].contiguous(), batch["lens"][r:r + 1].contiguous(),
                                 batch["clip_plans"][r:r + 1].contiguous(), width, mics)
        assert torch.equal(alone[0].view(torch.int32), batch["clipped"][r].view(torch.int32)), rows[r]["name"]
    # in place: the dense matrix is its own output
    dense = torch.zeros((len(rows), width), dtype=torch.float32)
    for r, row in enumerate(rows):
        dense[r, :row["x"].size] = torch.from_numpy(row["x"])
    dense = dense.cuda()
    offs = (torch.arange(len(rows), dtype=torch.int64) * width).cuda()
    out = cch.channel_rows(dense.view(-1), offs, batch["lens"], batch["clip_plans"], width, mics, out=dense)
    assert out.data_ptr() == dense.data_ptr()
    assert torch.equal(dense.view(torch.int32), batch["clipped"].view(torch.int32))
    # a narrower matrix cuts the rows: the first `width` samples, filtered as they are in the full row
    narrow = cch.channel_rows(batch["data"], batch["offs"], batch["lens"], batch["plain_plans"], 20000, mics)
    for r, row in enumerate(rows):
        if row["rule"] is None:
            assert torch.equal(narrow[r].view(torch.int32), batch["plain"][r, :20000].view(torch.int32)), row["name"]


def test_the_prepared_bank_is_the_restated_blob(mics):
    blob = mics.blob()
    assert blob.numel() == cch.bank_bytes(len(mics)) == 1280 * len(mics) and cch.bank_bytes(0) == 1280
    got = blob.cpu().numpy().view(np.float64).reshape(len(mics), R.ENTRY_WORDS)
    assert got.tobytes() == R.blob_ref(R.batch()[0]).tobytes()


def test_refusals(batch, mics):
    d, width = batch, R.WIDTH
    lib = _lib.load_channel()
    st = torch.cuda.current_stream().cuda_stream
    args = lambda **k: [k.get("src", d["data"].data_ptr()), d["offs"].data_ptr(), d["lens"].data_ptr(), k.get("b", 3),     # noqa: E731
                        d["clip_plans"].data_ptr(), k.get("bank", mics.blob().data_ptr()), k.get("n_bank", len(mics)),
                        k.get("out", d["plain"].data_ptr()), k.get("width", width), st]
    for bad in (dict(b=-1), dict(width=0), dict(width=2**30 + 1), dict(n_bank=-1), dict(src=None), dict(out=None), dict(bank=None),
                dict(src=d["data"].data_ptr() + 2), dict(bank=mics.blob().data_ptr() + 8), dict(b=2**24 + 1)):
        assert lib.cough_channel_rows(*args(**bad)) != 0, bad
        assert lib.cough_channel_last_error()
    assert lib.cough_channel_rows(*args(b=0, src=None, out=None)) == 0                   # launches nothing
    with pytest.raises(ValueError):
        cch.channel_rows(d["data"], d["offs"], d["lens"], R.plans_of(d["rows"], True), width, mics)       # host plans are checked
    one = np.array([[1.0, 0, 0, 1, 0, 0]])
    ws = torch.empty(2560, dtype=torch.uint8, device="cuda")
    for sos, n_sec in ((np.array([[1.0, 0, 0, 0, 0, 0]]), [1]), (np.array([[1.0, 0, 0, 1, 0, 1.0]]), [1]), (np.array([[np.nan, 0, 0, 1, 0, 0]]), [1]),
                       (np.array([[1.0, 0, 0, 1, 2.0, 1.0 - 1e-9]]), [1]), (np.concatenate([one] * 5), [5]), (one, [0])):
        with pytest.raises(ValueError):
            cch.prepare(sos, np.array(n_sec, dtype=np.int32), ws)
    with pytest.raises((ValueError, RuntimeError)):
        cch.prepare(np.concatenate([one] * 3), np.array([1, 1, 1], dtype=np.int32), ws)                  # three entries, room for two
    for kw in (dict(p_augment=1.5), dict(p_clip=-0.1), dict(clip_range=(0.8, 0.2)), dict(clip_range=(0.2, float("inf")))):
        with pytest.raises(ValueError):
            cda.draw_channel(1, 4, **{"p_augment": 0.5, "bank": 3, "p_clip": 0.3, "clip_range": (0.25, 1.0), **kw})


# ------------------------------------------------------------------------------------------------ 2. the draws
@pytest.mark.parametrize("b", [1, 64, 65, 1000])
def test_channel_draws_equal_the_restatement(b):
    for seed, p, n_bank, p_clip, rng in ((7, 0.5, 9, 0.3, (0.25, 1.0)), (2**63 + 12345, 0.8, 1, 1.0, (0.0, 0.5)), (3, 1.0, 0, 0.5, (0.5, 0.5)),
                                         (2**64 - 1, 0.0, 4, 0.5, (0.1, 0.9))):
        got = cda.draw_channel(seed, b, p, n_bank, p_clip, rng).cpu().numpy()
        want = R.draw_channel_ref(seed, b, p, n_bank, p_clip, *rng)
        assert got.dtype == np.int32 and got.shape == (b, 2)
        assert got.tobytes() == want.tobytes(), (seed, b)
    bank = cda.ChannelBank.from_sos([np.array([[1.0, 0, 0, 1, 0, 0]])] * 9)
    assert torch.equal(cda.draw_channel(5, b, 0.5, bank), cda.draw_channel(5, b, 0.5, 9))
    assert cda.draw_channel(5, 0, 0.5, 9).shape == (0, 2)


# ------------------------------------------------------------------------------------------------ 3. the chain
def _rows(lengths, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(n, generator=g) - 0.5) * 0.8 for n in lengths]


@pytest.fixture(scope="module")
def synth():
    return cda.synth_channels(6, seed=3)[0]


def _augmentor(p, channel, speed=False, pitch=False, reverb=None, n_bank=3, p_clip=0.5):
    g = torch.Generator().manual_seed(11)
    aug = cda.AudioAugmentor(p_augment=p, speed=speed, pitch=pitch, reverb=reverb, channel=channel, p_clip=p_clip)
    aug.noise_samples = [torch.randn((1, n), generator=g) * 0.3 for n in NOISE_BANK[:n_bank]]
    aug._pack_bank()
    return aug


CHAIN_LENGTHS = [1, 2, 257, 4097, 16000, 9000, 16385, 700]


def _matrix(rows):
    x = torch.zeros((len(rows), max(r.numel() for r in rows)))
    for r, row in enumerate(rows):
        x[r, :row.numel()] = row
    return x


@pytest.mark.parametrize("p,speed,pitch", [(1.0, False, False), (0.5, False, False), (0.7, True, True)])
def test_augment_batch_equals_augment_clip_by_clip(synth, p, speed, pitch):
    rows = _rows(CHAIN_LENGTHS, seed=5)
    x = _matrix(rows)
    aug = _augmentor(p, synth, speed=speed, pitch=pitch)
    random.seed(31)
    torch.manual_seed(31)
    got, got_lens = aug.augment_batch(x.cuda(), lengths=CHAIN_LENGTHS, noise="host", return_lengths=True)
    random.seed(31)
    torch.manual_seed(31)
    singles = [aug.augment(row[None].cuda()) for row in rows]
    random.seed(31)
    items = [aug.draw_item_channel(v) for v in CHAIN_LENGTHS]
    assert sum(it[5] is not None for it in items) >= 2 and (p == 1.0 or any(it[5] is None for it in items))
    assert got_lens.tolist() == [s.shape[1] for s in singles] == [it[2] for it in items]
    for r, s in enumerate(singles):
        assert torch.equal(got[r, :s.shape[1]], s[0]), r
        assert not got[r, s.shape[1]:].any(), r


def test_the_channel_step_alone_is_the_filter_and_the_ceiling(synth):
    """No other step fires: the augmentor's output is ``channel_rows`` of the clip with the drawn plan."""
    aug = cda.AudioAugmentor(p_augment=1.0, channel=synth, p_clip=1.0, clip_range=(0.3, 0.6))
    x = _rows([16000], seed=9)[0]
    random.seed(4)
    mic = aug.draw_item_channel(16000)[5]
    assert mic is not None and 0.3 <= mic[1] <= 0.6
    got = aug._run_channel(x[None].cuda(), [16000], [mic])[0].cpu().numpy()
    ref = R.recurrence([synth.sos[mic[0]]], [x.numpy()], np.longdouble)[0]
    g, peak = R.gain(synth.sos[mic[0]]), float(x.abs().max())
    unclipped = aug._run_channel(x[None].cuda(), [16000], [(mic[0], 1.0)])[0].cpu().numpy()
    assert (np.abs(unclipped.astype(np.longdouble) - ref) <= R.bound(ref, g, peak)).all()
    assert np.array_equal(_bits(got), _bits(R.clip_ref(unclipped, mic[1]))) and not np.array_equal(got, unclipped)


def test_channel_off_is_todays_output(synth, monkeypatch):
    rows = _rows(CHAIN_LENGTHS, seed=5)
    x = _matrix(rows)
    aug = _augmentor(0.7, None)
    random.seed(12)
    got = aug.augment_batch(x.cuda(), lengths=CHAIN_LENGTHS, noise="device", seed=99)
    random.seed(12)
    want = aug._run(x.cuda(), aug.draw_batch(CHAIN_LENGTHS), CHAIN_LENGTHS, None, 99)
    assert torch.equal(got, want)
    # a batch in which no channel coin fired runs the launches it ran before: channel_rows is not called
    called = []
    original = cch.channel_rows
    monkeypatch.setattr(cch, "channel_rows", lambda *a, **k: called.append(1) or original(*a, **k))
    mic = _augmentor(0.7, synth)
    monkeypatch.setattr(mic, "_draw_channel", lambda: None)
    random.seed(12)
    assert torch.equal(mic.augment_batch(x.cuda(), lengths=CHAIN_LENGTHS, noise="device", seed=99), want) and not called
    monkeypatch.setattr(mic, "_draw_channel", lambda: (2, 0.5))
    random.seed(12)
    wet = mic.augment_batch(x.cuda(), lengths=CHAIN_LENGTHS, noise="device", seed=99)
    assert called == [1] and not torch.equal(wet, want)


# ------------------------------------------------------------------------------------------------ 4. the loader
@pytest.fixture(scope="module")
def pre():
    return cda.AudioPreprocessor(device="cuda", **SHIPPED)


@pytest.fixture(scope="module")
def clip_bank():
    rng = np.random.default_rng(5)
    lengths = rng.integers(8000, 30001, size=24).tolist()
    labels = [int(i % 3 == 0) for i in range(24)]
    return cda.DeviceClipBank(_rows(lengths, seed=23), labels), lengths


def test_a_host_drawn_batch_equals_its_items_and_the_loader_without_the_step(clip_bank, pre, synth):
    bank, lengths = clip_bank
    loader = cda.DeviceDataLoader(bank, pre, batch_size=6, audio_augmentor=_augmentor(0.6, synth), spec_augmentor=cda.SpecAugment(p=0.5),
                                  noise="host", generator=torch.Generator().manual_seed(1))
    plain_loader = cda.DeviceDataLoader(bank, pre, batch_size=6, audio_augmentor=_augmentor(0.6, None), spec_augmentor=cda.SpecAugment(p=0.5),
                                        noise="host", generator=torch.Generator().manual_seed(1))
    indices = [(7 + 5 * i) % 24 for i in range(6)]
    random.seed(100)
    torch.manual_seed(100)
    plan = loader.draw_batch(indices)
    feats, targets = loader.launch_batch(indices, plan)
    assert tuple(feats.shape) == (6, 1, 90, 101) and torch.isfinite(feats).all() and plan.mics()
    for r, i in enumerate(indices):
        one = BatchPlan(clips=[plan.clips[r]], gaussian=plan.gaussian[r:r + 1].contiguous(), seed=plan.seed, masks=[plan.masks[r]],
                        channels=[plan.channels[r]])
        f, t = loader.launch_batch([i], one)
        assert torch.equal(f[0], feats[r]) and torch.equal(t[0], targets[r]), r
    # the step changes the features where it fired, and only there; with no coin fired the batch is the plain loader's
    fired = [c is not None for c in plan.channels]
    plan.channels = [None] * 6
    dry, _ = loader.launch_batch(indices, plan)
    assert any(fired) and not all(fired) and [not torch.equal(feats[r], dry[r]) for r in range(6)] == fired
    plan.channels = None
    plain, _ = plain_loader.launch_batch(indices, plan)
    assert torch.equal(dry, plain)


def _restated_plan(seed, lengths, aug, spec, shape):
    """The BatchPlan that holds the restated device draws of ``seed``: the records, the masks, the channel plans."""
    n_f, n_t = spec.n_freq_masks, spec.n_time_masks
    clips, masks, f = D.draw_ref(seed, np.asarray(lengths, dtype=np.int32), aug.p_augment, aug._bank_lengths, spec.p, n_f,
                                 spec.freq_mask_param, n_t, spec.time_mask_param, *shape)
    plan = BatchPlan(seed=seed)
    mics = R.draw_channel_ref(seed, len(lengths), aug.p_augment, len(aug.channel), aug.p_clip, *aug.clip_range)
    plan.channels = [(int(m["filter"]), float(m["clip_ratio"])) if m["filter"] >= 0 else None for m in mics]
    plan.clips = [_lib.CoughAugClip(shift=int(r["shift"]), gain=float(r["gain"]), gaussian=int(r["gaussian"]),
                                    bank_index=int(r["bank_index"]), gaussian_snr_db=float(r["gaussian_snr_db"]),
                                    bank_snr_db=float(r["bank_snr_db"]), bank_start=int(r["bank_start"])) for r in clips]
    plan.masks = [[tuple(int(v) for v in masks[:, r, m]) for m in range(n_f + n_t)] if f["spec"][r] else [] for r in range(len(lengths))]
    return plan


def test_launch_batch_drawn_equals_launch_batch_on_the_restated_plan(clip_bank, pre, synth, monkeypatch):
    bank, lengths = clip_bank
    aug, spec = _augmentor(0.5, synth), cda.SpecAugment(p=0.5)
    loader = cda.DeviceDataLoader(bank, pre, batch_size=8, audio_augmentor=aug, spec_augmentor=spec, draws="device",
                                  generator=torch.Generator().manual_seed(1))
    fired = 0
    for k, seed in enumerate((7, 2**63 + 12345)):
        indices = [(11 * k + 3 * i) % 24 for i in range(8)]
        feats, targets = loader.launch_batch_drawn(indices, seed)
        plan = _restated_plan(seed, [lengths[i] for i in indices], aug, spec, loader.feature_shape())
        want, want_targets = loader.launch_batch(indices, plan)
        assert torch.equal(feats, want) and torch.equal(targets, want_targets), (k, seed)
        fired += sum(c is not None for c in plan.channels)
    assert 0 < fired < 16                                                  # rows with and without a channel step
    monkeypatch.setattr(cda.DeviceDataLoader, "draw_batch", lambda *a: pytest.fail("draw_batch was called"))
    assert len(list(loader)) == 3 == len(loader)
