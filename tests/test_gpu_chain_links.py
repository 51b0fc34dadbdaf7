"""The waveform chain on the MI355X, link by link, against tests/chain_ref.py.

tests/chain_trace.py records what every launch of a run read and wrote; ``chain_ref.check_trace`` holds the record
against ``expected_links`` -- which launches ran, that each read bit for bit what the one before it wrote over exactly the
expected length, that the first launch and no other carries the time shift, every plan word, every width and zero tail --
and, with ``float_checks``, holds every link's output against the float64 restatement of that step on the link's own
recorded input, under the bound the step's own test uses.  No error has to be carried through the phase vocoder that way,
and the bit-equality of "input of link k = output of link k - 1" makes the links a chain.  tests/test_chain_ref_host.py
shows that these checks see the planted defects.

One batch (``chain_ref.LENGTHS``: below 257 samples the stretch copies, 4097 crosses a warp tile, 16385 needs two reverb
spans) runs through ``AudioAugmentor._run_chain`` and ``DeviceDataLoader.launch_batch`` in all 27 configurations (each step
off, on with nothing fired, fired), with values in the 8 that have every step on, plain and phase-locked, and through
``launch_batch_drawn`` for every on / off combination at two seeds, against the restated draws.  The final output of the
all-fired configuration is also held against ``chain_ref``'s whole-chain result, within ``WHOLE_CHAIN_FACTOR`` times what
the links' own tolerances move that result by (``chain_ref.WHOLE_CHAIN_MOVED``, profiles/chain_links.txt).
"""
import numpy as np
import pytest
import torch

import cough_detector_amd as cda
from cough_detector_amd import _lib
from cough_detector_amd.data import BatchPlan
import chain_ref as C
from chain_trace import recording

pytestmark = pytest.mark.gpu
SHIPPED = dict(use_pcen=False, use_pre_emphasis=False, use_delta_delta=False, use_spectral_contrast=False)
INDICES = list(range(len(C.LENGTHS)))


@pytest.fixture(scope="module")
def room():
    return cda.synth_rirs(C.N_RIRS, seed=3)[0]


@pytest.fixture(scope="module")
def batch():
    rows, (gaussian, bank) = C.batch_rows(), C.batch_noise()
    x = torch.zeros((len(rows), max(C.LENGTHS)))
    for r, row in enumerate(rows):
        x[r, :row.size] = torch.from_numpy(row)
    clips = cda.DeviceClipBank([torch.from_numpy(row) for row in rows], [r % 2 for r in INDICES])
    pre = cda.AudioPreprocessor(device="cuda", **SHIPPED)
    return dict(rows=rows, x=x.cuda(), gaussian=torch.from_numpy(gaussian), bank=bank, clips=clips, pre=pre)


def _augmentor(batch, room, speed=True, pitch=True, lock=False):
    aug = cda.AudioAugmentor(p_augment=C.DEVICE_P, speed=speed, pitch=pitch, phase_lock=lock, reverb=room)
    aug.noise_samples = [torch.from_numpy(entry)[None] for entry in batch["bank"]]
    aug._pack_bank()
    return aug


def _host_case(config, lock=False):
    shifts, pairs, steps, rirs = C.batch_draws(config)
    links = C.expected_links(shifts, pairs, steps, rirs, C.LENGTHS, max(C.LENGTHS), phase_lock=lock)
    records = C.batch_records(shifts, links[-1]["read"])
    clips = [_lib.CoughAugClip.from_buffer_copy(records[r].tobytes()) for r in INDICES]
    return dict(pairs=pairs, steps=steps, rirs=rirs, links=links, clips=clips, new=[int(v) for v in links[-1]["read"]])


def _both_paths(batch, room, config, lock, float_checks, worst=None):
    """The configuration through ``_run_chain`` and through ``launch_batch``; both records pass ``check_trace`` and end in
    the same bits -> the final output of the first."""
    case, aug = _host_case(config, lock), _augmentor(batch, room, lock=lock)
    with recording() as direct:
        out = aug._run_chain(batch["x"], case["clips"], C.LENGTHS, case["pairs"], case["steps"], batch["gaussian"], 0,
                             rirs=case["rirs"])
    torch.cuda.synchronize()
    C.check_trace(direct, case["links"], source=batch["rows"], float_checks=float_checks, taps=room.taps, worst=worst)
    width = case["links"][-1]["width"]
    assert tuple(out.shape) == (len(INDICES), width) and (out.cpu().numpy() == direct[-1]["out"][:, :width]).all()
    loader = cda.DeviceDataLoader(batch["clips"], batch["pre"], batch_size=len(INDICES), audio_augmentor=aug, noise="host")
    plan = BatchPlan(clips=case["clips"], gaussian=batch["gaussian"], seed=0, pairs=case["pairs"],
                     new_lengths=case["new"] if case["pairs"] is not None else None, steps=case["steps"], rirs=case["rirs"])
    with recording() as loaded:
        feats, _ = loader.launch_batch(INDICES, plan)
    torch.cuda.synchronize()
    C.check_trace(loaded, case["links"], source=batch["rows"], float_checks=float_checks, taps=room.taps, worst=worst)
    assert tuple(feats.shape) == (len(INDICES), 1, 90, 101)
    assert (loaded[-1]["out"].view(np.uint32) == direct[-1]["out"].view(np.uint32)).all()
    return direct[-1]["out"]


# ------------------------------------------------------------------------------------------------ host draws
@pytest.mark.parametrize("config", C.CONFIGS, ids=["-".join(c) for c in C.CONFIGS])
def test_host_draws_structure(batch, room, config):
    _both_paths(batch, room, config, False, float_checks=False)


@pytest.mark.parametrize("lock", [False, True], ids=["plain", "locked"])
@pytest.mark.parametrize("config", C.ON_CONFIGS, ids=["-".join(c) for c in C.ON_CONFIGS])
def test_host_draws_values(batch, room, config, lock):
    worst = {}
    _both_paths(batch, room, config, lock, float_checks=True, worst=worst)
    print("worst |y - y_ref| / tolerance:", {k: f"{v:.3g}" for k, v in worst.items()})
    carrier = {("fired",) * 3: "warp", ("idle", "fired", "fired"): "stretch", ("idle", "idle", "fired"): "reverb",
               ("idle",) * 3: "augment"}.get(config)
    if carrier is not None:                                                  # each of the four carriers of the shift
        assert _host_case(config, lock)["links"][0]["kind"] == carrier


# ------------------------------------------------------------------------------------------------ device draws
@pytest.mark.parametrize("seed,on", C.DEVICE_CASES, ids=[f"{seed}-{int(s)}{int(p)}{int(r)}" for seed, (s, p, r) in C.DEVICE_CASES])
def test_device_draws(batch, room, seed, on):
    """The plans and the records come back from the device and equal the restated draws' links; every link in front of the
    last is held to its restatement, the last only to its inputs (its noise is drawn on the device: test_gpu_draws.py)."""
    speed, pitch, reverb = on
    aug = _augmentor(batch, room if reverb else None, speed=speed, pitch=pitch)
    loader = cda.DeviceDataLoader(batch["clips"], batch["pre"], batch_size=len(INDICES), audio_augmentor=aug, draws="device")
    with recording() as trace:
        feats, _ = loader.launch_batch_drawn(INDICES, seed)
    torch.cuda.synchronize()
    links, records = C.device_links(seed, on)
    assert [link["kind"] for link in links] == (["warp"] if speed else []) + (["stretch", "back"] if pitch else []) \
        + (["reverb"] if reverb else []) + ["augment"]
    worst = {}
    C.check_trace(trace, links, source=batch["rows"], taps=room.taps, last_values=False, worst=worst)
    print("worst |y - y_ref| / tolerance:", {k: f"{v:.3g}" for k, v in worst.items()})
    want = records.copy()
    if len(links) > 1:
        want["shift"] = 0                                                    # cleared once a launch has shifted the rows
    assert trace[-1]["records"].tobytes() == want.tobytes()
    assert tuple(feats.shape) == (len(INDICES), 1, 90, 101) and torch.isfinite(feats).all()


# ------------------------------------------------------------------------------------------------ the whole chain
@pytest.mark.parametrize("lock", [False, True], ids=["plain", "locked"])
def test_the_whole_chain_agrees_with_chain_ref(batch, room, lock):
    config = ("fired",) * 3
    got = _both_paths(batch, room, config, lock, float_checks=False).astype(np.float64)
    shifts, pairs, steps, rirs = C.batch_draws(config)
    links = C.expected_links(shifts, pairs, steps, rirs, C.LENGTHS, max(C.LENGTHS), phase_lock=lock)
    trace = C.run_links(links, batch["rows"], C.batch_records(shifts, links[-1]["read"]), batch["gaussian"].numpy(),
                        batch["bank"], room.taps)
    want = trace[-1]["out"].astype(np.float64)
    assert got.shape == want.shape
    for r in INDICES:
        peak = float(np.abs(want[r]).max())
        off = float(np.abs(got[r] - want[r]).max())
        allowed = C.WHOLE_CHAIN_FACTOR * C.WHOLE_CHAIN_MOVED[lock][r] * peak
        print(f"row {r}: off by {off / peak if peak else off:.3e} of the peak, allowed {C.WHOLE_CHAIN_FACTOR * C.WHOLE_CHAIN_MOVED[lock][r]:.3e}")
        assert off <= allowed, (r, off, allowed)
