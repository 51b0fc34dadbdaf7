"""The chain's independent statement (tests/chain_ref.py) without a GPU.

* a trace executed from ``chain_ref`` passes ``check_trace``, and the rows the GPU test stretches are fit for the comparison;
* each of ten defects of the chain's rules, planted into that trace one at a time, makes ``check_trace`` fail -- with the
  message of the check that is meant to see it;
* ``augment_ref`` agrees with ``AudioAugmentorRef`` under the same seeded draws;
* over all 27 configurations ``chain.host_plans`` equals ``expected_links`` word by word.
"""
import copy
import random

import numpy as np
import pytest
import torch

import cough_detector_amd as cda
from cough_detector_amd import _lib
from cough_detector_amd import chain as cchain
import chain_ref as C
import draws_ref as D
from waveform_aug_ref import AudioAugmentorRef

ALL = ("fired", "fired", "fired")
_STRETCH = np.dtype([("shift", np.int32), ("reserved", np.int32), ("rate", np.float64)])


@pytest.fixture(scope="module")
def taps():
    return cda.synth_rirs(C.N_RIRS, seed=3)[0].taps


@pytest.fixture(scope="module")
def batch():
    gaussian, bank = C.batch_noise()
    return dict(rows=C.batch_rows(), gaussian=gaussian, bank=bank)


def _links(config, lock=False, **kw):
    shifts, pairs, steps, rirs = C.batch_draws(config)
    links = C.expected_links(shifts, pairs, steps, rirs, C.LENGTHS, max(C.LENGTHS), phase_lock=lock, **kw)
    return links, C.batch_records(shifts, links[-1]["read"])


def _run(batch, taps, links, records, **kw):
    return C.run_links(links, batch["rows"], records, batch["gaussian"], batch["bank"], taps, **kw)


# ------------------------------------------------------------------------------------------------ the faithful trace
@pytest.mark.parametrize("lock", [False, True])
def test_a_faithful_trace_passes(batch, taps, lock):
    links, records = _links(ALL, lock)
    assert [link["kind"] for link in links] == ["warp", "stretch", "back", "reverb", "augment"]
    worst = {}
    C.check_trace(_run(batch, taps, links, records), links, source=batch["rows"], taps=taps, worst=worst)
    print({k: f"{v:.3g}" for k, v in worst.items()})
    assert set(C.KINDS) <= set(worst) and max(worst[k] for k in C.KINDS) <= 1.0      # float32 rounding alone is inside


def test_every_configuration_passes_the_structural_checks(batch, taps):
    for config in C.CONFIGS:
        links, records = _links(config)
        C.check_trace(_run(batch, taps, links, records), links, source=batch["rows"], float_checks=False)


def _assert_fit(trace, name):
    stretch = [link for link in trace if link["kind"] == "stretch"][0]
    seen = 0
    for r, (x, shift, param) in enumerate(zip(stretch["rows"], stretch["shift"], stretch["param"])):
        f = C.cached_link_ref("stretch", x, shift, param)["fitness"]
        if f is None:
            continue
        print(f"{name} row {r}: margin {f['margin']:.2e}, max E / peak {f['e_over_peak']:.2e}, env_min {f['env_min']:.3f}")
        assert f["margin"] >= C.MIN_MARGIN and f["e_over_peak"] <= C.MAX_E and f["env_min"] >= C.MIN_ENV, (name, r, f)
        seen += 1
    return seen


def test_the_stretched_rows_of_every_gpu_configuration_are_fit_for_a_comparison(batch, taps):
    """The reference chain alone meets ``margin >= 64``, ``E <= 2^-20 peak`` and ``env_min >= 0.25`` on every row with
    semitones, in every configuration whose values the GPU test checks: the eight with all steps on, plain and
    phase-locked, and the device's draws at both seeds."""
    seen = 0
    for config in C.ON_CONFIGS:
        for lock in (False, True):
            links, records = _links(config, lock)
            if any(link["kind"] == "stretch" for link in links):
                seen += _assert_fit(_run(batch, taps, links, records, stop_after="stretch"), f"{config} lock={lock}")
    for seed, on in C.DEVICE_CASES:
        if on[1]:
            links, records = C.device_links(seed, on)
            seen += _assert_fit(_run(batch, taps, links, records, stop_after="stretch"), f"seed {seed} {on}")
    assert seen >= 40


@pytest.mark.parametrize("lock", [False, True])
def test_the_whole_chain_figures_are_the_measured_ones(taps, lock):
    """``WHOLE_CHAIN_MOVED`` is what ``measure`` gives here too (to a quarter: another numpy may sum in another order, and
    the vocoder hands a perturbation on in its own way), so the GPU test's tolerance is a measured one."""
    got, want = C.measure(taps, lock), np.asarray(C.WHOLE_CHAIN_MOVED[lock])
    print(f"phase_lock={lock}: measured {[f'{v:.3e}' for v in got]}")
    assert (got <= 1.25 * want).all() and (got >= 0.8 * want).all() and want[3] == 0.0


# ------------------------------------------------------------------------------------------------ the planted defects
def _two(links):
    links[1]["shift"] = links[0]["shift"].copy()


def _none(links):
    links[0]["shift"][:] = 0


def _second(links):
    links[1]["shift"], links[0]["shift"] = links[0]["shift"].copy(), links[1]["shift"].copy()


def _late(links):
    links[0]["late_shift"] = True


def _pitch_reads_n(links):
    links[1]["read"] = links[0]["read"].copy()


def _out_len_n(links):
    links[3]["param"] = [(rir, int(n)) for (rir, _), n in zip(links[3]["param"], links[0]["read"])]


def _records_shifted(links):
    links[4]["shift"] = links[0]["shift"].copy()


def _resampled(links):
    assert links[0]["param"][3] == (1, 1)
    links[0]["param"][3] = (15000, 16000)


# name -> (configuration, what a defective chain does to the links, the check that must see it)
DEFECTS = {
    "shift carried by two links": (ALL, _two, "plan: link 1"),
    "shift carried by none": (ALL, _none, "plan: link 0"),
    "shift carried by the second link instead of the first": (("off", "fired", "fired"), _second, "plan: link 0"),
    "shift applied after the speed step": (ALL, _late, "value: link 0"),
    "pitch handed n instead of n'": (ALL, _pitch_reads_n, "input: link 1"),
    "reverb out_len = n": (ALL, _out_len_n, "plan: link 3"),
    "augmentation records left shifted": (ALL, _records_shifted, "plan: link 4"),
    "a non-fired row resampled instead of copied": (ALL, _resampled, "plan: link 0"),
}


@pytest.mark.parametrize("name", list(DEFECTS))
def test_a_planted_defect_fails(batch, taps, name):
    config, plant, seen_by = DEFECTS[name]
    links, records = _links(config)
    C.check_trace(_run(batch, taps, links, records), links, source=batch["rows"], taps=taps)      # sound before the defect
    bad = copy.deepcopy(links)
    plant(bad)
    with pytest.raises(AssertionError, match=seen_by):
        C.check_trace(_run(batch, taps, bad, records), links, source=batch["rows"], taps=taps)


def test_the_late_shift_is_seen_by_the_values_alone(batch, taps):
    """Every plan word of that trace is right: only the comparison with the per-step restatement sees it."""
    links, records = _links(ALL)
    bad = copy.deepcopy(links)
    _late(bad)
    C.check_trace(_run(batch, taps, bad, records), links, source=batch["rows"], float_checks=False)


def test_an_output_that_is_not_zero_past_its_length_fails(batch, taps):
    links, records = _links(ALL)
    for k, link in enumerate(links):
        r = int(np.argmax(link["width"] - link["wrote"]))
        assert link["wrote"][r] < link["width"]
        trace = _run(batch, taps, links, records)
        trace[k]["out"][r, link["wrote"][r]] = 1e-3
        with pytest.raises(AssertionError, match=f"layout: link {k}"):
            C.check_trace(trace, links, source=batch["rows"], taps=taps)


def test_a_launch_although_nothing_fired_fails(batch, taps):
    config = ("fired", "fired", "idle")
    links, records = _links(config)
    eager, _ = _links(config, launches="on")
    assert [link["kind"] for link in links] == ["warp", "stretch", "back", "augment"]
    assert [link["kind"] for link in eager] == ["warp", "stretch", "back", "reverb", "augment"]
    assert all(p == (-1, n) for p, n in zip(eager[3]["param"], eager[3]["read"]))
    with pytest.raises(AssertionError, match="links: ran"):
        C.check_trace(_run(batch, taps, eager, records), links, source=batch["rows"], taps=taps)


# ------------------------------------------------------------------------------------------------ the augment restatement
@pytest.mark.parametrize("p", [0.5, 1.0])
def test_augment_ref_agrees_with_the_reference_restatement(p):
    g = torch.Generator().manual_seed(11)
    bank = [torch.randn((1, 700), generator=g) * 0.3, torch.randn((1, 9000), generator=g)]
    ref = AudioAugmentorRef(p_augment=p, noise_samples=bank)
    steps = set()
    for seed, n in enumerate((4000, 701, 16257, 2, 9000, 300, 4000, 1234)):
        x = ((torch.rand((1, n), generator=g) - 0.5) * torch.linspace(0.2, 1.0, n))
        random.seed(seed)
        torch.manual_seed(seed)
        ref.log = []
        want = ref.augment(x)[0].double().numpy()
        torch.manual_seed(seed)
        z = torch.randn_like(x)[0].numpy()                                   # the one randn_like of that call, if it made one
        rec = np.zeros(1, dtype=D.CLIP_DTYPE)[0]
        rec["gain"], rec["bank_index"] = 1.0, -1
        for entry in ref.log:
            steps.add(entry[0])
            if entry[0] == "shift":
                rec["shift"] = entry[1]
            elif entry[0] == "gain":
                rec["gain"] = entry[1]
            elif entry[0] == "gauss":
                rec["gaussian"], rec["gaussian_snr_db"] = 1, entry[1]
            else:
                rec["bank_index"], rec["bank_start"], rec["bank_snr_db"] = entry[1:]
        got = C.augment_ref(x[0].numpy(), int(rec["shift"]), rec, z, [b[0].numpy() for b in bank])
        peak = max(float(np.abs(want).max()), 1e-30)
        print(f"p = {p}, n = {n}: {sorted(e[0] for e in ref.log)}, worst {np.abs(got - want).max() / peak:.2e} of the peak")
        assert np.abs(got - want).max() <= C.REL * peak, (seed, n)
    assert steps == {"shift", "gain", "gauss", "bank"}


# ------------------------------------------------------------------------------------------------ the plans, word by word
@pytest.mark.parametrize("lock", [False, True])
def test_host_plans_equal_the_expected_links_word_by_word(lock):
    n, carriers = max(C.LENGTHS), set()
    for config in C.CONFIGS:
        shifts, pairs, steps, rirs = C.batch_draws(config)
        links = C.expected_links(shifts, pairs, steps, rirs, C.LENGTHS, n, phase_lock=lock)
        plans = cchain.host_plans(shifts, pairs, steps, C.LENGTHS, 16000, n, lock, reverb=rirs)
        by = {link["kind"]: link for link in links}
        assert [k for k in plans.arrays if k != "new_lengths"] == [link["kind"] for link in links[:-1]], config
        assert ("new_lengths" in plans.arrays) == ("warp" in by), config
        carriers.add(links[0]["kind"])
        for kind in ("warp", "back"):
            if kind in by:
                want = np.column_stack([by[kind]["shift"], [p[0] for p in by[kind]["param"]], [p[1] for p in by[kind]["param"]]])
                assert plans.arrays[kind].dtype == np.int32 and (plans.arrays[kind] == want).all(), (config, kind)
        if "stretch" in by:
            got = np.frombuffer(plans.arrays["stretch"].tobytes(), dtype=_STRETCH)
            assert got["shift"].tolist() == by["stretch"]["shift"].tolist(), config
            assert got["reserved"].tolist() == [m for _, m in by["stretch"]["param"]], config
            assert got["rate"].tobytes() == np.array([r for r, _ in by["stretch"]["param"]], dtype=np.float64).tobytes(), config
            assert plans.stretch_width == by["stretch"]["width"], config
            assert (got["reserved"] != 0).any() == lock
        if "reverb" in by:
            want = np.column_stack([by["reverb"]["shift"], [p[0] for p in by["reverb"]["param"]],
                                    [p[1] for p in by["reverb"]["param"]], np.zeros(len(shifts), dtype=np.int64)])
            assert plans.arrays["reverb"].dtype == np.int32 and (plans.arrays["reverb"] == want).all(), config
        assert list(plans.new_lengths) == by["augment"]["read"].tolist(), config
        if plans.arrays:                                                     # the records lose their shift, and nothing else
            assert plans.width == by["augment"]["width"] and not by["augment"]["shift"].any(), config
            records = C.batch_records(shifts, plans.new_lengths)
            clips = [_lib.CoughAugClip.from_buffer_copy(records[r].tobytes()) for r in range(len(shifts))]
            clean = np.frombuffer(b"".join(bytes(c) for c in cchain.unshifted(clips)), dtype=D.CLIP_DTYPE)
            records["shift"] = 0
            assert clean.tobytes() == records.tobytes() and clips[1].shift == shifts[1] != 0, config
        else:                                                                # nothing fired: the records keep it
            assert by["augment"]["shift"].tolist() == shifts and by["augment"]["width"] == n, config
    assert carriers == {"warp", "stretch", "reverb", "augment"}
