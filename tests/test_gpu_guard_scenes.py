"""Every entry point of libcough_amd_scenes.so between the guard zones of tests/guarded.py: the float inputs flush against
a trailing guard, every output allocated at exactly its promised size.  In range, the guarded run must equal the
unguarded one bit for bit.  With garbage in the device-side offset, length, start, index, onset and tile arrays
(negative values, values past the end, descending values) the result is unspecified, but the guards stay intact and no
guard word reaches an output."""
import numpy as np
import pytest
import torch

import cough_detector_amd as cda
from cough_detector_amd import scenes as cscenes
from cough_detector_amd.scenes import TILE, scene_tiles
import guarded as G
import scenes_calls as K

pytestmark = pytest.mark.gpu
HOP, WINDOW, SR = 4000, 16000, 16000
BIG, NEG = 2**31 - 1, -(2**31)
BIG64, NEG64 = 2**62, -(2**62)


def _same(g, what):
    """The guards are intact and no output holds a guard word; the values are whatever they are."""
    got = {x.name: x.view(x.dtype_) for x in g if hasattr(x, "dtype_")}
    G.check(g, got, got, what)


def _out(shape, dtype, name, zero=False):
    g = G.output(shape, dtype, name=name)
    g.dtype_ = dtype
    return g.fill("zeros") if zero else g


@pytest.mark.parametrize("phase", [0, 4, 8, 12])
def test_span_power_between_guards(phase):
    rng = np.random.default_rng(0)
    lengths = [1, 7, 300, 5000]
    bank = rng.standard_normal(sum(lengths)).astype(np.float32)
    offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    clip = np.array([0, 1, 2, 3, 3, 2, 1, 3])
    starts = np.array([0, 6, 299, 4999, 17, 0, 3, 4096])
    spans = np.array([9, 50, 301, 4097, 5000, 0, 1, 904])
    src = G.Guarded.holding(torch.from_numpy(bank).cuda(), align=16, phase=phase, name="bank")
    power = _out(len(clip), torch.float64, "power")
    K.span_power(src.ptr, bank.size, offsets[clip], np.array(lengths)[clip], starts, spans, power.ptr)
    plain = cscenes.span_power(cda.DeviceClipBank([torch.from_numpy(bank[o:o + n]) for o, n in zip(offsets, lengths)], [0] * 4,
                                              device="cuda"), clip, starts, spans)
    G.check([src, power], {"power": power.float64}, {"power": plain}, "cough_span_power")
    # garbage: offsets and lengths that leave the bank, negative starts and spans
    power = _out(8, torch.float64, "power")
    K.span_power(src.ptr, bank.size, [NEG64, BIG64, bank.size, bank.size - 1, 0, -1, 5300, 10],
                 [5, 5, 5, BIG, BIG, NEG, 100, -3], [0, 1, 2, BIG, NEG, 3, BIG, 0], [10, 10, 10, 4097, 300, 10, 700, NEG], power.ptr)
    _same([src, power], "cough_span_power, garbage")


def test_scene_gains_between_guards():
    p_bg = torch.tensor([0.25, 0.0, float("nan"), 4.0], dtype=torch.float64).cuda()
    p_ev = torch.tensor([1.0, 0.0, float("inf")], dtype=torch.float64).cuda()
    a, b = G.Guarded.holding(p_bg, align=8, name="p_bg"), G.Guarded.holding(p_ev, align=8, name="p_ev")
    scene, power = [0, 1, 2, 3, 3, 3, 0], [0, 0, 0, 1, 2, 0, 0]
    snr = [10.0, 10.0, 10.0, 10.0, 10.0, 4.0, 100.0]
    gain = _out(7, torch.float32, "gain")
    K.scene_gains(a.ptr, [1.0, 1.0, 1.0, 0.5], 4, b.ptr, 3, scene, power, snr, gain.ptr)
    want = torch.tensor([np.sqrt(2.5), 1, 1, 1, 1, 2.0, 5.0], dtype=torch.float32)
    G.check([a, b, gain], {"gain": gain.float32}, {"gain": want}, "cough_scene_gains")
    gain = _out(6, torch.float32, "gain")
    K.scene_gains(a.ptr, [1.0, 1.0, 1.0, 0.5], 4, b.ptr, 3, [-1, 4, BIG, NEG, 0, 0], [0, 0, 0, 0, -1, 3], [10.0] * 6, gain.ptr)
    G.check([a, b, gain], {"gain": gain.float32}, {"gain": torch.ones(6)}, "cough_scene_gains, indices outside")


def _mix_case(rng):
    L = [1, 255, TILE + 1, 2 * TILE + 77]
    bg_len = [3, 1000, 77, 9001]
    ev_len = [1, 30, 200, 12]
    bg = rng.standard_normal(sum(bg_len)).astype(np.float32)
    ev = rng.standard_normal(sum(ev_len)).astype(np.float32)
    bg_off = np.concatenate([[0], np.cumsum(bg_len)[:-1]])
    ev_off = np.concatenate([[0], np.cumsum(ev_len)[:-1]])
    out_off = np.concatenate([[0], np.cumsum(L)[:-1]])
    #        scene 0: one event of the scene's length; scene 1: none; scene 2: up to the tile's end and the last sample; scene 3
    src = [0, 1, 0, 2, 3, 1]
    onset = [0, TILE - 30, TILE, TILE - 100, 2 * TILE - 6, 2 * TILE + 47]
    ev_offsets = [0, 1, 1, 3, 6]
    return dict(L=L, bg=bg, ev=ev, bg_off=bg_off, bg_len=bg_len, starts=[2, 999, 5, 4000], bg_gain=[1.0, 0.5, 2.0, 1.5],
                out_off=out_off, ev_offsets=ev_offsets, src_off=ev_off[src], src_len=np.array(ev_len)[src], onset=onset,
                gains=rng.uniform(0.5, 2, 6).astype(np.float32), n_out=sum(L))


def _mix(c, bg_ptr, ev_ptr, out_ptr, **over):
    a = dict(c)
    a.update(over)
    return K.mix_scenes(bg_ptr, c["bg"].size, a["bg_off"], a["bg_len"], a["starts"], a["bg_gain"], a["L"], a["out_off"],
                        a["ev_offsets"], ev_ptr, c["ev"].size, a["src_off"], a["src_len"], a["onset"], a["gains"],
                        a.get("tiles", scene_tiles(np.array(c["L"]))), out_ptr, c["n_out"])


@pytest.mark.parametrize("phase", [0, 4, 8, 12])
def test_mix_scenes_between_guards(phase):
    c = _mix_case(np.random.default_rng(1))
    bg_t, ev_t = torch.from_numpy(c["bg"]).cuda(), torch.from_numpy(c["ev"]).cuda()
    bg = G.Guarded.holding(bg_t, align=16, phase=phase, name="backgrounds")
    ev = G.Guarded.holding(ev_t, align=16, phase=(phase + 4) % 16, name="events")
    out = G.output(c["n_out"], torch.float32, align=16, phase=(phase + 8) % 16, name="scenes")
    _mix(c, bg.ptr, ev.ptr, out.ptr)
    plain = torch.full((c["n_out"],), -7.0, dtype=torch.float32, device="cuda")
    _mix(c, bg_t.data_ptr(), ev_t.data_ptr(), plain.data_ptr())
    G.check([bg, ev, out], {"scenes": out.float32}, {"scenes": plain}, "cough_mix_scenes")
    assert (plain != -7.0).all()                                           # every sample of every scene was written

    tiles = scene_tiles(np.array(c["L"]))
    garbage = [
        dict(bg_off=[NEG64, BIG64, c["bg"].size - 1, -1], bg_len=[BIG, 5, BIG, NEG]),
        dict(starts=[NEG, BIG, -1, 77], bg_len=[BIG, BIG, 0, 1]),
        dict(L=[BIG, NEG, 3 * TILE, 5], out_off=[c["n_out"] - 3, 0, NEG64, BIG64]),
        dict(out_off=[c["n_out"], c["n_out"] - 1, -1, 17], L=[BIG, BIG, BIG, BIG]),
        dict(ev_offsets=[6, 4, 2, 0, -5]), dict(ev_offsets=[NEG64, BIG64, 0, 6, 6]), dict(ev_offsets=[0, 6, 0, 6, 0]),
        dict(src_off=[NEG64, BIG64, c["ev"].size - 1, -1, c["ev"].size, 200], src_len=[BIG, BIG, BIG, 9, 1, NEG]),
        dict(onset=[NEG, BIG, -5, 2 * TILE, TILE, 0], src_len=[BIG] * 6, ev_offsets=[0, 6, 6, 6, 6]),
        dict(onset=[9000, 8000, 300, 200, 100, NEG], ev_offsets=[0, 0, 0, 0, 6], src_len=[BIG] * 6),
        dict(tiles=np.array([[-1, 0], [4, 0], [BIG, 0], [NEG, 0], [3, -TILE], [3, NEG], [3, BIG], [3, 2 * TILE + 76], [2, 1], [0, 0]])),
        dict(tiles=np.concatenate([tiles, tiles]), onset=[0, 0, 0, 0, 0, 0], src_len=[BIG] * 6, src_off=[0] * 6),
    ]
    for k, over in enumerate(garbage):
        out = G.output(c["n_out"], torch.float32, align=16, phase=(phase + 8) % 16, name="scenes").fill("zeros")
        _mix(c, bg.ptr, ev.ptr, out.ptr, **over)
        G.check([bg, ev, out], {"scenes": out.float32}, {"scenes": out.float32}, f"cough_mix_scenes, garbage {k}: {sorted(over)}")


def _match_case():
    rng = np.random.default_rng(2)
    per = [0, 1, 64, 65, 130]
    prob = np.clip(0.5 + 0.5 * np.sin(np.arange(sum(per)) / 4.0) + rng.normal(0, 0.1, sum(per)), 0, 1).astype(np.float32)
    prob[100] = np.nan
    scores = cda.WindowScores.from_probabilities(prob, per, HOP, WINDOW, SR, 3)
    truth = cda.TruthTable.from_intervals([0, 2, 2, 3, 4, 4, 4], [10, 20000, 150000, 40000, 0, 100000, 400000],
                                          [900, 41000, 170000, 90000, 16000, 130000, 420000], n_clips=5)
    return scores, truth, np.concatenate([np.linspace(0.05, 0.95, 64), [0.0]])


def test_match_events_between_guards():
    scores, truth, thresholds = _match_case()
    want = cda.match_events(scores, truth, thresholds, debounce_seconds=0.25)
    sm = G.Guarded.holding(scores.smoothed, align=8, name="smoothed")
    n, nt, nw = len(scores), len(thresholds), scores.smoothed.numel()
    offs, t_offs = scores.window_offsets.numpy(), truth.offsets

    def run(zero=False, **over):
        a = dict(offs=offs, t_offs=t_offs, k_lo=want.k_lo, k_hi=want.k_hi, onset=truth.onset)
        a.update(over)
        outs = [_out((n, nt), torch.int32, name, zero) for name in ("hits", "false_alarms", "repeats")]
        outs.append(_out((n, nt), torch.int64, "latency", zero))
        K.match_events(sm.ptr, a["offs"], nw, thresholds, want.gap, a["t_offs"], a["k_lo"], a["k_hi"], a["onset"], HOP, WINDOW,
                       *(o.ptr for o in outs))
        return outs
    outs = run()
    G.check([sm] + outs, {o.name: o.view(o.dtype_, n, nt) for o in outs},
            {"hits": want.hits, "false_alarms": want.false_alarms, "repeats": want.repeats, "latency": want.latency_samples},
            "cough_match_events")
    for k, over in enumerate([dict(offs=[NEG64, BIG64, 0, -1, nw + 5, 3]), dict(offs=[nw, 200, 100, 50, 0, 0]),
                              dict(offs=[0, nw, 0, nw, 0, nw]), dict(t_offs=[7, 5, 3, 1, 0, -2]),
                              dict(t_offs=[NEG64, BIG64, 0, 7, 9, BIG64]), dict(t_offs=[0, 7, 0, 7, 0, 7]),
                              dict(k_lo=[NEG, BIG, 5, 4, 3, 2, 1], k_hi=[BIG, NEG, 9, 8, 7, BIG, NEG], onset=[NEG, BIG, 0, -1, 5, 6, 7],
                                   t_offs=[0, 7, 7, 7, 7, 7])]):
        outs = run(**over)                                                 # every (recording, threshold) is written whatever the arrays hold
        _same([sm] + outs, f"cough_match_events, garbage {k}")


def test_list_matches_between_guards():
    scores, truth, _ = _match_case()
    threshold, debounce = 0.4, 0.25
    events = cda.detect_events(scores, threshold, debounce_seconds=debounce)
    want_window, want_class = cscenes.list_matches(scores, truth, threshold, debounce_seconds=debounce, event_counts=events.counts)
    sweep = cda.match_events(scores, truth, [threshold], debounce_seconds=debounce)
    sm = G.Guarded.holding(scores.smoothed, align=8, name="smoothed")
    nw, n_events = scores.smoothed.numel(), len(events)
    assert n_events > 3 and int((want_window >= 0).sum()) > 0
    ev_offs = np.concatenate([[0], np.cumsum(events.counts.numpy())])

    def run(zero=False, **over):
        a = dict(offs=scores.window_offsets.numpy(), t_offs=truth.offsets, k_lo=sweep.k_lo, k_hi=sweep.k_hi, ev_offs=ev_offs)
        a.update(over)
        outs = [_out(len(truth), torch.int32, "truth_window", zero), _out(n_events, torch.int32, "event_class", zero)]
        K.list_matches(sm.ptr, a["offs"], nw, threshold, sweep.gap, a["t_offs"], a["k_lo"], a["k_hi"], outs[0].ptr, a["ev_offs"],
                       n_events, outs[1].ptr)
        return outs
    outs = run()
    G.check([sm] + outs, {"truth_window": outs[0].int32, "event_class": outs[1].int32},
            {"truth_window": want_window, "event_class": want_class}, "cough_list_event_matches")
    for k, over in enumerate([dict(offs=[NEG64, BIG64, 0, -1, nw + 5, 3]), dict(offs=[0, nw, 0, nw, 0, nw]),
                              dict(t_offs=[7, 5, 3, 1, 0, -2]), dict(t_offs=[NEG64, BIG64, 0, 7, 9, BIG64]),
                              dict(ev_offs=[n_events, 3, 2, 1, 0, -1]), dict(ev_offs=[NEG64, BIG64, 0, n_events + 9, 0, BIG64]),
                              dict(ev_offs=[0, n_events, 0, n_events, 0, n_events], k_lo=[NEG] * 7, k_hi=[BIG] * 7)]):
        outs = run(zero=True, **over)                                      # slots outside the clamped offsets stay as they were
        _same([sm] + outs, f"cough_list_event_matches, garbage {k}")
