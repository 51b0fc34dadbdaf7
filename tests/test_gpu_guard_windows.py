"""cough_compose_windows between the guard zones of tests/guarded.py: both banks and the event powers flush against a
trailing guard, the three outputs allocated at exactly their promised sizes, ``d_out`` at every 4-byte phase.  The plans
live on the device, where no host check reaches them: rows with clips, starts, onsets and event counts far outside
anything the banks hold sit between valid rows.  The guards must stay intact, no guard word may reach an output, and the
valid rows must equal the unguarded run bit for bit -- the same then with garbage in the banks' offset and length tables,
where the result is unspecified but stays inside its arrays.  Both kernels run: the one that keeps the background in
registers (300 samples a row) and the one that reads it twice (16385)."""
import numpy as np
import pytest
import torch

import cough_detector_amd as cda
from cough_detector_amd import windows as cwin
import guarded as G
import windows_calls as K

pytestmark = pytest.mark.gpu
BIG, NEG, FAR = 2**31 - 1, -(2**31), 2**30
BIG64, NEG64 = 2**62, -(2**62)
BG_LENGTHS, EV_LENGTHS = [3, 1000, 20001, 77], [1, 30, 200, 12, 17000]


def _case():
    rng = np.random.default_rng(5)
    bg = rng.standard_normal(sum(BG_LENGTHS)).astype(np.float32)
    ev = rng.standard_normal(sum(EV_LENGTHS)).astype(np.float32)
    offsets = lambda lengths: np.concatenate([[0], np.cumsum(lengths)[:-1]])
    return bg, ev, offsets(BG_LENGTHS), offsets(EV_LENGTHS)


def _rows(width):
    """(valid rows, garbage rows) as windows_calls.records takes them."""
    snr = [10.0, 4.0, 2.5, 1.0]
    valid = [(0, 2, 1.0, 1, [0, 0, 0, 0], [0, 0, 0, 0], snr),
             (1, 999, 0.5, 4, [1, 2, 3, 4], [-10, width - 100, 5, -8000], snr),
             (2, 20000, 2.0, 2, [4, 2], [width - 1, -199], snr[:2]),
             (3, 5, 1.5, 0, [0, 0, 0, 0], [0, 0, 0, 0], snr),
             (-1, 0, 1.0, 1, [2, 0, 0, 0], [7, 0, 0, 0], snr)]
    valid = [(b, s, g, n, (c + [0] * 4)[:4], (o + [0] * 4)[:4], (q + [1.0] * 4)[:4]) for b, s, g, n, c, o, q in valid]
    garbage = [(-5, 0, 1.0, 1, [0, 0, 0, 0], [0, 0, 0, 0], snr), (4, 0, 1.0, 1, [0, 0, 0, 0], [0, 0, 0, 0], snr),
               (BIG, BIG, 1.0, 4, [BIG, NEG, -1, 5], [0, 0, 0, 0], snr), (NEG, NEG, 1.0, 4, [4, 4, 4, 4], [FAR, -FAR, BIG, NEG], snr),
               (1, NEG, 1.0, -1, [1, 1, 1, 1], [0, 0, 0, 0], snr), (1, BIG, 1.0, 9, [4, 3, 2, 1], [-FAR, FAR, -16999, width - 1], snr),
               (2, -1, float("nan"), 9, [0, 1, 2, 3], [NEG, BIG, -1, 1], [float("nan"), float("inf"), -1.0, 0.0]),
               (0, 3, float("inf"), BIG, [4, 4, 4, 4], [-17000, -16999, width, width - 1], snr),
               (3, 77, 1.0, NEG, [0, 0, 0, 0], [0, 0, 0, 0], snr)]
    return valid, garbage


@pytest.mark.parametrize("width", [300, 16385])
@pytest.mark.parametrize("phase", [0, 4, 8, 12])
def test_compose_windows_between_guards(phase, width):
    bg, ev, bg_off, ev_off = _case()
    bg_t, ev_t = torch.from_numpy(bg).cuda(), torch.from_numpy(ev).cuda()
    ev_bank = cda.DeviceClipBank([torch.from_numpy(ev[o:o + n]) for o, n in zip(ev_off, EV_LENGTHS)], [1] * len(EV_LENGTHS), device="cuda")
    p_ev_t = cwin.event_powers(ev_bank)
    valid, garbage = _rows(width)
    rows = [valid[0], garbage[0], garbage[1], valid[1], garbage[2], garbage[3], valid[2], garbage[4], garbage[5], valid[3],
            garbage[6], garbage[7], valid[4], garbage[8]]
    where = [0, 3, 6, 9, 12]                                               # the valid rows among them
    rec, n = K.records(rows), len(rows)

    # the normal path: the valid rows alone, ordinary tensors
    plain = torch.full((len(valid), width), -7.0, dtype=torch.float32, device="cuda")
    plain_p, plain_g = torch.empty(len(valid), dtype=torch.float64, device="cuda"), torch.empty((len(valid), 4), dtype=torch.float32, device="cuda")
    K.compose_windows(bg_t.data_ptr(), bg.size, bg_off, BG_LENGTHS, ev_t.data_ptr(), ev.size, ev_off, EV_LENGTHS, p_ev_t.data_ptr(),
                      K.records(valid), width, plain.data_ptr(), plain_p.data_ptr(), plain_g.data_ptr())
    assert (plain != -7.0).all() and float(plain_p[4]) == 0.0 and float(plain_g[1].min()) > 0

    bank = G.Guarded.holding(bg_t, align=16, phase=(phase + 4) % 16, name="backgrounds")
    clips = G.Guarded.holding(ev_t, align=16, phase=(phase + 8) % 16, name="events")
    powers = G.Guarded.holding(p_ev_t, align=8, name="event powers")

    def run(**tables):
        t = dict(bg_off=bg_off, bg_len=BG_LENGTHS, ev_off=ev_off, ev_len=EV_LENGTHS)
        t.update(tables)
        out = G.output((n, width), torch.float32, align=16, phase=phase, name="windows")
        p_bg, gains = G.output(n, torch.float64, name="p_bg"), G.output((n, 4), torch.float32, name="gains")
        K.compose_windows(bank.ptr, bg.size, t["bg_off"], t["bg_len"], clips.ptr, ev.size, t["ev_off"], t["ev_len"], powers.ptr, rec,
                          width, out.ptr, p_bg.ptr, gains.ptr)
        return out, p_bg, gains

    out, p_bg, gains = run()
    got = {"windows": out.view(torch.float32, n, width), "p_bg": p_bg.float64, "gains": gains.view(torch.float32, n, 4)}
    G.check([bank, clips, powers, out, p_bg, gains], got, got, "cough_compose_windows, garbage plans")     # guards, no guard word
    G.check([], {"windows": got["windows"][where], "p_bg": got["p_bg"][where], "gains": got["gains"][where]},
            {"windows": plain, "p_bg": plain_p, "gains": plain_g}, "cough_compose_windows, the valid rows")
    # what the header says of clamped rows: a background outside its bank is silence, an event outside its bank is skipped
    assert float(got["p_bg"][1]) == 0.0 and float(got["p_bg"][2]) == 0.0
    assert float(got["windows"][1][0]) == float(ev[0]) and (got["windows"][1][1:] == 0).all()      # its one-sample event, gain 1
    assert got["gains"][4].tolist() == [1.0] * 4 and got["gains"][7].tolist() == [0.0] * 4 and (got["gains"][8] != 0).all()

    for k, tables in enumerate([dict(bg_off=[NEG64, BIG64, bg.size - 1, -1], bg_len=[BIG, 5, BIG, NEG]),
                                dict(bg_off=[bg.size, 0, 5, bg.size - 2], bg_len=[1, BIG, 0, BIG]),
                                dict(ev_off=[NEG64, BIG64, ev.size - 1, -1, ev.size], ev_len=[BIG, BIG, BIG, 9, 1]),
                                dict(ev_off=[0, 0, 0, 0, 200], ev_len=[NEG, 0, BIG, BIG, BIG])]):
        out, p_bg, gains = run(**tables)
        got = {"windows": out.float32, "p_bg": p_bg.float64, "gains": gains.float32}
        G.check([bank, clips, powers, out, p_bg, gains], got, got, f"cough_compose_windows, garbage tables {k}")
