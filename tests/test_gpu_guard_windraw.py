"""``cough_draw_window_plans`` between the guard zones of tests/guarded.py: every table it reads ends flush against a
trailing guard, the records and the labels sit in regions of exactly their sizes, and the run ends with guards intact, no
guard word in an output and the restatement's bits (tests/windraw_ref.py)."""
import numpy as np
import pytest
import torch

from cough_detector_amd import _lib
from cough_detector_amd.data import _stream
import guarded as G
import windraw_ref as D

pytestmark = pytest.mark.gpu
T = D.THREADS
BG = (48000, 7, 20000)
EV, LAB = (1600, 3000, 800, 1, 5000, 2400, 40000), (1, 1, 1, 1, 0, 0, 1)


def _table(values, dtype, name):
    """A guarded input whose last element is flush against the trailing guard, aligned to its element and no further."""
    arr = np.ascontiguousarray(values, dtype=dtype)
    g = G.Guarded(arr.nbytes, arr.itemsize, name=name)
    g.view(torch.int32 if arr.itemsize == 4 else torch.float64).copy_(torch.from_numpy(arr))
    return g


@pytest.mark.parametrize("b", [1, T - 1, T, T + 1, 2 * T + 1])
@pytest.mark.parametrize("chain", [False, True])
def test_the_draw_stays_inside_its_tables_and_its_outputs(b, chain):
    kw = dict(p_cough=0.8, p_distractor=0.9, coughs_per_window=(1, 4), bg_gain_range=(0.5, 2.0))
    if chain:
        kw.update(margin=3521, rho_min=16000 / 17600)
    a = D.arguments(BG, EV, LAB, 16000, **kw)
    want, want_labels = D.draw_batch(b + 40, b, a)
    bgl, evl = _table(BG, np.int32, "background lengths"), _table(EV, np.int32, "event lengths")
    coughs, others = _table(a["coughs"], np.int32, "cough clips"), _table(a["others"], np.int32, "distractor clips")
    snr = _table(a["snr"], np.float64, "snr levels")
    records = G.Guarded(b * 80, 8, name="records")
    labels = G.output((b,), torch.int64, name="labels")
    dev = torch.device("cuda", torch.cuda.current_device())
    _lib.check_windraw(_lib.load_windraw().cough_draw_window_plans(
        b + 40, b, 16000, bgl.ptr, len(BG), evl.ptr, len(EV), coughs.ptr, a["coughs"].size, others.ptr, a["others"].size,
        a["p_cough"], a["c_lo"], a["c_hi"], a["p_distractor"], a["g_lo"], a["g_hi"], snr.ptr, a["m"], a["margin"], a["rho_min"],
        records.ptr, labels.ptr, _stream(dev)), "cough_draw_window_plans")
    torch.cuda.synchronize()
    G.check([bgl, evl, coughs, others, snr, records, labels],
            {"records": records.int32, "labels": labels.int64},
            {"records": torch.from_numpy(want.view(np.int32).copy()), "labels": torch.from_numpy(want_labels)},
            what=f"{b} rows, chain={chain}")
