"""Direct calls of libcough_amd_windows.so for the GPU suites: the tables and the plans go up as ordinary tensors, the
float banks and every output are whatever pointers the test owns (guarded or not)."""
import numpy as np
import torch

from cough_detector_amd import _lib
from cough_detector_amd.windows import PLAN_DTYPE


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).cuda()


def records(rows):
    """``cough_window_plan`` records from ``[(background, bg_start, bg_gain, n_events, [clip] * 4, [onset] * 4,
    [snr_linear] * 4)]``: whatever values, nothing is checked."""
    rec = np.zeros(len(rows), dtype=PLAN_DTYPE)
    for r, (b, start, gain, n, clip, onset, snr) in enumerate(rows):
        rec[r] = (b, start, gain, n, clip, onset, snr)
    return rec


def compose_windows(bg_ptr, n_bg, bg_offsets, bg_lengths, ev_ptr, n_ev, ev_offsets, ev_lengths, p_ev_ptr, rec, width, out_ptr,
                    p_bg_ptr=None, gains_ptr=None):
    keep = [dev(bg_offsets, np.int64), dev(bg_lengths, np.int32), dev(ev_offsets, np.int64), dev(ev_lengths, np.int32),
            torch.from_numpy(rec.view(np.int64).reshape(-1).copy()).cuda()]
    p = [t.data_ptr() for t in keep]
    _lib.check_windows(_lib.load_windows().cough_compose_windows(
        bg_ptr, n_bg, p[0], p[1], len(bg_lengths), ev_ptr, n_ev, p[2], p[3], p_ev_ptr, len(ev_lengths), p[4], len(rec), width,
        out_ptr, p_bg_ptr, gains_ptr, None), "cough_compose_windows")
    return keep
