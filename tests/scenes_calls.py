"""Direct calls of libcough_amd_scenes.so for the GPU suites: the small index arrays go up as ordinary tensors, the
float banks and every output are whatever pointers the test owns (guarded or not)."""
import numpy as np
import torch

from cough_detector_amd import _lib


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).cuda()


def ptr(t):
    return None if t is None else (t if isinstance(t, int) else t.data_ptr())


def span_power(bank_ptr, n_bank, offsets, lengths, starts, spans, power_ptr):
    keep = [dev(offsets, np.int64), dev(lengths, np.int32), dev(starts, np.int32), dev(spans, np.int32)]
    _lib.check_scenes(_lib.load_scenes().cough_span_power(bank_ptr, n_bank, *(t.data_ptr() for t in keep), len(spans),
                                                          power_ptr, None), "cough_span_power")
    return keep


def scene_gains(p_bg_ptr, bg_gain, n_scenes, p_ev_ptr, n_powers, event_scene, event_power, snr_linear, gain_ptr):
    keep = [dev(bg_gain, np.float32), dev(event_scene, np.int32), dev(event_power, np.int32), dev(snr_linear, np.float64)]
    _lib.check_scenes(_lib.load_scenes().cough_scene_gains(p_bg_ptr, keep[0].data_ptr(), n_scenes, p_ev_ptr, n_powers,
                                                           keep[1].data_ptr(), keep[2].data_ptr(), keep[3].data_ptr(),
                                                           len(event_scene), gain_ptr, None), "cough_scene_gains")
    return keep


def mix_scenes(bg_ptr, n_bg, bg_offsets, bg_lengths, bg_starts, bg_gains, scene_lengths, out_offsets, ev_offsets, ev_ptr, n_ev,
               src_offsets, src_lengths, onsets, gains, tiles, out_ptr, n_out):
    """``gains``: a device float32 tensor, a pointer, or host values."""
    n, m = len(scene_lengths), len(onsets)
    if not isinstance(gains, (int, torch.Tensor)):
        gains = dev(gains, np.float32)
    keep = [dev(bg_offsets, np.int64), dev(bg_lengths, np.int32), dev(bg_starts, np.int32), dev(bg_gains, np.float32),
            dev(scene_lengths, np.int32), dev(out_offsets, np.int64), dev(ev_offsets, np.int64), dev(src_offsets, np.int64),
            dev(src_lengths, np.int32), dev(onsets, np.int32), dev(np.asarray(tiles).reshape(-1), np.int32), gains]
    p = [t.data_ptr() for t in keep[:11]]
    _lib.check_scenes(_lib.load_scenes().cough_mix_scenes(
        bg_ptr, n_bg, p[0], p[1], p[2], p[3], p[4], p[5], p[6], n, ev_ptr, n_ev, p[7], p[8], p[9], ptr(gains), m, p[10],
        len(np.asarray(tiles).reshape(-1)) // 2, out_ptr, n_out, None), "cough_mix_scenes")
    return keep


def match_events(smoothed_ptr, window_offsets, n_windows, thresholds, gap, truth_offsets, k_lo, k_hi, onset, hop, window,
                 hits_ptr, fas_ptr, reps_ptr, late_ptr):
    keep = [dev(window_offsets, np.int64), dev(thresholds, np.float64), dev(truth_offsets, np.int64), dev(k_lo, np.int32),
            dev(k_hi, np.int32), dev(onset, np.int32)]
    p = [t.data_ptr() for t in keep]
    _lib.check_scenes(_lib.load_scenes().cough_match_events(
        smoothed_ptr, p[0], len(window_offsets) - 1, n_windows, p[1], len(thresholds), gap, p[2], p[3], p[4], p[5], len(k_lo),
        hop, window, hits_ptr, fas_ptr, reps_ptr, late_ptr, None), "cough_match_events")
    return keep


def list_matches(smoothed_ptr, window_offsets, n_windows, threshold, gap, truth_offsets, k_lo, k_hi, truth_window_ptr,
                 event_offsets, n_events, event_class_ptr):
    keep = [dev(window_offsets, np.int64), dev(truth_offsets, np.int64), dev(k_lo, np.int32), dev(k_hi, np.int32),
            dev(event_offsets, np.int64)]
    p = [t.data_ptr() for t in keep]
    _lib.check_scenes(_lib.load_scenes().cough_list_event_matches(
        smoothed_ptr, p[0], len(window_offsets) - 1, n_windows, float(threshold), gap, p[1], p[2], p[3], len(k_lo),
        truth_window_ptr, p[4], n_events, event_class_ptr, None), "cough_list_event_matches")
    return keep
