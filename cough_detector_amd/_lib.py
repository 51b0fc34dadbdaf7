"""ctypes binding of the native libraries: one ``Library`` record per shared object, in ``LIBRARIES``.

A record's name gives everything regular about it: the file ``libcough_amd[_NAME].so`` beside this module (or the path in
the environment variable ``COUGH_AMD[_NAME]_LIB``), the C-ABI header ``include/cough_amd[_NAME].h`` and the entry points
``cough_NAME_abi_version`` / ``cough_NAME_last_error`` (``amd``, the main library, carries no suffix).  What is its own is
the ABI version it must report and its prototypes.  ``load`` / ``check`` bind the main library's record, ``load_NAME`` /
``check_NAME`` a companion's; ``NAME_SYMBOLS`` are the prototypes' names.

There are two tables.  ``LIBRARIES`` is closed: its nine records, their order, symbol counts and ABI versions are pinned by
``tests/test_libraries_host.py``, which later work must leave as it is.  ``LATER`` is open-ended: a library that comes
after the nine gets its record there (``build.LATER_UNITS`` is its counterpart), with the same naming rules and the same
module-level names ``load_NAME`` / ``check_NAME`` / ``NAME_SYMBOLS`` / ``NAME_LIB_PATH``.
``LATER`` is pinned too by now (``tests/test_slices_host.py``), so the libraries after it get their records in ``OPEN``
(``build.OPEN_UNITS``): same rules, same module-level names, and tests only ever ask whether their own library is in it.

There is no CPU fallback: if the shared object is missing or a call fails, this raises.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

HERE = os.path.dirname(os.path.abspath(__file__))

OK, EINVAL, EUNSUPPORTED, EHIP, EWORKSPACE = 0, 1, 2, 3, 4
FEAT_NORMALIZE = 1
PATH_GENERIC, PATH_TUNED, PATH_TUNED_FULLBAND, PATH_TUNED_GEOMETRY = 0, 1, 2, 3
SPEC_MAGNITUDE, SPEC_FULL_WINDOW = 1, 2
DTYPE_FP32, DTYPE_BF16, DTYPE_BF16X3 = 0, 1, 3
DTYPES = {"fp32": DTYPE_FP32, "bf16_approx": DTYPE_BF16, "bf16x3": DTYPE_BF16X3}
APPROX_NOTE = ("compute_dtype='bf16' selects the APPROXIMATE single-bf16 mode (bf16 operands and activations): at a trained "
               "head's scale its logits are 0.05-0.3 away from the f32 reference, far outside the 1e-3 parity tolerance. "
               "Pass 'bf16_approx' to say that is intended; the parity-grade modes are 'bf16x3' (residual net) and 'fp32'.")


def normalize_dtype(compute_dtype: str, allowed) -> str:
    """'bf16' is kept as an alias of 'bf16_approx' that warns: nobody gets the approximate mode without being told."""
    if compute_dtype == "bf16" and "bf16_approx" in allowed:
        import warnings
        warnings.warn(APPROX_NOTE, UserWarning, stacklevel=4)
        return "bf16_approx"
    if compute_dtype not in allowed:
        names = ", ".join(repr(a) for a in allowed if not a.startswith("_"))
        raise ValueError(f"compute_dtype must be one of {names}, got {compute_dtype!r}")
    return compute_dtype


EPOCH_METER_BYTES = 64   # COUGH_EPOCH_METER_BYTES
PREP_NORMALIZE = 1       # COUGH_PREP_NORMALIZE
MAX_MASKS = 16           # COUGH_MAX_MASKS
MAX_SEGMENTS = 16        # COUGH_MAX_SEGMENTS
MAX_FRAME_LENGTH = 4096  # COUGH_MAX_FRAME_LENGTH
MAX_SMOOTHING = 32       # COUGH_MAX_SMOOTHING
MAX_THRESHOLDS = 1024    # COUGH_MAX_THRESHOLDS
WARP_MAX_RATE, WARP_MAX_RATIO = 1 << 20, 4   # COUGH_WARP_MAX_RATE / COUGH_WARP_MAX_RATIO
PITCH_MAX_LENGTH, PITCH_MAX_SAMPLES, PITCH_MAX_STEPS = 1 << 20, 1 << 21, 12   # COUGH_PITCH_MAX_LENGTH / _SAMPLES / _STEPS
MAX_CONTRAST_BANDS = 16
TRAIN_NUM_PARAMS, TRAIN_NUM_RUNNING = 290370, 1216   # COUGH_TRAIN_NUM_PARAMS / COUGH_TRAIN_NUM_RUNNING
TRAIN_SMALL_NUM_PARAMS, TRAIN_SMALL_NUM_RUNNING = 21122, 480   # COUGH_TRAIN_SMALL_NUM_PARAMS / _NUM_RUNNING
TRAIN_STD_NUM_PARAMS, TRAIN_STD_NUM_RUNNING = 421954, 960      # COUGH_TRAIN_STD_NUM_PARAMS / _NUM_RUNNING


class FeatConfig(C.Structure):
    _fields_ = [("sample_rate", C.c_int), ("n_fft", C.c_int), ("hop_length", C.c_int), ("win_length", C.c_int),
                ("n_mels", C.c_int), ("n_mfcc", C.c_int), ("segment_samples", C.c_int),
                ("use_pre_emphasis", C.c_int), ("pre_emphasis_coef", C.c_float), ("use_delta_delta", C.c_int),
                ("use_pcen", C.c_int), ("use_mfcc", C.c_int), ("use_spectral_contrast", C.c_int),
                ("n_contrast_bands", C.c_int), ("contrast_edges", C.c_int * (MAX_CONTRAST_BANDS + 2))]


_FP = C.POINTER(C.c_float)


class ConvBN(C.Structure):
    _fields_ = [("w", _FP), ("b", _FP), ("bn_w", _FP), ("bn_b", _FP), ("bn_mean", _FP), ("bn_var", _FP)]


class ResBlockWeights(C.Structure):
    _fields_ = [("conv1", ConvBN), ("conv2", ConvBN), ("skip", ConvBN)]


class ResNetWeights(C.Structure):
    _fields_ = [("stem", ConvBN), ("block", ResBlockWeights * 2), ("fc_w", _FP), ("fc_b", _FP), ("bn_eps", C.c_float)]


class CnnBlock(C.Structure):
    _fields_ = [("cin", C.c_int), ("cout", C.c_int), ("ksize", C.c_int), ("dw_w", _FP), ("dw_b", _FP),
                ("conv", ConvBN), ("pool", C.c_int)]


class CnnWeights(C.Structure):
    _fields_ = [("n_blocks", C.c_int), ("blocks", C.POINTER(CnnBlock)), ("hidden", C.c_int), ("fc1_w", _FP),
                ("fc1_b", _FP), ("fc2_w", _FP), ("fc2_b", _FP), ("bn_eps", C.c_float)]


class CoughAugClip(C.Structure):
    """cough_aug_clip: one clip's draws of AudioAugmentor.augment."""
    _fields_ = [("shift", C.c_int), ("gain", C.c_float), ("gaussian", C.c_int), ("bank_index", C.c_int),
                ("gaussian_snr_db", C.c_double), ("bank_snr_db", C.c_double), ("bank_start", C.c_longlong)]


class CoughWarpPlan(C.Structure):
    """cough_warp_plan: one row's time shift and rate pair."""
    _fields_ = [("shift", C.c_int), ("orig", C.c_int), ("new_rate", C.c_int)]


class CoughStretchPlan(C.Structure):
    """cough_stretch_plan: one row's time shift and stretch rate."""
    _fields_ = [("shift", C.c_int), ("reserved", C.c_int), ("rate", C.c_double)]


class CoughPitchStep(C.Structure):
    """cough_pitch_step: the draw table's entry for one number of semitones."""
    _fields_ = [("rate", C.c_double), ("orig", C.c_int), ("reserved", C.c_int)]


def _raise(status: int, what: str, msg: str) -> None:
    if status in (EINVAL, EUNSUPPORTED):
        raise ValueError(f"{what}: {msg}")
    raise RuntimeError(f"{what}: {msg} (status {status})")


VOID = object()   # a prototype's restype for a function that returns nothing (None leaves ctypes' default, int)
_lock = threading.Lock()


class Library:
    """One shared object: where it is, the ABI version it must report, and its prototypes, an ordered mapping
    ``symbol -> (restype, argtypes)`` of every entry point its header declares.  ``None`` leaves ctypes' default.
    ``handle`` is the loaded ``CDLL`` (``None`` until ``load``), ``path`` the file ``load`` opens."""

    def __init__(self, name: str, abi: int, prototypes: dict):
        tag = "" if name == "amd" else "_" + name
        self.name, self.abi, self.prototypes = name, abi, prototypes
        self.soname = f"libcough_amd{tag}.so"
        # COUGH_AMD[_NAME]_LIB: alternative build of the same ABI (same-box A/B timing of kernel variants)
        self.path = os.environ.get(f"COUGH_AMD{tag.upper()}_LIB") or os.path.join(HERE, self.soname)
        self.abi_symbol, self.error_symbol = f"cough_{name}_abi_version", f"cough_{name}_last_error"
        self.symbols = tuple(prototypes)
        self.handle = None

    def load(self) -> C.CDLL:
        """Load (once) and type the library; raise loudly if it is not built."""
        if self.handle is not None:
            return self.handle
        with _lock:
            if self.handle is not None:
                return self.handle
            if not os.path.exists(self.path):
                raise RuntimeError(
                    f"{self.path} is missing: the HIP extension is not built. Run `python -m cough_detector_amd.build` "
                    "(needs hipcc / ROCm, target gfx950). There is no CPU fallback.")
            lib = C.CDLL(self.path)
            for symbol, (restype, argtypes) in self.prototypes.items():
                fn = getattr(lib, symbol)
                if restype is not None:
                    fn.restype = None if restype is VOID else restype
                if argtypes is not None:
                    fn.argtypes = argtypes
            if getattr(lib, self.abi_symbol)() != self.abi:
                raise RuntimeError(f"{self.soname} ABI version mismatch; rebuild it")
            self.handle = lib
        return self.handle

    def check(self, status: int, what: str) -> None:
        """Map a C status to the reference's exception convention (ValueError for argument/config errors, as
        src/model.py:313-314; RuntimeError otherwise), with this library's own last-error message."""
        if status != OK:
            _raise(status, what, getattr(self.load(), self.error_symbol)().decode("utf-8", "replace"))


def _libraries() -> dict:
    vp, ll, i, f, d, ull, sz, s = (C.c_void_p, C.c_longlong, C.c_int, C.c_float, C.c_double, C.c_ulonglong, C.c_size_t,
                                   C.c_char_p)
    P = C.POINTER
    step = [vp, i, i, i, vp, vp, vp, ull, ull, f, vp, vp, vp, vp, f, f, vp, vp, vp, vp, sz, vp]
    step_std = [vp, i, i, i, vp, vp, vp, ull, ull, f, f, vp, vp, vp, vp, f, f, vp, vp, vp, vp, sz, vp]
    return {lib.name: lib for lib in (
        # include/cough_amd.h, ABI v5: it stays at its 53 entry points, what came later lives in the companions
        Library("amd", 5, {
            "cough_amd_abi_version": (i, None), "cough_amd_arch": (s, None), "cough_amd_last_error": (s, None),
            "cough_featurizer_create": (None, [P(vp), P(FeatConfig), _FP, _FP, _FP]),
            "cough_featurizer_destroy": (VOID, [vp]),
            "cough_featurizer_num_features": (None, [vp]),
            "cough_featurizer_num_frames": (None, [vp]),
            "cough_featurizer_path": (None, [vp]),
            "cough_featurize": (None, [vp, vp, ll, vp, i, i, vp]),
            "cough_featurizer_workspace_bytes": (sz, [vp, i]),
            "cough_featurize_ws": (None, [vp, vp, ll, vp, i, i, vp, sz, vp]),
            "cough_spectrogram": (None, [vp, vp, ll, vp, i, i, vp]),
            "cough_featurizer_num_frames_for": (None, [vp, i]),
            "cough_featurizer_workspace_bytes_for": (sz, [vp, i, i]),
            "cough_featurize_any": (None, [vp, vp, ll, i, vp, i, i, vp, sz, vp]),
            "cough_spectrogram_any": (None, [vp, vp, ll, i, vp, i, i, vp]),
            "cough_resnet_create": (None, [P(vp), P(ResNetWeights), i]),
            "cough_resnet_create_ex": (None, [P(vp), i, P(i), P(ConvBN), P(ResBlockWeights), _FP, _FP, f, i]),
            "cough_resnet_destroy": (VOID, [vp]),
            "cough_resnet_workspace_bytes": (sz, [vp, i, i, i]),
            "cough_resblock_create": (None, [P(vp), i, i, i, P(ConvBN), P(ConvBN), P(ConvBN), f]),
            "cough_resblock_destroy": (VOID, [vp]),
            "cough_resblock_workspace_bytes": (sz, [vp, i, i, i]),
            "cough_resblock_out_shape": (None, [vp, i, i, P(i), P(i)]),
            "cough_resblock_forward": (None, [vp, vp, i, i, i, vp, vp, sz, vp]),
            "cough_resnet_forward": (None, [vp, vp, i, i, i, vp, vp, vp, vp, sz, vp]),
            "cough_resnet_read_activation": (None, [vp, vp, i, i, i, i, vp, vp]),
            "cough_cnn_create": (None, [P(vp), P(CnnWeights), i]),
            "cough_cnn_destroy": (VOID, [vp]),
            "cough_cnn_workspace_bytes": (sz, [vp, i, i, i]),
            "cough_cnn_forward": (None, [vp, vp, i, i, i, vp, vp, vp, vp, sz, vp]),
            "cough_cnn_conv_output": (None, [vp, vp, i, i, i, vp, vp, sz, vp]),
            "cough_pipeline_workspace_bytes": (sz, [vp, vp, i]),
            "cough_pipeline_forward": (None, [vp, vp, vp, ll, i, i, vp, vp, vp, vp, vp, sz, vp, vp, vp]),
            "cough_mask_axes": (None, [vp, vp, ll, i, i, i, P(i), P(i), P(i), vp]),
            "cough_prepare_clip": (None, [vp, ll, i, i, vp, i, i, vp]),
            "cough_resample": (None, [vp, ll, i, i, vp, i, i, i, vp, ll, i, vp]),
            "cough_ring_write": (None, [vp, i, vp, i, vp, vp, i, vp]),
            "cough_window_gather": (None, [vp, i, vp, vp, i, i, vp, vp]),
            "cough_synth_clips": (None, [vp, ll, i, ll, ll, vp]),
            "cough_pre_emphasis": (None, [vp, ll, vp, ll, i, i, f, vp]),
            "cough_compute_deltas": (None, [vp, vp, ll, i, vp]),
            "cough_pcen": (None, [vp, vp, ll, i, f, f, f, f, vp]),
            "cough_augment_workspace_bytes": (sz, [i]),
            "cough_augment_waveforms": (None, [vp, ll, vp, i, i, P(i), P(CoughAugClip), vp, ll, P(ll), P(i), i, vp, ull,
                                               vp, sz, vp]),
            "cough_mix_rows": (None, [vp, vp, vp, vp, ll, ll, vp, vp]),
            "cough_train_workspace_bytes": (sz, [i, i, i]),
            "cough_train_forward_backward": (None, step),
            "cough_adamw_step": (None, [vp, vp, vp, vp, ll, f, f, f, f, f, f, d, d, vp, vp]),
            "cough_train_small_workspace_bytes": (sz, [i, i, i]),
            "cough_train_small_forward_backward": (None, step),
            "cough_train_std_workspace_bytes": (sz, [i, i, i]),
            "cough_train_std_forward_backward": (None, step_std),
        }),
        # include/cough_amd_loop.h: what the epoch loop adds
        Library("loop", 1, {
            "cough_loop_abi_version": (i, None), "cough_loop_last_error": (s, None),
            "cough_epoch_meter_update": (None, [vp, vp, i, vp, vp, vp, vp, vp]),
        }),
        # include/cough_amd_data.h: the input pipeline
        Library("data", 1, {
            "cough_data_abi_version": (i, None), "cough_data_last_error": (s, None),
            "cough_gather_rows": (None, [vp, vp, vp, i, vp, ll, i, vp]),
            "cough_prepare_rows": (None, [vp, vp, vp, i, vp, i, i, vp]),
            "cough_mask_images": (None, [vp, vp, i, i, i, i, vp, vp, vp, vp]),
        }),
        # include/cough_amd_segments.h: corpus curation
        Library("segments", 1, {
            "cough_segments_abi_version": (i, None), "cough_segments_last_error": (s, None),
            "cough_frame_energy_tile_frames": (None, [i, i]),
            "cough_frame_energy": (None, [vp, vp, vp, vp, i, vp, i, i, i, vp, vp]),
            "cough_pick_segments": (None, [vp, vp, vp, i, i, i, i, i, i, d, d, vp, vp, vp, vp, vp]),
            "cough_copy_segments": (None, [vp, vp, vp, vp, vp, i, i, vp, vp]),
        }),
        # include/cough_amd_score.h: offline scoring
        Library("score", 1, {
            "cough_score_abi_version": (i, None), "cough_score_last_error": (s, None),
            "cough_smooth_windows": (None, [vp, vp, i, ll, i, vp, vp]),
            "cough_sweep_thresholds": (None, [vp, vp, i, ll, vp, i, i, vp, vp, vp, vp, vp]),
            "cough_list_events": (None, [vp, vp, i, ll, d, i, vp, ll, vp, vp, vp]),
        }),
        # include/cough_amd_draws.h: a batch's draws on the device
        Library("draws", 1, {
            "cough_draws_abi_version": (i, None), "cough_draws_last_error": (s, None),
            "cough_draw_batch": (None, [ull, i, vp, d, i, vp, d, i, i, i, i, i, i, vp, vp, vp, vp, vp]),
            "cough_augment_rows_drawn_workspace_bytes": (sz, [i]),
            "cough_augment_rows_drawn": (None, [vp, vp, vp, i, i, vp, vp, ll, vp, vp, i, ull, vp, vp, sz, vp]),
        }),
        # include/cough_amd_soft.h: the training steps on soft targets and the batch MixUp.  The steps take the argument
        # lists of the v5 steps, with the soft targets where the class indices were
        Library("soft", 1, {
            "cough_soft_abi_version": (i, None), "cough_soft_last_error": (s, None),
            "cough_train_forward_backward_soft": (None, step),
            "cough_train_small_forward_backward_soft": (None, step),
            "cough_train_std_forward_backward_soft": (None, step_std),
            "cough_mix_batch": (None, [vp, vp, vp, vp, i, ll, vp, vp, vp]),
        }),
        # include/cough_amd_warp.h: speed perturbation
        Library("warp", 1, {
            "cough_warp_abi_version": (i, None), "cough_warp_last_error": (s, None),
            "cough_warp_rows": (None, [vp, vp, vp, i, vp, vp, i, vp, vp]),
            "cough_draw_speed": (None, [ull, i, vp, d, d, d, i, vp, vp, vp]),
            "cough_clear_shifts": (None, [vp, i, vp]),
        }),
        # include/cough_amd_pitch.h: the pitch shift's time stretch
        Library("pitch", 1, {
            "cough_pitch_abi_version": (i, None), "cough_pitch_last_error": (s, None),
            "cough_stretch_rows": (None, [vp, vp, vp, i, vp, vp, i, vp, vp]),
            "cough_draw_pitch": (None, [ull, i, vp, d, i, i, vp, i, vp, vp, vp, vp]),
        }),
    )}


def _later() -> dict:
    vp, i, d, s = C.c_void_p, C.c_int, C.c_double, C.c_char_p
    return {lib.name: lib for lib in (
        # include/cough_amd_slices.h: fixed-length windows of long recordings, kept by their activity
        Library("slices", 1, {
            "cough_slices_abi_version": (i, None), "cough_slices_last_error": (s, None),
            "cough_window_activity": (None, [vp, vp, vp, vp, i, i, i, i, i, i, d, d, d, vp, vp, vp, vp, vp, vp]),
            "cough_list_windows": (None, [vp, vp, vp, vp, vp, i, i, i, vp, vp, vp, vp, vp]),
        }),
    )}


def _open() -> dict:
    vp, i, s, sz, ll, d = C.c_void_p, C.c_int, C.c_char_p, C.c_size_t, C.c_longlong, C.c_double
    match = [vp, vp, i, i, i, i, i]                  # words, live, n, Tw, L, max_err_1024, min_live
    walk = [vp, vp, i, ll]                           # smoothed, window offsets, n_clips, n_windows
    return {lib.name: lib for lib in (
        # include/cough_amd_dups.h: binary fingerprints of the feature images and the all-pairs matcher
        Library("dups", 1, {
            "cough_dups_abi_version": (i, None), "cough_dups_last_error": (s, None),
            "cough_fingerprint_images": (None, [vp, i, i, i, C.POINTER(i), i, i, vp, vp, vp]),
            "cough_match_workspace_bytes": (sz, [i, i]),
            "cough_count_matches": (None, match + [vp, vp, vp, sz, vp]),
            "cough_list_matches": (None, match + [vp, sz, vp, vp, vp, vp, vp, vp, vp]),
        }),
        # include/cough_amd_scenes.h: soundscapes with known cough times, detections matched to them
        Library("scenes", 1, {
            "cough_scenes_abi_version": (i, None), "cough_scenes_last_error": (s, None),
            "cough_span_power": (None, [vp, ll, vp, vp, vp, vp, i, vp, vp]),
            "cough_scene_gains": (None, [vp, vp, i, vp, i, vp, vp, vp, i, vp, vp]),
            "cough_mix_scenes": (None, [vp, ll, vp, vp, vp, vp, vp, vp, vp, i, vp, ll, vp, vp, vp, vp, i, vp, i, vp, ll, vp]),
            "cough_match_events": (None, walk + [vp, i, i, vp, vp, vp, vp, i, i, i, vp, vp, vp, vp, vp]),
            "cough_list_event_matches": (None, walk + [d, i, vp, vp, vp, i, vp, vp, ll, vp, vp]),
        }),
        # include/cough_amd_reverb.h: room reverberation, FFT convolution with a prepared bank of impulse responses
        Library("reverb", 1, {
            "cough_reverb_abi_version": (i, None), "cough_reverb_last_error": (s, None),
            "cough_reverb_bank_bytes": (sz, [i]),
            "cough_reverb_prepare": (None, [vp, C.POINTER(ll), C.POINTER(i), i, vp, sz, vp]),
            "cough_reverb_rows": (None, [vp, vp, vp, i, vp, vp, i, vp, i, vp]),
            "cough_draw_reverb": (None, [C.c_ulonglong, i, vp, d, i, vp, vp]),
        }),
        # include/cough_amd_channel.h: the capture channel, a biquad cascade out of a prepared bank and a hard clip
        Library("channel", 1, {
            "cough_channel_abi_version": (i, None), "cough_channel_last_error": (s, None),
            "cough_channel_bank_bytes": (sz, [i]),
            "cough_channel_prepare": (None, [C.POINTER(d), C.POINTER(i), i, vp, sz, vp]),
            "cough_channel_rows": (None, [vp, vp, vp, i, vp, vp, i, vp, i, vp]),
            "cough_draw_channel": (None, [C.c_ulonglong, i, d, i, d, d, d, vp, vp]),
        }),
        # include/cough_amd_windows.h: a batch of training windows composed in one launch
        Library("windows", 1, {
            "cough_windows_abi_version": (i, None), "cough_windows_last_error": (s, None),
            "cough_compose_windows": (None, [vp, ll, vp, vp, i, vp, ll, vp, vp, vp, i, vp, i, i, vp, vp, vp, vp]),
        }),
        # include/cough_amd_windraw.h: a batch's window plans and labels drawn on the device
        Library("windraw", 1, {
            "cough_windraw_abi_version": (i, None), "cough_windraw_last_error": (s, None),
            "cough_draw_window_plans": (None, [C.c_ulonglong, i, i, vp, i, vp, i, vp, i, vp, i, d, i, i, d, d, d, vp, i, i, d,
                                               vp, vp, vp]),
        }),
    )}


LIBRARIES = _libraries()
LATER = _later()
OPEN = _open()

# the names the rest of the package uses, bound to the records: the main library's carry no prefix
load, check, SYMBOLS, LIB_PATH = (LIBRARIES["amd"].load, LIBRARIES["amd"].check, LIBRARIES["amd"].symbols,
                                  LIBRARIES["amd"].path)
for _r in (*list(LIBRARIES.values())[1:], *LATER.values(), *OPEN.values()):
    globals().update({f"load_{_r.name}": _r.load, f"check_{_r.name}": _r.check,
                      f"{_r.name.upper()}_SYMBOLS": _r.symbols, f"{_r.name.upper()}_LIB_PATH": _r.path})
del _r


def fptr(t):
    """Host float32 pointer of a contiguous CPU torch tensor / numpy array (caller keeps it alive)."""
    import numpy as np
    if hasattr(t, "data_ptr"):
        return C.cast(t.data_ptr(), _FP)
    assert isinstance(t, np.ndarray) and t.dtype == np.float32 and t.flags["C_CONTIGUOUS"]
    return t.ctypes.data_as(_FP)
