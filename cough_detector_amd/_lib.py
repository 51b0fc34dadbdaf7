"""ctypes binding of ``libcough_amd.so`` (the C-ABI declared in ``include/cough_amd.h``) and of its companion
``libcough_amd_loop.so`` (``include/cough_amd_loop.h``: what the epoch loop adds; ``load_loop`` / ``check_loop``) and
``libcough_amd_data.so`` (``include/cough_amd_data.h``: the input pipeline; ``load_data`` / ``check_data``) and
``libcough_amd_segments.so`` (``include/cough_amd_segments.h``: corpus curation; ``load_segments`` / ``check_segments``)
and ``libcough_amd_score.so`` (``include/cough_amd_score.h``: offline scoring; ``load_score`` / ``check_score``) and
``libcough_amd_draws.so`` (``include/cough_amd_draws.h``: a batch's draws on the device; ``load_draws`` / ``check_draws``)
and ``libcough_amd_soft.so`` (``include/cough_amd_soft.h``: the training steps on soft targets; ``load_soft`` / ``check_soft``)
and ``libcough_amd_warp.so`` (``include/cough_amd_warp.h``: speed perturbation; ``load_warp`` / ``check_warp``)
and ``libcough_amd_pitch.so`` (``include/cough_amd_pitch.h``: the pitch shift's time stretch; ``load_pitch`` / ``check_pitch``).

There is no CPU fallback: if the shared object is missing or a call fails, this raises.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
# COUGH_AMD_LIB: alternative build of the same ABI (same-box A/B timing of kernel variants)
LIB_PATH = os.environ.get("COUGH_AMD_LIB") or os.path.join(HERE, "libcough_amd.so")

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

# every symbol include/cough_amd.h declares (tests check the library exports all of them)
SYMBOLS = (
    "cough_amd_abi_version", "cough_amd_arch", "cough_amd_last_error",
    "cough_featurizer_create", "cough_featurizer_destroy", "cough_featurizer_num_features",
    "cough_featurizer_num_frames", "cough_featurizer_path", "cough_featurize", "cough_featurizer_workspace_bytes", "cough_featurize_ws",
    "cough_spectrogram", "cough_featurizer_num_frames_for", "cough_featurizer_workspace_bytes_for", "cough_featurize_any",
    "cough_spectrogram_any",
    "cough_resnet_create", "cough_resnet_create_ex", "cough_resnet_destroy", "cough_resnet_workspace_bytes",
    "cough_resblock_create", "cough_resblock_destroy", "cough_resblock_workspace_bytes", "cough_resblock_out_shape",
    "cough_resblock_forward",
    "cough_resnet_forward", "cough_resnet_read_activation",
    "cough_cnn_create", "cough_cnn_destroy", "cough_cnn_workspace_bytes", "cough_cnn_forward", "cough_cnn_conv_output",
    "cough_pipeline_workspace_bytes", "cough_pipeline_forward",
    "cough_mask_axes", "cough_prepare_clip", "cough_resample", "cough_ring_write", "cough_window_gather",
    "cough_synth_clips", "cough_pre_emphasis", "cough_compute_deltas", "cough_pcen",
    "cough_augment_workspace_bytes", "cough_augment_waveforms", "cough_mix_rows",
    "cough_train_workspace_bytes", "cough_train_forward_backward", "cough_adamw_step",
    "cough_train_small_workspace_bytes", "cough_train_small_forward_backward",
    "cough_train_std_workspace_bytes", "cough_train_std_forward_backward",
)

# every symbol include/cough_amd_loop.h declares (the companion library of the epoch loop; cough_amd.h stays at ABI v5)
LOOP_LIB_PATH = os.environ.get("COUGH_AMD_LOOP_LIB") or os.path.join(HERE, "libcough_amd_loop.so")
LOOP_SYMBOLS = ("cough_loop_abi_version", "cough_loop_last_error", "cough_epoch_meter_update")
EPOCH_METER_BYTES = 64   # COUGH_EPOCH_METER_BYTES

# every symbol include/cough_amd_data.h declares (the companion library of the input pipeline)
DATA_LIB_PATH = os.environ.get("COUGH_AMD_DATA_LIB") or os.path.join(HERE, "libcough_amd_data.so")
DATA_SYMBOLS = ("cough_data_abi_version", "cough_data_last_error", "cough_gather_rows", "cough_prepare_rows",
                "cough_mask_images")
PREP_NORMALIZE = 1       # COUGH_PREP_NORMALIZE
MAX_MASKS = 16           # COUGH_MAX_MASKS

# every symbol include/cough_amd_segments.h declares (the companion library of corpus curation)
SEGMENTS_LIB_PATH = os.environ.get("COUGH_AMD_SEGMENTS_LIB") or os.path.join(HERE, "libcough_amd_segments.so")
SEGMENTS_SYMBOLS = ("cough_segments_abi_version", "cough_segments_last_error", "cough_frame_energy_tile_frames",
                    "cough_frame_energy", "cough_pick_segments", "cough_copy_segments")
MAX_SEGMENTS = 16        # COUGH_MAX_SEGMENTS
MAX_FRAME_LENGTH = 4096  # COUGH_MAX_FRAME_LENGTH

# every symbol include/cough_amd_score.h declares (the companion library of offline scoring)
SCORE_LIB_PATH = os.environ.get("COUGH_AMD_SCORE_LIB") or os.path.join(HERE, "libcough_amd_score.so")
SCORE_SYMBOLS = ("cough_score_abi_version", "cough_score_last_error", "cough_smooth_windows", "cough_sweep_thresholds",
                 "cough_list_events")
MAX_SMOOTHING = 32       # COUGH_MAX_SMOOTHING
MAX_THRESHOLDS = 1024    # COUGH_MAX_THRESHOLDS

# every symbol include/cough_amd_draws.h declares (the companion library of the device-side draws)
DRAWS_LIB_PATH = os.environ.get("COUGH_AMD_DRAWS_LIB") or os.path.join(HERE, "libcough_amd_draws.so")
DRAWS_SYMBOLS = ("cough_draws_abi_version", "cough_draws_last_error", "cough_draw_batch",
                 "cough_augment_rows_drawn_workspace_bytes", "cough_augment_rows_drawn")

# every symbol include/cough_amd_soft.h declares (the companion library of the soft-target steps and the batch MixUp)
SOFT_LIB_PATH = os.environ.get("COUGH_AMD_SOFT_LIB") or os.path.join(HERE, "libcough_amd_soft.so")
SOFT_SYMBOLS = ("cough_soft_abi_version", "cough_soft_last_error", "cough_train_forward_backward_soft",
                "cough_train_small_forward_backward_soft", "cough_train_std_forward_backward_soft", "cough_mix_batch")

# every symbol include/cough_amd_warp.h declares (the companion library of speed perturbation)
WARP_LIB_PATH = os.environ.get("COUGH_AMD_WARP_LIB") or os.path.join(HERE, "libcough_amd_warp.so")
WARP_SYMBOLS = ("cough_warp_abi_version", "cough_warp_last_error", "cough_warp_rows", "cough_draw_speed",
                "cough_clear_shifts")
WARP_MAX_RATE, WARP_MAX_RATIO = 1 << 20, 4   # COUGH_WARP_MAX_RATE / COUGH_WARP_MAX_RATIO

# every symbol include/cough_amd_pitch.h declares (the companion library of pitch shift)
PITCH_LIB_PATH = os.environ.get("COUGH_AMD_PITCH_LIB") or os.path.join(HERE, "libcough_amd_pitch.so")
PITCH_SYMBOLS = ("cough_pitch_abi_version", "cough_pitch_last_error", "cough_stretch_rows", "cough_draw_pitch")
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


_lib = None
_lock = threading.Lock()


def load() -> C.CDLL:
    """Load (once) and type the library; raise loudly if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: the HIP extension is not built. Run `python -m cough_detector_amd.build` "
                "(needs hipcc / ROCm, target gfx950). There is no CPU fallback.")
        lib = C.CDLL(LIB_PATH)
        vp, ll, i = C.c_void_p, C.c_longlong, C.c_int
        lib.cough_amd_abi_version.restype = i
        lib.cough_amd_arch.restype = C.c_char_p
        lib.cough_amd_last_error.restype = C.c_char_p
        lib.cough_featurizer_create.argtypes = [C.POINTER(vp), C.POINTER(FeatConfig), _FP, _FP, _FP]
        lib.cough_featurizer_destroy.argtypes = [vp]
        lib.cough_featurizer_destroy.restype = None
        lib.cough_featurizer_num_features.argtypes = [vp]
        lib.cough_featurizer_num_frames.argtypes = [vp]
        lib.cough_featurizer_path.argtypes = [vp]
        lib.cough_featurize.argtypes = [vp, vp, ll, vp, i, i, vp]
        lib.cough_spectrogram.argtypes = [vp, vp, ll, vp, i, i, vp]
        lib.cough_featurizer_workspace_bytes.argtypes = [vp, i]
        lib.cough_featurizer_workspace_bytes.restype = C.c_size_t
        lib.cough_featurize_ws.argtypes = [vp, vp, ll, vp, i, i, vp, C.c_size_t, vp]
        lib.cough_featurizer_num_frames_for.argtypes = [vp, i]
        lib.cough_featurizer_workspace_bytes_for.argtypes = [vp, i, i]
        lib.cough_featurizer_workspace_bytes_for.restype = C.c_size_t
        lib.cough_featurize_any.argtypes = [vp, vp, ll, i, vp, i, i, vp, C.c_size_t, vp]
        lib.cough_spectrogram_any.argtypes = [vp, vp, ll, i, vp, i, i, vp]
        lib.cough_resnet_create.argtypes = [C.POINTER(vp), C.POINTER(ResNetWeights), i]
        lib.cough_resnet_create_ex.argtypes = [C.POINTER(vp), i, C.POINTER(i), C.POINTER(ConvBN), C.POINTER(ResBlockWeights),
                                               _FP, _FP, C.c_float, i]
        lib.cough_resblock_create.argtypes = [C.POINTER(vp), i, i, i, C.POINTER(ConvBN), C.POINTER(ConvBN), C.POINTER(ConvBN),
                                              C.c_float]
        lib.cough_resblock_destroy.argtypes = [vp]
        lib.cough_resblock_destroy.restype = None
        lib.cough_resblock_workspace_bytes.argtypes = [vp, i, i, i]
        lib.cough_resblock_workspace_bytes.restype = C.c_size_t
        lib.cough_resblock_out_shape.argtypes = [vp, i, i, C.POINTER(i), C.POINTER(i)]
        lib.cough_resblock_forward.argtypes = [vp, vp, i, i, i, vp, vp, C.c_size_t, vp]
        lib.cough_resnet_destroy.argtypes = [vp]
        lib.cough_resnet_destroy.restype = None
        lib.cough_resnet_workspace_bytes.argtypes = [vp, i, i, i]
        lib.cough_resnet_workspace_bytes.restype = C.c_size_t
        lib.cough_resnet_forward.argtypes = [vp, vp, i, i, i, vp, vp, vp, vp, C.c_size_t, vp]
        lib.cough_resnet_read_activation.argtypes = [vp, vp, i, i, i, i, vp, vp]
        lib.cough_cnn_create.argtypes = [C.POINTER(vp), C.POINTER(CnnWeights), i]
        lib.cough_cnn_destroy.argtypes = [vp]
        lib.cough_cnn_destroy.restype = None
        lib.cough_cnn_workspace_bytes.argtypes = [vp, i, i, i]
        lib.cough_cnn_workspace_bytes.restype = C.c_size_t
        lib.cough_cnn_forward.argtypes = [vp, vp, i, i, i, vp, vp, vp, vp, C.c_size_t, vp]
        lib.cough_cnn_conv_output.argtypes = [vp, vp, i, i, i, vp, vp, C.c_size_t, vp]
        lib.cough_pipeline_workspace_bytes.argtypes = [vp, vp, i]
        lib.cough_pipeline_workspace_bytes.restype = C.c_size_t
        lib.cough_pipeline_forward.argtypes = [vp, vp, vp, ll, i, i, vp, vp, vp, vp, vp, C.c_size_t, vp, vp, vp]
        lib.cough_mask_axes.argtypes = [vp, vp, ll, i, i, i, C.POINTER(i), C.POINTER(i), C.POINTER(i), vp]
        lib.cough_prepare_clip.argtypes = [vp, ll, i, i, vp, i, i, vp]
        lib.cough_resample.argtypes = [vp, ll, i, i, vp, i, i, i, vp, ll, i, vp]
        lib.cough_ring_write.argtypes = [vp, i, vp, i, vp, vp, i, vp]
        lib.cough_window_gather.argtypes = [vp, i, vp, vp, i, i, vp, vp]
        lib.cough_synth_clips.argtypes = [vp, ll, i, ll, ll, vp]
        lib.cough_pre_emphasis.argtypes = [vp, ll, vp, ll, i, i, C.c_float, vp]
        lib.cough_compute_deltas.argtypes = [vp, vp, ll, i, vp]
        lib.cough_pcen.argtypes = [vp, vp, ll, i, C.c_float, C.c_float, C.c_float, C.c_float, vp]
        lib.cough_augment_workspace_bytes.argtypes = [i]
        lib.cough_augment_workspace_bytes.restype = C.c_size_t
        lib.cough_augment_waveforms.argtypes = [vp, ll, vp, i, i, C.POINTER(i), C.POINTER(CoughAugClip), vp, ll,
                                                C.POINTER(ll), C.POINTER(i), i, vp, C.c_ulonglong, vp, C.c_size_t, vp]
        lib.cough_mix_rows.argtypes = [vp, vp, vp, vp, ll, ll, vp, vp]
        f, ull = C.c_float, C.c_ulonglong
        lib.cough_train_workspace_bytes.argtypes = [i, i, i]
        lib.cough_train_workspace_bytes.restype = C.c_size_t
        lib.cough_train_forward_backward.argtypes = [vp, i, i, i, vp, vp, vp, ull, ull, f, vp, vp, vp, vp, f, f, vp, vp,
                                                     vp, vp, C.c_size_t, vp]
        lib.cough_train_small_workspace_bytes.argtypes = [i, i, i]
        lib.cough_train_small_workspace_bytes.restype = C.c_size_t
        lib.cough_train_small_forward_backward.argtypes = lib.cough_train_forward_backward.argtypes
        lib.cough_train_std_workspace_bytes.argtypes = [i, i, i]
        lib.cough_train_std_workspace_bytes.restype = C.c_size_t
        lib.cough_train_std_forward_backward.argtypes = [vp, i, i, i, vp, vp, vp, ull, ull, f, f, vp, vp, vp, vp, f, f,
                                                         vp, vp, vp, vp, C.c_size_t, vp]
        lib.cough_adamw_step.argtypes = [vp, vp, vp, vp, ll, f, f, f, f, f, f, C.c_double, C.c_double, vp, vp]
        if lib.cough_amd_abi_version() != 5:
            raise RuntimeError("libcough_amd.so ABI version mismatch; rebuild it")
        _lib = lib
    return _lib


_loop_lib = None


def load_loop() -> C.CDLL:
    """Load (once) and type the companion library of the epoch loop; raise loudly if it is not built."""
    global _loop_lib
    if _loop_lib is not None:
        return _loop_lib
    with _lock:
        if _loop_lib is not None:
            return _loop_lib
        if not os.path.exists(LOOP_LIB_PATH):
            raise RuntimeError(
                f"{LOOP_LIB_PATH} is missing: the HIP extension is not built. Run `python -m cough_detector_amd.build` "
                "(needs hipcc / ROCm, target gfx950). There is no CPU fallback.")
        lib = C.CDLL(LOOP_LIB_PATH)
        vp, i = C.c_void_p, C.c_int
        lib.cough_loop_abi_version.restype = i
        lib.cough_loop_last_error.restype = C.c_char_p
        lib.cough_epoch_meter_update.argtypes = [vp, vp, i, vp, vp, vp, vp, vp]
        if lib.cough_loop_abi_version() != 1:
            raise RuntimeError("libcough_amd_loop.so ABI version mismatch; rebuild it")
        _loop_lib = lib
    return _loop_lib


_data_lib = None


def load_data() -> C.CDLL:
    """Load (once) and type the companion library of the input pipeline; raise loudly if it is not built."""
    global _data_lib
    if _data_lib is not None:
        return _data_lib
    with _lock:
        if _data_lib is not None:
            return _data_lib
        if not os.path.exists(DATA_LIB_PATH):
            raise RuntimeError(
                f"{DATA_LIB_PATH} is missing: the HIP extension is not built. Run `python -m cough_detector_amd.build` "
                "(needs hipcc / ROCm, target gfx950). There is no CPU fallback.")
        lib = C.CDLL(DATA_LIB_PATH)
        vp, ll, i = C.c_void_p, C.c_longlong, C.c_int
        lib.cough_data_abi_version.restype = i
        lib.cough_data_last_error.restype = C.c_char_p
        lib.cough_gather_rows.argtypes = [vp, vp, vp, i, vp, ll, i, vp]
        lib.cough_prepare_rows.argtypes = [vp, vp, vp, i, vp, i, i, vp]
        lib.cough_mask_images.argtypes = [vp, vp, i, i, i, i, vp, vp, vp, vp]
        if lib.cough_data_abi_version() != 1:
            raise RuntimeError("libcough_amd_data.so ABI version mismatch; rebuild it")
        _data_lib = lib
    return _data_lib


_segments_lib = None


def load_segments() -> C.CDLL:
    """Load (once) and type the companion library of corpus curation; raise loudly if it is not built."""
    global _segments_lib
    if _segments_lib is not None:
        return _segments_lib
    with _lock:
        if _segments_lib is not None:
            return _segments_lib
        if not os.path.exists(SEGMENTS_LIB_PATH):
            raise RuntimeError(
                f"{SEGMENTS_LIB_PATH} is missing: the HIP extension is not built. Run `python -m cough_detector_amd.build` "
                "(needs hipcc / ROCm, target gfx950). There is no CPU fallback.")
        lib = C.CDLL(SEGMENTS_LIB_PATH)
        vp, i, d = C.c_void_p, C.c_int, C.c_double
        lib.cough_segments_abi_version.restype = i
        lib.cough_segments_last_error.restype = C.c_char_p
        lib.cough_frame_energy_tile_frames.argtypes = [i, i]
        lib.cough_frame_energy.argtypes = [vp, vp, vp, vp, i, vp, i, i, i, vp, vp]
        lib.cough_pick_segments.argtypes = [vp, vp, vp, i, i, i, i, i, i, d, d, vp, vp, vp, vp, vp]
        lib.cough_copy_segments.argtypes = [vp, vp, vp, vp, vp, i, i, vp, vp]
        if lib.cough_segments_abi_version() != 1:
            raise RuntimeError("libcough_amd_segments.so ABI version mismatch; rebuild it")
        _segments_lib = lib
    return _segments_lib


_score_lib = None


def load_score() -> C.CDLL:
    """Load (once) and type the companion library of offline scoring; raise loudly if it is not built."""
    global _score_lib
    if _score_lib is not None:
        return _score_lib
    with _lock:
        if _score_lib is not None:
            return _score_lib
        if not os.path.exists(SCORE_LIB_PATH):
            raise RuntimeError(
                f"{SCORE_LIB_PATH} is missing: the HIP extension is not built. Run `python -m cough_detector_amd.build` "
                "(needs hipcc / ROCm, target gfx950). There is no CPU fallback.")
        lib = C.CDLL(SCORE_LIB_PATH)
        vp, ll, i, d = C.c_void_p, C.c_longlong, C.c_int, C.c_double
        lib.cough_score_abi_version.restype = i
        lib.cough_score_last_error.restype = C.c_char_p
        lib.cough_smooth_windows.argtypes = [vp, vp, i, ll, i, vp, vp]
        lib.cough_sweep_thresholds.argtypes = [vp, vp, i, ll, vp, i, i, vp, vp, vp, vp, vp]
        lib.cough_list_events.argtypes = [vp, vp, i, ll, d, i, vp, ll, vp, vp, vp]
        if lib.cough_score_abi_version() != 1:
            raise RuntimeError("libcough_amd_score.so ABI version mismatch; rebuild it")
        _score_lib = lib
    return _score_lib


_draws_lib = None


def load_draws() -> C.CDLL:
    """Load (once) and type the companion library of the device-side draws; raise loudly if it is not built."""
    global _draws_lib
    if _draws_lib is not None:
        return _draws_lib
    with _lock:
        if _draws_lib is not None:
            return _draws_lib
        if not os.path.exists(DRAWS_LIB_PATH):
            raise RuntimeError(
                f"{DRAWS_LIB_PATH} is missing: the HIP extension is not built. Run `python -m cough_detector_amd.build` "
                "(needs hipcc / ROCm, target gfx950). There is no CPU fallback.")
        lib = C.CDLL(DRAWS_LIB_PATH)
        vp, ll, i, d, ull = C.c_void_p, C.c_longlong, C.c_int, C.c_double, C.c_ulonglong
        lib.cough_draws_abi_version.restype = i
        lib.cough_draws_last_error.restype = C.c_char_p
        lib.cough_draw_batch.argtypes = [ull, i, vp, d, i, vp, d, i, i, i, i, i, i, vp, vp, vp, vp, vp]
        lib.cough_augment_rows_drawn_workspace_bytes.argtypes = [i]
        lib.cough_augment_rows_drawn_workspace_bytes.restype = C.c_size_t
        lib.cough_augment_rows_drawn.argtypes = [vp, vp, vp, i, i, vp, vp, ll, vp, vp, i, ull, vp, vp, C.c_size_t, vp]
        if lib.cough_draws_abi_version() != 1:
            raise RuntimeError("libcough_amd_draws.so ABI version mismatch; rebuild it")
        _draws_lib = lib
    return _draws_lib


_soft_lib = None


def load_soft() -> C.CDLL:
    """Load (once) and type the companion library of the soft-target steps; raise loudly if it is not built."""
    global _soft_lib
    if _soft_lib is not None:
        return _soft_lib
    with _lock:
        if _soft_lib is not None:
            return _soft_lib
        if not os.path.exists(SOFT_LIB_PATH):
            raise RuntimeError(
                f"{SOFT_LIB_PATH} is missing: the HIP extension is not built. Run `python -m cough_detector_amd.build` "
                "(needs hipcc / ROCm, target gfx950). There is no CPU fallback.")
        lib = C.CDLL(SOFT_LIB_PATH)
        vp, ll, i, f, ull = C.c_void_p, C.c_longlong, C.c_int, C.c_float, C.c_ulonglong
        lib.cough_soft_abi_version.restype = i
        lib.cough_soft_last_error.restype = C.c_char_p
        # the argument lists of the v5 steps, with the soft targets where the class indices were
        lib.cough_train_forward_backward_soft.argtypes = [vp, i, i, i, vp, vp, vp, ull, ull, f, vp, vp, vp, vp, f, f, vp,
                                                          vp, vp, vp, C.c_size_t, vp]
        lib.cough_train_small_forward_backward_soft.argtypes = lib.cough_train_forward_backward_soft.argtypes
        lib.cough_train_std_forward_backward_soft.argtypes = [vp, i, i, i, vp, vp, vp, ull, ull, f, f, vp, vp, vp, vp, f,
                                                              f, vp, vp, vp, vp, C.c_size_t, vp]
        lib.cough_mix_batch.argtypes = [vp, vp, vp, vp, i, ll, vp, vp, vp]
        if lib.cough_soft_abi_version() != 1:
            raise RuntimeError("libcough_amd_soft.so ABI version mismatch; rebuild it")
        _soft_lib = lib
    return _soft_lib


_warp_lib = None


def load_warp() -> C.CDLL:
    """Load (once) and type the companion library of speed perturbation; raise loudly if it is not built."""
    global _warp_lib
    if _warp_lib is not None:
        return _warp_lib
    with _lock:
        if _warp_lib is not None:
            return _warp_lib
        if not os.path.exists(WARP_LIB_PATH):
            raise RuntimeError(
                f"{WARP_LIB_PATH} is missing: the HIP extension is not built. Run `python -m cough_detector_amd.build` "
                "(needs hipcc / ROCm, target gfx950). There is no CPU fallback.")
        lib = C.CDLL(WARP_LIB_PATH)
        vp, i, d, ull = C.c_void_p, C.c_int, C.c_double, C.c_ulonglong
        lib.cough_warp_abi_version.restype = i
        lib.cough_warp_last_error.restype = C.c_char_p
        lib.cough_warp_rows.argtypes = [vp, vp, vp, i, vp, vp, i, vp, vp]
        lib.cough_draw_speed.argtypes = [ull, i, vp, d, d, d, i, vp, vp, vp]
        lib.cough_clear_shifts.argtypes = [vp, i, vp]
        if lib.cough_warp_abi_version() != 1:
            raise RuntimeError("libcough_amd_warp.so ABI version mismatch; rebuild it")
        _warp_lib = lib
    return _warp_lib


_pitch_lib = None


def load_pitch() -> C.CDLL:
    """Load (once) and type the companion library of pitch shift; raise loudly if it is not built."""
    global _pitch_lib
    if _pitch_lib is not None:
        return _pitch_lib
    with _lock:
        if _pitch_lib is not None:
            return _pitch_lib
        if not os.path.exists(PITCH_LIB_PATH):
            raise RuntimeError(
                f"{PITCH_LIB_PATH} is missing: the HIP extension is not built. Run `python -m cough_detector_amd.build` "
                "(needs hipcc / ROCm, target gfx950). There is no CPU fallback.")
        lib = C.CDLL(PITCH_LIB_PATH)
        vp, i, d, ull = C.c_void_p, C.c_int, C.c_double, C.c_ulonglong
        lib.cough_pitch_abi_version.restype = i
        lib.cough_pitch_last_error.restype = C.c_char_p
        lib.cough_stretch_rows.argtypes = [vp, vp, vp, i, vp, vp, i, vp, vp]
        lib.cough_draw_pitch.argtypes = [ull, i, vp, d, i, i, vp, i, vp, vp, vp, vp]
        if lib.cough_pitch_abi_version() != 1:
            raise RuntimeError("libcough_amd_pitch.so ABI version mismatch; rebuild it")
        _pitch_lib = lib
    return _pitch_lib


def _raise(status: int, what: str, msg: str) -> None:
    if status in (EINVAL, EUNSUPPORTED):
        raise ValueError(f"{what}: {msg}")
    raise RuntimeError(f"{what}: {msg} (status {status})")


def check_loop(status: int, what: str) -> None:
    """``check`` for a call into the companion library (it keeps a last-error message of its own)."""
    if status != OK:
        _raise(status, what, load_loop().cough_loop_last_error().decode("utf-8", "replace"))


def check_data(status: int, what: str) -> None:
    """``check`` for a call into the input pipeline's library (it keeps a last-error message of its own)."""
    if status != OK:
        _raise(status, what, load_data().cough_data_last_error().decode("utf-8", "replace"))


def check_segments(status: int, what: str) -> None:
    """``check`` for a call into the curation library (it keeps a last-error message of its own)."""
    if status != OK:
        _raise(status, what, load_segments().cough_segments_last_error().decode("utf-8", "replace"))


def check_score(status: int, what: str) -> None:
    """``check`` for a call into the scoring library (it keeps a last-error message of its own)."""
    if status != OK:
        _raise(status, what, load_score().cough_score_last_error().decode("utf-8", "replace"))


def check_draws(status: int, what: str) -> None:
    """``check`` for a call into the draws library (it keeps a last-error message of its own)."""
    if status != OK:
        _raise(status, what, load_draws().cough_draws_last_error().decode("utf-8", "replace"))


def check_soft(status: int, what: str) -> None:
    """``check`` for a call into the soft-target library (it keeps a last-error message of its own)."""
    if status != OK:
        _raise(status, what, load_soft().cough_soft_last_error().decode("utf-8", "replace"))


def check_warp(status: int, what: str) -> None:
    """``check`` for a call into the speed-perturbation library (it keeps a last-error message of its own)."""
    if status != OK:
        _raise(status, what, load_warp().cough_warp_last_error().decode("utf-8", "replace"))


def check_pitch(status: int, what: str) -> None:
    """``check`` for a call into the pitch-shift library (it keeps a last-error message of its own)."""
    if status != OK:
        _raise(status, what, load_pitch().cough_pitch_last_error().decode("utf-8", "replace"))


def check(status: int, what: str) -> None:
    """Map a C status to the reference's exception convention
    (ValueError for argument/config errors, as src/model.py:313-314; RuntimeError otherwise)."""
    if status == OK:
        return
    _raise(status, what, load().cough_amd_last_error().decode("utf-8", "replace"))


def fptr(t):
    """Host float32 pointer of a contiguous CPU torch tensor / numpy array (caller keeps it alive)."""
    import numpy as np
    if hasattr(t, "data_ptr"):
        return C.cast(t.data_ptr(), _FP)
    assert isinstance(t, np.ndarray) and t.dtype == np.float32 and t.flags["C_CONTIGUOUS"]
    return t.ctypes.data_as(_FP)
