"""MI355X-native (gfx950) hot path of the cough detector: audio featuriser + CoughDetectorResidual
forward + sliding-window engine, behind the reference's Python call surface.  All arithmetic runs in
hand-written HIP kernels (``csrc/``) reached through the C-ABI in ``include/cough_amd.h``."""
from .preprocessing import AudioPreprocessor, RealtimePreprocessor, create_preprocessor
from .model import (CoughDetector, CoughDetectorResidual, CoughDetectorSmall, ConvBlock, ResidualBlock, create_model,
                    count_parameters)
from .inference import CoughDetectorInference, RealtimeQueueDetector
from .pipeline import CoughPipeline
from .augmentation import AudioAugmentor, MixUp, SpecAugment, create_augmentation_pipeline
from .training import HipAdamW, ResidualTrainer, SmallTrainer, StandardTrainer, create_trainer, train_epoch
from .loop import (EarlyStopping, EpochMeter, class_weights_from_counts, fit, load_checkpoint, save_checkpoint,
                   train_epoch_async, validate)
from .data import (DeviceClipBank, DeviceDataLoader, create_data_loaders, prepare_dataset_split, prepare_group_split,
                   stratified_group_split, stratified_split)
from .draws import augment_rows_drawn, draw_batch
from .warp import draw_speed, speed_rate_pair, warp_rows
from .pitch import draw_pitch, pitch_rate, pitch_rate_pair, pitch_shift_rows, stretch_rows, stretched_length
from .reverb import RirBank, draw_reverb, reverb_rows, reverberate_bank, synth_rirs
from .channel import ChannelBank, channel_rows, draw_channel, synth_channels
from .segments import SegmentTable, extract_segments, find_segments, frame_energy
from .slices import WindowTable, find_windows, inactive_clips, slice_bank, write_clips
from .duplicates import (DuplicateTable, Fingerprints, drop_duplicates, duplicate_groups, find_duplicates, fingerprint_bank,
                         fingerprint_images, label_conflicts)
from .score import (EventTable, ThresholdSweep, WindowScores, detect_events, detection_report, event_windows, score_bank,
                    sweep_thresholds)
from .audit import (LabelIssues, OutOfFoldScores, audit_labels, bank_files, find_label_issues, out_of_fold_scores,
                    stratified_kfold)
from .scenes import (EventSweep, ScenePlan, TruthTable, compose_scenes, draw_scene_plan, event_report, match_events,
                     missed_events, pick_threshold, truth_window_ranges)
from .windows import (ComposedWindowLoader, WindowLabels, WindowPlan, compose_windows, draw_window_plan, edge_margin,
                      scene_window_bank, window_labels)
from .windows import compose_window_records, draw_window_records, snr_levels, train_windows

__all__ = ["AudioPreprocessor", "RealtimePreprocessor", "create_preprocessor", "CoughDetectorResidual",
           "CoughDetector", "CoughDetectorSmall", "ConvBlock",
           "ResidualBlock", "create_model", "count_parameters", "CoughDetectorInference", "RealtimeQueueDetector",
           "CoughPipeline", "AudioAugmentor", "MixUp", "SpecAugment", "create_augmentation_pipeline",
           "ResidualTrainer", "SmallTrainer", "StandardTrainer", "create_trainer", "HipAdamW", "train_epoch",
           "EpochMeter", "EarlyStopping", "train_epoch_async", "validate", "save_checkpoint", "load_checkpoint",
           "class_weights_from_counts", "fit", "DeviceClipBank", "DeviceDataLoader", "create_data_loaders",
           "prepare_dataset_split", "stratified_split", "SegmentTable", "frame_energy", "find_segments", "extract_segments", "WindowScores", "ThresholdSweep",
           "EventTable", "score_bank", "sweep_thresholds", "detect_events", "event_windows", "detection_report",
           "draw_batch", "augment_rows_drawn", "warp_rows", "draw_speed", "speed_rate_pair",
           "stretch_rows", "pitch_shift_rows", "draw_pitch", "pitch_rate", "pitch_rate_pair", "stretched_length",
           "stratified_kfold", "out_of_fold_scores", "OutOfFoldScores", "find_label_issues", "LabelIssues", "audit_labels",
           "bank_files", "WindowTable", "find_windows", "slice_bank", "inactive_clips", "write_clips",
           "stratified_group_split", "prepare_group_split", "Fingerprints", "DuplicateTable", "fingerprint_images",
           "fingerprint_bank", "find_duplicates", "duplicate_groups", "label_conflicts", "drop_duplicates",
           "ScenePlan", "TruthTable", "EventSweep", "draw_scene_plan", "compose_scenes", "truth_window_ranges",
           "match_events", "event_report", "pick_threshold", "missed_events",
           "RirBank", "synth_rirs", "reverb_rows", "draw_reverb", "reverberate_bank",
           "ChannelBank", "synth_channels", "channel_rows", "draw_channel",
           "WindowPlan", "WindowLabels", "draw_window_plan", "edge_margin", "compose_windows", "ComposedWindowLoader",
           "window_labels", "scene_window_bank",
           "train_windows", "draw_window_records", "compose_window_records", "snr_levels"]
