/*
 * cough_amd_scenes.h -- C-ABI of libcough_amd_scenes.so, the companion of libcough_amd.so for soundscapes with known
 * cough times: cough segments mixed at chosen onsets and SNRs into long backgrounds (what the reference's add_noise,
 * src/augmentation.py, does to one clip, turned round: the cough is scaled against the background's power), and the
 * detections of the offline scorer (cough_amd_score.h) matched to those known events, at many thresholds at once.
 *
 * cough_amd.h is pinned at ABI v5 with its 53 entry points and every companion at version 1, so what the scenes need on
 * the device is exported from a library of its own with a version of its own.  The conventions are those of cough_amd.h:
 * plain pointers and sizes only, `d_` = device (HBM) pointer; every call returns COUGH_OK (0) or a COUGH_E* code of
 * cough_amd.h and leaves a thread-local message for the last-error call below; launches are stream-ordered on `stream`
 * (a hipStream_t; NULL = default stream); no call allocates or synchronises; every argument is checked before the
 * launch; no kernel uses atomics and every sum is formed in a fixed order, so the same input gives the same bits.
 *
 * What lives in device memory (offsets, lengths, starts, indices, onsets, tiles) cannot be checked by the host before
 * the launch: the kernels clamp every such value to the array sizes they were given (n_bank_samples, n_bg_samples,
 * n_ev_samples, n_out_samples, n_events, n_windows, n_truth, ...), so nothing is read or written out of bounds whatever
 * those arrays hold.  What a call computes from values it had to clamp is unspecified, but it stays inside its arrays.
 *
 * The clips of a packed bank: clip k is d_bank[offset[k] .. offset[k] + length[k]), offsets int64 in elements (a clip
 * starts at any element: 4-byte alignment only), lengths int32.
 * Windows and recordings: the layout of cough_amd_score.h (d_window_offsets, int64 [n_clips + 1]).
 */
#ifndef COUGH_AMD_SCENES_H
#define COUGH_AMD_SCENES_H

#include "cough_amd.h"

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden: exactly the entry points declared in this header are exported
 * (tests/test_scenes_host.py compares `nm -D` of the built library with this list). */
#pragma GCC visibility push(default)

#define COUGH_SCENES_ABI_VERSION 1
#define COUGH_SCENES_TILE 4096         /* samples of a scene that one workgroup of cough_mix_scenes composes */
#define COUGH_SCENES_MAX_THRESHOLDS 1024   /* thresholds per match at most: COUGH_MAX_THRESHOLDS of cough_amd_score.h */

int cough_scenes_abi_version(void);
const char* cough_scenes_last_error(void);  /* thread-local, never NULL */

/* ------------------------------------------------------------------ mean power of n spans of a packed bank
 * Span r reads clip (d_clip_offsets[r], d_clip_lengths[r]) cyclically from d_starts[r] on: sample i of the span is
 * clip[(d_starts[r] + i) mod length], i = 0 .. d_span_lengths[r] - 1, the way add_noise repeats a short noise sample.
 *   d_power[r] float64 = (sum of double(x_i)^2) / span length.
 * Order of the sum (every square is exact in float64, so only the additions round): one workgroup of 256 threads per
 * span; thread t adds the squares of samples i = t, t + 256, t + 512, ... in ascending i, starting from 0.0; the 256
 * partial sums are then added pairwise, p[t] += p[t ^ m] for m = 1, 2, 4, 8, 16, 32 (inside each wave of 64), and the
 * four wave sums as (w0 + w1) + (w2 + w3).  The order depends on the span alone: the same span gives the same bits
 * alone and in any batch.
 * A span of length <= 0 gives 0.0, and so does a clip whose clamped length is 0; a NaN or Inf sample gives a
 * non-finite power.  A negative start counts as 0, a start past the clip is taken mod its length.
 * n == 0 launches nothing. */
int cough_span_power(const float* d_bank, long long n_bank_samples, const long long* d_clip_offsets,
                     const int* d_clip_lengths, const int* d_starts, const int* d_span_lengths, int n, double* d_power,
                     void* stream);

/* ------------------------------------------------------------------ the gain of every event, one thread per event
 * Event e of scene s = d_event_scene[e] takes its own power from d_p_ev[d_event_power[e]]:
 *   gain[e] = float32(sqrt(((snr_linear[e] * (double(bg_gain[s]) * double(bg_gain[s]))) * P_bg[s]) / P_ev)),
 * float64 operations in that order, rounded to float32 once.  snr_linear is 10 ** (snr_db / 10), computed by the host
 * (there is no device pow).  The gain is 1.0 when P_bg[s] is 0 or not finite, when P_ev is 0 or not finite (the
 * reference's `if noise_power > 0` turned round: a cough over digital silence stays audible), or when an index lies
 * outside its array.
 *   d_p_bg [n_scenes] float64, d_bg_gain [n_scenes] float32, d_p_ev [n_powers] float64;
 *   d_event_scene, d_event_power [n_events] int32; d_snr_linear [n_events] float64; d_gain [n_events] float32.
 * n_events == 0 launches nothing. */
int cough_scene_gains(const double* d_p_bg, const float* d_bg_gain, int n_scenes, const double* d_p_ev, int n_powers,
                      const int* d_event_scene, const int* d_event_power, const double* d_snr_linear, int n_events,
                      float* d_gain, void* stream);

/* ------------------------------------------------------------------ the mix
 * Scene s has L_s = d_scene_lengths[s] samples, written to d_out[d_out_offsets[s] .. + L_s).  Its background is clip
 * (d_bg_offsets[s], d_bg_lengths[s]) of d_bg, read cyclically from d_bg_starts[s] on.  It owns the events
 * d_ev_offsets[s] .. d_ev_offsets[s + 1] (int64 [n_scenes + 1], ascending, last n_events); event e is clip
 * (d_src_offsets[e], d_src_lengths[e]) of d_ev placed at sample d_onsets[e] of the scene with gain d_gains[e].  The
 * events of a scene are sorted by onset and do not overlap: the caller guarantees that, and the kernel needs it for the
 * result only, not for memory safety.  Per sample i of scene s, in float32:
 *   acc = bg_gain[s] * B[(bg_start[s] + i) mod bg_len]                  (one rounded product)
 *   if event e covers i (onset[e] <= i < onset[e] + len[e]):  acc = fmaf(gain[e], E[i - onset[e]], acc)
 *   out[i] = acc
 * An event that reaches past L_s is cut there.  A background whose clamped length is 0 counts as silence (acc = 0).
 * Where events overlap all the same, they are added in the order of their indices.
 *
 * The grid is over tiles: d_tiles [n_tiles][2] int32 holds (scene, first sample); a tile composes the samples first ..
 * first + COUGH_SCENES_TILE - 1 of its scene that exist.  The caller lists, scene by scene, first = 0,
 * COUGH_SCENES_TILE, 2 * COUGH_SCENES_TILE, ...; a tile whose scene lies outside 0 .. n_scenes - 1 or whose first sample
 * does not exist writes nothing.  One workgroup per tile: it finds the tile's first event by a binary search of the
 * scene's onsets (once, the same in every lane), splits the background at its wrap points (no modulo per sample; a
 * background of fewer than 1024 samples, add_noise's short noise sample, would wrap many times per tile and is read
 * through a cyclic index per thread instead, 4 bytes at a time, again without a modulo per sample),
 * accumulates in LDS and moves each of the three streams with 16-byte accesses from the first 16-byte boundary of its
 * own pointer on, whatever 4-byte phase that pointer has.
 *   d_bg_gains, d_gains float32; lengths, starts, onsets int32; offsets int64.  d_out must not overlap d_bg or d_ev.
 *   The event arrays and d_ev may be NULL when n_events == 0.
 * n_scenes == 0 or n_tiles == 0 launches nothing. */
int cough_mix_scenes(const float* d_bg, long long n_bg_samples, const long long* d_bg_offsets, const int* d_bg_lengths,
                     const int* d_bg_starts, const float* d_bg_gains, const int* d_scene_lengths,
                     const long long* d_out_offsets, const long long* d_ev_offsets, int n_scenes, const float* d_ev,
                     long long n_ev_samples, const long long* d_src_offsets, const int* d_src_lengths,
                     const int* d_onsets, const float* d_gains, int n_events, const int* d_tiles, int n_tiles,
                     float* d_out, long long n_out_samples, void* stream);

/* ------------------------------------------------------------------ detections matched to known events
 * The walk of cough_sweep_thresholds (the same device functions decide: csrc/score_walk.h), one wave per (recording, 64
 * thresholds), a lane per threshold.  Truth event j of recording c lies in d_truth_offsets[c] .. d_truth_offsets[c + 1]
 * (int64 [n_clips + 1], ascending, last n_truth) and carries the closed window range [d_k_lo[j], d_k_hi[j]] (int32; a
 * range with k_lo > k_hi is empty and never hit) and its onset d_onset[j] in samples (int32).  Within a recording
 * d_k_lo is non-decreasing, and so is d_k_hi over the events whose range is not empty (an empty range may carry any
 * k_hi below its k_lo): the caller guarantees that, and the kernel needs it for the result only.
 * A window k that fires is classified:
 *   p = the first truth event after the last one already hit with k_hi[p] >= k (none: past the recording's events)
 *   hit          p exists and k_lo[p] <= k: event p is hit by k; `last` = p
 *   repeat       else, an event has been hit and k <= k_hi[last]
 *   false alarm  else
 * Why this is the greedy one-to-one assignment of every detection, in time order, to the earliest unhit event whose range
 * holds it: an unhit event q in front of p was passed over at some k' <= k with k_hi[q] < k', so it cannot hold k; and if
 * k_lo[p] > k, every later q has k_lo[q] >= k_lo[p] > k, so none holds k either.  Only the order of k_lo enters.
 * Outputs, each of which may be NULL, each [n_clips][n_thresholds]:
 *   d_hits, d_false_alarms, d_repeats  int32
 *   d_latency_samples                  int64: the sum over the hits of k * hop + window - onset[p]
 * hits + repeats + false_alarms equals the d_counts of cough_sweep_thresholds at the same thresholds and gap.
 *   1 <= n_thresholds <= COUGH_SCENES_MAX_THRESHOLDS; gap >= 1; hop >= 1; window >= 1; 0 <= n_windows < 2^38.
 *   The truth arrays may be NULL when n_truth == 0 (d_truth_offsets never).
 * n_clips == 0 launches nothing. */
int cough_match_events(const double* d_smoothed, const long long* d_window_offsets, int n_clips, long long n_windows,
                       const double* d_thresholds, int n_thresholds, int gap, const long long* d_truth_offsets,
                       const int* d_k_lo, const int* d_k_hi, const int* d_onset, int n_truth, int hop, int window,
                       int* d_hits, int* d_false_alarms, int* d_repeats, long long* d_latency_samples, void* stream);

/* ------------------------------------------------------------------ the matches at one threshold
 * The same walk and the same classification at one threshold, one thread per recording (not a hot path).
 *   d_truth_window [n_truth] int32: the window that hit event j, or -1.  Every event inside a recording's clamped
 *                  offsets is written.
 *   d_event_class  int32, may be NULL (then d_event_offsets may be too): the class of every window that fired -- 0 hit,
 *                  1 repeat, 2 false alarm -- recording c writing from d_event_offsets[c] on and stopping at
 *                  d_event_offsets[c + 1] (int64 [n_clips + 1], last n_events): with offsets built from the d_counts of
 *                  a sweep at this threshold and gap every slot is written, in the order of cough_list_events.
 *   threshold must not be NaN; gap >= 1; n_events >= 0.
 * (Not cough_list_matches: libcough_amd_dups.so exports that name with another signature, and a program may include
 * both headers and link both libraries.)
 * n_clips == 0 launches nothing. */
int cough_list_event_matches(const double* d_smoothed, const long long* d_window_offsets, int n_clips,
                             long long n_windows, double threshold, int gap, const long long* d_truth_offsets,
                             const int* d_k_lo, const int* d_k_hi, int n_truth, int* d_truth_window,
                             const long long* d_event_offsets, long long n_events, int* d_event_class, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* COUGH_AMD_SCENES_H */
