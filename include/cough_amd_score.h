/*
 * cough_amd_score.h -- C-ABI of libcough_amd_score.so, the companion of libcough_amd.so for scoring whole recordings
 * offline: what the reference's engine (src/inference.py: process_audio_chunk :191-241) does to the per-window cough
 * probabilities of ONE live stream -- a deque mean, a threshold, a debounce -- for every window of every recording of a
 * corpus at once, and at many thresholds at once.
 *
 * cough_amd.h is pinned at ABI v5 with its 53 entry points, cough_amd_loop.h, cough_amd_data.h and
 * cough_amd_segments.h at version 1, so what the scorer needs on the device is exported from a fifth library with a
 * version of its own.  The conventions are those of cough_amd.h: plain pointers and sizes only, `d_` = device (HBM)
 * pointer; every call returns COUGH_OK (0) or a COUGH_E* code of cough_amd.h and leaves a thread-local message for the
 * last-error call below; launches are stream-ordered on `stream` (a hipStream_t; NULL = default stream); no call
 * allocates or synchronises; every argument is checked before the launch; no kernel uses atomics and every sum is
 * formed in a fixed order, so the same input gives the same bits.
 *
 * What lives in device memory (the offset arrays) cannot be checked by the host before the launch: the kernels clamp
 * every offset and count they read to the array sizes they were given (n_windows, n_events), so nothing is read or
 * written out of bounds whatever those arrays hold.
 *
 * Windows.  The windows of all recordings lie end to end: recording c owns windows d_window_offsets[c] ..
 * d_window_offsets[c + 1] (int64 [n_clips + 1], ascending, first 0, last n_windows); window k of a recording is its
 * k-th in time.  A recording may own no window.
 */
#ifndef COUGH_AMD_SCORE_H
#define COUGH_AMD_SCORE_H

#include "cough_amd.h"

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden: exactly the entry points declared in this header are exported
 * (tests/test_score_host.py compares `nm -D` of the built library with this list). */
#pragma GCC visibility push(default)

#define COUGH_SCORE_ABI_VERSION 1
#define COUGH_MAX_SMOOTHING 32         /* windows in the mean at most */
#define COUGH_MAX_THRESHOLDS 1024      /* thresholds per sweep at most */

int cough_score_abi_version(void);
const char* cough_score_last_error(void);  /* thread-local, never NULL */

/* ------------------------------------------------------------------ the engine's deque mean, for every window
 * d_smoothed[i] for window k of its recording = float(np.mean(deque(p[max(0, k - W + 1) .. k]))): the float32
 * probabilities widened to float64 and added in numpy's order -- fewer than 8 values left to right; 8 or more with
 * eight accumulators r[j] = a[j], r[j] += a[i + j] over the whole blocks of 8, ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)),
 * then the remaining values in order -- and the sum divided by the count.  History never crosses recordings; a NaN
 * among the values gives NaN.  One thread per window; it finds its recording by a search of d_window_offsets.
 *   1 <= smoothing_window <= COUGH_MAX_SMOOTHING; 0 <= n_windows < 2^38.
 * n_clips == 0 or n_windows == 0 launches nothing. */
int cough_smooth_windows(const float* d_prob, const long long* d_window_offsets, int n_clips, long long n_windows,
                         int smoothing_window, double* d_smoothed, void* stream);

/* ------------------------------------------------------------------ the debounced decision at many thresholds
 * At threshold t window k of a recording fires iff s[k] >= t and k >= next, where next is 0 until a window of that
 * recording has fired and j + gap after window j has; a NaN never fires.  One wave per (recording, 64 thresholds): a
 * lane owns a threshold and walks the recording's windows in time order.
 *   d_thresholds   [n_thresholds] float64, 1 <= n_thresholds <= COUGH_MAX_THRESHOLDS (values are data: a NaN threshold
 *                  never fires)
 *   gap >= 1
 * Outputs, each of which may be NULL:
 *   d_counts       [n_clips][n_thresholds] int32: windows that fired
 *   d_first_window [n_clips][n_thresholds] int32: the first of them, -1 if none
 *   d_peak_conf    [n_clips] float64: the largest s[k] that is not NaN; NaN for a recording without one
 *   d_peak_window  [n_clips] int32: the first k that holds it; -1 for a recording without one
 * n_clips == 0 launches nothing. */
int cough_sweep_thresholds(const double* d_smoothed, const long long* d_window_offsets, int n_clips, long long n_windows,
                           const double* d_thresholds, int n_thresholds, int gap, int* d_counts, int* d_first_window,
                           double* d_peak_conf, int* d_peak_window, void* stream);

/* ------------------------------------------------------------------ the windows that fire at one threshold
 * The same walk (the same device function decides) at one threshold, one wave per recording: the ballot of s >= t over
 * 64 windows, then the set bits at or after `next`.  Recording c writes its events in time order from
 * d_event_offsets[c] on and stops at d_event_offsets[c + 1] (int64 [n_clips + 1], ascending, last n_events): with
 * offsets built from the d_counts of a sweep at this threshold and gap every slot is written.
 *   d_event_window [n_events] int32: k;   d_event_conf [n_events] float64: s[k]
 *   threshold must not be NaN; gap >= 1; n_events >= 0.
 * n_clips == 0 or n_events == 0 launches nothing. */
int cough_list_events(const double* d_smoothed, const long long* d_window_offsets, int n_clips, long long n_windows,
                      double threshold, int gap, const long long* d_event_offsets, long long n_events,
                      int* d_event_window, double* d_event_conf, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* COUGH_AMD_SCORE_H */
