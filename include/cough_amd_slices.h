/*
 * cough_amd_slices.h -- C-ABI of libcough_amd_slices.so: tile the recordings of a packed clip bank into fixed-length
 * windows at a stride, decide from the short-time energies which windows hold enough active signal, and list the kept
 * ones (the reference's second data stub, prepare_librispeech: a non-cough class "segmented into 1-2 second clips" with
 * silence kept minimal).
 *
 * The nine libraries before this one are pinned (names, order, entry points, ABI versions), so this one is the first of
 * the libraries that come after them; it has a version of its own.  The conventions are those of cough_amd_segments.h:
 * plain pointers and sizes only, `d_` = device (HBM) pointer; every call returns COUGH_OK (0) or a COUGH_E* code of
 * cough_amd.h and leaves a thread-local message for the last-error call below; launches are stream-ordered on `stream`
 * (a hipStream_t; NULL = default stream); no call allocates or synchronises; every argument the host can check is checked
 * before the launch; no kernel uses atomics and every result is formed in a fixed order, so the same input gives the
 * same bits.
 *
 * What lives in device memory (lengths, offsets) cannot be checked by the host before the launch: a kernel never
 * touches more windows of a clip than d_window_offsets gives it, more frames than d_frame_offsets gives it, or more rows
 * than d_row_offsets gives it.
 *
 * Inputs.  d_lengths [n_clips] int32 are the packed bank's clip lengths.  d_energy (float64) and d_frame_offsets
 * [n_clips + 1] int64 are exactly what cough_frame_energy (cough_amd_segments.h) wrote and took: a clip of n samples has
 * F = 1 frame if n < frame_length, else F = 1 + (n - frame_length) / hop_length; frame f covers
 * [f*hop_length, min(f*hop_length + frame_length, n)); clip k's energies are e[f] = d_energy[d_frame_offsets[k] + f].
 * d_window_offsets [n_clips + 1] int64 is the exclusive prefix sum of the clips' window counts W, formed by the host
 * from the lengths.
 *
 * Windows.  Clip k with n samples has W = 1 window [0, n) if n < seg_len; otherwise W = 1 + (n - seg_len) / stride
 * windows and window w is [w*stride, w*stride + seg_len).
 * Frames of a window.  Frame f belongs to window w iff its whole extent lies inside the window; cnt[w] is the number of
 * such frames.  In closed form (what the kernel evaluates), with the window [a, b): if n < frame_length the one frame
 * belongs to the one window; else first = ceil(a / hop_length), last = min(floor((b - frame_length) / hop_length), F - 1)
 * and cnt[w] = max(last - first + 1, 0).
 */
#ifndef COUGH_AMD_SLICES_H
#define COUGH_AMD_SLICES_H

#include "cough_amd.h"

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden: exactly the entry points declared in this header are exported
 * (tests/test_slices_host.py compares `nm -D` of the built library with this list). */
#pragma GCC visibility push(default)

#define COUGH_SLICES_ABI_VERSION 1

int cough_slices_abi_version(void);
const char* cough_slices_last_error(void);  /* thread-local, never NULL */

/* ------------------------------------------------------------------ energies -> kept windows, one wave per clip
 * For clip k with energies e[0 .. F) and windows 0 .. W - 1:
 *   gate        any e[f] not finite: d_peak[k] = NaN, no active frame, no window qualifies.
 *   peak        otherwise E_max = max e[f] and d_peak[k] = E_max; if E_max < floor there is no active frame and no
 *               window qualifies.
 *   activity    thr = fmax(E_max * ratio, floor) (E_max * ratio is one double product); active[f] = e[f] >= thr;
 *               d_clip_active[k] = the number of active frames.
 *   per window  m[w] = the number of active frames among the frames of window w, written to
 *               d_active[d_window_offsets[k] + w]; window w qualifies iff m[w] >= 1 and
 *               double(m[w]) >= min_active * double(cnt[w]) (one double product).
 *   cap         if more than max_windows windows qualify, the max_windows qualifying windows with the largest m are
 *               kept, ties going to the earlier window; otherwise every qualifying window is kept.
 *               d_keep[d_window_offsets[k] + w] = 1 for a kept window, else 0; d_counts[k] = the number kept.
 * Outputs: d_peak [n_clips] float64; d_clip_active and d_counts [n_clips] int32; d_active and d_keep
 * [d_window_offsets[n_clips]] int32, every element written.
 *   seg_len >= frame_length >= 1; hop_length >= 1; stride >= 1; max_windows >= 1 (INT_MAX: no cap); ratio, floor and
 *   min_active finite and >= 0.  A clip may have any number of frames and windows that fits 31 bits: the wave marches
 *   over the clip in chunks of 1024 frames and 64 windows and nothing is sized by the clip.
 * n_clips == 0 launches nothing. */
int cough_window_activity(const double* d_energy, const long long* d_frame_offsets, const int* d_lengths,
                          const long long* d_window_offsets, int n_clips, int frame_length, int hop_length, int seg_len,
                          int stride, int max_windows, double ratio, double floor, double min_active, double* d_peak,
                          int* d_clip_active, int* d_active, int* d_keep, int* d_counts, void* stream);

/* ------------------------------------------------------------------ kept windows -> rows, one wave per clip
 * d_keep, d_active and d_window_offsets as above; d_row_offsets [n_clips + 1] int64 is the exclusive prefix sum of
 * d_counts, formed by the host after its one read of them.  One row per kept window, in clip order and then time order:
 * row d_row_offsets[k] + j is the j-th kept window w of clip k,
 *   d_clip (int64) = k, d_start (int32) = w*stride, d_length (int32) = min(seg_len, n), d_row_active (int32) = m[w].
 * The compaction is a ballot prefix: no atomics.  seg_len >= 1, stride >= 1.  n_clips == 0 launches nothing. */
int cough_list_windows(const int* d_keep, const int* d_active, const int* d_lengths, const long long* d_window_offsets,
                       const long long* d_row_offsets, int n_clips, int seg_len, int stride, long long* d_clip,
                       int* d_start, int* d_length, int* d_row_active, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* COUGH_AMD_SLICES_H */
