/*
 * cough_amd_windows.h -- C-ABI of libcough_amd_windows.so, the companion of libcough_amd.so that composes a batch of
 * training windows in one launch: per row a stretch of background read cyclically, and up to four event clips (coughs,
 * hard negatives) laid over it at any phase -- reaching in front of the window, past its end, over each other -- each at
 * a chosen SNR against the power of the background the window holds.  It is cough_amd_scenes.h's span power, gain and mix
 * (the same arithmetic, operation for operation) fused into one kernel for rows of one width, so that a loader can
 * compose every batch anew; what cough_mix_scenes refuses by contract (overlapping events, events across an edge) is
 * the point here.
 *
 * cough_amd.h is pinned at ABI v5 with its 53 entry points and every companion at version 1, so this lives in a library
 * of its own with a version of its own.  The conventions are those of cough_amd.h: plain pointers and sizes only, `d_` =
 * device (HBM) pointer; every call returns COUGH_OK (0) or a COUGH_E* code of cough_amd.h and leaves a thread-local
 * message for the last-error call below; launches are stream-ordered on `stream` (a hipStream_t; NULL = default stream);
 * no call allocates or synchronises; every argument the host can see is checked before the launch; no kernel uses
 * atomics and every sum is formed in a fixed order, so the same input gives the same bits.
 *
 * The row plans live in device memory and cannot be checked by the host: the kernel clamps what they hold to the sizes
 * it was given (below), so nothing is read or written out of bounds whatever they hold.
 *
 * The clips of a packed bank: clip k is d_bank[offset[k] .. offset[k] + length[k]), offsets int64 in elements (a clip
 * starts at any element: 4-byte alignment only), lengths int32.
 */
#ifndef COUGH_AMD_WINDOWS_H
#define COUGH_AMD_WINDOWS_H

#include "cough_amd.h"

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden: exactly the entry points declared in this header are exported
 * (tests/test_windows_host.py compares `nm -D` of the built library with this list). */
#pragma GCC visibility push(default)

#define COUGH_WINDOWS_ABI_VERSION 1
#define COUGH_WINDOWS_MAX_EVENTS 4            /* events per row at most */
#define COUGH_WINDOWS_MAX_WIDTH (1 << 20)     /* samples per row at most */
#define COUGH_WINDOWS_THREADS 256             /* threads of a row's workgroup: the order of the power sum is tied to it */
#define COUGH_WINDOWS_KEEP_WIDTH 16384        /* up to this width a row's background is read from memory once */

int cough_windows_abi_version(void);
const char* cough_windows_last_error(void);  /* thread-local, never NULL */

/* One row's plan: 80 bytes, 8-byte aligned, in this order and with no padding.
 *   background   clip of the background bank, -1 for silence
 *   bg_start     the first background sample the row reads
 *   bg_gain      float32
 *   n_events     0 .. COUGH_WINDOWS_MAX_EVENTS; the events are slots 0 .. n_events - 1
 *   clip[e]      clip of the event bank
 *   onset[e]     where the clip's first sample falls, in samples from the row's first; may be negative
 *   snr_linear[e] float64, 10 ** (snr_db / 10), computed by the host (there is no device pow) */
typedef struct cough_window_plan {
    int background;
    int bg_start;
    float bg_gain;
    int n_events;
    int clip[COUGH_WINDOWS_MAX_EVENTS];
    int onset[COUGH_WINDOWS_MAX_EVENTS];
    double snr_linear[COUGH_WINDOWS_MAX_EVENTS];
} cough_window_plan;

/* ------------------------------------------------------------------ a batch of composed windows, one launch
 * Row r of d_out [n_rows][width] float32 is composed from d_plans[r] by one workgroup of COUGH_WINDOWS_THREADS threads.
 * With B the row's background clip of n_b samples and E_e, n_e the clip and length of its event e:
 *
 * Background power (float64).  P_bg = (sum over i = 0 .. width - 1 of double(B[(bg_start + i) mod n_b])^2) / width, in
 * the order of cough_span_power: thread t adds the squares of samples i = t, t + 256, t + 512, ... in ascending i,
 * starting from 0.0; the 256 partial sums are added pairwise, p[t] += p[t ^ m] for m = 1, 2, 4, 8, 16, 32 (inside each
 * wave of 64), and the four wave sums as (w0 + w1) + (w2 + w3).  Its bits are those cough_span_power gives for the span
 * (clip, bg_start, width).
 * Gain.  gain[e] = float32(sqrt(((snr_linear[e] * (double(bg_gain) * double(bg_gain))) * P_bg) / d_p_ev[clip[e]])),
 * float64 operations in that order, rounded to float32 once: cough_scene_gains' expression.  d_p_ev [n_event_clips]
 * float64 holds every event clip's mean power over the whole clip (cough_span_power of the clip from 0 over its
 * length).  The gain is 1.0 when P_bg or d_p_ev[clip[e]] is 0 or not finite.
 * Mix (float32), per sample i:
 *   acc = bg_gain * B[(bg_start + i) mod n_b]                              (one rounded product)
 *   for e = 0 .. n_events - 1 in this order, where onset[e] <= i < onset[e] + n_e:
 *       acc = fmaf(gain[e], E_e[i - onset[e]], acc)
 *   out[i] = acc
 * Events may overlap each other; an event that reaches in front of sample 0 or past width is cut there; an event that
 * misses the row contributes nothing.  A background that is -1 or whose clamped length is 0 is silence: acc starts at
 * +0.0 (whatever bg_gain is) and P_bg is 0.  NaN and Inf samples get no rule of their own: the arithmetic decides.
 *
 * What the kernel clamps: n_events to 0 .. COUGH_WINDOWS_MAX_EVENTS; a negative bg_start to 0 and one past the clip
 * mod its length; a background outside 0 .. n_bg_clips - 1 is silence; an event whose clip lies outside 0 ..
 * n_event_clips - 1 is skipped (its gain is reported as 1.0); every clip is cut to the n_bg_samples / n_ev_samples of
 * its bank.
 *
 * Optional outputs, either may be NULL: d_p_bg_out [n_rows] float64, the rows' P_bg; d_gains_out [n_rows][4] float32, the
 * gains of slots 0 .. n_events - 1 and 0.0 in the slots behind them.
 *
 * Every row is composed from its own plan alone: a row gives the same bits alone and in any batch.  For width <=
 * COUGH_WINDOWS_KEEP_WIDTH the background samples stay in registers between the power sum and the mix and are read from
 * memory once; a wider row reads them twice.  The cyclic read costs no modulo per sample (a cyclic index per thread
 * that advances by 256 mod n_b with one conditional subtraction), and every stream is read and written 4 bytes per
 * lane, consecutive lanes on consecutive samples, whatever 4-byte phase a clip or d_out has.
 *   1 <= width <= COUGH_WINDOWS_MAX_WIDTH; n_rows, n_bg_clips, n_event_clips, n_bg_samples, n_ev_samples >= 0.
 *   d_out must not overlap d_bg or d_ev.  d_bg and its tables may be NULL when n_bg_clips == 0 (every row is then
 *   silence), d_ev, its tables and d_p_ev when n_event_clips == 0.
 * n_rows == 0 launches nothing. */
int cough_compose_windows(const float* d_bg, long long n_bg_samples, const long long* d_bg_offsets,
                          const int* d_bg_lengths, int n_bg_clips, const float* d_ev, long long n_ev_samples,
                          const long long* d_ev_offsets, const int* d_ev_lengths, const double* d_p_ev,
                          int n_event_clips, const cough_window_plan* d_plans, int n_rows, int width, float* d_out,
                          double* d_p_bg_out, float* d_gains_out, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* COUGH_AMD_WINDOWS_H */
