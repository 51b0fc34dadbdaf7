/*
 * cough_amd_warp.h -- C-ABI of libcough_amd_warp.so, the companion of libcough_amd.so that runs the waveform chain's
 * speed perturbation on the device: a windowed-sinc resampler that takes a rate pair PER ROW and evaluates each tap's
 * coefficient on the fly, so no polyphase table exists.  (torchaudio's table for a pair such as 15999 -> 16000, which
 * has no common factor, would hold 16000 x 16013 coefficients of which about 14 per row are not zero.)
 *
 * cough_amd.h is pinned at ABI v5 with its 53 entry points and the six other companions at version 1 with theirs, so
 * these entry points are exported from an eighth library with a version of its own.  The conventions are those of
 * cough_amd.h: plain pointers and sizes only, `d_` = device (HBM) pointer; every call returns COUGH_OK (0) or a COUGH_E*
 * code of cough_amd.h and leaves a thread-local message for the last-error call below; launches are stream-ordered on
 * `stream` (a hipStream_t; NULL = default stream); no call allocates, copies from the host or synchronises; every
 * argument is checked before the launch; no kernel uses atomics, so the same input gives the same bits.
 *
 * THE RESAMPLER'S ARITHMETIC, pinned to cough_resample with the table of T.Resample(orig, new) (sinc_interp_hann,
 * lowpass_filter_width 6, rolloff 0.99) so that the two agree.  For a row x of n samples with plan (shift, orig, new):
 *   x_s[i] = x[i - shift] for 0 <= i - shift < n, else 0, i = 0 .. n-1      (the time shift, fused into the read: the
 *            reference shifts BEFORE it changes the speed)
 *   n'     = ceil(n * new / orig), in exact integer arithmetic
 *   width  = ceil(6 * orig / (0.99 * min(orig, new)))                       (float64: min * 0.99, then 6 * orig / that)
 *   for output m = 0 .. n'-1, inputs i = floor(m * orig / new) - width .. floor(m * orig / new) + width + 1 ascending:
 *     num = i * new - m * orig                                              (an exact 64-bit integer)
 *     t   = clamp(num * c, -6, 6),  c = 0.99 * min(orig, new) / (orig * new)
 *     h   = sinc(pi t) * cos^2(pi t / 12) * (0.99 * min(orig, new) / orig)  (float64, rounded ONCE to float32;
 *            sinc(0) = 1; at |t| = 6 the value is below 1e-40 and rounds to 0)
 *     y[m] = fmaf(x_s[i], h, y[m])                                          (float32, starting from 0; i outside
 *            0 .. n-1 contributes nothing)
 * The formula depends on orig / new only, so the pair need not be reduced by its gcd.  The kernel may advance
 * sin(pi t) and cos(pi t / 12) from tap to tap by a float64 rotation seeded with one sincos per output; a coefficient
 * may therefore differ from the one evaluated directly by one float32 rounding, no more.
 *   orig == new   y = x_s, a bit-exact copy (torchaudio returns its input for equal rates)
 *
 * THE SPEED DRAW CONTRACT, in the conventions of cough_amd_draws.h: Philox4x32-10, key = seed (low word, high word); a
 * 32-bit word x gives u = (x + 0.5) * 2^-32 in float64; a coin with probability p fires iff u <= p; all arithmetic is
 * float64, one IEEE operation per operator (no fused multiply-add), conversions to int truncate toward zero.
 *   counter (0, row, 0, 1)   slot 0 of cough_amd_draws.h, evaluated with the ORIGINAL length n:
 *                            shift coin x, shift = (int)((double)n * (-0.2 + 0.4 * u_y))
 *   counter (0, row, 0, 2)   speed coin x;  factor = lo + (hi - lo) * u_y;
 *                            orig = (int)(factor * (double)sample_rate), new = sample_rate   (torchaudio's `speed`)
 * The other draws of the batch count (slot, row, 0, 1) and its gaussian noise (group, row, 0, 0), so the streams never
 * meet.  A step that did not fire leaves shift 0, orig = new = sample_rate.  The rest of the row's record is what
 * cough_draw_batch draws for the new length n'; its shift word is then cleared (cough_clear_shifts), because the shift
 * has already been applied by the resampler's read.
 */
#ifndef COUGH_AMD_WARP_H
#define COUGH_AMD_WARP_H

#include "cough_amd.h"

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden: exactly the entry points declared in this header are exported
 * (tests/test_warp_host.py compares `nm -D` of the built library with this list). */
#pragma GCC visibility push(default)

#define COUGH_WARP_ABI_VERSION 1
#define COUGH_WARP_MAX_RATE (1 << 20)   /* 1 <= orig, new <= 2^20 */
#define COUGH_WARP_MAX_RATIO 4          /* 1/4 <= orig / new <= 4 */

int cough_warp_abi_version(void);
const char* cough_warp_last_error(void);  /* thread-local, never NULL */

/* One row's plan.  12 bytes, three int32. */
typedef struct cough_warp_plan {
    int shift;     /* time_shift samples: > 0 right (zeros on the left), < 0 left */
    int orig;      /* the rate the row is taken to have ... */
    int new_rate;  /* ... and the rate it is resampled to: n' = ceil(n * new_rate / orig) */
} cough_warp_plan;

/* ------------------------------------------------------------------ per-row resampling
 * Row b is the d_lengths[b] samples at d_src + d_row_offsets[b] (int64 element offsets), read in place -- a row may
 * start at any element of a packed buffer -- and its plan is d_plans[b].  d_out: [n_rows][n_samples] float32; row b
 * receives its min(n', n_samples) resampled samples and zeros behind them.  d_new_lengths: NULL, or [n_rows] int32 that
 * receives min(n', n_samples).  d_out must not overlap d_src.
 *
 * The host cannot check arrays that live on the device, so the kernel makes an entry it cannot use harmless:
 *   orig or new_rate outside 1 .. 2^20, or orig / new_rate outside [1/4, 4]   the row is treated as orig == new_rate
 *   a length outside 0 .. 2^30                                                is clamped to that range
 *   shift                                                                     any value (|shift| >= n: a silent row)
 * Nothing is read outside the rows, and nothing written outside d_out and d_new_lengths, whatever the device arrays
 * hold; the caller answers for d_row_offsets[b] + d_lengths[b] lying inside d_src.
 *   1 <= n_samples <= 2^30;  n_rows * ceil(n_samples / 1024) <= 2^24 (the grid);  n_rows == 0 launches nothing. */
int cough_warp_rows(const float* d_src, const long long* d_row_offsets, const int* d_lengths, int n_rows,
                    const cough_warp_plan* d_plans, float* d_out, int n_samples, int* d_new_lengths, void* stream);

/* ------------------------------------------------------------------ the speed draws of one batch
 * One thread per row writes the row's plan to d_plans_out[row] and its new length n' = ceil(n * new / orig), at most
 * 2^30, to d_new_lengths_out[row], by the contract above.  d_lengths: [n_rows] int32, the rows' lengths n (a length < 1 yields
 * the blank plan (0, sample_rate, sample_rate) and n' = 0; a length above 2^30 counts as 2^30).
 *   p_augment in [0, 1]: the probability of the shift and of the speed step;  1/4 <= lo <= hi <= 4;
 *   1 <= sample_rate <= 2^20 with 4 * (int)(lo * sample_rate) >= sample_rate and, when hi > 1,
 *   (int)(hi * sample_rate) < 2^20, so every drawn pair is one cough_warp_rows accepts.  n_rows == 0 launches nothing. */
int cough_draw_speed(unsigned long long seed, int n_rows, const int* d_lengths, double p_augment, double lo, double hi,
                     int sample_rate, cough_warp_plan* d_plans_out, int* d_new_lengths_out, void* stream);

/* Sets the shift word of n_rows records of cough_amd.h's cough_aug_clip to 0: what cough_draw_batch drew for a row the
 * resampler has already shifted. */
int cough_clear_shifts(cough_aug_clip* d_clips, int n_rows, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* COUGH_AMD_WARP_H */
