/*
 * cough_amd_windraw.h -- C-ABI of libcough_amd_windraw.so, the companion of libcough_amd.so that draws a batch's window
 * plans on the device: the 80-byte records cough_compose_windows of cough_amd_windows.h composes from, and the rows'
 * labels, come from a seeded counter-based generator instead of the host's numpy, so a loader of composed windows
 * uploads no plan, writes no label from the host and runs no numpy per batch.
 *
 * cough_amd.h is pinned at ABI v5 with its 53 entry points, every companion at version 1 with its own, and
 * libcough_amd_windows.so at exactly its three, so this entry point is exported from a library of its own with a version
 * of its own.  The conventions are those of cough_amd.h: plain pointers and sizes only, `d_` = device (HBM) pointer;
 * every call returns COUGH_OK (0) or a COUGH_E* code of cough_amd.h and leaves a thread-local message for the last-error
 * call below; launches are stream-ordered on `stream` (a hipStream_t; NULL = default stream); no call allocates, copies
 * from the host or synchronises; every argument is checked before the launch; no kernel uses atomics, so the same input
 * gives the same bits.
 *
 * THE DRAW CONTRACT.  Generator: Philox4x32-10, key = seed (low word, high word), counter (slot, row, 0, 6).  The chain
 * behind the composer counts last words 0 to 5 under the same key (the gaussian noise 0, cough_draw_batch 1, the speed,
 * pitch, reverb and channel draws 2 to 5), so one batch seed serves the plan and the chain and the streams never meet.
 * A 32-bit word x gives u = (x + 0.5) * 2^-32 in float64 (exact, strictly inside (0, 1)); a coin with probability p
 * fires iff u <= p (p = 0 never, p = 1 always); an integer in [lo, hi] is
 *     lo + min((long long)(u * (double)(hi - lo + 1)), hi - lo).
 * All draw arithmetic is float64, one IEEE operation per operator (no fused multiply-add), conversions to an integer
 * truncate toward zero:
 *   slot 0 (x, y, z, w)   x: background, an integer in [0, n_bg - 1];  y: bg_start, an integer in [0, n_b - 1] with
 *                         n_b = d_bg_lengths[background];  z: bg_gain = (float)(bg_gain_lo + (bg_gain_hi - bg_gain_lo) * u);
 *                         w: the cough coin against p_cough
 *   slot 1                x: the number of coughs, an integer in [coughs_lo, coughs_hi] (0 if the cough coin did not
 *                         fire);  y: the distractor coin against p_distractor;  z: the number of distractors, an integer
 *                         in [1, 2] cut to 4 - the number of coughs (0 if the coin did not fire, or n_distractors == 0);
 *                         w unused
 *   slot 2 + e, e = 0..3  event slot e.  x: the cough pick, d_cough_clips[an integer in [0, n_coughs - 1]];  y: the
 *                         distractor pick, d_distractor_clips[an integer in [0, n_distractors - 1]];  z: the SNR level
 *                         j = z >> 22 (the word's top ten bits), snr_linear = d_snr_linear[j];  w: the onset, an
 *                         integer in [lowest, highest]
 * The coughs take the first slots of a row and read the cough pick, the distractors take the next and read the
 * distractor pick; n_events is their sum.  With n_c = d_ev_lengths[clip] the drawn clip's length, m =
 * min_overlap_samples, m_c = min(m, n_c) and need = min(n_c, (long long)ceil((double)m_c / rho_min)):
 *     lowest = margin + need - n_c,    highest = width - margin - need
 * so at least `need` samples of the clip lie inside [margin, width - margin): rule 7 of cough_detector_amd/windows.py,
 * with the same float64 division and ceil as the host's draw_window_plan.
 * A slot that is not used is written as clip = -1, onset = 0, snr_linear = 1.0 (what WindowPlan.records() writes for it)
 * and its block is not drawn.  n_bg == 0, or a background whose length is < 1, gives background = -1, bg_start = 0.
 * d_labels[row] = 1 if the row holds a cough, else 0.
 *
 * How this differs from draw_window_plan.  The distributions are its own but for one: the SNR is not uniform over the
 * range in dB, it is one of COUGH_WINDRAW_SNR_LEVELS = 1024 equally likely levels that the HOST works out once,
 *     d_snr_linear[j] = 10 ** ((lo + (hi - lo) * (j + 0.5) / 1024) / 10)      (float64)
 * the centres of 1024 equal steps of the range (0.015 dB apart for the default 5..20 dB).  There is no device pow -- as
 * cough_draw_pitch picks from a host table of rates -- so the records do not depend on a math library and can be compared
 * bit for bit.  The random stream is Philox by counter, not numpy's Generator(Philox(seed)): a seeded run repeats itself,
 * not a host-drawn plan.
 */
#ifndef COUGH_AMD_WINDRAW_H
#define COUGH_AMD_WINDRAW_H

#include "cough_amd.h"
#include "cough_amd_windows.h" /* cough_window_plan, COUGH_WINDOWS_MAX_EVENTS, COUGH_WINDOWS_MAX_WIDTH */

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden: exactly the entry points declared in this header are exported
 * (tests/test_windraw_host.py compares `nm -D` of the built library with this list). */
#pragma GCC visibility push(default)

#define COUGH_WINDRAW_ABI_VERSION 1
#define COUGH_WINDRAW_SNR_LEVELS 1024         /* entries of d_snr_linear: the word's top ten bits pick one */
#define COUGH_WINDRAW_THREADS 64              /* threads of a workgroup: one row each */

int cough_windraw_abi_version(void);
const char* cough_windraw_last_error(void);  /* thread-local, never NULL */

/* ------------------------------------------------------------------ the window plans of one batch, one launch
 * One thread per row writes the row's record to d_plans[row] (the 80-byte cough_window_plan of cough_amd_windows.h, 8-byte
 * aligned) and its label to d_labels[row] (int64), by the draw contract above.
 *   d_bg_lengths        [n_bg] int32, the background bank's clip lengths; NULL when n_bg == 0 (every row is then silence)
 *   d_ev_lengths        [n_ev] int32, the event bank's clip lengths; NULL when n_ev == 0.  A length < 0 counts as 0
 *   d_cough_clips       [n_coughs] int32, the clips of the event bank that are coughs; NULL when n_coughs == 0
 *   d_distractor_clips  [n_distractors] int32, the clips of the event bank that are hard negatives; NULL when
 *                       n_distractors == 0
 *   d_snr_linear        [COUGH_WINDRAW_SNR_LEVELS] float64, the table above
 *   margin, rho_min     the inner window of rule 7: edge_margin / speed_ratios of the waveform chain behind the composer,
 *                       0 and 1.0 without one
 * Refused with COUGH_EINVAL: a negative n_rows, n_bg, n_ev, n_coughs, n_distractors or margin; a probability that is NaN
 * or outside 0..1; coughs_lo / coughs_hi outside 1 <= lo <= hi <= COUGH_WINDOWS_MAX_EVENTS; p_cough > 0 with n_coughs
 * == 0; p_distractor > 0 with n_distractors == 0; rho_min outside (0, 1]; min_overlap_samples < 1; width outside 1 ..
 * COUGH_WINDOWS_MAX_WIDTH; an inner window width - 2 * margin smaller than ceil(min_overlap_samples / rho_min); a gain
 * that is not finite or does not fit a float32; a NULL pointer that is needed; int32 arrays that are not 4-byte aligned,
 * d_snr_linear, d_plans or d_labels that are not 8-byte aligned.
 * The caller answers for the two index lists lying inside the event bank (a loader builds them from the bank's host
 * labels).  The kernel still reads nothing outside d_ev_lengths: a listed index outside 0 .. n_ev - 1 is written to the
 * record as it is, with onset 0 -- cough_compose_windows skips such an event.
 * Every row is drawn from (seed, row) alone: the first k rows of a larger batch are a batch of k.
 * n_rows == 0 launches nothing. */
int cough_draw_window_plans(unsigned long long seed, int n_rows, int width, const int* d_bg_lengths, int n_bg,
                            const int* d_ev_lengths, int n_ev, const int* d_cough_clips, int n_coughs,
                            const int* d_distractor_clips, int n_distractors, double p_cough, int coughs_lo, int coughs_hi,
                            double p_distractor, double bg_gain_lo, double bg_gain_hi, const double* d_snr_linear,
                            int min_overlap_samples, int margin, double rho_min, cough_window_plan* d_plans,
                            long long* d_labels, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* COUGH_AMD_WINDRAW_H */
