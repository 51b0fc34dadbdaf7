/*
 * cough_amd_draws.h -- C-ABI of libcough_amd_draws.so, the companion of libcough_amd.so that draws a training batch's
 * augmentation on the device: the per-clip records of AudioAugmentor.augment and the per-image masks of SpecAugment come
 * from a seeded counter-based generator instead of the host's `random`, and the waveform augmentation reads those
 * records, and the clips themselves, where they already are -- in device memory.
 *
 * cough_amd.h is pinned at ABI v5 with its 53 entry points and the four other companions at version 1 with theirs, so
 * these entry points are exported from a sixth library with a version of its own.  The conventions are those of
 * cough_amd.h: plain pointers and sizes only, `d_` = device (HBM) pointer; every call returns COUGH_OK (0) or a COUGH_E*
 * code of cough_amd.h and leaves a thread-local message for the last-error call below; launches are stream-ordered on
 * `stream` (a hipStream_t; NULL = default stream); no call allocates, copies from the host or synchronises; every
 * argument is checked before the launch; no kernel uses atomics, so the same input gives the same bits.
 *
 * THE DRAW CONTRACT.  Generator: Philox4x32-10, key = seed (low word, high word), counter (slot, row, 0, 1).  The
 * gaussian noise of the same batch counts (sample group, row, 0, 0) under the same key, so the two streams never meet.
 * A 32-bit word x gives u = (x + 0.5) * 2^-32 in float64 (exact, strictly inside (0, 1)); a coin with probability p
 * fires iff u <= p (p = 0 never, p = 1 always: the reference's `random.random() > p -> skip`).  All draw arithmetic is
 * float64, one IEEE operation per operator (no fused multiply-add), conversions to int truncate toward zero:
 *   slot 0 (x, y, z, w)   shift coin x, shift = (int)((double)n * (-0.2 + 0.4 * u_y));
 *                         gain coin z,  gain = (float)(0.7 + 0.6 * u_w)
 *   slot 1                gaussian coin x, gaussian_snr_db = 10 + 20 * u_y;  bank coin z, bank_snr_db = 5 + 15 * u_w
 *   slot 2                bank_index = min((int)(u_x * n_bank), n_bank - 1);  with bl = d_bank_lengths[bank_index] and
 *                         rep = bl < n ? (n / bl + 1) * bl : bl:
 *                         bank_start = min((long long)(u_y * (double)(rep - n + 1)), rep - n);  z unused;
 *                         w is SpecAugment's coin.  The bank step fires only if its coin fired and n_bank > 0.
 *   slot 3 + m            mask m (frequency masks first, then time masks): value = u_x * param,
 *                         minv = u_y * (size - value), start = (int)minv, end = start + (int)value; axis 0 = frequency
 *                         (size = height), 1 = time (size = width)
 * n is the row's length d_lengths[row].  A step that did not fire leaves its fields at shift 0, gain 1, gaussian 0,
 * bank_index -1, both SNRs 0.0, bank_start 0; an image whose coin did not fire gets (0, 0, 0) in every mask.
 * These are the reference's distributions for every draw (/root/reference/src/augmentation.py:77-213, :271-331), not its
 * random stream; its masks are drawn in float32 (torch.rand(1)), these in float64.
 */
#ifndef COUGH_AMD_DRAWS_H
#define COUGH_AMD_DRAWS_H

#include "cough_amd.h"

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden: exactly the entry points declared in this header are exported
 * (tests/test_draws_host.py compares `nm -D` of the built library with this list). */
#pragma GCC visibility push(default)

#define COUGH_DRAWS_ABI_VERSION 1

int cough_draws_abi_version(void);
const char* cough_draws_last_error(void);  /* thread-local, never NULL */

/* ------------------------------------------------------------------ the draws of one batch
 * One thread per row writes the row's record, a cough_aug_clip of cough_amd.h, to d_clips_out[row] and its n_freq_masks +
 * n_time_masks mask triples to d_mask_axis / d_mask_start / d_mask_end, each int32 [n_rows][n_masks]: the layout
 * cough_mask_images reads.
 *   d_lengths       [n_rows] int32, the rows' lengths n >= 1 (a length < 1 yields the blank record)
 *   p_augment       probability of each waveform step; < 0: no waveform augmentor, nothing is written to d_clips_out
 *                   (it and d_lengths may then be NULL)
 *   d_bank_lengths  [n_bank] int32 >= 1, the noise bank's entry lengths (an entry < 1 drops the bank step); NULL when
 *                   n_bank == 0
 *   spec_p          SpecAugment's probability; < 0, or n_freq_masks + n_time_masks == 0: no SpecAugment, the mask
 *                   arrays are not written and may be NULL
 *   n_freq_masks + n_time_masks <= COUGH_MAX_MASKS; on an axis that has masks 1 <= mask_param <= size (height for
 *   frequency, width for time); a probability that is NaN is refused.
 * n_rows == 0, or neither of the two switched on, launches nothing. */
int cough_draw_batch(unsigned long long seed, int n_rows, const int* d_lengths, double p_augment, int n_bank,
                     const int* d_bank_lengths, double spec_p, int n_freq_masks, int freq_mask_param, int n_time_masks,
                     int time_mask_param, int height, int width, cough_aug_clip* d_clips_out, int* d_mask_axis,
                     int* d_mask_start, int* d_mask_end, void* stream);

/* ------------------------------------------------------------------ waveform augmentation from device records
 * What cough_augment_waveforms of cough_amd.h computes (the same kernel, the same arithmetic, the same counter-based gaussian noise
 * keyed by `seed`), with everything the host used to hand over read from DEVICE memory: row b is the d_lengths[b]
 * samples at d_src + d_row_offsets[b], read in place (a row may start at any element of a packed bank: no gather into a
 * matrix first), its record is d_clips[b], and the noise bank's tables d_bank_offsets (int64) / d_bank_lengths (int32),
 * [n_bank] each, are device arrays too.  d_out: [n_rows][n_samples] float32, samples [len_b, n_samples) written as 0;
 * it must not overlap d_src.  A resolve kernel first turns each record into the augment kernel's form in d_workspace
 * (10^(snr_db / 10) in float64, rounded to float; bank_start modulo the entry length; the entry's offset).
 *
 * The host cannot check records that live on the device, so the resolve kernel makes a record it cannot use harmless
 * instead of refusing it:
 *   a length outside 1..n_samples            is clamped to 0..n_samples (a row of length 0 is written as zeros)
 *   bank_index outside [0, n_bank)           drops the bank step (-1 is "not fired")
 *   an entry with length < 1 or not inside [0, bank_numel)   drops the bank step
 *   bank_start outside [0, rep - len_b]      drops the bank step (rep as in the draw contract)
 *   gaussian other than 0 or 1               counts as 0
 *   shift                                    any value: samples shifted out of [0, len_b) read as 0, so |shift| >= len_b
 *                                            gives a silent clip (the value is clamped to +-len_b, which is the same clip)
 * Nothing is read outside the rows and the bank entries, and nothing written outside d_out and d_workspace, whatever
 * d_clips holds; the caller answers for d_row_offsets[b] + d_lengths[b] lying inside d_src.
 *   n_samples <= 2^30;  d_workspace: 256-byte aligned, >= cough_augment_rows_drawn_workspace_bytes(n_rows)
 * n_rows == 0 launches nothing. */
size_t cough_augment_rows_drawn_workspace_bytes(int n_rows);
int cough_augment_rows_drawn(const float* d_src, const long long* d_row_offsets, const int* d_lengths, int n_rows,
                             int n_samples, const cough_aug_clip* d_clips, const float* d_bank, long long bank_numel,
                             const long long* d_bank_offsets, const int* d_bank_lengths, int n_bank,
                             unsigned long long seed, float* d_out, void* d_workspace, size_t workspace_bytes, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* COUGH_AMD_DRAWS_H */
