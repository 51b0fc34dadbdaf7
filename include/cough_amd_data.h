/*
 * cough_amd_data.h -- C-ABI of libcough_amd_data.so, the companion of libcough_amd.so for the input pipeline of the
 * training loop (the reference's src/dataset.py: what CoughDataset.__getitem__ :121-173 does to a clip around the
 * augmentor and the featuriser, for a whole batch of clips that live in device memory).
 *
 * cough_amd.h is pinned at ABI v5 with its 53 entry points and cough_amd_loop.h at version 1, so what the loader needs
 * on the device is exported from a third library with a version of its own.  The conventions are those of cough_amd.h:
 * plain pointers and sizes only, `d_` = device (HBM) pointer; every call returns COUGH_OK (0) or a COUGH_E* code of
 * cough_amd.h and leaves a thread-local message for the last-error call below; launches are stream-ordered on `stream`
 * (a hipStream_t; NULL = default stream); no call allocates or synchronises; every argument is checked before the
 * launch; no kernel uses atomics, so the same input gives the same bits.
 *
 * What lives in device memory (row offsets, lengths, mask triples) cannot be checked by the host before the launch:
 * the kernels clamp a length to its row and treat a mask triple they cannot use as empty, so nothing is WRITTEN out
 * of bounds whatever those arrays hold; the caller answers for d_row_offsets[r] + d_lengths[r] lying inside d_src.
 */
#ifndef COUGH_AMD_DATA_H
#define COUGH_AMD_DATA_H

#include "cough_amd.h"

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden: exactly the entry points declared in this header are exported
 * (tests/test_data_host.py compares `nm -D` of the built library with this list). */
#pragma GCC visibility push(default)

#define COUGH_DATA_ABI_VERSION 1

int cough_data_abi_version(void);
const char* cough_data_last_error(void);  /* thread-local, never NULL */

/* ------------------------------------------------------------------ ragged rows -> matrix
 * Assembles a batch of clips of different lengths from a packed bank into the [n_rows][row_len] matrix that
 * cough_augment_waveforms takes: row r of d_out (at d_out + r*out_stride) receives
 * d_src[d_row_offsets[r] .. d_row_offsets[r] + d_lengths[r]), then zeros up to row_len.
 *   d_row_offsets [n_rows] int64, in elements (rows may start at any element: 4-byte alignment only)
 *   d_lengths     [n_rows] int32, 1 <= len <= row_len (a value outside 0..row_len is clamped to it)
 *   out_stride >= row_len, in elements; d_out must not overlap d_src
 * n_rows == 0 launches nothing. */
int cough_gather_rows(const float* d_src, const long long* d_row_offsets, const int* d_lengths, int n_rows,
                      float* d_out, long long out_stride, int row_len, void* stream);

/* ------------------------------------------------------------------ normalize -> pad_or_trim of a batch
 * The mono case of cough_prepare_clip for a whole batch, one workgroup per row: AudioPreprocessor.normalize
 * (/root/reference/src/preprocessing.py:199-212) then pad_or_trim (:358-385).  Row r is the d_lengths[r] samples at
 * d_src + d_row_offsets[r]; its peak is max |x| over ALL of them (the reference normalises before it trims); with
 * COUGH_PREP_NORMALIZE every sample is divided by the peak (an IEEE division) when the peak is > 0 and no sample is
 * NaN (`NaN > 0` is false in the reference: such a row stays unscaled, as an all-zero one does).  The row is then
 * centre-trimmed (start = (len - out_len) / 2) or zero-padded (left = (out_len - len) / 2, the odd sample on the
 * right) into d_out + r*out_len.
 * Rows start at arbitrary element offsets, so the same call serves a matrix (offset r*stride) and a packed bank
 * (gather, normalise and trim in one launch).  d_out must not overlap the rows read.
 *   d_row_offsets [n_rows] int64 (elements), d_lengths [n_rows] int32 >= 1 (a length < 1 yields a zero row)
 *   flags: COUGH_PREP_NORMALIZE (cough_amd.h) or 0
 * n_rows == 0 launches nothing. */
int cough_prepare_rows(const float* d_src, const long long* d_row_offsets, const int* d_lengths, int n_rows,
                       float* d_out, int out_len, int flags, void* stream);

/* ------------------------------------------------------------------ SpecAugment, a mask set per image
 * cough_mask_axes with masks of its own for every image, as a Dataset that calls SpecAugment per item produces them
 * (/root/reference/src/dataset.py:169-171): d_in / d_out [n_images][height][width] float32 (d_out may equal d_in);
 * mask k of image b zeroes rows (d_axis = 0, frequency) or columns (d_axis = 1, time) d_start <= i < d_end, each
 * array device int32 [n_images][n_masks], 0 <= n_masks <= COUGH_MAX_MASKS.  start == end is an empty mask: an image
 * whose coin did not fire passes through with all of its masks empty.  A triple with another axis value masks
 * nothing.  n_masks == 0 copies (or, in place, does nothing); the three arrays may then be NULL.
 * n_images == 0 launches nothing. */
int cough_mask_images(const float* d_in, float* d_out, int n_images, int height, int width, int n_masks,
                      const int* d_axis, const int* d_start, const int* d_end, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* COUGH_AMD_DATA_H */
