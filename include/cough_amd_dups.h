/*
 * cough_amd_dups.h -- C-ABI of libcough_amd_dups.so: find copies of a clip in a corpus.  A binary fingerprint in the
 * style of Haitsma and Kalker ("A Highly Robust Audio Fingerprinting System", ISMIR 2002) is taken from the mel rows of
 * the feature image the featuriser already computes, and every pair of clips is compared at a few alignments by XOR and
 * popcount.  It finds COPIES -- re-uploads, gain changes, trims, offsets of a few frames -- not re-recordings and not
 * copies under heavy noise.
 *
 * This library comes after the nine pinned ones and after cough_amd_slices.h; it has a version of its own.  The
 * conventions are those of cough_amd_slices.h: plain pointers and sizes only, `d_` = device (HBM) pointer; every call
 * returns COUGH_OK (0) or a COUGH_E* code of cough_amd.h and leaves a thread-local message for the last-error call
 * below; launches are stream-ordered on `stream` (a hipStream_t; NULL = default stream); no call allocates or
 * synchronises; every argument the host can check is checked before the first launch.  After one float comparison per
 * bit everything is integers and bits: every result is formed in a fixed place and the same input gives the same bytes.
 * The only atomics are the integer additions into the histogram, whose sums do not depend on their order.
 */
#ifndef COUGH_AMD_DUPS_H
#define COUGH_AMD_DUPS_H

#include <stddef.h>

#include "cough_amd.h"

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden: exactly the entry points declared in this header are exported
 * (tests/test_dups_host.py compares `nm -D` of the built library with this list). */
#pragma GCC visibility push(default)

#define COUGH_DUPS_ABI_VERSION 1
#define COUGH_DUPS_ROWS 33           /* image rows a fingerprint reads: 32 differences, one bit each */
#define COUGH_DUPS_MAX_FRAMES 256    /* the largest Tw */
#define COUGH_DUPS_HIST_BINS 65      /* (err * 64) / bits lies in 0 .. 64 */
#define COUGH_DUPS_MAX_CLIPS 65536   /* the largest n of the matcher; a larger n is refused, never truncated */

int cough_dups_abi_version(void);
const char* cough_dups_last_error(void);  /* thread-local, never NULL */

/* ------------------------------------------------------------------ images -> fingerprints, one workgroup per clip
 * d_images [n][F][T] float32 (row-major), E = one clip's image.  rows[33] (HOST int32) names the image rows r_0 .. r_32,
 * each in [0, F).  With window W >= 1, delta D >= 1 and Tw = T - W + 1 - D (1 <= Tw <= 256), every operation a
 * separately rounded float32 operation (there is no multiply, so nothing contracts into an FMA):
 *   S[k][t] = (((E[r_k][t] + E[r_k][t+1]) + E[r_k][t+2]) + ... + E[r_k][t+W-1])     ascending, k = 0 .. 32
 *   d[k][t] = S[k][t] - S[k+1][t]                                                    k = 0 .. 31
 *   bit k of d_words[clip][t] = (d[k][t+D] - d[k][t]) > 0                            t = 0 .. Tw-1
 *   d_live[clip] = the number of t with d_words[clip][t] != 0
 * A NaN makes its comparison false: an all-NaN image fingerprints as all zeros, like digital silence.  A clip with
 * live == 0 is FLAT.  Outputs: d_words [n][Tw] uint32, d_live [n] int32, every element written.  No atomics.
 * n == 0 launches nothing. */
int cough_fingerprint_images(const float* d_images, int n, int F, int T, const int* rows, int window, int delta,
                             unsigned int* d_words, int* d_live, void* stream);

/* ------------------------------------------------------------------ the matcher
 * Clips a < b and a lag l with |l| <= L.  Frame t of a meets frame t + l of b for max(0, -l) <= t < min(Tw, Tw - l).
 *   a met frame is LIVE when (a[t] | b[t+l]) != 0
 *   bits(l) = 32 * (live frames),   err(l) = sum over met frames of popcount(a[t] ^ b[t+l])
 *   a lag with fewer than min_live (>= 1) live frames does not count
 *   lags are visited in the order 0, -1, +1, -2, +2, ..., -L, +L; a lag replaces the best so far only if
 *   err * bits_best < err_best * bits (strict, integers: ties keep the earlier lag)
 *   the pair MATCHES when a best lag exists and err * 1024 <= max_err_1024 * bits
 * A pair with a flat clip (d_live == 0; d_live is what cough_fingerprint_images wrote, only == 0 is looked at) has no
 * best lag: flat clips match nothing.  No float appears anywhere.
 *
 * The workspace holds one int32 per clip and tile of 64 clips, and one more per clip:
 * cough_match_workspace_bytes(n, Tw) = 4 * 64*ceil(n/64) * (ceil(n/64) + 1) bytes, 256-byte aligned; 0 if n < 1,
 * n > COUGH_DUPS_MAX_CLIPS or Tw outside 1 .. 256. */
size_t cough_match_workspace_bytes(int n, int Tw);

/* d_counts[a] (int32) = the number of matching b > a, summed in a fixed order from per-tile counts that each have a
 * place of their own in the workspace.  d_hist[65] (int64) is zeroed and then hist[(err * 64) / bits] counts the best lag
 * of EVERY pair that has one, matching or not (integer atomics).  The call leaves in the workspace, for every clip a,
 * the number of its matches in front of each tile of b: cough_list_matches reads them.
 *   1 <= n <= COUGH_DUPS_MAX_CLIPS, 1 <= Tw <= 256, L >= 0, 0 <= max_err_1024 <= 1024, min_live >= 1,
 *   workspace_bytes >= cough_match_workspace_bytes(n, Tw).  n == 0 launches nothing. */
int cough_count_matches(const unsigned int* d_words, const int* d_live, int n, int Tw, int L, int max_err_1024,
                        int min_live, int* d_counts, long long* d_hist, void* d_workspace, size_t workspace_bytes,
                        void* stream);

/* The matches sorted by (a, b): d_row_offsets [n + 1] int64 is the exclusive prefix sum of d_counts, formed by the host
 * after its one read of them; the workspace is as cough_count_matches left it for the same words, live and parameters.
 * Row d_row_offsets[a] + j is the j-th smallest matching b of clip a: d_a, d_b, d_lag (the best lag), d_err, d_bits
 * (int32 each).  Every row's place follows from the counts alone: no atomic append, and no row of clip a is written at
 * or past d_row_offsets[a + 1]. */
int cough_list_matches(const unsigned int* d_words, const int* d_live, int n, int Tw, int L, int max_err_1024,
                       int min_live, const void* d_workspace, size_t workspace_bytes, const long long* d_row_offsets,
                       int* d_a, int* d_b, int* d_lag, int* d_err, int* d_bits, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* COUGH_AMD_DUPS_H */
