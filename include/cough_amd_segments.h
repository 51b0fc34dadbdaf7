/*
 * cough_amd_segments.h -- C-ABI of libcough_amd_segments.so, the companion of libcough_amd.so for corpus curation: find
 * the cough-length segments of long recordings that sit on a short-time-energy peak, and copy them into a packed clip
 * bank of their own (the step the reference leaves as a stub: find_energy_peaks / extract_segments).
 *
 * cough_amd.h is pinned at ABI v5 with its 53 entry points, cough_amd_loop.h and cough_amd_data.h at version 1, so what
 * curation needs on the device is exported from a fourth library with a version of its own.  The conventions are those
 * of cough_amd.h: plain pointers and sizes only, `d_` = device (HBM) pointer; every call returns COUGH_OK (0) or a
 * COUGH_E* code of cough_amd.h and leaves a thread-local message for the last-error call below; launches are
 * stream-ordered on `stream` (a hipStream_t; NULL = default stream); no call allocates or synchronises; every argument
 * is checked before the launch; no kernel uses atomics and every sum is formed in a fixed order, so the same input gives
 * the same bits.
 *
 * What lives in device memory (offsets, lengths, tiles, starts) cannot be checked by the host before the launch: the
 * kernels skip a tile that names no frame of its clip and clamp a negative start or length to 0; the caller answers for
 * the rows read lying inside d_bank and the rows written lying inside the output.
 *
 * The clips of a packed bank: clip k is d_bank[d_clip_offsets[k] .. d_clip_offsets[k] + d_lengths[k]), offsets int64 in
 * elements (a clip starts at any element: 4-byte alignment only), lengths int32 >= 1.
 * Frames of a clip of n samples: n_frames = 1 if n < frame_length, else 1 + (n - frame_length) / hop_length; frame f
 * covers [f*hop_length, min(f*hop_length + frame_length, n)).  Its energy is the sum of double(x)^2 over the frame
 * divided by its sample count.  d_frame_offsets [n_clips + 1] int64: clip k's energies are
 * d_energy[d_frame_offsets[k] .. d_frame_offsets[k + 1]).
 */
#ifndef COUGH_AMD_SEGMENTS_H
#define COUGH_AMD_SEGMENTS_H

#include "cough_amd.h"

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden: exactly the entry points declared in this header are exported
 * (tests/test_segments_host.py compares `nm -D` of the built library with this list). */
#pragma GCC visibility push(default)

#define COUGH_SEGMENTS_ABI_VERSION 1
#define COUGH_MAX_SEGMENTS 16          /* segments per clip at most */
#define COUGH_MAX_FRAME_LENGTH 4096    /* a frame's sub-block sums and samples stay in one workgroup's LDS */

int cough_segments_abi_version(void);
const char* cough_segments_last_error(void);  /* thread-local, never NULL */

/* ------------------------------------------------------------------ short-time energy of every frame of every clip
 * One workgroup takes a tile of consecutive frames of one clip: it brings the tile's samples from HBM into LDS once,
 * sums double(x)^2 over sub-blocks of gcd(frame_length, hop_length) samples (sample order), and forms each frame from
 * its frame_length / gcd consecutive sub-block sums (sub-block order).
 *   cough_frame_energy_tile_frames: the frames of a tile for this frame / hop pair (>= 1), or 0 when the pair is not
 *     accepted (either < 1, or frame_length > COUGH_MAX_FRAME_LENGTH).
 *   d_tiles [n_tiles][2] int32: (clip, first frame).  Tile t holds the frames first .. first + tile_frames - 1 of its
 *     clip that exist; the caller lists, clip by clip, first = 0, tile_frames, 2 * tile_frames, ...  A tile whose clip
 *     lies outside 0 .. n_clips - 1 or whose first frame does not exist writes nothing.
 * hop_length > frame_length (gaps between frames) is legal.  n_clips == 0 or n_tiles == 0 launches nothing. */
int cough_frame_energy_tile_frames(int frame_length, int hop_length);
int cough_frame_energy(const float* d_bank, const long long* d_clip_offsets, const int* d_lengths,
                       const long long* d_frame_offsets, int n_clips, const int* d_tiles, int n_tiles, int frame_length,
                       int hop_length, double* d_energy, void* stream);

/* ------------------------------------------------------------------ energies -> segments, one wave per clip
 * For clip k with energies e[0 .. F):
 *   gate      any e[f] not finite, or E_max = max e[f] < floor: no segment.
 *   activity  active[f] = e[f] >= E_max * ratio (one double product).
 *   runs      maximal stretches of consecutive active frames, kept when at least min_frames long.
 *   segments  the kept runs in time order; p = the first frame of the run with the largest e; c = p*hop_length +
 *             frame_length/2; length = min(seg_len, n); start = min(max(c - seg_len/2, 0), max(n - seg_len, 0)); a run
 *             whose start lies before the end (start + length) of the clip's last emitted segment is dropped; at most
 *             max_segments are emitted.
 * Outputs: d_counts [n_clips] int32; d_starts, d_seg_lengths (int32) and d_peak_db (float32 = 10*log10(e[p]) rounded
 * once) [n_clips][max_segments], the slots past a clip's count zeroed.
 *   1 <= max_segments <= COUGH_MAX_SEGMENTS; seg_len >= 1; min_frames >= 1; ratio and floor finite, >= 0.
 * n_clips == 0 launches nothing. */
int cough_pick_segments(const double* d_energy, const long long* d_frame_offsets, const int* d_lengths, int n_clips,
                        int frame_length, int hop_length, int seg_len, int min_frames, int max_segments, double ratio,
                        double floor, int* d_counts, int* d_starts, int* d_seg_lengths, float* d_peak_db, void* stream);

/* ------------------------------------------------------------------ ragged rows -> packed rows
 * Row r of the output, d_dst[d_dst_offsets[r] .. + d_row_lengths[r]), receives
 * d_src[d_src_offsets[r] + d_starts[r] .. + d_row_lengths[r]).  Offsets int64 in elements, starts and lengths int32 (a
 * negative one counts as 0); max_len >= the longest row (it sizes the grid; a longer row is still copied whole).
 * d_dst must not overlap the rows read.  n_rows == 0 launches nothing. */
int cough_copy_segments(const float* d_src, const long long* d_src_offsets, const int* d_starts, const int* d_row_lengths,
                        const long long* d_dst_offsets, int n_rows, int max_len, float* d_dst, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* COUGH_AMD_SEGMENTS_H */
