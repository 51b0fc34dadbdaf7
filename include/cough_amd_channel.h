/*
 * cough_amd_channel.h -- C-ABI of libcough_amd_channel.so, the companion of libcough_amd.so that puts a clip through
 * the device that records it: a microphone response (a short cascade of second-order IIR sections out of a prepared
 * bank) and the converter's ceiling (a hard clip relative to the row's own peak).  It is the last link of the waveform
 * chain: it runs on the matrix the augmentation kernel wrote, because a microphone hears the room and the noise.
 *
 * The conventions are those of cough_amd.h: plain pointers and sizes only, `d_` = device (HBM) pointer, `h_` = host
 * pointer; every call returns COUGH_OK (0) or a COUGH_E* code of cough_amd.h and leaves a thread-local message for the
 * last-error call below; launches are stream-ordered on `stream` (a hipStream_t; NULL = default stream); every
 * argument the host can see is checked before anything is launched; no kernel uses atomics, so the same input gives
 * the same bits, and a row alone gives the bits it has inside a batch.  cough_channel_rows and cough_draw_channel
 * neither allocate, copy from the host nor synchronise; cough_channel_prepare, which runs once per bank, is host code:
 * it computes the bank's blob, copies it (one hipMemcpyAsync on `stream`) and waits for that copy.
 *
 * THE FILTER.  A bank entry is a cascade of 1 .. COUGH_CHANNEL_MAX_SECTIONS second-order sections, all in float64.
 * Section j with coefficients (b0, b1, b2, a1, a2) -- a0 = 1 after cough_channel_prepare divided by it -- is direct
 * form II transposed with zero initial state, the recurrence of scipy.signal.sosfilt:
 *     y  = b0*x + z1
 *     z1 = b1*x - a1*y + z2
 *     z2 = b2*x - a2*y
 * Section j+1 reads section j's output; section 0 reads the row's float32 samples converted to float64; the last
 * section's output is rounded once to float32.  The compiler may contract a multiply and an add into an fma.
 *
 * THE ALGORITHM (what the tests' bound is measured for).  The recurrence is serial in the sample index, so a workgroup
 * of T = COUGH_CHANNEL_THREADS threads runs it block-parallel.  The row is cut into spans of T chunks of
 * C = COUGH_CHANNEL_CHUNK consecutive samples (a span is T*C = 16384 samples); thread t owns chunk t.  The state
 * z = (z1, z2) obeys z' = A z + B x with A = [[-a1, 1], [-a2, 0]], so over one chunk z_end = M z_start + e with
 * M = A^C and e the end state reached from zero state.  Per span and per section:
 *   1. thread t runs the recurrence over its chunk from zero state and keeps e[t];
 *   2. thread 0 adds M s_in to e[0], s_in being the carry of the previous span (zero for the first);
 *   3. the carries s[t] = M s[t-1] + e[t] come from a log-step scan: for j = 0 .. 7, d = 2^j, every t >= d replaces
 *      s[t] by (M^d) s[t-d] + s[t], all t at once; a 2-vector product is (m00*p0 + m01*p1) + s0, (m10*p0 + m11*p1) + s1;
 *   4. thread t runs its chunk again from s[t-1] (thread 0 from s_in) and keeps the outputs: inside a chunk the
 *      arithmetic is the sequential filter's own, only the 2-vector start state carries the scan's rounding;
 *   5. s[T-1] is the next span's s_in.
 * A span is read whole before any of it is written.  The span lives in LDS as float64.
 *
 * THE CEILING.  While a row's float32 samples are written the workgroup takes their peak p = max |y32| (exact, whatever
 * the order).  A row whose plan has 0 <= clip_ratio < 1 is then rewritten as
 *     c = clip_ratio * p  (one float32 product);   y > c ? c : (y < -c ? -c : y)
 * which is min(max(y, -c), c) with the sign of a zero kept.  clip_ratio >= 1, negative or NaN: no clip.  A hard clip
 * only: no soft saturation, no gain control, no codec.
 *
 * RULES.
 *   The row.  Row b is its first m = min(n, width) samples, n = d_lengths[b] clamped to 0 .. 2^30.  Columns m .. width-1
 *            of the output are +0.0.  The step keeps the length and shifts nothing.
 *   Copy.    A row with no filter (filter == -1, or a filter the bank does not have) and no clip is copied bit for bit,
 *            NaNs, Infs and negative zeros included.
 *   Non-finite input.  Every other row that holds a NaN or an Inf among its m samples comes out as the quiet NaN
 *            0x7FC00000 in all m (the recurrence alone would only poison what follows the sample).
 *   Silence. Every other row whose m samples are all zero comes out as +0.0.
 *   Determinism.  The same call twice gives the same bits; the bits of a row do not depend on the batch around it.
 *
 * THE BANK'S BLOB, word by word (8-byte words, little endian).  Entry r is the COUGH_CHANNEL_ENTRY_WORDS = 160 words
 * at word 160 r: four section records of 40 words each, section j at word 40 j of the entry:
 *     0 .. 4    b0, b1, b2, a1, a2  as float64, already divided by a0
 *     5         in section 0: the entry's number of sections as float64 (1.0 .. 4.0); in the others 0.0
 *     6, 7      0.0
 *     8 + 4 j .. 11 + 4 j,  j = 0 .. 7:   M^(2^j) as m00, m01, m10, m11
 * Records of sections the entry does not have are all 0.0.  The powers are computed in float64, one IEEE operation per
 * operator and no fma, by repeated squaring P <- P * P with
 *     (X*Y)00 = x00*y00 + x01*y10    (X*Y)01 = x00*y01 + x01*y11
 *     (X*Y)10 = x10*y00 + x11*y10    (X*Y)11 = x10*y01 + x11*y11
 * starting from A: six squarings give M = A^64, seven more M^2 .. M^128.  The device recomputes none of it.
 *
 * THE CHANNEL DRAW CONTRACT, in the conventions of cough_amd_draws.h and with the coin rule of cough_amd_pitch.h:
 * Philox4x32-10, key = seed (low word, high word); a 32-bit word x gives u = (x + 0.5) * 2^-32 in float64; a coin with
 * probability p fires iff u <= p; conversions to int truncate toward zero.
 *   counter (0, row, 0, 5)   x: the step's coin against p_augment.  When it fires:
 *                            y: filter = (int)((double)n_bank * u_y)  (-1 when n_bank == 0)
 *                            z: the clip coin against p_clip;  w: clip_ratio = (float)(clip_lo + (clip_hi - clip_lo) * u_w)
 *                            when the clip coin fires, else 1.0f
 *                            A row whose step coin does not fire gets (-1, 1.0f).
 * The shift counts (0, row, 0, 1), the speed (0, row, 0, 2), the pitch (0, row, 0, 3), the reverb (0, row, 0, 4), the
 * other draws (slot, row, 0, 1) and the gaussian noise (group, row, 0, 0), so the streams never meet.
 */
#ifndef COUGH_AMD_CHANNEL_H
#define COUGH_AMD_CHANNEL_H

#include <stddef.h>

#include "cough_amd.h"

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden: exactly the entry points declared in this header are exported. */
#pragma GCC visibility push(default)

#define COUGH_CHANNEL_ABI_VERSION 1
#define COUGH_CHANNEL_MAX_SECTIONS 4
#define COUGH_CHANNEL_CHUNK 64              /* C: consecutive samples of one thread */
#define COUGH_CHANNEL_THREADS 256           /* T: chunks of one span, threads of one workgroup */
#define COUGH_CHANNEL_ENTRY_WORDS 160       /* 8-byte words of one bank entry */
#define COUGH_CHANNEL_MAX_LENGTH (1 << 30)  /* a row's length is clamped to 0 .. 2^30; width <= 2^30 */

int cough_channel_abi_version(void);
const char* cough_channel_last_error(void);  /* thread-local, never NULL */

/* One row's plan.  8 bytes. */
typedef struct cough_channel_plan {
    int filter;        /* the entry of the bank, 0 .. n_bank-1; -1: no filter */
    float clip_ratio;  /* 0 <= r < 1: clip at r times the row's peak; anything else: no clip */
} cough_channel_plan;

/* ------------------------------------------------------------------ the prepared bank
 * The device blob of a bank of n_bank entries: 1280 * max(n_bank, 1) bytes.  0 for n_bank < 0 or a size that does
 * not fit. */
size_t cough_channel_bank_bytes(int n_bank);

/* Host code.  h_sos: the sections of all entries, packed, one scipy-layout row (b0, b1, b2, a0, a1, a2) of float64
 * each; entry r has h_n_sections[r] rows, behind those of entry r-1.  Every coefficient is divided by its row's a0.
 * Refused with COUGH_EINVAL before anything is copied: a coefficient that is not finite, a0 == 0, an entry with fewer
 * than 1 or more than COUGH_CHANNEL_MAX_SECTIONS sections, and a section outside the stability triangle
 * |a2| < 1, |a1| < 1 + a2 (after the division).  d_bank: 256-byte aligned, bank_bytes >= cough_channel_bank_bytes(n_bank)
 * (COUGH_EWORKSPACE otherwise); every byte of it that a later call reads is written here, whatever it held.  The call
 * returns after the copy has completed.  n_bank == 0 copies nothing. */
int cough_channel_prepare(const double* h_sos, const int* h_n_sections, int n_bank, void* d_bank, size_t bank_bytes,
                          void* stream);

/* ------------------------------------------------------------------ filter and clip, one launch per batch
 * Row b is the d_lengths[b] samples at d_src + d_row_offsets[b] (int64 element offsets), read in place -- a row may
 * start at any element of a packed buffer -- and its plan is d_plans[b].  d_out: [n_rows][width] float32, every
 * element of which is written.  d_bank: what cough_channel_prepare left for a bank of n_bank entries (not read, and may
 * be NULL, when n_bank == 0).  d_out may BE the input -- d_out == d_src with d_row_offsets[b] == b * width -- and must
 * not overlap it in any other way.
 *
 * The host cannot check arrays that live on the device (a caller that holds its plans on the host checks them there,
 * as the Python front's plan_array does), so the kernel makes an entry it cannot use harmless:
 *   filter outside 0 .. n_bank-1      no filter, as for -1
 *   a length outside 0 .. 2^30        is clamped to that range
 * Nothing is read outside the rows and the bank, and nothing written outside d_out, whatever the device arrays hold;
 * the caller answers for d_row_offsets[b] + d_lengths[b] lying inside d_src.
 *   1 <= width <= 2^30;  n_bank >= 0;  n_rows <= 2^24 (the grid);  n_rows == 0 launches nothing. */
int cough_channel_rows(const float* d_src, const long long* d_row_offsets, const int* d_lengths, int n_rows,
                       const cough_channel_plan* d_plans, const void* d_bank, int n_bank, float* d_out, int width,
                       void* stream);

/* ------------------------------------------------------------------ the channel draws of one batch
 * One thread per row writes the row's plan by the contract above.
 *   p_augment, p_clip in [0, 1];  clip_lo <= clip_hi, both finite;  n_bank >= 0.  n_rows == 0 launches nothing. */
int cough_draw_channel(unsigned long long seed, int n_rows, double p_augment, int n_bank, double p_clip, double clip_lo,
                       double clip_hi, cough_channel_plan* d_plans_out, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* COUGH_AMD_CHANNEL_H */
