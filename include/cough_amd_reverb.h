/*
 * cough_amd_reverb.h -- C-ABI of libcough_amd_reverb.so, the companion of libcough_amd.so that puts a clip into a
 * room: every row of a batch is convolved with a room impulse response (RIR) of a bank, by FFT overlap-save inside
 * the LDS of one workgroup.  All other steps of the waveform chain keep a dry clip dry; this is the far-field step.
 *
 * The conventions are those of cough_amd.h: plain pointers and sizes only, `d_` = device (HBM) pointer, `h_` = host
 * pointer; every call returns COUGH_OK (0) or a COUGH_E* code of cough_amd.h and leaves a thread-local message for the
 * last-error call below; launches are stream-ordered on `stream` (a hipStream_t; NULL = default stream); every
 * argument the host can see is checked before anything is launched; no kernel uses atomics, so the same input gives
 * the same bits, and a row alone gives the bits it has inside a batch.  cough_reverb_rows and cough_draw_reverb neither
 * allocate, copy from the host nor synchronise; cough_reverb_prepare, which runs once per bank, copies the twiddle
 * table from the host (one hipMemcpyAsync on `stream`).
 *
 * THE CONVOLUTION.  For a row x of n samples with plan (shift, rir, out_len) and the rir-th response h of L taps:
 *   x_s[i] = x[i - shift] for 0 <= i < n and 0 <= i - shift < n, else 0      (cough_warp_plan's shift rule, fused into
 *            the read; x_s is zero outside [0, n))
 *   y[m]   = sum over k = 0 .. L-1 of h[k] * x_s[m - k],  m = 0 .. out_len-1
 * out_len <= width is the caller's choice: n gives "same length, tail dropped", n + L - 1 the full convolution.
 * Columns out_len .. width-1 of the dense (n_rows, width) output are +0.0.  A row with rir == -1 is not convolved: its
 * first min(n, out_len) columns are x_s, bit for bit, and zeros follow.
 *
 * THE ALGORITHM (what the bound below is derived for).  The output columns are cut into spans of 16384; span w covers
 * m = 16384 w .. 16384 w + 16383 and is the work of one workgroup.  Its two halves of 8192 outputs are overlap-save
 * segments with the same h: segment a = x_s[s - 8192 .. s + 8191] (s = 16384 w) goes into the real parts and segment b,
 * 8192 later, into the imaginary parts of one 16384-point complex float32 sequence z.  Because h is real, the circular
 * convolution of z with h carries a's in its real and b's in its imaginary part, and with L - 1 <= 8192 the positions
 * 8192 .. 16383 are free of wrap-around: their real parts are y[s ..  s + 8191], their imaginary parts
 * y[s + 8192 .. s + 16383].  No real-input split pass exists.  The forward transform is seven radix-4
 * decimation-in-frequency passes, in place, and leaves the spectrum in base-4 digit-reversed order;
 * cough_reverb_prepare stores every H = FFT(h) / 16384 in that order, transformed by the same code; the inverse is
 * seven radix-4 decimation-in-time passes from digit-reversed input with the conjugate twiddles, so no pass reorders.
 * (The last forward pass, the product with H and the first inverse pass touch the same four elements and run in
 * registers.)  The twiddles exp(-2 pi i m / 16384), m = 0 .. 16383, are computed on the host in float64 and rounded
 * once to float32; no device sine or cosine enters.  The compiler may contract a multiply and an add into an fma.
 *
 * RULES.
 *   Non-finite input.  Span w of a row with rir >= 0 is written as NaN in all its columns below out_len if and only
 *            if any of x_s[16384 w - 8192 .. 16384 w + 16383] is a NaN or an Inf: a workgroup-wide OR at load time,
 *            whatever L is.  (An FFT does not turn an Inf into NaN everywhere on its own; this rule does.)  No transform
 *            runs for such a span, and every NaN written is the quiet NaN 0x7FC00000.  Every other span holds, bit for bit, what it holds without that sample.
 *   Silence. A span whose 2 x 16384 inputs are all zero is written as +0.0 (no transform runs).
 *   Determinism.  The same call twice gives the same bits; the bits of a row do not depend on the batch around it.
 *
 * ACCURACY.  Let u = 2^-24, z_w the 2 x 16384 inputs of the span as one complex vector, N = 16384, t = 7 passes.
 * Following Higham, "Accuracy and Stability of Numerical Algorithms", 2nd ed., section 24.1, pass by pass:
 *   - a radix-4 butterfly is two levels of complex additions (each: relative error u per component) behind one complex
 *     multiplication by a stored twiddle (4 real operations, relative error at most sqrt(2) * 2u ~ 3u in modulus, with
 *     or without fma) whose table entry is itself off by at most u / sqrt(2) ~ 0.71 u in modulus.  One pass therefore
 *     multiplies the data by an orthogonal-times-2 matrix up to a relative perturbation of at most
 *     eta = 2u + 3u + 0.71u < 6u in the 2-norm;
 *   - the forward transform, t passes:  || fl(Z) - Z ||_2 <= t eta ||Z||_2 = 42 u ||Z||_2  (first order), with
 *     ||Z||_2 = sqrt(N) ||z_w||_2;
 *   - the stored spectrum went through the same passes on h and one exact scaling by 2^-14:
 *     || fl(H) - H ||_2 <= 42 u ||H||_2.  This is a NORMWISE statement.  Taken rigorously per entry it only gives
 *     | fl(H_j) - H_j | <= 42 u ||H||_2 <= 42 u sqrt(N) max|H|, and the term would be 42 u sqrt(N) ||z_w||_2 ||h||_2, up to
 *     sqrt(N) = 128 times larger than what follows for an impulse-like h.  The bound below instead ASSUMES that the
 *     spectrum's error is spread over its N entries as rounding errors are (no entry off by more than 42 u max|H|,
 *     max|H| <= ||h||_1 / N), so that it enters the product as a relative error of 42 u; that assumption is statistical,
 *     not proved, and the tests measure against it (profiles/reverb_precision.txt: every row below 1 % of the bound,
 *     the impulse responses included);
 *   - the product, one complex multiplication: 3u;
 *   - the inverse transform, t passes: 42 u.
 * The circular result c = IFFT(Z * H) satisfies ||c||_2 <= ||z_w||_2 * N max|H| <= ||z_w||_2 ||h||_1, and the errors
 * above add to (42 + 42 + 3 + 42) u = 129 u relative to that in the 2-norm.  An error at one position is at most the
 * 2-norm of the whole error vector, so with K = 129 rounded up to
 *
 *   | y[m] - y_ref[m] |  <=  COUGH_REVERB_BOUND_K * 2^-24 * ||z_w||_2 * ||h||_1,     COUGH_REVERB_BOUND_K = 160
 *
 * where y_ref is the float64 convolution of the float32 inputs.  K is thus 129 from a first-order normwise argument
 * (with the one statistical step named above) plus a margin for the second-order terms and the final rounding of y
 * itself, which is below u |y| <= u ||z_w||_2 ||h||_1; it is a contract that the tests hold the kernel to, not a
 * theorem about every conceivable h.  The bound is a worst case over the
 * whole span and is loose by orders of magnitude for noise-like input (the errors behave like sqrt(t), spread over N
 * positions).  It is NOT relative to y[m]: an error anywhere in the span can land anywhere in it, so the outputs ahead
 * of a burst's onset, where y_ref is exactly zero, are rounding noise of that size and not exact zeros.
 *
 * THE REVERB DRAW CONTRACT, in the conventions of cough_amd_draws.h and with the coin rule of cough_amd_pitch.h:
 * Philox4x32-10, key = seed (low word, high word); a 32-bit word x gives u = (x + 0.5) * 2^-32 in float64; a coin with
 * probability p fires iff u <= p; conversions to int truncate toward zero.
 *   counter (0, row, 0, 4)   reverb coin x;  rir = (int)((double)n_rirs * u_y) when it fires, else -1
 * The shift counts (0, row, 0, 1), the speed (0, row, 0, 2), the pitch (0, row, 0, 3), the other draws (slot, row, 0, 1)
 * and the gaussian noise (group, row, 0, 0), so the streams never meet.
 */
#ifndef COUGH_AMD_REVERB_H
#define COUGH_AMD_REVERB_H

#include <stddef.h>

#include "cough_amd.h"

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden: exactly the entry points declared in this header are exported
 * (tests/test_reverb_host.py compares `nm -D` of the built library with this list). */
#pragma GCC visibility push(default)

#define COUGH_REVERB_ABI_VERSION 1
#define COUGH_REVERB_FFT 16384          /* the transform's length, and the outputs of one span */
#define COUGH_REVERB_MAX_TAPS 8193      /* L - 1 <= 8192: half a second at 16 kHz */
#define COUGH_REVERB_MAX_LENGTH (1 << 30)   /* a row's length is clamped to 0 .. 2^30; width <= 2^30 */
#define COUGH_REVERB_BOUND_K 160        /* ACCURACY above */

int cough_reverb_abi_version(void);
const char* cough_reverb_last_error(void);  /* thread-local, never NULL */

/* One row's plan.  16 bytes, four int32. */
typedef struct cough_reverb_plan {
    int shift;     /* time_shift samples: > 0 right (zeros on the left), < 0 left */
    int rir;       /* the response of the bank, 0 .. n_rirs-1; -1: the row is copied */
    int out_len;   /* y has out_len samples, 0 <= out_len <= width */
    int reserved;  /* written as 0, not read */
} cough_reverb_plan;

/* ------------------------------------------------------------------ the prepared bank
 * The device workspace of a bank of n_rirs responses: the twiddle table (16384 complex float32) followed by one
 * digit-reversed, pre-scaled spectrum of 16384 complex float32 per response -- 131072 * (n_rirs + 1) bytes.  0 for
 * n_rirs < 0 or a size that does not fit. */
size_t cough_reverb_bank_bytes(int n_rirs);

/* Transforms the bank once.  d_taps: the responses' float32 taps, packed; response r is the h_lengths[r] taps at
 * d_taps + h_offsets[r] (element offsets).  h_offsets and h_lengths are HOST arrays of n_rirs entries: the lengths are
 * checked here, 1 <= L <= COUGH_REVERB_MAX_TAPS (a longer response is refused with COUGH_EUNSUPPORTED, nothing is
 * launched), 0 <= offset.  d_workspace: 256-byte aligned, workspace_bytes >= cough_reverb_bank_bytes(n_rirs)
 * (COUGH_EWORKSPACE otherwise); every byte of it that a later call reads is written here, whatever it held.  One
 * launch per response.  A tap that is not finite gives a spectrum of NaNs: every span convolved with that response
 * comes out as NaN.  n_rirs == 0 writes the table only. */
int cough_reverb_prepare(const float* d_taps, const long long* h_offsets, const int* h_lengths, int n_rirs,
                         void* d_workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ per-row convolution, one launch per batch
 * Row b is the d_lengths[b] samples at d_src + d_row_offsets[b] (int64 element offsets), read in place -- a row may
 * start at any element of a packed buffer -- and its plan is d_plans[b].  d_out: [n_rows][width] float32, every
 * element of which is written.  d_workspace: what cough_reverb_prepare left for a bank of n_rirs responses.  d_out must
 * not overlap d_src.
 *
 * The host cannot check arrays that live on the device (a caller that holds its plans on the host checks them there:
 * rir >= n_rirs, rir < -1, out_len < 0 and out_len > width are refused before anything is launched by the Python
 * front's plan_array), so the kernel makes an entry it cannot use harmless:
 *   rir outside -1 .. n_rirs-1        the row is copied, as for rir == -1
 *   out_len outside 0 .. width        is clamped to that range
 *   a length outside 0 .. 2^30        is clamped to that range
 *   shift                             any value (|shift| >= n: a silent row)
 * Nothing is read outside the rows and the workspace, and nothing written outside d_out, whatever the device arrays
 * hold; the caller answers for d_row_offsets[b] + d_lengths[b] lying inside d_src.
 *   1 <= width <= 2^30;  n_rirs >= 0;  n_rows * ceil(width / 16384) <= 2^24 (the grid);  n_rows == 0 launches nothing. */
int cough_reverb_rows(const float* d_src, const long long* d_row_offsets, const int* d_lengths, int n_rows,
                      const cough_reverb_plan* d_plans, const void* d_workspace, int n_rirs, float* d_out, int width,
                      void* stream);

/* ------------------------------------------------------------------ the reverb draws of one batch
 * One thread per row writes the row's plan by the contract above: (0, rir or -1, n, 0) with n = d_lengths[row] clamped
 * to 0 .. 2^30 -- the step keeps the row's length.  A row with n < 1, and every row when n_rirs == 0, gets rir = -1.
 *   p_augment in [0, 1];  n_rirs >= 0.  n_rows == 0 launches nothing. */
int cough_draw_reverb(unsigned long long seed, int n_rows, const int* d_lengths, double p_augment, int n_rirs,
                      cough_reverb_plan* d_plans_out, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* COUGH_AMD_REVERB_H */
