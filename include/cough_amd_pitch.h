/*
 * cough_amd_pitch.h -- C-ABI of libcough_amd_pitch.so, the companion of libcough_amd.so that runs the first half of the
 * waveform chain's pitch shift on the device: a phase vocoder that stretches every row of a batch in time by a rate of
 * its own and keeps its pitch.  The second half, the resampling back to the row's length, is cough_warp_rows of
 * cough_amd_warp.h: a pitch shift by n_steps semitones is `stretch by rate = 2^(-n_steps / 12)` followed by `resample
 * from int(sample_rate / rate) to sample_rate` (torchaudio.functional.pitch_shift), and pairs such as 16951 -> 16000
 * have no common factor, which is what the tableless resampler was written for.
 *
 * cough_amd.h is pinned at ABI v5 with its 53 entry points and the seven other companions at version 1 with theirs, so
 * these entry points are exported from a ninth library with a version of its own.  The conventions are those of
 * cough_amd.h: plain pointers and sizes only, `d_` = device (HBM) pointer; every call returns COUGH_OK (0) or a COUGH_E*
 * code of cough_amd.h and leaves a thread-local message for the last-error call below; launches are stream-ordered on
 * `stream` (a hipStream_t; NULL = default stream); no call allocates, copies from the host or synchronises; every
 * argument is checked before the launch; no kernel uses atomics, so the same input gives the same bits.
 *
 * THE STRETCH'S ARITHMETIC.  It restates torchaudio's phase_vocoder followed by istft, as functional.pitch_shift calls
 * them (n_fft 512, hop 128, a periodic Hann window, centred frames with reflect padding), from memory: torchaudio is
 * not a dependency of this project and was not at hand when this was written, so THIS HEADER IS THE CONTRACT, and
 * tests/pitch_ref.py restates it in numpy.  Two things differ from torchaudio on purpose.  Everything is float64 and
 * there is a magnitude floor: a vocoder sums per-bin phase differences over time, for a rate other than 1 the sum does
 * not telescope, and the phase of a bin in a silent frame -- FFT rounding noise of arbitrary phase -- then enters every
 * later output frame of that bin.  Without a floor the output after digital silence (which pad_or_trim and time_shift
 * produce all the time) moves by more than its own peak when the spectrum changes in its last bit, so it is not a
 * function of the input that two implementations can agree on; in float32 it is off by as much again.
 * For a row x of n samples with plan (shift, rate); all of it float64, one IEEE operation per operator (no fused
 * multiply-add), the result rounded ONCE to float32:
 *   x_s[i] = x[i - shift] for 0 <= i - shift < n, else 0, i = 0 .. n-1      (the time shift, fused into the read, as
 *            in cough_warp_rows);  peak = max |x_s[i]|
 *   w[j]   = 0.5 - 0.5 cos(2 pi j / 512), j = 0 .. 511
 *   T      = 1 + n / 128 (integer division) frames;  frame t, sample j is w[j] * x_r[128 t - 256 + j], where x_r
 *            reflects about both ends: x_r[i] = x_s[-i] for i < 0 and x_s[2 (n - 1) - i] for i >= n
 *   S[t][k], k = 0 .. 256: the one-sided DFT of frame t, sum_j frame[j] exp(-2 pi i j k / 512);  frames T and T + 1
 *            are zero
 *   floor  = 2^-24 * 256 * peak;  u(S) = (1, 0) when |S| <= floor -- the phase torch.angle gives 0 -- else S / |S|
 *   T_out  = ceil(T / rate)
 *   for t = 0 .. T_out-1:  ts = (double)t * rate, i0 = floor(ts), a = ts - i0
 *            mag  = a |S[i0+1][k]| + (1 - a) |S[i0][k]|
 *            Y[t][k] = mag * P[t][k],  P[0] = u(S[0]),  P[t+1] = P[t] * u(S[i0+1]) * conj(u(S[i0]))
 *            (the phase-advance term 2 pi k hop / n_fft that torchaudio subtracts, wraps and adds back cancels exactly
 *            modulo 2 pi, so no atan2 is needed; the kernel may keep P as a renormalised product of unit phasors or as
 *            an angle)
 *   frame'[t][j] = w[j] * (1 / 512) sum over the Hermitian extension of Y[t] (the imaginary parts of bins 0 and 256
 *            do not enter), overlap-added at 128 t + j and divided by env[m] = sum_t w[m - 128 t]^2
 *   n_s    = (int)rint((double)n / rate), round half to even;  y[m] = (overlap-add / env)[256 + m], m = 0 .. n_s-1,
 *            and 0 where the overlap-add ends first
 * env stays at or above 1/4 over the kept range, so torch's guard (it refuses an envelope below 1e-11) never matters:
 * a kept sample m lies in 256 .. 255 + n_s, and n_s <= 128 T_out because n / rate < 128 T / rate <= 128 T_out.  Frame
 * 0 covers m < 512 with w^2 >= 1/4 on 256 .. 384; from 384 on up to 128 T_out - 1 all four overlapping frames exist
 * or, at the end, the last frame covers m at j = m - 128 (T_out - 1) <= 383 with the frame before it at j + 128:
 * with theta = 2 pi j / 512 in [pi / 2, 3 pi / 2) their squares sum to (1 - cos theta)^2 / 4 + (1 + sin theta)^2 / 4,
 * which is least, 1/4, at the open end.  The overlap-add, 128 T_out + 384 samples, never ends before 256 + n_s.
 * Rows the kernel does not stretch are copies of x_s, bit for bit, with n_s = n:
 *   rate == 1;  rate outside [1/2, 2] or not finite;  n < 257 (the reflect padding needs 257 samples)
 * A row whose x_s holds a NaN or an Inf comes out as n_s NaNs: the featuriser's rule for such a clip (torch would
 * poison only the frames that overlap the sample, and through P every later frame of those bins).  A row with
 * peak == 0 comes out as n_s exact zeros.
 * An implementation meets the contract when every sample satisfies |y - y_ref| <= 2^-24 |y_ref| + E[m] with the
 * first-order bound E of tests/pitch_ref.py, which allows the spectrum an error of 16 * 2^-53 * 256 * peak per bin.
 *
 * THE LOCKED STRETCH'S ARITHMETIC (a plan whose mode word has bit 0 set: identity phase locking, Laroche & Dolson 1999).
 * A plain vocoder advances every bin's phase on its own, so the bins of a sinusoid's main lobe drift apart and the
 * sinusoid loses level (a steady 440 Hz tone shifted up two semitones comes back at 0.6 of its level).  Here only the
 * spectral peaks carry a phase forward; the bins around a peak keep the phase relation they had to it in the analysis
 * frame.  Everything not named below is exactly as in the plain stretch: float64 without contraction, the floor, u(),
 * mag, T, T_out, i0, a, the inverse transform, the overlap-add, the envelope, n_s, the rows that are copied, the NaN /
 * Inf rows and the silent rows.  Write f = i0(t) and M[k] = |S[f][k]|.
 *   peaks of input frame f < T: bin k is a peak when M[k] > floor and M[k] > M[j] for every j in {k-2, k-1, k+1, k+2}
 *            with 0 <= j <= 256 (there is no Hermitian mirror);  the zero frames T and T + 1 have no peaks
 *   own[f][k] = k when frame f has no peak;  else the peak p that minimises |k - p|, the lower p on a tie (a peak owns
 *            itself)
 *   R[0] = u(S[0]);  for t = 0 .. T_out-1, with p = own[f][k]:
 *            Q[t][k]   = R[t][k] when p == k, else R[t][p] * u(S[f][k]) * conj(u(S[f][p]))
 *            Y[t][k]   = mag[t][k] * Q[t][k]
 *            R[t+1][k] = Q[t][k] * u(S[f+1][k]) * conj(u(S[f][k]))
 *            (the kernel may renormalise any product of unit phasors)
 * With mode 0, Q = R = P.  In both modes frame 0 is u(S[0]).  While i0(t) == t the two modes coincide, because
 * R[t] = u(S[t]) telescopes and Q[t][k] = u(S[t][p]) u(S[t][k]) conj(u(S[t][p])): that covers the first frames of any row
 * and all of a short row at rate 2^(1/12).
 * The contract is the plain one, |y - y_ref| <= 2^-24 |y_ref| + E_lock[m], with the first-order bound E_lock of
 * tests/pitch_lock_ref.py: delta and the per-bin phasor uncertainty eu (delta / |S| above the floor, 0 at or below it)
 * as for E, and  eR[0] = eu[0];  eQ[k] = eR[k] for a bin that owns itself, else eR[p] + eu[f][k] + eu[f][p];
 * eY = mag * eQ + delta;  eR' = eQ + eu[f+1] + eu[f];  then through the inverse transform, the window, the overlap-add
 * and the envelope as E is.  Two implementations must also pick the same peaks: for every frame f < T and every bin with
 * M[k] > floor let m_k = min(M[k] - floor, min over the existing neighbours j of (M[k] - M[j]) / 2); m_k > 0 exactly when
 * k is a peak, and |m_k| is what a perturbation must overcome to flip the decision.  A row is fit for a comparison only
 * when its peak margin, min |m_k| / delta, is at least 64, like its floor margin.
 *
 * THE PITCH DRAW CONTRACT, in the conventions of cough_amd_draws.h: Philox4x32-10, key = seed (low word, high word); a
 * 32-bit word x gives u = (x + 0.5) * 2^-32 in float64; a coin with probability p fires iff u <= p; all arithmetic is
 * float64, one IEEE operation per operator, conversions to int truncate toward zero.
 *   counter (0, row, 0, 3)   pitch coin x;  n_steps = lo + (int)((double)(hi - lo + 1) * u_y)      (random.randint)
 * The shift counts (0, row, 0, 1) and the speed (0, row, 0, 2) (cough_amd_warp.h), the other draws (slot, row, 0, 1)
 * and the gaussian noise (group, row, 0, 0), so the streams never meet.  The rate 2^(-n_steps / 12) and the resampler's
 * orig = (int)(sample_rate / rate) come from a table the host computes, so that no device pow enters the contract.
 */
#ifndef COUGH_AMD_PITCH_H
#define COUGH_AMD_PITCH_H

#include "cough_amd.h"
#include "cough_amd_warp.h"

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden: exactly the entry points declared in this header are exported
 * (tests/test_pitch_host.py compares `nm -D` of the built library with this list). */
#pragma GCC visibility push(default)

#define COUGH_PITCH_ABI_VERSION 1
#define COUGH_PITCH_N_FFT 512
#define COUGH_PITCH_HOP 128
#define COUGH_PITCH_MAX_LENGTH (1 << 20)    /* a row's length is clamped to 0 .. 2^20 */
#define COUGH_PITCH_MAX_SAMPLES (1 << 21)   /* n_s <= 2^21 at rate 1/2 */
#define COUGH_PITCH_MAX_STEPS 12            /* -12 <= n_steps <= 12: 1/2 <= rate <= 2 */

int cough_pitch_abi_version(void);
const char* cough_pitch_last_error(void);  /* thread-local, never NULL */

/* The mode word of a plan or a table entry (the field `reserved`, which every version 1 caller wrote as 0): bit 0 set
 * means identity phase locking, THE LOCKED STRETCH'S ARITHMETIC above; mode 0 is the plain stretch, unchanged.  All other
 * bits are ignored -- the host never sees device plans, so a word the kernel does not know must be harmless. */
#define COUGH_STRETCH_PHASE_LOCK 1

/* One row's plan.  16 bytes. */
typedef struct cough_stretch_plan {
    int shift;     /* time_shift samples: > 0 right (zeros on the left), < 0 left */
    int reserved;  /* the mode: COUGH_STRETCH_PHASE_LOCK or 0; only bit 0 is read */
    double rate;   /* the row becomes n_s = rint(n / rate) samples long: > 1 shorter, < 1 longer */
} cough_stretch_plan;

/* One entry of the draw's table, for one number of semitones.  16 bytes. */
typedef struct cough_pitch_step {
    double rate;   /* 2^(-n_steps / 12) */
    int orig;      /* (int)(sample_rate / rate): the rate the stretched row is taken to have */
    int reserved;  /* the mode a row that draws this entry gets: COUGH_STRETCH_PHASE_LOCK or 0; only bit 0 is read */
} cough_pitch_step;

/* ------------------------------------------------------------------ per-row time stretch
 * Row b is the d_lengths[b] samples at d_src + d_row_offsets[b] (int64 element offsets), read in place -- a row may
 * start at any element of a packed buffer -- and its plan is d_plans[b].  d_out: [n_rows][n_samples] float32; row b
 * receives its min(n_s, n_samples) stretched samples and zeros behind them.  d_new_lengths: NULL, or [n_rows] int32 that
 * receives min(n_s, n_samples).  d_out must not overlap d_src.
 *
 * The host cannot check arrays that live on the device, so the kernel makes an entry it cannot use harmless:
 *   a rate outside [1/2, 2] or not finite     the row is copied, as for rate == 1
 *   a length outside 0 .. 2^20                is clamped to that range
 *   shift                                     any value (|shift| >= n: a silent row)
 * Nothing is read outside the rows, and nothing written outside d_out and d_new_lengths, whatever the device arrays
 * hold; the caller answers for d_row_offsets[b] + d_lengths[b] lying inside d_src.
 *   1 <= n_samples <= 2^21 (more is COUGH_EUNSUPPORTED);  n_rows <= 2^24 (the grid);  n_rows == 0 launches nothing. */
int cough_stretch_rows(const float* d_src, const long long* d_row_offsets, const int* d_lengths, int n_rows,
                       const cough_stretch_plan* d_plans, float* d_out, int n_samples, int* d_new_lengths, void* stream);

/* ------------------------------------------------------------------ the pitch draws of one batch
 * One thread per row draws by the contract above and writes the row's stretch plan (shift 0, the drawn entry's rate) to
 * d_stretch_plans_out[row], the resampler's plan (0, the entry's orig, sample_rate) to d_warp_plans_out[row] and the
 * length n_s the stretch gives the row to d_stretch_lengths_out[row].  A coin that did not fire, or n_steps == 0,
 * writes rate 1 and (0, sample_rate, sample_rate).  The stretch plan's mode word is (table[n_steps - lo].reserved & 1)
 * when the coin fired and n_steps != 0, and 0 otherwise: a table of zeros draws plain plans, as version 1 callers get.
 *   d_lengths: [n_rows] int32, the rows' lengths n (a length < 1 yields the blank plans and n_s = 0; a length above
 *              2^20 counts as 2^20)
 *   d_table:   [hi - lo + 1] cough_pitch_step, entry n_steps - lo for n_steps = lo .. hi, 8-byte aligned
 *   p_augment in [0, 1];  -12 <= lo <= hi <= 12;  1 <= sample_rate <= 2^20.  n_rows == 0 launches nothing. */
int cough_draw_pitch(unsigned long long seed, int n_rows, const int* d_lengths, double p_augment, int lo, int hi,
                     const cough_pitch_step* d_table, int sample_rate, cough_stretch_plan* d_stretch_plans_out,
                     cough_warp_plan* d_warp_plans_out, int* d_stretch_lengths_out, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* COUGH_AMD_PITCH_H */
