// libcough_amd_pitch.so: the time stretch of the waveform chain's pitch shift on the device (include/cough_amd_pitch.h).
// The stretch kernel runs a float64 phase vocoder over every row of a batch at a rate of its own; the draw kernel
// writes the per-row plans of the stretch and of the resampler that follows it from a seeded Philox stream.
//
// Launch shape.  One workgroup of 256 threads per row marches over the row's OUTPUT frames.  The spectra never leave
// the CU: a second of audio has 126 x 257 complex doubles (518 KB), so the workgroup keeps only the two input spectra
// an output frame interpolates between -- as magnitude and unit phasor per bin, transformed once each as the march
// reaches them -- the accumulated phasor P of bin `tid` in registers (thread 0 also carries bin 256), two FFT buffers
// and a 512-sample overlap-add ring whose finished 128 samples leave as float32 after every frame.  About 49 KB of LDS.
//
// Identity phase locking (plan.reserved bit 0, uniform over the block).  When an input frame is analysed, every bin
// decides whether it is a peak, the waves publish the decisions as ballots (four 64-bit words and bin 256), and every
// bin finds its nearest peak with a count-leading / find-first-set over at most five words: O(1) per bin whatever the
// number of peaks, once per input frame and at the cost of one barrier.  An output frame costs no barrier of its own:
// every bin leaves the phasor it carries into the next frame in LDS before the barriers of the inverse transform, and
// the bins that a peak owns read the peak's there and the two analysis phasors that tie them to it (two buffers, by
// the parity of t, because a wave may run ahead into the next frame's write).  A plain row skips all of it.
//
// The FFT is a 512-point complex radix-2 Stockham transform, one butterfly per thread and stage, nine barriers.  A
// real frame goes in with a zero imaginary part; the inverse transforms the conjugated Hermitian extension and keeps
// the real part.  Twiddles and window come from sincospi / cospi into LDS at kernel start.  Each thread's 16-byte
// element is one ds_read_b128 / ds_write_b128; the early stages write at a stride of 32 bytes (two passes).
//
// Cost.  A chain of about two dependent FFTs per output frame (one inverse and, on average, `rate` forward ones), each
// nine barriers deep: the kernel is bound by that chain and by the float64 pipe, not by memory (4 bytes in, 4 out per
// sample).
#include "../../include/cough_amd_pitch.h"

#include <cstdint>
#include <cstring>

#include "common.h"
#include "philox.h"

namespace cough {

namespace {

constexpr int PT = 256;                        // threads of the stretch kernel: one butterfly each
constexpr int NFFT = COUGH_PITCH_N_FFT, HOP = COUGH_PITCH_HOP, HALF = NFFT / 2, BINS = HALF + 1;
constexpr int SPEC = BINS + 1;                 // a slot's arrays, padded to an even count
constexpr int MAX_LEN = COUGH_PITCH_MAX_LENGTH;
constexpr int DT = 64;                         // threads of the draw kernel: one row each
static_assert(NFFT == 512 && HOP == 128 && PT == HALF, "the kernel's index arithmetic is written for 512 / 128");

__device__ __forceinline__ bool stretchable(double rate, int n) {
    return rate >= 0.5 && rate <= 2.0 && rate != 1.0 && n >= HALF + 1;      // a NaN fails the comparisons
}

// n_s = (int)rint(n / rate), at most 2^21
__device__ __forceinline__ int stretched_length(int n, double rate) { return int(rint(double(n) / rate)); }

// One 512-point forward transform of x (complete and visible to the block on entry) through the ping-pong pair
// (x, y); returns the buffer that holds the result, visible to the block.  tw[m] = exp(-2 pi i m / 512).
__device__ __forceinline__ double2* fft512(double2* x, double2* y, const double2* __restrict__ tw, int tid) {
#pragma clang fp contract(off)
#pragma unroll 1
    for (int s = 0; s < 9; ++s) {
        const int ns = 1 << s, k = tid & (ns - 1);
        const double2 w = tw[k << (8 - s)];
        const double2 a = x[tid], c = x[tid + HALF];
        const double2 b = make_double2(c.x * w.x - c.y * w.y, c.x * w.y + c.y * w.x);
        const int j0 = ((tid - k) << 1) + k;
        y[j0] = make_double2(a.x + b.x, a.y + b.y);
        y[j0 + ns] = make_double2(a.x - b.x, a.y - b.y);
        __syncthreads();
        double2* t = x;
        x = y;
        y = t;
    }
    return x;
}

__global__ __launch_bounds__(PT) void stretch_kernel(const float* __restrict__ src, const long long* __restrict__ row_offsets,
                                                     const int* __restrict__ lengths,
                                                     const cough_stretch_plan* __restrict__ plans, float* __restrict__ out,
                                                     int n_samples, int* __restrict__ new_lengths) {
#pragma clang fp contract(off)
    __shared__ double2 tw[HALF];               // exp(-2 pi i m / 512)
    __shared__ double win[NFFT];               // the periodic Hann window
    __shared__ double2 buf_a[NFFT], buf_b[NFFT];
    __shared__ double s_mag[2][SPEC], s_ux[2][SPEC], s_uy[2][SPEC];   // the two cached input spectra
    __shared__ double ring[NFFT];              // overlap-add, sample m at m & 511
    __shared__ double2 s_q[2][SPEC];           // locked rows: R[t] of every bin at [t & 1], for the bins a peak owns
    __shared__ unsigned long long s_peaks[2][PT / 64 + 1];       // locked rows: per slot, the peaks of bins 0 .. 256 as bits
    __shared__ float red_peak[PT / 64];
    __shared__ int red_bad[PT / 64];

    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = min(max(lengths[b], 0), MAX_LEN);
    const cough_stretch_plan plan = plans[b];
    const int shift = min(max(plan.shift, -n), n);
    const double rate = plan.rate;
    const bool lock = (plan.reserved & COUGH_STRETCH_PHASE_LOCK) != 0;       // uniform over the block
    const float* x = src + row_offsets[b];
    float* o = out + (long long)b * n_samples;

    auto shifted = [&](int i) {                // x_s[i] for 0 <= i < n
        const int j = i - shift;
        return (j >= 0 && j < n) ? x[j] : 0.0f;
    };

    if (!stretchable(rate, n)) {               // a (shifted) copy; n_s = n
        const int kept = min(n, n_samples);
        if (tid == 0 && new_lengths) new_lengths[b] = kept;
        for (int m = tid; m < n_samples; m += PT) o[m] = m < kept ? shifted(m) : 0.0f;
        return;
    }

    const int n_s = stretched_length(n, rate), kept = min(n_s, n_samples);
    if (tid == 0 && new_lengths) new_lengths[b] = kept;

    // ---- peak of x_s and whether it is finite
    float pk = 0.0f;
    int bad = 0;
    for (int i = tid; i < n; i += PT) {
        const float v = shifted(i);
        bad |= !(fabsf(v) <= 3.4028234663852886e38f);          // NaN or Inf
        pk = fmaxf(pk, fabsf(v));
    }
    pk = wave_max(pk);
    bad = __any(bad);
    if ((tid & 63) == 0) {
        red_peak[tid >> 6] = pk;
        red_bad[tid >> 6] = bad;
    }
    // ---- tables
    {
        double sn, cs;
        sincospi(double(tid) / double(HALF), &sn, &cs);        // 2 pi tid / 512 = pi tid / 256
        tw[tid] = make_double2(cs, -sn);
        win[tid] = 0.5 - 0.5 * cs;
        win[tid + HALF] = 0.5 - 0.5 * cospi(double(tid + HALF) / double(HALF));
        ring[tid] = 0.0;
        ring[tid + HALF] = 0.0;
    }
    __syncthreads();
    const double peak = double(fmaxf(fmaxf(red_peak[0], red_peak[1]), fmaxf(red_peak[2], red_peak[3])));
    const bool poisoned = (red_bad[0] | red_bad[1] | red_bad[2] | red_bad[3]) != 0;
    if (poisoned || peak == 0.0) {             // uniform over the block
        const float fill = poisoned ? __builtin_nanf("") : 0.0f;
        for (int m = tid; m < n_samples; m += PT) o[m] = m < kept ? fill : 0.0f;
        return;
    }
    const double floor_mag = peak * 0x1p-16;   // 2^-24 * 256 * peak
    const int T = 1 + n / HOP;
    const int T_out = int(ceil(double(T) / rate));

    // the transform of input frame f into slot s: magnitude and unit phasor of bins 0 .. 256
    auto analyse = [&](int f, int s) {
        if (f >= T) {                          // the two zero frames behind the row
            s_mag[s][tid] = 0.0;
            s_ux[s][tid] = 1.0;
            s_uy[s][tid] = 0.0;
            if (tid == 0) {
                s_mag[s][HALF] = 0.0;
                s_ux[s][HALF] = 1.0;
                s_uy[s][HALF] = 0.0;
            }
            if (lock && tid <= PT / 64) s_peaks[s][tid] = 0ull;               // no peaks: every bin owns itself
            __syncthreads();
            return;
        }
        for (int j = tid; j < NFFT; j += PT) {
            int i = f * HOP - HALF + j;        // -256 .. n + 255: one reflection is enough, n >= 257
            i = i < 0 ? -i : i;
            i = i >= n ? 2 * (n - 1) - i : i;
            buf_a[j] = make_double2(win[j] * double(shifted(i)), 0.0);
        }
        __syncthreads();
        const double2* S = fft512(buf_a, buf_b, tw, tid);
        for (int k = tid; k < BINS; k += PT) {
            const double2 v = S[k];
            const double m = sqrt(v.x * v.x + v.y * v.y);
            const bool low = m <= floor_mag;
            s_mag[s][k] = m;
            s_ux[s][k] = low ? 1.0 : v.x / m;
            s_uy[s][k] = low ? 0.0 : v.y / m;
        }
        __syncthreads();
        if (!lock) return;
        // a peak is above the floor and above the bins within two of it (0 .. 256: there is no mirror)
        auto is_peak = [&](int k) {
            const double m = s_mag[s][k];
            bool pk = m > floor_mag;
            for (int d = -2; d <= 2; ++d) {
                const int j = k + d;
                if (d != 0 && j >= 0 && j <= HALF) pk = pk && m > s_mag[s][j];
            }
            return pk;
        };
        const unsigned long long votes = __ballot(is_peak(tid));
        if ((tid & 63) == 0) s_peaks[s][tid >> 6] = votes;
        if (tid == 0) s_peaks[s][PT / 64] = is_peak(HALF) ? 1ull : 0ull;
        __syncthreads();
    };
    // the nearest peak of bin k in slot s, the lower one on a tie; k itself when the frame has no peak.  Five words,
    // no loop over the peaks and no branch on them: selects only.
    auto owner = [&](int k, int s) {
        const int w = k >> 6, bit = k & 63;
        int below = -1, above = -1;
#pragma unroll
        for (int i = 0; i <= PT / 64; ++i) {
            const unsigned long long word = s_peaks[s][i];
            const unsigned long long lo = i < w ? word : i == w ? word & (~0ull >> (63 - bit)) : 0ull;      // peaks <= k
            const unsigned long long hi = i > w ? word : i == w ? word & (~0ull << bit) : 0ull;             // peaks >= k
            below = lo ? (i << 6) + 63 - __clzll((long long)lo) : below;                                    // the last word wins
            above = hi && above < 0 ? (i << 6) + __ffsll(hi) - 1 : above;                                   // the first
        }
        const int near = above < 0 || (below >= 0 && k - below <= above - k) ? below : above;
        return near < 0 ? k : near;
    };

    // env[m] = sum over the frames t that cover m of w[m - 128 t]^2, ascending t
    auto envelope = [&](int m) {
        const int t_lo = m >= NFFT ? (m - NFFT) / HOP + 1 : 0, t_hi = min(m / HOP, T_out - 1);
        double e = 0.0;
        for (int t = t_lo; t <= t_hi; ++t) {
            const double w = win[m - t * HOP];
            e = e + w * w;
        }
        return e;
    };
    // sample m of the overlap-add leaves the ring: output index m - 256
    auto emit = [&](int m) {
        const int q = m - HALF;
        if (q >= 0 && q < kept) o[q] = float(ring[m & (NFFT - 1)] / envelope(m));
        ring[m & (NFFT - 1)] = 0.0;
    };

    int slot_frame[2] = {-1, -1};              // which input frame each slot holds (uniform over the block)
    int own_0 = tid, own_1 = tid, own_nyq_0 = HALF, own_nyq_1 = HALF;        // locked rows: per slot, the owner of bin tid; of bin 256
    auto adopt = [&](int s) {                  // after analyse(f, s), whose last barrier published the slot's peaks
        if (!lock) return;
        const int p = owner(tid, s), p_nyq = tid == 0 ? owner(HALF, s) : HALF;
        own_0 = s ? own_0 : p;
        own_1 = s ? p : own_1;
        own_nyq_0 = s ? own_nyq_0 : p_nyq;
        own_nyq_1 = s ? p_nyq : own_nyq_1;
    };
    double2 P = make_double2(1.0, 0.0), P_nyq = make_double2(1.0, 0.0);      // bin tid; bin 256 (thread 0)
    for (int t = 0; t < T_out; ++t) {
        const double ts = double(t) * rate;
        const int i0 = int(floor(ts));
        const double a = ts - double(i0);
        // the slots of frames i0 and i0 + 1; a frame not held yet goes where the other one is not
        int s0 = slot_frame[0] == i0 ? 0 : slot_frame[1] == i0 ? 1 : -1;
        int s1 = slot_frame[0] == i0 + 1 ? 0 : slot_frame[1] == i0 + 1 ? 1 : -1;
        if (s0 < 0) {
            s0 = s1 == 0 ? 1 : 0;
            analyse(i0, s0);
            adopt(s0);
            slot_frame[s0] = i0;
        }
        if (s1 < 0) {
            s1 = 1 - s0;
            analyse(i0 + 1, s1);
            adopt(s1);
            slot_frame[s1] = i0 + 1;
        }
        if (t == 0) {
            P = make_double2(s_ux[s0][tid], s_uy[s0][tid]);
            if (tid == 0) P_nyq = make_double2(s_ux[s0][HALF], s_uy[s0][HALF]);
        }
        if (lock) {
            // Q[t]: a peak keeps the phasor it carries; a bin it owns takes the peak's, turned by the phase the bin
            // has against the peak in input frame i0.  P holds R[t] on entry and Q[t] on exit.  Every bin left its
            // R[t] in s_q[t & 1] before the barriers of frame t - 1's inverse transform, so frame 0 alone needs one.
            if (t == 0) {
                s_q[0][tid] = P;
                if (tid == 0) s_q[0][HALF] = P_nyq;
                __syncthreads();
            }
            auto led = [&](int k, int p) {
                const double2 r = s_q[t & 1][p];
                const double ukx = s_ux[s0][k], uky = s_uy[s0][k], upx = s_ux[s0][p], upy = s_uy[s0][p];
                const double cx = ukx * upx + uky * upy, cy = uky * upx - ukx * upy;  // u(S[k]) * conj(u(S[p]))
                return make_double2(r.x * cx - r.y * cy, r.x * cy + r.y * cx);
            };
            const int p = s0 ? own_1 : own_0, p_nyq = s0 ? own_nyq_1 : own_nyq_0;
            if (p != tid) P = led(tid, p);
            if (tid == 0 && p_nyq != HALF) P_nyq = led(HALF, p_nyq);
        }
        // Y[t] = mag * P into the conjugated Hermitian extension; then P advances by u(S[i0+1]) conj(u(S[i0])) (locked
        // rows: R[t+1] = Q[t] times the same step)
        auto synthesise = [&](int k, double2& p) {
            const double mag = a * s_mag[s1][k] + (1.0 - a) * s_mag[s0][k];
            const double yr = mag * p.x, yi = mag * p.y;
            buf_a[k] = make_double2(yr, -yi);
            if (k > 0 && k < HALF) buf_a[NFFT - k] = make_double2(yr, yi);
            const double u1x = s_ux[s1][k], u1y = s_uy[s1][k], u0x = s_ux[s0][k], u0y = s_uy[s0][k];
            const double dx = u1x * u0x + u1y * u0y, dy = u1y * u0x - u1x * u0y;      // u1 * conj(u0)
            const double px = p.x * dx - p.y * dy, py = p.x * dy + p.y * dx;
            const double r = sqrt(px * px + py * py);
            p = make_double2(px / r, py / r);
        };
        synthesise(tid, P);
        if (tid == 0) synthesise(HALF, P_nyq);
        if (lock) {                            // R[t + 1] for the bins that a peak of the next frame's i0 owns
            s_q[(t + 1) & 1][tid] = P;
            if (tid == 0) s_q[(t + 1) & 1][HALF] = P_nyq;
        }
        __syncthreads();
        const double2* y = fft512(buf_a, buf_b, tw, tid);
        for (int j = tid; j < NFFT; j += PT) {
            const int slot = (t * HOP + j) & (NFFT - 1);       // every slot exactly once per frame
            ring[slot] = ring[slot] + win[j] * (y[j].x * (1.0 / NFFT));
        }
        __syncthreads();
        if (tid < HOP) emit(t * HOP + tid);    // nothing later touches [128 t, 128 t + 128)
        __syncthreads();
    }
    // the last frame's remaining 384 samples
    for (int j = tid; j < NFFT - HOP; j += PT) emit(T_out * HOP + j);
    for (int m = kept + tid; m < n_samples; m += PT) o[m] = 0.0f;
    // the overlap-add holds 128 T_out + 384 samples, of which the first 256 are dropped: it never ends before n_s
    // (cough_amd_pitch.h), but a sample it did not reach is 0 by the contract
    for (int m = max(T_out * HOP + (NFFT - HOP) - HALF, 0) + tid; m < kept; m += PT) o[m] = 0.0f;
}

// ------------------------------------------------------------------------------------------ the pitch draws of one row
// The contract of cough_amd_pitch.h, operator by operator; tests/pitch_ref.py restates it in numpy and the plans are
// compared bit for bit: contraction is off for this function.
__global__ __launch_bounds__(DT) void draw_pitch_kernel(unsigned long long seed, int n_rows, const int* __restrict__ lengths,
                                                        double p, int lo, int hi, const cough_pitch_step* __restrict__ table,
                                                        int sample_rate, cough_stretch_plan* __restrict__ stretch_plans,
                                                        cough_warp_plan* __restrict__ warp_plans, int* __restrict__ stretch_lengths) {
#pragma clang fp contract(off)
    const int row = blockIdx.x * DT + threadIdx.x;
    if (row >= n_rows) return;
    const uint2 key = make_uint2(unsigned(seed), unsigned(seed >> 32));
    auto unit = [](unsigned x) { return (double(x) + 0.5) * 0x1p-32; };
    cough_stretch_plan sp;
    sp.shift = 0;
    sp.reserved = 0;                           // the mode
    sp.rate = 1.0;
    cough_warp_plan wp;
    wp.shift = 0;
    wp.orig = sample_rate;
    wp.new_rate = sample_rate;
    const int n = min(lengths[row], MAX_LEN);
    int n_s = 0;
    if (n >= 1) {
        const uint4 d = philox4x32_10(make_uint4(0u, unsigned(row), 0u, 3u), key);
        if (unit(d.x) <= p) {
            const int steps = min(lo + int(double(hi - lo + 1) * unit(d.y)), hi);
            if (steps != 0) {
                sp.rate = table[steps - lo].rate;
                sp.reserved = table[steps - lo].reserved & COUGH_STRETCH_PHASE_LOCK;
                wp.orig = table[steps - lo].orig;
            }
        }
        n_s = stretchable(sp.rate, n) ? stretched_length(n, sp.rate) : n;
    }
    stretch_plans[row] = sp;
    warp_plans[row] = wp;
    stretch_lengths[row] = n_s;
}

}  // namespace
}  // namespace cough

extern "C" int cough_pitch_abi_version(void) { return COUGH_PITCH_ABI_VERSION; }
// this library's own last-error slot (libcough_amd.so keeps its own behind cough_amd_last_error)
COUGH_DEFINE_LAST_ERROR(cough_pitch_last_error)

extern "C" int cough_stretch_rows(const float* d_src, const long long* d_row_offsets, const int* d_lengths, int n_rows,
                                  const cough_stretch_plan* d_plans, float* d_out, int n_samples, int* d_new_lengths,
                                  void* stream) {
    using namespace cough;
    const char* fn = "cough_stretch_rows";
    COUGH_REQUIRE(n_rows >= 0 && n_samples >= 1, COUGH_EINVAL, "%s: bad sizes (%d rows of %d samples)", fn, n_rows, n_samples);
    COUGH_REQUIRE(n_samples <= COUGH_PITCH_MAX_SAMPLES, COUGH_EUNSUPPORTED, "%s: n_samples = %d is more than 2^21", fn, n_samples);
    COUGH_REQUIRE(n_rows <= (1 << 24), COUGH_EUNSUPPORTED, "%s: %d rows are more than 2^24 blocks; split the batch", fn, n_rows);
    if (n_rows == 0) return COUGH_OK;
    COUGH_REQUIRE(d_src && d_row_offsets && d_lengths && d_plans && d_out, COUGH_EINVAL, "%s: NULL argument", fn);
    COUGH_REQUIRE(d_out != d_src, COUGH_EINVAL, "%s: d_out must not alias d_src", fn);
    COUGH_REQUIRE(aligned(d_src, 4) && aligned(d_out, 4) && aligned(d_lengths, 4) && aligned(d_new_lengths, 4), COUGH_EINVAL,
                  "%s: float32 and int32 arrays must be 4-byte aligned", fn);
    COUGH_REQUIRE(aligned(d_row_offsets, 8) && aligned(d_plans, 8), COUGH_EINVAL,
                  "%s: d_row_offsets and d_plans must be 8-byte aligned", fn);
    hipLaunchKernelGGL(stretch_kernel, dim3(unsigned(n_rows)), dim3(PT), 0, static_cast<hipStream_t>(stream), d_src, d_row_offsets,
                       d_lengths, d_plans, d_out, n_samples, d_new_lengths);
    COUGH_HIP_CHECK(hipGetLastError());
    return COUGH_OK;
}

extern "C" int cough_draw_pitch(unsigned long long seed, int n_rows, const int* d_lengths, double p_augment, int lo, int hi,
                                const cough_pitch_step* d_table, int sample_rate, cough_stretch_plan* d_stretch_plans_out,
                                cough_warp_plan* d_warp_plans_out, int* d_stretch_lengths_out, void* stream) {
    using namespace cough;
    const char* fn = "cough_draw_pitch";
    COUGH_REQUIRE(n_rows >= 0, COUGH_EINVAL, "%s: n_rows must not be negative, got %d", fn, n_rows);
    COUGH_REQUIRE(p_augment >= 0.0 && p_augment <= 1.0, COUGH_EINVAL, "%s: p_augment = %g (0..1)", fn, p_augment);
    COUGH_REQUIRE(lo >= -COUGH_PITCH_MAX_STEPS && lo <= hi && hi <= COUGH_PITCH_MAX_STEPS, COUGH_EINVAL,
                  "%s: pitch range (%d, %d) must satisfy -12 <= lo <= hi <= 12", fn, lo, hi);
    COUGH_REQUIRE(sample_rate >= 1 && sample_rate <= COUGH_WARP_MAX_RATE, COUGH_EINVAL, "%s: sample_rate = %d (1..2^20)", fn,
                  sample_rate);
    if (n_rows == 0) return COUGH_OK;
    COUGH_REQUIRE(d_lengths && d_table && d_stretch_plans_out && d_warp_plans_out && d_stretch_lengths_out, COUGH_EINVAL,
                  "%s: NULL argument", fn);
    COUGH_REQUIRE(aligned(d_lengths, 4) && aligned(d_warp_plans_out, 4) && aligned(d_stretch_lengths_out, 4), COUGH_EINVAL,
                  "%s: int32 arrays must be 4-byte aligned", fn);
    COUGH_REQUIRE(aligned(d_table, 8) && aligned(d_stretch_plans_out, 8), COUGH_EINVAL,
                  "%s: d_table and d_stretch_plans_out must be 8-byte aligned", fn);
    hipLaunchKernelGGL(draw_pitch_kernel, dim3(unsigned((n_rows + DT - 1) / DT)), dim3(DT), 0, static_cast<hipStream_t>(stream), seed,
                       n_rows, d_lengths, p_augment, lo, hi, d_table, sample_rate, d_stretch_plans_out, d_warp_plans_out,
                       d_stretch_lengths_out);
    COUGH_HIP_CHECK(hipGetLastError());
    return COUGH_OK;
}
