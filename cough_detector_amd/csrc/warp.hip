// libcough_amd_warp.so: speed perturbation on the device (include/cough_amd_warp.h).  The warp kernel resamples every row
// of a batch by a rate pair of its own with a windowed-sinc filter whose coefficients are evaluated per tap in float64 --
// there is no polyphase table -- and the draw kernel writes the per-row plans from a seeded Philox stream.
//
// Launch shape.  One block per (row, tile of WARP_TILE outputs).  The block stages the tile's input span -- at most
// WARP_TILE * 4 + 2 * 25 + 3 floats at the widest accepted ratio -- in LDS once, with the time shift and the row's ends
// already applied, so the tap loop reads LDS without a bound check.  Each thread then produces WARP_TILE / WARP_THREADS
// outputs, WARP_THREADS apart: a wave's 64 outputs are consecutive, its LDS reads are (nearly) consecutive addresses and
// its stores coalesce.  A row may start at any element, so the global reads are 4-byte scalars (64 consecutive floats
// of a wave still coalesce into whole cache lines).
//
// Cost.  The arithmetic is the float64 coefficient: per tap one rotation of (sin, cos)(pi t) and of (sin, cos)(pi t / 12)
// (8 multiply-adds), one float64 division, four multiplies and a conversion, against 4 bytes read and 4 written per
// output.  The kernel is bound by the float64 pipe, not by memory.
#include "../../include/cough_amd_warp.h"

#include <cstdint>
#include <cstring>

#include "common.h"
#include "philox.h"

namespace cough {

namespace {

constexpr int WARP_THREADS = 256;
constexpr int WARP_TILE = 1024;                // outputs per block
constexpr int WARP_MAX_WIDTH = 25;             // ceil(6 * 4 / 0.99): the widest filter of an accepted pair
// the span of a tile: floor((m0 + TILE - 1) * orig / new) - floor(m0 * orig / new) <= (TILE - 1) * 4 + 1, plus width
// taps before the first centre and width + 1 behind the last one
constexpr int WARP_SPAN = (WARP_TILE - 1) * COUGH_WARP_MAX_RATIO + 1 + 2 * WARP_MAX_WIDTH + 2;
constexpr int WARP_MAX_LEN = 1 << 30;
constexpr int DT = 64;                         // threads of the draw kernels: one row each
constexpr double PI = 3.14159265358979323846;

// A row's plan with everything the device cannot trust made harmless (cough_amd_warp.h lists how).
struct Row {
    int n;                 // 0 .. 2^30
    int shift;             // -n .. n
    int orig, nw;          // an accepted pair; 1, 1 for a copy
    int width;             // <= WARP_MAX_WIDTH
    long long n_new;       // ceil(n * nw / orig) <= 2^32
    double base;           // 0.99 * min(orig, nw)
};

__device__ __forceinline__ Row resolve(cough_warp_plan p, int len) {
#pragma clang fp contract(off)
    Row r;
    r.n = min(max(len, 0), WARP_MAX_LEN);
    r.shift = min(max(p.shift, -r.n), r.n);
    int orig = p.orig, nw = p.new_rate;
    const bool usable = orig >= 1 && nw >= 1 && orig <= COUGH_WARP_MAX_RATE && nw <= COUGH_WARP_MAX_RATE &&
                        orig <= COUGH_WARP_MAX_RATIO * nw && nw <= COUGH_WARP_MAX_RATIO * orig;
    if (!usable || orig == nw) orig = nw = 1;
    r.base = double(min(orig, nw)) * 0.99;
    r.width = int(ceil(double(6LL * orig) / r.base));
    if (r.width > WARP_MAX_WIDTH) {            // cannot happen for an accepted pair; it keeps the LDS span provable
        orig = nw = 1;
        r.width = 0;
    }
    r.orig = orig;
    r.nw = nw;
    r.n_new = ((long long)r.n * nw + orig - 1) / orig;
    return r;
}

__global__ __launch_bounds__(WARP_THREADS) void warp_kernel(const float* __restrict__ src, const long long* __restrict__ row_offsets,
                                                            const int* __restrict__ lengths,
                                                            const cough_warp_plan* __restrict__ plans, float* __restrict__ out,
                                                            int n_samples, int tiles, int* __restrict__ new_lengths) {
    __shared__ float xs[WARP_SPAN];
    const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles, tid = threadIdx.x;
    const Row r = resolve(plans[b], lengths[b]);
    const float* x = src + row_offsets[b];
    float* o = out + (long long)b * n_samples;
    const int kept = int(min(r.n_new, (long long)n_samples));      // the row's samples that fit the output
    if (tile == 0 && tid == 0 && new_lengths) new_lengths[b] = kept;
    const int m0 = tile * WARP_TILE;
    const int m_end = min(m0 + WARP_TILE, n_samples);              // this tile writes [m0, m_end)
    const int m_live = min(m_end, kept);                           // ... of which [m0, m_live) are samples

    auto shifted = [&](long long i) {                              // x_s[i]; i may lie outside the row
        const long long j = i - r.shift;
        return (i >= 0 && i < r.n && j >= 0 && j < r.n) ? x[j] : 0.0f;
    };

    if (r.orig == r.nw) {                                          // a (shifted) copy; n' = n
        for (int m = m0 + tid; m < m_end; m += WARP_THREADS) o[m] = m < m_live ? shifted(m) : 0.0f;
        return;
    }
    if (m_live <= m0) {                                            // behind the row's end: zeros
        for (int m = m0 + tid; m < m_end; m += WARP_THREADS) o[m] = 0.0f;
        return;
    }

    const long long orig = r.orig, nw = r.nw;
    const long long i_lo = ((long long)m0 * orig) / nw - r.width;                       // first input of the first output
    const int span = int(((long long)(m_live - 1) * orig) / nw + r.width + 1 - i_lo) + 1;   // <= WARP_SPAN
    for (int k = tid; k < span; k += WARP_THREADS) xs[k] = shifted(i_lo + k);
    __syncthreads();

    const double cc = r.base / (double(orig) * double(nw));        // t per unit of num
    const double scale = r.base / double(orig);
    // the rotation from one tap to the next: num grows by nw, so pi t by pi * nw * cc and pi t / 12 by a twelfth of it
    double rs, rc, ws, wc;
    sincos(PI * (double(nw) * cc), &rs, &rc);
    sincos(PI * (double(nw) * cc) / 12.0, &ws, &wc);
    const int taps = 2 * r.width + 2;
    for (int m = m0 + tid; m < m_end; m += WARP_THREADS) {
        float acc = 0.0f;
        if (m < m_live) {
            const long long first = ((long long)m * orig) / nw - r.width;
            long long num = first * nw - (long long)m * orig;
            const float* xt = xs + (first - i_lo);
            double s, c, sw, cw;
            sincos(PI * (double(num) * cc), &s, &c);
            sincos(PI * (double(num) * cc) / 12.0, &sw, &cw);
            for (int k = 0; k < taps; ++k) {
                const double t = double(num) * cc;
                float h = 0.0f;                                    // |t| >= 6: the clamped value rounds to 0
                if (fabs(t) < 6.0) {
                    const double tp = t * PI;
                    const double sinc = num == 0 ? 1.0 : s / tp;
                    h = float(sinc * (cw * cw * scale));
                }
                acc = fmaf(xt[k], h, acc);
                const double s2 = s * rc + c * rs, sw2 = sw * wc + cw * ws;
                c = c * rc - s * rs;
                cw = cw * wc - sw * ws;
                s = s2;
                sw = sw2;
                num += nw;
            }
        }
        o[m] = acc;
    }
}

// ------------------------------------------------------------------------------------------ the speed draws of one row
// The contract of cough_amd_warp.h, operator by operator; tests/warp_ref.py restates it in numpy, which has no fused
// multiply-add, and the plans are compared bit for bit: contraction is off for this function.
__global__ __launch_bounds__(DT) void draw_speed_kernel(unsigned long long seed, int n_rows, const int* __restrict__ lengths,
                                                        double p, double lo, double hi, int sample_rate,
                                                        cough_warp_plan* __restrict__ plans, int* __restrict__ new_lengths) {
#pragma clang fp contract(off)
    const int row = blockIdx.x * DT + threadIdx.x;
    if (row >= n_rows) return;
    const uint2 key = make_uint2(unsigned(seed), unsigned(seed >> 32));
    auto unit = [](unsigned x) { return (double(x) + 0.5) * 0x1p-32; };
    cough_warp_plan pl;
    pl.shift = 0;
    pl.orig = sample_rate;
    pl.new_rate = sample_rate;
    const int n = min(lengths[row], WARP_MAX_LEN);
    long long n_new = 0;
    if (n >= 1) {
        const uint4 s0 = philox4x32_10(make_uint4(0u, unsigned(row), 0u, 1u), key);
        const uint4 sp = philox4x32_10(make_uint4(0u, unsigned(row), 0u, 2u), key);
        if (unit(s0.x) <= p) {
            const double f = -0.2 + 0.4 * unit(s0.y);
            pl.shift = int(double(n) * f);
        }
        if (unit(sp.x) <= p) {
            const double factor = lo + (hi - lo) * unit(sp.y);
            pl.orig = int(factor * double(sample_rate));
        }
        n_new = ((long long)n * pl.new_rate + pl.orig - 1) / pl.orig;
    }
    plans[row] = pl;
    new_lengths[row] = int(min(n_new, (long long)WARP_MAX_LEN));
}

__global__ __launch_bounds__(DT) void clear_shifts_kernel(cough_aug_clip* __restrict__ clips, int n_rows) {
    const int row = blockIdx.x * DT + threadIdx.x;
    if (row < n_rows) clips[row].shift = 0;
}

}  // namespace
}  // namespace cough

extern "C" int cough_warp_abi_version(void) { return COUGH_WARP_ABI_VERSION; }
// this library's own last-error slot (libcough_amd.so keeps its own behind cough_amd_last_error)
COUGH_DEFINE_LAST_ERROR(cough_warp_last_error)

extern "C" int cough_warp_rows(const float* d_src, const long long* d_row_offsets, const int* d_lengths, int n_rows,
                               const cough_warp_plan* d_plans, float* d_out, int n_samples, int* d_new_lengths, void* stream) {
    using namespace cough;
    const char* fn = "cough_warp_rows";
    COUGH_REQUIRE(n_rows >= 0 && n_samples >= 1, COUGH_EINVAL, "%s: bad sizes (%d rows of %d samples)", fn, n_rows, n_samples);
    COUGH_REQUIRE(n_samples <= WARP_MAX_LEN, COUGH_EUNSUPPORTED, "%s: n_samples = %d is more than 2^30", fn, n_samples);
    const long long tiles = ((long long)n_samples + WARP_TILE - 1) / WARP_TILE;
    COUGH_REQUIRE(tiles * n_rows <= (1LL << 24), COUGH_EUNSUPPORTED,
                  "%s: %d rows of %lld tiles are more than 2^24 blocks; split the batch", fn, n_rows, tiles);
    if (n_rows == 0) return COUGH_OK;
    COUGH_REQUIRE(d_src && d_row_offsets && d_lengths && d_plans && d_out, COUGH_EINVAL, "%s: NULL argument", fn);
    COUGH_REQUIRE(d_out != d_src, COUGH_EINVAL, "%s: d_out must not alias d_src", fn);
    COUGH_REQUIRE(aligned(d_src, 4) && aligned(d_out, 4) && aligned(d_lengths, 4) && aligned(d_plans, 4) && aligned(d_new_lengths, 4),
                  COUGH_EINVAL, "%s: float32 and int32 arrays must be 4-byte aligned", fn);
    COUGH_REQUIRE(aligned(d_row_offsets, 8), COUGH_EINVAL, "%s: d_row_offsets must be 8-byte aligned", fn);
    hipLaunchKernelGGL(warp_kernel, dim3(unsigned(tiles * n_rows)), dim3(WARP_THREADS), 0, static_cast<hipStream_t>(stream), d_src,
                       d_row_offsets, d_lengths, d_plans, d_out, n_samples, int(tiles), d_new_lengths);
    COUGH_HIP_CHECK(hipGetLastError());
    return COUGH_OK;
}

extern "C" int cough_draw_speed(unsigned long long seed, int n_rows, const int* d_lengths, double p_augment, double lo, double hi,
                                int sample_rate, cough_warp_plan* d_plans_out, int* d_new_lengths_out, void* stream) {
    using namespace cough;
    const char* fn = "cough_draw_speed";
    COUGH_REQUIRE(n_rows >= 0, COUGH_EINVAL, "%s: n_rows must not be negative, got %d", fn, n_rows);
    COUGH_REQUIRE(p_augment >= 0.0 && p_augment <= 1.0, COUGH_EINVAL, "%s: p_augment = %g (0..1)", fn, p_augment);
    COUGH_REQUIRE(lo >= 0.25 && lo <= hi && hi <= 4.0, COUGH_EINVAL, "%s: speed range (%g, %g) must satisfy 1/4 <= lo <= hi <= 4", fn,
                  lo, hi);
    COUGH_REQUIRE(sample_rate >= 1 && sample_rate <= COUGH_WARP_MAX_RATE, COUGH_EINVAL, "%s: sample_rate = %d (1..2^20)", fn,
                  sample_rate);
    COUGH_REQUIRE(hi <= 1.0 || (long long)(hi * double(sample_rate)) < COUGH_WARP_MAX_RATE, COUGH_EINVAL,
                  "%s: speed range: (int)(%g * %d) must stay below 2^20", fn, hi, sample_rate);
    COUGH_REQUIRE(4LL * (long long)(lo * double(sample_rate)) >= sample_rate, COUGH_EINVAL,
                  "%s: speed range: (int)(%g * %d) is less than a quarter of the sample_rate", fn, lo, sample_rate);
    if (n_rows == 0) return COUGH_OK;
    COUGH_REQUIRE(d_lengths && d_plans_out && d_new_lengths_out, COUGH_EINVAL, "%s: NULL argument", fn);
    COUGH_REQUIRE(aligned(d_lengths, 4) && aligned(d_plans_out, 4) && aligned(d_new_lengths_out, 4), COUGH_EINVAL,
                  "%s: int32 arrays must be 4-byte aligned", fn);
    hipLaunchKernelGGL(draw_speed_kernel, dim3(unsigned((n_rows + DT - 1) / DT)), dim3(DT), 0, static_cast<hipStream_t>(stream), seed,
                       n_rows, d_lengths, p_augment, lo, hi, sample_rate, d_plans_out, d_new_lengths_out);
    COUGH_HIP_CHECK(hipGetLastError());
    return COUGH_OK;
}

extern "C" int cough_clear_shifts(cough_aug_clip* d_clips, int n_rows, void* stream) {
    using namespace cough;
    const char* fn = "cough_clear_shifts";
    COUGH_REQUIRE(n_rows >= 0, COUGH_EINVAL, "%s: n_rows must not be negative, got %d", fn, n_rows);
    if (n_rows == 0) return COUGH_OK;
    COUGH_REQUIRE(d_clips, COUGH_EINVAL, "%s: NULL argument", fn);
    COUGH_REQUIRE(aligned(d_clips, 8), COUGH_EINVAL, "%s: d_clips must be 8-byte aligned", fn);
    hipLaunchKernelGGL(clear_shifts_kernel, dim3(unsigned((n_rows + DT - 1) / DT)), dim3(DT), 0, static_cast<hipStream_t>(stream),
                       d_clips, n_rows);
    COUGH_HIP_CHECK(hipGetLastError());
    return COUGH_OK;
}
