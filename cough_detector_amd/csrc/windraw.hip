// libcough_amd_windraw.so: a batch's window plans drawn on the device (include/cough_amd_windraw.h).  One thread per row
// turns six Philox blocks at most into the 80-byte record cough_compose_windows reads and the row's label.
//
// Launch shape.  Workgroups of 64 threads, one row per thread: a batch of 32 to 256 rows is one to four waves, and a row
// is a few hundred scalar-like operations with three dependent table reads (the background's length, the picked clip,
// its length), so the launch is latency, not throughput.  The tables are read through the vector path -- every row picks
// its own entry -- and the record is written as one 80-byte struct per lane with plain stores; nothing is shared between
// rows, so there is no LDS, no barrier and no atomic.
#include "../../include/cough_amd_windraw.h"

#include <cmath>
#include <cstdint>

#include "common.h"
#include "philox.h"

namespace cough {

namespace {

constexpr int DT = COUGH_WINDRAW_THREADS, SLOTS = COUGH_WINDOWS_MAX_EVENTS, LEVELS = COUGH_WINDRAW_SNR_LEVELS;
static_assert(LEVELS == 1 << 10, "the SNR level is the word's top ten bits");
static_assert(sizeof(cough_window_plan) == 80 && SLOTS == 4, "the record of cough_amd_windows.h");

struct DrawArgs {
    unsigned long long seed;
    int n_rows, width;
    const int* bg_lengths;
    int n_bg;
    const int* ev_lengths;
    int n_ev;
    const int* cough_clips;
    int n_coughs;
    const int* distractor_clips;
    int n_distractors;
    double p_cough;
    int coughs_lo, coughs_hi;
    double p_distractor, gain_lo, gain_hi;
    const double* snr_linear;
    int m, margin;
    double rho_min;
    cough_window_plan* plans;
    long long* labels;
};

__device__ __forceinline__ double unit(unsigned x) {
#pragma clang fp contract(off)
    return (double(x) + 0.5) * 0x1p-32;
}

// an integer in [lo, hi], lo <= hi
__device__ __forceinline__ long long pick(unsigned x, long long lo, long long hi) {
#pragma clang fp contract(off)
    const long long span = hi - lo;
    const double scaled = unit(x) * double(span + 1);
    return lo + min((long long)scaled, span);
}

// The contract of cough_amd_windraw.h, operator by operator; tests/windraw_ref.py restates it in numpy.
__global__ __launch_bounds__(DT) void draw_window_plans_kernel(const DrawArgs a) {
#pragma clang fp contract(off)
    const int row = blockIdx.x * DT + threadIdx.x;
    if (row >= a.n_rows) return;
    const uint2 key = make_uint2(unsigned(a.seed), unsigned(a.seed >> 32));
    auto block = [&](unsigned s) { return philox4x32_10(make_uint4(s, unsigned(row), 0u, 6u), key); };

    cough_window_plan plan;
    const uint4 s0 = block(0u);
    plan.background = -1;
    plan.bg_start = 0;
    if (a.n_bg >= 1) {
        const int background = int(pick(s0.x, 0, a.n_bg - 1));
        const int n_b = a.bg_lengths[background];
        if (n_b >= 1) {
            plan.background = background;
            plan.bg_start = int(pick(s0.y, 0, n_b - 1));
        }
    }
    const double gain_span = a.gain_hi - a.gain_lo;
    const double gain_scaled = gain_span * unit(s0.z);
    plan.bg_gain = float(a.gain_lo + gain_scaled);
    const bool positive = unit(s0.w) <= a.p_cough;

    const uint4 s1 = block(1u);
    const int n_coughs = positive ? int(pick(s1.x, a.coughs_lo, a.coughs_hi)) : 0;
    const bool distracted = unit(s1.y) <= a.p_distractor && a.n_distractors > 0;
    const int n_others = distracted ? min(int(pick(s1.z, 1, 2)), SLOTS - n_coughs) : 0;
    plan.n_events = n_coughs + n_others;

#pragma unroll
    for (int e = 0; e < SLOTS; ++e) {
        int clip = -1, onset = 0;
        double snr = 1.0;
        if (e < plan.n_events) {
            const uint4 d = block(2u + unsigned(e));
            clip = e < n_coughs ? a.cough_clips[pick(d.x, 0, a.n_coughs - 1)] : a.distractor_clips[pick(d.y, 0, a.n_distractors - 1)];
            snr = a.snr_linear[d.z >> 22];
            if (clip >= 0 && clip < a.n_ev) {                // an index outside the bank keeps onset 0: the composer skips it
                const long long n_c = max(a.ev_lengths[clip], 0);
                const long long m_c = min((long long)a.m, n_c);
                const double stretched = double(m_c) / a.rho_min;
                const long long need = min(n_c, (long long)ceil(stretched));
                onset = int(pick(d.w, a.margin + need - n_c, a.width - a.margin - need));
            }
        }
        plan.clip[e] = clip;
        plan.onset[e] = onset;
        plan.snr_linear[e] = snr;
    }
    a.plans[row] = plan;
    a.labels[row] = n_coughs > 0 ? 1 : 0;
}

bool probability(double p) { return p >= 0.0 && p <= 1.0; }                          // false for a NaN
bool fits_float(double g) { return std::isfinite(g) && std::fabs(g) <= 3.4028234663852886e38; }

}  // namespace
}  // namespace cough

extern "C" int cough_windraw_abi_version(void) { return COUGH_WINDRAW_ABI_VERSION; }
// this library's own last-error slot
COUGH_DEFINE_LAST_ERROR(cough_windraw_last_error)

extern "C" int cough_draw_window_plans(unsigned long long seed, int n_rows, int width, const int* d_bg_lengths, int n_bg,
                                       const int* d_ev_lengths, int n_ev, const int* d_cough_clips, int n_coughs,
                                       const int* d_distractor_clips, int n_distractors, double p_cough, int coughs_lo,
                                       int coughs_hi, double p_distractor, double bg_gain_lo, double bg_gain_hi,
                                       const double* d_snr_linear, int min_overlap_samples, int margin, double rho_min,
                                       cough_window_plan* d_plans, long long* d_labels, void* stream) {
    using namespace cough;
    const char* fn = "cough_draw_window_plans";
    COUGH_REQUIRE(n_rows >= 0 && n_bg >= 0 && n_ev >= 0 && n_coughs >= 0 && n_distractors >= 0 && margin >= 0, COUGH_EINVAL,
                  "%s: n_rows = %d, n_bg = %d, n_ev = %d, n_coughs = %d, n_distractors = %d, margin = %d must not be negative",
                  fn, n_rows, n_bg, n_ev, n_coughs, n_distractors, margin);
    COUGH_REQUIRE(width >= 1 && width <= COUGH_WINDOWS_MAX_WIDTH, COUGH_EINVAL, "%s: width = %d (1..%d)", fn, width,
                  COUGH_WINDOWS_MAX_WIDTH);
    COUGH_REQUIRE(probability(p_cough), COUGH_EINVAL, "%s: p_cough = %g (0..1)", fn, p_cough);
    COUGH_REQUIRE(probability(p_distractor), COUGH_EINVAL, "%s: p_distractor = %g (0..1)", fn, p_distractor);
    COUGH_REQUIRE(1 <= coughs_lo && coughs_lo <= coughs_hi && coughs_hi <= SLOTS, COUGH_EINVAL,
                  "%s: coughs per window (%d, %d) must satisfy 1 <= lo <= hi <= %d", fn, coughs_lo, coughs_hi, SLOTS);
    COUGH_REQUIRE(p_cough == 0.0 || n_coughs > 0, COUGH_EINVAL, "%s: p_cough = %g but there is no cough clip", fn, p_cough);
    COUGH_REQUIRE(p_distractor == 0.0 || n_distractors > 0, COUGH_EINVAL, "%s: p_distractor = %g but there is no distractor clip",
                  fn, p_distractor);
    COUGH_REQUIRE(rho_min > 0.0 && rho_min <= 1.0, COUGH_EINVAL, "%s: rho_min = %g must lie in (0, 1]", fn, rho_min);
    COUGH_REQUIRE(min_overlap_samples >= 1, COUGH_EINVAL, "%s: min_overlap_samples = %d must be at least 1", fn,
                  min_overlap_samples);
    const double asked = std::ceil(double(min_overlap_samples) / rho_min);
    const long long inner = (long long)width - 2LL * margin;
    COUGH_REQUIRE(double(inner) >= asked, COUGH_EINVAL,
                  "%s: the inner window (width %d less a margin of %d on each side: %lld samples) cannot hold the %.0f samples "
                  "that min_overlap_samples = %d asks for at rho_min = %g", fn, width, margin, inner, asked, min_overlap_samples,
                  rho_min);
    COUGH_REQUIRE(fits_float(bg_gain_lo) && fits_float(bg_gain_hi), COUGH_EINVAL,
                  "%s: the gain range (%g, %g) must be finite and fit a float32", fn, bg_gain_lo, bg_gain_hi);
    if (n_rows == 0) return COUGH_OK;
    COUGH_REQUIRE(d_snr_linear && d_plans && d_labels, COUGH_EINVAL, "%s: NULL argument", fn);
    COUGH_REQUIRE(n_bg == 0 || d_bg_lengths, COUGH_EINVAL, "%s: NULL background lengths with n_bg = %d", fn, n_bg);
    COUGH_REQUIRE(n_ev == 0 || d_ev_lengths, COUGH_EINVAL, "%s: NULL event lengths with n_ev = %d", fn, n_ev);
    COUGH_REQUIRE((n_coughs == 0 || d_cough_clips) && (n_distractors == 0 || d_distractor_clips), COUGH_EINVAL,
                  "%s: NULL clip list with n_coughs = %d, n_distractors = %d", fn, n_coughs, n_distractors);
    COUGH_REQUIRE(aligned(d_bg_lengths, 4) && aligned(d_ev_lengths, 4) && aligned(d_cough_clips, 4) && aligned(d_distractor_clips, 4),
                  COUGH_EINVAL, "%s: int32 arrays must be 4-byte aligned", fn);
    COUGH_REQUIRE(aligned(d_snr_linear, 8) && aligned(d_plans, 8) && aligned(d_labels, 8), COUGH_EINVAL,
                  "%s: d_snr_linear, d_plans and d_labels must be 8-byte aligned", fn);
    const DrawArgs a{seed, n_rows, width, d_bg_lengths, n_bg, d_ev_lengths, n_ev, d_cough_clips, n_coughs, d_distractor_clips,
                     n_distractors, p_cough, coughs_lo, coughs_hi, p_distractor, bg_gain_lo, bg_gain_hi, d_snr_linear,
                     min_overlap_samples, margin, rho_min, d_plans, d_labels};
    hipLaunchKernelGGL(draw_window_plans_kernel, dim3(unsigned((n_rows + DT - 1) / DT)), dim3(DT), 0,
                       static_cast<hipStream_t>(stream), a);
    COUGH_HIP_CHECK(hipGetLastError());
    return COUGH_OK;
}
