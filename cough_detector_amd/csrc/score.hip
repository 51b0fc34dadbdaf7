// libcough_amd_score.so: whole recordings scored offline (include/cough_amd_score.h).  The per-window probabilities
// come from the existing pipeline; what is here is the reference engine's state machine -- a deque mean, a threshold,
// a debounce (src/inference.py:219-241) -- for every window of a corpus and for many thresholds at once.  Three kernels:
//
// smooth_windows_kernel   one thread per window.  The mean of <= 32 float64 values in numpy's order (a left-to-right sum
//     under 8 values, eight accumulators over whole blocks of 8 from there on): only additions and one IEEE division, so
//     the result equals float(np.mean(deque)) bit for bit.  The accumulators are indexed by unrolled constants and stay
//     in registers.
// sweep_thresholds_kernel one wave per (recording, 64 thresholds), lane = threshold.  The debounce makes a threshold's
//     walk over a recording sequential, but the walks of different thresholds are independent: the wave loads 64
//     consecutive s values with one coalesced load, and every lane then meets them one by one (v_readlane with a uniform
//     lane number: the control flow never diverges), keeping its threshold, the next index allowed to fire, its count
//     and its first index in registers.  A recording of 0 windows and one of 5,000 take the same loop.
// list_events_kernel      one wave per recording at one threshold: the ballot of s >= t over 64 windows, then the set bits
//     at or after `next`.  Both decide through walk_fires() / walk_advance(), so a recording's listed events number its
//     sweep count.
#include "../../include/cough_amd_score.h"

#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdint>

#include "common.h"
#include "score_walk.h"

namespace cough {

namespace {

constexpr int ST = 256;                               // threads of the smoothing kernel
constexpr int WPB = 4;                                // waves per workgroup of the two walking kernels
constexpr long long MAX_WINDOWS = 1LL << 38;          // ceil(n / ST) fits a grid
constexpr int NO_INDEX = INT_MAX;

// the walking rule -- walk_fires(), walk_advance(), clip_windows(), read_lane() -- lives in score_walk.h

// ------------------------------------------------------------------------------------------ deque mean
__global__ __launch_bounds__(ST) void smooth_windows_kernel(const float* __restrict__ prob, const long long* __restrict__ offs,
                                                            int n_clips, long long n_windows, int w,
                                                            double* __restrict__ smoothed) {
    const long long i = (long long)blockIdx.x * ST + threadIdx.x;
    if (i >= n_windows) return;
    // the last recording c with offs[c] <= i (recordings without a window share their successor's offset)
    int lo = 0, hi = n_clips;                          // offs[lo] <= i is taken for granted at lo = 0
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (offs[mid] <= i) lo = mid; else hi = mid;
    }
    const long long k = min(max(i - offs[lo], 0LL), i);   // the window's index in its recording; garbage offsets stay inside prob
    const int n = int(min((long long)w, k + 1));
    const float* a = prob + (i - n + 1);
    double sum;
    if (n < 8) {
        sum = double(a[0]);
        for (int j = 1; j < n; ++j) sum += double(a[j]);
    } else {
        double r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = double(a[j]);
        const int whole = n & ~7;
        for (int b = 8; b < whole; b += 8) {
#pragma unroll
            for (int j = 0; j < 8; ++j) r[j] += double(a[b + j]);
        }
        sum = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (int j = whole; j < n; ++j) sum += double(a[j]);
    }
    smoothed[i] = sum / double(n);
}

// ------------------------------------------------------------------------------------------ many thresholds at once
// the largest value and the lowest index that holds it, in every lane; idx == NO_INDEX marks a lane without a value
__device__ __forceinline__ void wave_first_max(double& v, int& idx) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const double ov = __shfl_xor(v, m, 64);
        const int oi = __shfl_xor(idx, m, 64);
        if (oi != NO_INDEX && (idx == NO_INDEX || ov > v || (ov == v && oi < idx))) {
            v = ov;
            idx = oi;
        }
    }
}

__global__ __launch_bounds__(64 * WPB) void sweep_thresholds_kernel(const double* __restrict__ smoothed,
                                                                    const long long* __restrict__ offs, int n_clips,
                                                                    long long n_windows, const double* __restrict__ thresholds,
                                                                    int n_thr, int groups, int gap, int* __restrict__ counts,
                                                                    int* __restrict__ first_window,
                                                                    double* __restrict__ peak_conf, int* __restrict__ peak_window) {
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * WPB + (threadIdx.x >> 6);
    if (wave >= (long long)n_clips * groups) return;   // a whole wave
    const int c = int(wave / groups), g = int(wave % groups);
    long long w0;
    int n;
    clip_windows(offs, c, n_windows, w0, n);
    const double* s = smoothed + w0;
    const int t = g * 64 + lane;
    const bool mine = t < n_thr;
    const double thr = mine ? thresholds[t] : 0.0;
    const bool peaks = g == 0 && (peak_conf || peak_window);   // wave-uniform

    long long next = 0;
    int count = 0, first = -1;
    double best = 0.0;
    int best_k = NO_INDEX;
    for (int base = 0; base < n; base += 64) {
        const int k_mine = base + lane;
        const double v = k_mine < n ? s[k_mine] : 0.0;
        if (peaks && k_mine < n && v == v && (best_k == NO_INDEX || v > best)) {   // ascending k per lane: the first stays
            best = v;
            best_k = k_mine;
        }
        const int cnt = min(64, n - base);
        for (int j = 0; j < cnt; ++j) {
            const double sv = read_lane(v, j);
            const int k = base + j;
            if (walk_fires(sv, thr, k, next)) {
                next = walk_advance(k, gap);
                if (first < 0) first = k;
                ++count;
            }
        }
    }
    if (mine) {
        const long long o = (long long)c * n_thr + t;
        if (counts) counts[o] = count;
        if (first_window) first_window[o] = first;
    }
    if (peaks) {
        wave_first_max(best, best_k);
        if (lane == 0) {
            if (peak_conf) peak_conf[c] = best_k == NO_INDEX ? __longlong_as_double(0x7ff8000000000000LL) : best;
            if (peak_window) peak_window[c] = best_k == NO_INDEX ? -1 : best_k;
        }
    }
}

// ------------------------------------------------------------------------------------------ one threshold: the events
__global__ __launch_bounds__(64 * WPB) void list_events_kernel(const double* __restrict__ smoothed,
                                                               const long long* __restrict__ offs, int n_clips,
                                                               long long n_windows, double thr, int gap,
                                                               const long long* __restrict__ event_offs, long long n_events,
                                                               int* __restrict__ event_window, double* __restrict__ event_conf) {
    const int lane = threadIdx.x & 63;
    const int c = blockIdx.x * WPB + (threadIdx.x >> 6);
    if (c >= n_clips) return;                          // a whole wave
    long long w0;
    int n;
    clip_windows(offs, c, n_windows, w0, n);
    const double* s = smoothed + w0;
    const long long e0 = min(max(event_offs[c], 0LL), n_events);
    const long long room = min(max(event_offs[c + 1], e0), n_events) - e0;

    long long next = 0, count = 0;
    for (int base = 0; base < n && count < room; base += 64) {
        const int k_mine = base + lane;
        const double v = k_mine < n ? s[k_mine] : 0.0;
        const unsigned long long above = __ballot(k_mine < n && v >= thr);
        long long pos = max(next - base, 0LL);         // every lane holds the same state: the walk is uniform
        while (pos < 64 && count < room) {
            const unsigned long long rest = above >> pos;
            if (!rest) break;
            pos += __builtin_ctzll(rest);
            const long long k = base + pos;
            if (walk_fires(read_lane(v, int(pos)), thr, k, next)) {   // true: a set bit at or after `next`
                if (lane == pos) {
                    event_window[e0 + count] = int(k);
                    event_conf[e0 + count] = v;
                }
                ++count;
                next = walk_advance(k, gap);
            }
            pos = max(next - base, pos + 1);
        }
    }
}

}  // namespace
}  // namespace cough

extern "C" int cough_score_abi_version(void) { return COUGH_SCORE_ABI_VERSION; }
// this library's own last-error slot (libcough_amd.so keeps its own behind cough_amd_last_error)
COUGH_DEFINE_LAST_ERROR(cough_score_last_error)

extern "C" int cough_smooth_windows(const float* d_prob, const long long* d_window_offsets, int n_clips, long long n_windows,
                                    int smoothing_window, double* d_smoothed, void* stream) {
    using namespace cough;
    const char* fn = "cough_smooth_windows";
    COUGH_REQUIRE(d_prob && d_window_offsets && d_smoothed, COUGH_EINVAL, "%s: NULL argument", fn);
    COUGH_REQUIRE(n_clips >= 0, COUGH_EINVAL, "%s: n_clips must not be negative, got %d", fn, n_clips);
    COUGH_REQUIRE(n_windows >= 0 && n_windows < MAX_WINDOWS, COUGH_EINVAL, "%s: n_windows = %lld (0..2^38 - 1)", fn,
                  n_windows);
    COUGH_REQUIRE(smoothing_window >= 1 && smoothing_window <= COUGH_MAX_SMOOTHING, COUGH_EINVAL,
                  "%s: smoothing_window = %d (1..%d)", fn, smoothing_window, COUGH_MAX_SMOOTHING);
    COUGH_REQUIRE(aligned(d_prob, 4), COUGH_EINVAL, "%s: float32 arrays must be 4-byte aligned", fn);
    COUGH_REQUIRE(aligned(d_window_offsets, 8) && aligned(d_smoothed, 8), COUGH_EINVAL,
                  "%s: int64 and float64 arrays must be 8-byte aligned", fn);
    if (n_clips == 0 || n_windows == 0) return COUGH_OK;
    hipLaunchKernelGGL(smooth_windows_kernel, dim3(unsigned((n_windows + ST - 1) / ST)), dim3(ST), 0,
                       static_cast<hipStream_t>(stream), d_prob, d_window_offsets, n_clips, n_windows, smoothing_window,
                       d_smoothed);
    COUGH_HIP_CHECK(hipGetLastError());
    return COUGH_OK;
}

extern "C" int cough_sweep_thresholds(const double* d_smoothed, const long long* d_window_offsets, int n_clips,
                                      long long n_windows, const double* d_thresholds, int n_thresholds, int gap,
                                      int* d_counts, int* d_first_window, double* d_peak_conf, int* d_peak_window,
                                      void* stream) {
    using namespace cough;
    const char* fn = "cough_sweep_thresholds";
    COUGH_REQUIRE(d_smoothed && d_window_offsets && d_thresholds, COUGH_EINVAL, "%s: NULL argument", fn);
    COUGH_REQUIRE(n_clips >= 0, COUGH_EINVAL, "%s: n_clips must not be negative, got %d", fn, n_clips);
    COUGH_REQUIRE(n_windows >= 0 && n_windows < MAX_WINDOWS, COUGH_EINVAL, "%s: n_windows = %lld (0..2^38 - 1)", fn,
                  n_windows);
    COUGH_REQUIRE(n_thresholds >= 1 && n_thresholds <= COUGH_MAX_THRESHOLDS, COUGH_EINVAL, "%s: n_thresholds = %d (1..%d)",
                  fn, n_thresholds, COUGH_MAX_THRESHOLDS);
    COUGH_REQUIRE(gap >= 1, COUGH_EINVAL, "%s: gap must be positive, got %d", fn, gap);
    COUGH_REQUIRE(aligned(d_counts, 4) && aligned(d_first_window, 4) && aligned(d_peak_window, 4), COUGH_EINVAL,
                  "%s: int32 arrays must be 4-byte aligned", fn);
    COUGH_REQUIRE(aligned(d_smoothed, 8) && aligned(d_window_offsets, 8) && aligned(d_thresholds, 8) &&
                  aligned(d_peak_conf, 8), COUGH_EINVAL, "%s: int64 and float64 arrays must be 8-byte aligned", fn);
    if (n_clips == 0) return COUGH_OK;
    const int groups = (n_thresholds + 63) / 64;
    const long long blocks = ((long long)n_clips * groups + WPB - 1) / WPB;
    COUGH_REQUIRE(blocks <= INT_MAX, COUGH_EUNSUPPORTED, "%s: %d recordings x %d thresholds do not fit one launch", fn,
                  n_clips, n_thresholds);
    hipLaunchKernelGGL(sweep_thresholds_kernel, dim3(unsigned(blocks)), dim3(64 * WPB), 0, static_cast<hipStream_t>(stream),
                       d_smoothed, d_window_offsets, n_clips, n_windows, d_thresholds, n_thresholds, groups, gap, d_counts,
                       d_first_window, d_peak_conf, d_peak_window);
    COUGH_HIP_CHECK(hipGetLastError());
    return COUGH_OK;
}

extern "C" int cough_list_events(const double* d_smoothed, const long long* d_window_offsets, int n_clips,
                                 long long n_windows, double threshold, int gap, const long long* d_event_offsets,
                                 long long n_events, int* d_event_window, double* d_event_conf, void* stream) {
    using namespace cough;
    const char* fn = "cough_list_events";
    COUGH_REQUIRE(d_smoothed && d_window_offsets && d_event_offsets && d_event_window && d_event_conf, COUGH_EINVAL,
                  "%s: NULL argument", fn);
    COUGH_REQUIRE(n_clips >= 0, COUGH_EINVAL, "%s: n_clips must not be negative, got %d", fn, n_clips);
    COUGH_REQUIRE(n_windows >= 0 && n_windows < MAX_WINDOWS, COUGH_EINVAL, "%s: n_windows = %lld (0..2^38 - 1)", fn,
                  n_windows);
    COUGH_REQUIRE(n_events >= 0, COUGH_EINVAL, "%s: n_events must not be negative, got %lld", fn, n_events);
    COUGH_REQUIRE(threshold == threshold, COUGH_EINVAL, "%s: threshold must not be NaN", fn);
    COUGH_REQUIRE(gap >= 1, COUGH_EINVAL, "%s: gap must be positive, got %d", fn, gap);
    COUGH_REQUIRE(aligned(d_event_window, 4), COUGH_EINVAL, "%s: int32 arrays must be 4-byte aligned", fn);
    COUGH_REQUIRE(aligned(d_smoothed, 8) && aligned(d_window_offsets, 8) && aligned(d_event_offsets, 8) &&
                  aligned(d_event_conf, 8), COUGH_EINVAL, "%s: int64 and float64 arrays must be 8-byte aligned", fn);
    if (n_clips == 0 || n_events == 0) return COUGH_OK;
    hipLaunchKernelGGL(list_events_kernel, dim3(unsigned((n_clips + WPB - 1) / WPB)), dim3(64 * WPB), 0,
                       static_cast<hipStream_t>(stream), d_smoothed, d_window_offsets, n_clips, n_windows, threshold, gap,
                       d_event_offsets, n_events, d_event_window, d_event_conf);
    COUGH_HIP_CHECK(hipGetLastError());
    return COUGH_OK;
}
