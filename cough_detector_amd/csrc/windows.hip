// libcough_amd_windows.so: a batch of training windows composed in one launch (include/cough_amd_windows.h).
// One kernel:
//
// compose_windows_kernel   one workgroup of 256 threads per row.  Thread t owns the samples t, t + 256, ... of the row:
//     consecutive lanes on consecutive samples for every stream, and the order cough_span_power sums in.  First pass: the
//     background, read through a cyclic index per thread (it advances by 256 mod length with one conditional subtraction:
//     no modulo per sample), squared and summed in float64; a butterfly inside each wave and (w0 + w1) + (w2 + w3)
//     through LDS give P_bg.  Threads 0 .. 3 then work out one gain each (scenes.hip's expression) and hand them round
//     through LDS.  Second pass: bg_gain * b, one fmaf per event that covers the sample, in index order, and the store.
//     KEEP (width <= 16384, at most 64 samples per thread) holds the first pass's samples in registers, so the background
//     crosses HBM once; without it the second pass walks the cyclic index again.  An event is tested per stretch of 256
//     samples first (the same in every lane), so a stretch no event meets costs no per-lane compare.
#include "../../include/cough_amd_windows.h"

#include <cmath>
#include <cstdint>

#include "common.h"

namespace cough {

namespace {

constexpr int WT = COUGH_WINDOWS_THREADS;
constexpr int MAX_EV = COUGH_WINDOWS_MAX_EVENTS;
constexpr int KEEP_WIDTH = COUGH_WINDOWS_KEEP_WIDTH;
constexpr int KEEP = KEEP_WIDTH / WT;                 // samples per thread that stay in registers
static_assert(WT == 256, "the order of the power sum is cough_span_power's: 256 threads");
static_assert(sizeof(cough_window_plan) == 80 && alignof(cough_window_plan) == 8, "the plan's layout is part of the ABI");

__device__ __forceinline__ long long clampll(long long v, long long lo, long long hi) { return min(max(v, lo), hi); }

struct ComposeArgs {
    const float* bg;
    long long n_bg;
    const long long* bg_offsets;
    const int* bg_lengths;
    int n_bg_clips;
    const float* ev;
    long long n_ev;
    const long long* ev_offsets;
    const int* ev_lengths;
    const double* p_ev;
    int n_ev_clips;
    const cough_window_plan* plans;
    int width;
    float* out;
    double* p_bg_out;
    float* gains_out;
};

// One event of a row as the second pass needs it; the same in every lane.  It covers the samples lo <= i < hi of the row
// (already cut to the row); sample i reads x[i - onset].
struct Event {
    const float* x;
    int onset, lo, hi;
    float gain;
};

template <bool KEPT>
__global__ __launch_bounds__(WT) void compose_windows_kernel(const ComposeArgs a) {
    __shared__ double wave_sums[WT / 64];
    __shared__ float gains[MAX_EV];
    const int r = blockIdx.x, tid = threadIdx.x, width = a.width;
    // the plan is read where it is used, field by field: every field is the same in every lane, and slot `tid` of the gains
    // is a load of its own (a copy of the record indexed by a lane would live in scratch)
    const cough_window_plan* plan = a.plans + r;
    const int background = plan->background, bg_start = plan->bg_start;
    const float bg_gain = plan->bg_gain;

    // the background: a clip outside its bank, -1 among them, or one whose clamped length is 0 is silence
    const float* b = nullptr;
    unsigned len = 0;
    if (background >= 0 && background < a.n_bg_clips) {
        const long long off = clampll(a.bg_offsets[background], 0, a.n_bg);
        len = unsigned(min((long long)max(a.bg_lengths[background], 0), a.n_bg - off));
        b = a.bg + off;
    }
    const unsigned first = len ? unsigned(((unsigned long long)max(bg_start, 0) + tid) % len) : 0u;
    const unsigned step = len ? WT % len : 0u;         // idx + step < 2 * len <= 2^32 - 2

    // ---- first pass: the power of the window's background, in cough_span_power's order
    float kept[KEPT ? KEEP : 1];
    double acc = 0.0;
    if (len) {
        unsigned idx = first;
        if constexpr (KEPT) {
#pragma unroll
            for (int j = 0; j < KEEP; ++j) {
                if (j * WT >= width) break;            // the same in every lane
                // the cyclic index is inside the clip whatever i is, so the load needs no guard and the loads of a thread
                // do not wait for each other; a sample past the row counts as +0.0, which leaves the sum as it is
                const float x = b[idx];
                kept[j] = x;
                const double v = j * WT + tid < width ? double(x) : 0.0;
                acc += v * v;                          // the square is exact, fused or not
                idx += step;
                if (idx >= len) idx -= len;
            }
        } else {
            for (int i = tid; i < width; i += WT) {
                const double v = double(b[idx]);
                acc += v * v;
                idx += step;
                if (idx >= len) idx -= len;
            }
        }
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) acc += __shfl_xor(acc, m, 64);
    if ((tid & 63) == 0) wave_sums[tid >> 6] = acc;
    __syncthreads();
    const double p_bg = len ? ((wave_sums[0] + wave_sums[1]) + (wave_sums[2] + wave_sums[3])) / double(width) : 0.0;

    // ---- the gains: thread e works out slot e
    const int n_events = min(max(plan->n_events, 0), MAX_EV);
    if (tid < MAX_EV) {
        float g = 0.0f;
        if (tid < n_events) {
            g = 1.0f;
            const int c = plan->clip[tid];
            if (c >= 0 && c < a.n_ev_clips) {
                const double pe = a.p_ev[c];
                if (p_bg != 0.0 && isfinite(p_bg) && pe != 0.0 && isfinite(pe)) {
                    const double bgain = double(bg_gain);
                    g = float(sqrt(((plan->snr_linear[tid] * (bgain * bgain)) * p_bg) / pe));
                }
            }
        }
        gains[tid] = g;
        if (a.gains_out) a.gains_out[(long long)r * MAX_EV + tid] = g;
    }
    if (tid == 0 && a.p_bg_out) a.p_bg_out[r] = p_bg;
    __syncthreads();

    // the events that meet the row, in index order
    Event events[MAX_EV];
    int n_live = 0;
#pragma unroll
    for (int e = 0; e < MAX_EV; ++e) {
        events[e] = Event{nullptr, 0, 0, 0, 0.0f};
        if (e < n_events) {
            const int c = plan->clip[e];
            if (c >= 0 && c < a.n_ev_clips) {
                const long long off = clampll(a.ev_offsets[c], 0, a.n_ev);
                const long long n = min((long long)max(a.ev_lengths[c], 0), a.n_ev - off);
                const long long lo = max((long long)plan->onset[e], 0LL), hi = min((long long)plan->onset[e] + n, (long long)width);
                if (lo < hi) {
                    events[e] = Event{a.ev + off, plan->onset[e], int(lo), int(hi), gains[e]};
                    ++n_live;
                }
            }
        }
    }

    // ---- second pass: the mix
    float* out = a.out + (long long)r * width;
    auto mix = [&](int i0, float x) {                  // sample i0 + tid of the row; i0 is the same in every lane
        const int i = i0 + tid;
        float v = len ? bg_gain * x : 0.0f;
        if (n_live) {
#pragma unroll
            for (int e = 0; e < MAX_EV; ++e) {
                const Event& ev = events[e];
                if (ev.lo < i0 + WT && ev.hi > i0) {   // the stretch meets the event: the same in every lane
                    // i - onset < n <= n_ev - off: inside the bank; it does not overflow, lo <= i < hi <= onset + n
                    if (i >= ev.lo && i < ev.hi) v = fmaf(ev.gain, ev.x[(long long)i - ev.onset], v);
                }
            }
        }
        if (i < width) out[i] = v;
    };
    if constexpr (KEPT) {
#pragma unroll
        for (int j = 0; j < KEEP; ++j) {
            if (j * WT >= width) break;
            mix(j * WT, len ? kept[j] : 0.0f);
        }
    } else {
        unsigned idx = first;
        for (int i0 = 0; i0 < width; i0 += WT) {
            float x = 0.0f;
            if (len && i0 + tid < width) {
                x = b[idx];
                idx += step;
                if (idx >= len) idx -= len;
            }
            mix(i0, x);
        }
    }
}

// [p, p + n) and [q, q + m) share a byte
inline bool overlaps(const void* p, long long n, const void* q, long long m) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return p && q && n > 0 && m > 0 && a < b + uintptr_t(m) && b < a + uintptr_t(n);
}

}  // namespace
}  // namespace cough

extern "C" int cough_windows_abi_version(void) { return COUGH_WINDOWS_ABI_VERSION; }
// this library's own last-error slot
COUGH_DEFINE_LAST_ERROR(cough_windows_last_error)

extern "C" int cough_compose_windows(const float* d_bg, long long n_bg_samples, const long long* d_bg_offsets,
                                     const int* d_bg_lengths, int n_bg_clips, const float* d_ev, long long n_ev_samples,
                                     const long long* d_ev_offsets, const int* d_ev_lengths, const double* d_p_ev,
                                     int n_event_clips, const cough_window_plan* d_plans, int n_rows, int width,
                                     float* d_out, double* d_p_bg_out, float* d_gains_out, void* stream) {
    using namespace cough;
    const char* fn = "cough_compose_windows";
    COUGH_REQUIRE(n_rows >= 0 && n_bg_clips >= 0 && n_event_clips >= 0, COUGH_EINVAL,
                  "%s: n_rows = %d, n_bg_clips = %d, n_event_clips = %d must not be negative", fn, n_rows, n_bg_clips,
                  n_event_clips);
    COUGH_REQUIRE(n_bg_samples >= 0 && n_ev_samples >= 0, COUGH_EINVAL,
                  "%s: n_bg_samples = %lld, n_ev_samples = %lld must not be negative", fn, n_bg_samples, n_ev_samples);
    COUGH_REQUIRE(width >= 1 && width <= COUGH_WINDOWS_MAX_WIDTH, COUGH_EINVAL, "%s: width = %d (1..%d)", fn, width,
                  COUGH_WINDOWS_MAX_WIDTH);
    if (n_rows == 0) return COUGH_OK;
    COUGH_REQUIRE(d_plans && d_out, COUGH_EINVAL, "%s: NULL argument", fn);
    COUGH_REQUIRE(n_bg_clips == 0 || (d_bg_offsets && d_bg_lengths), COUGH_EINVAL,
                  "%s: NULL background tables with n_bg_clips = %d", fn, n_bg_clips);
    COUGH_REQUIRE(d_bg || n_bg_samples == 0, COUGH_EINVAL, "%s: d_bg is NULL", fn);
    COUGH_REQUIRE(n_event_clips == 0 || (d_ev_offsets && d_ev_lengths && d_p_ev), COUGH_EINVAL,
                  "%s: NULL event tables with n_event_clips = %d", fn, n_event_clips);
    COUGH_REQUIRE(d_ev || n_ev_samples == 0, COUGH_EINVAL, "%s: d_ev is NULL", fn);
    COUGH_REQUIRE(aligned(d_bg, 4) && aligned(d_ev, 4) && aligned(d_out, 4) && aligned(d_bg_lengths, 4) &&
                  aligned(d_ev_lengths, 4) && aligned(d_gains_out, 4), COUGH_EINVAL,
                  "%s: float32 and int32 arrays must be 4-byte aligned", fn);
    COUGH_REQUIRE(aligned(d_bg_offsets, 8) && aligned(d_ev_offsets, 8) && aligned(d_p_ev, 8) && aligned(d_plans, 8) &&
                  aligned(d_p_bg_out, 8), COUGH_EINVAL, "%s: int64 and float64 arrays and the plans must be 8-byte aligned", fn);
    const long long out_bytes = (long long)n_rows * width * 4;
    COUGH_REQUIRE(!overlaps(d_out, out_bytes, d_bg, n_bg_samples * 4) && !overlaps(d_out, out_bytes, d_ev, n_ev_samples * 4),
                  COUGH_EINVAL, "%s: d_out overlaps a bank", fn);
    const ComposeArgs a{d_bg, n_bg_samples, d_bg_offsets, d_bg_lengths, n_bg_clips, d_ev, n_ev_samples, d_ev_offsets,
                        d_ev_lengths, d_p_ev, n_event_clips, d_plans, width, d_out, d_p_bg_out, d_gains_out};
    if (width <= KEEP_WIDTH)
        hipLaunchKernelGGL(compose_windows_kernel<true>, dim3(unsigned(n_rows)), dim3(WT), 0, static_cast<hipStream_t>(stream), a);
    else
        hipLaunchKernelGGL(compose_windows_kernel<false>, dim3(unsigned(n_rows)), dim3(WT), 0, static_cast<hipStream_t>(stream), a);
    COUGH_HIP_CHECK(hipGetLastError());
    return COUGH_OK;
}
