// libcough_amd_scenes.so: soundscapes with known cough times and event-level scoring (include/cough_amd_scenes.h).
// Five kernels:
//
// span_power_kernel    one workgroup per span: thread t adds double(x)^2 of the samples t, t + 256, ... of a cyclic read of
//     its clip (the cyclic index advances by 256 mod length with one conditional subtraction: no modulo per sample), then
//     a butterfly inside each wave and (w0 + w1) + (w2 + w3) through LDS.  The order depends on the span alone.
// scene_gains_kernel   one thread per event: the SNR rule in float64, rounded to float32 once.
// mix_scenes_kernel    the kernel with the bytes: one workgroup per (scene, tile of COUGH_SCENES_TILE samples).  The tile is
//     accumulated in LDS, laid out with the 16-byte phase of its place in the output: the background goes in as
//     bg_gain * b, split at the wrap points of the cyclic read (a background under 1024 samples, which would wrap many
//     times per tile, through a cyclic index per thread instead); every event that meets the tile (the first one by a
//     binary search of the scene's onsets, uniform across the workgroup) is added with one fmaf per sample; the tile
//     then leaves with 16-byte LDS reads and 16-byte stores.  Each of the three streams is moved with 16-byte global
//     accesses from the first 16-byte boundary of its own pointer on (stream_in), so every combination of 4-byte phases
//     takes the same path.  HBM traffic: the scene's samples in, the event samples in, the scene's samples out.
// match_events_kernel  sweep_thresholds_kernel's walk (score_walk.h), one wave per (recording, 64 thresholds); a lane that
//     fires classifies the window with Matcher::classify, which walks the recording's truth events by a pointer.
// list_matches_kernel  the same at one threshold, one thread per recording.
#include "../../include/cough_amd_scenes.h"

#include <climits>
#include <cmath>
#include <cstdint>

#include "common.h"
#include "score_walk.h"

namespace cough {

namespace {

constexpr int PT = 256;                               // threads of the power kernel: the order of its sum is tied to it
constexpr int GT = 256;                               // threads of the gains kernel
constexpr int MT = 256;                               // threads of the mix kernel
constexpr int TILE = COUGH_SCENES_TILE;
constexpr int SHORT_BG = 1024;                        // backgrounds shorter than this take the per-thread cyclic index
constexpr int WPB = 4;                                // waves per workgroup of the matcher
constexpr int LT = 64;                                // threads of the list kernel
constexpr long long MAX_WINDOWS = 1LL << 38;

__device__ __forceinline__ long long clampll(long long v, long long lo, long long hi) { return min(max(v, lo), hi); }

// ------------------------------------------------------------------------------------------ span power
__global__ __launch_bounds__(PT) void span_power_kernel(const float* __restrict__ bank, long long n_bank,
                                                        const long long* __restrict__ offs, const int* __restrict__ lens,
                                                        const int* __restrict__ starts, const int* __restrict__ spans,
                                                        double* __restrict__ power) {
    __shared__ double wave_sums[PT / 64];
    const int r = blockIdx.x, tid = threadIdx.x;
    const long long off = clampll(offs[r], 0, n_bank);
    const unsigned len = unsigned(min((long long)max(lens[r], 0), n_bank - off));
    const int n = max(spans[r], 0);
    if (len == 0 || n == 0) {                          // the whole workgroup
        if (tid == 0) power[r] = 0.0;
        return;
    }
    const float* x = bank + off;
    unsigned idx = unsigned(((unsigned long long)max(starts[r], 0) + tid) % len);
    const unsigned step = PT % len;                    // idx + step < 2 * len <= 2^32 - 2
    double acc = 0.0;
    for (int i = tid; i < n; i += PT) {
        const double v = double(x[idx]);
        acc += v * v;                                  // the square is exact, fused or not
        idx += step;
        if (idx >= len) idx -= len;
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) acc += __shfl_xor(acc, m, 64);
    if ((tid & 63) == 0) wave_sums[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) power[r] = ((wave_sums[0] + wave_sums[1]) + (wave_sums[2] + wave_sums[3])) / double(n);
}

// ------------------------------------------------------------------------------------------ gains
__global__ __launch_bounds__(GT) void scene_gains_kernel(const double* __restrict__ p_bg, const float* __restrict__ bg_gain,
                                                         int n_scenes, const double* __restrict__ p_ev, int n_powers,
                                                         const int* __restrict__ event_scene,
                                                         const int* __restrict__ event_power,
                                                         const double* __restrict__ snr_linear, int n_events,
                                                         float* __restrict__ gain) {
    const int e = blockIdx.x * GT + threadIdx.x;
    if (e >= n_events) return;
    const int s = event_scene[e], q = event_power[e];
    float g = 1.0f;
    if (s >= 0 && s < n_scenes && q >= 0 && q < n_powers) {
        const double pb = p_bg[s], pe = p_ev[q];
        if (pb != 0.0 && isfinite(pb) && pe != 0.0 && isfinite(pe)) {
            const double b = double(bg_gain[s]);
            g = float(sqrt(((snr_linear[e] * (b * b)) * pb) / pe));
        }
    }
    gain[e] = g;
}

// ------------------------------------------------------------------------------------------ the mix
struct MixArgs {
    const float* bg;
    long long n_bg;
    const long long* bg_offsets;
    const int* bg_lengths;
    const int* bg_starts;
    const float* bg_gains;
    const int* scene_lengths;
    const long long* out_offsets;
    const long long* ev_offsets;
    int n_scenes;
    const float* ev;
    long long n_ev;
    const long long* src_offsets;
    const int* src_lengths;
    const int* onsets;
    const float* gains;
    int n_events;
    const int* tiles;
    float* out;
    long long n_out;
};

// f(j, g[j]) for j = 0 .. n - 1, by the whole workgroup: single samples up to g's first 16-byte boundary, 16-byte loads
// from there, single samples for what is left
template <class F>
__device__ __forceinline__ void stream_in(const float* __restrict__ g, int n, F f) {
    const int tid = threadIdx.x;
    const int head = min(n, int((4 - ((reinterpret_cast<uintptr_t>(g) >> 2) & 3)) & 3));
    if (tid < head) f(tid, g[tid]);
    const float4* g4 = reinterpret_cast<const float4*>(g + head);
    const int n4 = (n - head) >> 2;
#pragma unroll 4
    for (int q = tid; q < n4; q += MT) {
        const float4 v = g4[q];
        const int j = head + 4 * q;
        f(j, v.x);
        f(j + 1, v.y);
        f(j + 2, v.z);
        f(j + 3, v.w);
    }
    const int done = head + 4 * n4;
    if (tid < n - done) f(done + tid, g[done + tid]);
}

__global__ __launch_bounds__(MT) void mix_scenes_kernel(const MixArgs a) {
    __shared__ __attribute__((aligned(16))) float acc[TILE + 4];
    const int tid = threadIdx.x;
    const int s = a.tiles[2 * blockIdx.x], i0 = a.tiles[2 * blockIdx.x + 1];
    if (s < 0 || s >= a.n_scenes || i0 < 0) return;   // everything up to the output is the same in every lane
    const long long oo = a.out_offsets[s];
    if (oo < 0 || oo > a.n_out) return;
    const long long L = min((long long)max(a.scene_lengths[s], 0), a.n_out - oo);
    if (i0 >= L) return;
    const int n = int(min((long long)TILE, L - i0));
    float* out = a.out + oo + i0;
    // acc[pad + j] is sample i0 + j: the tile lies in LDS with the 16-byte phase it has in the output
    const int pad = int((reinterpret_cast<uintptr_t>(out) >> 2) & 3);

    // the background, cyclic: one modulo per tile, then whole stretches up to each wrap point
    const long long bo = clampll(a.bg_offsets[s], 0, a.n_bg);
    const long long bl = min((long long)max(a.bg_lengths[s], 0), a.n_bg - bo);
    if (bl == 0) {
        for (int j = tid; j < n; j += MT) acc[pad + j] = 0.0f;
    } else if (bl < SHORT_BG) {
        // a short noise sample wraps many times inside the tile: stretches of a few samples would leave most lanes idle, so
        // every thread keeps a cyclic index of its own (it advances by MT mod length: no modulo per sample).  The clip
        // stays in cache; the loads are 4 bytes wide
        const float g = a.bg_gains[s];
        const float* b = a.bg + bo;
        const unsigned len = unsigned(bl);
        unsigned idx = unsigned(((long long)max(a.bg_starts[s], 0) + i0 + tid) % bl);
        const unsigned step = MT % len;
        for (int j = tid; j < n; j += MT) {
            acc[pad + j] = g * b[idx];
            idx += step;
            if (idx >= len) idx -= len;
        }
    } else {
        const float g = a.bg_gains[s];
        const float* b = a.bg + bo;
        long long p = ((long long)max(a.bg_starts[s], 0) + i0) % bl;
        for (int j = 0; j < n;) {
            const int seg = int(min((long long)(n - j), bl - p));
            stream_in(b + p, seg, [&](int q, float v) { acc[pad + j + q] = g * v; });
            j += seg;
            p = 0;
        }
    }
    __syncthreads();

    // the events: the first one that ends after i0, then on while they start inside the tile
    const long long e_lo = clampll(a.ev_offsets[s], 0, a.n_events);
    const long long e_hi = clampll(a.ev_offsets[s + 1], e_lo, a.n_events);
    long long lo = e_lo, hi = e_hi;
    while (lo < hi) {
        const long long mid = lo + (hi - lo) / 2;
        if ((long long)a.onsets[mid] + max(a.src_lengths[mid], 0) > i0) hi = mid; else lo = mid + 1;
    }
    for (long long e = lo; e < e_hi; ++e) {
        const long long on = a.onsets[e];
        if (on >= (long long)i0 + n) break;
        const long long so = clampll(a.src_offsets[e], 0, a.n_ev);
        const long long sl = min((long long)max(a.src_lengths[e], 0), a.n_ev - so);
        const long long from = max(on, (long long)i0), to = min(on + sl, (long long)i0 + n);
        if (from < to) {
            const float g = a.gains[e];
            const int at = pad + int(from - i0);
            stream_in(a.ev + so + (from - on), int(to - from), [&](int q, float v) { acc[at + q] = fmaf(g, v, acc[at + q]); });
        }
        __syncthreads();                               // overlapping events (the caller's fault) still add one after another
    }

    // out: 16-byte LDS reads and stores from the output's first 16-byte boundary on
    const int head = min(n, (4 - pad) & 3);
    if (tid < head) out[tid] = acc[pad + tid];
    const int n4 = (n - head) >> 2;
    float4* o4 = reinterpret_cast<float4*>(out + head);
    const float4* a4 = reinterpret_cast<const float4*>(acc + pad + head);
#pragma unroll 4
    for (int q = tid; q < n4; q += MT) o4[q] = a4[q];
    const int done = head + 4 * n4;
    if (tid < n - done) out[done + tid] = acc[pad + done + tid];
}

// ------------------------------------------------------------------------------------------ the matcher
// The truth events of one recording, [.., t_hi) of k_lo / k_hi, met by the firing windows of one walk in time order.
struct Matcher {
    long long ptr;                                     // the first event after the last one hit that may still hold a window
    long long last;                                    // the last event hit, -1 before the first
    // 0: window k hits event `last` (just set); 1: a repeat of `last`; 2: a false alarm
    __device__ __forceinline__ int classify(int k, const int* __restrict__ k_lo, const int* __restrict__ k_hi, long long t_hi) {
        while (ptr < t_hi && k_hi[ptr] < k) ++ptr;
        if (ptr < t_hi && k_lo[ptr] <= k) {
            last = ptr++;
            return 0;
        }
        return last >= 0 && k <= k_hi[last] ? 1 : 2;
    }
};

__device__ __forceinline__ void truth_range(const long long* __restrict__ offs, int c, int n_truth, long long& lo, long long& hi) {
    lo = clampll(offs[c], 0, n_truth);
    hi = clampll(offs[c + 1], lo, n_truth);
}

__global__ __launch_bounds__(64 * WPB) void match_events_kernel(
    const double* __restrict__ smoothed, const long long* __restrict__ offs, int n_clips, long long n_windows,
    const double* __restrict__ thresholds, int n_thr, int groups, int gap, const long long* __restrict__ truth_offs,
    const int* __restrict__ k_lo, const int* __restrict__ k_hi, const int* __restrict__ onset, int n_truth, int hop,
    int window, int* __restrict__ hits, int* __restrict__ false_alarms, int* __restrict__ repeats,
    long long* __restrict__ latency) {
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * WPB + (threadIdx.x >> 6);
    if (wave >= (long long)n_clips * groups) return;   // a whole wave
    const int c = int(wave / groups), g = int(wave % groups);
    long long w0;
    int n;
    clip_windows(offs, c, n_windows, w0, n);
    const double* s = smoothed + w0;
    long long t_lo, t_hi;
    truth_range(truth_offs, c, n_truth, t_lo, t_hi);
    const int t = g * 64 + lane;
    const bool mine = t < n_thr;
    const double thr = mine ? thresholds[t] : 0.0;

    Matcher m{t_lo, -1};
    long long next = 0, late = 0;
    int n_hit = 0, n_repeat = 0, n_false = 0;
    for (int base = 0; base < n; base += 64) {
        const int k_mine = base + lane;
        const double v = k_mine < n ? s[k_mine] : 0.0;
        const int cnt = min(64, n - base);
        for (int j = 0; j < cnt; ++j) {
            const double sv = read_lane(v, j);
            const int k = base + j;
            if (walk_fires(sv, thr, k, next)) {
                next = walk_advance(k, gap);
                const int cls = m.classify(k, k_lo, k_hi, t_hi);
                if (cls == 0) {
                    ++n_hit;
                    late += (long long)k * hop + window - onset[m.last];
                } else if (cls == 1) {
                    ++n_repeat;
                } else {
                    ++n_false;
                }
            }
        }
    }
    if (mine) {
        const long long o = (long long)c * n_thr + t;
        if (hits) hits[o] = n_hit;
        if (false_alarms) false_alarms[o] = n_false;
        if (repeats) repeats[o] = n_repeat;
        if (latency) latency[o] = late;
    }
}

__global__ __launch_bounds__(LT) void list_matches_kernel(const double* __restrict__ smoothed, const long long* __restrict__ offs,
                                                          int n_clips, long long n_windows, double thr, int gap,
                                                          const long long* __restrict__ truth_offs, const int* __restrict__ k_lo,
                                                          const int* __restrict__ k_hi, int n_truth,
                                                          int* __restrict__ truth_window, const long long* __restrict__ event_offs,
                                                          long long n_events, int* __restrict__ event_class) {
    const int c = blockIdx.x * LT + threadIdx.x;
    if (c >= n_clips) return;
    long long w0;
    int n;
    clip_windows(offs, c, n_windows, w0, n);
    const double* s = smoothed + w0;
    long long t_lo, t_hi;
    truth_range(truth_offs, c, n_truth, t_lo, t_hi);
    for (long long j = t_lo; j < t_hi; ++j) truth_window[j] = -1;
    long long e0 = 0, room = 0;
    if (event_class) {
        e0 = clampll(event_offs[c], 0, n_events);
        room = clampll(event_offs[c + 1], e0, n_events) - e0;
    }
    Matcher m{t_lo, -1};
    long long next = 0, count = 0;
    for (int k = 0; k < n; ++k) {
        if (walk_fires(s[k], thr, k, next)) {
            next = walk_advance(k, gap);
            const int cls = m.classify(k, k_lo, k_hi, t_hi);
            if (cls == 0) truth_window[m.last] = k;
            if (count < room) event_class[e0 + count] = cls;
            ++count;
        }
    }
}

}  // namespace
}  // namespace cough

extern "C" int cough_scenes_abi_version(void) { return COUGH_SCENES_ABI_VERSION; }
// this library's own last-error slot
COUGH_DEFINE_LAST_ERROR(cough_scenes_last_error)

extern "C" int cough_span_power(const float* d_bank, long long n_bank_samples, const long long* d_clip_offsets,
                                const int* d_clip_lengths, const int* d_starts, const int* d_span_lengths, int n,
                                double* d_power, void* stream) {
    using namespace cough;
    const char* fn = "cough_span_power";
    COUGH_REQUIRE(n >= 0, COUGH_EINVAL, "%s: n must not be negative, got %d", fn, n);
    COUGH_REQUIRE(n_bank_samples >= 0, COUGH_EINVAL, "%s: n_bank_samples must not be negative, got %lld", fn, n_bank_samples);
    COUGH_REQUIRE(d_clip_offsets && d_clip_lengths && d_starts && d_span_lengths && d_power, COUGH_EINVAL,
                  "%s: NULL argument", fn);
    COUGH_REQUIRE(d_bank || n_bank_samples == 0, COUGH_EINVAL, "%s: d_bank is NULL", fn);
    COUGH_REQUIRE(aligned(d_bank, 4) && aligned(d_clip_lengths, 4) && aligned(d_starts, 4) && aligned(d_span_lengths, 4),
                  COUGH_EINVAL, "%s: float32 and int32 arrays must be 4-byte aligned", fn);
    COUGH_REQUIRE(aligned(d_clip_offsets, 8) && aligned(d_power, 8), COUGH_EINVAL,
                  "%s: int64 and float64 arrays must be 8-byte aligned", fn);
    if (n == 0) return COUGH_OK;
    hipLaunchKernelGGL(span_power_kernel, dim3(unsigned(n)), dim3(PT), 0, static_cast<hipStream_t>(stream), d_bank,
                       n_bank_samples, d_clip_offsets, d_clip_lengths, d_starts, d_span_lengths, d_power);
    COUGH_HIP_CHECK(hipGetLastError());
    return COUGH_OK;
}

extern "C" int cough_scene_gains(const double* d_p_bg, const float* d_bg_gain, int n_scenes, const double* d_p_ev, int n_powers,
                                 const int* d_event_scene, const int* d_event_power, const double* d_snr_linear,
                                 int n_events, float* d_gain, void* stream) {
    using namespace cough;
    const char* fn = "cough_scene_gains";
    COUGH_REQUIRE(n_scenes >= 0 && n_powers >= 0 && n_events >= 0, COUGH_EINVAL,
                  "%s: n_scenes = %d, n_powers = %d, n_events = %d must not be negative", fn, n_scenes, n_powers, n_events);
    if (n_events == 0) return COUGH_OK;
    COUGH_REQUIRE(d_event_scene && d_event_power && d_snr_linear && d_gain, COUGH_EINVAL, "%s: NULL argument", fn);
    COUGH_REQUIRE((d_p_bg && d_bg_gain) || n_scenes == 0, COUGH_EINVAL, "%s: NULL scene arrays", fn);
    COUGH_REQUIRE(d_p_ev || n_powers == 0, COUGH_EINVAL, "%s: d_p_ev is NULL", fn);
    COUGH_REQUIRE(aligned(d_bg_gain, 4) && aligned(d_event_scene, 4) && aligned(d_event_power, 4) && aligned(d_gain, 4),
                  COUGH_EINVAL, "%s: float32 and int32 arrays must be 4-byte aligned", fn);
    COUGH_REQUIRE(aligned(d_p_bg, 8) && aligned(d_p_ev, 8) && aligned(d_snr_linear, 8), COUGH_EINVAL,
                  "%s: float64 arrays must be 8-byte aligned", fn);
    hipLaunchKernelGGL(scene_gains_kernel, dim3(unsigned((n_events + GT - 1) / GT)), dim3(GT), 0,
                       static_cast<hipStream_t>(stream), d_p_bg, d_bg_gain, n_scenes, d_p_ev, n_powers, d_event_scene,
                       d_event_power, d_snr_linear, n_events, d_gain);
    COUGH_HIP_CHECK(hipGetLastError());
    return COUGH_OK;
}

extern "C" int cough_mix_scenes(const float* d_bg, long long n_bg_samples, const long long* d_bg_offsets,
                                const int* d_bg_lengths, const int* d_bg_starts, const float* d_bg_gains,
                                const int* d_scene_lengths, const long long* d_out_offsets, const long long* d_ev_offsets,
                                int n_scenes, const float* d_ev, long long n_ev_samples, const long long* d_src_offsets,
                                const int* d_src_lengths, const int* d_onsets, const float* d_gains, int n_events,
                                const int* d_tiles, int n_tiles, float* d_out, long long n_out_samples, void* stream) {
    using namespace cough;
    const char* fn = "cough_mix_scenes";
    COUGH_REQUIRE(n_scenes >= 0 && n_events >= 0 && n_tiles >= 0, COUGH_EINVAL,
                  "%s: n_scenes = %d, n_events = %d, n_tiles = %d must not be negative", fn, n_scenes, n_events, n_tiles);
    COUGH_REQUIRE(n_bg_samples >= 0 && n_ev_samples >= 0 && n_out_samples >= 0, COUGH_EINVAL,
                  "%s: n_bg_samples = %lld, n_ev_samples = %lld, n_out_samples = %lld must not be negative", fn, n_bg_samples,
                  n_ev_samples, n_out_samples);
    if (n_scenes == 0 || n_tiles == 0) return COUGH_OK;
    COUGH_REQUIRE(d_bg_offsets && d_bg_lengths && d_bg_starts && d_bg_gains && d_scene_lengths && d_out_offsets &&
                  d_ev_offsets && d_tiles, COUGH_EINVAL, "%s: NULL argument", fn);
    COUGH_REQUIRE(d_bg || n_bg_samples == 0, COUGH_EINVAL, "%s: d_bg is NULL", fn);
    COUGH_REQUIRE(d_out || n_out_samples == 0, COUGH_EINVAL, "%s: d_out is NULL", fn);
    COUGH_REQUIRE(n_events == 0 || (d_src_offsets && d_src_lengths && d_onsets && d_gains), COUGH_EINVAL,
                  "%s: NULL event arrays with n_events = %d", fn, n_events);
    COUGH_REQUIRE(d_ev || n_ev_samples == 0, COUGH_EINVAL, "%s: d_ev is NULL", fn);
    COUGH_REQUIRE(aligned(d_bg, 4) && aligned(d_ev, 4) && aligned(d_out, 4) && aligned(d_bg_lengths, 4) &&
                  aligned(d_bg_starts, 4) && aligned(d_bg_gains, 4) && aligned(d_scene_lengths, 4) &&
                  aligned(d_src_lengths, 4) && aligned(d_onsets, 4) && aligned(d_gains, 4) && aligned(d_tiles, 4),
                  COUGH_EINVAL, "%s: float32 and int32 arrays must be 4-byte aligned", fn);
    COUGH_REQUIRE(aligned(d_bg_offsets, 8) && aligned(d_out_offsets, 8) && aligned(d_ev_offsets, 8) &&
                  aligned(d_src_offsets, 8), COUGH_EINVAL, "%s: int64 arrays must be 8-byte aligned", fn);
    const MixArgs a{d_bg, n_bg_samples, d_bg_offsets, d_bg_lengths, d_bg_starts, d_bg_gains, d_scene_lengths, d_out_offsets,
                    d_ev_offsets, n_scenes, d_ev, n_ev_samples, d_src_offsets, d_src_lengths, d_onsets, d_gains, n_events,
                    d_tiles, d_out, n_out_samples};
    hipLaunchKernelGGL(mix_scenes_kernel, dim3(unsigned(n_tiles)), dim3(MT), 0, static_cast<hipStream_t>(stream), a);
    COUGH_HIP_CHECK(hipGetLastError());
    return COUGH_OK;
}

namespace {
// what the two matching entry points check alike
int check_walk(const char* fn, const double* d_smoothed, const long long* d_window_offsets, int n_clips, long long n_windows,
               int gap, const long long* d_truth_offsets, const int* d_k_lo, const int* d_k_hi, int n_truth) {
    using namespace cough;
    COUGH_REQUIRE(n_clips >= 0, COUGH_EINVAL, "%s: n_clips must not be negative, got %d", fn, n_clips);
    COUGH_REQUIRE(n_windows >= 0 && n_windows < MAX_WINDOWS, COUGH_EINVAL, "%s: n_windows = %lld (0..2^38 - 1)", fn,
                  n_windows);
    COUGH_REQUIRE(n_truth >= 0, COUGH_EINVAL, "%s: n_truth must not be negative, got %d", fn, n_truth);
    COUGH_REQUIRE(gap >= 1, COUGH_EINVAL, "%s: gap must be positive, got %d", fn, gap);
    COUGH_REQUIRE(d_window_offsets && d_truth_offsets, COUGH_EINVAL, "%s: NULL argument", fn);
    COUGH_REQUIRE(d_smoothed || n_windows == 0, COUGH_EINVAL, "%s: d_smoothed is NULL", fn);
    COUGH_REQUIRE(n_truth == 0 || (d_k_lo && d_k_hi), COUGH_EINVAL, "%s: NULL truth arrays with n_truth = %d", fn, n_truth);
    COUGH_REQUIRE(aligned(d_k_lo, 4) && aligned(d_k_hi, 4), COUGH_EINVAL, "%s: int32 arrays must be 4-byte aligned", fn);
    COUGH_REQUIRE(aligned(d_smoothed, 8) && aligned(d_window_offsets, 8) && aligned(d_truth_offsets, 8), COUGH_EINVAL,
                  "%s: int64 and float64 arrays must be 8-byte aligned", fn);
    return COUGH_OK;
}
}  // namespace

extern "C" int cough_match_events(const double* d_smoothed, const long long* d_window_offsets, int n_clips, long long n_windows,
                                  const double* d_thresholds, int n_thresholds, int gap, const long long* d_truth_offsets,
                                  const int* d_k_lo, const int* d_k_hi, const int* d_onset, int n_truth, int hop, int window,
                                  int* d_hits, int* d_false_alarms, int* d_repeats, long long* d_latency_samples,
                                  void* stream) {
    using namespace cough;
    const char* fn = "cough_match_events";
    if (const int st = check_walk(fn, d_smoothed, d_window_offsets, n_clips, n_windows, gap, d_truth_offsets, d_k_lo, d_k_hi,
                                  n_truth))
        return st;
    COUGH_REQUIRE(d_thresholds, COUGH_EINVAL, "%s: NULL argument", fn);
    COUGH_REQUIRE(n_truth == 0 || d_onset, COUGH_EINVAL, "%s: d_onset is NULL with n_truth = %d", fn, n_truth);
    COUGH_REQUIRE(n_thresholds >= 1 && n_thresholds <= COUGH_SCENES_MAX_THRESHOLDS, COUGH_EINVAL,
                  "%s: n_thresholds = %d (1..%d)", fn, n_thresholds, COUGH_SCENES_MAX_THRESHOLDS);
    COUGH_REQUIRE(hop >= 1 && window >= 1, COUGH_EINVAL, "%s: hop = %d and window = %d must be positive", fn, hop, window);
    COUGH_REQUIRE(aligned(d_onset, 4) && aligned(d_hits, 4) && aligned(d_false_alarms, 4) && aligned(d_repeats, 4),
                  COUGH_EINVAL, "%s: int32 arrays must be 4-byte aligned", fn);
    COUGH_REQUIRE(aligned(d_thresholds, 8) && aligned(d_latency_samples, 8), COUGH_EINVAL,
                  "%s: int64 and float64 arrays must be 8-byte aligned", fn);
    if (n_clips == 0) return COUGH_OK;
    const int groups = (n_thresholds + 63) / 64;
    const long long blocks = ((long long)n_clips * groups + WPB - 1) / WPB;
    COUGH_REQUIRE(blocks <= INT_MAX, COUGH_EUNSUPPORTED, "%s: %d recordings x %d thresholds do not fit one launch", fn,
                  n_clips, n_thresholds);
    hipLaunchKernelGGL(match_events_kernel, dim3(unsigned(blocks)), dim3(64 * WPB), 0, static_cast<hipStream_t>(stream),
                       d_smoothed, d_window_offsets, n_clips, n_windows, d_thresholds, n_thresholds, groups, gap,
                       d_truth_offsets, d_k_lo, d_k_hi, d_onset, n_truth, hop, window, d_hits, d_false_alarms, d_repeats,
                       d_latency_samples);
    COUGH_HIP_CHECK(hipGetLastError());
    return COUGH_OK;
}

extern "C" int cough_list_event_matches(const double* d_smoothed, const long long* d_window_offsets, int n_clips, long long n_windows,
                                  double threshold, int gap, const long long* d_truth_offsets, const int* d_k_lo,
                                  const int* d_k_hi, int n_truth, int* d_truth_window, const long long* d_event_offsets,
                                  long long n_events, int* d_event_class, void* stream) {
    using namespace cough;
    const char* fn = "cough_list_event_matches";
    if (const int st = check_walk(fn, d_smoothed, d_window_offsets, n_clips, n_windows, gap, d_truth_offsets, d_k_lo, d_k_hi,
                                  n_truth))
        return st;
    COUGH_REQUIRE(threshold == threshold, COUGH_EINVAL, "%s: threshold must not be NaN", fn);
    COUGH_REQUIRE(n_events >= 0, COUGH_EINVAL, "%s: n_events must not be negative, got %lld", fn, n_events);
    COUGH_REQUIRE(n_truth == 0 || d_truth_window, COUGH_EINVAL, "%s: d_truth_window is NULL with n_truth = %d", fn, n_truth);
    COUGH_REQUIRE(!d_event_class || d_event_offsets, COUGH_EINVAL, "%s: d_event_class needs d_event_offsets", fn);
    COUGH_REQUIRE(aligned(d_truth_window, 4) && aligned(d_event_class, 4), COUGH_EINVAL,
                  "%s: int32 arrays must be 4-byte aligned", fn);
    COUGH_REQUIRE(aligned(d_event_offsets, 8), COUGH_EINVAL, "%s: int64 arrays must be 8-byte aligned", fn);
    if (n_clips == 0) return COUGH_OK;
    hipLaunchKernelGGL(list_matches_kernel, dim3(unsigned((n_clips + LT - 1) / LT)), dim3(LT), 0,
                       static_cast<hipStream_t>(stream), d_smoothed, d_window_offsets, n_clips, n_windows, threshold, gap,
                       d_truth_offsets, d_k_lo, d_k_hi, n_truth, d_truth_window, d_event_offsets, n_events,
                       n_events > 0 ? d_event_class : nullptr);
    COUGH_HIP_CHECK(hipGetLastError());
    return COUGH_OK;
}
