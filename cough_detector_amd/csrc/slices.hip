// libcough_amd_slices.so: fixed-length windows of long recordings and which of them hold enough active signal
// (include/cough_amd_slices.h, which states the arithmetic).  Two kernels, one wave per clip each.
//
// Window activity.  A window's active frames are a popcount over a range of activity bits, so the wave turns the clip's
// energies into bits once -- one ballot per 64 frames -- and every lane then answers one window with two LDS lookups.
// Nothing is sized by the clip: the wave marches over the frames in chunks of CF = 1024, keeps a chunk's CW ballot words
// and their running popcounts in LDS, and adds to m[w] what the chunk holds of window w's frames.  m[w] lives where it
// ends up anyway, in d_active: a window whose frames cross a chunk boundary (or that is longer than a chunk) is added to
// in place.  Window w is always handled by lane w % 64 -- in the zeroing, in every chunk and in every pass of the cap -- so
// each thread only ever reads back what it stored itself, in program order; no lane depends on seeing another lane's
// store.  The cap is a bisection on m (a wave count per round) and a ballot prefix over the windows of the threshold
// level, in time order.  Control flow is uniform throughout: every lane holds the same loop state.
#include "../../include/cough_amd_slices.h"

#include <cfloat>
#include <cmath>

#include "common.h"

namespace cough {

namespace {

constexpr int PW = 4;          // waves (clips) per workgroup
constexpr int CW = 16;         // ballot words of a chunk, word i in lane i (<= 64); a 10 s clip at 400 / 160 is one chunk
constexpr int CF = CW * 64;    // frames of a chunk
constexpr int LU = 4;          // energy loads a lane keeps in flight before the first ballot
static_assert(CW <= 64 && CW % LU == 0, "a chunk's words live one per lane and are formed LU at a time");

struct Tiling {
    int frame_length, hop_length, seg_len, stride;
};

// the windows of a clip of n samples
__device__ __forceinline__ long long window_count(int n, const Tiling& t) {
    return n < t.seg_len ? 1 : 1 + (long long)(n - t.seg_len) / t.stride;
}

// first and last frame of window w of a clip of n samples and F frames, in closed form; first > last: no frame
__device__ __forceinline__ void window_frames(long long w, int n, long long F, const Tiling& t, long long& first,
                                              long long& last) {
    if (n < t.frame_length) {                                    // the clip is one frame and one window
        first = 0;
        last = min(0LL, F - 1);
        return;
    }
    const long long a = w * t.stride, b = a + min(t.seg_len, n);
    first = (a + t.hop_length - 1) / t.hop_length;
    last = min((b - t.frame_length) / t.hop_length, F - 1);
}

__device__ __forceinline__ int wave_max_i32(int v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = max(v, __shfl_xor(v, m, 64));
    return v;
}

__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = fmax(v, __shfl_xor(v, m, 64));
    return v;
}

__global__ __launch_bounds__(64 * PW) void window_activity_kernel(const double* __restrict__ energy,
                                                                  const long long* __restrict__ frame_offs,
                                                                  const int* __restrict__ lens,
                                                                  const long long* __restrict__ window_offs, int n_clips,
                                                                  Tiling t, int max_windows, double ratio, double floor_e,
                                                                  double min_active, double* peak, int* clip_active,
                                                                  int* active, int* keep, int* counts) {
    __shared__ unsigned long long s_words[PW][CW + 1];           // a chunk's ballots, and a zero word behind them
    __shared__ int s_below[PW][CW + 1];                          // active frames of the chunk in front of each word
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int clip = blockIdx.x * PW + wave;
    if (clip >= n_clips) return;                                 // a whole wave
    unsigned long long* words = s_words[wave];
    int* below = s_below[wave];
    const long long fo = frame_offs[clip];
    const long long F = frame_offs[clip + 1] - fo;
    const double* e = energy + fo;
    const int n = lens[clip];
    const long long wo = window_offs[clip];
    const long long W = n < 1 ? 0 : max(0LL, min(window_count(n, t), window_offs[clip + 1] - wo));
    int* m_out = active + wo;
    int* k_out = keep + wo;

    // pass 1: every energy finite, and the largest
    double e_max = -INFINITY;
    int bad = 0;
    for (long long f = lane; f < F; f += 64) {
        const double v = e[f];
        bad |= !(fabs(v) <= DBL_MAX);                            // NaN or Inf
        e_max = fmax(e_max, v);
    }
    e_max = wave_max_f64(e_max);
    const bool finite = F >= 1 && !__any(bad);
    const bool gated = !finite || n < 1 || e_max < floor_e;
    if (lane == 0) peak[clip] = finite ? e_max : __builtin_nan("");

    for (long long wb = 0; wb < W; wb += 64)
        if (wb + lane < W) {
            m_out[wb + lane] = 0;
            if (gated) k_out[wb + lane] = 0;
        }
    if (gated) {
        if (lane == 0) {
            clip_active[clip] = 0;
            counts[clip] = 0;
        }
        return;
    }

    // pass 2: chunk by chunk, the activity as bits and what each window holds of them
    const double thr = fmax(e_max * ratio, floor_e);
    const int win_len = min(t.seg_len, n);                       // >= frame_length unless the clip is one short frame
    long long n_active = 0;
    for (long long c0 = 0; c0 < F; c0 += CF) {
        const long long c1 = min(c0 + CF, F);
        unsigned long long word = 0;
        for (int it = 0; it < CW && c0 + it * 64 < c1; it += LU) {
            double v[LU];
#pragma unroll
            for (int u = 0; u < LU; ++u) {
                const long long f = c0 + (it + u) * 64 + lane;
                v[u] = f < c1 ? e[f] : -1.0;
            }
#pragma unroll
            for (int u = 0; u < LU; ++u) {
                const long long f = c0 + (it + u) * 64 + lane;
                const unsigned long long mask = __ballot(f < c1 && v[u] >= thr);
                if (lane == it + u) word = mask;
            }
        }
        const int pc = __popcll(word);
        int incl = pc;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (lane < CW) {
            words[lane] = word;
            below[lane] = incl - pc;
        }
        if (lane == 63) {                                        // lanes CW.. hold no word: lane 63 has the chunk's total
            words[CW] = 0;
            below[CW] = incl;
        }
        n_active += __shfl(incl, 63, 64);
        wave_lds_fence();

        // the windows with a frame in [c0, c1): first(w) <= c1 - 1 and last(w) >= c0
        const long long need = c0 * t.hop_length - win_len + min(t.frame_length, n);   // a short clip's frame is the clip
        const long long w_lo = need > 0 ? (need + t.stride - 1) / t.stride : 0;
        const long long w_hi = min(((c1 - 1) * t.hop_length) / t.stride, W - 1);
        auto frames_below = [&](long long p) {                   // active frames of the chunk in front of its frame p
            const int i = int(p >> 6), r = int(p & 63);
            return below[i] + __popcll(words[i] & ((1ull << r) - 1ull));
        };
        for (long long wb = w_lo & ~63LL; wb <= w_hi; wb += 64) {
            const long long w = wb + lane;
            if (w < w_lo || w > w_hi) continue;
            long long first, last;
            window_frames(w, n, F, t, first, last);
            const long long lo = max(first, c0), hi = min(last, c1 - 1);
            if (lo > hi) continue;
            const int add = frames_below(hi + 1 - c0) - frames_below(lo - c0);
            if (add) m_out[w] += add;
        }
        wave_lds_fence();                                        // the next chunk overwrites the words
    }
    if (lane == 0) clip_active[clip] = int(n_active);

    // which windows qualify
    int qualifying = 0, m_max = 0;
    for (long long wb = 0; wb < W; wb += 64) {
        const long long w = wb + lane;
        bool q = false;
        if (w < W) {
            long long first, last;
            window_frames(w, n, F, t, first, last);
            const int cnt = int(max(last - first + 1, 0LL)), m = m_out[w];
            q = m >= 1 && double(m) >= min_active * double(cnt);
            k_out[w] = q ? 1 : 0;
            if (q) m_max = max(m_max, m);
        }
        qualifying += __popcll(__ballot(q));
    }
    if (qualifying <= max_windows) {
        if (lane == 0) counts[clip] = qualifying;
        return;
    }

    // the cap: the largest level T with at least max_windows qualifying windows of m >= T, by bisection
    m_max = wave_max_i32(m_max);
    auto count_from = [&](int level) {
        int c = 0;
        for (long long wb = 0; wb < W; wb += 64) {
            const long long w = wb + lane;
            c += __popcll(__ballot(w < W && k_out[w] && m_out[w] >= level));
        }
        return c;
    };
    int level = 1, above_level = m_max + 1, n_above = 0;         // count_from(level) >= max_windows > count_from(above_level)
    while (above_level - level > 1) {
        const int mid = level + (above_level - level) / 2;
        const int c = count_from(mid);
        if (c >= max_windows) {
            level = mid;
        } else {
            above_level = mid;
            n_above = c;
        }
    }
    // every window above the level, and the earliest of the level until max_windows are kept
    const int from_level = max_windows - n_above;
    int taken = 0;
    for (long long wb = 0; wb < W; wb += 64) {
        const long long w = wb + lane;
        const bool q = w < W && k_out[w];
        const int m = q ? m_out[w] : 0;
        const bool at = q && m == level;
        const unsigned long long at_mask = __ballot(at);
        const int rank = taken + __popcll(at_mask & ((1ull << lane) - 1ull));
        if (w < W) k_out[w] = (q && m > level) || (at && rank < from_level) ? 1 : 0;
        taken += __popcll(at_mask);
    }
    if (lane == 0) counts[clip] = max_windows;
}

__global__ __launch_bounds__(64 * PW) void list_windows_kernel(const int* __restrict__ keep, const int* __restrict__ active,
                                                               const int* __restrict__ lens,
                                                               const long long* __restrict__ window_offs,
                                                               const long long* __restrict__ row_offs, int n_clips,
                                                               Tiling t, long long* __restrict__ row_clip,
                                                               int* __restrict__ row_start, int* __restrict__ row_length,
                                                               int* __restrict__ row_active) {
    const int lane = threadIdx.x & 63;
    const int clip = blockIdx.x * PW + (threadIdx.x >> 6);
    if (clip >= n_clips) return;                                 // a whole wave
    const int n = lens[clip];
    const long long wo = window_offs[clip], ro = row_offs[clip];
    const long long W = n < 1 ? 0 : max(0LL, min(window_count(n, t), window_offs[clip + 1] - wo));
    const long long rows = row_offs[clip + 1] - ro;
    long long taken = 0;
    for (long long wb = 0; wb < W && taken < rows; wb += 64) {
        const long long w = wb + lane;
        const bool k = w < W && keep[wo + w] != 0;
        const unsigned long long mask = __ballot(k);
        const long long row = taken + __popcll(mask & ((1ull << lane) - 1ull));
        if (k && row < rows) {
            row_clip[ro + row] = clip;
            row_start[ro + row] = int(w * t.stride);
            row_length[ro + row] = min(t.seg_len, n);
            row_active[ro + row] = active[wo + w];
        }
        taken += __popcll(mask);
    }
}

}  // namespace
}  // namespace cough

extern "C" int cough_slices_abi_version(void) { return COUGH_SLICES_ABI_VERSION; }
// this library's own last-error slot
COUGH_DEFINE_LAST_ERROR(cough_slices_last_error)

extern "C" int cough_window_activity(const double* d_energy, const long long* d_frame_offsets, const int* d_lengths,
                                     const long long* d_window_offsets, int n_clips, int frame_length, int hop_length,
                                     int seg_len, int stride, int max_windows, double ratio, double floor, double min_active,
                                     double* d_peak, int* d_clip_active, int* d_active, int* d_keep, int* d_counts,
                                     void* stream) {
    using namespace cough;
    const char* fn = "cough_window_activity";
    COUGH_REQUIRE(d_energy && d_frame_offsets && d_lengths && d_window_offsets && d_peak && d_clip_active && d_active &&
                  d_keep && d_counts, COUGH_EINVAL, "%s: NULL argument", fn);
    COUGH_REQUIRE(n_clips >= 0, COUGH_EINVAL, "%s: n_clips must not be negative, got %d", fn, n_clips);
    COUGH_REQUIRE(frame_length >= 1, COUGH_EINVAL, "%s: frame_length must be positive, got %d", fn, frame_length);
    COUGH_REQUIRE(hop_length >= 1, COUGH_EINVAL, "%s: hop_length must be positive, got %d", fn, hop_length);
    COUGH_REQUIRE(seg_len >= frame_length, COUGH_EINVAL, "%s: seg_len = %d must not be below frame_length = %d", fn, seg_len,
                  frame_length);
    COUGH_REQUIRE(stride >= 1, COUGH_EINVAL, "%s: stride must be positive, got %d", fn, stride);
    COUGH_REQUIRE(max_windows >= 1, COUGH_EINVAL, "%s: max_windows must be positive, got %d", fn, max_windows);
    COUGH_REQUIRE(ratio >= 0.0 && ratio <= DBL_MAX && floor >= 0.0 && floor <= DBL_MAX && min_active >= 0.0 &&
                  min_active <= DBL_MAX, COUGH_EINVAL,
                  "%s: ratio, floor and min_active must be finite and not negative, got %g, %g and %g", fn, ratio, floor,
                  min_active);
    COUGH_REQUIRE(aligned(d_lengths, 4) && aligned(d_clip_active, 4) && aligned(d_active, 4) && aligned(d_keep, 4) &&
                  aligned(d_counts, 4), COUGH_EINVAL, "%s: int32 arrays must be 4-byte aligned", fn);
    COUGH_REQUIRE(aligned(d_energy, 8) && aligned(d_frame_offsets, 8) && aligned(d_window_offsets, 8) && aligned(d_peak, 8),
                  COUGH_EINVAL, "%s: int64 and float64 arrays must be 8-byte aligned", fn);
    if (n_clips == 0) return COUGH_OK;
    const Tiling t{frame_length, hop_length, seg_len, stride};
    hipLaunchKernelGGL(window_activity_kernel, dim3(unsigned((n_clips + PW - 1) / PW)), dim3(64 * PW), 0,
                       static_cast<hipStream_t>(stream), d_energy, d_frame_offsets, d_lengths, d_window_offsets, n_clips, t,
                       max_windows, ratio, floor, min_active, d_peak, d_clip_active, d_active, d_keep, d_counts);
    COUGH_HIP_CHECK(hipGetLastError());
    return COUGH_OK;
}

extern "C" int cough_list_windows(const int* d_keep, const int* d_active, const int* d_lengths,
                                  const long long* d_window_offsets, const long long* d_row_offsets, int n_clips, int seg_len,
                                  int stride, long long* d_clip, int* d_start, int* d_length, int* d_row_active,
                                  void* stream) {
    using namespace cough;
    const char* fn = "cough_list_windows";
    COUGH_REQUIRE(d_keep && d_active && d_lengths && d_window_offsets && d_row_offsets && d_clip && d_start && d_length &&
                  d_row_active, COUGH_EINVAL, "%s: NULL argument", fn);
    COUGH_REQUIRE(n_clips >= 0, COUGH_EINVAL, "%s: n_clips must not be negative, got %d", fn, n_clips);
    COUGH_REQUIRE(seg_len >= 1, COUGH_EINVAL, "%s: seg_len must be positive, got %d", fn, seg_len);
    COUGH_REQUIRE(stride >= 1, COUGH_EINVAL, "%s: stride must be positive, got %d", fn, stride);
    COUGH_REQUIRE(aligned(d_keep, 4) && aligned(d_active, 4) && aligned(d_lengths, 4) && aligned(d_start, 4) &&
                  aligned(d_length, 4) && aligned(d_row_active, 4), COUGH_EINVAL, "%s: int32 arrays must be 4-byte aligned",
                  fn);
    COUGH_REQUIRE(aligned(d_window_offsets, 8) && aligned(d_row_offsets, 8) && aligned(d_clip, 8), COUGH_EINVAL,
                  "%s: int64 arrays must be 8-byte aligned", fn);
    if (n_clips == 0) return COUGH_OK;
    const Tiling t{1, 1, seg_len, stride};
    hipLaunchKernelGGL(list_windows_kernel, dim3(unsigned((n_clips + PW - 1) / PW)), dim3(64 * PW), 0,
                       static_cast<hipStream_t>(stream), d_keep, d_active, d_lengths, d_window_offsets, d_row_offsets,
                       n_clips, t, d_clip, d_start, d_length, d_row_active);
    COUGH_HIP_CHECK(hipGetLastError());
    return COUGH_OK;
}
