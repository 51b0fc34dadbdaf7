// libcough_amd_segments.so: corpus curation on the packed clip bank (include/cough_amd_segments.h).  Three kernels: the
// short-time energy of every frame of every clip (the one that touches the whole corpus, bandwidth-bound), the pick of
// segments from a clip's energies (one wave per clip, a few KB each), and the copy of the picked rows into a packed bank.
//
// Frame energy.  Frames overlap (400 samples every 160), so a workgroup takes a TILE of consecutive frames of one clip and
// brings the samples the tile spans from HBM into LDS once; only the frame_length - hop_length samples that the first
// frames of the next tile share are fetched again, by a neighbour, out of L2.  Both frame_length and hop_length are
// multiples of g = gcd(frame_length, hop_length), so every frame is a whole number of g-sample sub-blocks: a thread sums
// double(x)^2 over one sub-block in sample order, and a frame is the sum of its frame_length / g sub-block sums in
// sub-block order.  The order never depends on the tiling, the grid or the clip's alignment: the same samples give the
// same bits.  (float32 squares are exact in float64, so whether the compiler contracts the sum into FMAs changes nothing.)
//
// LDS image.  Sub-block s of the tile lives at s * pitch with pitch = g | 1: thread s walks its sub-block while its
// neighbours walk theirs, and an odd pitch spreads the 32 lanes of a ds_read_b32 group over 32 banks (g = 80 would put
// them on two).  The loads align on the SOURCE (float4 from the first 16-byte boundary of the span, a scalar head and
// tail), since a clip starts at any element, and a thread keeps LU of them in flight before it stores the first.
#include "../../include/cough_amd_segments.h"

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdint>
#include <numeric>

#include "common.h"

namespace cough {

namespace {

constexpr int ET = 256;              // threads of the energy kernel
constexpr int LU = 6;                // float4 loads a thread of it keeps in flight
constexpr int LDS_BUDGET = 48 << 10; // bytes of a tile's LDS image: three workgroups per CU
constexpr int PW = 4;                // waves (clips) per workgroup of the pick kernel
constexpr int CT = 256;              // threads of the copy kernel
constexpr int MAX_CHUNKS = 64;       // workgroups per copied row at most; each strides over the rest

// what a frame / hop pair makes of a tile: the sub-block, the sub-blocks of a frame and of a hop, the frames of a tile
struct TileShape {
    int sub, frame_subs, hop_subs, tile_frames;
    size_t lds_bytes;
};

constexpr size_t sub_bytes(int sub) { return size_t(sub | 1) * sizeof(float) + sizeof(double); }

TileShape tile_shape(int frame_length, int hop_length) {
    TileShape s;
    s.sub = std::gcd(frame_length, hop_length);
    s.frame_subs = frame_length / s.sub;
    s.hop_subs = hop_length / s.sub;
    const long long max_subs = (long long)(LDS_BUDGET / sub_bytes(s.sub));   // >= frame_subs for every accepted pair
    s.tile_frames = int(std::min<long long>((max_subs - s.frame_subs) / s.hop_subs + 1, 1 << 20));
    const long long subs = (long long)(s.tile_frames - 1) * s.hop_subs + s.frame_subs;
    // a clip shorter than a frame is one sub-block of its own length (< frame_length)
    s.lds_bytes = std::max(size_t(subs) * sub_bytes(s.sub), sub_bytes(frame_length));
    return s;
}

// four consecutive floats from a pointer that is 4-byte aligned only
__device__ __forceinline__ float4 load4_unaligned(const float* p) {
    float t[4];
    __builtin_memcpy(t, p, 16);
    return make_float4(t[0], t[1], t[2], t[3]);
}

// elements from `p` to the next 16-byte boundary (0..3)
__device__ __forceinline__ int head_to_16(const float* p) {
    return int((4u - unsigned((reinterpret_cast<uintptr_t>(p) >> 2) & 3u)) & 3u);
}

// ------------------------------------------------------------------------------------------ frame energies
__global__ __launch_bounds__(ET) void frame_energy_kernel(const float* __restrict__ bank, const long long* __restrict__ offs,
                                                          const int* __restrict__ lens,
                                                          const long long* __restrict__ frame_offs, int n_clips,
                                                          const int* __restrict__ tiles, int frame_length, int hop_length,
                                                          TileShape shape, double* __restrict__ energy) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x;
    const int clip = tiles[2 * blockIdx.x], f0 = tiles[2 * blockIdx.x + 1];
    if (clip < 0 || clip >= n_clips || f0 < 0) return;          // the whole workgroup takes these branches
    const int n = lens[clip];
    if (n < 1) return;
    const bool whole = n < frame_length;                         // one frame: the whole clip
    const int clip_frames = whole ? 1 : 1 + (n - frame_length) / hop_length;
    if (f0 >= clip_frames) return;
    const int nf = min(shape.tile_frames, clip_frames - f0);
    const int sub = whole ? n : shape.sub, fs = whole ? 1 : shape.frame_subs, hs = whole ? 1 : shape.hop_subs;
    const int pitch = sub | 1;
    const int n_sub = (nf - 1) * hs + fs;
    const int span = n_sub * sub;                                // <= LDS_BUDGET / 4 samples, all of them inside the clip
    double* ss = reinterpret_cast<double*>(smem);                // [n_sub] sub-block sums
    float* xs = reinterpret_cast<float*>(ss + n_sub);            // [n_sub][pitch] samples
    const float* p = bank + offs[clip] + (long long)f0 * hop_length;

    // sample i of the span -> (sub-block, place in it); i < 2^14, so the float quotient is off by one at the most
    const float inv = 1.0f / float(sub);
    auto place = [&](int i, int& d, int& r) {
        d = int((float(i) + 0.5f) * inv);
        r = i - d * sub;
        if (r < 0) {
            --d;
            r += sub;
        } else if (r >= sub) {
            ++d;
            r -= sub;
        }
    };
    auto put = [&](int i, float v) {
        int d, r;
        place(i, d, r);
        xs[d * pitch + r] = v;
    };
    const int head = min(span, head_to_16(p));
    if (tid < head) put(tid, p[tid]);
    const int groups = (span - head) >> 2;
    const float4* p4 = reinterpret_cast<const float4*>(p + head);
    // LU loads in flight per thread before the first of them is stored: 12 waves per CU with one 16-byte load each
    // would keep 12 KB on its way from HBM, far too little to cover its latency
    for (int q0 = tid; q0 < groups; q0 += LU * ET) {
        float4 v[LU];
#pragma unroll
        for (int u = 0; u < LU; ++u)
            if (q0 + u * ET < groups) v[u] = p4[q0 + u * ET];
#pragma unroll
        for (int u = 0; u < LU; ++u) {
            const int q = q0 + u * ET;
            if (q >= groups) break;
            const float x[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
            int d, r;
            place(head + 4 * q, d, r);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (r == sub) {
                    r = 0;
                    ++d;
                }
                xs[d * pitch + r] = x[k];
                ++r;
            }
        }
    }
    const int done = head + 4 * groups;
    if (tid < span - done) put(done + tid, p[done + tid]);
    __syncthreads();

    for (int s = tid; s < n_sub; s += ET) {
        const float* row = xs + s * pitch;
        double acc = 0.0;
#pragma unroll 8
        for (int j = 0; j < sub; ++j) {
            const double x = double(row[j]);
            acc += x * x;
        }
        ss[s] = acc;
    }
    __syncthreads();

    const double count = double(whole ? n : frame_length);
    double* e = energy + frame_offs[clip] + f0;
    for (int t = tid; t < nf; t += ET) {
        const double* first = ss + t * hs;
        double acc = 0.0;
        for (int k = 0; k < fs; ++k) acc += first[k];
        e[t] = acc / count;
    }
}

// ------------------------------------------------------------------------------------------ energies -> segments
__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = fmax(v, __shfl_xor(v, m, 64));
    return v;
}

// the largest value of the wave and the lowest lane that holds it, in every lane
__device__ __forceinline__ void wave_first_max(double& v, int& i) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const double ov = __shfl_xor(v, m, 64);
        const int oi = __shfl_xor(i, m, 64);
        if (ov > v || (ov == v && oi < i)) {
            v = ov;
            i = oi;
        }
    }
}

// One wave per clip.  Pass 1: every energy finite, and the largest.  Pass 2: 64 frames at a time, the activity of a
// chunk is one ballot; the wave walks its stretches of ones and zeros (every lane holds the same state, the control flow
// is uniform), takes the first largest energy of a stretch of ones with one wave reduction, and carries the open run --
// its length, its peak -- into the next chunk.  A run is closed by the first inactive frame after it, or by the end.
__global__ __launch_bounds__(64 * PW) void pick_segments_kernel(const double* __restrict__ energy,
                                                                const long long* __restrict__ frame_offs,
                                                                const int* __restrict__ lens, int n_clips, int frame_length,
                                                                int hop_length, int seg_len, int min_frames, int max_segments,
                                                                double ratio, double floor_e, int* __restrict__ counts,
                                                                int* __restrict__ starts, int* __restrict__ seg_lengths,
                                                                float* __restrict__ peak_db) {
    const int lane = threadIdx.x & 63;
    const int clip = blockIdx.x * PW + (threadIdx.x >> 6);
    if (clip >= n_clips) return;                                 // a whole wave
    const long long fo = frame_offs[clip];
    const long long frames = frame_offs[clip + 1] - fo;
    const double* e = energy + fo;
    const int n = lens[clip];
    int* st = starts + (long long)clip * max_segments;
    int* ln = seg_lengths + (long long)clip * max_segments;
    float* pk = peak_db + (long long)clip * max_segments;

    double e_max = 0.0;
    int bad = 0;
    for (long long f = lane; f < frames; f += 64) {
        const double v = e[f];
        bad |= !(fabs(v) <= DBL_MAX);                            // NaN or Inf
        e_max = fmax(e_max, v);
    }
    e_max = wave_max_f64(e_max);
    const bool gated = n < 1 || frames < 1 || __any(bad) || e_max < floor_e;

    int count = 0;
    if (!gated) {
        const double thr = e_max * ratio;
        bool in_run = false;
        long long run_len = 0, best_f = 0, last_end = 0;
        double best = -1.0;
        auto close_run = [&]() {
            in_run = false;
            if (run_len < min_frames || count >= max_segments) return;
            const long long c = best_f * hop_length + frame_length / 2;
            const long long hi = n > seg_len ? n - seg_len : 0;
            const long long start = min(max(c - seg_len / 2, 0LL), hi);
            const int length = min(seg_len, n);
            if (count > 0 && start < last_end) return;
            if (lane == 0) {
                st[count] = int(start);
                ln[count] = length;
                pk[count] = float(10.0 * log10(best));
            }
            last_end = start + length;
            ++count;
        };
        for (long long base = 0; base < frames && count < max_segments; base += 64) {
            const long long f = base + lane;
            const double v = f < frames ? e[f] : -1.0;
            const unsigned long long mask = __ballot(f < frames && v >= thr);
            const int cnt = int(min(64LL, frames - base));
            int pos = 0;
            while (pos < cnt) {
                const unsigned long long rest = mask >> pos;
                if (rest & 1ull) {
                    const unsigned long long inv = ~rest;
                    const int len = min(inv ? __builtin_ctzll(inv) : 64, cnt - pos);
                    double bv = lane >= pos && lane < pos + len ? v : -1.0;
                    int bi = lane;
                    wave_first_max(bv, bi);
                    if (!in_run) {
                        in_run = true;
                        run_len = 0;
                        best = -1.0;
                    }
                    if (bv > best) {                             // an equal peak later in the run does not replace it
                        best = bv;
                        best_f = base + bi;
                    }
                    run_len += len;
                    pos += len;
                } else {
                    if (in_run) close_run();
                    pos += min(rest ? __builtin_ctzll(rest) : 64, cnt - pos);
                }
            }
        }
        if (in_run) close_run();
    }
    if (lane == 0) counts[clip] = count;
    if (lane >= count && lane < max_segments) {
        st[lane] = 0;
        ln[lane] = 0;
        pk[lane] = 0.0f;
    }
}

// ------------------------------------------------------------------------------------------ ragged rows -> packed rows
// grid (row, chunk), aligned on what it WRITES as the kernels of data.hip are: one float4 store per thread and step, the
// four source samples as one 4-byte-aligned 16-byte access, a scalar head and tail
__global__ __launch_bounds__(CT) void copy_segments_kernel(const float* __restrict__ src, const long long* __restrict__ src_offs,
                                                           const int* __restrict__ row_starts, const int* __restrict__ lens,
                                                           const long long* __restrict__ dst_offs, float* __restrict__ dst) {
    const int r = blockIdx.x;
    const float* in = src + src_offs[r] + max(row_starts[r], 0);
    const int len = max(lens[r], 0);
    float* o = dst + dst_offs[r];
    const int gt = blockIdx.y * CT + threadIdx.x, gthreads = gridDim.y * CT;
    const int head = min(len, head_to_16(o));
    if (gt < head) o[gt] = in[gt];
    const int groups = (len - head) >> 2;
    for (int g = gt; g < groups; g += gthreads) {
        const int i = head + 4 * g;
        *reinterpret_cast<float4*>(o + i) = load4_unaligned(in + i);
    }
    const int done = head + 4 * groups;
    if (gt < len - done) o[done + gt] = in[done + gt];
}

bool frame_pair_ok(int frame_length, int hop_length) {
    return frame_length >= 1 && hop_length >= 1 && frame_length <= COUGH_MAX_FRAME_LENGTH;
}

}  // namespace
}  // namespace cough

extern "C" int cough_segments_abi_version(void) { return COUGH_SEGMENTS_ABI_VERSION; }
// this library's own last-error slot (libcough_amd.so keeps its own behind cough_amd_last_error)
COUGH_DEFINE_LAST_ERROR(cough_segments_last_error)

extern "C" int cough_frame_energy_tile_frames(int frame_length, int hop_length) {
    using namespace cough;
    return frame_pair_ok(frame_length, hop_length) ? tile_shape(frame_length, hop_length).tile_frames : 0;
}

extern "C" int cough_frame_energy(const float* d_bank, const long long* d_clip_offsets, const int* d_lengths,
                                  const long long* d_frame_offsets, int n_clips, const int* d_tiles, int n_tiles,
                                  int frame_length, int hop_length, double* d_energy, void* stream) {
    using namespace cough;
    const char* fn = "cough_frame_energy";
    COUGH_REQUIRE(d_bank && d_clip_offsets && d_lengths && d_frame_offsets && d_tiles && d_energy, COUGH_EINVAL,
                  "%s: NULL argument", fn);
    COUGH_REQUIRE(n_clips >= 0, COUGH_EINVAL, "%s: n_clips must not be negative, got %d", fn, n_clips);
    COUGH_REQUIRE(n_tiles >= 0, COUGH_EINVAL, "%s: n_tiles must not be negative, got %d", fn, n_tiles);
    COUGH_REQUIRE(frame_length >= 1, COUGH_EINVAL, "%s: frame_length must be positive, got %d", fn, frame_length);
    COUGH_REQUIRE(hop_length >= 1, COUGH_EINVAL, "%s: hop_length must be positive, got %d", fn, hop_length);
    COUGH_REQUIRE(frame_length <= COUGH_MAX_FRAME_LENGTH, COUGH_EUNSUPPORTED, "%s: frame_length %d is above %d", fn,
                  frame_length, COUGH_MAX_FRAME_LENGTH);
    COUGH_REQUIRE(aligned(d_bank, 4) && aligned(d_lengths, 4) && aligned(d_tiles, 4), COUGH_EINVAL,
                  "%s: float32 and int32 arrays must be 4-byte aligned", fn);
    COUGH_REQUIRE(aligned(d_clip_offsets, 8) && aligned(d_frame_offsets, 8) && aligned(d_energy, 8), COUGH_EINVAL,
                  "%s: int64 and float64 arrays must be 8-byte aligned", fn);
    if (n_clips == 0 || n_tiles == 0) return COUGH_OK;
    const TileShape shape = tile_shape(frame_length, hop_length);
    hipLaunchKernelGGL(frame_energy_kernel, dim3(unsigned(n_tiles)), dim3(ET), shape.lds_bytes,
                       static_cast<hipStream_t>(stream), d_bank, d_clip_offsets, d_lengths, d_frame_offsets, n_clips,
                       d_tiles, frame_length, hop_length, shape, d_energy);
    COUGH_HIP_CHECK(hipGetLastError());
    return COUGH_OK;
}

extern "C" int cough_pick_segments(const double* d_energy, const long long* d_frame_offsets, const int* d_lengths,
                                   int n_clips, int frame_length, int hop_length, int seg_len, int min_frames,
                                   int max_segments, double ratio, double floor, int* d_counts, int* d_starts,
                                   int* d_seg_lengths, float* d_peak_db, void* stream) {
    using namespace cough;
    const char* fn = "cough_pick_segments";
    COUGH_REQUIRE(d_energy && d_frame_offsets && d_lengths && d_counts && d_starts && d_seg_lengths && d_peak_db,
                  COUGH_EINVAL, "%s: NULL argument", fn);
    COUGH_REQUIRE(n_clips >= 0, COUGH_EINVAL, "%s: n_clips must not be negative, got %d", fn, n_clips);
    COUGH_REQUIRE(frame_length >= 1, COUGH_EINVAL, "%s: frame_length must be positive, got %d", fn, frame_length);
    COUGH_REQUIRE(hop_length >= 1, COUGH_EINVAL, "%s: hop_length must be positive, got %d", fn, hop_length);
    COUGH_REQUIRE(seg_len >= 1, COUGH_EINVAL, "%s: seg_len must be positive, got %d", fn, seg_len);
    COUGH_REQUIRE(min_frames >= 1, COUGH_EINVAL, "%s: min_frames must be positive, got %d", fn, min_frames);
    COUGH_REQUIRE(max_segments >= 1 && max_segments <= COUGH_MAX_SEGMENTS, COUGH_EINVAL, "%s: max_segments = %d (1..%d)",
                  fn, max_segments, COUGH_MAX_SEGMENTS);
    COUGH_REQUIRE(ratio >= 0.0 && ratio <= DBL_MAX && floor >= 0.0 && floor <= DBL_MAX, COUGH_EINVAL,
                  "%s: ratio and floor must be finite and not negative, got %g and %g", fn, ratio, floor);
    COUGH_REQUIRE(aligned(d_lengths, 4) && aligned(d_counts, 4) && aligned(d_starts, 4) && aligned(d_seg_lengths, 4) &&
                  aligned(d_peak_db, 4), COUGH_EINVAL, "%s: float32 and int32 arrays must be 4-byte aligned", fn);
    COUGH_REQUIRE(aligned(d_energy, 8) && aligned(d_frame_offsets, 8), COUGH_EINVAL,
                  "%s: int64 and float64 arrays must be 8-byte aligned", fn);
    if (n_clips == 0) return COUGH_OK;
    hipLaunchKernelGGL(pick_segments_kernel, dim3(unsigned((n_clips + PW - 1) / PW)), dim3(64 * PW), 0,
                       static_cast<hipStream_t>(stream), d_energy, d_frame_offsets, d_lengths, n_clips, frame_length,
                       hop_length, seg_len, min_frames, max_segments, ratio, floor, d_counts, d_starts, d_seg_lengths,
                       d_peak_db);
    COUGH_HIP_CHECK(hipGetLastError());
    return COUGH_OK;
}

extern "C" int cough_copy_segments(const float* d_src, const long long* d_src_offsets, const int* d_starts,
                                   const int* d_row_lengths, const long long* d_dst_offsets, int n_rows, int max_len,
                                   float* d_dst, void* stream) {
    using namespace cough;
    const char* fn = "cough_copy_segments";
    COUGH_REQUIRE(d_src && d_src_offsets && d_starts && d_row_lengths && d_dst_offsets && d_dst, COUGH_EINVAL,
                  "%s: NULL argument", fn);
    COUGH_REQUIRE(n_rows >= 0, COUGH_EINVAL, "%s: n_rows must not be negative, got %d", fn, n_rows);
    COUGH_REQUIRE(max_len >= 1, COUGH_EINVAL, "%s: max_len must be positive, got %d", fn, max_len);
    COUGH_REQUIRE(aligned(d_src, 4) && aligned(d_dst, 4) && aligned(d_starts, 4) && aligned(d_row_lengths, 4), COUGH_EINVAL,
                  "%s: float32 and int32 arrays must be 4-byte aligned", fn);
    COUGH_REQUIRE(aligned(d_src_offsets, 8) && aligned(d_dst_offsets, 8), COUGH_EINVAL,
                  "%s: int64 arrays must be 8-byte aligned", fn);
    if (n_rows == 0) return COUGH_OK;
    const unsigned chunks = unsigned(std::clamp((max_len / 4 + CT - 1) / CT, 1, MAX_CHUNKS));
    hipLaunchKernelGGL(copy_segments_kernel, dim3(unsigned(n_rows), chunks), dim3(CT), 0, static_cast<hipStream_t>(stream),
                       d_src, d_src_offsets, d_starts, d_row_lengths, d_dst_offsets, d_dst);
    COUGH_HIP_CHECK(hipGetLastError());
    return COUGH_OK;
}
