// libcough_amd_data.so: the device side of the input pipeline (include/cough_amd_data.h).  Three bandwidth-bound kernels
// around the augmentor and the featuriser: ragged rows of a packed clip bank into a matrix, normalize -> pad_or_trim of a
// batch of rows, and SpecAugment's masking with a mask set per image.
//
// Access width.  A clip of the bank starts at any element, so a row's source is 4-byte aligned only, while the rows
// written (a matrix row, a feature image) are 16-byte aligned whenever the base pointer and the row pitch allow it.  The
// kernels therefore align on what they WRITE (one float4 store per thread and step, a scalar head and tail where a row
// does not start or end on 16 bytes) and read the four source samples as one 4-byte-aligned 16-byte access, which gfx950
// serves in one instruction; the peak pass of the prepare kernel, which only reads, aligns on its source instead.
#include "../../include/cough_amd_data.h"

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstring>

#include "common.h"

namespace cough {

namespace {

constexpr int GT = 256;        // threads of the gather and mask kernels
constexpr int PT = 1024;       // threads of the prepare kernel: one workgroup walks a whole clip twice
constexpr int MAX_CHUNKS = 64; // workgroups per row / image at most; each strides over the rest

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

// ------------------------------------------------------------------------------------------ ragged rows -> matrix
// grid (row, chunk): thread t of chunk c takes the output groups c * GT + t, + chunks * GT, ... of its row
__global__ __launch_bounds__(GT) void gather_rows_kernel(const float* __restrict__ src, const long long* __restrict__ offs,
                                                         const int* __restrict__ lens, float* __restrict__ out,
                                                         long long out_stride, int row_len) {
    const int r = blockIdx.x;
    const float* in = src + offs[r];
    const int len = min(max(lens[r], 0), row_len);
    float* o = out + (long long)r * out_stride;
    const int gt = blockIdx.y * GT + threadIdx.x, gthreads = gridDim.y * GT;
    auto at = [&](int i) { return i < len ? in[i] : 0.0f; };
    const int head = min(row_len, head_to_16(o));
    if (gt < head) o[gt] = at(gt);
    const int groups = (row_len - head) >> 2;
    for (int g = gt; g < groups; g += gthreads) {
        const int i = head + 4 * g;
        const float4 v = i + 3 < len ? load4_unaligned(in + i) : make_float4(at(i), at(i + 1), at(i + 2), at(i + 3));
        *reinterpret_cast<float4*>(o + i) = v;
    }
    const int done = head + 4 * groups;
    if (gt < row_len - done) o[done + gt] = at(done + gt);
}

// ------------------------------------------------------------------------------------------ normalize -> pad_or_trim
// one workgroup per row: pass 1 takes the peak of the whole row (float4 reads from its first 16-byte boundary on), pass 2
// writes the centre-trimmed / zero-padded, normalised window (float4 stores).  max is exact in any order, and a NaN is
// tracked apart from it, so the result does not depend on how the samples are spread over the threads.
__global__ __launch_bounds__(PT) void prepare_rows_kernel(const float* __restrict__ src, const long long* __restrict__ offs,
                                                          const int* __restrict__ lens, float* __restrict__ out, int out_len,
                                                          int normalize) {
    __shared__ float red[PT / 64];
    const int r = blockIdx.x, tid = threadIdx.x;
    const float* in = src + offs[r];
    const int n = lens[r];
    float* o = out + (long long)r * out_len;
    if (n < 1) {                               // not a clip: a zero row (the whole workgroup takes this branch)
        for (int i = tid; i < out_len; i += PT) o[i] = 0.0f;
        return;
    }
    float peak = 0.f;
    int isnan = 0;   // `waveform.abs().max()` of a signal holding a NaN is NaN, and `NaN > 0` leaves the signal unscaled
    if (normalize) {
        auto take = [&](float v) {
            peak = fmaxf(peak, fabsf(v));
            isnan |= v != v;
        };
        const int head = min(n, head_to_16(in));
        if (tid < head) take(in[tid]);
        const int groups = (n - head) >> 2;
        const float4* in4 = reinterpret_cast<const float4*>(in + head);
        for (int g = tid; g < groups; g += PT) {
            const float4 v = in4[g];
            take(v.x); take(v.y); take(v.z); take(v.w);
        }
        const int done = head + 4 * groups;
        if (tid < n - done) take(in[done + tid]);
        peak = wave_max(peak);
        if ((tid & 63) == 0) red[tid >> 6] = peak;
        isnan = __syncthreads_or(isnan);
        peak = red[0];
        for (int w = 1; w < PT / 64; ++w) peak = fmaxf(peak, red[w]);
    }
    const bool scale = normalize && peak > 0.f && !isnan;   // all-zero row: unchanged, no 0 / 0
    // n > out_len: window [start, start + out_len), start = (n - out_len) / 2; n < out_len: left = (out_len - n) / 2
    const int shift = n >= out_len ? (n - out_len) / 2 : -((out_len - n) / 2);
    auto at = [&](int oi) {
        const int i = oi + shift;
        float v = 0.f;
        if (i >= 0 && i < n) {
            v = in[i];
            if (scale) v = v / peak;
        }
        return v;
    };
    const int head = min(out_len, head_to_16(o));
    if (tid < head) o[tid] = at(tid);
    const int groups = (out_len - head) >> 2;
    for (int g = tid; g < groups; g += PT) {
        const int oi = head + 4 * g, i = oi + shift;
        float4 v;
        if (i >= 0 && i + 3 < n) {
            v = load4_unaligned(in + i);
            if (scale) v = make_float4(v.x / peak, v.y / peak, v.z / peak, v.w / peak);
        } else {
            v = make_float4(at(oi), at(oi + 1), at(oi + 2), at(oi + 3));
        }
        *reinterpret_cast<float4*>(o + oi) = v;
    }
    const int done = head + 4 * groups;
    if (tid < out_len - done) o[done + tid] = at(done + tid);
}

// ------------------------------------------------------------------------------------------ per-image masks
// grid (image, chunk).  Threads 0 .. n_masks - 1 bring the image's mask triples into LDS (a triple that masks nothing --
// empty, or an axis that is neither 0 nor 1 -- becomes the empty row range [0, 0)); every thread then tests each of its
// elements against them.  in and out may be the same buffer: a thread reads what it writes and nothing else.
__global__ __launch_bounds__(GT) void mask_images_kernel(const float* in, float* out, int height, int width, int n_masks,
                                                         const int* __restrict__ axis, const int* __restrict__ start,
                                                         const int* __restrict__ end, int vec) {
    __shared__ int ax[COUGH_MAX_MASKS], lo[COUGH_MAX_MASKS], hi[COUGH_MAX_MASKS];
    const int img = blockIdx.x, tid = threadIdx.x;
    if (tid < n_masks) {
        const long long j = (long long)img * n_masks + tid;
        const int a = axis[j], s = start[j], e = end[j];
        const bool live = (a == 0 || a == 1) && e > s;
        ax[tid] = live ? a : 0;
        lo[tid] = live ? s : 0;
        hi[tid] = live ? e : 0;
    }
    __syncthreads();
    auto hit = [&](int row, int col) {
        bool h = false;
        for (int k = 0; k < n_masks; ++k) {
            const int i = ax[k] == 0 ? row : col;
            h = h || (i >= lo[k] && i < hi[k]);
        }
        return h;
    };
    const int hw = height * width;             // <= INT_MAX (checked by the caller)
    const long long base = (long long)img * hw;
    const float* pin = in + base;
    float* pout = out + base;
    const int gt = blockIdx.y * GT + tid, gthreads = gridDim.y * GT;
    auto one = [&](int e) {
        const int row = e / width, col = e - row * width;
        pout[e] = hit(row, col) ? 0.0f : pin[e];
    };
    if (!vec) {                                // a base pointer off 16 bytes, or in and out out of phase
        for (int e = gt; e < hw; e += gthreads) one(e);
        return;
    }
    const int head = min(hw, head_to_16(pout));   // pin has the same phase
    if (gt < head) one(gt);
    const int groups = (hw - head) >> 2;
    for (int g = gt; g < groups; g += gthreads) {
        const int e = head + 4 * g;
        int row = e / width, col = e - row * width;
        const float4 v = *reinterpret_cast<const float4*>(pin + e);
        float x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (col == width) {
                col = 0;
                ++row;
            }
            if (hit(row, col)) x[k] = 0.0f;
            ++col;
        }
        *reinterpret_cast<float4*>(pout + e) = make_float4(x[0], x[1], x[2], x[3]);
    }
    const int done = head + 4 * groups;
    if (gt < hw - done) one(done + gt);
}

// workgroups per row for `groups` float4 groups of GT threads each: all of them up to MAX_CHUNKS
unsigned chunks_for(long long groups) { return unsigned(std::clamp<long long>((groups + GT - 1) / GT, 1, MAX_CHUNKS)); }

}  // namespace
}  // namespace cough

extern "C" int cough_data_abi_version(void) { return COUGH_DATA_ABI_VERSION; }
// this library's own last-error slot (libcough_amd.so keeps its own behind cough_amd_last_error)
COUGH_DEFINE_LAST_ERROR(cough_data_last_error)

extern "C" int cough_gather_rows(const float* d_src, const long long* d_row_offsets, const int* d_lengths, int n_rows,
                                 float* d_out, long long out_stride, int row_len, void* stream) {
    using namespace cough;
    const char* fn = "cough_gather_rows";
    COUGH_REQUIRE(d_src && d_row_offsets && d_lengths && d_out, COUGH_EINVAL, "%s: NULL argument", fn);
    COUGH_REQUIRE(n_rows >= 0, COUGH_EINVAL, "%s: n_rows must not be negative, got %d", fn, n_rows);
    COUGH_REQUIRE(row_len >= 1, COUGH_EINVAL, "%s: row_len must be positive, got %d", fn, row_len);
    COUGH_REQUIRE(out_stride >= row_len, COUGH_EINVAL, "%s: out_stride %lld is shorter than row_len %d", fn, out_stride,
                  row_len);
    COUGH_REQUIRE(aligned(d_src, 4) && aligned(d_out, 4) && aligned(d_lengths, 4), COUGH_EINVAL,
                  "%s: float32 and int32 arrays must be 4-byte aligned", fn);
    COUGH_REQUIRE(aligned(d_row_offsets, 8), COUGH_EINVAL, "%s: d_row_offsets must be 8-byte aligned", fn);
    if (n_rows == 0) return COUGH_OK;
    hipLaunchKernelGGL(gather_rows_kernel, dim3(unsigned(n_rows), chunks_for(row_len / 4)), dim3(GT), 0,
                       static_cast<hipStream_t>(stream), d_src, d_row_offsets, d_lengths, d_out, out_stride, row_len);
    COUGH_HIP_CHECK(hipGetLastError());
    return COUGH_OK;
}

extern "C" int cough_prepare_rows(const float* d_src, const long long* d_row_offsets, const int* d_lengths, int n_rows,
                                  float* d_out, int out_len, int flags, void* stream) {
    using namespace cough;
    const char* fn = "cough_prepare_rows";
    COUGH_REQUIRE(d_src && d_row_offsets && d_lengths && d_out, COUGH_EINVAL, "%s: NULL argument", fn);
    COUGH_REQUIRE(n_rows >= 0, COUGH_EINVAL, "%s: n_rows must not be negative, got %d", fn, n_rows);
    COUGH_REQUIRE(out_len >= 1, COUGH_EINVAL, "%s: out_len must be positive, got %d", fn, out_len);
    COUGH_REQUIRE((flags & ~COUGH_PREP_NORMALIZE) == 0, COUGH_EINVAL, "%s: unknown flags 0x%x", fn, flags);
    COUGH_REQUIRE(aligned(d_src, 4) && aligned(d_out, 4) && aligned(d_lengths, 4), COUGH_EINVAL,
                  "%s: float32 and int32 arrays must be 4-byte aligned", fn);
    COUGH_REQUIRE(aligned(d_row_offsets, 8), COUGH_EINVAL, "%s: d_row_offsets must be 8-byte aligned", fn);
    if (n_rows == 0) return COUGH_OK;
    hipLaunchKernelGGL(prepare_rows_kernel, dim3(unsigned(n_rows)), dim3(PT), 0, static_cast<hipStream_t>(stream), d_src,
                       d_row_offsets, d_lengths, d_out, out_len, (flags & COUGH_PREP_NORMALIZE) ? 1 : 0);
    COUGH_HIP_CHECK(hipGetLastError());
    return COUGH_OK;
}

extern "C" int cough_mask_images(const float* d_in, float* d_out, int n_images, int height, int width, int n_masks,
                                 const int* d_axis, const int* d_start, const int* d_end, void* stream) {
    using namespace cough;
    const char* fn = "cough_mask_images";
    COUGH_REQUIRE(n_masks >= 0 && n_masks <= COUGH_MAX_MASKS, COUGH_EINVAL, "%s: n_masks = %d (0..%d)", fn, n_masks,
                  COUGH_MAX_MASKS);
    COUGH_REQUIRE(d_in && d_out && (n_masks == 0 || (d_axis && d_start && d_end)), COUGH_EINVAL, "%s: NULL argument", fn);
    COUGH_REQUIRE(n_images >= 0, COUGH_EINVAL, "%s: n_images must not be negative, got %d", fn, n_images);
    COUGH_REQUIRE(height >= 1 && width >= 1, COUGH_EINVAL, "%s: bad shape (%d x %d)", fn, height, width);
    COUGH_REQUIRE((long long)height * width <= INT_MAX, COUGH_EUNSUPPORTED, "%s: an image of %d x %d has more than 2^31 - 1 "
                  "elements", fn, height, width);
    COUGH_REQUIRE(aligned(d_in, 4) && aligned(d_out, 4) && aligned(d_axis, 4) && aligned(d_start, 4) && aligned(d_end, 4),
                  COUGH_EINVAL, "%s: float32 and int32 arrays must be 4-byte aligned", fn);
    if (n_images == 0) return COUGH_OK;
    // float4 access needs in and out in the same phase: both bases on 16 bytes (an image may still start off 16 bytes)
    const int vec = aligned(d_in, 16) && aligned(d_out, 16);
    hipLaunchKernelGGL(mask_images_kernel, dim3(unsigned(n_images), chunks_for((long long)height * width / 4)), dim3(GT), 0,
                       static_cast<hipStream_t>(stream), d_in, d_out, height, width, n_masks, d_axis, d_start, d_end, vec);
    COUGH_HIP_CHECK(hipGetLastError());
    return COUGH_OK;
}
