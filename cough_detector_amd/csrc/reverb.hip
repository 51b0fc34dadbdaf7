// libcough_amd_reverb.so: room reverberation on the device (include/cough_amd_reverb.h).  Every row of a batch is
// convolved with a room impulse response of a prepared bank by FFT overlap-save; the transform never leaves the CU.
//
// Launch shape.  One workgroup of 1024 threads per (row, span of 16384 outputs).  The span's two overlap-save
// segments of 16384 inputs go into the real and the imaginary parts of one 16384-point complex float32 sequence that
// fills 128 KiB of LDS (the response is real, so the two results come back in the real and the imaginary parts: no
// split pass).  Seven radix-4 passes forward, decimation in frequency, in place: the spectrum is left in base-4
// digit-reversed order, which is the order cough_reverb_prepare stored H in -- transformed by the very same passes and
// pre-scaled by 1/16384 -- and the order the seven decimation-in-time passes of the inverse start from, so no pass
// reorders anything.  The last forward pass, the product with H and the first inverse pass work on the same four
// adjacent elements and run in registers: twelve LDS passes and fourteen barriers per span (two of them the load-time
// reductions of the non-finite and the silence predicate).
//
// LDS layout: z[i] at float2 index i in 128 KiB of dynamic LDS, besides the few static words the two workgroup
// reductions (__syncthreads_or) use.  In a pass of quarter
// length q a thread's butterflies read z[base + p q]; consecutive lanes take consecutive base, so the passes with
// q >= 64 are conflict-free 8-byte accesses.  The passes with q = 16 and q = 4 stride across banks (lanes 4 q elements
// apart in groups); the register pass reads 32 contiguous bytes per lane.
//
// Twiddles: tw[m] = exp(-2 pi i m / 16384), computed on the host in float64, rounded once, and kept in front of the
// spectra in the workspace; a pass of length M reads tw[p k (16384 / M)], p = 1 .. 3, which is at most 3/4 of the table
// and lives in L2 (128 KiB shared by every workgroup).
//
// HBM traffic per one-second row: the row in, the row out, one 128 KiB spectrum (from L2 / the Infinity Cache when the
// bank is small).
#include "../../include/cough_amd_reverb.h"

#include <cmath>
#include <cstdint>
#include <vector>

#include "common.h"
#include "philox.h"

namespace cough {

namespace {

constexpr int N = COUGH_REVERB_FFT, HALF = N / 2, RT = 1024, PER = N / 4 / RT;   // 4 butterflies per thread and pass
constexpr int MAX_LEN = COUGH_REVERB_MAX_LENGTH;
constexpr size_t SPEC_BYTES = size_t(N) * sizeof(float2);                          // the table, and one spectrum
constexpr int DT = 64;                                                             // threads of the draw kernel
static_assert(N == 16384 && PER == 4, "seven radix-4 passes of 4096 butterflies");

__device__ __forceinline__ float2 cmul(float2 a, float2 w) { return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x); }
__device__ __forceinline__ float2 cmulc(float2 a, float2 w) { return make_float2(a.x * w.x + a.y * w.y, a.y * w.x - a.x * w.y); }

// the 4-point DFT of (x0 .. x3) with exp(-2 pi i / 4) = -i: what a forward butterfly does before its twiddles
__device__ __forceinline__ void dft4(float2& x0, float2& x1, float2& x2, float2& x3) {
    const float2 a0 = make_float2(x0.x + x2.x, x0.y + x2.y), a1 = make_float2(x0.x - x2.x, x0.y - x2.y);
    const float2 a2 = make_float2(x1.x + x3.x, x1.y + x3.y), a3 = make_float2(x1.x - x3.x, x1.y - x3.y);
    x0 = make_float2(a0.x + a2.x, a0.y + a2.y);
    x2 = make_float2(a0.x - a2.x, a0.y - a2.y);
    x1 = make_float2(a1.x + a3.y, a1.y - a3.x);      // a1 - i a3
    x3 = make_float2(a1.x - a3.y, a1.y + a3.x);      // a1 + i a3
}
// its conjugate (the inverse up to the factor 4 that H's scaling carries)
__device__ __forceinline__ void idft4(float2& x0, float2& x1, float2& x2, float2& x3) {
    const float2 a0 = make_float2(x0.x + x2.x, x0.y + x2.y), a1 = make_float2(x0.x - x2.x, x0.y - x2.y);
    const float2 a2 = make_float2(x1.x + x3.x, x1.y + x3.y), a3 = make_float2(x1.x - x3.x, x1.y - x3.y);
    x0 = make_float2(a0.x + a2.x, a0.y + a2.y);
    x2 = make_float2(a0.x - a2.x, a0.y - a2.y);
    x1 = make_float2(a1.x - a3.y, a1.y + a3.x);      // a1 + i a3
    x3 = make_float2(a1.x + a3.y, a1.y - a3.x);      // a1 - i a3
}

// One decimation-in-frequency pass over sub-transforms of length 4 q: butterfly, then the twiddles W^(p k).
__device__ __forceinline__ void forward_pass(float2* z, const float2* __restrict__ tw, int q, int tid) {
    const int step = HALF / 2 / q;                    // 16384 / (4 q)
#pragma unroll
    for (int t = 0; t < PER; ++t) {
        const int j = tid + RT * t, k = j & (q - 1), base = ((j - k) << 2) + k;
        float2 x0 = z[base], x1 = z[base + q], x2 = z[base + 2 * q], x3 = z[base + 3 * q];
        dft4(x0, x1, x2, x3);
        z[base] = x0;
        z[base + q] = cmul(x1, tw[k * step]);
        z[base + 2 * q] = cmul(x2, tw[2 * k * step]);
        z[base + 3 * q] = cmul(x3, tw[3 * k * step]);
    }
}

// One decimation-in-time pass of the inverse: the conjugate twiddles, then the conjugate butterfly.
__device__ __forceinline__ void inverse_pass(float2* z, const float2* __restrict__ tw, int q, int tid) {
    const int step = HALF / 2 / q;
#pragma unroll
    for (int t = 0; t < PER; ++t) {
        const int j = tid + RT * t, k = j & (q - 1), base = ((j - k) << 2) + k;
        float2 x0 = z[base];
        float2 x1 = cmulc(z[base + q], tw[k * step]);
        float2 x2 = cmulc(z[base + 2 * q], tw[2 * k * step]);
        float2 x3 = cmulc(z[base + 3 * q], tw[3 * k * step]);
        idft4(x0, x1, x2, x3);
        z[base] = x0;
        z[base + q] = x1;
        z[base + 2 * q] = x2;
        z[base + 3 * q] = x3;
    }
}

// the six forward passes with q = 4096 .. 4; z complete and visible on entry, and on return
__device__ __forceinline__ void forward_to_quads(float2* z, const float2* __restrict__ tw, int tid) {
#pragma unroll 1
    for (int q = N / 4; q >= 4; q >>= 2) {
        forward_pass(z, tw, q, tid);
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------ the bank's spectra
// One workgroup: h zero-extended to 16384 real samples, the seven forward passes, the scaling by 2^-14.
__global__ __launch_bounds__(RT) void prepare_kernel(const float* __restrict__ taps, int L, const float2* __restrict__ tw,
                                                     float2* __restrict__ spectrum) {
    extern __shared__ float2 z[];
    const int tid = threadIdx.x;
    for (int i = tid; i < N; i += RT) z[i] = make_float2(i < L ? taps[i] : 0.0f, 0.0f);
    __syncthreads();
    forward_to_quads(z, tw, tid);
#pragma unroll
    for (int t = 0; t < PER; ++t) {
        const int base = 4 * (tid + RT * t);
        float2 x0 = z[base], x1 = z[base + 1], x2 = z[base + 2], x3 = z[base + 3];
        dft4(x0, x1, x2, x3);
        const float s = 1.0f / float(N);              // a power of two: exact
        spectrum[base] = make_float2(x0.x * s, x0.y * s);
        spectrum[base + 1] = make_float2(x1.x * s, x1.y * s);
        spectrum[base + 2] = make_float2(x2.x * s, x2.y * s);
        spectrum[base + 3] = make_float2(x3.x * s, x3.y * s);
    }
}

// ------------------------------------------------------------------------------------------ the rows
__global__ __launch_bounds__(RT) void reverb_kernel(const float* __restrict__ src, const long long* __restrict__ row_offsets,
                                                    const int* __restrict__ lengths, const cough_reverb_plan* __restrict__ plans,
                                                    const float2* __restrict__ tw, const float2* __restrict__ spectra, int n_rirs,
                                                    float* __restrict__ out, int width, int n_spans) {
    extern __shared__ float2 z[];
    const int tid = threadIdx.x;
    const int b = int(blockIdx.x) / n_spans, w = int(blockIdx.x) - b * n_spans;
    const int n = min(max(lengths[b], 0), MAX_LEN);
    const cough_reverb_plan plan = plans[b];
    const int shift = min(max(plan.shift, -n), n);
    const int out_len = min(max(plan.out_len, 0), width);
    const int rir = (plan.rir >= 0 && plan.rir < n_rirs) ? plan.rir : -1;
    const float* x = src + row_offsets[b];
    float* o = out + (long long)b * width;
    const int s = w * N, span_end = min(s + N, width);           // this workgroup writes columns s .. span_end-1

    auto shifted = [&](int i) {                // x_s[i], any i
        if (i < 0 || i >= n) return 0.0f;
        const int j = i - shift;
        return (j >= 0 && j < n) ? x[j] : 0.0f;
    };

    if (rir < 0) {                             // a (shifted) copy of min(n, out_len) samples
        const int kept = min(n, out_len);
        for (int m = s + tid; m < span_end; m += RT) o[m] = m < kept ? shifted(m) : 0.0f;
        return;
    }
    if (s >= out_len) {                        // padding columns only
        for (int m = s + tid; m < span_end; m += RT) o[m] = 0.0f;
        return;
    }

    // ---- load: segment a = x_s[s - 8192 ..] into the real parts, segment b, 8192 later, into the imaginary parts
    int bad = 0, live = 0;
    for (int i = tid; i < N; i += RT) {
        const float va = shifted(s - HALF + i), vb = shifted(s + i);
        bad |= !(fabsf(va) <= 3.4028234663852886e38f) | !(fabsf(vb) <= 3.4028234663852886e38f);     // NaN or Inf
        live |= (va != 0.0f) | (vb != 0.0f);
        z[i] = make_float2(va, vb);
    }
    // __syncthreads_or reduces ONE predicate (it returns the OR of !!p): the two flags take a reduction each
    const bool any_bad = __syncthreads_or(bad) != 0;      // also makes z visible
    const bool any_live = __syncthreads_or(live) != 0;
    if (any_bad || !any_live) {                // a non-finite input: NaN; silence: +0.0
        const float fill = any_bad ? __int_as_float(0x7FC00000) : 0.0f;
        for (int m = s + tid; m < span_end; m += RT) o[m] = m < out_len ? fill : 0.0f;
        return;
    }

    forward_to_quads(z, tw, tid);
    // ---- the last forward pass, the product with H and the first inverse pass, on four adjacent elements
    const float2* __restrict__ H = spectra + size_t(rir) * N;
#pragma unroll
    for (int t = 0; t < PER; ++t) {
        const int base = 4 * (tid + RT * t);
        float2 x0 = z[base], x1 = z[base + 1], x2 = z[base + 2], x3 = z[base + 3];
        dft4(x0, x1, x2, x3);
        x0 = cmul(x0, H[base]);
        x1 = cmul(x1, H[base + 1]);
        x2 = cmul(x2, H[base + 2]);
        x3 = cmul(x3, H[base + 3]);
        idft4(x0, x1, x2, x3);
        z[base] = x0;
        z[base + 1] = x1;
        z[base + 2] = x2;
        z[base + 3] = x3;
    }
    __syncthreads();
#pragma unroll 1
    for (int q = 4; q <= N / 4; q <<= 2) {
        inverse_pass(z, tw, q, tid);
        __syncthreads();
    }

    // ---- positions 8192 .. 16383: the real parts are y[s ..], the imaginary parts y[s + 8192 ..]
    for (int p = tid; p < HALF; p += RT) {
        const float2 v = z[HALF + p];
        const int m0 = s + p, m1 = s + HALF + p;
        if (m0 < span_end) o[m0] = m0 < out_len ? v.x : 0.0f;
        if (m1 < span_end) o[m1] = m1 < out_len ? v.y : 0.0f;
    }
}

// ------------------------------------------------------------------------------------------ the reverb draws of one row
// The contract of cough_amd_reverb.h, operator by operator; tests/reverb_ref.py restates it in numpy.
__global__ __launch_bounds__(DT) void draw_reverb_kernel(unsigned long long seed, int n_rows, const int* __restrict__ lengths,
                                                         double p, int n_rirs, cough_reverb_plan* __restrict__ plans) {
#pragma clang fp contract(off)
    const int row = blockIdx.x * DT + threadIdx.x;
    if (row >= n_rows) return;
    const uint2 key = make_uint2(unsigned(seed), unsigned(seed >> 32));
    auto unit = [](unsigned x) { return (double(x) + 0.5) * 0x1p-32; };
    const int n = min(max(lengths[row], 0), MAX_LEN);
    cough_reverb_plan plan;
    plan.shift = 0;
    plan.rir = -1;
    plan.out_len = n;
    plan.reserved = 0;
    if (n >= 1 && n_rirs >= 1) {
        const uint4 d = philox4x32_10(make_uint4(0u, unsigned(row), 0u, 4u), key);
        if (unit(d.x) <= p) plan.rir = min(int(double(n_rirs) * unit(d.y)), n_rirs - 1);
    }
    plans[row] = plan;
}

// exp(-2 pi i m / 16384) in float64, rounded once: computed on the first call, then kept
const std::vector<float2>& twiddles() {
    static const std::vector<float2> table = [] {
        std::vector<float2> t(N);
        for (int m = 0; m < N; ++m) {
            const double a = -2.0 * M_PI * double(m) / double(N);
            t[m] = make_float2(float(std::cos(a)), float(std::sin(a)));
        }
        return t;
    }();
    return table;
}

// 128 KiB of dynamic LDS is a per-device attribute of each kernel: set once per thread and device
int allow_lds() {
    thread_local int allowed_on = -1;
    int dev = 0;
    COUGH_HIP_CHECK(hipGetDevice(&dev));
    if (dev == allowed_on) return COUGH_OK;
    COUGH_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&prepare_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        int(SPEC_BYTES)));
    COUGH_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&reverb_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        int(SPEC_BYTES)));
    allowed_on = dev;
    return COUGH_OK;
}

}  // namespace
}  // namespace cough

extern "C" int cough_reverb_abi_version(void) { return COUGH_REVERB_ABI_VERSION; }
// this library's own last-error slot
COUGH_DEFINE_LAST_ERROR(cough_reverb_last_error)

extern "C" size_t cough_reverb_bank_bytes(int n_rirs) {
    if (n_rirs < 0 || size_t(n_rirs) > (SIZE_MAX / cough::SPEC_BYTES) - 1) return 0;
    return cough::SPEC_BYTES * (size_t(n_rirs) + 1);
}

extern "C" int cough_reverb_prepare(const float* d_taps, const long long* h_offsets, const int* h_lengths, int n_rirs,
                                    void* d_workspace, size_t workspace_bytes, void* stream) {
    using namespace cough;
    const char* fn = "cough_reverb_prepare";
    COUGH_REQUIRE(n_rirs >= 0, COUGH_EINVAL, "%s: n_rirs must not be negative, got %d", fn, n_rirs);
    COUGH_REQUIRE(d_workspace, COUGH_EINVAL, "%s: NULL workspace", fn);
    COUGH_REQUIRE(aligned(d_workspace, 256), COUGH_EINVAL, "%s: the workspace must be 256-byte aligned", fn);
    const size_t need = cough_reverb_bank_bytes(n_rirs);
    COUGH_REQUIRE(need != 0 && workspace_bytes >= need, COUGH_EWORKSPACE, "%s: the workspace holds %zu bytes, %zu are needed", fn,
                  workspace_bytes, need);
    if (n_rirs > 0) {
        COUGH_REQUIRE(d_taps && h_offsets && h_lengths, COUGH_EINVAL, "%s: NULL argument", fn);
        COUGH_REQUIRE(aligned(d_taps, 4), COUGH_EINVAL, "%s: d_taps must be 4-byte aligned", fn);
    }
    for (int r = 0; r < n_rirs; ++r) {
        COUGH_REQUIRE(h_lengths[r] >= 1 && h_offsets[r] >= 0, COUGH_EINVAL, "%s: response %d has %d taps at offset %lld", fn, r,
                      h_lengths[r], h_offsets[r]);
        COUGH_REQUIRE(h_lengths[r] <= COUGH_REVERB_MAX_TAPS, COUGH_EUNSUPPORTED, "%s: response %d has %d taps, at most %d fit", fn, r,
                      h_lengths[r], COUGH_REVERB_MAX_TAPS);
    }
    if (const int e = allow_lds()) return e;
    hipStream_t st = static_cast<hipStream_t>(stream);
    float2* tw = static_cast<float2*>(d_workspace);
    COUGH_HIP_CHECK(hipMemcpyAsync(tw, twiddles().data(), SPEC_BYTES, hipMemcpyHostToDevice, st));
    for (int r = 0; r < n_rirs; ++r)
        hipLaunchKernelGGL(prepare_kernel, dim3(1), dim3(RT), SPEC_BYTES, st, d_taps + h_offsets[r], h_lengths[r], tw,
                           tw + size_t(r + 1) * N);
    COUGH_HIP_CHECK(hipGetLastError());
    return COUGH_OK;
}

extern "C" int cough_reverb_rows(const float* d_src, const long long* d_row_offsets, const int* d_lengths, int n_rows,
                                 const cough_reverb_plan* d_plans, const void* d_workspace, int n_rirs, float* d_out, int width,
                                 void* stream) {
    using namespace cough;
    const char* fn = "cough_reverb_rows";
    COUGH_REQUIRE(n_rows >= 0 && width >= 1 && n_rirs >= 0, COUGH_EINVAL, "%s: bad sizes (%d rows of %d columns, %d responses)", fn,
                  n_rows, width, n_rirs);
    COUGH_REQUIRE(width <= COUGH_REVERB_MAX_LENGTH, COUGH_EUNSUPPORTED, "%s: width = %d is more than 2^30", fn, width);
    const int n_spans = (width + N - 1) / N;
    COUGH_REQUIRE((long long)n_rows * n_spans <= (1 << 24), COUGH_EUNSUPPORTED,
                  "%s: %d rows of %d spans are more than 2^24 blocks; split the batch", fn, n_rows, n_spans);
    if (n_rows == 0) return COUGH_OK;
    COUGH_REQUIRE(d_src && d_row_offsets && d_lengths && d_plans && d_workspace && d_out, COUGH_EINVAL, "%s: NULL argument", fn);
    COUGH_REQUIRE(d_out != d_src, COUGH_EINVAL, "%s: d_out must not alias d_src", fn);
    COUGH_REQUIRE(aligned(d_src, 4) && aligned(d_out, 4) && aligned(d_lengths, 4) && aligned(d_plans, 4), COUGH_EINVAL,
                  "%s: float32 and int32 arrays must be 4-byte aligned", fn);
    COUGH_REQUIRE(aligned(d_row_offsets, 8) && aligned(d_workspace, 256), COUGH_EINVAL,
                  "%s: d_row_offsets must be 8-byte and the workspace 256-byte aligned", fn);
    if (const int e = allow_lds()) return e;
    const float2* tw = static_cast<const float2*>(d_workspace);
    hipLaunchKernelGGL(reverb_kernel, dim3(unsigned(n_rows * n_spans)), dim3(RT), SPEC_BYTES, static_cast<hipStream_t>(stream), d_src,
                       d_row_offsets, d_lengths, d_plans, tw, tw + N, n_rirs, d_out, width, n_spans);
    COUGH_HIP_CHECK(hipGetLastError());
    return COUGH_OK;
}

extern "C" int cough_draw_reverb(unsigned long long seed, int n_rows, const int* d_lengths, double p_augment, int n_rirs,
                                 cough_reverb_plan* d_plans_out, void* stream) {
    using namespace cough;
    const char* fn = "cough_draw_reverb";
    COUGH_REQUIRE(n_rows >= 0 && n_rirs >= 0, COUGH_EINVAL, "%s: bad sizes (%d rows, %d responses)", fn, n_rows, n_rirs);
    COUGH_REQUIRE(p_augment >= 0.0 && p_augment <= 1.0, COUGH_EINVAL, "%s: p_augment = %g (0..1)", fn, p_augment);
    if (n_rows == 0) return COUGH_OK;
    COUGH_REQUIRE(d_lengths && d_plans_out, COUGH_EINVAL, "%s: NULL argument", fn);
    COUGH_REQUIRE(aligned(d_lengths, 4) && aligned(d_plans_out, 4), COUGH_EINVAL, "%s: int32 arrays must be 4-byte aligned", fn);
    hipLaunchKernelGGL(draw_reverb_kernel, dim3(unsigned((n_rows + DT - 1) / DT)), dim3(DT), 0, static_cast<hipStream_t>(stream), seed,
                       n_rows, d_lengths, p_augment, n_rirs, d_plans_out);
    COUGH_HIP_CHECK(hipGetLastError());
    return COUGH_OK;
}
