// libcough_amd_soft.so: training on soft targets (include/cough_amd_soft.h).  The three *_forward_backward_soft entry
// points are not here: they come from train.hip, train_small.hip and train_std.hip, compiled a second time with
// -DCOUGH_SOFT_EXPORTS, so the step code exists once.  This file holds the library's version, its last-error slot and
// cough_mix_batch.
//
// Access width of the mix kernel.  It streams 2 reads and 1 write per element, nothing is reused: 16 bytes per lane.  A row
// starts at element row * row_len, so with row_len = 90 * 101 = 9090 every other row starts 8 bytes off a 16-byte
// boundary, and a row's partner may sit differently from the row itself.  Each row is therefore cut where ITS OUTPUT is
// 16-byte aligned: up to 3 scalar elements in front, float4 stores over the body, up to 3 scalar elements behind.  The two
// reads of a body chunk are one 16-byte load where their address is 16-byte aligned, two 8-byte loads where it is 8-byte
// aligned and four 4-byte loads otherwise; which of the three is uniform over the block (it depends on the row alone).
#include "../../include/cough_amd_soft.h"

#include <algorithm>
#include <cstdint>

#include "common.h"

namespace cough {

namespace {

constexpr int MIX_THREADS = 256;
constexpr int MIX_MAX_X = 16;       // blocks along a row: 16 * 256 lanes * 16 bytes = 64 KiB of a row per sweep

// 4 consecutive floats at p (4-byte aligned), read as wide as p's alignment allows; al = address mod 16
__device__ __forceinline__ float4 load4(const float* p, unsigned al) {
    if (al == 0) return *reinterpret_cast<const float4*>(p);
    if (al == 8) {
        const float2 lo = *reinterpret_cast<const float2*>(p), hi = *reinterpret_cast<const float2*>(p + 2);
        return make_float4(lo.x, lo.y, hi.x, hi.y);
    }
    return make_float4(p[0], p[1], p[2], p[3]);
}

// cough_mix_rows' arithmetic: each product rounded on its own, then one add
__device__ __forceinline__ float mix1(float a, float x, float c, float y) { return mul_rn(a, x) + mul_rn(c, y); }

// grid (blocks along the row, rows): row = blockIdx.y + 65535 * blockIdx.z
__global__ __launch_bounds__(MIX_THREADS) void mix_batch_kernel(const float* __restrict__ x, const long long* __restrict__ labels,
                                                                const int* __restrict__ perm, const float2* __restrict__ coef,
                                                                int n_rows, long long n, float* __restrict__ out,
                                                                float* __restrict__ soft) {
    const long long row = blockIdx.y + (long long)blockIdx.z * 65535;
    if (row >= n_rows) return;
    const int pr = perm[row];
    const bool partner = pr >= 0 && pr < n_rows;     // otherwise the row is copied as it is
    const float2 ac = coef[row];
    if (blockIdx.x == 0 && threadIdx.x < 2) {
        const int c = threadIdx.x;
        const float y1 = labels[row] == c ? 1.f : 0.f;
        soft[2 * row + c] = partner ? mix1(ac.x, y1, ac.y, labels[pr] == c ? 1.f : 0.f) : y1;
    }
    const float* a = x + row * n;
    const float* b = x + (partner ? (long long)pr : row) * n;
    float* d = out + row * n;
    const long long t = (long long)blockIdx.x * MIX_THREADS + threadIdx.x, T = (long long)gridDim.x * MIX_THREADS;
    // [0, head): in front of the output row's first 16-byte boundary; [head, head + 4 * nv): the float4 body; the rest: tail
    const long long lead = (long long)((16u - unsigned(reinterpret_cast<uintptr_t>(d) & 15u)) & 15u) >> 2;
    const long long head = lead < n ? lead : n;
    const long long nv = (n - head) >> 2, tail0 = head + 4 * nv;
    const unsigned al_a = unsigned(reinterpret_cast<uintptr_t>(a + head) & 15u), al_b = unsigned(reinterpret_cast<uintptr_t>(b + head) & 15u);
    if (partner) {
        for (long long i = t; i < nv; i += T) {
            const float4 u = load4(a + head + 4 * i, al_a), v = load4(b + head + 4 * i, al_b);
            *reinterpret_cast<float4*>(d + head + 4 * i) = make_float4(mix1(ac.x, u.x, ac.y, v.x), mix1(ac.x, u.y, ac.y, v.y),
                                                                       mix1(ac.x, u.z, ac.y, v.z), mix1(ac.x, u.w, ac.y, v.w));
        }
        for (long long i = t; i < head + (n - tail0); i += T) {
            const long long e = i < head ? i : tail0 + (i - head);
            d[e] = mix1(ac.x, a[e], ac.y, b[e]);
        }
    } else {
        for (long long i = t; i < nv; i += T) *reinterpret_cast<float4*>(d + head + 4 * i) = load4(a + head + 4 * i, al_a);
        for (long long i = t; i < head + (n - tail0); i += T) {
            const long long e = i < head ? i : tail0 + (i - head);
            d[e] = a[e];
        }
    }
}

}  // namespace
}  // namespace cough

extern "C" int cough_soft_abi_version(void) { return COUGH_SOFT_ABI_VERSION; }
// this library's own last-error slot (libcough_amd.so keeps its own behind cough_amd_last_error)
COUGH_DEFINE_LAST_ERROR(cough_soft_last_error)

extern "C" int cough_mix_batch(const float* d_x, const long long* d_labels, const int* d_perm, const float* d_coef, int n_rows,
                               long long row_len, float* d_out, float* d_soft, void* stream) {
    using namespace cough;
    COUGH_REQUIRE(d_x && d_labels && d_perm && d_coef && d_out && d_soft, COUGH_EINVAL, "cough_mix_batch: NULL argument");
    COUGH_REQUIRE(n_rows >= 1 && row_len >= 1, COUGH_EINVAL, "cough_mix_batch: bad sizes (%d rows of %lld)", n_rows, row_len);
    COUGH_REQUIRE(d_out != d_x, COUGH_EINVAL, "cough_mix_batch: d_out must not alias d_x");
    COUGH_REQUIRE(((reinterpret_cast<uintptr_t>(d_x) | reinterpret_cast<uintptr_t>(d_out) | reinterpret_cast<uintptr_t>(d_soft)
                    | reinterpret_cast<uintptr_t>(d_perm)) & 3) == 0 && (reinterpret_cast<uintptr_t>(d_coef) & 7) == 0
                      && (reinterpret_cast<uintptr_t>(d_labels) & 7) == 0,
                  COUGH_EINVAL, "cough_mix_batch: misaligned argument");
    const long long chunks = (row_len + 4LL * MIX_THREADS - 1) / (4LL * MIX_THREADS);
    const unsigned gx = unsigned(std::min<long long>(chunks, MIX_MAX_X));
    const unsigned gy = unsigned(std::min(n_rows, 65535)), gz = unsigned((n_rows + 65534LL) / 65535);
    hipLaunchKernelGGL(mix_batch_kernel, dim3(gx, gy, gz), dim3(MIX_THREADS), 0, static_cast<hipStream_t>(stream), d_x, d_labels,
                       d_perm, reinterpret_cast<const float2*>(d_coef), n_rows, row_len, d_out, d_soft);
    COUGH_HIP_CHECK(hipGetLastError());
    return COUGH_OK;
}
