// Pieces shared verbatim by the training steps of CoughDetectorSmall (train_small.hip) and CoughDetector
// (train_std.hip): the pixel ranges of the partial sums, BN-apply, the pool's argmax, and the two per-channel merges of
// the BatchNorm partials (forward: a fixed-order Chan tree of (count, mean, M2); backward: a fixed-order tree of
// (sum dy, sum dy * xhat)).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace cough {
namespace {

constexpr int NT = 256;                     // threads of every block-reducing kernel

__device__ __forceinline__ long long range_lo(int s, int S, long long M) { return M * s / S; }

__device__ __forceinline__ float bn_act(float z, const float* st, const float* g, const float* bt, int c, int C) {
    return (z - st[c]) * st[C + c] * g[c] + bt[c];
}

// first index of the largest of a[0..3] (torch's max_pool2d keeps the first of equal values)
__device__ __forceinline__ int argmax4(const float (&a)[4]) {
    int k = 0;
#pragma unroll
    for (int j = 1; j < 4; ++j)
        if (a[j] > a[k]) k = j;
    return k;
}

struct Chan {
    double n, mean, m2;
};
__device__ __forceinline__ Chan chan_merge(Chan a, Chan b) {
    if (b.n == 0.0) return a;
    if (a.n == 0.0) return b;
    const double n = a.n + b.n, d = b.mean - a.mean;
    return Chan{n, a.mean + d * b.n / n, a.m2 + b.m2 + d * d * a.n * b.n / n};
}

// one block per channel: thread t merges ranges t, t + 256, ... in order, then a fixed pairwise tree.  Batch mean /
// invstd -> stat[0..1], running statistics (momentum, unbiased variance), num_batches_tracked + 1.
__global__ __launch_bounds__(NT) void stats_finalize_kernel(const float* __restrict__ part, int S, int C, float eps,
                                                            float momentum, float* __restrict__ run_mean,
                                                            float* __restrict__ run_var, long long* __restrict__ nbt,
                                                            float* __restrict__ stat) {
    __shared__ double sh[3][NT];
    const int c = blockIdx.x, t = threadIdx.x;
    Chan a{0.0, 0.0, 0.0};
    for (int i = t; i < S; i += NT) {
        const float* p = part + ((long long)i * C + c) * 3;
        a = chan_merge(a, Chan{double(p[0]), double(p[1]), double(p[2])});
    }
    sh[0][t] = a.n; sh[1][t] = a.mean; sh[2][t] = a.m2;
    __syncthreads();
    for (int off = NT / 2; off > 0; off >>= 1) {
        if (t < off) {
            const Chan m = chan_merge(Chan{sh[0][t], sh[1][t], sh[2][t]}, Chan{sh[0][t + off], sh[1][t + off], sh[2][t + off]});
            sh[0][t] = m.n; sh[1][t] = m.mean; sh[2][t] = m.m2;
        }
        __syncthreads();
    }
    if (t == 0) {
        const double n = sh[0][0], mean = sh[1][0], m2 = sh[2][0];
        const float var = float(m2 / n), uvar = float(m2 / (n - 1.0)), mu = float(mean);
        stat[c] = mu;
        stat[C + c] = 1.0f / sqrtf(var + eps);
        run_mean[c] = momentum * mu + (1.0f - momentum) * run_mean[c];
        run_var[c] = momentum * uvar + (1.0f - momentum) * run_var[c];
        if (c == 0) nbt[0] += 1;
    }
}

// one block per channel: the S ranges summed (thread t: ranges t, t + 256, ...; then a fixed tree) -> stat[2..3],
// dgamma = sum dy * xhat, dbeta = sum dy
__global__ __launch_bounds__(NT) void bn_bwd_finalize_kernel(const float* __restrict__ part, int S, int C,
                                                             float* __restrict__ stat, float* __restrict__ dgamma,
                                                             float* __restrict__ dbeta) {
    __shared__ double sh[2][NT];
    const int c = blockIdx.x, t = threadIdx.x;
    double s = 0.0, sx = 0.0;
    for (int i = t; i < S; i += NT) {
        s += part[((long long)i * C + c) * 2];
        sx += part[((long long)i * C + c) * 2 + 1];
    }
    sh[0][t] = s; sh[1][t] = sx;
    __syncthreads();
    for (int off = NT / 2; off > 0; off >>= 1) {
        if (t < off) { sh[0][t] += sh[0][t + off]; sh[1][t] += sh[1][t + off]; }
        __syncthreads();
    }
    if (t == 0) {
        const float fs = float(sh[0][0]), fsx = float(sh[1][0]);
        stat[2 * C + c] = fs;
        stat[3 * C + c] = fsx;
        dgamma[c] = fsx;
        dbeta[c] = fs;
    }
}

}  // namespace
}  // namespace cough
