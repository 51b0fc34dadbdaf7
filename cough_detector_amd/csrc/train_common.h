// Pieces shared by the training steps of CoughDetectorResidual (train.hip), CoughDetectorSmall (train_small.hip) and
// CoughDetector (train_std.hip):
//   all three      the dropout keep draw, a clip's weighted CE terms and dlogits (the loss contract), the MFMA 32x32x2
//                  accumulator row, and the host side: workspace carving, launch grids and the entry points' shared checks
//   Residual, Std  the index-order reduction of the conv weight-gradient slabs
//   Small, Std     the pixel ranges of the partial sums, BN-apply, the pool's argmax, the two per-channel merges of the
//                  BatchNorm partials (forward: a fixed-order Chan tree of (count, mean, M2); backward: a fixed-order tree
//                  of (sum dy, sum dy * xhat)), and the two-layer classifier head (Linear, ReLU, Dropout, Linear)
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <initializer_list>

#include "common.h"
#include "philox.h"

namespace cough {
namespace {

constexpr int NT = 256;                     // threads of every block-reducing kernel

// MFMA 32x32x2 f32 operand / result layout: lane (r, h) supplies A[row r][k h] and B[k h][col r]; accumulator register
// reg of lane (r, h) is C[row (reg & 3) + 8 (reg >> 2) + 4 h][col r].
__device__ __forceinline__ int acc_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

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

// sum the S weight-gradient slabs [N][kp] in index order; column (kh, kw, ci) -> the OIHW weight gradient (KK taps),
// column kcols -> the bias gradient
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ slab, int S, int N, int kp, int kcols,
                                                           int C, int KK, float* __restrict__ gw, float* __restrict__ gb) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= N * (kcols + 1)) return;
    const int co = e / (kcols + 1), col = e - co * (kcols + 1);
    const float* p = slab + (long long)co * kp + col;
    float s = 0.f;
    for (int i = 0; i < S; ++i) s += p[(long long)i * N * kp];
    if (col == kcols) {
        gb[co] = s;
    } else {
        const int t = col / C, ci = col - t * C;
        gw[((long long)co * C + ci) * KK + t] = s;
    }
}

// ------------------------------------------------------------------------------------------ dropout and loss
// the Dropout keep of unit u of clip b: Philox counter (u / 4, clip, offset lo, offset hi), word u % 4; keep where u >= p
__device__ __forceinline__ float dropout_keep(int u, int b, unsigned long long seed, unsigned long long offset, float p) {
    const uint4 r = philox4x32_10(make_uint4(unsigned(u >> 2), unsigned(b), unsigned(offset), unsigned(offset >> 32)),
                                  make_uint2(unsigned(seed), unsigned(seed >> 32)));
    const unsigned v = (u & 3) == 0 ? r.x : (u & 3) == 1 ? r.y : (u & 3) == 2 ? r.z : r.w;
    return (float(v >> 8) * (1.0f / 16777216.0f) >= p) ? 1.f : 0.f;
}

// clip b's logits and weighted CE terms: wnll[2b] = w_y (logsumexp(z) - z_y), wnll[2b + 1] = w_y.  With soft targets
// (soft != nullptr: [B][2] class probabilities, torch's F.cross_entropy(z, y, weight=w) for a floating y; targets is then
// not read) wnll[2b] = -(w0 y0 lp0 + w1 y1 lp1) with lp_c = z_c - logsumexp(z), and wnll[2b + 1] = 1: the batch's loss
// divides by B, not by the sum of the weights.  Rows need not sum to 1; a NaN in a row gives a NaN loss.
__device__ __forceinline__ void ce_terms(int b, float z0, float z1, const long long* targets, const float* soft,
                                         const float* class_w, float* logits, float* wnll) {
    logits[2 * b] = z0;
    logits[2 * b + 1] = z1;
    if (soft) {
        const float mx = fmaxf(z0, z1);
        const float lse = mx + logf(expf(z0 - mx) + expf(z1 - mx));
        const float a0 = (class_w ? class_w[0] : 1.f) * soft[2 * b], a1 = (class_w ? class_w[1] : 1.f) * soft[2 * b + 1];
        wnll[2 * b] = -(a0 * (z0 - lse) + a1 * (z1 - lse));
        wnll[2 * b + 1] = 1.f;
        return;
    }
    const long long y = targets[b];
    if (y == 0 || y == 1) {
        const float mx = fmaxf(z0, z1);
        const float lse = mx + logf(expf(z0 - mx) + expf(z1 - mx));
        const float wt = class_w ? class_w[y] : 1.f;
        wnll[2 * b] = wt * (lse - (y ? z1 : z0));
        wnll[2 * b + 1] = wt;
    } else {                                // a target outside [0, 2): the loss is NaN (torch raises instead)
        wnll[2 * b] = __builtin_nanf("");
        wnll[2 * b + 1] = __builtin_nanf("");
    }
}

// dlogits of clip b: k (the clip's CE weight over the batch's total, formed by the caller) * (softmax(z) - onehot(y)); with
// soft targets k * (softmax(z) S - w_c y_c), S = w0 y0 + w1 y1 (k is then 1 / B).  The soft form multiplies e_c by inv * S
// so that a one-hot row without class weights (S = 1) is the hard expression operation by operation.
__device__ __forceinline__ float2 clip_dlogits(const float* logits, const long long* targets, const float* soft,
                                               const float* class_w, int b, float k) {
    const float z0 = logits[2 * b], z1 = logits[2 * b + 1];
    const float mx = fmaxf(z0, z1);
    const float e0 = expf(z0 - mx), e1 = expf(z1 - mx), inv = 1.0f / (e0 + e1);
    if (soft) {
        const float a0 = (class_w ? class_w[0] : 1.f) * soft[2 * b], a1 = (class_w ? class_w[1] : 1.f) * soft[2 * b + 1];
        const float inv_s = inv * (a0 + a1);
        return make_float2(k * (e0 * inv_s - a0), k * (e1 * inv_s - a1));
    }
    const long long y = targets[b];
    return make_float2(k * (e0 * inv - (y == 0 ? 1.f : 0.f)), k * (e1 * inv - (y == 1 ? 1.f : 0.f)));
}

// ------------------------------------------------------------------------------------------ two-layer head
// Linear(CIN, HID) -> ReLU -> Dropout(p) -> Linear(HID, 2) on a clip's CIN pooled features; CIN threads per clip.  The
// keep of hidden unit j of clip b is mask[b * MLD + MOFF + j].

// v[0] + v[s] + ... + v[(N - 1) s] as a pairwise tree: (v0 + v1) + (v2 + v3) for N = 4
template <int N>
__device__ __forceinline__ float pairwise_sum(const float* v, int s) {
    if constexpr (N == 1) return v[0];
    else return pairwise_sum<N / 2>(v, s) + pairwise_sum<N / 2>(v + N / 2 * s, s);
}

// hidden unit j before dropout: relu(b1[j] + sum over k of w1[j][k] x[k])
template <int CIN>
__device__ __forceinline__ float mlp_hidden(const float* w1, const float* b1, const float* x, int j) {
    float hv = b1[j];
    for (int k = 0; k < CIN; ++k) hv += w1[j * CIN + k] * x[k];
    return fmaxf(hv, 0.f);
}

// the output Linear on the dropped-out hidden units hd, then clip b's logits and CE terms
template <int HID>
__device__ __forceinline__ void mlp_out(const float* w2, const float* b2, const float* hd, int b, const long long* targets,
                                        const float* soft, const float* class_w, float* logits, float* wnll) {
    float z0 = b2[0], z1 = b2[1];
    for (int j = 0; j < HID; ++j) {
        z0 += w2[j] * hd[j];
        z1 += w2[HID + j] * hd[j];
    }
    ce_terms(b, z0, z1, targets, soft, class_w, logits, wnll);
}

// one block per clip: the batch's loss and CE weight (every block sums them in the same order, the CIN / 64 waves as a
// pairwise tree; block 0 writes the loss), dlogits, the hidden gradient dh (ReLU and dropout folded in) and dgap = the
// gradient of the pooled features over HW (the global mean's 1 / HW included).  st0 [2][C0]: the first BN's mean, invstd.
template <int CIN, int HID, int MLD, int MOFF>
__global__ __launch_bounds__(CIN) void mlp_head_bwd_kernel(int B, int HW, const float* __restrict__ logits,
                                                           const long long* __restrict__ targets,
                                                           const float* __restrict__ soft,
                                                           const float* __restrict__ class_w,
                                                           const float* __restrict__ wnll, const float* __restrict__ hr,
                                                           const float* __restrict__ mask, float p,
                                                           const float* __restrict__ w1, const float* __restrict__ w2,
                                                           const float* __restrict__ st0, int C0, float* __restrict__ loss,
                                                           float* __restrict__ dl, float* __restrict__ dh,
                                                           float* __restrict__ dgap) {
    __shared__ float lds[8], sdh[HID];
    const int t = threadIdx.x, b = blockIdx.x;
    float v0 = 0.f, v1 = 0.f;
    for (int i = t; i < B; i += CIN) { v0 += wnll[2 * i]; v1 += wnll[2 * i + 1]; }
    v0 = wave_sum(v0);
    v1 = wave_sum(v1);
    if ((t & 63) == 0) { lds[(t >> 6) * 2] = v0; lds[(t >> 6) * 2 + 1] = v1; }
    __syncthreads();
    const float tot = pairwise_sum<CIN / 64>(lds, 2), totw = pairwise_sum<CIN / 64>(lds + 1, 2);
    if (b == 0 && t == 0) {
        // a non-finite input reaches the first BN's batch statistics of every channel; ReLU and max-pool (v_max_f32)
        // would otherwise drop the NaN before the loss
        const bool finite = isfinite(st0[0]) && isfinite(st0[C0]);
        loss[0] = finite ? tot / totw : __builtin_nanf("");
    }
    const float2 d = clip_dlogits(logits, targets, soft, class_w, b, wnll[2 * b + 1] / totw);
    if (t == 0) { dl[2 * b] = d.x; dl[2 * b + 1] = d.y; }
    const float scale = p < 1.f ? 1.0f / (1.0f - p) : 0.f;
    if (t < HID) {
        const float dhd = d.x * w2[t] + d.y * w2[HID + t];
        const float g = hr[(long long)b * HID + t] > 0.f ? dhd * (mask[(long long)b * MLD + MOFF + t] * scale) : 0.f;
        sdh[t] = g;
        dh[(long long)b * HID + t] = g;
    }
    __syncthreads();
    float s = 0.f;
    for (int j = 0; j < HID; ++j) s += w1[j * CIN + t] * sdh[j];
    dgap[(long long)b * CIN + t] = s / float(HW);
}

// the head's gradients into g (w1 [HID][CIN], b1, w2 [2][HID], b2: contiguous in the parameters): 64 outputs per block,
// the batch split in 4 fixed quarters, added ((q0 + q1) + (q2 + q3))
template <int CIN, int HID, int MLD, int MOFF>
__global__ __launch_bounds__(NT) void mlp_fc_grad_kernel(int B, const float* __restrict__ gap, const float* __restrict__ hr,
                                                         const float* __restrict__ mask, float p,
                                                         const float* __restrict__ dl, const float* __restrict__ dh,
                                                         float* __restrict__ g) {
    constexpr int LC = __builtin_ctz(CIN);  // CIN is a power of two
    __shared__ float red[4][64];
    const int o = blockIdx.x * 64 + (threadIdx.x & 63), q = threadIdx.x >> 6;
    constexpr int NOUT = CIN * HID + HID + 2 * HID + 2;
    const int b0 = int((long long)B * q / 4), b1 = int((long long)B * (q + 1) / 4);
    const float scale = p < 1.f ? 1.0f / (1.0f - p) : 0.f;
    float s = 0.f;
    if (o < CIN * HID) {
        const int j = o >> LC, c = o & (CIN - 1);
        for (int b = b0; b < b1; ++b) s += dh[(long long)b * HID + j] * gap[(long long)b * CIN + c];
    } else if (o < CIN * HID + HID) {
        const int j = o - CIN * HID;
        for (int b = b0; b < b1; ++b) s += dh[(long long)b * HID + j];
    } else if (o < CIN * HID + 3 * HID) {
        const int k = (o - CIN * HID - HID) / HID, j = (o - CIN * HID - HID) % HID;
        for (int b = b0; b < b1; ++b)
            s += dl[2 * b + k] * (hr[(long long)b * HID + j] * (mask[(long long)b * MLD + MOFF + j] * scale));
    } else if (o < NOUT) {
        const int k = o - CIN * HID - 3 * HID;
        for (int b = b0; b < b1; ++b) s += dl[2 * b + k];
    }
    red[q][threadIdx.x & 63] = s;
    __syncthreads();
    if (q == 0 && o < NOUT) g[o] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// ------------------------------------------------------------------------------------------ host
size_t align256(size_t v) { return (v + 255) & ~size_t(255); }

// hands out 256-byte aligned pieces of a workspace in the order they are taken; with base == nullptr it only measures
struct Carver {
    char* base;
    size_t off = 0;
    char* take(size_t bytes) {
        char* p = base ? base + off : nullptr;
        off += align256(bytes);
        return p;
    }
    float* floats(long long n) { return reinterpret_cast<float*>(take(size_t(n) * 4)); }
};

// blocks of 256 threads for n elements of a grid-stride loop, at most cap
int grid_for(long long n, int cap) { return int(std::min<long long>((n + NT - 1) / NT, cap)); }

bool finite_f(float v) { return std::isfinite(v); }

// the checks every training step's entry point fn makes after its shape checks: the arguments every step needs, dropout
// probabilities in [0, 1], BatchNorm momentum / eps, the workspace's alignment and size (need bytes)
int check_step_args(const char* fn, std::initializer_list<const void*> args, std::initializer_list<float> ps, float momentum,
                    float eps, const void* ws, size_t ws_bytes, size_t need) {
    for (const void* a : args) COUGH_REQUIRE(a, COUGH_EINVAL, "%s: NULL argument", fn);
    for (const float p : ps) COUGH_REQUIRE(p >= 0.f && p <= 1.f, COUGH_EINVAL, "%s: dropout p must be in [0, 1]", fn);
    COUGH_REQUIRE(finite_f(momentum) && momentum >= 0.f && momentum <= 1.f && finite_f(eps) && eps >= 0.f, COUGH_EINVAL,
                  "%s: bad BatchNorm momentum / eps", fn);
    COUGH_REQUIRE((reinterpret_cast<size_t>(ws) & 255) == 0, COUGH_EINVAL, "%s: workspace must be 256-byte aligned", fn);
    COUGH_REQUIRE(ws_bytes >= need, COUGH_EWORKSPACE, "%s: workspace too small", fn);
    return COUGH_OK;
}

}  // namespace
}  // namespace cough
