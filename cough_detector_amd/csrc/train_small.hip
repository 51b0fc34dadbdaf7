// Training step of CoughDetectorSmall for gfx950: the train-mode forward pass, the backward pass, as the reference's
// train_epoch takes one step (/root/reference/src/train.py:54-112, model src/model.py:144-207).  clip_grad_norm_ + AdamW
// run in cough_adamw_step (train.hip), unchanged: it works on any flat parameter buffer.
//
//   features   conv3x3(1->16) BN ReLU maxpool2 | 3 x [dw3x3 -> pw1x1 -> BN ReLU (maxpool2 on the first two)] | mean
//   classifier Linear(128, 64) ReLU Dropout(p) Linear(64, 2); weighted CrossEntropyLoss
//
// Everything is exact f32 on VALU (f32 MFMA issues at the VALU rate on gfx950, and the depthwise convolutions have no
// GEMM shape).  Activations are planar [B][C][h][w].  Parameters, gradients and running statistics are flat caller
// buffers in model.parameters() / model.buffers() order.
//
//   conv1      never stored: its pre-BN output (16 x H x W per clip) is 16x the input image, so the statistics pass, the
//              BN-ReLU-pool pass, BN1's backward and conv1's weight gradient each recompute it from x, one 2x2 pool
//              window per thread (a 4x4 patch of x gives the window's four outputs)
//   dw + pw    one forward kernel per block (the dw output is kept: it is the pw weight gradient's input)
//   BatchNorm  per-range (count, mean, centred M2) partials, merged per channel by a 256-thread fixed-order Chan tree;
//              backward sums dy and dy * xhat the same way.  A pooled BN's dy is non-zero only at the argmax of each
//              window, which both the partial sums and the dz pass recompute from z with the same arithmetic
//   wgrad      every conv's weight and bias gradient is summed over S fixed pixel ranges into one slab [S][12256]; a
//              single launch at the end adds the S rows in index order, 4 interleaved lanes per output
//   head       one workgroup per clip forward (mean, Linear, ReLU, dropout, Linear, CE terms) and backward (every block
//              sums the batch's CE weights in the same order); the Linear gradients split the batch in 4 fixed quarters
// No float atomics; every reduction runs in a fixed order, so the same inputs and state give bit-identical results.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>

#include "common.h"
#include "train_common.h"

namespace cough {
namespace {

constexpr int NC[4] = {16, 32, 64, 128};   // channels of BN k (conv1, then the three pw convs)
constexpr int HID = 64;                     // classifier hidden width
// model.parameters() offsets (26 tensors, 21122 values)
constexpr int CONV1_W = 0, CONV1_B = 144;
constexpr int DW_W[4] = {0, 192, 960, 3520}, DW_B[4] = {0, 336, 1248, 4096};
constexpr int PW_W[4] = {0, 352, 1280, 4160}, PW_B[4] = {0, 864, 3328, 12352};
constexpr int BN_G[4] = {160, 896, 3392, 12480}, BN_B[4] = {176, 928, 3456, 12608};
constexpr int FC1_W = 12736, FC1_B = 20928, FC2_W = 20992, FC2_B = 21120, N_PARAMS = 21122;
constexpr int RUN[4] = {0, 32, 96, 224}, N_RUNNING = 480;
// the conv weights + biases (contiguous in the parameters) as rows of the wgrad slab: conv1, dw1, pw1, dw2, pw2, dw3, pw3
static_assert(FC2_B + 2 == N_PARAMS && RUN[3] + 2 * NC[3] == N_RUNNING, "parameter / running-statistics layout");
constexpr int NSEG = 7;
constexpr int SEG_SLAB[NSEG] = {0, 160, 320, 864, 1184, 3296, 3936};
constexpr int SEG_PARAM[NSEG] = {0, 192, 352, 960, 1280, 3520, 4160};
constexpr int SLAB_N = 12256;
__host__ __device__ constexpr int seg_dw(int k) { return 2 * k - 1; }
__host__ __device__ constexpr int seg_pw(int k) { return 2 * k; }

constexpr int TP = 32;                      // pw wgrad: pixels per LDS tile


// v[i] summed over the 256 threads of the block in a fixed order; every thread gets the sums
template <int N>
__device__ __forceinline__ void block_sum(float (&v)[N], float* lds /* [4 * N] */) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = wave_sum(v[i]);
    if (lane == 0)
#pragma unroll
        for (int i = 0; i < N; ++i) lds[wave * N + i] = v[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = (lds[i] + lds[N + i]) + (lds[2 * N + i] + lds[3 * N + i]);
    __syncthreads();
}

// v[i] of a thread-dependent i without dynamic indexing of a private array (which would go to scratch)
template <int N>
__device__ __forceinline__ float pick(const float (&v)[N], int i) {
    float r = 0.f;
#pragma unroll
    for (int j = 0; j < N; ++j) r = j == i ? v[j] : r;
    return r;
}


// ------------------------------------------------------------------------------------------ conv1, recomputed
// a pool window of conv1's output: rows 2wy, 2wy+1 and columns 2wx, 2wx+1 (those inside the image) read the 4x4 patch
// of x at rows 2wy-1 .. 2wy+2, columns 2wx-1 .. 2wx+2 (zero outside)
struct Patch {
    float v[4][4];
};
__device__ __forceinline__ Patch load_patch(const float* x, int H, int W, int b, int wy, int wx) {
    Patch p;
    const float* src = x + (long long)b * H * W;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int y = 2 * wy - 1 + i, xx = 2 * wx - 1 + j;
            p.v[i][j] = (y >= 0 && y < H && xx >= 0 && xx < W) ? src[y * W + xx] : 0.f;
        }
    return p;
}
// conv1 output of channel c at window position q = dy * 2 + dx
__device__ __forceinline__ float conv1_at(const Patch& p, const float* prm, int c, int q) {
    const int oy = q >> 1, ox = q & 1;
    float s = prm[CONV1_B + c];
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) s += prm[CONV1_W + c * 9 + kh * 3 + kw] * p.v[oy + kh][ox + kw];
    return s;
}


// ------------------------------------------------------------------------------------------ BN statistics
// part[s][C][3] = (count, mean, centred sum of squares) of range s.  Stage 0: windows of conv1's output, 4 channels per
// block (blockIdx.y = channel group); count = the valid pixels of the range's windows.
__global__ __launch_bounds__(NT) void stats0_kernel(const float* __restrict__ x, int B, int H, int W,
                                                    const float* __restrict__ prm, int S, float* __restrict__ part) {
    __shared__ float lds[4 * 4];
    const int WH = (H + 1) / 2, WW = (W + 1) / 2, c0 = blockIdx.y * 4;
    const long long M = (long long)B * WH * WW;
    const long long r0 = range_lo(blockIdx.x, S, M), r1 = range_lo(blockIdx.x + 1, S, M);
    float s[4] = {0.f, 0.f, 0.f, 0.f}, cnt[1] = {0.f};
    for (long long m = r0 + threadIdx.x; m < r1; m += NT) {
        const int b = int(m / (WH * WW)), rem = int(m - (long long)b * WH * WW), wy = rem / WW, wx = rem - wy * WW;
        const Patch p = load_patch(x, H, W, b, wy, wx);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (2 * wy + (q >> 1) >= H || 2 * wx + (q & 1) >= W) continue;
            cnt[0] += 1.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) s[i] += conv1_at(p, prm, c0 + i, q);
        }
    }
    block_sum(cnt, lds);
    block_sum(s, lds);
    float mean[4], q2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i) mean[i] = cnt[0] > 0.f ? s[i] / cnt[0] : 0.f;
    for (long long m = r0 + threadIdx.x; m < r1; m += NT) {
        const int b = int(m / (WH * WW)), rem = int(m - (long long)b * WH * WW), wy = rem / WW, wx = rem - wy * WW;
        const Patch p = load_patch(x, H, W, b, wy, wx);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (2 * wy + (q >> 1) >= H || 2 * wx + (q & 1) >= W) continue;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float d = conv1_at(p, prm, c0 + i, q) - mean[i];
                q2[i] += d * d;
            }
        }
    }
    block_sum(q2, lds);
    if (threadIdx.x < 4) {
        const int i = threadIdx.x;
        float* o = part + ((long long)blockIdx.x * 16 + c0 + i) * 3;
        o[0] = cnt[0];
        o[1] = pick(mean, i);
        o[2] = pick(q2, i);
    }
}

// stages 1..3: z stored planar [B][C][HW]; one channel per block (blockIdx.y)
__global__ __launch_bounds__(NT) void stats_kernel(const float* __restrict__ z, int B, int HW, int C, int S,
                                                   float* __restrict__ part) {
    __shared__ float lds[4];
    const int c = blockIdx.y;
    const long long M = (long long)B * HW;
    const long long r0 = range_lo(blockIdx.x, S, M), r1 = range_lo(blockIdx.x + 1, S, M);
    float s[1] = {0.f};
    for (long long m = r0 + threadIdx.x; m < r1; m += NT) {
        const int b = int(m / HW), pix = int(m - (long long)b * HW);
        s[0] += z[((long long)b * C + c) * HW + pix];
    }
    block_sum(s, lds);
    const float n = float(r1 - r0), mean = n > 0.f ? s[0] / n : 0.f;
    float q[1] = {0.f};
    for (long long m = r0 + threadIdx.x; m < r1; m += NT) {
        const int b = int(m / HW), pix = int(m - (long long)b * HW);
        const float d = z[((long long)b * C + c) * HW + pix] - mean;
        q[0] += d * d;
    }
    block_sum(q, lds);
    if (threadIdx.x == 0) {
        float* o = part + ((long long)blockIdx.x * C + c) * 3;
        o[0] = n;
        o[1] = mean;
        o[2] = q[0];
    }
}

// ------------------------------------------------------------------------------------------ forward
// p1[b][c][py][px] = max over the window of relu(bn(conv1(x))); one thread per (pooled pixel, group of 4 channels)
__global__ __launch_bounds__(NT) void conv1_pool_kernel(const float* __restrict__ x, int B, int H, int W, int PH, int PW,
                                                        const float* __restrict__ prm, const float* __restrict__ st,
                                                        float* __restrict__ p1) {
    const long long n = (long long)B * 4 * PH * PW;
    for (long long e = (long long)blockIdx.x * NT + threadIdx.x; e < n; e += (long long)gridDim.x * NT) {
        const long long pix = e % ((long long)PH * PW), bg = e / ((long long)PH * PW);
        const int b = int(bg >> 2), g = int(bg & 3), py = int(pix / PW), px = int(pix - (long long)py * PW);
        const Patch p = load_patch(x, H, W, b, py, px);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = 4 * g + i;
            float a[4];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                a[q] = fmaxf(bn_act(conv1_at(p, prm, c, q), st, prm + BN_G[0], prm + BN_B[0], c, 16), 0.f);
            p1[((long long)b * 16 + c) * PH * PW + pix] = a[argmax4(a)];
        }
    }
}

// depthwise 3x3 (pad 1) then pointwise: d = dw(p) (kept), z = pw(d); one thread per pixel
template <int CIN, int COUT>
__global__ __launch_bounds__(NT) void dwpw_fwd_kernel(const float* __restrict__ p, int B, int h, int w,
                                                      const float* __restrict__ wdw, const float* __restrict__ bdw,
                                                      const float* __restrict__ wpw, const float* __restrict__ bpw,
                                                      float* __restrict__ d, float* __restrict__ z) {
    const int HW = h * w;
    const long long m = (long long)blockIdx.x * NT + threadIdx.x;
    if (m >= (long long)B * HW) return;
    const int b = int(m / HW), pix = int(m - (long long)b * HW), y = pix / w, xx = pix - y * w;
    float dv[CIN];
#pragma unroll
    for (int ci = 0; ci < CIN; ++ci) {
        const float* src = p + ((long long)b * CIN + ci) * HW;
        float s = bdw[ci];
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int iy = y + kh - 1, ix = xx + kw - 1;
                if (iy >= 0 && iy < h && ix >= 0 && ix < w) s += wdw[ci * 9 + kh * 3 + kw] * src[iy * w + ix];
            }
        dv[ci] = s;
        d[((long long)b * CIN + ci) * HW + pix] = s;
    }
    for (int co = 0; co < COUT; ++co) {
        float s = bpw[co];
#pragma unroll
        for (int ci = 0; ci < CIN; ++ci) s += wpw[co * CIN + ci] * dv[ci];
        z[((long long)b * COUT + co) * HW + pix] = s;
    }
}

// relu(bn(z)) then maxpool 2 (floor): one thread per pooled element
__global__ __launch_bounds__(NT) void bn_relu_pool_kernel(const float* __restrict__ z, int B, int C, int h, int w,
                                                          const float* __restrict__ st, const float* __restrict__ g,
                                                          const float* __restrict__ bt, float* __restrict__ out) {
    const int PH = h / 2, PW = w / 2;
    const long long n = (long long)B * C * PH * PW;
    for (long long e = (long long)blockIdx.x * NT + threadIdx.x; e < n; e += (long long)gridDim.x * NT) {
        const long long bc = e / (PH * PW);
        const int rem = int(e - bc * PH * PW), py = rem / PW, px = rem - py * PW, c = int(bc % C);
        const float* src = z + bc * h * w;
        float a[4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
            a[q] = fmaxf(bn_act(src[(2 * py + (q >> 1)) * w + 2 * px + (q & 1)], st, g, bt, c, C), 0.f);
        out[e] = a[argmax4(a)];
    }
}

// head, one block (128 threads) per clip: mean of relu(bn(z3)) -> Linear(128, 64) -> ReLU -> dropout -> Linear(64, 2)
// -> weighted CE terms
__global__ __launch_bounds__(128) void mlp_head_fwd_kernel(const float* __restrict__ z3, int HW, const float* __restrict__ st3,
                                                           const float* __restrict__ prm, const float* __restrict__ mask_in,
                                                           unsigned long long seed, unsigned long long offset, float p,
                                                           const long long* __restrict__ targets,
                                                           const float* __restrict__ soft,
                                                           const float* __restrict__ class_w, float* __restrict__ logits,
                                                           float* __restrict__ gap, float* __restrict__ hr,
                                                           float* __restrict__ mask, float* __restrict__ mask_out,
                                                           float* __restrict__ wnll) {
    __shared__ float sg[128], shd[HID];
    const int c = threadIdx.x, b = blockIdx.x;
    const float* src = z3 + ((long long)b * 128 + c) * HW;
    float s = 0.f;
    for (int i = 0; i < HW; ++i) s += fmaxf(bn_act(src[i], st3, prm + BN_G[3], prm + BN_B[3], c, 128), 0.f);
    const float gv = s / float(HW);
    sg[c] = gv;
    gap[(long long)b * 128 + c] = gv;
    __syncthreads();
    if (c < HID) {
        const float hv = mlp_hidden<128>(prm + FC1_W, prm + FC1_B, sg, c);
        const float keep = mask_in ? mask_in[(long long)b * HID + c] : dropout_keep(c, b, seed, offset, p);
        const float scale = p < 1.f ? 1.0f / (1.0f - p) : 0.f;
        hr[(long long)b * HID + c] = hv;
        mask[(long long)b * HID + c] = keep;
        if (mask_out) mask_out[(long long)b * HID + c] = keep;
        shd[c] = hv * (keep * scale);
    }
    __syncthreads();
    if (c == 0) mlp_out<HID>(prm + FC2_W, prm + FC2_B, shd, b, targets, soft, class_w, logits, wnll);
}

// ------------------------------------------------------------------------------------------ BN backward
// Where BN k's output gradient comes from: MODE_GAP (BN 3: relu, then the global mean: dgap [B][128] already / HW),
// MODE_POOL (BNs 1, 2: relu, maxpool; dp = gradient of the pooled output), MODE_POOL0 (BN 0, z recomputed from x).
enum { MODE_GAP = 0, MODE_POOL = 1, MODE_POOL0 = 2 };

struct BwdSrc {
    const float* z;        // MODE_GAP / MODE_POOL: [B][C][h][w]
    const float* x;        // MODE_POOL0: the input image [B][H][W]
    const float* dsrc;     // MODE_GAP: dgap [B][128]; pool modes: dp [B][C][h/2][w/2]
    int B, C, h, w;
};

// part[s][C][2] = (sum dy, sum dy * xhat) of range s.  Pool modes: one item per pooled pixel (dy is 0 off the argmax);
// MODE_GAP: one item per pixel.  MODE_POOL0: 4 channels per block (blockIdx.y = group), otherwise one.
template <int MODE>
__global__ __launch_bounds__(NT) void bn_bwd_part_kernel(BwdSrc a, const float* __restrict__ prm, int k,
                                                         const float* __restrict__ st, int S, float* __restrict__ part) {
    constexpr int CPB = MODE == MODE_POOL0 ? 4 : 1;
    __shared__ float lds[4 * 2 * CPB];
    const int C = a.C, c0 = blockIdx.y * CPB;
    const float* g = prm + BN_G[k];
    const float* bt = prm + BN_B[k];
    const int PH = a.h / 2, PW = a.w / 2;
    const long long per = MODE == MODE_GAP ? (long long)a.h * a.w : (long long)PH * PW;
    const long long M = (long long)a.B * per;
    const long long r0 = range_lo(blockIdx.x, S, M), r1 = range_lo(blockIdx.x + 1, S, M);
    float v[2 * CPB];
#pragma unroll
    for (int i = 0; i < 2 * CPB; ++i) v[i] = 0.f;
    for (long long m = r0 + threadIdx.x; m < r1; m += NT) {
        const int b = int(m / per), pix = int(m - (long long)b * per);
        if constexpr (MODE == MODE_GAP) {
            const float zv = a.z[((long long)b * C + c0) * per + pix];
            const float dy = bn_act(zv, st, g, bt, c0, C) > 0.f ? a.dsrc[(long long)b * 128 + c0] : 0.f;
            v[0] += dy;
            v[1] += dy * ((zv - st[c0]) * st[C + c0]);
        } else if constexpr (MODE == MODE_POOL) {
            const int py = pix / PW, px = pix - py * PW;
            const float* src = a.z + ((long long)b * C + c0) * a.h * a.w;
            float zq[4], aq[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                zq[q] = src[(2 * py + (q >> 1)) * a.w + 2 * px + (q & 1)];
                aq[q] = fmaxf(bn_act(zq[q], st, g, bt, c0, C), 0.f);
            }
            const int j = argmax4(aq);
            const float dy = aq[j] > 0.f ? a.dsrc[((long long)b * C + c0) * per + pix] : 0.f;
            v[0] += dy;
            v[1] += dy * ((zq[j] - st[c0]) * st[C + c0]);
        } else {
            const int py = pix / PW, px = pix - py * PW;
            const Patch p = load_patch(a.x, a.h, a.w, b, py, px);
#pragma unroll
            for (int i = 0; i < CPB; ++i) {
                const int c = c0 + i;
                float zq[4], aq[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    zq[q] = conv1_at(p, prm, c, q);
                    aq[q] = fmaxf(bn_act(zq[q], st, g, bt, c, C), 0.f);
                }
                const int j = argmax4(aq);
                const float dy = aq[j] > 0.f ? a.dsrc[((long long)b * C + c) * per + pix] : 0.f;
                v[2 * i] += dy;
                v[2 * i + 1] += dy * ((zq[j] - st[c]) * st[C + c]);
            }
        }
    }
    block_sum(v, lds);
    if (threadIdx.x < CPB) {
        const int i = threadIdx.x;
        float* o = part + ((long long)blockIdx.x * C + c0 + i) * 2;
        o[0] = pick(v, 2 * i);
        o[1] = pick(v, 2 * i + 1);
    }
}

// dz = gamma * invstd * (dy - sum dy / n - xhat * sum(dy xhat) / n) of every pixel of BN k (k = 1..3), stored, and the
// pw conv's input gradient dd[ci] = sum_co W[co][ci] dz[co]; one thread per pixel
template <int CIN, int COUT, int MODE>
__global__ __launch_bounds__(NT) void bn_apply_pw_dgrad_kernel(BwdSrc a, const float* __restrict__ prm, int k,
                                                               const float* __restrict__ st, float inv_n,
                                                               float* __restrict__ dz, float* __restrict__ dd) {
    const int h = a.h, w = a.w, HW = h * w, PH = h / 2, PW = w / 2;
    const long long m = (long long)blockIdx.x * NT + threadIdx.x;
    if (m >= (long long)a.B * HW) return;
    const int b = int(m / HW), pix = int(m - (long long)b * HW), y = pix / w, xx = pix - y * w;
    const float* g = prm + BN_G[k];
    const float* bt = prm + BN_B[k];
    const float* wpw = prm + PW_W[k];
    const bool in_pool = y < 2 * PH && xx < 2 * PW;
    const int wy = y >> 1, wx = xx >> 1, mine = ((y & 1) << 1) | (xx & 1);
    float acc[CIN];
#pragma unroll
    for (int ci = 0; ci < CIN; ++ci) acc[ci] = 0.f;
    for (int co = 0; co < COUT; ++co) {
        const float* src = a.z + ((long long)b * COUT + co) * HW;
        const float zv = src[pix];
        float dy = 0.f;
        if constexpr (MODE == MODE_GAP) {
            if (bn_act(zv, st, g, bt, co, COUT) > 0.f) dy = a.dsrc[(long long)b * 128 + co];
        } else {
            if (in_pool) {
                float aq[4];
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    aq[q] = fmaxf(bn_act(src[(2 * wy + (q >> 1)) * w + 2 * wx + (q & 1)], st, g, bt, co, COUT), 0.f);
                const int j = argmax4(aq);
                if (j == mine && aq[j] > 0.f) dy = a.dsrc[((long long)b * COUT + co) * PH * PW + wy * PW + wx];
            }
        }
        const float is = st[COUT + co];
        const float xh = (zv - st[co]) * is;
        const float dzv = g[co] * is * (dy - st[2 * COUT + co] * inv_n - xh * (st[3 * COUT + co] * inv_n));
        dz[((long long)b * COUT + co) * HW + pix] = dzv;
#pragma unroll
        for (int ci = 0; ci < CIN; ++ci) acc[ci] += wpw[co * CIN + ci] * dzv;
    }
#pragma unroll
    for (int ci = 0; ci < CIN; ++ci) dd[((long long)b * CIN + ci) * HW + pix] = acc[ci];
}

// ------------------------------------------------------------------------------------------ weight gradients
// pw k: slab[s][W (COUT x CIN), bias (COUT)] = sum over the pixels of range s of dz[co] * d[ci] (and dz[co]).  LDS tiles of
// TP pixels; thread t owns RC output channels x RK input channels.
template <int CIN, int COUT, int RC, int RK>
__global__ __launch_bounds__(NT) void pw_wgrad_kernel(const float* __restrict__ dz, const float* __restrict__ d, int B,
                                                      int HW, int S, int seg, float* __restrict__ slab) {
    static_assert((COUT / RC) * (CIN / RK) == NT, "one thread per RC x RK block");
    __shared__ float sdz[COUT][TP + 1], sd[CIN][TP + 1];
    const long long M = (long long)B * HW;
    const long long r0 = range_lo(blockIdx.x, S, M), r1 = range_lo(blockIdx.x + 1, S, M);
    const int t = threadIdx.x, rc0 = (t / (CIN / RK)) * RC, rk0 = (t % (CIN / RK)) * RK;
    float acc[RC][RK], accb[RC];
#pragma unroll
    for (int i = 0; i < RC; ++i) {
        accb[i] = 0.f;
#pragma unroll
        for (int j = 0; j < RK; ++j) acc[i][j] = 0.f;
    }
    for (long long mt = r0; mt < r1; mt += TP) {
        for (int e = t; e < COUT * TP; e += NT) {
            const int co = e / TP, mm = e - co * TP;
            const long long m = mt + mm;
            float v = 0.f;
            if (m < r1) {
                const int b = int(m / HW), pix = int(m - (long long)b * HW);
                v = dz[((long long)b * COUT + co) * HW + pix];
            }
            sdz[co][mm] = v;
        }
        for (int e = t; e < CIN * TP; e += NT) {
            const int ci = e / TP, mm = e - ci * TP;
            const long long m = mt + mm;
            float v = 0.f;
            if (m < r1) {
                const int b = int(m / HW), pix = int(m - (long long)b * HW);
                v = d[((long long)b * CIN + ci) * HW + pix];
            }
            sd[ci][mm] = v;
        }
        __syncthreads();
#pragma unroll 4
        for (int mm = 0; mm < TP; ++mm) {
            float av[RC], bv[RK];
#pragma unroll
            for (int i = 0; i < RC; ++i) av[i] = sdz[rc0 + i][mm];
#pragma unroll
            for (int j = 0; j < RK; ++j) bv[j] = sd[rk0 + j][mm];
#pragma unroll
            for (int i = 0; i < RC; ++i) {
                accb[i] += av[i];
#pragma unroll
                for (int j = 0; j < RK; ++j) acc[i][j] += av[i] * bv[j];
            }
        }
        __syncthreads();
    }
    float* dst = slab + (long long)blockIdx.x * SLAB_N + SEG_SLAB[seg];
#pragma unroll
    for (int i = 0; i < RC; ++i) {
#pragma unroll
        for (int j = 0; j < RK; ++j) dst[(rc0 + i) * CIN + rk0 + j] = acc[i][j];
        if (rk0 == 0) dst[COUT * CIN + rc0 + i] = accb[i];
    }
}

// dw k, one channel per block (blockIdx.y): dp = the input gradient (transposed 3x3 of dd) of every pixel of the range,
// and slab[s][c * 9 + tap] = sum dd * p under that tap, slab[s][C * 9 + c] = sum dd
__global__ __launch_bounds__(NT) void dw_bwd_kernel(const float* __restrict__ dd, const float* __restrict__ p, int B, int C,
                                                    int h, int w, const float* __restrict__ wdw, int S, int seg,
                                                    float* __restrict__ dp, float* __restrict__ slab) {
    __shared__ float lds[4 * 10];
    const int c = blockIdx.y, HW = h * w;
    const long long M = (long long)B * HW;
    const long long r0 = range_lo(blockIdx.x, S, M), r1 = range_lo(blockIdx.x + 1, S, M);
    float acc[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) acc[i] = 0.f;
    float wk[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) wk[t] = wdw[c * 9 + t];
    for (long long m = r0 + threadIdx.x; m < r1; m += NT) {
        const int b = int(m / HW), pix = int(m - (long long)b * HW), y = pix / w, xx = pix - y * w;
        const long long base = ((long long)b * C + c) * HW;
        const float v = dd[base + pix];
        float g = 0.f;
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int iy = y + kh - 1, ix = xx + kw - 1;
                if (iy >= 0 && iy < h && ix >= 0 && ix < w) acc[kh * 3 + kw] += v * p[base + iy * w + ix];
                const int oy = y + 1 - kh, ox = xx + 1 - kw;
                if (oy >= 0 && oy < h && ox >= 0 && ox < w) g += wk[kh * 3 + kw] * dd[base + oy * w + ox];
            }
        acc[9] += v;
        dp[base + pix] = g;
    }
    block_sum(acc, lds);
    if (threadIdx.x < 10) {
        float* dst = slab + (long long)blockIdx.x * SLAB_N + SEG_SLAB[seg];
        const int i = threadIdx.x;
        if (i < 9) dst[c * 9 + i] = pick(acc, i);
        else dst[C * 9 + c] = acc[9];
    }
}

// conv1: dz of every pixel recomputed (conv, BN, ReLU, pool routing from dp1, BN backward) per window of 4 pixels, 4
// channels per block (blockIdx.y = group); slab[s][c * 9 + tap] = sum dz * x under that tap, slab[s][144 + c] = sum dz
__global__ __launch_bounds__(NT) void conv1_wgrad_kernel(const float* __restrict__ x, int B, int H, int W,
                                                         const float* __restrict__ prm, const float* __restrict__ st,
                                                         const float* __restrict__ dp1, float inv_n, int S,
                                                         float* __restrict__ slab) {
    __shared__ float lds[4 * 40];
    const int WH = (H + 1) / 2, WW = (W + 1) / 2, PH = H / 2, PW = W / 2, c0 = blockIdx.y * 4;
    const long long M = (long long)B * WH * WW;
    const long long r0 = range_lo(blockIdx.x, S, M), r1 = range_lo(blockIdx.x + 1, S, M);
    const float* g = prm + BN_G[0];
    const float* bt = prm + BN_B[0];
    float acc[40];
#pragma unroll
    for (int i = 0; i < 40; ++i) acc[i] = 0.f;
    for (long long m = r0 + threadIdx.x; m < r1; m += NT) {
        const int b = int(m / (WH * WW)), rem = int(m - (long long)b * WH * WW), wy = rem / WW, wx = rem - wy * WW;
        const Patch p = load_patch(x, H, W, b, wy, wx);
        const bool pool = wy < PH && wx < PW;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = c0 + i;
            float zq[4], aq[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                zq[q] = conv1_at(p, prm, c, q);
                aq[q] = fmaxf(bn_act(zq[q], st, g, bt, c, 16), 0.f);
            }
            const int j = argmax4(aq);
            const float dpv = (pool && aq[j] > 0.f) ? dp1[((long long)b * 16 + c) * PH * PW + wy * PW + wx] : 0.f;
            const float is = st[16 + c], k1 = st[32 + c] * inv_n, k2 = st[48 + c] * inv_n;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (2 * wy + (q >> 1) >= H || 2 * wx + (q & 1) >= W) continue;
                const float dy = q == j ? dpv : 0.f;
                const float dzv = g[c] * is * (dy - k1 - ((zq[q] - st[c]) * is) * k2);
                const int oy = q >> 1, ox = q & 1;
#pragma unroll
                for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                    for (int kw = 0; kw < 3; ++kw) acc[i * 10 + kh * 3 + kw] += dzv * p.v[oy + kh][ox + kw];
                acc[i * 10 + 9] += dzv;
            }
        }
    }
    block_sum(acc, lds);
    if (threadIdx.x < 40) {
        const int i = threadIdx.x / 10, t = threadIdx.x - i * 10, c = c0 + i;
        float* dst = slab + (long long)blockIdx.x * SLAB_N;
        const float v = pick(acc, threadIdx.x);
        if (t < 9) dst[c * 9 + t] = v;
        else dst[144 + c] = v;
    }
}

// grads[conv params] = sum over the S slab rows in index order: 64 outputs per block, 4 lanes each taking every 4th row,
// added ((l0 + l1) + (l2 + l3))
__global__ __launch_bounds__(NT) void slab_reduce_kernel(const float* __restrict__ slab, int S, float* __restrict__ grads) {
    __shared__ float red[4][64];
    const int o = blockIdx.x * 64 + (threadIdx.x & 63), l = threadIdx.x >> 6;
    float s = 0.f;
    if (o < SLAB_N)
        for (int i = l; i < S; i += 4) s += slab[(long long)i * SLAB_N + o];
    red[l][threadIdx.x & 63] = s;
    __syncthreads();
    if (l == 0 && o < SLAB_N) {
        int seg = 0;
#pragma unroll
        for (int i = 1; i < NSEG; ++i)
            if (o >= SEG_SLAB[i]) seg = i;
        grads[SEG_PARAM[seg] + (o - SEG_SLAB[seg])] =
            (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
    }
}

// ------------------------------------------------------------------------------------------ workspace
struct Shapes {
    int h[4], w[4];          // BN k's image: conv1's (the input's), then every pool halves it (floor)
    int S;                   // pixel ranges of every partial sum
};
Shapes make_shapes(int B, int H, int W) {
    Shapes s;
    s.h[0] = H; s.w[0] = W;
    for (int k = 1; k < 4; ++k) { s.h[k] = s.h[k - 1] / 2; s.w[k] = s.w[k - 1] / 2; }
    const long long px = (long long)B * H * W;
    s.S = int(std::min<long long>(512, std::max<long long>(1, (px + 4095) / 4096)));
    return s;
}

struct Ws {
    float *p[4], *d[4], *z[4], *dz[4], *dd[4], *dp[4];   // index k = 1..3 (the dw / pw block feeding BN k)
    float* stat[4];
    float *part, *slab, *gap, *hr, *mask, *wnll, *dl, *dh, *dgap;
    size_t total;
};

Ws carve(char* base, int B, const Shapes& s) {
    Ws w{};
    Carver ws{base};
    auto f = [&](long long n) { return ws.floats(n); };
    for (int k = 1; k < 4; ++k) {
        const long long px = (long long)B * s.h[k] * s.w[k];
        w.p[k] = f(px * NC[k - 1]);
        w.d[k] = f(px * NC[k - 1]);
        w.z[k] = f(px * NC[k]);
        w.dz[k] = f(px * NC[k]);
        w.dd[k] = f(px * NC[k - 1]);
        w.dp[k] = f(px * NC[k - 1]);
    }
    for (int k = 0; k < 4; ++k) w.stat[k] = f(4 * NC[k]);
    w.part = f((long long)s.S * 128 * 3);
    w.slab = f((long long)s.S * SLAB_N);
    w.gap = f((long long)B * 128);
    w.hr = f((long long)B * HID);
    w.mask = f((long long)B * HID);
    w.dh = f((long long)B * HID);
    w.dgap = f((long long)B * 128);
    w.wnll = f(2LL * B);
    w.dl = f(2LL * B);
    w.total = ws.off;
    return w;
}

constexpr int GRID_CAP = 8192;    // blocks of a grid-stride launch
unsigned blocks_for(long long n) { return unsigned((n + NT - 1) / NT); }

// the shapes torch's train-mode forward accepts: three 2x2 pools need H, W >= 8 and the last BN more than one value per
// channel; the element count of the largest activation must fit the 32-bit pixel arithmetic of the kernels
bool trainable(int B, int H, int W) {
    if (B < 1 || H < 8 || W < 8) return false;
    if ((long long)B * (H / 8) * (W / 8) <= 1) return false;
    return (long long)B * H * W <= (1LL << 27);
}

// The step behind cough_train_small_forward_backward (d_targets: class indices, d_soft null) and
// cough_train_small_forward_backward_soft of libcough_amd_soft.so (d_soft: [B][2] class probabilities, d_targets null); fn
// names the entry point in the messages.  The two differ in what the two head kernels read, nowhere else.
int train_step(const char* fn, const float* d_x, int n_clips, int height, int width, const long long* d_targets,
               const float* d_soft, const float* d_class_weights, const float* d_dropout_mask, unsigned long long seed,
               unsigned long long offset, float p, const float* d_params, float* d_grads, float* d_running,
               long long* d_num_batches, float momentum, float eps, float* d_loss, float* d_logits, float* d_mask_out,
               void* d_workspace, size_t workspace_bytes, void* stream) {
    COUGH_REQUIRE(n_clips >= 1 && height >= 1 && width >= 1, COUGH_EINVAL, "%s: bad shape (%d, %d, %d)", fn, n_clips, height,
                  width);
    COUGH_REQUIRE(height >= 8 && width >= 8, COUGH_EINVAL, "%s: input %dx%d too small for the network (three 2x2 pools)", fn,
                  height, width);
    COUGH_REQUIRE((long long)n_clips * (height / 8) * (width / 8) > 1, COUGH_EINVAL,
                  "%s: the last BatchNorm sees one value per channel (batch statistics need more)", fn);
    COUGH_REQUIRE(trainable(n_clips, height, width), COUGH_EINVAL, "%s: batch of %d images of %dx%d too large", fn, n_clips,
                  height, width);
    const int B = n_clips, H = height, W = width;
    const Shapes s = make_shapes(B, H, W);
    const Ws w = carve(static_cast<char*>(d_workspace), B, s);
    const void* d_y = d_soft ? static_cast<const void*>(d_soft) : d_targets;
    if (const int rc = check_step_args(fn, {d_x, d_y, d_params, d_grads, d_running, d_num_batches, d_loss, d_logits,
                                                  d_workspace},
                                       {p}, momentum, eps, d_workspace, workspace_bytes, w.total);
        rc != COUGH_OK)
        return rc;

    hipStream_t st = static_cast<hipStream_t>(stream);
    const float* prm = d_params;
    const int S = s.S;
    auto finalize = [&](int k) {
        hipLaunchKernelGGL(stats_finalize_kernel, dim3(NC[k]), dim3(NT), 0, st, w.part, S, NC[k], eps, momentum,
                           d_running + RUN[k], d_running + RUN[k] + NC[k], d_num_batches + k, w.stat[k]);
    };
    auto px = [&](int k) { return (long long)B * s.h[k] * s.w[k]; };

    // ---- forward
    hipLaunchKernelGGL(stats0_kernel, dim3(S, 4), dim3(NT), 0, st, d_x, B, H, W, prm, S, w.part);
    finalize(0);
    hipLaunchKernelGGL(conv1_pool_kernel, dim3(grid_for((long long)B * 4 * s.h[1] * s.w[1], GRID_CAP)), dim3(NT), 0, st, d_x,
                       B, H, W, s.h[1], s.w[1], prm, w.stat[0], w.p[1]);
    for (int k = 1; k < 4; ++k) {
        const int h = s.h[k], wd = s.w[k];
        const dim3 g(blocks_for(px(k)));
        const float *wdw = prm + DW_W[k], *bdw = prm + DW_B[k], *wpw = prm + PW_W[k], *bpw = prm + PW_B[k];
        if (k == 1) hipLaunchKernelGGL((dwpw_fwd_kernel<16, 32>), g, dim3(NT), 0, st, w.p[k], B, h, wd, wdw, bdw, wpw, bpw, w.d[k], w.z[k]);
        if (k == 2) hipLaunchKernelGGL((dwpw_fwd_kernel<32, 64>), g, dim3(NT), 0, st, w.p[k], B, h, wd, wdw, bdw, wpw, bpw, w.d[k], w.z[k]);
        if (k == 3) hipLaunchKernelGGL((dwpw_fwd_kernel<64, 128>), g, dim3(NT), 0, st, w.p[k], B, h, wd, wdw, bdw, wpw, bpw, w.d[k], w.z[k]);
        hipLaunchKernelGGL(stats_kernel, dim3(S, NC[k]), dim3(NT), 0, st, w.z[k], B, h * wd, NC[k], S, w.part);
        finalize(k);
        if (k < 3)
            hipLaunchKernelGGL(bn_relu_pool_kernel, dim3(grid_for((long long)B * NC[k] * (h / 2) * (wd / 2), GRID_CAP)), dim3(NT),
                               0, st, w.z[k], B, NC[k], h, wd, w.stat[k], prm + BN_G[k], prm + BN_B[k], w.p[k + 1]);
    }
    const int HW3 = s.h[3] * s.w[3];
    hipLaunchKernelGGL(mlp_head_fwd_kernel, dim3(B), dim3(128), 0, st, w.z[3], HW3, w.stat[3], prm, d_dropout_mask, seed,
                       offset, p, d_targets, d_soft, d_class_weights, d_logits, w.gap, w.hr, w.mask, d_mask_out, w.wnll);

    // ---- backward
    hipLaunchKernelGGL((mlp_head_bwd_kernel<128, HID, HID, 0>), dim3(B), dim3(128), 0, st, B, HW3, d_logits, d_targets, d_soft,
                       d_class_weights, w.wnll, w.hr, w.mask, p, prm + FC1_W, prm + FC2_W, w.stat[0], NC[0], d_loss, w.dl, w.dh, w.dgap);
    hipLaunchKernelGGL((mlp_fc_grad_kernel<128, HID, HID, 0>), dim3((128 * HID + 3 * HID + 2 + 63) / 64), dim3(NT), 0, st, B,
                       w.gap, w.hr, w.mask, p, w.dl, w.dh, d_grads + FC1_W);
    for (int k = 3; k >= 1; --k) {
        const int h = s.h[k], wd = s.w[k], C = NC[k];
        BwdSrc src{w.z[k], nullptr, k == 3 ? w.dgap : w.dp[k + 1], B, C, h, wd};
        if (k == 3) hipLaunchKernelGGL(bn_bwd_part_kernel<MODE_GAP>, dim3(S, C), dim3(NT), 0, st, src, prm, k, w.stat[k], S, w.part);
        else hipLaunchKernelGGL(bn_bwd_part_kernel<MODE_POOL>, dim3(S, C), dim3(NT), 0, st, src, prm, k, w.stat[k], S, w.part);
        hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(C), dim3(NT), 0, st, w.part, S, C, w.stat[k], d_grads + BN_G[k],
                           d_grads + BN_B[k]);
        const float inv_n = float(1.0 / double(px(k)));
        const dim3 g(blocks_for(px(k)));
        if (k == 3) {
            hipLaunchKernelGGL((bn_apply_pw_dgrad_kernel<64, 128, MODE_GAP>), g, dim3(NT), 0, st, src, prm, k, w.stat[k], inv_n, w.dz[k], w.dd[k]);
            hipLaunchKernelGGL((pw_wgrad_kernel<64, 128, 4, 8>), dim3(S), dim3(NT), 0, st, w.dz[k], w.d[k], B, h * wd, S, seg_pw(k), w.slab);
        } else if (k == 2) {
            hipLaunchKernelGGL((bn_apply_pw_dgrad_kernel<32, 64, MODE_POOL>), g, dim3(NT), 0, st, src, prm, k, w.stat[k], inv_n, w.dz[k], w.dd[k]);
            hipLaunchKernelGGL((pw_wgrad_kernel<32, 64, 2, 4>), dim3(S), dim3(NT), 0, st, w.dz[k], w.d[k], B, h * wd, S, seg_pw(k), w.slab);
        } else {
            hipLaunchKernelGGL((bn_apply_pw_dgrad_kernel<16, 32, MODE_POOL>), g, dim3(NT), 0, st, src, prm, k, w.stat[k], inv_n, w.dz[k], w.dd[k]);
            hipLaunchKernelGGL((pw_wgrad_kernel<16, 32, 2, 1>), dim3(S), dim3(NT), 0, st, w.dz[k], w.d[k], B, h * wd, S, seg_pw(k), w.slab);
        }
        hipLaunchKernelGGL(dw_bwd_kernel, dim3(S, NC[k - 1]), dim3(NT), 0, st, w.dd[k], w.p[k], B, NC[k - 1], h, wd,
                           prm + DW_W[k], S, seg_dw(k), w.dp[k], w.slab);
    }
    BwdSrc src0{nullptr, d_x, w.dp[1], B, 16, H, W};
    hipLaunchKernelGGL(bn_bwd_part_kernel<MODE_POOL0>, dim3(S, 4), dim3(NT), 0, st, src0, prm, 0, w.stat[0], S, w.part);
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(16), dim3(NT), 0, st, w.part, S, 16, w.stat[0], d_grads + BN_G[0],
                       d_grads + BN_B[0]);
    hipLaunchKernelGGL(conv1_wgrad_kernel, dim3(S, 4), dim3(NT), 0, st, d_x, B, H, W, prm, w.stat[0], w.dp[1],
                       float(1.0 / double(px(0))), S, w.slab);
    hipLaunchKernelGGL(slab_reduce_kernel, dim3((SLAB_N + 63) / 64), dim3(NT), 0, st, w.slab, S, d_grads);
    COUGH_HIP_CHECK(hipGetLastError());
    return COUGH_OK;
}

}  // namespace
}  // namespace cough

#ifdef COUGH_SOFT_EXPORTS   // the second compilation of this file, for libcough_amd_soft.so: the soft entry point alone
#include "../../include/cough_amd_soft.h"

extern "C" int cough_train_small_forward_backward_soft(const float* d_x, int n_clips, int height, int width,
                                                       const float* d_soft_targets, const float* d_class_weights,
                                                       const float* d_dropout_mask, unsigned long long seed,
                                                       unsigned long long offset, float p, const float* d_params,
                                                       float* d_grads, float* d_running, long long* d_num_batches,
                                                       float momentum, float eps, float* d_loss, float* d_logits,
                                                       float* d_mask_out, void* d_workspace, size_t workspace_bytes,
                                                       void* stream) {
    return cough::train_step(__func__, d_x, n_clips, height, width, nullptr, d_soft_targets, d_class_weights, d_dropout_mask,
                             seed, offset, p, d_params, d_grads, d_running, d_num_batches, momentum, eps, d_loss, d_logits,
                             d_mask_out, d_workspace, workspace_bytes, stream);
}
#else
extern "C" size_t cough_train_small_workspace_bytes(int n_clips, int height, int width) {
    using namespace cough;
    if (!trainable(n_clips, height, width)) return 0;
    return carve(nullptr, n_clips, make_shapes(n_clips, height, width)).total;
}

extern "C" int cough_train_small_forward_backward(const float* d_x, int n_clips, int height, int width,
                                                  const long long* d_targets, const float* d_class_weights,
                                                  const float* d_dropout_mask, unsigned long long seed,
                                                  unsigned long long offset, float p, const float* d_params,
                                                  float* d_grads, float* d_running, long long* d_num_batches,
                                                  float momentum, float eps, float* d_loss, float* d_logits,
                                                  float* d_mask_out, void* d_workspace, size_t workspace_bytes,
                                                  void* stream) {
    return cough::train_step(__func__, d_x, n_clips, height, width, d_targets, nullptr, d_class_weights, d_dropout_mask, seed,
                             offset, p, d_params, d_grads, d_running, d_num_batches, momentum, eps, d_loss, d_logits,
                             d_mask_out, d_workspace, workspace_bytes, stream);
}
#endif
