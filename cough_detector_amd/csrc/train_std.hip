// Training step of CoughDetector ("standard", channels (32, 64, 128, 256), fc_hidden 128) for gfx950: the train-mode
// forward pass and the backward pass, as the reference's train_epoch takes one step (src/train.py:54-112,
// model src/model.py:11-141).  clip_grad_norm_ + AdamW run in cough_adamw_step (train.hip), unchanged.
//
//   4 x ConvBlock   conv3x3 pad 1 -> BatchNorm2d (batch statistics) -> ReLU -> MaxPool2d(2) -> Dropout2d(p_block)
//   head            global mean -> Linear(256, 128) -> ReLU -> Dropout(p_fc) -> Linear(128, 2); weighted CrossEntropyLoss
//
// Everything is exact f32.  Activations are NHWC; parameters, gradients and running statistics are flat caller buffers in
// model.parameters() / model.buffers() order.
//
//   convs 1-3   implicit GEMMs on v_mfma_f32_32x32x2_f32 with both operands staged through LDS (a global load feeds
//               the MFMAs of every wave of the workgroup), the next K chunk prefetched into registers while the
//               current one is multiplied:
//                 forward  rows = pixels, cols = Cout, K = (tap, Cin); 128 x 64 tiles
//                 dgrad    the same kernel: for stride 1, pad 1 the input gradient is a 3x3 conv of dz with the weights
//                          transposed and the taps flipped (repacked once per step with the forward's)
//                 wgrad    rows = Cout, cols = Cin of one tap, K = the pixels of one of S fixed ranges; each range
//                          writes a partial slab [Cout][9 Cin + 1] (last column: the bias gradient, sum of dz), and a
//                          second launch adds the S slabs in index order
//   conv 0      Cin = 1, K = 9: VALU.  Its input gradient is never needed; its weight gradient recomputes dz from z0
//               on the fly (dz0 is never stored)
//   BatchNorm   per-range (count, mean, centred M2) partials for up to 256 channels, merged per channel by a 256-thread
//               fixed-order Chan tree; backward sums dy and dy * xhat the same way.  BN-apply, ReLU, the 2x2 max-pool
//               and Dropout2d are one forward pass, which stores the window's argmax (one byte); backward routes the
//               gradient of a pooled value to that pixel when its BN output is > 0, scaled by the plane's keep / (1 - p)
//   dropout     one keep mask [B][608]: block 0's 32 channels, block 1's 64, block 2's 128, block 3's 256, the head's 128
//               hidden units; a caller mask or Philox draws (counter (unit / 4, clip, offset), keep where u >= p)
//   head        one workgroup per clip forward (mean, Linear, ReLU, dropout, Linear, CE terms) and backward (every block
//               sums the batch's CE weights in the same order); the Linear gradients split the batch in 4 fixed quarters
// No float atomics; every reduction runs in a fixed order, so the same inputs and state give bit-identical results.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>

#include "common.h"
#include "nn_common.h"
#include "train_common.h"

namespace cough {
namespace {

constexpr int NB = 4;                                   // conv blocks
constexpr int CH[NB] = {32, 64, 128, 256};              // output channels of block k
constexpr int CI[NB] = {1, 32, 64, 128};                // input channels of block k
constexpr int HID = 128;                                // fc_hidden
constexpr int MASK_W = 608;                             // keep-mask units per clip
constexpr int MOFF[NB + 1] = {0, 32, 96, 224, 480};     // first unit of block k (k = 4: the head's hidden units)
// model.parameters() offsets (20 tensors, 421,954 values): per block conv.weight, conv.bias, bn.weight, bn.bias; fc.0, fc.3
constexpr int CONV_W[NB] = {0, 384, 19008, 93120};
constexpr int CONV_B[NB] = {288, 18816, 92736, 388032};
constexpr int BN_G[NB] = {320, 18880, 92864, 388288};
constexpr int BN_B[NB] = {352, 18944, 92992, 388544};
constexpr int FC0_W = 388800, FC0_B = 421568, FC3_W = 421696, FC3_B = 421952, N_PARAMS = 421954;
constexpr int RUN[NB] = {0, 64, 192, 448}, N_RUNNING = 960;
static_assert(CONV_B[0] == CONV_W[0] + 32 * 9 && BN_G[0] == CONV_B[0] + 32 && BN_B[0] == BN_G[0] + 32, "block 0 layout");
static_assert(CONV_W[1] == BN_B[0] + 32 && CONV_B[1] == CONV_W[1] + 64 * 32 * 9 && BN_B[1] == BN_G[1] + 64, "block 1");
static_assert(CONV_W[2] == BN_B[1] + 64 && CONV_B[2] == CONV_W[2] + 128 * 64 * 9 && BN_B[2] == BN_G[2] + 128, "block 2");
static_assert(CONV_W[3] == BN_B[2] + 128 && CONV_B[3] == CONV_W[3] + 256 * 128 * 9 && BN_B[3] == BN_G[3] + 256, "block 3");
static_assert(FC0_W == BN_B[3] + 256 && FC0_B == FC0_W + HID * 256 && FC3_W == FC0_B + HID && FC3_B == FC3_W + 2 * HID &&
              N_PARAMS == FC3_B + 2, "head layout");
static_assert(RUN[3] + 2 * 256 == N_RUNNING && MOFF[4] + HID == MASK_W, "running statistics / mask layout");

// ------------------------------------------------------------------------------------------ dropout mask
// mask[b][u] = the keep of unit u of clip b (a caller mask, or a Philox draw against p_block / p_fc)
__global__ __launch_bounds__(NT) void mask_kernel(int B, const float* __restrict__ mask_in, unsigned long long seed,
                                                  unsigned long long offset, float p_block, float p_fc,
                                                  float* __restrict__ mask, float* __restrict__ mask_out) {
    const long long e = (long long)blockIdx.x * NT + threadIdx.x;
    if (e >= (long long)B * MASK_W) return;
    const int b = int(e / MASK_W), u = int(e - (long long)b * MASK_W);
    const float keep = mask_in ? mask_in[e] : dropout_keep(u, b, seed, offset, u < MOFF[NB] ? p_block : p_fc);
    mask[e] = keep;
    if (mask_out) mask_out[e] = keep;
}

// ------------------------------------------------------------------------------------------ weights
// blocks 1..3 (blockIdx.y + 1): wt [Cout][tap][Cin] (forward B operand), wd [Cin][tap][Cout] with the taps flipped (dgrad
// B operand); both at the flat parameters' offsets
__global__ __launch_bounds__(NT) void prep_weights_kernel(const float* __restrict__ prm, float* __restrict__ wt,
                                                          float* __restrict__ wd) {
    const int k = blockIdx.y + 1;
    const int cin = k == 1 ? 32 : k == 2 ? 64 : 128, cout = 2 * cin;
    const int off = k == 1 ? CONV_W[1] : k == 2 ? CONV_W[2] : CONV_W[3];
    const int n = cout * cin * 9;
    for (int e = blockIdx.x * NT + threadIdx.x; e < n; e += gridDim.x * NT) {
        const int co = e / (cin * 9), rem = e - co * cin * 9, ci = rem / 9, t = rem - ci * 9;
        const float v = prm[off + e];
        wt[off + (co * 9 + t) * cin + ci] = v;
        wd[off + (ci * 9 + (8 - t)) * cout + co] = v;
    }
}

// ------------------------------------------------------------------------------------------ convolutions
// conv 0 (Cin = 1): z0[m][c], one thread per output value
__global__ __launch_bounds__(NT) void conv0_fwd_kernel(const float* __restrict__ x, int B, int H, int W,
                                                       const float* __restrict__ prm, float* __restrict__ z) {
    const long long n = (long long)B * H * W * 32;
    for (long long e = (long long)blockIdx.x * NT + threadIdx.x; e < n; e += (long long)gridDim.x * NT) {
        const int m = int(e >> 5), c = int(e & 31);         // m < 2^27 (trainable): 32-bit pixel arithmetic
        const int b = m / (H * W), pix = m - b * H * W, y = pix / W, xx = pix - y * W;
        const float* src = x + (long long)b * H * W;
        float s = prm[CONV_B[0] + c];
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int iy = y + kh - 1, ix = xx + kw - 1;
                if (iy >= 0 && iy < H && ix >= 0 && ix < W) s += prm[CONV_W[0] + c * 9 + kh * 3 + kw] * src[iy * W + ix];
            }
        z[e] = s;
    }
}

constexpr int KC = 32;     // K chunk: 32 channels of one tap (forward / dgrad) or 32 pixels (wgrad)
constexpr int KP = 36;     // forward LDS row stride in floats: 16-byte rows, ds_read_b128 without bank conflicts

// out[m][n] = bias[n] + sum over taps t and channels c of in[pixel m shifted by t][c] * wt[n][t][c]: a 3x3, pad 1 conv
// of the NHWC image in [B][h][w][C] (C % 32 == 0), out [M = B h w][N].  Four waves stacked along the rows, each 32 rows x
// 32 NTL columns; a K chunk is one tap x 32 channels, staged as As[row][k] / Bs[col][k], and MFMA slot h of step j takes
// k = 16 h + j, so a lane reads its 16 k values with four ds_read_b128.
template <int NTL>
__global__ __launch_bounds__(256) void conv3x3_kernel(const float* __restrict__ in, int C, int h, int w, long long M,
                                                      const float* __restrict__ wt, const float* __restrict__ bias, int N,
                                                      float* __restrict__ out) {
    constexpr int BM = 128, BN = 32 * NTL;
    __shared__ __attribute__((aligned(16))) float As[BM * KP];
    __shared__ __attribute__((aligned(16))) float Bs[BN * KP];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, hh = lane >> 5;
    const long long m0 = (long long)blockIdx.x * BM;
    const int n0 = blockIdx.y * BN;
    const int q = tid & 7, lrow = tid >> 3;              // loader: float4 q of rows lrow + 32 i
    const int HW = h * w;
    int ly[4], lx[4];
    long long lbase[4];
    bool lok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long long m = m0 + lrow + 32 * i;
        lok[i] = m < M;
        const long long mc = lok[i] ? m : 0;
        const long long b = mc / HW;
        const int pix = int(mc - b * HW);
        ly[i] = pix / w;
        lx[i] = pix - ly[i] * w;
        lbase[i] = b * HW;
    }
    const int cchunks = C / KC, nk = 9 * cchunks;
    float4 ra[4], rb0, rb1;
    f32x16 acc[NTL];
#pragma unroll
    for (int nt = 0; nt < NTL; ++nt) acc[nt] = f32x16{0};
    // iteration kc stages chunk kc - 1 (held in registers), loads chunk kc, then multiplies chunk kc - 1
    for (int kc = 0; kc <= nk; ++kc) {
        if (kc > 0) {
            if (kc > 1) __syncthreads();
#pragma unroll
            for (int i = 0; i < 4; ++i) *reinterpret_cast<float4*>(&As[(lrow + 32 * i) * KP + 4 * q]) = ra[i];
            *reinterpret_cast<float4*>(&Bs[lrow * KP + 4 * q]) = rb0;
            if constexpr (NTL > 1) *reinterpret_cast<float4*>(&Bs[(lrow + 32) * KP + 4 * q]) = rb1;
            __syncthreads();
        }
        if (kc < nk) {
            const int t = kc / cchunks, c0 = (kc - t * cchunks) * KC, kh = t / 3, kw = t - kh * 3;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int yy = ly[i] + kh - 1, xx = lx[i] + kw - 1;
                const bool ok = lok[i] && yy >= 0 && yy < h && xx >= 0 && xx < w;
                ra[i] = ok ? *reinterpret_cast<const float4*>(in + (lbase[i] + yy * w + xx) * C + c0 + 4 * q)
                           : make_float4(0.f, 0.f, 0.f, 0.f);
            }
            const float* wp = wt + (long long)(n0 + lrow) * 9 * C + t * C + c0 + 4 * q;
            rb0 = *reinterpret_cast<const float4*>(wp);
            if constexpr (NTL > 1) rb1 = *reinterpret_cast<const float4*>(wp + 32 * 9 * C);
        }
        if (kc == 0) continue;
        float4 a4[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) a4[j] = *reinterpret_cast<const float4*>(&As[(wv * 32 + r) * KP + 16 * hh + 4 * j]);
#pragma unroll
        for (int nt = 0; nt < NTL; ++nt) {
            float4 b4[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) b4[j] = *reinterpret_cast<const float4*>(&Bs[(nt * 32 + r) * KP + 16 * hh + 4 * j]);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[j].x, b4[j].x, acc[nt], 0, 0, 0);
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[j].y, b4[j].y, acc[nt], 0, 0, 0);
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[j].z, b4[j].z, acc[nt], 0, 0, 0);
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[j].w, b4[j].w, acc[nt], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int nt = 0; nt < NTL; ++nt) {
        const int n = n0 + nt * 32 + r;
        const float bn = bias ? bias[n] : 0.f;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const long long mo = m0 + wv * 32 + acc_row(reg, hh);
            if (mo < M) out[mo * N + n] = acc[nt][reg] + bn;
        }
    }
}

// wgrad partial of a 3x3, pad 1 conv: slab[s][co][t Cin + ci] = sum over the pixels m of range s of dz[m][co] *
// in[pixel m shifted by tap t][ci]; slab[s][co][9 Cin] = sum of dz[m][co] (written by the blockIdx.z == 0 blocks).
// Workgroup tile: 32 WM output channels x 32 NTL WN input channels of one tap (blockIdx.z = tap x Cin tiles); a K chunk is
// 32 pixels, staged as As[px][co] / Bs[px][ci] (channels contiguous, as in global memory).
template <int WM, int WN, int NTL>
__global__ __launch_bounds__(64 * WM * WN) void wgrad3x3_kernel(const float* __restrict__ dz, int Cout,
                                                                const float* __restrict__ in, int Cin, int h, int w,
                                                                long long M, int S, float* __restrict__ slab) {
    constexpr int NTH = 64 * WM * WN, BM = 32 * WM, BN = 32 * NTL * WN, AQ = BM / 4, BQ = BN / 4;
    constexpr int NA = (KC * AQ + NTH - 1) / NTH, NBL = (KC * BQ + NTH - 1) / NTH;
    __shared__ __attribute__((aligned(16))) float As[KC * BM];
    __shared__ __attribute__((aligned(16))) float Bs[KC * BN];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, wm = wv % WM, wn = wv / WM, r = lane & 31, hh = lane >> 5;
    const int co0 = blockIdx.y * BM, cit = Cin / BN, t = blockIdx.z / cit, ci0 = (blockIdx.z - t * cit) * BN;
    const int kh = t / 3, kw = t - kh * 3, HW = h * w;
    const long long r0 = range_lo(blockIdx.x, S, M), r1 = range_lo(blockIdx.x + 1, S, M);
    const bool bias_blk = blockIdx.z == 0;
    float4 ra[NA], rb[NBL];
    auto load = [&](long long mb) {
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int e = tid + i * NTH, px = e / AQ, qq = e - px * AQ;
            const long long m = mb + px;
            ra[i] = (e < KC * AQ && m < r1) ? *reinterpret_cast<const float4*>(dz + m * Cout + co0 + 4 * qq)
                                             : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int i = 0; i < NBL; ++i) {
            const int e = tid + i * NTH, px = e / BQ, qq = e - px * BQ;
            const long long m = mb + px;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (e < KC * BQ && m < r1) {
                const int b = int(m) / HW, pix = int(m) - b * HW, y = pix / w, x = pix - y * w, yy = y + kh - 1,
                          xx = x + kw - 1;
                if (yy >= 0 && yy < h && xx >= 0 && xx < w)
                    v = *reinterpret_cast<const float4*>(in + (long long)(b * HW + yy * w + xx) * Cin + ci0 + 4 * qq);
            }
            rb[i] = v;
        }
    };
    f32x16 acc[NTL];
#pragma unroll
    for (int nt = 0; nt < NTL; ++nt) acc[nt] = f32x16{0};
    float accb = 0.f;
    if (r0 < r1) load(r0);
    for (long long mb = r0; mb < r1; mb += KC) {
        if (mb != r0) __syncthreads();
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int e = tid + i * NTH;
            if (e < KC * AQ) *reinterpret_cast<float4*>(&As[(e / AQ) * BM + 4 * (e % AQ)]) = ra[i];
        }
#pragma unroll
        for (int i = 0; i < NBL; ++i) {
            const int e = tid + i * NTH;
            if (e < KC * BQ) *reinterpret_cast<float4*>(&Bs[(e / BQ) * BN + 4 * (e % BQ)]) = rb[i];
        }
        __syncthreads();
        if (mb + KC < r1) load(mb + KC);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int k = 16 * hh + j;
            const float a = As[k * BM + wm * 32 + r];
#pragma unroll
            for (int nt = 0; nt < NTL; ++nt)
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Bs[k * BN + wn * 32 * NTL + nt * 32 + r], acc[nt], 0, 0, 0);
        }
        if (bias_blk && tid < BM)
#pragma unroll 8
            for (int px = 0; px < KC; ++px) accb += As[px * BM + tid];
    }
    const int ld = 9 * Cin + 1;
    float* dst = slab + (long long)blockIdx.x * Cout * ld;
#pragma unroll
    for (int nt = 0; nt < NTL; ++nt) {
        const int col = t * Cin + ci0 + wn * 32 * NTL + nt * 32 + r;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) dst[(long long)(co0 + wm * 32 + acc_row(reg, hh)) * ld + col] = acc[nt][reg];
    }
    if (bias_blk && tid < BM) dst[(long long)(co0 + tid) * ld + 9 * Cin] = accb;
}

// ------------------------------------------------------------------------------------------ BatchNorm
// BN k of block k, with what its backward needs: z [B h w][C] (pre-BN), stat [4][C] (mean, invstd, sum dy,
// sum dy * xhat), the pool's argmax idx [B ph pw][C], the gradient of the block's output da ([B ph pw][C], or for the last
// block dgap [B][C] = the gradient of every pooled pixel) and the Dropout2d keep mask of its planes
struct BnSrc {
    const float* z;
    const float* st;
    const float* g;
    const float* bt;
    const unsigned char* idx;
    const float* da;
    const float* mask;
    int C, h, w, ph, pw, moff, gap;
    float scale;
};

// part[s][C][3] = (count, mean, centred sum of squares) of the rows of range s of z [M][C]; thread (g, c) takes channel c
// of rows g, g + 256 / C, ...
__global__ __launch_bounds__(NT) void stats_part_kernel(const float* __restrict__ z, long long M, int C, int S,
                                                        float* __restrict__ part) {
    __shared__ float red[NT];
    __shared__ float smean[256];
    const int tid = threadIdx.x, G = NT / C, g = tid / C, c = tid - g * C;
    const long long r0 = range_lo(blockIdx.x, S, M), r1 = range_lo(blockIdx.x + 1, S, M);
    const float n = float(r1 - r0);
    float s = 0.f;
    for (long long r = r0 + g; r < r1; r += G) s += z[r * C + c];
    red[tid] = s;
    __syncthreads();
    if (tid < C) {
        float t = 0.f;
        for (int i = 0; i < G; ++i) t += red[i * C + tid];
        smean[tid] = n > 0.f ? t / n : 0.f;
    }
    __syncthreads();
    const float mu = smean[c];
    float q = 0.f;
    for (long long r = r0 + g; r < r1; r += G) {
        const float d = z[r * C + c] - mu;
        q += d * d;
    }
    red[tid] = q;
    __syncthreads();
    if (tid < C) {
        float t = 0.f;
        for (int i = 0; i < G; ++i) t += red[i * C + tid];
        float* o = part + ((long long)blockIdx.x * C + tid) * 3;
        o[0] = n;
        o[1] = smean[tid];
        o[2] = t;
    }
}

// out[b][py][px][c] = max over the 2x2 window of relu(bn(z)), times the plane's keep / (1 - p); idx = the window's argmax
// (dy * 2 + dx).  One thread per pooled value.
__global__ __launch_bounds__(NT) void bn_pool_drop_kernel(BnSrc a, long long n, float* __restrict__ out,
                                                          unsigned char* __restrict__ idx) {
    const int C = a.C, lc = __ffs(C) - 1;                  // C is a power of two
    for (long long e = (long long)blockIdx.x * NT + threadIdx.x; e < n; e += (long long)gridDim.x * NT) {
        const int pp = int(e >> lc), c = int(e & (C - 1));
        const int b = pp / (a.ph * a.pw), rem = pp - b * a.ph * a.pw, py = rem / a.pw, px = rem - py * a.pw;
        const float* src = a.z + (long long)((b * a.h + 2 * py) * a.w + 2 * px) * C + c;
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = fmaxf(bn_act(src[((q >> 1) * a.w + (q & 1)) * C], a.st, a.g, a.bt, c, C), 0.f);
        const int j = argmax4(v);
        out[e] = v[j] * (a.mask[(long long)b * MASK_W + a.moff + c] * a.scale);
        idx[e] = (unsigned char)j;
    }
}

// the gradient of BN k's output (after ReLU, pool and Dropout2d routing) at pixel m, channel c
__device__ __forceinline__ float dy_at(const BnSrc& a, long long m, int c) {
    const int HW = a.h * a.w, b = int(m) / HW, pix = int(m) - b * HW, y = pix / a.w, x = pix - y * a.w;
    if (y >= 2 * a.ph || x >= 2 * a.pw) return 0.f;
    const long long pp = (b * a.ph + (y >> 1)) * a.pw + (x >> 1);
    if (a.idx[pp * a.C + c] != (((y & 1) << 1) | (x & 1))) return 0.f;
    if (!(bn_act(a.z[m * a.C + c], a.st, a.g, a.bt, c, a.C) > 0.f)) return 0.f;
    const float d = a.gap ? a.da[(long long)b * a.C + c] : a.da[pp * a.C + c];
    return d * (a.mask[(long long)b * MASK_W + a.moff + c] * a.scale);
}

__device__ __forceinline__ float dz_at(const BnSrc& a, long long m, int c, float inv_n) {
    const int C = a.C;
    const float is = a.st[C + c];
    const float xh = (a.z[m * C + c] - a.st[c]) * is;
    return a.g[c] * is * (dy_at(a, m, c) - a.st[2 * C + c] * inv_n - xh * (a.st[3 * C + c] * inv_n));
}

// part[s][C][2] = (sum dy, sum dy * xhat) over the pooled values of range s (dy is 0 off each window's argmax)
__global__ __launch_bounds__(NT) void bn_bwd_part_kernel(BnSrc a, long long MP, int S, float* __restrict__ part) {
    __shared__ float red[2][NT];
    const int C = a.C, tid = threadIdx.x, G = NT / C, g = tid / C, c = tid - g * C;
    const long long r0 = range_lo(blockIdx.x, S, MP), r1 = range_lo(blockIdx.x + 1, S, MP);
    const float mu = a.st[c], is = a.st[C + c], ks = a.scale;
    float s = 0.f, sx = 0.f;
    for (long long pp = r0 + g; pp < r1; pp += G) {
        const int j = a.idx[pp * C + c];
        const int b = int(pp) / (a.ph * a.pw), rem = int(pp) - b * a.ph * a.pw, py = rem / a.pw, px = rem - py * a.pw;
        const long long m = (b * a.h + 2 * py + (j >> 1)) * a.w + 2 * px + (j & 1);
        const float zv = a.z[m * C + c];
        if (bn_act(zv, a.st, a.g, a.bt, c, C) > 0.f) {
            const float d = (a.gap ? a.da[(long long)b * C + c] : a.da[pp * C + c]) *
                            (a.mask[(long long)b * MASK_W + a.moff + c] * ks);
            s += d;
            sx += d * ((zv - mu) * is);
        }
    }
    red[0][tid] = s;
    red[1][tid] = sx;
    __syncthreads();
    if (tid < C) {
        float t = 0.f, tx = 0.f;
        for (int i = 0; i < G; ++i) { t += red[0][i * C + tid]; tx += red[1][i * C + tid]; }
        float* o = part + ((long long)blockIdx.x * C + tid) * 2;
        o[0] = t;
        o[1] = tx;
    }
}

// dz = gamma * invstd * (dy - sum dy / n - xhat * sum(dy xhat) / n) of every value of BN k (k = 1..3)
__global__ __launch_bounds__(NT) void bn_bwd_apply_kernel(BnSrc a, long long n, float inv_n, float* __restrict__ dz) {
    const int C = a.C, lc = __ffs(C) - 1;                  // C is a power of two
    for (long long e = (long long)blockIdx.x * NT + threadIdx.x; e < n; e += (long long)gridDim.x * NT)
        dz[e] = dz_at(a, e >> lc, int(e & (C - 1)), inv_n);
}

// conv 0's weight gradient: dz0 recomputed per value; slab[s][c][t] = sum over the pixels of range s of dz0 * x under tap
// t, slab[s][c][9] = sum of dz0.  Thread (g, c): channel c of pixels g, g + 8, ...
__global__ __launch_bounds__(NT) void wgrad0_kernel(BnSrc a, const float* __restrict__ x, int B, int H, int W, float inv_n,
                                                    int S, float* __restrict__ slab) {
    __shared__ float red[8 * 320];
    const int tid = threadIdx.x, c = tid & 31, g = tid >> 5;
    const long long M = (long long)B * H * W;
    const long long r0 = range_lo(blockIdx.x, S, M), r1 = range_lo(blockIdx.x + 1, S, M);
    float acc[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) acc[i] = 0.f;
    for (long long m = r0 + g; m < r1; m += 8) {
        const float d = dz_at(a, m, c, inv_n);
        const int b = int(m) / (H * W), pix = int(m) - b * H * W, y = pix / W, xx = pix - y * W;
        const float* src = x + (long long)b * H * W;
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int iy = y + kh - 1, ix = xx + kw - 1;
                if (iy >= 0 && iy < H && ix >= 0 && ix < W) acc[kh * 3 + kw] += d * src[iy * W + ix];
            }
        acc[9] += d;
    }
#pragma unroll
    for (int i = 0; i < 10; ++i) red[g * 320 + c * 10 + i] = acc[i];
    __syncthreads();
    for (int o = tid; o < 320; o += NT) {
        float s = 0.f;
        for (int i = 0; i < 8; ++i) s += red[i * 320 + o];
        slab[(long long)blockIdx.x * 320 + o] = s;
    }
}

// ------------------------------------------------------------------------------------------ head
// one block (256 threads) per clip: mean of the last block's output -> Linear(256, 128) -> ReLU -> dropout ->
// Linear(128, 2) -> weighted CE terms
__global__ __launch_bounds__(NT) void mlp_head_fwd_kernel(const float* __restrict__ a3, int HW, const float* __restrict__ prm,
                                                          const float* __restrict__ mask, float p_fc,
                                                          const long long* __restrict__ targets,
                                                          const float* __restrict__ soft,
                                                          const float* __restrict__ class_w, float* __restrict__ logits,
                                                          float* __restrict__ gap, float* __restrict__ hr,
                                                          float* __restrict__ wnll) {
    __shared__ float sg[256], shd[HID];
    const int c = threadIdx.x, b = blockIdx.x;
    const float* src = a3 + (long long)b * HW * 256 + c;
    float s = 0.f;
    for (int i = 0; i < HW; ++i) s += src[(long long)i * 256];
    const float gv = s / float(HW);
    sg[c] = gv;
    gap[(long long)b * 256 + c] = gv;
    __syncthreads();
    if (c < HID) {
        const float hv = mlp_hidden<256>(prm + FC0_W, prm + FC0_B, sg, c);
        const float scale = p_fc < 1.f ? 1.0f / (1.0f - p_fc) : 0.f;
        hr[(long long)b * HID + c] = hv;
        shd[c] = hv * (mask[(long long)b * MASK_W + MOFF[NB] + c] * scale);
    }
    __syncthreads();
    if (c == 0) mlp_out<HID>(prm + FC3_W, prm + FC3_B, shd, b, targets, soft, class_w, logits, wnll);
}

// ------------------------------------------------------------------------------------------ workspace
// wgrad tiles: block 1 64 x 32 (2 waves), blocks 2, 3 64 x 64 (4 waves)
constexpr int WG_BM = 64;
constexpr int wg_bn(int k) { return k == 1 ? 32 : 64; }

struct Shapes {
    int h[NB + 1], w[NB + 1];  // block k's image; h[k + 1] = h[k] / 2 (its pooled output)
    long long M[NB];           // B h w of block k
    int S;                     // pixel ranges of the BN partial sums
    int Sw[NB];                // pixel ranges of block k's weight gradient
};
Shapes make_shapes(int B, int H, int W) {
    Shapes s;
    s.h[0] = H; s.w[0] = W;
    for (int k = 1; k <= NB; ++k) { s.h[k] = s.h[k - 1] / 2; s.w[k] = s.w[k - 1] / 2; }
    for (int k = 0; k < NB; ++k) s.M[k] = (long long)B * s.h[k] * s.w[k];
    s.S = int(std::min<long long>(1024, std::max<long long>(1, (s.M[0] * 32 + 65535) / 65536)));
    s.Sw[0] = int(std::min<long long>(1024, std::max<long long>(1, s.M[0] / 2048)));
    for (int k = 1; k < NB; ++k) {
        const long long tiles = (long long)(CH[k] / WG_BM) * 9 * (CI[k] / wg_bn(k));
        const long long want = (2048 + tiles - 1) / tiles, most = std::max<long long>(1, s.M[k] / 256);
        s.Sw[k] = int(std::max<long long>(1, std::min(want, most)));
    }
    return s;
}

struct Ws {
    float *wt, *wd;
    float *z[NB], *a[NB], *da[NB], *dz[NB];
    unsigned char* idx[NB];
    float* stat[NB];
    float *part, *slab, *mask, *gap, *hr, *dh, *dgap, *wnll, *dl;
    size_t total;
};

Ws carve(char* base, int B, const Shapes& s) {
    Ws w{};
    Carver ws{base};
    auto f = [&](long long n) { return ws.floats(n); };
    w.wt = f(N_PARAMS);
    w.wd = f(N_PARAMS);
    long long slab_most = (long long)s.Sw[0] * 320;
    for (int k = 0; k < NB; ++k) {
        const long long pooled = (long long)B * s.h[k + 1] * s.w[k + 1] * CH[k];
        w.z[k] = f(s.M[k] * CH[k]);
        w.a[k] = f(pooled);
        w.idx[k] = reinterpret_cast<unsigned char*>(ws.take(size_t(pooled)));
        if (k < NB - 1) w.da[k] = f(pooled);
        if (k > 0) {
            w.dz[k] = f(s.M[k] * CH[k]);
            slab_most = std::max(slab_most, (long long)s.Sw[k] * CH[k] * (9 * CI[k] + 1));
        }
        w.stat[k] = f(4 * CH[k]);
    }
    w.part = f((long long)s.S * 256 * 3);
    w.slab = f(slab_most);
    w.mask = f((long long)B * MASK_W);
    w.gap = f((long long)B * 256);
    w.dgap = f((long long)B * 256);
    w.hr = f((long long)B * HID);
    w.dh = f((long long)B * HID);
    w.wnll = f(2LL * B);
    w.dl = f(2LL * B);
    w.total = ws.off;
    return w;
}

constexpr int GRID_CAP = 8192;    // blocks of a grid-stride launch

// the shapes torch's train-mode forward accepts: four 2x2 pools need H, W >= 16 (the last BN then sees B (H/8) (W/8) >= 4
// values per channel); the pixel count of the largest image must fit the 32-bit pixel arithmetic of the kernels
bool trainable(int B, int H, int W) {
    if (B < 1 || H < 16 || W < 16) return false;
    return (long long)B * H * W <= (1LL << 27);
}

// The step behind cough_train_std_forward_backward (d_targets: class indices, d_soft null) and
// cough_train_std_forward_backward_soft of libcough_amd_soft.so (d_soft: [B][2] class probabilities, d_targets null); fn
// names the entry point in the messages.  The two differ in what the two head kernels read, nowhere else.
int train_step(const char* fn, const float* d_x, int n_clips, int height, int width, const long long* d_targets,
               const float* d_soft, const float* d_class_weights, const float* d_dropout_mask, unsigned long long seed,
               unsigned long long offset, float p_block, float p_fc, const float* d_params, float* d_grads, float* d_running,
               long long* d_num_batches, float momentum, float eps, float* d_loss, float* d_logits, float* d_mask_out,
               void* d_workspace, size_t workspace_bytes, void* stream) {
    COUGH_REQUIRE(n_clips >= 1 && height >= 1 && width >= 1, COUGH_EINVAL, "%s: bad shape (%d, %d, %d)", fn, n_clips, height,
                  width);
    COUGH_REQUIRE(height >= 16 && width >= 16, COUGH_EINVAL, "%s: input %dx%d too small for the network (four 2x2 pools)", fn,
                  height, width);
    COUGH_REQUIRE(trainable(n_clips, height, width), COUGH_EINVAL, "%s: batch of %d images of %dx%d too large", fn, n_clips,
                  height, width);
    const int B = n_clips, H = height, W = width;
    const Shapes s = make_shapes(B, H, W);
    const Ws w = carve(static_cast<char*>(d_workspace), B, s);
    const void* d_y = d_soft ? static_cast<const void*>(d_soft) : d_targets;
    if (const int rc = check_step_args(fn, {d_x, d_y, d_params, d_grads, d_running, d_num_batches, d_loss, d_logits,
                                                  d_workspace},
                                       {p_block, p_fc}, momentum, eps, d_workspace, workspace_bytes, w.total);
        rc != COUGH_OK)
        return rc;

    hipStream_t st = static_cast<hipStream_t>(stream);
    const float* prm = d_params;
    const int S = s.S;
    const float scale_block = p_block < 1.f ? 1.0f / (1.0f - p_block) : 0.f;
    auto src_of = [&](int k) {
        BnSrc a{w.z[k], w.stat[k], prm + BN_G[k], prm + BN_B[k], w.idx[k], k == NB - 1 ? w.dgap : w.da[k], w.mask,
                CH[k], s.h[k], s.w[k], s.h[k + 1], s.w[k + 1], MOFF[k], k == NB - 1 ? 1 : 0, scale_block};
        return a;
    };
    auto conv = [&](const float* in, int C, int k, const float* wts, const float* bias, int N, float* out) {
        const dim3 grid(unsigned((s.M[k] + 127) / 128), unsigned(N / (N == 32 ? 32 : 64)));
        if (N == 32) hipLaunchKernelGGL((conv3x3_kernel<1>), grid, dim3(256), 0, st, in, C, s.h[k], s.w[k], s.M[k], wts, bias, N, out);
        else hipLaunchKernelGGL((conv3x3_kernel<2>), grid, dim3(256), 0, st, in, C, s.h[k], s.w[k], s.M[k], wts, bias, N, out);
    };

    // ---- forward
    hipLaunchKernelGGL(mask_kernel, dim3(unsigned((B * MASK_W + NT - 1) / NT)), dim3(NT), 0, st, B, d_dropout_mask, seed,
                       offset, p_block, p_fc, w.mask, d_mask_out);
    hipLaunchKernelGGL(prep_weights_kernel, dim3(64, 3), dim3(NT), 0, st, prm, w.wt, w.wd);
    hipLaunchKernelGGL(conv0_fwd_kernel, dim3(grid_for(s.M[0] * 32, GRID_CAP)), dim3(NT), 0, st, d_x, B, H, W, prm, w.z[0]);
    for (int k = 0; k < NB; ++k) {
        if (k > 0) conv(w.a[k - 1], CI[k], k, w.wt + CONV_W[k], prm + CONV_B[k], CH[k], w.z[k]);
        hipLaunchKernelGGL(stats_part_kernel, dim3(S), dim3(NT), 0, st, w.z[k], s.M[k], CH[k], S, w.part);
        hipLaunchKernelGGL(stats_finalize_kernel, dim3(CH[k]), dim3(NT), 0, st, w.part, S, CH[k], eps, momentum,
                           d_running + RUN[k], d_running + RUN[k] + CH[k], d_num_batches + k, w.stat[k]);
        const long long pooled = (long long)B * s.h[k + 1] * s.w[k + 1] * CH[k];
        hipLaunchKernelGGL(bn_pool_drop_kernel, dim3(grid_for(pooled, GRID_CAP)), dim3(NT), 0, st, src_of(k), pooled, w.a[k],
                           w.idx[k]);
    }
    const int HW4 = s.h[NB] * s.w[NB];
    hipLaunchKernelGGL(mlp_head_fwd_kernel, dim3(B), dim3(NT), 0, st, w.a[NB - 1], HW4, prm, w.mask, p_fc, d_targets, d_soft,
                       d_class_weights, d_logits, w.gap, w.hr, w.wnll);

    // ---- backward
    hipLaunchKernelGGL((mlp_head_bwd_kernel<256, HID, MASK_W, MOFF[NB]>), dim3(B), dim3(NT), 0, st, B, HW4, d_logits,
                       d_targets, d_soft, d_class_weights, w.wnll, w.hr, w.mask, p_fc, prm + FC0_W, prm + FC3_W, w.stat[0],
                       CH[0], d_loss, w.dl, w.dh, w.dgap);
    hipLaunchKernelGGL((mlp_fc_grad_kernel<256, HID, MASK_W, MOFF[NB]>), dim3((256 * HID + 3 * HID + 2 + 63) / 64), dim3(NT),
                       0, st, B, w.gap, w.hr, w.mask, p_fc, w.dl, w.dh, d_grads + FC0_W);
    for (int k = NB - 1; k >= 0; --k) {
        const BnSrc a = src_of(k);
        const long long MP = (long long)B * s.h[k + 1] * s.w[k + 1];
        hipLaunchKernelGGL(bn_bwd_part_kernel, dim3(S), dim3(NT), 0, st, a, MP, S, w.part);
        hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(CH[k]), dim3(NT), 0, st, w.part, S, CH[k], w.stat[k],
                           d_grads + BN_G[k], d_grads + BN_B[k]);
        const float inv_n = float(1.0 / double(s.M[k]));
        const int Sw = s.Sw[k];
        if (k > 0) {
            hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(grid_for(s.M[k] * CH[k], GRID_CAP)), dim3(NT), 0, st, a, s.M[k] * CH[k],
                               inv_n, w.dz[k]);
            const dim3 g(unsigned(Sw), unsigned(CH[k] / WG_BM), unsigned(9 * (CI[k] / wg_bn(k))));
            if (k == 1)
                hipLaunchKernelGGL((wgrad3x3_kernel<2, 1, 1>), g, dim3(128), 0, st, w.dz[k], CH[k], w.a[k - 1], CI[k],
                                   s.h[k], s.w[k], s.M[k], Sw, w.slab);
            else
                hipLaunchKernelGGL((wgrad3x3_kernel<2, 2, 1>), g, dim3(256), 0, st, w.dz[k], CH[k], w.a[k - 1], CI[k],
                                   s.h[k], s.w[k], s.M[k], Sw, w.slab);
            conv(w.dz[k], CH[k], k, w.wd + CONV_W[k], nullptr, CI[k], w.da[k - 1]);
        } else {
            hipLaunchKernelGGL(wgrad0_kernel, dim3(Sw), dim3(NT), 0, st, a, d_x, B, H, W, inv_n, Sw, w.slab);
        }
        const int kcols = 9 * CI[k], nout = CH[k] * (kcols + 1);
        hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((nout + NT - 1) / NT), dim3(NT), 0, st, w.slab, Sw, CH[k], kcols + 1,
                           kcols, CI[k], 9, d_grads + CONV_W[k], d_grads + CONV_B[k]);
    }
    COUGH_HIP_CHECK(hipGetLastError());
    return COUGH_OK;
}

}  // namespace
}  // namespace cough

#ifdef COUGH_SOFT_EXPORTS   // the second compilation of this file, for libcough_amd_soft.so: the soft entry point alone
#include "../../include/cough_amd_soft.h"

extern "C" int cough_train_std_forward_backward_soft(const float* d_x, int n_clips, int height, int width,
                                                     const float* d_soft_targets, const float* d_class_weights,
                                                     const float* d_dropout_mask, unsigned long long seed,
                                                     unsigned long long offset, float p_block, float p_fc,
                                                     const float* d_params, float* d_grads, float* d_running,
                                                     long long* d_num_batches, float momentum, float eps, float* d_loss,
                                                     float* d_logits, float* d_mask_out, void* d_workspace,
                                                     size_t workspace_bytes, void* stream) {
    return cough::train_step(__func__, d_x, n_clips, height, width, nullptr, d_soft_targets, d_class_weights, d_dropout_mask,
                             seed, offset, p_block, p_fc, d_params, d_grads, d_running, d_num_batches, momentum, eps, d_loss,
                             d_logits, d_mask_out, d_workspace, workspace_bytes, stream);
}
#else
extern "C" size_t cough_train_std_workspace_bytes(int n_clips, int height, int width) {
    using namespace cough;
    if (!trainable(n_clips, height, width)) return 0;
    return carve(nullptr, n_clips, make_shapes(n_clips, height, width)).total;
}

extern "C" int cough_train_std_forward_backward(const float* d_x, int n_clips, int height, int width,
                                                const long long* d_targets, const float* d_class_weights,
                                                const float* d_dropout_mask, unsigned long long seed,
                                                unsigned long long offset, float p_block, float p_fc,
                                                const float* d_params, float* d_grads, float* d_running,
                                                long long* d_num_batches, float momentum, float eps, float* d_loss,
                                                float* d_logits, float* d_mask_out, void* d_workspace,
                                                size_t workspace_bytes, void* stream) {
    return cough::train_step(__func__, d_x, n_clips, height, width, d_targets, nullptr, d_class_weights, d_dropout_mask, seed,
                             offset, p_block, p_fc, d_params, d_grads, d_running, d_num_batches, momentum, eps, d_loss,
                             d_logits, d_mask_out, d_workspace, workspace_bytes, stream);
}
#endif
