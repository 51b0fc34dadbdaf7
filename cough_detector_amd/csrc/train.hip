// Training step of CoughDetectorResidual (channels (32, 64, 128)) for gfx950: the train-mode forward pass, the backward
// pass and clip_grad_norm_ + AdamW, as the reference's train_epoch takes one step (/root/reference/src/train.py:54-112):
//   outputs = model(inputs)                      batch-statistics BatchNorm, Dropout(p) before the Linear head
//   loss = CrossEntropyLoss(weight)(outputs, y); loss.backward()
//   clip_grad_norm_(params, max_norm); AdamW.step()
//
// Everything is exact f32.  Activations are NHWC; parameters, gradients and the BN running statistics are flat caller
// buffers in model.parameters() / model.buffers() order, so the kernels read the module's own tensors.
//
//   convolutions   implicit GEMMs on v_mfma_f32_32x32x2_f32, one 32-row tile per wave:
//                    forward   rows = output pixels,  cols = Cout, K = (kh, kw, Cin)
//                    dgrad     rows = input pixels,   cols = Cin,  K = (kh, kw, Cout)  (taps whose output pixel does
//                                                                                       not exist contribute 0)
//                    wgrad     rows = Cout, cols = (kh, kw, Cin) + one column of ones (the bias gradient, sum of dz),
//                              K = every output pixel of the batch, split into S fixed ranges: each range writes a
//                              partial slab and a second kernel adds the S slabs in index order (no float atomics)
//   BatchNorm      per-channel statistics in two launches: per-range mean and centred sum of squares (two passes over
//                  the range), then a fixed-order Chan merge; backward sums dy and dy * xhat the same way
//   head           one workgroup per clip (global average, dropout, Linear, weighted CE terms), then one workgroup for
//                  the batch (loss, dlogits, dFC, the gradient of the global average)
//   optimizer      one workgroup for the global L2 norm, one elementwise clip + AdamW launch
// Every cross-workgroup reduction runs in a fixed order, so the same inputs and state give bit-identical results.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "common.h"
#include "nn_common.h"
#include "train_common.h"

namespace cough {
namespace {

constexpr int NCONV = 7;        // conv (and BN) order: stem, block0 conv1 / conv2 / skip, block1 conv1 / conv2 / skip
constexpr int HEAD_C = 128;
constexpr int KGEO[NCONV][5] = {  // cin, cout, kernel, stride, pad (model.py: conv1, ResidualBlock)
    {1, 32, 7, 2, 3}, {32, 64, 3, 2, 1}, {64, 64, 3, 1, 1}, {32, 64, 1, 2, 0},
    {64, 128, 3, 2, 1}, {128, 128, 3, 1, 1}, {64, 128, 1, 2, 0}};

struct Layout {
    long long conv_w[NCONV], conv_b[NCONV], bn_g[NCONV], bn_b[NCONV];
    int run[NCONV];               // running_mean of BN i at run[i], running_var at run[i] + C
    long long fc_w, fc_b, n_params;
    int n_running;
};

// model.parameters() order: conv1.0.{weight,bias}, conv1.1.{weight,bias}, then per block conv1, bn1, conv2, bn2, skip.0,
// skip.1 (weight, bias each), then fc.2.{weight,bias} -- conv i is always followed by its BN i
Layout make_layout() {
    Layout L;
    long long o = 0;
    int r = 0;
    for (int i = 0; i < NCONV; ++i) {
        const int cin = KGEO[i][0], cout = KGEO[i][1], k = KGEO[i][2];
        L.conv_w[i] = o; o += (long long)cout * cin * k * k;
        L.conv_b[i] = o; o += cout;
        L.bn_g[i] = o; o += cout;
        L.bn_b[i] = o; o += cout;
        L.run[i] = r; r += 2 * cout;
    }
    L.fc_w = o; o += 2 * HEAD_C;
    L.fc_b = o; o += 2;
    L.n_params = o;
    L.n_running = r;
    return L;
}

struct TShapes {
    int ih[NCONV], iw[NCONV], oh[NCONV], ow[NCONV];   // input / output image of every conv
    int P1h, P1w;                                     // after the stem's maxpool
};
TShapes make_tshapes(int H, int W) {
    TShapes s;
    auto out = [](int n, int k, int st, int p) { return (n + 2 * p - k) / st + 1; };
    s.ih[0] = H; s.iw[0] = W;
    s.oh[0] = out(H, 7, 2, 3); s.ow[0] = out(W, 7, 2, 3);
    s.P1h = s.oh[0] / 2; s.P1w = s.ow[0] / 2;
    int h = s.P1h, w = s.P1w;
    for (int blk = 0; blk < 2; ++blk) {
        const int c1 = 1 + 3 * blk, c2 = c1 + 1, sk = c1 + 2;
        const int oh = out(h, 3, 2, 1), ow = out(w, 3, 2, 1);
        s.ih[c1] = h; s.iw[c1] = w; s.oh[c1] = oh; s.ow[c1] = ow;
        s.ih[c2] = oh; s.iw[c2] = ow; s.oh[c2] = oh; s.ow[c2] = ow;
        s.ih[sk] = h; s.iw[sk] = w; s.oh[sk] = out(h, 1, 2, 0); s.ow[sk] = out(w, 1, 2, 0);
        h = oh; w = ow;
    }
    return s;
}

// ------------------------------------------------------------------------------------------ launch geometry
long long bn_rows_per(long long M) { return std::max<long long>(256, (M + 1023) / 1024); }
int bn_nblk(long long M) { return int((M + bn_rows_per(M) - 1) / bn_rows_per(M)); }

constexpr int WG_NT = 2;          // wgrad: 64 columns per wave
struct WgGeo {
    int kcols, kp, S;
    long long m_per;
};
WgGeo wg_geo(int conv, long long M) {
    WgGeo g;
    const int cin = KGEO[conv][0], cout = KGEO[conv][1], k = KGEO[conv][2];
    g.kcols = k * k * cin;
    g.kp = (g.kcols + 1 + 32 * WG_NT - 1) / (32 * WG_NT) * (32 * WG_NT);
    const long long tiles = (long long)(cout / 32) * (g.kp / (32 * WG_NT));
    const long long want = std::max<long long>(1, (2048 + tiles - 1) / tiles);
    const long long most = std::max<long long>(1, (M + 127) / 128);   // at least 64 MFMA steps per wave
    long long S = std::min(want, most);
    g.m_per = (M + S - 1) / S;
    g.S = int((M + g.m_per - 1) / g.m_per);
    return g;
}

// ------------------------------------------------------------------------------------------ weights
struct PrepArgs {
    long long off[NCONV];
};
// wt[conv]: [cout][kh][kw][cin] (forward B operand); wd[conv]: [cin][kh][kw][cout] (dgrad B operand); same offsets as the
// flat parameters
__global__ __launch_bounds__(256) void prep_weights_kernel(const float* __restrict__ params, float* __restrict__ wt,
                                                           float* __restrict__ wd, PrepArgs a) {
    const int conv = blockIdx.y;
    int cin = 0, cout = 0, kk = 0;
#pragma unroll
    for (int i = 0; i < NCONV; ++i)
        if (i == conv) { cin = KGEO[i][0]; cout = KGEO[i][1]; kk = KGEO[i][2] * KGEO[i][2]; }
    const long long off = a.off[conv];
    const int n = cout * cin * kk;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < n; e += gridDim.x * 256) {
        const int co = e / (cin * kk), rem = e - co * cin * kk, ci = rem / kk, t = rem - ci * kk;
        const float v = params[off + e];
        wt[off + (co * kk + t) * cin + ci] = v;
        wd[off + (ci * kk + t) * cout + co] = v;
    }
}

// ------------------------------------------------------------------------------------------ convolutions
// stem forward: z[m][32] = conv7x7 s2 p3 (x) + bias, m = (b, oh, ow); K = 49 taps, two per MFMA
__global__ __launch_bounds__(256) void stem_fwd_kernel(const float* __restrict__ x, int H, int W, int OH, int OW, long long M,
                                                       const float* __restrict__ w /* [32][49] */,
                                                       const float* __restrict__ bias, float* __restrict__ z) {
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const long long m0 = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 32;
    if (m0 >= M) return;
    const long long m = m0 + r;
    const bool rowok = m < M;
    const long long mc = rowok ? m : 0;
    const int per = OH * OW;
    const int b = int(mc / per), rem = int(mc - (long long)b * per), oh = rem / OW, ow = rem - oh * OW;
    const float* src = x + (long long)b * H * W;
    const int ih0 = 2 * oh - 3, iw0 = 2 * ow - 3;
    f32x16 acc = {0};
#pragma unroll
    for (int ks = 0; ks < 25; ++ks) {
        const int k = 2 * ks + h;
        const int kh = k < 49 ? k / 7 : 0, kw = k < 49 ? k % 7 : 0;
        const float bw = k < 49 ? w[r * 49 + k] : 0.f;
        const int ih = ih0 + kh, iw = iw0 + kw;
        float av = 0.f;
        if (k < 49 && rowok && ih >= 0 && ih < H && iw >= 0 && iw < W) av = src[ih * W + iw];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bw, acc, 0, 0, 0);
    }
    const float bn = bias[r];
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const long long mo = m0 + acc_row(reg, h);
        if (mo < M) z[mo * 32 + r] = acc[reg] + bn;
    }
}

struct IgArgs {
    const float* in;     // NHWC [B][IH][IW][C]: forward -> the conv input; dgrad -> dz (the conv output gradient)
    const float* w;      // [N][KH][KW][C]
    const float* bias;   // [N] or nullptr
    float* out;          // [M][N], rows (b, oh, ow) of an OH x OW grid
    long long M;
    int C, N, IH, IW, OH, OW, KH, KW, stride, pad, accumulate;
};

// DG = false: out = conv(in) + bias.  DG = true: out (+)= the input gradient of a conv with this geometry (OH x OW = the
// conv's input image, IH x IW = its output image).  C % 8 == 0: 8 channels per chunk, k-slot h of MFMA e <-> channel 4h+e.
template <int NT, bool DG>
__global__ __launch_bounds__(256) void conv_gemm_kernel(IgArgs a) {
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const long long m0 = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 32;
    if (m0 >= a.M) return;
    const long long m = m0 + r;
    const bool rowok = m < a.M;
    const long long mc = rowok ? m : 0;
    const int per = a.OH * a.OW;
    const int b = int(mc / per), rem = int(mc - (long long)b * per), oh = rem / a.OW, ow = rem - oh * a.OW;
    f32x16 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = f32x16{0};
    const int n_base = blockIdx.y * 32 * NT;
    const int ktot = a.KH * a.KW * a.C;
    const float* wrow[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) wrow[nt] = a.w + (long long)(n_base + nt * 32 + r) * ktot;
    int kbase = 0;
    for (int kh = 0; kh < a.KH; ++kh)
        for (int kw = 0; kw < a.KW; ++kw, kbase += a.C) {
            int ih, iw;
            bool ok;
            if constexpr (DG) {
                const int ty = oh + a.pad - kh, tx = ow + a.pad - kw;
                ih = ty / a.stride; iw = tx / a.stride;
                ok = rowok && ty >= 0 && tx >= 0 && ih * a.stride == ty && iw * a.stride == tx && ih < a.IH && iw < a.IW;
            } else {
                ih = oh * a.stride - a.pad + kh; iw = ow * a.stride - a.pad + kw;
                ok = rowok && ih >= 0 && ih < a.IH && iw >= 0 && iw < a.IW;
            }
            const float* ap = a.in + (((long long)b * a.IH + (ok ? ih : 0)) * a.IW + (ok ? iw : 0)) * a.C;
            for (int c0 = 0; c0 < a.C; c0 += 8) {
                float4 av = make_float4(0.f, 0.f, 0.f, 0.f);
                if (ok) av = *reinterpret_cast<const float4*>(ap + c0 + 4 * h);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const float4 bv = *reinterpret_cast<const float4*>(wrow[nt] + kbase + c0 + 4 * h);
                    acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, acc[nt], 0, 0, 0);
                    acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, acc[nt], 0, 0, 0);
                    acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, acc[nt], 0, 0, 0);
                    acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, acc[nt], 0, 0, 0);
                }
            }
        }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int n = n_base + nt * 32 + r;
        const float bn = a.bias ? a.bias[n] : 0.f;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const long long mo = m0 + acc_row(reg, h);
            if (mo < a.M) {
                float v = acc[nt][reg] + bn;
                if (a.accumulate) v = a.out[mo * a.N + n] + v;
                a.out[mo * a.N + n] = v;
            }
        }
    }
}

struct WgArgs {
    const float* dz;     // [M][N] conv output gradient, rows (b, oh, ow) of the OH x OW output image
    const float* x;      // NHWC [B][IH][IW][C] conv input
    float* slab;         // [S][N][kp]
    long long M, m_per;
    int N, C, IH, IW, OH, OW, KW, stride, pad, kcols, kp;
};

// wgrad partial: slab[s][co][col] = sum over the output pixels m of range s of dz[m][co] * X[m][col], X[m][col] = the
// input value under tap col = (kh, kw, ci) of pixel m; col == kcols is the constant 1 (bias gradient).  One wave per
// (range, 32 output channels, 64 columns); k-slot h of every MFMA <-> pixel m + h.
__global__ __launch_bounds__(64) void wgrad_kernel(WgArgs a) {
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const int co = blockIdx.y * 32 + r;
    int kind[WG_NT], tkh[WG_NT], tkw[WG_NT], tci[WG_NT];   // kind 0: data tap, 1: the ones column, 2: padding
#pragma unroll
    for (int nt = 0; nt < WG_NT; ++nt) {
        const int col = blockIdx.z * 32 * WG_NT + nt * 32 + r;
        kind[nt] = col < a.kcols ? 0 : (col == a.kcols ? 1 : 2);
        const int cc = col < a.kcols ? col : 0;
        tkh[nt] = cc / (a.KW * a.C);
        const int rem = cc - tkh[nt] * a.KW * a.C;
        tkw[nt] = rem / a.C;
        tci[nt] = rem - tkw[nt] * a.C;
    }
    const long long m_begin = (long long)blockIdx.x * a.m_per;
    const long long m_end = std::min(a.M, m_begin + a.m_per);
    long long m = m_begin + h;
    const int per = a.OH * a.OW;
    const long long mc = m < a.M ? m : 0;
    int b = int(mc / per), rem = int(mc - (long long)b * per), oh = rem / a.OW, ow = rem - oh * a.OW;
    f32x16 acc[WG_NT];
#pragma unroll
    for (int nt = 0; nt < WG_NT; ++nt) acc[nt] = f32x16{0};
    for (long long mm = m_begin; mm < m_end; mm += 2, m += 2) {
        const bool valid = m < m_end;
        const float av = valid ? a.dz[m * a.N + co] : 0.f;
        float bv[WG_NT];
#pragma unroll
        for (int nt = 0; nt < WG_NT; ++nt) {
            const int ih = oh * a.stride - a.pad + tkh[nt], iw = ow * a.stride - a.pad + tkw[nt];
            const bool in = valid && kind[nt] == 0 && ih >= 0 && ih < a.IH && iw >= 0 && iw < a.IW;
            bv[nt] = in ? a.x[(((long long)b * a.IH + ih) * a.IW + iw) * a.C + tci[nt]] : 0.f;
            if (kind[nt] == 1) bv[nt] = valid ? 1.f : 0.f;
        }
#pragma unroll
        for (int nt = 0; nt < WG_NT; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[nt], acc[nt], 0, 0, 0);
        ow += 2;
        while (ow >= a.OW) { ow -= a.OW; ++oh; }
        while (oh >= a.OH) { oh -= a.OH; ++b; }
    }
    float* dst = a.slab + ((long long)blockIdx.x * a.N + blockIdx.y * 32) * a.kp + blockIdx.z * 32 * WG_NT;
#pragma unroll
    for (int nt = 0; nt < WG_NT; ++nt)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) dst[(long long)acc_row(reg, h) * a.kp + nt * 32 + r] = acc[nt][reg];
}

// ------------------------------------------------------------------------------------------ BatchNorm
// stat[4][C] per BN: mean, invstd (forward); sum dy, sum dy * xhat (backward)

// rows [blk * rows_per, +rows_per) of z[M][C]: the range mean and the sum of squares about it (two passes)
__global__ __launch_bounds__(256) void bn_stats_partial_kernel(const float* __restrict__ z, long long M, int C,
                                                               long long rows_per, float* __restrict__ part) {
    __shared__ float red[256];
    __shared__ float bmean[128];
    const int tid = threadIdx.x, G = 256 / C, g = tid / C, c = tid - g * C;
    const long long r0 = (long long)blockIdx.x * rows_per, r1 = std::min(M, r0 + rows_per);
    const float nb = float(r1 - r0);
    float s = 0.f;
    if (g < G)
        for (long long r = r0 + g; r < r1; r += G) s += z[r * C + c];
    red[tid] = s;
    __syncthreads();
    if (tid < C) {
        float t = 0.f;
        for (int i = 0; i < G; ++i) t += red[i * C + tid];
        bmean[tid] = t / nb;
    }
    __syncthreads();
    const float mu = bmean[c];
    float q = 0.f;
    if (g < G)
        for (long long r = r0 + g; r < r1; r += G) {
            const float d = z[r * C + c] - mu;
            q += d * d;
        }
    red[tid] = q;
    __syncthreads();
    if (tid < C) {
        float t = 0.f;
        for (int i = 0; i < G; ++i) t += red[i * C + tid];
        part[(2LL * blockIdx.x) * C + tid] = bmean[tid];
        part[(2LL * blockIdx.x + 1) * C + tid] = t;
    }
}

// one block, one thread per channel: Chan merge of the rows_per ranges in index order; batch mean / invstd, running
// statistics (momentum, unbiased variance), num_batches_tracked + 1
__global__ void bn_stats_seq_merge_kernel(const float* __restrict__ part, int nblk, long long M, long long rows_per, int C,
                                          float eps, float momentum, float* __restrict__ run_mean,
                                          float* __restrict__ run_var, long long* __restrict__ nbt,
                                          float* __restrict__ stat) {
    const int c = threadIdx.x;
    if (c >= C) return;
    double n = 0.0, mean = 0.0, m2 = 0.0;
    for (int i = 0; i < nblk; ++i) {
        const double nb = double(std::min(M, (long long)(i + 1) * rows_per) - (long long)i * rows_per);
        const double mb = part[(2LL * i) * C + c], m2b = part[(2LL * i + 1) * C + c];
        const double nt = n + nb, d = mb - mean;
        mean += d * nb / nt;
        m2 += m2b + d * d * n * nb / nt;
        n = nt;
    }
    const float var = float(m2 / n), uvar = float(m2 / (n - 1.0)), mu = float(mean);
    stat[c] = mu;
    stat[C + c] = 1.0f / sqrtf(var + eps);
    run_mean[c] = momentum * mu + (1.0f - momentum) * run_mean[c];
    run_var[c] = momentum * uvar + (1.0f - momentum) * run_var[c];
    if (c == 0) nbt[0] += 1;
}

// y = relu(bn(z))
__global__ __launch_bounds__(256) void bn_relu_kernel(const float* __restrict__ z, long long n, int C,
                                                      const float* __restrict__ stat, const float* __restrict__ g,
                                                      const float* __restrict__ bt, float* __restrict__ y) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const int c = int(e % C);
        y[e] = fmaxf(bn_act(z[e], stat, g, bt, c, C), 0.f);
    }
}

// block output: relu(bn2(z2) + bn_skip(zs))
__global__ __launch_bounds__(256) void bn_add_relu_kernel(const float* __restrict__ z2, const float* __restrict__ zs, long long n,
                                                          int C, const float* __restrict__ st2, const float* __restrict__ g2,
                                                          const float* __restrict__ b2, const float* __restrict__ sts,
                                                          const float* __restrict__ gs, const float* __restrict__ bs,
                                                          float* __restrict__ y) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const int c = int(e % C);
        y[e] = fmaxf(bn_act(z2[e], st2, g2, b2, c, C) + bn_act(zs[e], sts, gs, bs, c, C), 0.f);
    }
}

// stem: relu(bn(z)) then maxpool 2 (floor); p = the pooled value, idx = which of the 4 (dy * 2 + dx) holds it
__global__ __launch_bounds__(256) void stem_bn_pool_kernel(const float* __restrict__ z, int OH, int OW, int P1h, int P1w,
                                                           long long n, const float* __restrict__ stat,
                                                           const float* __restrict__ g, const float* __restrict__ bt,
                                                           float* __restrict__ p, unsigned char* __restrict__ idx) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const int c = int(e & 31);
        const long long pi = e >> 5;
        const int per = P1h * P1w;
        const long long b = pi / per;
        const int rem = int(pi - b * per), py = rem / P1w, px = rem - py * P1w;
        float best = 0.f;
        int k = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int oy = 2 * py + (j >> 1), ox = 2 * px + (j & 1);
            const float v = fmaxf(bn_act(z[((b * OH + oy) * OW + ox) * 32 + c], stat, g, bt, c, 32), 0.f);
            if (j == 0 || v > best) { best = v; k = j; }
        }
        p[e] = best;
        idx[e] = (unsigned char)k;
    }
}

// Where a BN's output gradient dy comes from (the ReLU after it folded in):
enum { DY_MASK = 0, DY_GAP = 1, DY_POOL = 2 };
struct DySrc {
    int mode;
    const float* g;            // DY_MASK: gradient of the ReLU output [M][C]
    const float* act;          // DY_MASK / DY_GAP: the ReLU output [M][C]
    const float* dgap;         // DY_GAP: [B][C] gradient of every pixel of clip b (1/HW and dropout included)
    int HW;
    const float* dp;           // DY_POOL: gradient of the pooled stem output [B][P1h][P1w][32]
    const float* p;
    const unsigned char* idx;
    int OH, OW, P1h, P1w;
};

__device__ __forceinline__ float load_dy(const DySrc& s, long long m, int c, int C) {
    if (s.mode == DY_MASK) return s.act[m * C + c] > 0.f ? s.g[m * C + c] : 0.f;
    if (s.mode == DY_GAP) return s.act[m * C + c] > 0.f ? s.dgap[(m / s.HW) * C + c] : 0.f;
    const int per = s.OH * s.OW;
    const long long b = m / per;
    const int rem = int(m - b * per), oy = rem / s.OW, ox = rem - oy * s.OW, py = oy >> 1, px = ox >> 1;
    if (py >= s.P1h || px >= s.P1w) return 0.f;
    const long long pe = ((b * s.P1h + py) * s.P1w + px) * 32 + c;
    return (s.idx[pe] == ((oy & 1) << 1 | (ox & 1)) && s.p[pe] > 0.f) ? s.dp[pe] : 0.f;
}

__global__ __launch_bounds__(256) void bn_bwd_partial_kernel(DySrc src, const float* __restrict__ z,
                                                             const float* __restrict__ stat, long long M, int C,
                                                             long long rows_per, float* __restrict__ part) {
    __shared__ float red[2][256];
    const int tid = threadIdx.x, G = 256 / C, g = tid / C, c = tid - g * C;
    const long long r0 = (long long)blockIdx.x * rows_per, r1 = std::min(M, r0 + rows_per);
    float s = 0.f, sx = 0.f;
    if (g < G) {
        const float mu = stat[c], is = stat[C + c];
        for (long long r = r0 + g; r < r1; r += G) {
            const float dy = load_dy(src, r, c, C);
            s += dy;
            sx += dy * ((z[r * C + c] - mu) * is);
        }
    }
    red[0][tid] = s;
    red[1][tid] = sx;
    __syncthreads();
    if (tid < C) {
        float t = 0.f, tx = 0.f;
        for (int i = 0; i < G; ++i) { t += red[0][i * C + tid]; tx += red[1][i * C + tid]; }
        part[(2LL * blockIdx.x) * C + tid] = t;
        part[(2LL * blockIdx.x + 1) * C + tid] = tx;
    }
}

// one block, one thread per channel: the rows_per ranges summed in index order -> stat[2..3], dgamma = sum dy * xhat,
// dbeta = sum dy
__global__ void bn_bwd_seq_merge_kernel(const float* __restrict__ part, int nblk, int C, float* __restrict__ stat,
                                        float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int c = threadIdx.x;
    if (c >= C) return;
    float s = 0.f, sx = 0.f;
    for (int i = 0; i < nblk; ++i) {
        s += part[(2LL * i) * C + c];
        sx += part[(2LL * i + 1) * C + c];
    }
    stat[2 * C + c] = s;
    stat[3 * C + c] = sx;
    dgamma[c] = sx;
    dbeta[c] = s;
}

// dz = gamma * invstd * (dy - sum dy / n - xhat * sum(dy xhat) / n)
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(DySrc src, const float* __restrict__ z,
                                                           const float* __restrict__ stat, const float* __restrict__ gamma,
                                                           long long M, int C, float inv_n, float* __restrict__ dz) {
    const long long n = M * C;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const long long m = e / C;
        const int c = int(e - m * C);
        const float xh = (z[e] - stat[c]) * stat[C + c];
        const float dy = load_dy(src, m, c, C);
        dz[e] = gamma[c] * stat[C + c] * (dy - stat[2 * C + c] * inv_n - xh * (stat[3 * C + c] * inv_n));
    }
}

// ------------------------------------------------------------------------------------------ head
// one workgroup (128 threads = channels) per clip: global average -> dropout -> Linear(128, 2) -> weighted CE terms
__global__ __launch_bounds__(128) void head_fwd_kernel(const float* __restrict__ a, int HW, const float* __restrict__ fcw,
                                                       const float* __restrict__ fcb, const float* __restrict__ mask_in,
                                                       unsigned long long seed, unsigned long long offset, float p,
                                                       const long long* __restrict__ targets,
                                                       const float* __restrict__ soft,
                                                       const float* __restrict__ class_w, float* __restrict__ logits,
                                                       float* __restrict__ dvec, float* __restrict__ mask,
                                                       float* __restrict__ mask_out, float* __restrict__ wnll) {
    __shared__ float red[2][2];
    const int c = threadIdx.x, b = blockIdx.x;
    const float* src = a + (long long)b * HW * HEAD_C + c;
    float s = 0.f;
    for (int i = 0; i < HW; ++i) s += src[(long long)i * HEAD_C];
    const float gap = s / float(HW);
    const float keep = mask_in ? mask_in[(long long)b * HEAD_C + c] : dropout_keep(c, b, seed, offset, p);
    const float scale = p < 1.f ? 1.0f / (1.0f - p) : 0.f;
    const float d = gap * (keep * scale);
    dvec[(long long)b * HEAD_C + c] = d;
    mask[(long long)b * HEAD_C + c] = keep;
    if (mask_out) mask_out[(long long)b * HEAD_C + c] = keep;
    const float l0 = wave_sum(d * fcw[c]), l1 = wave_sum(d * fcw[HEAD_C + c]);
    if ((c & 63) == 0) { red[c >> 6][0] = l0; red[c >> 6][1] = l1; }
    __syncthreads();
    if (c == 0) {
        const float z0 = (red[0][0] + red[1][0]) + fcb[0], z1 = (red[0][1] + red[1][1]) + fcb[1];
        ce_terms(b, z0, z1, targets, soft, class_w, logits, wnll);
    }
}

// one workgroup for the batch: loss, dlogits, dFC, and the gradient reaching every pixel of the last block's output
__global__ __launch_bounds__(256) void head_bwd_kernel(int B, int HW, const float* __restrict__ logits,
                                                       const long long* __restrict__ targets, const float* __restrict__ soft,
                                                       const float* __restrict__ class_w, const float* __restrict__ wnll,
                                                       const float* __restrict__ dvec, const float* __restrict__ mask, float p,
                                                       const float* __restrict__ fcw, const float* __restrict__ stem_stat,
                                                       float* __restrict__ loss, float* __restrict__ dl,
                                                       float* __restrict__ gfcw, float* __restrict__ gfcb,
                                                       float* __restrict__ dgap) {
    __shared__ float red[2][256];
    __shared__ float tot[2];
    const int t = threadIdx.x;
    float s = 0.f, sw = 0.f;
    for (int b = t; b < B; b += 256) { s += wnll[2 * b]; sw += wnll[2 * b + 1]; }
    red[0][t] = s;
    red[1][t] = sw;
    __syncthreads();
    if (t == 0) {
        float a = 0.f, w = 0.f;
        for (int i = 0; i < 256; ++i) { a += red[0][i]; w += red[1][i]; }
        tot[0] = a;
        tot[1] = w;
        // a non-finite input image reaches the stem's batch statistics of every channel (every pixel lies under a
        // window); ReLU and max-pool (v_max_f32) would otherwise drop the NaN before the loss
        const bool finite = isfinite(stem_stat[0]) && isfinite(stem_stat[32]);
        loss[0] = finite ? a / w : __builtin_nanf("");
    }
    __syncthreads();
    const float inv_w = 1.0f / tot[1];
    for (int b = t; b < B; b += 256) {
        const float2 d = clip_dlogits(logits, targets, soft, class_w, b, wnll[2 * b + 1] * inv_w);
        dl[2 * b] = d.x;
        dl[2 * b + 1] = d.y;
    }
    __syncthreads();
    {
        const int j = t >> 7, c = t & 127;
        float g = 0.f;
        for (int b = 0; b < B; ++b) g += dl[2 * b + j] * dvec[(long long)b * HEAD_C + c];
        gfcw[j * HEAD_C + c] = g;
        if (t < 2) {
            float gb = 0.f;
            for (int b = 0; b < B; ++b) gb += dl[2 * b + t];
            gfcb[t] = gb;
        }
    }
    const float scale = (p < 1.f ? 1.0f / (1.0f - p) : 0.f) / float(HW);
    for (long long e = t; e < (long long)B * HEAD_C; e += 256) {
        const long long b = e / HEAD_C;
        const int c = int(e - b * HEAD_C);
        dgap[e] = (dl[2 * b] * fcw[c] + dl[2 * b + 1] * fcw[HEAD_C + c]) * (mask[e] * scale);
    }
}

// ------------------------------------------------------------------------------------------ optimizer
constexpr int NORM_THREADS = 1024;
__global__ __launch_bounds__(NORM_THREADS) void grad_norm_kernel(const float* __restrict__ g, long long n,
                                                                 float* __restrict__ out) {
    __shared__ float red[NORM_THREADS / 64];
    float s = 0.f;
    for (long long i = threadIdx.x; i < n; i += NORM_THREADS) s += g[i] * g[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int w = 0; w < NORM_THREADS / 64; ++w) t += red[w];
        out[0] = sqrtf(t);
    }
}

// clip_grad_norm_ (coef = max_norm / (norm + 1e-6) clamped at 1, always applied; the clipped gradient is written back),
// then torch.optim.AdamW's single-tensor update order.  A NaN norm gives a NaN coefficient, as torch.clamp keeps it
// (fminf would drop the NaN and clip nothing).
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ prm, float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, long long n, const float* __restrict__ norm,
                                                    float max_norm, float lr, float beta1, float beta2, float eps, float wd,
                                                    float step_size, float bc2_sqrt) {
    const float ratio = max_norm / (norm[0] + 1e-6f);
    const float coef = ratio > 1.0f ? 1.0f : ratio;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float gi = g[i] * coef;
        g[i] = gi;
        float p = prm[i] * (1.0f - lr * wd);
        float mi = m[i];
        mi = mi + (1.0f - beta1) * (gi - mi);
        const float vi = v[i] * beta2 + (1.0f - beta2) * gi * gi;
        const float denom = sqrtf(vi) / bc2_sqrt + eps;
        p = p - step_size * (mi / denom);
        prm[i] = p;
        m[i] = mi;
        v[i] = vi;
    }
}

// ------------------------------------------------------------------------------------------ workspace
struct TWs {
    float *wt, *wd;
    float *z0, *p0, *dz0, *dp0;
    unsigned char* idx;
    struct Blk { float *z1, *h, *z2, *zs, *out, *dz1, *dz2, *dzs, *dh, *dout; } blk[2];
    float* stat[NCONV];
    float *part, *dvec, *mask, *wnll, *dl, *dgap, *slab;
    size_t total;
};

TWs carve(char* base, int B, const TShapes& s) {
    TWs w{};
    Carver ws{base};
    auto f = [&](long long n) { return ws.floats(n); };
    const Layout L = make_layout();
    w.wt = f(L.n_params);
    w.wd = f(L.n_params);
    const long long m0 = (long long)B * s.oh[0] * s.ow[0], mp = (long long)B * s.P1h * s.P1w;
    w.z0 = f(m0 * 32);
    w.dz0 = f(m0 * 32);
    w.p0 = f(mp * 32);
    w.dp0 = f(mp * 32);
    w.idx = reinterpret_cast<unsigned char*>(ws.take(size_t(mp) * 32));
    long long wg_most = 0, part_most = 0;
    for (int k = 0; k < 2; ++k) {
        const int c1 = 1 + 3 * k, C = KGEO[c1][1];
        const long long n = (long long)B * s.oh[c1] * s.ow[c1] * C;
        TWs::Blk& q = w.blk[k];
        q.z1 = f(n); q.h = f(n); q.z2 = f(n); q.zs = f(n); q.out = f(n);
        q.dz1 = f(n); q.dz2 = f(n); q.dzs = f(n); q.dh = f(n); q.dout = f(n);
    }
    for (int i = 0; i < NCONV; ++i) {
        const int C = KGEO[i][1];
        w.stat[i] = f(4 * C);
        const long long M = (long long)B * s.oh[i] * s.ow[i];
        part_most = std::max(part_most, 2LL * bn_nblk(M) * C);
        const WgGeo g = wg_geo(i, M);
        wg_most = std::max(wg_most, (long long)g.S * C * g.kp);
    }
    w.part = f(part_most);
    w.dvec = f((long long)B * HEAD_C);
    w.mask = f((long long)B * HEAD_C);
    w.dgap = f((long long)B * HEAD_C);
    w.wnll = f(2LL * B);
    w.dl = f(2LL * B);
    w.slab = f(wg_most);
    w.total = ws.off;
    return w;
}

constexpr int GRID_CAP = 4096;    // blocks of a grid-stride launch

struct Step {
    const Layout& L;
    const TShapes& s;
    const TWs& w;
    int B;
    const float* prm;
    float* grd;
    float* running;
    long long* nbt;
    float eps, momentum;
    hipStream_t st;

    long long rows(int conv) const { return (long long)B * s.oh[conv] * s.ow[conv]; }

    void conv_fwd(int conv, const float* in, float* z) const {
        const int C = KGEO[conv][0], N = KGEO[conv][1], k = KGEO[conv][2];
        IgArgs a{in, w.wt + L.conv_w[conv], prm + L.conv_b[conv], z, rows(conv), C, N, s.ih[conv], s.iw[conv],
                 s.oh[conv], s.ow[conv], k, k, KGEO[conv][3], KGEO[conv][4], 0};
        const dim3 grid(unsigned((a.M + 127) / 128), 1);   // NT * 32 = N: 2 tiles for 64 channels, 4 for 128
        if (N == 64) hipLaunchKernelGGL((conv_gemm_kernel<2, false>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((conv_gemm_kernel<4, false>), grid, dim3(256), 0, st, a);
    }
    // input gradient of conv `conv` from dz into dx (accumulate: add to what dx holds)
    void conv_dgrad(int conv, const float* dz, float* dx, int accumulate) const {
        const int Cin = KGEO[conv][0], Cout = KGEO[conv][1], k = KGEO[conv][2];
        IgArgs a{dz, w.wd + L.conv_w[conv], nullptr, dx, (long long)B * s.ih[conv] * s.iw[conv], Cout, Cin, s.oh[conv],
                 s.ow[conv], s.ih[conv], s.iw[conv], k, k, KGEO[conv][3], KGEO[conv][4], accumulate};
        const int nt = Cin == 32 ? 1 : 2;   // blockIdx.y: slice of 32 * nt input channels (two slices for 128)
        const dim3 grid(unsigned((a.M + 127) / 128), unsigned(Cin / (32 * nt)));
        if (nt == 1) hipLaunchKernelGGL((conv_gemm_kernel<1, true>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((conv_gemm_kernel<2, true>), grid, dim3(256), 0, st, a);
    }
    void conv_wgrad(int conv, const float* x, const float* dz) const {
        const int Cin = KGEO[conv][0], Cout = KGEO[conv][1], k = KGEO[conv][2];
        const long long M = rows(conv);
        const WgGeo g = wg_geo(conv, M);
        WgArgs a{dz, x, w.slab, M, g.m_per, Cout, Cin, s.ih[conv], s.iw[conv], s.oh[conv], s.ow[conv], k, KGEO[conv][3],
                 KGEO[conv][4], g.kcols, g.kp};
        hipLaunchKernelGGL(wgrad_kernel, dim3(g.S, Cout / 32, g.kp / (32 * WG_NT)), dim3(64), 0, st, a);
        const int n = Cout * (g.kcols + 1);
        hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((n + 255) / 256), dim3(256), 0, st, w.slab, g.S, Cout, g.kp, g.kcols,
                           Cin, k * k, grd + L.conv_w[conv], grd + L.conv_b[conv]);
    }
    void bn_stats(int i, const float* z) const {
        const int C = KGEO[i][1];
        const long long M = rows(i), rp = bn_rows_per(M);
        const int nb = bn_nblk(M);
        hipLaunchKernelGGL(bn_stats_partial_kernel, dim3(nb), dim3(256), 0, st, z, M, C, rp, w.part);
        hipLaunchKernelGGL(bn_stats_seq_merge_kernel, dim3(1), dim3(128), 0, st, w.part, nb, M, rp, C, eps, momentum,
                           running + L.run[i], running + L.run[i] + C, nbt + i, w.stat[i]);
    }
    void bn_backward(int i, const DySrc& src, const float* z, float* dz) const {
        const int C = KGEO[i][1];
        const long long M = rows(i), rp = bn_rows_per(M);
        const int nb = bn_nblk(M);
        hipLaunchKernelGGL(bn_bwd_partial_kernel, dim3(nb), dim3(256), 0, st, src, z, w.stat[i], M, C, rp, w.part);
        hipLaunchKernelGGL(bn_bwd_seq_merge_kernel, dim3(1), dim3(128), 0, st, w.part, nb, C, w.stat[i], grd + L.bn_g[i],
                           grd + L.bn_b[i]);
        hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(grid_for(M * C, GRID_CAP)), dim3(256), 0, st, src, z, w.stat[i],
                           prm + L.bn_g[i], M, C, float(1.0 / double(M)), dz);
    }
};

// The step behind cough_train_forward_backward (d_targets: class indices, d_soft null) and
// cough_train_forward_backward_soft of libcough_amd_soft.so (d_soft: [B][2] class probabilities, d_targets null); fn names
// the entry point in the messages.  The two differ in what the two head kernels read, nowhere else.
int train_step(const char* fn, const float* d_x, int n_clips, int height, int width, const long long* d_targets,
               const float* d_soft, const float* d_class_weights, const float* d_dropout_mask, unsigned long long seed,
               unsigned long long offset, float p, const float* d_params, float* d_grads, float* d_running,
               long long* d_num_batches, float momentum, float eps, float* d_loss, float* d_logits, float* d_mask_out,
               void* d_workspace, size_t workspace_bytes, void* stream) {
    COUGH_REQUIRE(n_clips >= 1 && height >= 1 && width >= 1, COUGH_EINVAL, "%s: bad shape (%d, %d, %d)", fn, n_clips, height,
                  width);
    const TShapes s = make_tshapes(height, width);
    COUGH_REQUIRE(s.P1h >= 1 && s.P1w >= 1, COUGH_EINVAL, "%s: input %dx%d too small for the network", fn, height, width);
    for (int i = 0; i < NCONV; ++i)
        COUGH_REQUIRE((long long)n_clips * s.oh[i] * s.ow[i] > 1, COUGH_EINVAL,
                      "%s: BatchNorm %d sees one value per channel (batch statistics need more)", fn, i);
    const TWs w = carve(static_cast<char*>(d_workspace), n_clips, s);
    const void* d_y = d_soft ? static_cast<const void*>(d_soft) : d_targets;
    if (const int rc = check_step_args(fn, {d_x, d_y, d_params, d_grads, d_running, d_num_batches, d_loss, d_logits,
                                                  d_workspace},
                                       {p}, momentum, eps, d_workspace, workspace_bytes, w.total);
        rc != COUGH_OK)
        return rc;

    const Layout L = make_layout();
    const int B = n_clips;
    hipStream_t st = static_cast<hipStream_t>(stream);
    Step S{L, s, w, B, d_params, d_grads, d_running, d_num_batches, eps, momentum, st};

    // ---- forward
    PrepArgs pa;
    for (int i = 0; i < NCONV; ++i) pa.off[i] = L.conv_w[i];
    hipLaunchKernelGGL(prep_weights_kernel, dim3(64, NCONV), dim3(256), 0, st, d_params, w.wt, w.wd, pa);
    const long long M0 = S.rows(0), MP = (long long)B * s.P1h * s.P1w;
    hipLaunchKernelGGL(stem_fwd_kernel, dim3(unsigned((M0 + 127) / 128)), dim3(256), 0, st, d_x, height, width, s.oh[0],
                       s.ow[0], M0, w.wt + L.conv_w[0], d_params + L.conv_b[0], w.z0);
    S.bn_stats(0, w.z0);
    hipLaunchKernelGGL(stem_bn_pool_kernel, dim3(grid_for(MP * 32, GRID_CAP)), dim3(256), 0, st, w.z0, s.oh[0], s.ow[0], s.P1h,
                       s.P1w, MP * 32, w.stat[0], d_params + L.bn_g[0], d_params + L.bn_b[0], w.p0, w.idx);
    for (int k = 0; k < 2; ++k) {
        const int c1 = 1 + 3 * k, c2 = c1 + 1, sk = c1 + 2, C = KGEO[c1][1];
        const TWs::Blk& q = w.blk[k];
        const float* in = k == 0 ? w.p0 : w.blk[0].out;
        const long long n = S.rows(c1) * C;
        S.conv_fwd(c1, in, q.z1);
        S.bn_stats(c1, q.z1);
        hipLaunchKernelGGL(bn_relu_kernel, dim3(grid_for(n, GRID_CAP)), dim3(256), 0, st, q.z1, n, C, w.stat[c1],
                           d_params + L.bn_g[c1], d_params + L.bn_b[c1], q.h);
        S.conv_fwd(c2, q.h, q.z2);
        S.bn_stats(c2, q.z2);
        S.conv_fwd(sk, in, q.zs);
        S.bn_stats(sk, q.zs);
        hipLaunchKernelGGL(bn_add_relu_kernel, dim3(grid_for(n, GRID_CAP)), dim3(256), 0, st, q.z2, q.zs, n, C, w.stat[c2],
                           d_params + L.bn_g[c2], d_params + L.bn_b[c2], w.stat[sk], d_params + L.bn_g[sk],
                           d_params + L.bn_b[sk], q.out);
    }
    const int HW = s.oh[5] * s.ow[5];
    hipLaunchKernelGGL(head_fwd_kernel, dim3(B), dim3(HEAD_C), 0, st, w.blk[1].out, HW, d_params + L.fc_w, d_params + L.fc_b,
                       d_dropout_mask, seed, offset, p, d_targets, d_soft, d_class_weights, d_logits, w.dvec, w.mask,
                       d_mask_out, w.wnll);

    // ---- backward
    hipLaunchKernelGGL(head_bwd_kernel, dim3(1), dim3(256), 0, st, B, HW, d_logits, d_targets, d_soft, d_class_weights, w.wnll,
                       w.dvec, w.mask, p, d_params + L.fc_w, w.stat[0], d_loss, w.dl, d_grads + L.fc_w, d_grads + L.fc_b, w.dgap);
    for (int k = 1; k >= 0; --k) {
        const int c1 = 1 + 3 * k, c2 = c1 + 1, sk = c1 + 2;
        const TWs::Blk& q = w.blk[k];
        const float* in = k == 0 ? w.p0 : w.blk[0].out;
        float* din = k == 0 ? w.dp0 : w.blk[0].dout;
        DySrc out_src{};
        out_src.act = q.out;
        if (k == 1) { out_src.mode = DY_GAP; out_src.dgap = w.dgap; out_src.HW = HW; }
        else { out_src.mode = DY_MASK; out_src.g = q.dout; }
        S.bn_backward(c2, out_src, q.z2, q.dz2);
        S.bn_backward(sk, out_src, q.zs, q.dzs);
        S.conv_wgrad(c2, q.h, q.dz2);
        S.conv_dgrad(c2, q.dz2, q.dh, 0);
        DySrc h_src{};
        h_src.mode = DY_MASK; h_src.g = q.dh; h_src.act = q.h;
        S.bn_backward(c1, h_src, q.z1, q.dz1);
        S.conv_wgrad(c1, in, q.dz1);
        S.conv_wgrad(sk, in, q.dzs);
        S.conv_dgrad(c1, q.dz1, din, 0);
        S.conv_dgrad(sk, q.dzs, din, 1);
    }
    DySrc pool_src{};
    pool_src.mode = DY_POOL; pool_src.dp = w.dp0; pool_src.p = w.p0; pool_src.idx = w.idx;
    pool_src.OH = s.oh[0]; pool_src.OW = s.ow[0]; pool_src.P1h = s.P1h; pool_src.P1w = s.P1w;
    S.bn_backward(0, pool_src, w.z0, w.dz0);
    S.conv_wgrad(0, d_x, w.dz0);
    COUGH_HIP_CHECK(hipGetLastError());
    return COUGH_OK;
}

}  // namespace
}  // namespace cough

#ifdef COUGH_SOFT_EXPORTS   // the second compilation of this file, for libcough_amd_soft.so: the soft entry point alone
#include "../../include/cough_amd_soft.h"

extern "C" int cough_train_forward_backward_soft(const float* d_x, int n_clips, int height, int width,
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
extern "C" size_t cough_train_workspace_bytes(int n_clips, int height, int width) {
    using namespace cough;
    if (n_clips < 1 || height < 1 || width < 1) return 0;
    const TShapes s = make_tshapes(height, width);
    if (s.P1h < 1 || s.P1w < 1) return 0;
    return carve(nullptr, n_clips, s).total;
}

extern "C" int cough_train_forward_backward(const float* d_x, int n_clips, int height, int width,
                                            const long long* d_targets, const float* d_class_weights,
                                            const float* d_dropout_mask, unsigned long long seed,
                                            unsigned long long offset, float p, const float* d_params, float* d_grads,
                                            float* d_running, long long* d_num_batches, float momentum, float eps,
                                            float* d_loss, float* d_logits, float* d_mask_out, void* d_workspace,
                                            size_t workspace_bytes, void* stream) {
    return cough::train_step(__func__, d_x, n_clips, height, width, d_targets, nullptr, d_class_weights, d_dropout_mask, seed,
                             offset, p, d_params, d_grads, d_running, d_num_batches, momentum, eps, d_loss, d_logits,
                             d_mask_out, d_workspace, workspace_bytes, stream);
}

extern "C" int cough_adamw_step(float* d_params, float* d_grads, float* d_exp_avg, float* d_exp_avg_sq, long long n,
                                float lr, float beta1, float beta2, float eps, float weight_decay, float max_norm,
                                double bias_correction1, double bias_correction2, float* d_total_norm, void* stream) {
    using namespace cough;
    COUGH_REQUIRE(d_params && d_grads && d_exp_avg && d_exp_avg_sq && d_total_norm, COUGH_EINVAL,
                  "cough_adamw_step: NULL argument");
    COUGH_REQUIRE(n >= 1, COUGH_EINVAL, "cough_adamw_step: n must be >= 1");
    COUGH_REQUIRE(finite_f(lr) && lr >= 0.f && finite_f(eps) && eps >= 0.f && finite_f(weight_decay) && weight_decay >= 0.f,
                  COUGH_EINVAL, "cough_adamw_step: bad lr / eps / weight_decay");
    COUGH_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, COUGH_EINVAL,
                  "cough_adamw_step: betas must be in [0, 1)");
    COUGH_REQUIRE(max_norm > 0.f, COUGH_EINVAL, "cough_adamw_step: max_norm must be > 0");
    COUGH_REQUIRE(bias_correction1 > 0.0 && bias_correction1 <= 1.0 && bias_correction2 > 0.0 && bias_correction2 <= 1.0,
                  COUGH_EINVAL, "cough_adamw_step: bias corrections must be in (0, 1]");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(grad_norm_kernel, dim3(1), dim3(NORM_THREADS), 0, st, d_grads, n, d_total_norm);
    const float step_size = float(double(lr) / bias_correction1), bc2_sqrt = float(std::sqrt(bias_correction2));
    hipLaunchKernelGGL(adamw_kernel, dim3(grid_for(n, GRID_CAP)), dim3(256), 0, st, d_params, d_grads, d_exp_avg, d_exp_avg_sq, n,
                       d_total_norm, max_norm, lr, beta1, beta2, eps, weight_decay, step_size, bc2_sqrt);
    COUGH_HIP_CHECK(hipGetLastError());
    return COUGH_OK;
}
#endif
