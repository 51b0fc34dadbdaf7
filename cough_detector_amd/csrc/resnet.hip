// K2-K5 -- CoughDetectorResidual forward for gfx950 (eval mode).
//
// Replaces /root/reference/src/model.py:253-259 (forward), :285-293 (ResidualBlock.forward),
// :261-265 (predict).  BatchNorm (running stats) is folded into the conv weights at create time;
// Dropout is the identity in eval mode.
//
//   K2 stem   conv7x7 s2 p3 (1->32) + BN + ReLU + maxpool2: implicit GEMM on v_mfma_f32_32x32x2_f32
//             (exact f32; K = 49).  GEMM rows are ordered (pool window, dy, dx) so that the 2x2 max
//             is a max over 4 accumulator registers of one lane -- the 32x45x51 conv output is
//             never materialised.
//   K3/K4     residual blocks as implicit GEMMs over NHWC activations:
//               h   = ReLU(conv3x3 s2 (x) * bn1)                      K = 9*Cin
//               out = ReLU(conv3x3 s1 (h) * bn2 + conv1x1 s2 (x) * bn_skip)   K = 9*Cout + Cin
//             the projection skip is appended to the K loop of conv2, so skip / add / ReLU cost no
//             extra pass.  FP32: v_mfma_f32_32x32x2_f32; BF16: v_mfma_f32_32x32x16_bf16, f32 accumulate.
//   K5 tail   global mean over HxW -> Linear(128,2) -> optional softmax / argmax.
#include <hip/hip_bf16.h>

#include <algorithm>
#include <array>
#include <utility>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include "common.h"
#include "internal.h"
#include "nn_common.h"
#include "conv_gemm.h"
#include "resblock_x3.h"
#include "resnet_plan.h"   // what a forward runs: plan_resnet decides, run_plan (below) launches

namespace cough {
namespace {

// ------------------------------------------------------------------------------------ K2 stem
constexpr int STEM_K = 49, STEM_KS = 25, STEM_N = 32;

template <typename T>
__global__ __launch_bounds__(256) void stem_mfma_kernel(const float* __restrict__ feat, int H, int W, int P1h, int P1w,
                                                        long long n_pool /* B*P1h*P1w */,
                                                        const float* __restrict__ wk /* [50][N] */,
                                                        const float* __restrict__ bias, T* __restrict__ out,
                                                        int N /* output channels, multiple of 32; blockIdx.y = 32-channel tile */) {
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int n0 = blockIdx.y * 32;
    const long long n_tiles = (n_pool + 7) / 8;
    const long long wave_id = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const long long n_waves = (long long)gridDim.x * (blockDim.x >> 6);
    float bw[STEM_KS];
#pragma unroll
    for (int ks = 0; ks < STEM_KS; ++ks) bw[ks] = wk[(2 * ks + h) * N + n0 + r];
    const float bn = bias[n0 + r];
    const int q = r >> 2, dy = (r >> 1) & 1, dx = r & 1;
    const int per_clip = P1h * P1w;
    for (long long tile = wave_id; tile < n_tiles; tile += n_waves) {
        const long long P = tile * 8 + q;
        const bool rowok = P < n_pool;
        const long long Pc = rowok ? P : 0;
        const int b = int(Pc / per_clip), rem = int(Pc - (long long)b * per_clip);
        const int ph = rem / P1w, pw = rem - ph * P1w;
        const int ih0 = 2 * (2 * ph + dy) - 3, iw0 = 2 * (2 * pw + dx) - 3;
        const float* src = feat + (long long)b * H * W;
        f32x16 acc = {0};
#pragma unroll
        for (int ks = 0; ks < STEM_KS; ++ks) {
            const int k0 = 2 * ks, k1 = 2 * ks + 1;                       // compile-time taps of the two halves
            const int kh = h ? (k1 < STEM_K ? k1 / 7 : 0) : k0 / 7;
            const int kw = h ? (k1 < STEM_K ? k1 % 7 : 0) : k0 % 7;
            const int ih = ih0 + kh, iw = iw0 + kw;
            float a = 0.f;
            if (rowok && ih >= 0 && ih < H && iw >= 0 && iw < W) a = src[ih * W + iw];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bw[ks], acc, 0, 0, 0);
        }
        // C layout: col = lane&31 (channel), row = (reg&3) + 8*(reg>>2) + 4*h -> pool window 2*(reg>>2)+h
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const long long Po = tile * 8 + 2 * g + h;
            float v = fmaxf(fmaxf(acc[4 * g], acc[4 * g + 1]), fmaxf(acc[4 * g + 2], acc[4 * g + 3])) + bn;
            v = fmaxf(v, 0.f);
            if (Po < n_pool) out[Po * N + n0 + r] = from_f32<T>(v);
        }
    }
}

// q = a / b for 0 <= a < 2^24 via a float reciprocal plus one correction step (no integer divide)
__device__ __forceinline__ int fdiv(int a, int b, float inv) {
    int q = __float2int_rz(__int2float_rn(a) * inv);
    const int rem = a - q * b;
    q += (rem >= b) ? 1 : 0;
    q -= (rem < 0) ? 1 : 0;
    return q;
}

// bf16 stem: one workgroup per clip.  The feature image is converted to bf16 once and staged in LDS
// with a zero border (rows/cols -3..), so every A fragment is 4 aligned ds_read_b32.  K is re-ordered as
// 8 kernel rows x 8 taps (7 + one zero tap; the 8th row is all zero): MFMA step s, lane half h <-> kernel
// row 2s+h, element jj <-> tap jj, i.e. 8 consecutive input pixels of one image row per lane.
// The image geometry (nrows, pitch: stem_lds) and the pixel limit (STEM_SB_MAXL) are resnet_plan.h's.

// X3: split-bf16 operands -- the image and the weights as hi + lo bf16 pairs, three MFMAs per step
// (image_hi * w_hi + image_lo * w_hi + image_hi * w_lo, the order of the fused stem in featurize.hip), f32 output.
template <bool X3>
__global__ __launch_bounds__(256) void stem_bf16_kernel(const float* __restrict__ feat, int H, int W, int P1h, int P1w,
                                                        int nrows, int pitch,
                                                        const bf16_t* __restrict__ wfrag /* [X3 ? 2 : 1][4][2][32][8] */,
                                                        const float* __restrict__ bias,
                                                        std::conditional_t<X3, float, bf16_t>* __restrict__ out,
                                                        int* __restrict__ nanflag /* [clips]: 1 = the image holds a NaN (nan_rule_kernel) */) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16_t* img = reinterpret_cast<bf16_t*>(smem);
    constexpr int NP = X3 ? 2 : 1;
    const int plane = nrows * pitch;   // elements of one image (even: pitch is even); the lo image follows the hi one
    auto put = [&](int idx, float v) {
        const bf16_t hi = f2bf(v);
        img[idx] = hi;
        if constexpr (X3) img[plane + idx] = f2bf(v - bf2f(hi));
    };
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const long long clip = blockIdx.x;
    const float* src = feat + clip * (long long)H * W;
    // stage: all of this thread's 8-byte global loads are issued first (the clip is one linear run of
    // H*W floats, 8-byte aligned for every clip when H*W is even), the image is zero-filled meanwhile,
    // then the pairs are converted to bf16 and written to their (row, col) cells
    constexpr int SB_MAXL = STEM_SB_MAXL;            // float2 loads per thread (H*W <= 2*256*SB_MAXL)
    const int npairs = (H * W + 1) / 2;
    const bool even = ((H * W) & 1) == 0;
    float2 pv[SB_MAXL];
#pragma unroll
    for (int u = 0; u < SB_MAXL; ++u) {
        const int p = tid + u * 256;
        pv[u] = make_float2(0.f, 0.f);
        if (p < npairs) {
            if (even) pv[u] = reinterpret_cast<const float2*>(src)[p];
            else { pv[u].x = src[2 * p]; if (2 * p + 1 < H * W) pv[u].y = src[2 * p + 1]; }
        }
    }
    for (int i = tid; i < NP * plane / 8; i += 256) reinterpret_cast<uint4*>(img)[i] = make_uint4(0, 0, 0, 0);
    for (int i = (NP * plane / 8) * 8 + tid; i < NP * plane; i += 256) img[i] = 0;
    int bad = 0;
#pragma unroll
    for (int u = 0; u < SB_MAXL; ++u) bad |= (pv[u].x != pv[u].x || pv[u].y != pv[u].y) ? 1 : 0;
    bad = __syncthreads_or(bad);
    if (tid == 0) nanflag[clip] = bad;
    const float inv_w = 1.0f / float(W);
#pragma unroll
    for (int u = 0; u < SB_MAXL; ++u) {
        const int e = 2 * (tid + u * 256);
        if (e < H * W) {
            const int ih = fdiv(e, W, inv_w), iw = e - ih * W;
            put((ih + 3) * pitch + iw + 3, pv[u].x);
            if (e + 1 < H * W) {
                const int ih1 = iw + 1 < W ? ih : ih + 1, iw1 = iw + 1 < W ? iw + 1 : 0;
                put((ih1 + 3) * pitch + iw1 + 3, pv[u].y);
            }
        }
    }
    bf16x8 bw[NP][4];
#pragma unroll
    for (int pl = 0; pl < NP; ++pl)
#pragma unroll
        for (int st = 0; st < 4; ++st)
            bw[pl][st] = *reinterpret_cast<const bf16x8*>(wfrag + pl * 2048 + ((st * 2 + h) * 32 + r) * 8);
    const float bn = bias[r];
    __syncthreads();

    const int per_clip = P1h * P1w, n_tiles = (per_clip + 7) / 8;
    const int q = r >> 2, dy = (r >> 1) & 1, dx = r & 1;
    auto* o = out + clip * (long long)per_clip * STEM_N;
    for (int tile = wave; tile < n_tiles; tile += 4) {
        int P = tile * 8 + q;
        if (P >= per_clip) P = per_clip - 1;
        const int ph = P / P1w, pw = P - ph * P1w;
        // image row of tap row kh: 2*oh + kh, first column 2*ow (both in padded coordinates)
        const uint32_t* base = reinterpret_cast<const uint32_t*>(img + (2 * (2 * ph + dy) + h) * pitch + 2 * (2 * pw + dx));
        f32x16 acc = {0};
#pragma unroll
        for (int st = 0; st < 4; ++st) {
            const uint32_t* p = base + st * pitch;   // +2 image rows per step = 2*pitch bf16 = pitch dwords
            union { uint32_t u[4]; bf16x8 v; } a;
            a.u[0] = p[0]; a.u[1] = p[1]; a.u[2] = p[2]; a.u[3] = p[3];
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.v, bw[0][st], acc, 0, 0, 0);
            if constexpr (X3) {
                const uint32_t* pl = p + plane / 2;
                union { uint32_t u[4]; bf16x8 v; } al;
                al.u[0] = pl[0]; al.u[1] = pl[1]; al.u[2] = pl[2]; al.u[3] = pl[3];
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al.v, bw[0][st], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.v, bw[1][st], acc, 0, 0, 0);
            }
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int Po = tile * 8 + 2 * g + h;
            float v = fmaxf(fmaxf(acc[4 * g], acc[4 * g + 1]), fmaxf(acc[4 * g + 2], acc[4 * g + 3])) + bn;
            v = fmaxf(v, 0.f);
            if (Po < per_clip) {
                if constexpr (X3) o[Po * STEM_N + r] = v;
                else o[Po * STEM_N + r] = f2bf(v);
            }
        }
    }
}

// ------------------------------------------------------------------------------------ K3/K4 convs
// K chunking of the implicit GEMM (A and B use the same channel <-> k-slot map):
//   f32 : 8 channels per chunk, four v_mfma_f32_32x32x2_f32; k-slot h of step e <-> channel 4h+e
//   bf16: 16 channels per chunk, one v_mfma_f32_32x32x16_bf16; lane half h holds channels 8h..8h+7
template <typename T, int NT>
__global__ __launch_bounds__(256) void conv_mfma_kernel(ConvArgs<T> a) {
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const long long m0 = ((long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 32;
    if (m0 >= a.M) return;
    const long long m = m0 + r;
    const bool rowok = m < a.M;
    const long long mc = rowok ? m : 0;
    const int per = a.OH * a.OW;
    const int b = int(mc / per), rem = int(mc - (long long)b * per), oh = rem / a.OW, ow = rem - oh * a.OW;

    f32x16 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = f32x16{0};

    const int n_base = blockIdx.y * 32 * NT;   // blockIdx.y: slice of 32 * NT output channels (0 for the shipped 64 / 128)
    const T* wrow[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) wrow[nt] = a.wp + (long long)(n_base + nt * 32 + r) * a.Ktot;

    int kbase = 0;
    for (int kh = 0; kh < a.KH; ++kh)
        for (int kw = 0; kw < a.KW; ++kw) {
            const int ih = oh * a.stride - a.pad + kh, iw = ow * a.stride - a.pad + kw;
            const bool ok = rowok && ih >= 0 && ih < a.H && iw >= 0 && iw < a.W;
            const T* ap = a.in + (((long long)b * a.H + (ok ? ih : 0)) * a.W + (ok ? iw : 0)) * a.C;
            if constexpr (sizeof(T) == 4) {
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
            } else {
                for (int c0 = 0; c0 < a.C; c0 += 16) {
                    bf16x8 av = {0};
                    if (ok) av = *reinterpret_cast<const bf16x8*>(ap + c0 + 8 * h);
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        const bf16x8 bv = *reinterpret_cast<const bf16x8*>(wrow[nt] + kbase + c0 + 8 * h);
                        acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, acc[nt], 0, 0, 0);
                    }
                }
            }
            kbase += a.C;
        }
    if (a.C2 > 0) {   // fused 1x1 stride-s projection of the block input (model.py:280-283)
        const T* ap = a.in2 + (((long long)b * a.H2 + oh * a.stride2) * a.W2 + ow * a.stride2) * a.C2;
        if constexpr (sizeof(T) == 4) {
            for (int c0 = 0; c0 < a.C2; c0 += 8) {
                float4 av = make_float4(0.f, 0.f, 0.f, 0.f);
                if (rowok) av = *reinterpret_cast<const float4*>(ap + c0 + 4 * h);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const float4 bv = *reinterpret_cast<const float4*>(wrow[nt] + kbase + c0 + 4 * h);
                    acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, acc[nt], 0, 0, 0);
                    acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, acc[nt], 0, 0, 0);
                    acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, acc[nt], 0, 0, 0);
                    acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, acc[nt], 0, 0, 0);
                }
            }
        } else {
            for (int c0 = 0; c0 < a.C2; c0 += 16) {
                bf16x8 av = {0};
                if (rowok) av = *reinterpret_cast<const bf16x8*>(ap + c0 + 8 * h);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const bf16x8 bv = *reinterpret_cast<const bf16x8*>(wrow[nt] + kbase + c0 + 8 * h);
                    acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, acc[nt], 0, 0, 0);
                }
            }
        }
    }
    // epilogue: + folded bias, ReLU, NHWC store (lane = channel -> 32 consecutive channels per row)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int n = n_base + nt * 32 + r;
        const float bn = a.bias[n];
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const long long mo = m0 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
            if (mo < a.M) a.out[mo * a.N + n] = from_f32<T>(fmaxf(acc[nt][reg] + bn, 0.f));
        }
    }
}

// ---------------------------------------------------------------------------- fused residual block (bf16)
// One workgroup = G clips.  The block input x (NHWC bf16) is staged ONCE in LDS as a zero-bordered image
// (16-byte channel chunks XOR-swizzled by pixel so ds_read_b128 of 16 consecutive pixels is conflict-free);
// conv1 (3x3 s2) runs out of that image, its ReLU'd output h is written back into the same LDS region
// (bordered) and never touches HBM; conv2 (3x3 s1) runs out of h, with the 1x1 stride-2 projection of x
// (its 2*oh,2*ow pixels were copied to a compact LDS buffer up front) appended to its K loop.  Weights
// stream global/L2 -> registers (two 64-wide chunks ahead) -> a two-stage LDS ring shared by all waves.
// GEMM view per workgroup: M = G*OH*OW output pixels (32-row MFMA tiles), N = COUT, K = 9*CIN then
// 9*COUT + CIN.  Wave (mg, ng) owns MW M-tiles x NW N-tiles.

constexpr int WREP = 4;   // replicas of the fragment-packed weights (L2 channel spreading)

struct RbArgs {
    const bf16_t* x;      // [B][XH][XW][CIN]
    int XH, XW, OH, OW, n_clips;
    const bf16_t* wf1;    // conv1 weights as MFMA fragments [KS1][NT][64 lanes][8]: lane (r,h) of (k-step s, n-tile t)
    const bf16_t* wf2;    //   holds W[n = 32t + r][k = 16s + 8h .. +7]; conv2 K = 9*COUT taps, then the CIN projection
    const float* b1;
    const float* b2;      // conv2 bias + projection bias
    bf16_t* out;          // [B][OH][OW][COUT]
    // optional fused head (block 1 only; fcw == nullptr: none): global mean over OHxOW -> Linear(COUT, 2)
    const float* fcw;     // [2][COUT]
    const float* fcb;     // [2]
    float* logits;        // [B][2]
    float* probs;         // [B][2] or nullptr
    int* preds;           // [B] or nullptr
};

template <int CIN, int COUT, int G, int MW, int WAVES>
struct RbCfg {
    // tiles, threads and the LDS size (rb_lds_bytes) follow from the parameter tuple in resnet_plan.h (RB_CFG)
    static constexpr int NT = COUT / 32, MTMAX = rb_mtmax(RbParams{CIN, COUT, G, MW, WAVES});
    static constexpr int THREADS = rb_threads(RbParams{CIN, COUT, G, MW, WAVES});
    static constexpr int KS1 = 9 * CIN / 16, KS2 = (9 * COUT + CIN) / 16;   // 16-wide MFMA k-steps
};

__device__ __forceinline__ uint2 pack4_bf16(float a, float b, float c, float d) {
    return make_uint2(uint32_t(f2bf(a)) | (uint32_t(f2bf(b)) << 16), uint32_t(f2bf(c)) | (uint32_t(f2bf(d)) << 16));
}

// Fused residual block, v3.  One workgroup = G clips.
//   * x is staged ONCE into a zero-bordered, XOR-swizzled LDS image; h = ReLU(conv1) goes to a second
//     bordered LDS image and never touches HBM; the 1x1 stride-2 projection reads the centre tap of the x image.
//   * Waves free-run: wave (mg, ng) owns MW 32-pixel tiles x one 32-channel tile.  Its weight fragments come
//     straight from global/L2 in fragment order (1 KB coalesced per load) through an 8-deep register ring
//     that runs ahead across the conv1 -> conv2 boundary; activation fragments are read from LDS one k-step
//     ahead.  Only two workgroup barriers exist: after staging and between the two convolutions.
//   * MFMA operands are swapped (weights = A, activations = B): a lane owns one pixel and 4 consecutive
//     channels per register quad, so h and the output are written with 8-byte stores.
// XH_T x XW_T: the block's input size when it is known at compile time (the shipped 90x101 feature image gives
// 22x25 and 11x13); every pixel <-> (clip, row, column) division of the staging and geometry code is then a
// multiply-shift by a constant instead of a ~15-instruction reciprocal division (they were a quarter of the
// kernel's vector instructions).  0: sizes come from RbArgs.
template <int CIN, int COUT, int G, int MW, int WAVES, int XH_T = 0, int XW_T = 0>
__global__ __launch_bounds__(WAVES * 64) void resblock_bf16_kernel(RbArgs a) {
    using Cfg = RbCfg<CIN, COUT, G, MW, WAVES>;
    constexpr bool FIX = XH_T > 0;
    const int XH = FIX ? XH_T : a.XH, XW = FIX ? XW_T : a.XW;
    const int OH = FIX ? (XH_T - 1) / 2 + 1 : a.OH, OW = FIX ? (XW_T - 1) / 2 + 1 : a.OW;
    auto qdiv = [&](int x, int d, float inv) { return FIX ? x / d : fdiv(x, d, inv); };   // d is a constant when FIX
    constexpr int THREADS = Cfg::THREADS, NT = Cfg::NT, KS1 = Cfg::KS1, KS2 = Cfg::KS2, KS = KS1 + KS2;
    constexpr int CHI = CIN / 8, CHO = COUT / 8, K2M = 9 * COUT;
    constexpr int D = 16;  // weight prefetch depth (k-steps)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int XHb = XH + 2, XWb = XW + 2, OHb = OH + 2, OWb = OW + 2;
    const int per = OH * OW, M = G * per;
    bf16_t* ximg = reinterpret_cast<bf16_t*>(smem);
    bf16_t* himg = ximg + size_t(G) * XHb * XWb * CIN;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int ng = wave % NT, mg = wave / NT;
    const int clip0 = blockIdx.x * G;
    RB_STAMP(0);

    // ---- weight fragment stream ------------------------------------------------------------------
    // Every workgroup walks the same weight stream, so the copies are replicated WREP times in memory and
    // neighbouring workgroups of an XCD (blockIdx / 8) read different copies: the reads spread over L2 channels
    // instead of all CUs hitting the same lines at the same moment.
    const int rep = (blockIdx.x >> 3) % WREP;
    const bf16_t* wf1 = a.wf1 + size_t(rep) * KS1 * NT * 512;
    const bf16_t* wf2 = a.wf2 + size_t(rep) * KS2 * NT * 512;
    auto wfrag = [&](int s) -> bf16x8 {
        const bf16_t* p = s < KS1 ? wf1 + (size_t(s) * NT + ng) * 512 : wf2 + (size_t(s - KS1) * NT + ng) * 512;
        return *reinterpret_cast<const bf16x8*>(p + lane * 8);
    };
    bf16x8 bring[D];
#pragma unroll
    for (int i = 0; i < D; ++i) bring[i] = wfrag(i);
    // folded biases of this wave's 32 channels (lane half h: 4 of every 8), fetched now: loaded where they are used,
    // behind the scheduling barriers of the k-loop, each fetch would expose a full global-memory latency
    float4 bias1[4], bias2[4];
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
        bias1[gq] = *reinterpret_cast<const float4*>(a.b1 + ng * 32 + 8 * gq + 4 * h);
        bias2[gq] = *reinterpret_cast<const float4*>(a.b2 + ng * 32 + 8 * gq + 4 * h);
    }
    float fw0 = 0.f, fw1 = 0.f, fb0 = 0.f, fb1 = 0.f;   // fused head (block 1): Linear(128, 2) row pair of channel tid & 127
    if constexpr (COUT == 128) {
        if (a.fcw != nullptr) {
            fw0 = a.fcw[tid & 127]; fw1 = a.fcw[128 + (tid & 127)];
            fb0 = a.fcb[0]; fb1 = a.fcb[1];
        }
    }

    // ---- stage: the x image of the G clips is one linear run of 16-byte pieces: every load is issued first,
    // the borders of both LDS images are zeroed while the data is in flight, then the pieces are scattered to
    // their swizzled interior cells ---------------------------------------------------------------------
    {
        const int npix = XH * XW, total = G * npix * CHI;
        const int valid = (a.n_clips - clip0 < G ? a.n_clips - clip0 : G) * npix * CHI;   // pieces of real clips
        const uint4* src = reinterpret_cast<const uint4*>(a.x + (long long)clip0 * npix * CIN);
        constexpr int UN = 16;   // covers G*XH*XW*CIN/8 <= 16*THREADS pieces (host-checked)
        uint4 v[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int i = tid + u * THREADS;
            v[u] = make_uint4(0, 0, 0, 0);
            if (i < valid) v[u] = src[i];
        }
        const int nb_x = 2 * XWb + 2 * XH, nb_h = 2 * OWb + 2 * OH;
        const float inv_x = 1.0f / float(nb_x), inv_h = 1.0f / float(nb_h);
        for (int i = tid; i < G * nb_x * CHI; i += THREADS) {
            const int j = i & (CHI - 1), bi = i / CHI;
            const int g = qdiv(bi, nb_x, inv_x), bp = bi - g * nb_x;
            int row, col;
            if (bp < XWb) { row = 0; col = bp; }
            else if (bp < 2 * XWb) { row = XHb - 1; col = bp - XWb; }
            else { const int qq = bp - 2 * XWb; row = 1 + (qq >> 1); col = (qq & 1) ? XWb - 1 : 0; }
            *reinterpret_cast<uint4*>(ximg + swz_off<CIN>((g * XHb + row) * XWb + col, j)) = make_uint4(0, 0, 0, 0);
        }
        for (int i = tid; i < G * nb_h * CHO; i += THREADS) {
            const int j = i & (CHO - 1), bi = i / CHO;
            const int g = qdiv(bi, nb_h, inv_h), bp = bi - g * nb_h;
            int row, col;
            if (bp < OWb) { row = 0; col = bp; }
            else if (bp < 2 * OWb) { row = OHb - 1; col = bp - OWb; }
            else { const int qq = bp - 2 * OWb; row = 1 + (qq >> 1); col = (qq & 1) ? OWb - 1 : 0; }
            *reinterpret_cast<uint4*>(himg + swz_off<COUT>((g * OHb + row) * OWb + col, j)) = make_uint4(0, 0, 0, 0);
        }
        const float inv_np = 1.0f / float(npix), inv_xw = 1.0f / float(XW);
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int i = tid + u * THREADS;
            if (i < total) {
                const int j = i & (CHI - 1), pi_all = i / CHI;
                const int g = qdiv(pi_all, npix, inv_np), pi = pi_all - g * npix;
                const int y = qdiv(pi, XW, inv_xw), xx = pi - y * XW;
                *reinterpret_cast<uint4*>(ximg + swz_off<CIN>((g * XHb + y + 1) * XWb + xx + 1, j)) = v[u];
            }
        }
    }

    // ---- per-lane geometry: lane r owns output pixel R of each of its M-tiles ---------------------------
    int pr1[MW][3], pr2[MW][3];
    const float inv_per = 1.0f / float(per), inv_ow = 1.0f / float(OW);
#pragma unroll
    for (int mt = 0; mt < MW; ++mt) {
        const int R = (mg * MW + mt) * 32 + r;
        const int Rc = R < M ? R : M - 1;
        const int g = qdiv(Rc, per, inv_per), rem = Rc - g * per;
        const int oh = qdiv(rem, OW, inv_ow), ow = rem - oh * OW;
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
            pr1[mt][kh] = (g * XHb + 2 * oh + kh) * XWb + 2 * ow;   // x-image pixel of tap (kh, 0)
            pr2[mt][kh] = (g * OHb + oh + kh) * OWb + ow;           // h-image pixel of tap (kh, 0)
        }
    }
    const bool active = (mg * MW) * 32 < M;   // waves whose tiles all lie beyond M only take part in barriers
    RB_STAMP(1);
    __syncthreads();
    RB_STAMP(2);

    constexpr int OPITCH = COUT + 8;   // bf16 elements per LDS row of the output tile
    bf16_t* otile = ximg;              // the epilogue's output tile lies over the (then dead) x image
    // The compute part is instantiated for MW and MW - 1 tiles per wave: a wave whose last tile lies entirely beyond
    // the M valid rows (block 0: 143 rows = 4.5 tiles for 2 x 3) runs the shorter body -- one wave-uniform choice up
    // front instead of a branch around every MFMA (that version doubled the kernel time).
    auto body = [&]<int MWX>() {
        f32x16 acc[MWX];
    #pragma unroll
        for (int mt = 0; mt < MWX; ++mt) acc[mt] = f32x16{0};

        // Activation fragments of k-step s (compile-time at every call site).  The pixel-dependent part of the
        // swizzled LDS address -- base pointer of the tap's pixel and hs = h ^ swizzle(pixel) -- is computed once
        // per (tile, tap) when the first k-step of a tap is fetched; every further k-step of that tap costs one
        // xor and one shift-add per fragment.
        const bf16_t* tbase[MWX];
        int ths[MWX];
        auto afrag1 = [&](auto sc, int mt) -> bf16x8 {
            constexpr int s = decltype(sc)::value;
            constexpr bool conv1 = s < KS1;
            constexpr int kg = conv1 ? s * 16 : (s - KS1) * 16;
            constexpr bool proj = !conv1 && kg >= K2M;
            constexpr int C = (conv1 || proj) ? CIN : COUT, CH = C / 8;
            constexpr int kt = proj ? kg - K2M : kg;                 // k inside this operand
            constexpr int tap = proj ? 4 : kt / C, c16 = (kt % C) / 16, kh = tap / 3, kw = tap % 3;
            if constexpr (c16 == 0) {                                // first k-step of a tap: new pixel
                const int P = ((conv1 || proj) ? pr1[mt][kh] : pr2[mt][kh]) + kw;
                ths[mt] = h ^ int((unsigned(P) / (16 / CH)) & (CH - 1));   // unsigned: a shift, not a signed division
                tbase[mt] = ((conv1 || proj) ? ximg : himg) + P * C;
            }
            return *reinterpret_cast<const bf16x8*>(tbase[mt] + 8 * ((2 * c16) ^ ths[mt]));
        };
        auto afrags = [&](auto sc, bf16x8 (&dst)[MWX]) {
    #pragma unroll
            for (int mt = 0; mt < MWX; ++mt) dst[mt] = afrag1(sc, mt);
        };

        bf16x8 af[2][MWX];
        if (active) afrags(std::integral_constant<int, 0>{}, af[0]);

        auto step = [&]<int s>() {
            if constexpr (s == KS1) {
                RB_STAMP(3);
                // ---- h = ReLU(conv1 + b1) -> interior of the h image (its border was zeroed while staging) ----
                if (active) {
    #pragma unroll
                    for (int mt = 0; mt < MWX; ++mt) {
                        const bool rok = (mg * MW + mt) * 32 + r < M;
                        const int P = pr2[mt][1] + 1;
    #pragma unroll
                        for (int gq = 0; gq < 4; ++gq) {
                            const int n0 = ng * 32 + 8 * gq + 4 * h;
                            const float4 bb = bias1[gq];
                            const uint2 pk = pack4_bf16(fmaxf(acc[mt][4 * gq] + bb.x, 0.f), fmaxf(acc[mt][4 * gq + 1] + bb.y, 0.f),
                                                        fmaxf(acc[mt][4 * gq + 2] + bb.z, 0.f), fmaxf(acc[mt][4 * gq + 3] + bb.w, 0.f));
                            if (rok) *reinterpret_cast<uint2*>(himg + swz_off<COUT>(P, n0 >> 3) + (n0 & 7)) = pk;
                        }
                        acc[mt] = f32x16{0};
                    }
                }
                __syncthreads();
                RB_STAMP(4);
                if (active) afrags(std::integral_constant<int, s>{}, af[s & 1]);
            }
            if (active) {
                // Software pipeline, pinned with scheduling barriers: ahead of MFMA mt of this step sit the address
                // math + ds_read of the NEXT step's fragment mt (and, once per step, the weight load D steps ahead).
                // Each pair issues in the ~24 cycles an MFMA leaves free; left alone, the scheduler sinks every
                // ds_read next to its MFMA (ds_read -> lgkmcnt(0) -> mfma) and each MFMA pays the full LDS latency.
                const bf16x8 bw = bring[s % D];
    #pragma unroll
                for (int mt = 0; mt < MWX; ++mt) {
                    if constexpr (s + 1 < KS && s + 1 != KS1)
                        af[(s + 1) & 1][mt] = afrag1(std::integral_constant<int, s + 1>{}, mt);
                    if constexpr (s + D < KS) {
                        if (mt == 0) bring[s % D] = wfrag(s + D);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bw, af[s & 1][mt], acc[mt], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        };
        [&]<int... Ss>(std::integer_sequence<int, Ss...>) {
            (step.template operator()<Ss>(), ...);
        }(std::make_integer_sequence<int, KS>{});

        RB_STAMP(5);
        // ---- epilogue: out = ReLU(conv2 + projection + b2).  The accumulators go to a bf16 [pixel][COUT] tile in
        // LDS (over the dead x image; rows padded by 16 B), then the workgroup copies the tile -- which is one
        // contiguous run of NHWC output -- to global with 16-byte-per-lane coalesced stores. ----------------------
        __syncthreads();                   // every wave is done reading the x / h images
        if (active) {
    #pragma unroll
            for (int mt = 0; mt < MWX; ++mt) {
                const int R = (mg * MW + mt) * 32 + r;
    #pragma unroll
                for (int gq = 0; gq < 4; ++gq) {
                    const int n0 = ng * 32 + 8 * gq + 4 * h;
                    const float4 bb = bias2[gq];
                    const uint2 pk = pack4_bf16(fmaxf(acc[mt][4 * gq] + bb.x, 0.f), fmaxf(acc[mt][4 * gq + 1] + bb.y, 0.f),
                                                fmaxf(acc[mt][4 * gq + 2] + bb.z, 0.f), fmaxf(acc[mt][4 * gq + 3] + bb.w, 0.f));
                    *reinterpret_cast<uint2*>(otile + R * OPITCH + n0) = pk;
                }
            }
        }
    };
    if (MW > 1 && M - mg * MW * 32 <= (MW - 1) * 32) body.template operator()<(MW > 1 ? MW - 1 : 1)>();
    else body.template operator()<MW>();
    __syncthreads();
    if (a.out != nullptr) {   // nullptr: the block output is only consumed by the fused head (pipeline: no parity tap)
        const int mvalid = (a.n_clips - clip0 < G ? a.n_clips - clip0 : G) * per;
        uint4* o = reinterpret_cast<uint4*>(a.out + (long long)clip0 * per * COUT);
        for (int p = tid; p < mvalid * CHO; p += THREADS) {
            const int row = p / CHO, ch = p - row * CHO;
            o[p] = *reinterpret_cast<const uint4*>(otile + row * OPITCH + ch * 8);
        }
    }
    if constexpr (COUT == 128 && THREADS % 128 == 0) {
        // ---- fused head (model.py:242-247, :257-265): the block output tile is still in LDS, so the global
        // mean, Linear(128, 2), softmax and argmax of the workgroup's clips finish here (same summation order
        // as tail_kernel: pixels in order, then lanes of a wave, then the two waves of a clip) ------------
        if (a.fcw != nullptr) {
            float* hred = reinterpret_cast<float*>(otile + Cfg::MTMAX * 32 * OPITCH);   // [THREADS/64][2]
            const int c = tid & 127;
            for (int g0 = 0; g0 < G; g0 += THREADS / 128) {   // one pass when THREADS/128 >= G
                const int g = g0 + (tid >> 7);
                float l0 = 0.f, l1 = 0.f;
                if (g < G) {
                    float sum = 0.f;
#pragma unroll 6
                    for (int i = 0; i < per; ++i) sum += bf2f(otile[(g * per + i) * OPITCH + c]);
                    const float mean = sum / float(per);
                    l0 = wave_sum(mean * fw0);
                    l1 = wave_sum(mean * fw1);
                }
                __syncthreads();
                if (lane == 0) { hred[wave * 2] = l0; hred[wave * 2 + 1] = l1; }
                __syncthreads();
                if (g < G && c == 0 && clip0 + g < a.n_clips) {
                    const int w0 = (tid >> 7) * 2;   // the clip's two waves
                    l0 = hred[w0 * 2] + hred[(w0 + 1) * 2] + fb0;
                    l1 = hred[w0 * 2 + 1] + hred[(w0 + 1) * 2 + 1] + fb1;
                    const long long b = clip0 + g;
                    a.logits[b * 2] = l0;
                    a.logits[b * 2 + 1] = l1;
                    if (a.probs) {
                        const float mx = fmaxf(l0, l1), e0 = expf(l0 - mx), e1 = expf(l1 - mx), inv = 1.0f / (e0 + e1);
                        a.probs[b * 2] = e0 * inv;
                        a.probs[b * 2 + 1] = e1 * inv;
                    }
                    if (a.preds) a.preds[b] = (l1 > l0) ? 1 : 0;
                }
            }
        }
    }
    RB_STAMP(6);
}

// ------------------------------------------------------------------------------------ K5 tail
template <typename T>
__global__ __launch_bounds__(128) void tail_kernel(const T* __restrict__ a3, int HW, const float* __restrict__ fcw,
                                                   const float* __restrict__ fcb, float* __restrict__ logits,
                                                   float* __restrict__ probs, int* __restrict__ preds) {
    __shared__ float red[2][2];
    const int c = threadIdx.x;   // 128 channels
    const long long b = blockIdx.x;
    const T* p = a3 + b * (long long)HW * 128 + c;
    float s = 0.f;
    for (int i = 0; i < HW; ++i) s += to_f32<T>(p[(long long)i * 128]);
    const float mean = s / float(HW);
    float l0 = wave_sum(mean * fcw[c]), l1 = wave_sum(mean * fcw[128 + c]);
    if ((c & 63) == 0) { red[c >> 6][0] = l0; red[c >> 6][1] = l1; }
    __syncthreads();
    if (c == 0) {
        l0 = red[0][0] + red[1][0] + fcb[0];
        l1 = red[0][1] + red[1][1] + fcb[1];
        logits[b * 2] = l0;
        logits[b * 2 + 1] = l1;
        if (probs) {
            const float mx = fmaxf(l0, l1), e0 = expf(l0 - mx), e1 = expf(l1 - mx), inv = 1.0f / (e0 + e1);
            probs[b * 2] = e0 * inv;
            probs[b * 2 + 1] = e1 * inv;
        }
        if (preds) preds[b] = (l1 > l0) ? 1 : 0;   // argmax returns the first maximal index on ties
    }
}

// Head for any channel count (CoughDetectorResidual(channels=...) other than the shipped tuple): C real channels at
// stride Cp (channels are padded to a multiple of 32 in memory), one workgroup per clip.
__global__ __launch_bounds__(128) void tail_generic_kernel(const float* __restrict__ a, int HW, int C, int Cp,
                                                           const float* __restrict__ fcw /* [2][C] */,
                                                           const float* __restrict__ fcb, float* __restrict__ logits,
                                                           float* __restrict__ probs, int* __restrict__ preds) {
    __shared__ float red[2][2];
    const long long b = blockIdx.x;
    const float* p = a + b * (long long)HW * Cp;
    float l0 = 0.f, l1 = 0.f;
    for (int c = threadIdx.x; c < C; c += 128) {
        float s = 0.f;
        for (int i = 0; i < HW; ++i) s += p[(long long)i * Cp + c];
        const float mean = s / float(HW);
        l0 += mean * fcw[c];
        l1 += mean * fcw[C + c];
    }
    l0 = wave_sum(l0);
    l1 = wave_sum(l1);
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = l0; red[threadIdx.x >> 6][1] = l1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        l0 = red[0][0] + red[1][0] + fcb[0];
        l1 = red[0][1] + red[1][1] + fcb[1];
        logits[b * 2] = l0;
        logits[b * 2 + 1] = l1;
        if (probs) {
            const float mx = fmaxf(l0, l1), e0 = expf(l0 - mx), e1 = expf(l1 - mx), inv = 1.0f / (e0 + e1);
            probs[b * 2] = e0 * inv;
            probs[b * 2 + 1] = e1 * inv;
        }
        if (preds) preds[b] = (l1 > l0) ? 1 : 0;
    }
}

__global__ void nhwc_padded_to_nchw_kernel(const float* __restrict__ in, float* __restrict__ out, int C, int Cp, int HW,
                                           long long total) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int hw = int(idx % HW);
    const long long t = idx / HW;
    const int c = int(t % C);
    const long long b = t / C;
    out[idx] = in[(b * HW + hw) * Cp + c];
}

// (n, C, H, W) f32 -> NHWC with the channel count padded to Cp (zeros), the layout of the exact-f32 conv kernels
__global__ void nchw_to_nhwc_padded_kernel(const float* __restrict__ in, float* __restrict__ out, int C, int Cp, int HW,
                                           long long total /* n * HW * Cp */) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int c = int(idx % Cp);
    const long long t = idx / Cp;
    const int hw = int(t % HW);
    const long long b = t / HW;
    out[idx] = c < C ? in[(b * C + c) * HW + hw] : 0.f;
}

template <typename T>
__global__ void nhwc_to_nchw_f32_kernel(const T* __restrict__ in, float* __restrict__ out, int C, int HW, long long total) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int hw = int(idx % HW);
    const long long t = idx / HW;
    const int c = int(t % C);
    const long long b = t / C;
    out[idx] = to_f32<T>(in[(b * HW + hw) * C + c]);
}

// ------------------------------------------------------------------------------------ host side
struct FoldedConv {
    std::vector<float> w;   // [N][K] with k = (kh*KW + kw)*C + c
    std::vector<float> b;   // [N]
    int N, C, KH, KW;
};

FoldedConv fold(const cough_conv_bn& p, int N, int C, int KH, int KW, float eps) {
    FoldedConv f;
    f.N = N; f.C = C; f.KH = KH; f.KW = KW;
    const int K = KH * KW * C;
    f.w.resize(size_t(N) * K);
    f.b.resize(N);
    for (int n = 0; n < N; ++n) {
        const double scale = double(p.bn_w[n]) / std::sqrt(double(p.bn_var[n]) + double(eps));
        f.b[n] = float((double(p.b[n]) - double(p.bn_mean[n])) * scale + double(p.bn_b[n]));
        for (int c = 0; c < C; ++c)
            for (int kh = 0; kh < KH; ++kh)
                for (int kw = 0; kw < KW; ++kw)
                    f.w[size_t(n) * K + (kh * KW + kw) * C + c] =
                        float(double(p.w[((size_t(n) * C + c) * KH + kh) * KW + kw]) * scale);
    }
    return f;
}

size_t align256(size_t v) { return (v + 255) & ~size_t(255); }

}  // namespace
}  // namespace cough

struct cough_resnet {
    int dtype;
    size_t esize;          // activation element size
    float* d_stem_w;       // [50][32]
    cough::bf16_t* d_stem_wfrag;   // bf16 mode: [4 steps][2 halves][32 n][8 taps] MFMA B fragments
    float* d_stem_b;       // [32]
    void* d_w[4];          // packed [N][Ktot]: b0.conv1, b0.conv2+skip, b1.conv1, b1.conv2+skip
    cough::bf16_t* d_wfrag[4];   // bf16 mode: the same weights as MFMA fragments [K/16][N/32][64][8] (fused block kernels)
    cough::bf16_t* d_wx3[2];     // bf16x3 mode: split-bf16 32x32x16 fragments of block i (conv1, projection, conv2; RbxArgs::wf)
    cough::bf16_t* d_wx3t16[2];  //   ... and as 16x16x32 fragments (the heights rbx_t16 picks that body for)
    float* d_b[4];
    int ktot[4];
    float* d_fcw;          // [2][128]
    float* d_fcb;
    struct cough_resnet_generic* gen;   // channels other than (32, 64, 128): exact-f32 kernels over padded channels
};

// CoughDetectorResidual(channels=(c0, ..., cn)) for any tuple (model.py:216-247): channel counts are padded to
// multiples of 32 with zero weights / biases (a padded channel is ReLU(0) = 0 everywhere), the kernels are the f32
// MFMA kernels of the shipped net with the output channels tiled over blockIdx.y.
struct cough_resnet_generic {
    int n_blocks;
    std::vector<int> ch, chp;          // real / padded channels, n_blocks + 1 entries
    float *d_stem_w, *d_stem_b;        // [50][chp0], [chp0]
    std::vector<float*> d_w, d_b;      // per block: conv1 [N][9*Cin], conv2 + skip [N][9*N + Cin] (padded sizes), biases
    std::vector<int> ktot;
    float *d_fcw, *d_fcb;              // [2][c_last], [2]
};

namespace cough {
namespace {

template <typename T>
int upload(void** dst, const std::vector<T>& v) {
    COUGH_HIP_CHECK(hipMalloc(dst, v.size() * sizeof(T)));
    COUGH_HIP_CHECK(hipMemcpy(*dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return COUGH_OK;
}

int upload_x3(cough_resnet* m, int blk, const FoldedConv& c1, const FoldedConv& c2, const FoldedConv& sk) {
    std::vector<bf16_t> wf;
    pack_x3_fragments(wf, c1.w, 9 * c1.C, sk.w, sk.C, c2.w, 9 * c2.C, c1.N);
    if (int e = upload(reinterpret_cast<void**>(&m->d_wx3[blk]), wf)) return e;
    if (!rbx_t16_shape(c1.C, c1.N)) return COUGH_OK;
    pack_x3_t16_fragments(wf, c1.w, 9 * c1.C, sk.w, sk.C, c2.w, 9 * c2.C, c1.N);
    return upload(reinterpret_cast<void**>(&m->d_wx3t16[blk]), wf);
}

int upload_packed(cough_resnet* m, int slot, const FoldedConv& main, const FoldedConv* skip) {
    const int N = main.N, Km = main.KH * main.KW * main.C, Ks = skip ? skip->C : 0;
    const int K = (m->esize == 2) ? ((Km + Ks + 63) / 64) * 64 : Km + Ks;   // bf16 GEMM: zero-padded to 64
    std::vector<float> w(size_t(N) * K, 0.f), b(N);
    for (int n = 0; n < N; ++n) {
        std::memcpy(&w[size_t(n) * K], &main.w[size_t(n) * Km], Km * sizeof(float));
        if (skip) std::memcpy(&w[size_t(n) * K + Km], &skip->w[size_t(n) * Ks], Ks * sizeof(float));
        b[n] = main.b[n] + (skip ? skip->b[n] : 0.f);
    }
    m->ktot[slot] = K;
    if (m->esize == 4) {
        if (int e = upload(&m->d_w[slot], w)) return e;
    } else {
        std::vector<bf16_t> wb(w.size());
        for (size_t i = 0; i < w.size(); ++i) wb[i] = f2bf_host(w[i]);
        if (int e = upload(&m->d_w[slot], wb)) return e;
        // fragment order for the fused block kernels: lane (r, h) of (k-step s, n-tile t) holds W[32t + r][16s + 8h ..+7]
        const int Kr = Km + Ks, ks = Kr / 16, nt = N / 32;
        std::vector<bf16_t> wf(size_t(ks) * nt * 512 * WREP);
        for (int st = 0; st < ks; ++st)
            for (int t = 0; t < nt; ++t)
                for (int lane = 0; lane < 64; ++lane)
                    for (int jj = 0; jj < 8; ++jj)
                        wf[((size_t(st) * nt + t) * 64 + lane) * 8 + jj] =
                            wb[size_t(32 * t + (lane & 31)) * K + 16 * st + 8 * (lane >> 5) + jj];
        for (int rp = 1; rp < WREP; ++rp)
            std::copy(wf.begin(), wf.begin() + size_t(ks) * nt * 512, wf.begin() + size_t(rp) * ks * nt * 512);
        if (int e = upload(reinterpret_cast<void**>(&m->d_wfrag[slot]), wf)) return e;
    }
    return upload(reinterpret_cast<void**>(&m->d_b[slot]), b);
}

struct Workspace {
    char *a1, *h0, *a2, *h1, *a3;
    int* nanflag;
    size_t total;
};
Workspace carve(const cough_resnet* m, char* base, int n, const Shapes& s) {
    Workspace w;
    size_t off = 0;
    w.nanflag = reinterpret_cast<int*>(base);   // one int per clip (nan_rule_kernel)
    off += align256(size_t(n) * sizeof(int));
    auto take = [&](size_t elems) { char* p = base + off; off += align256(elems * m->esize); return p; };
    w.a1 = take(size_t(n) * s.P1h * s.P1w * 32);
    w.h0 = take(size_t(n) * s.B0h * s.B0w * 64);
    w.a2 = take(size_t(n) * s.B0h * s.B0w * 64);
    w.h1 = take(size_t(n) * s.B1h * s.B1w * 128);
    w.a3 = take(size_t(n) * s.B1h * s.B1w * 128);
    w.total = off;
    return w;
}

// ------------------------------------------------------------------------------ generic channel tuples (f32)
// spatial sizes: [0] after the stem + pool, [i + 1] after block i
std::vector<HW> gen_shapes(const cough_resnet_generic* g, int H, int W) {
    std::vector<HW> v{stem_out({H, W})};
    for (int i = 0; i < g->n_blocks; ++i) v.push_back(block_out(v.back()));
    return v;
}
// workspace: a[0] (stem out), then per block h[i] and a[i + 1]; NHWC f32 with padded channels
struct GenWorkspace {
    std::vector<float*> a, h;
    size_t total;
};
GenWorkspace gen_carve(const cough_resnet_generic* g, char* base, int n, const std::vector<HW>& sh) {
    GenWorkspace w;
    size_t off = 0;
    auto take = [&](size_t elems) { float* p = reinterpret_cast<float*>(base + off); off += align256(elems * 4); return p; };
    w.a.push_back(take(size_t(n) * sh[0].h * sh[0].w * g->chp[0]));
    for (int i = 0; i < g->n_blocks; ++i) {
        w.h.push_back(take(size_t(n) * sh[i + 1].h * sh[i + 1].w * g->chp[i + 1]));
        w.a.push_back(take(size_t(n) * sh[i + 1].h * sh[i + 1].w * g->chp[i + 1]));
    }
    w.total = off;
    return w;
}

void gen_destroy(cough_resnet_generic* g) {
    if (!g) return;
    (void)hipFree(g->d_stem_w);
    (void)hipFree(g->d_stem_b);
    for (float* p : g->d_w) (void)hipFree(p);
    for (float* p : g->d_b) (void)hipFree(p);
    (void)hipFree(g->d_fcw);
    (void)hipFree(g->d_fcb);
    delete g;
}

// BN-folded [N][K] weights re-laid for padded channel counts: k = (kh*KW + kw)*Cp + c, zero for padded n / c
void pad_folded(const FoldedConv& f, int Np, int Cp, std::vector<float>& w, int koff, int K, std::vector<float>& b, bool add_bias) {
    for (int n = 0; n < f.N; ++n) {
        for (int t = 0; t < f.KH * f.KW; ++t)
            for (int c = 0; c < f.C; ++c) w[size_t(n) * K + koff + t * Cp + c] = f.w[size_t(n) * f.KH * f.KW * f.C + t * f.C + c];
        b[n] = (add_bias ? b[n] : 0.f) + f.b[n];
    }
    (void)Np;
}

// ------------------------------------------------------------------------------ the instantiation tables
// The split-bf16 block kernels: one per row of RBX_BLOCK0_ROWS / RBX_BLOCK1_ROWS (resnet_plan.h).  A launch takes its
// entry by BlockPlan::row; cough_resnet_create raises the dynamic-LDS limit of every entry.
struct RbxEntry {
    void (*kernel)(RbxArgs);
    int lds, threads;   // RbxCfg::LDS, RbxCfg::THREADS
};
template <int BLK, int XH>
constexpr RbxEntry rbx_entry() {
    constexpr int CIN = NET_CH[BLK], COUT = NET_CH[BLK + 1], G = rbx_clips(BLK, XH), XW = RBX_COLS[BLK];
    using Cfg = RbxCfg<CIN, COUT, G, XH, XW>;
    return {resblock_x3_kernel<CIN, COUT, G, XH, XW>, Cfg::LDS, Cfg::THREADS};
}
template <int BLK, int... I>
constexpr std::array<RbxEntry, sizeof...(I)> rbx_table(std::integer_sequence<int, I...>) {
    return {{rbx_entry<BLK, rbx_rows(BLK, I)>()...}};
}
constexpr auto RBX_TABLE0 = rbx_table<0>(std::make_integer_sequence<int, RBX_NROWS[0]>{});
constexpr auto RBX_TABLE1 = rbx_table<1>(std::make_integer_sequence<int, RBX_NROWS[1]>{});
constexpr const RbxEntry* RBX_TABLE[2] = {RBX_TABLE0.data(), RBX_TABLE1.data()};
// The single-bf16 block kernels of RB_CFG: [block][0: geometry from RbArgs, 1: RB_FIXED compiled in]
template <int BLK, bool FIXED>
constexpr auto rb_kernel() {
    constexpr RbParams P = RB_CFG[BLK];
    return resblock_bf16_kernel<P.cin, P.cout, P.g, P.mw, P.waves, FIXED ? RB_FIXED[BLK].h : 0, FIXED ? RB_FIXED[BLK].w : 0>;
}
constexpr void (*RB_KERNEL[2][2])(RbArgs) = {{rb_kernel<0, false>(), rb_kernel<0, true>()},
                                             {rb_kernel<1, false>(), rb_kernel<1, true>()}};

// ------------------------------------------------------------------------------ running a plan
// One residual block's activations and packed weights: of either net, or of a lone cough_resblock
struct BlockIO {
    const void* x;           // NHWC activations: block input,
    void *h, *out;           //   ReLU(conv1) (the unfused kernels), block output
    int cin, cout;           // channels as laid out in memory (the generic kernels: padded to a multiple of 32)
    const void *w1, *w2;     // packed [cout][k1] conv1, [cout][k2] conv2 followed by the projection
    const float *b1, *b2;    // folded biases: conv1, conv2 + projection
    int k1, k2;
};

// h = ReLU(conv3x3 s(x)), out = ReLU(conv3x3 s1(h) + conv1x1 s(x)) as the two launches of the unfused kernels
template <typename T>
std::pair<ConvArgs<T>, ConvArgs<T>> conv_pair(const BlockIO& k, HW in, HW out, int stride, int n) {
    ConvArgs<T> c1{};
    c1.in = static_cast<const T*>(k.x); c1.H = in.h; c1.W = in.w; c1.C = k.cin;
    c1.KH = 3; c1.KW = 3; c1.stride = stride; c1.pad = 1;
    c1.in2 = nullptr; c1.C2 = 0; c1.H2 = c1.W2 = 0; c1.stride2 = 1;
    c1.wp = static_cast<const T*>(k.w1); c1.bias = k.b1;
    c1.out = static_cast<T*>(k.h); c1.OH = out.h; c1.OW = out.w; c1.N = k.cout; c1.Ktot = k.k1;
    c1.M = (long long)n * out.h * out.w;
    ConvArgs<T> c2{};
    c2.in = static_cast<const T*>(k.h); c2.H = out.h; c2.W = out.w; c2.C = k.cout;
    c2.KH = 3; c2.KW = 3; c2.stride = 1; c2.pad = 1;
    c2.in2 = static_cast<const T*>(k.x); c2.H2 = in.h; c2.W2 = in.w; c2.C2 = k.cin; c2.stride2 = stride;
    c2.wp = static_cast<const T*>(k.w2); c2.bias = k.b2;
    c2.out = static_cast<T*>(k.out); c2.OH = out.h; c2.OW = out.w; c2.N = k.cout; c2.Ktot = k.k2;
    c2.M = c1.M;
    return {c1, c2};
}

// nt: 32-channel tiles per wave (BlockPlan::nt); the f32 kernel tiles the remaining channels over blockIdx.y
template <typename T>
int launch_conv(const ConvArgs<T>& a, int nt, hipStream_t st) {
    if (a.M == 0) return COUGH_OK;
    if constexpr (sizeof(T) == 2) {
        const dim3 grid((unsigned)((a.M + CG_BM - 1) / CG_BM));
        if (nt == 2) hipLaunchKernelGGL((conv_gemm_bf16_kernel<2>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((conv_gemm_bf16_kernel<4>), grid, dim3(256), 0, st, a);
    } else {
        const long long tiles = (a.M + 31) / 32;
        const dim3 grid((unsigned)((tiles + 3) / 4), a.N / (32 * nt));
        if (nt == 1) hipLaunchKernelGGL((conv_mfma_kernel<T, 1>), grid, dim3(256), 0, st, a);
        else if (nt == 2) hipLaunchKernelGGL((conv_mfma_kernel<T, 2>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((conv_mfma_kernel<T, 4>), grid, dim3(256), 0, st, a);
    }
    COUGH_HIP_CHECK(hipGetLastError());
    return COUGH_OK;
}

template <typename T>
int launch_conv_pair(const BlockIO& k, HW in, HW out, int stride, int n, int nt, hipStream_t st) {
    const auto [c1, c2] = conv_pair<T>(k, in, out, stride, n);
    if (int e = launch_conv(c1, nt, st)) return e;
    return launch_conv(c2, nt, st);
}

template <typename T>
void launch_stem_mfma(const float* d_feat, int n, int H, int W, HW p1, const float* wk, const float* bias, void* a1, int channels,
                      hipStream_t st) {
    const long long n_pool = (long long)n * p1.h * p1.w;
    const long long tiles = (n_pool + 7) / 8;
    long long blocks = (tiles + 3) / 4;
    if (blocks > 256 * 8) blocks = 256 * 8;   // grid-stride over tiles: weights stay in registers
    hipLaunchKernelGGL(stem_mfma_kernel<T>, dim3((unsigned)blocks, channels / 32), dim3(256), 0, st, d_feat, H, W, p1.h, p1.w,
                       n_pool, wk, bias, static_cast<T*>(a1), channels);
}

// The buffers (carved from the workspace) and weights a forward of either net reads and writes
struct NetIO {
    const float *stem_w, *stem_b;   // stem_mfma_kernel: [50][stem_ch], [stem_ch]
    int stem_ch;                    // stem channels as laid out
    char* a1;                       // stem + pool output
    int* nanflag;                   // [n] written by the staged stems (or the featurise kernel); nullptr: the generic net
    BlockIO blk[PLAN_MAX_BLOCKS];
    const float *fcw, *fcb;
    int c_last;                     // real channels of the last activation (tail_generic_kernel)
};
NetIO net_io(const cough_resnet* m, char* ws, int n, int H, int W) {
    NetIO io{};
    if (const cough_resnet_generic* g = m->gen) {
        const GenWorkspace w = gen_carve(g, ws, n, gen_shapes(g, H, W));
        io.stem_w = g->d_stem_w; io.stem_b = g->d_stem_b; io.stem_ch = g->chp[0];
        io.a1 = reinterpret_cast<char*>(w.a[0]);
        for (int i = 0; i < g->n_blocks; ++i)
            io.blk[i] = {w.a[i], w.h[i], w.a[i + 1], g->chp[i], g->chp[i + 1], g->d_w[2 * i], g->d_w[2 * i + 1],
                         g->d_b[2 * i], g->d_b[2 * i + 1], g->ktot[2 * i], g->ktot[2 * i + 1]};
        io.fcw = g->d_fcw; io.fcb = g->d_fcb; io.c_last = g->ch[g->n_blocks];
        return io;
    }
    const Workspace w = carve(m, ws, n, make_shapes(H, W));
    char* const act[5] = {w.a1, w.h0, w.a2, w.h1, w.a3};
    io.stem_w = m->d_stem_w; io.stem_b = m->d_stem_b; io.stem_ch = NET_CH[0];
    io.a1 = w.a1;
    io.nanflag = w.nanflag;
    for (int i = 0; i < 2; ++i)
        io.blk[i] = {act[2 * i], act[2 * i + 1], act[2 * i + 2], NET_CH[i], NET_CH[i + 1], m->d_w[2 * i], m->d_w[2 * i + 1],
                     m->d_b[2 * i], m->d_b[2 * i + 1], m->ktot[2 * i], m->ktot[2 * i + 1]};
    io.fcw = m->d_fcw; io.fcb = m->d_fcb; io.c_last = NET_CH[2];
    return io;
}

// stem -> blocks -> tail (unless block 1 ran the head) -> nan_rule_kernel (unless block 1 applied the rule)
int run_plan(const cough_resnet* m, const NetPlan& p, const NetIO& io, const float* d_feat, int n, int H, int W,
             float* d_logits, float* d_probs, int* d_preds, hipStream_t st) {
    // the per-clip flag is set when a staging loop has looked at every pixel (pipeline: every sample)
    const int* nanflag = p.nan == NAN_FLAG ? io.nanflag : nullptr;
    switch (p.stem) {
        case STEM_FEATURIZER: break;   // a1 was produced by the featurise kernel (cough_pipeline_forward), which also left its verdict
        case STEM_BF16:
            hipLaunchKernelGGL(stem_bf16_kernel<false>, dim3(n), dim3(256), p.stem_lds.bytes, st, d_feat, H, W, p.stem_hw.h,
                               p.stem_hw.w, p.stem_lds.nrows, p.stem_lds.pitch, m->d_stem_wfrag, io.stem_b,
                               reinterpret_cast<bf16_t*>(io.a1), io.nanflag);
            break;
        case STEM_X3:
            hipLaunchKernelGGL(stem_bf16_kernel<true>, dim3(n), dim3(256), p.stem_lds.bytes, st, d_feat, H, W, p.stem_hw.h,
                               p.stem_hw.w, p.stem_lds.nrows, p.stem_lds.pitch, m->d_stem_wfrag, io.stem_b,
                               reinterpret_cast<float*>(io.a1), io.nanflag);
            break;
        case STEM_MFMA_F32: launch_stem_mfma<float>(d_feat, n, H, W, p.stem_hw, io.stem_w, io.stem_b, io.a1, io.stem_ch, st); break;
        case STEM_MFMA_BF16: launch_stem_mfma<bf16_t>(d_feat, n, H, W, p.stem_hw, io.stem_w, io.stem_b, io.a1, io.stem_ch, st); break;
    }
    COUGH_HIP_CHECK(hipGetLastError());

    for (int i = 0; i < p.n_blocks; ++i) {
        const BlockPlan& b = p.block[i];
        const BlockIO& k = io.blk[i];
        switch (b.kernel) {
            case BLOCK_X3: {
                RbxArgs ra{};
                ra.x = static_cast<const float*>(k.x);
                ra.n_clips = n;
                ra.wf = b.body == BODY_16X16X32 ? m->d_wx3t16[i] : m->d_wx3[i];
                ra.b1 = k.b1;
                ra.b2 = k.b2;
                ra.out = static_cast<float*>(k.out);
                if (i == 1) {   // block 1 also runs the head
                    ra.fcw = io.fcw; ra.fcb = io.fcb; ra.logits = d_logits; ra.probs = d_probs; ra.preds = d_preds;
                    if (!p.store_a3) ra.out = nullptr;
                    if (p.nan_in_block1) ra.nanflag = nanflag;
                }
                const RbxEntry& e = RBX_TABLE[i][b.row];
                hipLaunchKernelGGL(e.kernel, dim3((n + b.clips - 1) / b.clips), dim3(e.threads), e.lds, st, ra);
                COUGH_HIP_CHECK(hipGetLastError());
                break;
            }
            case BLOCK_BF16_FIXED:
            case BLOCK_BF16_RUNTIME: {
                RbArgs ra{};
                ra.x = static_cast<const bf16_t*>(k.x); ra.XH = b.in.h; ra.XW = b.in.w; ra.OH = b.out.h; ra.OW = b.out.w;
                ra.n_clips = n;
                ra.wf1 = m->d_wfrag[2 * i]; ra.b1 = k.b1;
                ra.wf2 = m->d_wfrag[2 * i + 1]; ra.b2 = k.b2;
                ra.out = static_cast<bf16_t*>(k.out);
                if (i == 1) {
                    ra.fcw = io.fcw; ra.fcb = io.fcb; ra.logits = d_logits; ra.probs = d_probs; ra.preds = d_preds;
                    if (!p.store_a3) ra.out = nullptr;
                }
                hipLaunchKernelGGL(RB_KERNEL[i][b.kernel == BLOCK_BF16_FIXED], dim3((n + b.clips - 1) / b.clips),
                                   dim3(rb_threads(RB_CFG[i])), b.lds, st, ra);
                COUGH_HIP_CHECK(hipGetLastError());
                break;
            }
            case BLOCK_CONV_MFMA:
                if (int e = launch_conv_pair<float>(k, b.in, b.out, 2, n, b.nt, st)) return e;
                break;
            case BLOCK_CONV_GEMM_BF16:
                if (int e = launch_conv_pair<bf16_t>(k, b.in, b.out, 2, n, b.nt, st)) return e;
                break;
        }
    }

    const BlockIO& last = io.blk[p.n_blocks - 1];
    const int HWl = p.block[p.n_blocks - 1].out.h * p.block[p.n_blocks - 1].out.w;
    switch (p.head) {
        case HEAD_FUSED: break;
        case HEAD_TAIL_F32:
            hipLaunchKernelGGL(tail_kernel<float>, dim3(n), dim3(128), 0, st, static_cast<const float*>(last.out), HWl, io.fcw,
                               io.fcb, d_logits, d_probs, d_preds);
            break;
        case HEAD_TAIL_BF16:
            hipLaunchKernelGGL(tail_kernel<bf16_t>, dim3(n), dim3(128), 0, st, static_cast<const bf16_t*>(last.out), HWl, io.fcw,
                               io.fcb, d_logits, d_probs, d_preds);
            break;
        case HEAD_TAIL_GENERIC:
            hipLaunchKernelGGL(tail_generic_kernel, dim3(n), dim3(128), 0, st, static_cast<const float*>(last.out), HWl, io.c_last,
                               last.cout, io.fcw, io.fcb, d_logits, d_probs, d_preds);
            break;
    }
    if (p.head != HEAD_FUSED) COUGH_HIP_CHECK(hipGetLastError());
    if (!p.nan_in_block1) {   // a NaN pixel (pipeline: a non-finite sample) -> NaN logits, as torch's ReLU / max-pool propagate it
        hipLaunchKernelGGL(nan_rule_kernel, dim3(n), dim3(256), 0, st, d_feat, (long long)H * W, nanflag, d_logits, d_probs,
                           d_preds);
        COUGH_HIP_CHECK(hipGetLastError());
    }
    return COUGH_OK;
}

// Carve, then run the plan: the shipped net of every dtype and the generic net.  stem_done: the featurise kernel ran the stem.
int run_net(const cough_resnet* m, const float* d_feat, int n, int H, int W, float* d_logits, float* d_probs, int* d_preds,
            char* ws, hipStream_t st, bool stem_done = false) {
    const NetPlan p = plan_resnet(m->dtype, !m->gen, m->gen ? m->gen->n_blocks : 2, H, W, stem_done);
    return run_plan(m, p, net_io(m, ws, n, H, W), d_feat, n, H, W, d_logits, d_probs, d_preds, st);
}

}  // namespace
}  // namespace cough

#ifdef COUGH_K1_STAMPS
extern "C" __attribute__((visibility("default"))) int cough_debug_set_rb_stamp_buffer(void* d_buf) {
    return hipMemcpyToSymbol(HIP_SYMBOL(cough::g_rb_stamp_buf), &d_buf, sizeof(d_buf)) == hipSuccess ? 0 : 3;
}
#endif

extern "C" int cough_resnet_create(cough_resnet** out, const cough_resnet_weights* w, int dtype) {
    using namespace cough;
    COUGH_REQUIRE(out && w, COUGH_EINVAL, "cough_resnet_create: NULL argument");
    COUGH_REQUIRE(dtype == COUGH_DTYPE_FP32 || dtype == COUGH_DTYPE_BF16 || dtype == COUGH_DTYPE_BF16X3, COUGH_EINVAL,
                  "cough_resnet_create: unknown dtype %d", dtype);
    const cough_conv_bn* all[7] = {&w->stem, &w->block[0].conv1, &w->block[0].conv2, &w->block[0].skip,
                                   &w->block[1].conv1, &w->block[1].conv2, &w->block[1].skip};
    for (const cough_conv_bn* p : all)
        COUGH_REQUIRE(p->w && p->b && p->bn_w && p->bn_b && p->bn_mean && p->bn_var, COUGH_EINVAL,
                      "cough_resnet_create: NULL weight pointer");
    COUGH_REQUIRE(w->fc_w && w->fc_b, COUGH_EINVAL, "cough_resnet_create: NULL fc pointer");

    cough_resnet* m = new cough_resnet();
    std::memset(m, 0, sizeof(*m));
    m->dtype = dtype;
    m->esize = (dtype == COUGH_DTYPE_BF16) ? 2 : 4;
    const float eps = w->bn_eps;

    int err = COUGH_OK;
    {   // stem: [50][32], k = kh*7 + kw, row 49 = 0 (K padded to the MFMA k-step)
        const FoldedConv f = fold(w->stem, 32, 1, 7, 7, eps);
        std::vector<float> wk(size_t(50) * 32, 0.f);
        for (int n = 0; n < 32; ++n)
            for (int k = 0; k < 49; ++k) wk[size_t(k) * 32 + n] = f.w[size_t(n) * 49 + k];
        err = upload(reinterpret_cast<void**>(&m->d_stem_w), wk);
        if (!err) err = upload(reinterpret_cast<void**>(&m->d_stem_b), f.b);
        if (!err && (dtype == COUGH_DTYPE_BF16 || dtype == COUGH_DTYPE_BF16X3)) {
            // B fragments of stem_bf16_kernel: k = 16*st + 8*h + jj <-> (kh = 2*st+h, kw = jj); the lo fragments
            // (bf16 of the rounding residual, used by the split-bf16 stem) follow the hi ones
            std::vector<bf16_t> wf(size_t(2) * 4 * 2 * 32 * 8, 0);
            for (int st = 0; st < 4; ++st)
                for (int hh = 0; hh < 2; ++hh)
                    for (int n = 0; n < 32; ++n)
                        for (int jj = 0; jj < 7; ++jj) {
                            const int kh = 2 * st + hh;
                            if (kh >= 7) continue;
                            const float v = f.w[size_t(n) * 49 + kh * 7 + jj];
                            const size_t idx = ((size_t(st) * 2 + hh) * 32 + n) * 8 + jj;
                            split_bf16_host(v, wf[idx], wf[2048 + idx]);
                        }
            err = upload(reinterpret_cast<void**>(&m->d_stem_wfrag), wf);
        }
    }
    const int cin[2] = {32, 64}, cout[2] = {64, 128};
    for (int i = 0; i < 2 && !err; ++i) {
        const FoldedConv c1 = fold(w->block[i].conv1, cout[i], cin[i], 3, 3, eps);
        const FoldedConv c2 = fold(w->block[i].conv2, cout[i], cout[i], 3, 3, eps);
        const FoldedConv sk = fold(w->block[i].skip, cout[i], cin[i], 1, 1, eps);
        err = upload_packed(m, 2 * i, c1, nullptr);
        if (!err) err = upload_packed(m, 2 * i + 1, c2, &sk);
        if (!err && dtype == COUGH_DTYPE_BF16X3) err = upload_x3(m, i, c1, c2, sk);
    }
    if (!err) {
        std::vector<float> fw(w->fc_w, w->fc_w + 256), fb(w->fc_b, w->fc_b + 2);
        err = upload(reinterpret_cast<void**>(&m->d_fcw), fw);
        if (!err) err = upload(reinterpret_cast<void**>(&m->d_fcb), fb);
    }
    if (!err) {   // the fused block kernels of the mode use more than 64 KB of dynamic LDS
        std::vector<const void*> fused;
        if (dtype == COUGH_DTYPE_BF16)
            for (const auto& blk : RB_KERNEL)
                for (const auto kernel : blk) fused.push_back(reinterpret_cast<const void*>(kernel));
        if (dtype == COUGH_DTYPE_BF16X3)
            for (int i = 0; i < 2; ++i)
                for (int r = 0; r < RBX_NROWS[i]; ++r) fused.push_back(reinterpret_cast<const void*>(RBX_TABLE[i][r].kernel));
        hipError_t e = hipSuccess;
        for (const void* fn : fused)
            if (e == hipSuccess) e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, int(RB_LDS_LIMIT));
        if (e != hipSuccess) {
            set_error("cough_resnet_create: %s", hipGetErrorString(e));
            err = COUGH_EHIP;
        }
    }
    if (err) {
        cough_resnet_destroy(m);
        return err;
    }
    *out = m;
    return COUGH_OK;
}

extern "C" int cough_resnet_create_ex(cough_resnet** out, int n_blocks, const int* channels, const cough_conv_bn* stem,
                                      const cough_resblock_weights* blocks, const float* fc_w, const float* fc_b,
                                      float bn_eps, int dtype) {
    using namespace cough;
    COUGH_REQUIRE(out && channels && stem && blocks && fc_w && fc_b, COUGH_EINVAL, "cough_resnet_create_ex: NULL argument");
    COUGH_REQUIRE(n_blocks >= 1 && n_blocks <= 16, COUGH_EINVAL, "cough_resnet_create_ex: n_blocks must be 1..16");
    COUGH_REQUIRE(dtype == COUGH_DTYPE_FP32 || dtype == COUGH_DTYPE_BF16 || dtype == COUGH_DTYPE_BF16X3, COUGH_EINVAL,
                  "cough_resnet_create_ex: unknown dtype %d", dtype);
    for (int i = 0; i <= n_blocks; ++i)
        COUGH_REQUIRE(channels[i] >= 1 && channels[i] <= 1024, COUGH_EINVAL, "cough_resnet_create_ex: channels[%d] = %d", i, channels[i]);
    cough_resnet* m = new cough_resnet();
    std::memset(m, 0, sizeof(*m));
    m->dtype = COUGH_DTYPE_FP32;   // every dtype runs a non-shipped channel tuple on the exact-f32 kernels
    m->esize = 4;
    cough_resnet_generic* g = new cough_resnet_generic();
    g->n_blocks = n_blocks;
    g->d_stem_w = g->d_stem_b = g->d_fcw = g->d_fcb = nullptr;
    for (int i = 0; i <= n_blocks; ++i) {
        g->ch.push_back(channels[i]);
        g->chp.push_back((channels[i] + 31) / 32 * 32);
    }
    m->gen = g;
    int err = COUGH_OK;
    {
        const FoldedConv f = fold(*stem, g->ch[0], 1, 7, 7, bn_eps);
        const int Np = g->chp[0];
        std::vector<float> wk(size_t(50) * Np, 0.f), b(Np, 0.f);
        for (int n = 0; n < g->ch[0]; ++n) {
            for (int k = 0; k < 49; ++k) wk[size_t(k) * Np + n] = f.w[size_t(n) * 49 + k];
            b[n] = f.b[n];
        }
        err = upload(reinterpret_cast<void**>(&g->d_stem_w), wk);
        if (!err) err = upload(reinterpret_cast<void**>(&g->d_stem_b), b);
    }
    for (int i = 0; i < n_blocks && !err; ++i) {
        const int ci = g->ch[i], co = g->ch[i + 1], cip = g->chp[i], cop = g->chp[i + 1];
        const FoldedConv c1 = fold(blocks[i].conv1, co, ci, 3, 3, bn_eps);
        const FoldedConv c2 = fold(blocks[i].conv2, co, co, 3, 3, bn_eps);
        const FoldedConv sk = fold(blocks[i].skip, co, ci, 1, 1, bn_eps);
        const int K1 = 9 * cip, K2 = 9 * cop + cip;
        std::vector<float> w1(size_t(cop) * K1, 0.f), b1(cop, 0.f), w2(size_t(cop) * K2, 0.f), b2(cop, 0.f);
        pad_folded(c1, cop, cip, w1, 0, K1, b1, false);
        pad_folded(c2, cop, cop, w2, 0, K2, b2, false);
        pad_folded(sk, cop, cip, w2, 9 * cop, K2, b2, true);
        float *dw1 = nullptr, *dw2 = nullptr, *db1 = nullptr, *db2 = nullptr;
        err = upload(reinterpret_cast<void**>(&dw1), w1);
        if (!err) err = upload(reinterpret_cast<void**>(&db1), b1);
        if (!err) err = upload(reinterpret_cast<void**>(&dw2), w2);
        if (!err) err = upload(reinterpret_cast<void**>(&db2), b2);
        g->d_w.push_back(dw1); g->d_w.push_back(dw2);
        g->d_b.push_back(db1); g->d_b.push_back(db2);
        g->ktot.push_back(K1); g->ktot.push_back(K2);
    }
    if (!err) {
        std::vector<float> fw(fc_w, fc_w + 2 * size_t(g->ch[n_blocks])), fb(fc_b, fc_b + 2);
        err = upload(reinterpret_cast<void**>(&g->d_fcw), fw);
        if (!err) err = upload(reinterpret_cast<void**>(&g->d_fcb), fb);
    }
    if (err) {
        cough_resnet_destroy(m);
        return err;
    }
    *out = m;
    return COUGH_OK;
}

extern "C" void cough_resnet_destroy(cough_resnet* m) {
    if (!m) return;
    cough::gen_destroy(m->gen);
    (void)hipFree(m->d_stem_w);
    (void)hipFree(m->d_stem_wfrag);
    (void)hipFree(m->d_stem_b);
    for (int i = 0; i < 4; ++i) {
        (void)hipFree(m->d_wfrag[i]);
        (void)hipFree(m->d_w[i]);
        (void)hipFree(m->d_b[i]);
    }
    (void)hipFree(m->d_wx3[0]);
    (void)hipFree(m->d_wx3[1]);
    (void)hipFree(m->d_wx3t16[0]);
    (void)hipFree(m->d_wx3t16[1]);
    (void)hipFree(m->d_fcw);
    (void)hipFree(m->d_fcb);
    delete m;
}

extern "C" size_t cough_resnet_workspace_bytes(const cough_resnet* m, int n_clips, int height, int width) {
    using namespace cough;
    if (!m || n_clips < 0 || height < 1 || width < 1) return 0;
    if (m->gen) return gen_carve(m->gen, nullptr, n_clips, gen_shapes(m->gen, height, width)).total;
    return carve(m, nullptr, n_clips, make_shapes(height, width)).total;
}

extern "C" int cough_resnet_forward(const cough_resnet* m, const float* d_feat, int n_clips, int height, int width,
                                    float* d_logits, float* d_probs, int* d_preds, void* d_workspace,
                                    size_t workspace_bytes, void* stream) {
    using namespace cough;
    COUGH_REQUIRE(m && d_feat && d_logits && d_workspace, COUGH_EINVAL, "cough_resnet_forward: NULL argument");
    COUGH_REQUIRE(n_clips >= 0 && height >= 1 && width >= 1, COUGH_EINVAL, "cough_resnet_forward: bad shape");
    const Shapes s = make_shapes(height, width);
    if (m->gen) {
        const std::vector<HW> sh = gen_shapes(m->gen, height, width);
        COUGH_REQUIRE(sh.back().h >= 1 && sh.back().w >= 1 && sh[0].h >= 1 && sh[0].w >= 1, COUGH_EINVAL,
                      "cough_resnet_forward: input %dx%d too small for the network", height, width);
    } else
    COUGH_REQUIRE(s.B1h >= 1 && s.B1w >= 1 && s.P1h >= 1 && s.P1w >= 1, COUGH_EINVAL,
                  "cough_resnet_forward: input %dx%d too small for the network", height, width);
    COUGH_REQUIRE((reinterpret_cast<size_t>(d_workspace) & 255) == 0, COUGH_EINVAL,
                  "cough_resnet_forward: workspace must be 256-byte aligned");
    COUGH_REQUIRE(workspace_bytes >= cough_resnet_workspace_bytes(m, n_clips, height, width), COUGH_EWORKSPACE,
                  "cough_resnet_forward: workspace too small");
    if (n_clips == 0) return COUGH_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(d_workspace);
    return run_net(m, d_feat, n_clips, height, width, d_logits, d_probs, d_preds, ws, st);
}

extern "C" int cough_resnet_read_activation(const cough_resnet* m, const void* d_workspace, int n_clips, int height,
                                            int width, int which, float* d_out, void* stream) {
    using namespace cough;
    COUGH_REQUIRE(m && d_workspace && d_out, COUGH_EINVAL, "cough_resnet_read_activation: NULL argument");
    if (m->gen) {
        const cough_resnet_generic* g = m->gen;
        COUGH_REQUIRE(which >= 1 && which <= g->n_blocks + 1, COUGH_EINVAL, "cough_resnet_read_activation: which must be 1..%d",
                      g->n_blocks + 1);
        const std::vector<HW> sh = gen_shapes(g, height, width);
        const GenWorkspace gw = gen_carve(g, const_cast<char*>(static_cast<const char*>(d_workspace)), n_clips, sh);
        const int C = g->ch[which - 1], Cp = g->chp[which - 1], HW = sh[which - 1].h * sh[which - 1].w;
        const long long total = (long long)n_clips * C * HW;
        if (total == 0) return COUGH_OK;
        hipLaunchKernelGGL(nhwc_padded_to_nchw_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                           static_cast<hipStream_t>(stream), gw.a[which - 1], d_out, C, Cp, HW, total);
        COUGH_HIP_CHECK(hipGetLastError());
        return COUGH_OK;
    }
    COUGH_REQUIRE(which >= 1 && which <= 3, COUGH_EINVAL, "cough_resnet_read_activation: which must be 1..3");
    const Shapes s = make_shapes(height, width);
    const Workspace w = carve(m, const_cast<char*>(static_cast<const char*>(d_workspace)), n_clips, s);
    const char* src = which == 1 ? w.a1 : which == 2 ? w.a2 : w.a3;
    const int C = which == 1 ? 32 : which == 2 ? 64 : 128;
    const int HW = which == 1 ? s.P1h * s.P1w : which == 2 ? s.B0h * s.B0w : s.B1h * s.B1w;
    const long long total = (long long)n_clips * C * HW;
    if (total == 0) return COUGH_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((total + 255) / 256));
    if (m->esize == 4)
        hipLaunchKernelGGL(nhwc_to_nchw_f32_kernel<float>, grid, dim3(256), 0, st, reinterpret_cast<const float*>(src),
                           d_out, C, HW, total);
    else
        hipLaunchKernelGGL(nhwc_to_nchw_f32_kernel<bf16_t>, grid, dim3(256), 0, st,
                           reinterpret_cast<const bf16_t*>(src), d_out, C, HW, total);
    COUGH_HIP_CHECK(hipGetLastError());
    return COUGH_OK;
}

// ------------------------------------------------------------------------------------------ fused pipeline
namespace cough {
namespace {
bool can_fuse_stem(const cough_featurizer* f, const cough_resnet* m) {
    const FeatPlan p = plan_featurize(f);
    return !m->gen && (m->dtype == COUGH_DTYPE_BF16X3 ? p.stem_x3 : m->dtype == COUGH_DTYPE_BF16 && p.stem_bf16);
}
}  // namespace
}  // namespace cough

extern "C" size_t cough_pipeline_workspace_bytes(const cough_featurizer* f, const cough_resnet* m, int n_clips) {
    using namespace cough;
    if (!f || !m || n_clips < 0) return 0;
    const int H = featurizer_num_features(f), W = cough_featurizer_num_frames(f);
    size_t b = cough_resnet_workspace_bytes(m, n_clips, H, W);
    if (!can_fuse_stem(f, m)) b += align256(size_t(n_clips) * H * W * sizeof(float));   // feature scratch
    return b + align256(plan_featurize(f, 0, n_clips).workspace);                         // spectral-contrast scratch
}

extern "C" int cough_pipeline_forward(const cough_featurizer* f, const cough_resnet* m, const float* d_wav,
                                      long long wav_stride, int n_clips, int flags, float* d_feat, float* d_logits,
                                      float* d_probs, int* d_preds, void* d_workspace, size_t workspace_bytes,
                                      void* stream, void* ev_featurize_begin, void* ev_featurize_end) {
    using namespace cough;
    COUGH_REQUIRE(f && m && d_wav && d_logits && d_workspace, COUGH_EINVAL, "cough_pipeline_forward: NULL argument");
    COUGH_REQUIRE(n_clips >= 0, COUGH_EINVAL, "cough_pipeline_forward: n_clips < 0");
    COUGH_REQUIRE((reinterpret_cast<size_t>(d_workspace) & 255) == 0, COUGH_EINVAL,
                  "cough_pipeline_forward: workspace must be 256-byte aligned");
    COUGH_REQUIRE(workspace_bytes >= cough_pipeline_workspace_bytes(f, m, n_clips), COUGH_EWORKSPACE,
                  "cough_pipeline_forward: workspace too small");
    if (n_clips == 0) return COUGH_OK;
    const int H = featurizer_num_features(f), W = cough_featurizer_num_frames(f);
    const Shapes s = make_shapes(H, W);
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(d_workspace);
    if (ev_featurize_begin) COUGH_HIP_CHECK(hipEventRecord(static_cast<hipEvent_t>(ev_featurize_begin), st));
    if (can_fuse_stem(f, m)) {
        const Workspace w = carve(m, ws, n_clips, s);
        const StemFuse stem{m->d_stem_wfrag, m->d_stem_b, w.a1, m->dtype == COUGH_DTYPE_BF16X3 ? 1 : 0, w.nanflag};
        if (int e = launch_featurize(f, d_wav, wav_stride, d_feat, n_clips, flags, &stem, st)) return e;
        if (ev_featurize_end) COUGH_HIP_CHECK(hipEventRecord(static_cast<hipEvent_t>(ev_featurize_end), st));
        return run_net(m, nullptr, n_clips, H, W, d_logits, d_probs, d_preds, ws, st, true);
    }
    const size_t net_bytes = cough_resnet_workspace_bytes(m, n_clips, H, W);
    const size_t feat_bytes = align256(size_t(n_clips) * H * W * sizeof(float));
    float* feat = d_feat ? d_feat : reinterpret_cast<float*>(ws + net_bytes);
    if (int e = launch_featurize(f, d_wav, wav_stride, feat, n_clips, flags, nullptr, st, ws + net_bytes + feat_bytes,
                                 plan_featurize(f, 0, n_clips).workspace))
        return e;
    if (ev_featurize_end) COUGH_HIP_CHECK(hipEventRecord(static_cast<hipEvent_t>(ev_featurize_end), st));
    return run_net(m, feat, n_clips, H, W, d_logits, d_probs, d_preds, ws, st);
}

// ------------------------------------------------------------------------------ one ResidualBlock on its own
// ResidualBlock (/root/reference/src/model.py:268-293) as a module of its own: any in / out channel count, stride 1 or
// 2, projection skip (1x1 conv + BN) or -- stride 1 and in == out -- the identity (:280-283).  Exact-f32 MFMA conv
// kernels; the skip is the 1x1 operand appended to conv2's K (an identity matrix for the identity skip: x * 1 + 0s is
// exact in f32).  CoughDetectorResidual never builds the identity form; this entry exists so that the class is a
// drop-in wherever the reference's is used directly.
struct cough_resblock {
    int cin, cout, cinp, coutp, stride;
    float *d_w1, *d_b1, *d_w2, *d_b2;
    int k1, k2;
};

extern "C" int cough_resblock_create(cough_resblock** out, int in_ch, int out_ch, int stride, const cough_conv_bn* conv1,
                                     const cough_conv_bn* conv2, const cough_conv_bn* skip, float bn_eps) {
    using namespace cough;
    COUGH_REQUIRE(out && conv1 && conv2, COUGH_EINVAL, "cough_resblock_create: NULL argument");
    COUGH_REQUIRE(in_ch >= 1 && in_ch <= 1024 && out_ch >= 1 && out_ch <= 1024, COUGH_EINVAL,
                  "cough_resblock_create: channels %d -> %d", in_ch, out_ch);
    COUGH_REQUIRE(stride >= 1 && stride <= 4, COUGH_EINVAL, "cough_resblock_create: stride %d", stride);
    COUGH_REQUIRE(skip || (stride == 1 && in_ch == out_ch), COUGH_EINVAL,
                  "cough_resblock_create: the identity skip needs stride 1 and in_ch == out_ch (model.py:280-283)");
    cough_resblock* m = new cough_resblock();
    std::memset(m, 0, sizeof(*m));
    m->cin = in_ch; m->cout = out_ch; m->stride = stride;
    m->cinp = (in_ch + 31) / 32 * 32;
    m->coutp = (out_ch + 31) / 32 * 32;
    const FoldedConv c1 = fold(*conv1, out_ch, in_ch, 3, 3, bn_eps);
    const FoldedConv c2 = fold(*conv2, out_ch, out_ch, 3, 3, bn_eps);
    m->k1 = 9 * m->cinp;
    m->k2 = 9 * m->coutp + m->cinp;
    std::vector<float> w1(size_t(m->coutp) * m->k1, 0.f), b1(m->coutp, 0.f), w2(size_t(m->coutp) * m->k2, 0.f), b2(m->coutp, 0.f);
    pad_folded(c1, m->coutp, m->cinp, w1, 0, m->k1, b1, false);
    pad_folded(c2, m->coutp, m->coutp, w2, 0, m->k2, b2, false);
    if (skip) {
        const FoldedConv sk = fold(*skip, out_ch, in_ch, 1, 1, bn_eps);
        pad_folded(sk, m->coutp, m->cinp, w2, 9 * m->coutp, m->k2, b2, true);
    } else {
        for (int n = 0; n < out_ch; ++n) w2[size_t(n) * m->k2 + 9 * m->coutp + n] = 1.0f;   // out += x
    }
    int err = upload(reinterpret_cast<void**>(&m->d_w1), w1);
    if (!err) err = upload(reinterpret_cast<void**>(&m->d_b1), b1);
    if (!err) err = upload(reinterpret_cast<void**>(&m->d_w2), w2);
    if (!err) err = upload(reinterpret_cast<void**>(&m->d_b2), b2);
    if (err) {
        cough_resblock_destroy(m);
        return err;
    }
    *out = m;
    return COUGH_OK;
}

extern "C" void cough_resblock_destroy(cough_resblock* m) {
    if (!m) return;
    (void)hipFree(m->d_w1);
    (void)hipFree(m->d_b1);
    (void)hipFree(m->d_w2);
    (void)hipFree(m->d_b2);
    delete m;
}

namespace {
struct RbShapes { int oh, ow; size_t x, h, y, total; };
RbShapes rb_shapes(const cough_resblock* m, int n, int H, int W) {
    RbShapes s;
    s.oh = (H + 2 - 3) / m->stride + 1;
    s.ow = (W + 2 - 3) / m->stride + 1;
    s.x = cough::align256(size_t(n) * H * W * m->cinp * 4);
    s.h = cough::align256(size_t(n) * s.oh * s.ow * m->coutp * 4);
    s.y = s.h;
    s.total = s.x + s.h + s.y;
    return s;
}
}  // namespace

extern "C" size_t cough_resblock_workspace_bytes(const cough_resblock* m, int n, int height, int width) {
    if (!m || n < 0 || height < 1 || width < 1) return 0;
    return rb_shapes(m, n, height, width).total;
}

extern "C" int cough_resblock_out_shape(const cough_resblock* m, int height, int width, int* out_h, int* out_w) {
    COUGH_REQUIRE(m && out_h && out_w && height >= 1 && width >= 1, COUGH_EINVAL, "cough_resblock_out_shape: bad argument");
    const RbShapes s = rb_shapes(m, 0, height, width);
    *out_h = s.oh;
    *out_w = s.ow;
    return COUGH_OK;
}

extern "C" int cough_resblock_forward(const cough_resblock* m, const float* d_x, int n, int height, int width, float* d_y,
                                      void* d_workspace, size_t workspace_bytes, void* stream) {
    using namespace cough;
    COUGH_REQUIRE(m && d_x && d_y && d_workspace, COUGH_EINVAL, "cough_resblock_forward: NULL argument");
    COUGH_REQUIRE(n >= 0 && height >= 1 && width >= 1, COUGH_EINVAL, "cough_resblock_forward: bad shape");
    COUGH_REQUIRE((reinterpret_cast<size_t>(d_workspace) & 255) == 0, COUGH_EINVAL,
                  "cough_resblock_forward: workspace must be 256-byte aligned");
    const RbShapes s = rb_shapes(m, n, height, width);
    COUGH_REQUIRE(workspace_bytes >= s.total, COUGH_EWORKSPACE, "cough_resblock_forward: workspace too small");
    if (n == 0) return COUGH_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(d_workspace);
    float* x = reinterpret_cast<float*>(ws);
    float* h = reinterpret_cast<float*>(ws + s.x);
    float* y = reinterpret_cast<float*>(ws + s.x + s.h);
    {
        const long long total = (long long)n * height * width * m->cinp;
        hipLaunchKernelGGL(nchw_to_nhwc_padded_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, d_x, x, m->cin,
                           m->cinp, height * width, total);
    }
    const BlockIO io{x, h, y, m->cinp, m->coutp, m->d_w1, m->d_w2, m->d_b1, m->d_b2, m->k1, m->k2};
    if (int e = launch_conv_pair<float>(io, {height, width}, {s.oh, s.ow}, m->stride, n, 1, st)) return e;
    {
        const long long total = (long long)n * m->cout * s.oh * s.ow;
        hipLaunchKernelGGL(nhwc_padded_to_nchw_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, y, d_y, m->cout,
                           m->coutp, s.oh * s.ow, total);
    }
    COUGH_HIP_CHECK(hipGetLastError());
    return COUGH_OK;
}
