// What a conv-stack classifier (CoughDetector "standard", CoughDetectorSmall, any _ConvStackNet) packs at create time
// and runs for an (H, W) feature image: layer_forms and plan_cnn alone decide it, in plain host C++17 (no HIP header:
// tests/cnn_plan_dump.cpp builds this file with a host compiler and prints the plans).  cnn.hip packs from layer_forms,
// executes the plan (run_plan) and instantiates the kernels the tables below name.  Every number the decision rests on
// is defined in this file and nowhere else.
#pragma once
#include <cstddef>

#include "resnet_plan.h"   // PLAN_FP32 / PLAN_BF16 / PLAN_BF16X3, HW

namespace cough {
namespace {

constexpr int PLAN_MAX_LAYERS = 16;   // cough_cnn_create accepts 2..16
struct CnnDims { int cin, cout, pool; };   // one block: 3x3 conv (pad 1) cin -> cout, BN, ReLU, 2x2 floor max-pool if pool == 2

// ------------------------------------------------------------------------------------------------ first block, split-bf16
constexpr int CNN_FIRST_MAXL = 22;   // float2 loads per thread: H * W <= 2 * 256 * 22 = 11 264 (the 110 x 101 image fits)
constexpr size_t CNN_FIRST_LDS_LIMIT = 64 * 1024;   // dynamic LDS a kernel gets without hipFuncSetAttribute
struct FirstLds {
    int nrows, pitch;   // bf16 image in LDS with a zero border
    size_t bytes;       // of one plane (cnn_first_x3_kernel stages two: hi, lo)
};
constexpr FirstLds first_lds(int H, int W) {
    const int nrows = H + 3;            // rows -1 .. H + 1 (the row below the last conv row is read with zero weights)
    const int pitch = (W + 7) & ~1;     // cols -1 .. W + 4, even (dword-aligned pairs)
    return {nrows, pitch, size_t(nrows) * pitch * 2};
}

// ------------------------------------------------------------------------------------------------ LDS-image blocks
constexpr int CNN_LDS_UNP = 12;   // single bf16: 16-byte pieces of the LDS image per thread (image <= 48 KB)
// cnn_conv_lds_kernel<CIN, NT, MW, POOL>: the (cin, cout = 32 nt) pairs that have one, 4 waves x MW 32-row tiles
struct LdsCfg { int cin, nt, mw; };
constexpr LdsCfg CNN_LDS_CFG[] = {{16, 1, 4}, {32, 2, 4}, {64, 4, 2}};
constexpr int CNN_LDS_ROWS = int(sizeof(CNN_LDS_CFG) / sizeof(LdsCfg));

// cnn_conv_lds_x3_kernel per input width: NT 32-channel tiles per workgroup, WM x WN waves, MW 32-row tiles per wave,
// PIECES = LDS capacity of the band's two images in 16-byte units, LEAN = the one-tile-ahead fragment pipeline.
// Measured (profiles/r04_cnn_x3_experiments.txt): 4-wave workgroups of 2 x 2 waves with bands small enough for TWO per
// CU (one's staging overlaps the other's MFMA phase) for the 64-channel input and THREE (lean pipeline, <= 168
// registers, bands <= 52 KB) for the 32-channel one; the 128-channel input (one clip = 120 GEMM rows, 86 KB of images:
// one workgroup per CU) as 2 x 4 waves so that all eight waves have rows
struct X3Cfg { int cin, nt, mw, wm, wn, pieces; bool lean; };
constexpr X3Cfg CNN_X3_TABLE[] = {
    {16, 1, 4, 4, 1, 6144, false},
    {32, 2, 5, 2, 2, 3328, true},
    {64, 4, 3, 2, 2, 5056, false},
    {128, 4, 2, 2, 4, 6144, false}};
constexpr int CNN_X3_ROWS = int(sizeof(CNN_X3_TABLE) / sizeof(X3Cfg));
constexpr int x3_threads(X3Cfg c) { return 64 * c.wm * c.wn; }
constexpr int x3_max_lds(X3Cfg c) { return c.pieces * 16 + 64; }   // hipFuncAttributeMaxDynamicSharedMemorySize

constexpr int conv_nt(int cout) { return cout >= 128 ? 4 : cout / 32; }   // 32-channel tiles per wave / workgroup
constexpr int lds_row(int cin, int cout) {      // row of CNN_LDS_CFG, or -1
    for (int r = 0; r < CNN_LDS_ROWS; ++r)
        if (CNN_LDS_CFG[r].cin == cin && 32 * CNN_LDS_CFG[r].nt == cout) return r;
    return -1;
}
constexpr int x3_row_of(int cin) {              // row of CNN_X3_TABLE for an input width, or -1
    for (int r = 0; r < CNN_X3_ROWS; ++r)
        if (CNN_X3_TABLE[r].cin == cin) return r;
    return -1;
}
constexpr int x3_row(int cin, int cout) {       // ... whose tile shape the layer has, or -1
    const int r = x3_row_of(cin);
    return r >= 0 && CNN_X3_TABLE[r].nt == conv_nt(cout) ? r : -1;
}

// ------------------------------------------------------------------------------------------------ what a layer owns
// The weight forms cough_cnn_create packs for layer i and the forward reads.  Every layer has its plain rows: the first
// float [9][cout], the others [cout][ktot] in f32 (fp32, bf16x3) or bf16 (ktot padded to 64 for the LDS-staged GEMM).
// At most one fragment form is set.
struct LayerForms {
    bool bf16_rows;   // plain rows are bf16, else f32
    int ktot;         // row pitch of the plain rows
    bool gemm;        // conv_gemm_bf16_kernel can take the layer
    bool frag_bf16;   // MFMA fragments of cnn_conv_lds_kernel
    bool frag_x3;     // (hi, lo) MFMA fragments of cnn_conv_lds_x3_kernel
    bool first_x3;    // (hi, lo) 16-wide fragment of cnn_first_x3_kernel
};
constexpr LayerForms layer_forms(int dtype, int i, int cin, int cout, int pool) {
    LayerForms f{};
    const bool later = i > 0;
    f.bf16_rows = later && dtype == PLAN_BF16;
    f.gemm = f.bf16_rows && cin % 32 == 0 && cout % 64 == 0;
    f.ktot = f.gemm ? (9 * cin + 63) / 64 * 64 : 9 * cin;
    f.frag_bf16 = f.bf16_rows && lds_row(cin, cout) >= 0;
    f.frag_x3 = later && dtype == PLAN_BF16X3 && x3_row_of(cin) >= 0 && (cout == 32 || cout == 64 || cout % 128 == 0);
    f.first_x3 = !later && dtype == PLAN_BF16X3 && pool == 2 && cout <= 32;
    return f;
}

// ------------------------------------------------------------------------------------------------ bands
// Output rows per workgroup of the split-bf16 LDS-image convolution (0: the layer does not fit, the f32 kernel runs): the
// band's GEMM rows must fit WM waves x MW tiles and its two bf16 images the configuration's LDS capacity
constexpr int x3_band(X3Cfg c, int pool, HW out, int in_w) {
    int band = (c.wm * c.mw * 32) / ((pool == 2 ? 4 : 1) * out.w);
    if (band > out.h) band = out.h;
    while (band >= 1 && size_t((pool == 2 ? 2 : 1) * band + 2) * (in_w + 2) * (c.cin / 4) > size_t(c.pieces)) --band;
    return band;
}
constexpr size_t x3_lds_bytes(X3Cfg c, int pool, int band, int in_w) {   // two images, each rounded to 16 bytes
    return (size_t((pool == 2 ? 2 : 1) * band + 2) * (in_w + 2) * c.cin * 2 + 15) / 16 * 16 * 2;
}
// single bf16: 4 waves x MW tiles x 32 GEMM rows (x4 rows per output when pooled)
constexpr int lds_band(LdsCfg c, int pool, HW out) {
    const int band = (4 * c.mw * 32) / ((pool == 2 ? 4 : 1) * out.w);
    return band > out.h ? out.h : band;
}
constexpr size_t lds_bytes(LdsCfg c, int pool, int band, int in_w) {
    return size_t((pool == 2 ? 2 : 1) * band + 2) * (in_w + 2) * c.cin * 2;
}

// ------------------------------------------------------------------------------------------------ the plan
enum CnnKernel { CNN_FIRST, CNN_FIRST_X3, CNN_CONV_F32, CNN_LDS_X3, CNN_LDS_BF16, CNN_GEMM_BF16, CNN_CONV_BF16 };

struct CnnLayerPlan {
    CnnKernel kernel;
    int row;           // CNN_LDS_X3 / CNN_LDS_BF16: row of the configuration (and instantiation) table
    int nt, mw;        // 32-channel tiles per wave / workgroup (the template argument NT), 32-row tiles per wave
    HW in, out;
    int band;          // LDS-image kernels: output rows per workgroup; 0 under CNN_LDS_BF16: the launch is refused
    int n_bands;       // workgroups per clip
    size_t lds;        // dynamic LDS of the launch
    int gx;            // grid.x per clip: workgroups (CNN_FIRST_X3, the LDS-image kernels), else the threads
                       // (CNN_FIRST) or GEMM rows the launch divides by its tile
    int gy;            // grid.y
    bool fused_mean;   // CNN_LDS_X3, last layer: the epilogue writes the head's channel means instead of the activation
};
struct CnnPlan {
    bool ok;                   // false: the image vanishes inside the network
    int n_layers;
    int unsupported_layer;     // single bf16: first layer whose band does not fit its LDS image (its `in` is the image
                               // of the message), or -1
    FirstLds first;            // CNN_FIRST_X3
    CnnLayerPlan layer[PLAN_MAX_LAYERS];
    int head_hw;               // the tail kernel's HW: 1 when the last layer left channel means
    size_t act_bytes;          // largest activation of one clip
    // one of the two ping-pong buffers for n clips
    constexpr size_t buf_bytes(int n) const { return (size_t(n) * act_bytes + 255) & ~size_t(255); }
};

// Order of a forward: the layers -> the tapped layer's NCHW copy -> tail (if logits are wanted) -> nan_rule_kernel.
// tap_layer: the layer whose activation somebody reads (cough_cnn_conv_output: the last), or -1.
// Single bf16 keeps its asymmetry: a layer that owns frag_bf16 and whose band does not fit is refused, even where the
// GEMM kernel could take it.
constexpr CnnPlan plan_cnn(int dtype, const CnnDims* dims, int n_layers, int H, int W, bool want_logits, int tap_layer) {
    CnnPlan p{};
    p.n_layers = n_layers;
    p.ok = true;
    p.unsupported_layer = -1;
    const size_t esize = dtype == PLAN_BF16 ? 2 : 4;
    HW x{H, W};
    for (int i = 0; i < n_layers; ++i) {
        const CnnDims d = dims[i];
        const LayerForms f = layer_forms(dtype, i, d.cin, d.cout, d.pool);
        CnnLayerPlan& s = p.layer[i];
        s.in = x;
        s.out = x = d.pool == 2 ? HW{x.h / 2, x.w / 2} : x;
        if (x.h < 1 || x.w < 1) {
            p.ok = false;
            return p;
        }
        const size_t act = size_t(x.h) * x.w * d.cout * esize;
        if (act > p.act_bytes) p.act_bytes = act;
        const int rows = x.h * x.w * (d.pool == 2 ? 4 : 1);   // GEMM rows of one clip
        s.row = -1;
        s.gx = rows;
        s.gy = 1;
        if (i == 0) {
            const FirstLds fl = first_lds(H, W);
            if (f.first_x3 && H * W <= 2 * 256 * CNN_FIRST_MAXL && 2 * fl.bytes <= CNN_FIRST_LDS_LIMIT) {
                s.kernel = CNN_FIRST_X3;
                p.first = fl;
                s.lds = 2 * fl.bytes;
                s.gx = 1;
            } else {
                s.kernel = CNN_FIRST;
                s.gx = x.h * x.w;
            }
        } else if (f.frag_bf16) {
            const LdsCfg c = CNN_LDS_CFG[lds_row(d.cin, d.cout)];
            const int band = lds_band(c, d.pool, x);
            s.kernel = CNN_LDS_BF16;
            s.row = lds_row(d.cin, d.cout);
            s.nt = c.nt;
            s.mw = c.mw;
            if (band >= 1 && lds_bytes(c, d.pool, band, s.in.w) <= size_t(CNN_LDS_UNP) * 256 * 16) {
                s.band = band;
                s.gx = s.n_bands = (x.h + band - 1) / band;
                s.lds = lds_bytes(c, d.pool, band, s.in.w);
            } else {
                s.gx = 0;
                if (p.unsupported_layer < 0) p.unsupported_layer = i;
            }
        } else if (f.gemm) {
            s.kernel = CNN_GEMM_BF16;
            s.nt = d.cout % 128 == 0 ? 4 : 2;
            s.gy = d.cout / (32 * s.nt);
        } else {
            const int r = f.frag_x3 ? x3_row(d.cin, d.cout) : -1;
            const int band = r >= 0 ? x3_band(CNN_X3_TABLE[r], d.pool, x, s.in.w) : 0;
            s.nt = conv_nt(d.cout);
            s.gy = d.cout / (32 * s.nt);
            if (band >= 1) {
                s.kernel = CNN_LDS_X3;
                s.row = r;
                s.mw = CNN_X3_TABLE[r].mw;
                s.band = band;
                s.gx = s.n_bands = (x.h + band - 1) / band;
                s.lds = x3_lds_bytes(CNN_X3_TABLE[r], d.pool, band, s.in.w);
                // last block, whole image in one band, logits wanted, nobody taps the activation
                s.fused_mean = i + 1 == n_layers && s.n_bands == 1 && want_logits && tap_layer != i;
            } else {
                s.kernel = dtype == PLAN_BF16 ? CNN_CONV_BF16 : CNN_CONV_F32;
            }
        }
    }
    p.head_hw = p.layer[n_layers - 1].fused_mean ? 1 : x.h * x.w;
    return p;
}

}  // namespace
}  // namespace cough
