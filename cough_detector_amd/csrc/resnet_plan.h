// What a CoughDetectorResidual forward runs for an (H, W) feature image: plan_resnet alone decides it, in plain host
// C++17 (no HIP header: tests/resnet_plan_dump.cpp builds this file with a host compiler and prints the plans).
// resnet.hip executes the plan (run_plan) and instantiates the kernels the tables below name; resblock_x3.h takes its
// body choice (rbx_t16) and its LDS layout (rbx_layout) from here.  Every number the decision rests on is defined in this file and nowhere else.
#pragma once
#include <cstddef>

namespace cough {
namespace {

// cough_amd.h: COUGH_DTYPE_*
constexpr int PLAN_FP32 = 0, PLAN_BF16 = 1, PLAN_BF16X3 = 3;

constexpr int NET_CH[3] = {32, 64, 128};   // the shipped channels: stem, block 0, block 1

// ------------------------------------------------------------------------------------------------ shapes
struct HW { int h, w; };
constexpr HW stem_out(HW i) { return {((i.h + 6 - 7) / 2 + 1) / 2, ((i.w + 6 - 7) / 2 + 1) / 2}; }   // conv 7x7 s2 p3, max-pool 2
constexpr HW block_out(HW i) { return {(i.h + 2 - 3) / 2 + 1, (i.w + 2 - 3) / 2 + 1}; }               // conv 3x3 s2 p1

struct Shapes {        // the shipped net
    int H, W;          // feature image
    int P1h, P1w;      // after stem + maxpool
    int B0h, B0w;      // after block 0
    int B1h, B1w;      // after block 1
};
constexpr Shapes make_shapes(int H, int W) {
    const HW p1 = stem_out({H, W}), b0 = block_out(p1), b1 = block_out(b0);
    return {H, W, p1.h, p1.w, b0.h, b0.w, b1.h, b1.w};
}

// ------------------------------------------------------------------------------------------------ stem
constexpr size_t STEM_LDS_LIMIT = 64 * 1024;   // dynamic LDS a kernel gets without hipFuncSetAttribute
constexpr int STEM_SB_MAXL = 22;   // 2 * 256 * 22 = 11 264 pixels: the 110 x 101 image of the reference's default flags fits
struct StemLds {
    int nrows, pitch;   // bf16 image in LDS: row = ih + 3, col = iw + 3, pitch even
    size_t bytes;       // of one plane (the split-bf16 stem stages two)
};
constexpr int plan_max(int a, int b) { return a > b ? a : b; }
constexpr StemLds stem_lds(const Shapes& s) {
    const int nrows = plan_max(4 * s.P1h + 6, s.H + 3), pitch = (plan_max(4 * s.P1w + 6, s.W + 3) + 1) & ~1;
    return {nrows, pitch, size_t(nrows) * pitch * 2};
}

// ------------------------------------------------------------------------------------------------ split-bf16 blocks
// Block-input geometries resblock_x3_kernel is instantiated for (rows x RBX_COLS[block]): every feature image the
// reference's flags produce at 99..102 frames.  Image rows -> block-0 rows -> block-1 rows:
//   63..66 (use_mfcc = False: 64) 16 -> 8 | 67..70 (+ contrast rows) 17 -> 9 | 87..90 (shipped) 22 -> 11 | 91..94 (+ contrast rows) 23 -> 12 |
//   95..98 24 -> 12 | 103..106 (delta-delta on) 26 -> 13 | 107..110 (+ contrast rows: the constructor's defaults) 27 -> 14
constexpr int RBX_BLOCK0_ROWS[] = {16, 17, 22, 23, 24, 26, 27};
constexpr int RBX_BLOCK1_ROWS[] = {8, 9, 11, 12, 13, 14};
constexpr int RBX_COLS[2] = {25, 13};
constexpr int RBX_NROWS[2] = {int(sizeof(RBX_BLOCK0_ROWS) / sizeof(int)), int(sizeof(RBX_BLOCK1_ROWS) / sizeof(int))};
constexpr int rbx_rows(int blk, int i) { return blk == 0 ? RBX_BLOCK0_ROWS[i] : RBX_BLOCK1_ROWS[i]; }
// clips per workgroup of block 1 at the 13x13 / 14x13 inputs: 1 (49-53 KB of LDS, three workgroups per CU; two clips per
// workgroup = 95-102 KB, one workgroup per CU, measured the same: profiles/r04_heights.txt)
constexpr int RBX_G_TALL = 1;
// clips per workgroup of block 1: 2 up to 12 rows, RBX_G_TALL above.  The shipped 11x13 takes 81 440 B of LDS and 220
// VGPRs: two workgroups per CU (12 rows: 89 632 B, one)
constexpr int rbx_block1_clips(int xh) { return xh <= 12 ? 2 : RBX_G_TALL; }
constexpr int rbx_clips(int blk, int xh) { return blk == 0 ? 1 : rbx_block1_clips(xh); }
// index of the instantiation for a block input in its row list (the row of resnet.hip's RBX_TABLE), or -1
constexpr int rbx_row(int blk, int xh, int xw) {
    if (xw != RBX_COLS[blk]) return -1;
    for (int i = 0; i < RBX_NROWS[blk]; ++i)
        if (rbx_rows(blk, i) == xh) return i;
    return -1;
}
constexpr bool rbx_compiled(int blk, int xh, int xw) { return rbx_row(blk, xh, xw) >= 0; }

// Which body a block runs.  The 16x16x32 body needs one or two 16-channel tiles per wave and at most two clips per
// workgroup (block 0: 32 -> 64 channels, one clip; block 1: 64 -> 128 channels, one or two clips).  Block 0 runs it up
// to 26 rows; at 27 rows (110-row images) the 32x32x16 body was faster (same-box kernel trace: 315 against 322 us;
// 26 rows: 312 against 307 us; profiles/r06_block0_t16.txt).  Block 1 runs it at every compiled height: 2-16 % faster
// than the 32x32x16 body at 8-14 rows (profiles/r07_block1_t16.txt).
constexpr bool rbx_t16_shape(int cin, int cout) { return (cin == 32 && cout == 64) || (cin == 64 && cout == 128); }
constexpr bool rbx_t16(int cin, int cout, int xh) {
    return rbx_t16_shape(cin, cout) && (cin == 64 || xh <= 26);
}

// ------------------------------------------------------------------------------------------------ split-bf16 blocks: LDS layout
// Everything resblock_x3_kernel<CIN, COUT, G, XH, XW> knows about where a pixel lives in LDS (RbxCfg takes its values from
// rbx_layout; tests/rbx_layout_check.cpp enumerates the same functions on the host).  A plane (hi or lo) holds CIN / 8
// (x) or COUT / 8 (h) chunk planes of 16-byte cells; the x pixels of a clip are stored parity-split: sub-image (row parity
// a, column parity b) holds pixel (2i + a, 2j + b) at cell base(a, b) + i * OW + j.
//   un-bordered x (every body but the one below): the four sub-images back to back; a tap outside the image is
//     redirected to a zero cell by a per-tap select in the kernel.
//   bordered x (rbx_border_x: the 16x16x32 body of block 0 where the workgroups-per-CU bound leaves room): the zeros lie
//     where the taps outside the image point, so a tap is the tile's base + a compile-time offset and nothing else.  Such
//     a tap leaves through an odd-row or an odd-column sub-image only.  XW is odd, so the odd-column sub-images carry one
//     unused column j = OW - 1: zeroed, it is the right border (kw = 2 at ow = OW - 1) and, rows being contiguous, the
//     left border of the next row (kw = 0 at ow = 0).  Zero runs in front of the sub-images give row -1 and cell -1 of
//     the first row, and OW cells behind the odd-row sub-images give row RO of an odd XH:
//       [even, even][0-2 unused][1][even, odd][OW][odd, even][OW + 1][odd, odd][OW if XH is odd][padding up to 16 NP cells past b11]
//     (the OW + 1 run serves the (odd, even) sub-image's row RO and the (odd, odd) one's row -1 / cell -1; the unused
//     cells keep the staging stores of two neighbouring pixels on different banks, see rbx_layout).  The padding
//     rows of the last 16-pixel tile (R >= M) read whatever lies at their offsets: a pixel is one column of the MFMA's B
//     operand and their accumulators are never stored, but every such cell lies inside the chunk plane.
//   h: pixel R at cell R; zero rows of 16 cells (16x16x32 body) or one zero cell (32x32x16 body) at the end of each chunk plane.
constexpr int RBX_LDS_2WG = 80 * 1024, RBX_LDS_CU = 160 * 1024;   // two workgroups / one workgroup per CU
constexpr int rbx_up(int v, int a) { return (v + a - 1) / a * a; }

struct RbxGeo {
    int cin, cout, g, xh, xw;
    bool t16, border_x;
    int oh, ow, npx, per, m, np;   // output image, pixels of a clip (in / out), of a workgroup, 16-pixel tiles
    int chi, cho, re, ro;          // chunk planes of x / h, even / odd rows of x
    int b01, b10, b11;             // sub-image bases in a chunk plane (cells; b00 = 0)
    int npp, nppc;                 // x cells of one clip in a chunk plane, cells between the starts of two clips
    int zc, cpx, zx, kx;           // zero cells per zero row, bytes of an x chunk plane, byte offsets of the zero row(s)
    int zh, cph;                   // byte offset of an h chunk plane's zero cells, bytes of an h chunk plane
    int xbytes, hbytes, pl, bias, hred, lds;
};

// byte offset of x chunk plane c inside a plane (RbxCfg explains the order at CIN = 64)
constexpr int rbx_xoff(bool t16, int chi, int cpx, int c) {
    if (!t16 || chi == 4) return c * cpx;
    const int s = (c & 1) * 4 + (c >> 1);
    return 256 + s * cpx + (s >= 2 ? 256 : 0) + (s >= 6 ? 256 : 0);
}

constexpr RbxGeo rbx_layout(int cin, int cout, int g, int xh, int xw, bool border_x) {
    RbxGeo L{};
    L.cin = cin; L.cout = cout; L.g = g; L.xh = xh; L.xw = xw;
    L.t16 = rbx_t16(cin, cout, xh);
    L.border_x = border_x;
    L.oh = (xh - 1) / 2 + 1; L.ow = (xw - 1) / 2 + 1;
    L.npx = xh * xw; L.per = L.oh * L.ow; L.m = g * L.per; L.np = (L.m + 15) / 16;
    L.chi = cin / 8; L.cho = cout / 8; L.re = (xh + 1) / 2; L.ro = xh / 2;
    L.zc = L.t16 ? 16 : 1;
    if (border_x) {   // 16x16x32 body, CIN = 32, one clip, odd XW
        // The staging stores 8 bytes per lane, 16 lanes = two raster neighbours x 8 quarter-chunks to a bank group; the
        // four chunk planes of a pixel share their banks, and so do the two pixels unless their cells differ mod 8: cells
        // j and b01 + j (even, odd column), or b01 + j and j + 1.  Unused cells in front of the zero cell keep b01 mod 8
        // off 0 and 1; b11 - b10 is off them at every compiled height (RbxCfg asserts it).
        L.b01 = L.re * L.ow + 1;
        while (L.b01 % 8 < 2) ++L.b01;
        L.b10 = L.b01 + L.re * L.ow + L.ow;
        L.b11 = L.b10 + L.ro * L.ow + L.ow + 1;
        L.npp = L.nppc = L.b11 + 16 * L.np;
        L.cpx = rbx_up(L.npp * 16, 256);
        L.zx = 0; L.kx = 0;
        L.xbytes = L.chi * L.cpx;
    } else {
        L.b01 = L.re * L.ow; L.b10 = 2 * L.re * L.ow; L.b11 = 2 * L.re * L.ow + L.ro * L.ow;
        L.npp = 2 * xh * L.ow;
        // 16x16x32 body with two clips: rounded so that nppc - per is a multiple of 16, and the 16 pixels of a tile that
        // straddles the clips still read 16 distinct residues mod 16
        L.nppc = L.t16 && g > 1 ? L.per + rbx_up(L.npp - L.per, 16) : L.npp;
        L.cpx = !L.t16 ? (g * L.npp + 1) * 16 : L.chi == 4 ? rbx_up(g * L.nppc * 16, 256) : rbx_up(g * L.nppc * 16, 64);
        L.zx = !L.t16 ? g * L.npp * 16 : L.chi == 4 ? 4 * L.cpx : 0;
        L.kx = L.t16 && L.chi == 8 ? rbx_xoff(true, 8, L.cpx, 4) - rbx_xoff(true, 8, L.cpx, 0) : 0;
        L.xbytes = !L.t16 ? L.chi * L.cpx : L.chi == 4 ? 4 * L.cpx + 256 : rbx_xoff(true, 8, L.cpx, 7) + L.cpx;
    }
    L.zh = L.t16 ? rbx_up(L.m * 16, 256) : L.m * 16;
    L.cph = L.zh + L.zc * 16;
    L.hbytes = L.cho * L.cph;
    L.pl = rbx_up(L.xbytes > L.hbytes ? L.xbytes : L.hbytes, 256);   // pitch between the hi and lo planes
    L.bias = 2 * L.pl;                                              // b1[COUT], b2[COUT] f32
    L.hred = L.bias + 2 * cout * 4;                                  // head reduction scratch [4 waves][2] f32
    L.lds = L.hred + 4 * 2 * 4;
    return L;
}

// Bordered x planes for block blk at xh input rows?  Only block 0's 16x16x32 body (one clip, four chunk planes, odd XW);
// and only where the bordered layout stays within the workgroups-per-CU bound the un-bordered one meets: 80 KB for two
// workgroups, else one CU's 160 KB.  Block 0: 16, 17, 22 and 26 rows; 23 and 24 rows (82 464 / 84 512 B bordered) keep the
// selects.  Block 1 (the shipped 11x13 with two clips: 81 440 of 81 920 B) keeps them at every height.
constexpr bool rbx_border_x(int blk, int xh) {
    if (blk != 0 || !rbx_t16(NET_CH[0], NET_CH[1], xh) || RBX_COLS[0] % 2 == 0) return false;
    const int sel = rbx_layout(NET_CH[0], NET_CH[1], 1, xh, RBX_COLS[0], false).lds;
    const int bor = rbx_layout(NET_CH[0], NET_CH[1], 1, xh, RBX_COLS[0], true).lds;
    return bor <= (sel <= RBX_LDS_2WG ? RBX_LDS_2WG : RBX_LDS_CU);
}
constexpr RbxGeo rbx_geo(int cin, int cout, int g, int xh, int xw) {
    const bool bx = cin == NET_CH[0] && cout == NET_CH[1] && g == 1 && xw == RBX_COLS[0] && rbx_border_x(0, xh);
    return rbx_layout(cin, cout, g, xh, xw, bx);
}

// x cell of input pixel (ih, iw) of the clip whose cells start at `clip` in a chunk plane: what the staging writes.  The
// kernel expands the macro in place: through a function call the same arithmetic reaches the optimiser in another form, and
// the staging code of every instantiation comes out differently scheduled (block 1: + 1.7 % vector instructions).
#define RBX_X_CELL(clip, b01, b10, b11, ow, ih, iw) \
    ((clip) + (((ih) & 1) ? (((iw) & 1) ? (b11) : (b10)) : (((iw) & 1) ? (b01) : 0)) + ((ih) >> 1) * (ow) + ((iw) >> 1))
constexpr int rbx_x_cell(int clip, int b01, int b10, int b11, int ow, int ih, int iw) { return RBX_X_CELL(clip, b01, b10, b11, ow, ih, iw); }
// cell offset of conv1 tap (kh, kw) from cell (oh, ow) of sub-image (0, 0): input (2 oh - 1 + kh, 2 ow - 1 + kw) lies in the
// sub-image of parities ((kh + 1) & 1, (kw + 1) & 1) at (oh - [kh == 0], ow - [kw == 0]).  The projection is tap (1, 1).
constexpr int rbx_x_tap(int b01, int b10, int b11, int ow, int kh, int kw) {
    const int a = (kh + 1) & 1, b = (kw + 1) & 1;
    return (a ? (b ? b11 : b10) : (b ? b01 : 0)) - (kh == 0 ? ow : 0) - (kw == 0 ? 1 : 0);
}
// bordered x: the zero cells of a chunk plane, k = 0 .. rbx_x_nzero - 1 (the unused column of the two odd-column
// sub-images, then the four runs)
constexpr int rbx_x_nzero(int re, int ro, int ow) { return re + ro + 1 + ow + ow + 1 + (re > ro ? ow : 0); }
constexpr int rbx_x_zero(int b01, int b10, int b11, int ow, int re, int ro, int k) {
    if (k < re) return b01 + k * ow + ow - 1;
    k -= re;
    if (k < ro) return b11 + k * ow + ow - 1;
    k -= ro;
    if (k < 1) return b01 - 1;
    k -= 1;
    if (k < ow) return b10 - ow + k;
    k -= ow;
    if (k < ow + 1) return b10 + ro * ow + k;
    k -= ow + 1;
    return b11 + ro * ow + k;
}
// h: cell of output pixel R of the workgroup, cell offset of conv2 tap (kh, kw)
constexpr int rbx_h_cell(int R) { return R; }
constexpr int rbx_h_tap(int ow, int kh, int kw) { return (kh - 1) * ow + kw - 1; }

// ------------------------------------------------------------------------------------------------ single-bf16 blocks
constexpr size_t RB_LDS_LIMIT = 160 * 1024;   // one workgroup must fit a CU's LDS (set by hipFuncSetAttribute at create time)
struct RbParams { int cin, cout, g, mw, waves; };   // RbCfg<CIN, COUT, G, MW, WAVES> of resblock_bf16_kernel
constexpr RbParams RB_CFG[2] = {
    {32, 64, 1, 3, 4},     // block 0: 1 clip (66 KB LDS: two workgroups per CU), 4 waves = 2 tile groups x 2 channel tiles
    {64, 128, 3, 2, 8}};   // block 1: 3 clips, 8 waves = 2 pixel-tile pairs x 4 channel tiles (2 waves per SIMD)
// the shipped 90x101 feature image: block inputs 22x25 and 11x13 have an instantiation with compiled-in geometry
constexpr HW RB_FIXED[2] = {{22, 25}, {11, 13}};
static_assert(RB_CFG[0].cin == NET_CH[0] && RB_CFG[0].cout == NET_CH[1] && RB_CFG[1].cin == NET_CH[1] && RB_CFG[1].cout == NET_CH[2],
              "the block kernels' channels are the net's");
constexpr int rb_mtmax(RbParams p) { return p.waves / (p.cout / 32) * p.mw; }   // 32-pixel tiles of one workgroup
constexpr int rb_threads(RbParams p) { return p.waves * 64; }
constexpr size_t rb_lds_bytes(RbParams p, int XH, int XW, int OH, int OW) {
    const size_t images = (size_t(p.g) * (XH + 2) * (XW + 2) * p.cin + size_t(p.g) * (OH + 2) * (OW + 2) * p.cout) * 2;
    // the epilogue re-uses the region as a [MTMAX * 32][COUT + 8] bf16 output tile followed by the head's
    // reduction scratch: for small images that is the larger of the two
    const size_t tile = size_t(rb_mtmax(p)) * 32 * (p.cout + 8) * 2 + size_t(p.waves) * 2 * sizeof(float);
    return images > tile ? images : tile;
}
// the clip group fits one workgroup: its LDS, its pixel tiles, its 16 staging registers per thread
constexpr bool rb_fits(RbParams p, HW x, HW o) {
    return rb_lds_bytes(p, x.h, x.w, o.h, o.w) <= RB_LDS_LIMIT && p.g * o.h * o.w <= rb_mtmax(p) * 32 &&
           p.g * x.h * x.w * (p.cin / 8) <= 16 * rb_threads(p);
}

// ------------------------------------------------------------------------------------------------ the plan
enum StemKernel { STEM_FEATURIZER /* a1 and the per-clip flag were left by the featurise kernel */, STEM_BF16, STEM_X3,
                  STEM_MFMA_F32, STEM_MFMA_BF16 };
enum BlockKernel { BLOCK_X3, BLOCK_BF16_FIXED, BLOCK_BF16_RUNTIME, BLOCK_CONV_MFMA, BLOCK_CONV_GEMM_BF16 };
enum BlockBody { BODY_32X32, BODY_16X16X32 };
enum HeadKernel { HEAD_FUSED /* block 1's epilogue */, HEAD_TAIL_F32, HEAD_TAIL_BF16, HEAD_TAIL_GENERIC };
enum NanSource { NAN_FLAG /* the stem's staging loop looked at every pixel */, NAN_RESCAN /* nan_rule_kernel reads the image */ };

struct BlockPlan {
    BlockKernel kernel;
    BlockBody body;
    int clips;     // per workgroup; 0: the kernel is not clip-grouped
    int nt;        // conv kernels: 32-channel tiles per wave (the template argument NT)
    int row;       // BLOCK_X3: row of the instantiation table
    size_t lds;    // dynamic LDS the plan sizes (single-bf16 blocks); BLOCK_X3 takes its table row's
    HW in, out;
};
constexpr int PLAN_MAX_BLOCKS = 16;   // cough_resnet_create_ex accepts 1..16
struct NetPlan {
    bool ok;                 // false: the image vanishes inside the network
    int n_blocks;
    StemKernel stem;
    StemLds stem_lds;        // STEM_BF16 / STEM_X3 (bytes: the launch's, both planes)
    HW stem_hw;              // stem + pool output
    BlockPlan block[PLAN_MAX_BLOCKS];
    HeadKernel head;
    NanSource nan;
    bool nan_in_block1;      // block 1's fused head applies the rule from the flag; else nan_rule_kernel runs last
    bool store_a3;           // block 1 writes its output to memory (the pipeline's fused block 1 does not: nobody reads it)
};

// Order of a forward: stem -> blocks -> tail (unless HEAD_FUSED) -> nan_rule_kernel (unless nan_in_block1).
// A channel tuple other than (32, 64, 128) runs the exact-f32 kernels over padded channels, whatever the dtype.
constexpr NetPlan plan_resnet(int dtype, bool shipped_channels, int n_blocks, int H, int W, bool stem_done) {
    NetPlan p{};
    p.n_blocks = n_blocks;
    p.stem_hw = stem_out({H, W});
    p.ok = p.stem_hw.h >= 1 && p.stem_hw.w >= 1;
    HW x = p.stem_hw;
    for (int i = 0; i < n_blocks; ++i) {
        BlockPlan& b = p.block[i];
        b.in = x;
        b.out = x = block_out(x);
        p.ok = p.ok && x.h >= 1 && x.w >= 1;
        b.kernel = BLOCK_CONV_MFMA;
        b.body = BODY_32X32;
        b.nt = 1;
        b.row = -1;
    }
    p.store_a3 = true;
    if (!shipped_channels) {
        p.stem = STEM_MFMA_F32;
        p.head = HEAD_TAIL_GENERIC;
        p.nan = NAN_RESCAN;
        return p;
    }
    const Shapes s = make_shapes(H, W);
    const StemLds l = stem_lds(s);
    const bool fits = H * W <= 2 * 256 * STEM_SB_MAXL;
    p.nan = NAN_FLAG;
    if (stem_done) {
        p.stem = STEM_FEATURIZER;
    } else if (dtype == PLAN_BF16 && l.bytes <= STEM_LDS_LIMIT && fits) {
        p.stem = STEM_BF16;
        p.stem_lds = l;
    } else if (dtype == PLAN_BF16X3 && 2 * l.bytes <= STEM_LDS_LIMIT && fits) {
        p.stem = STEM_X3;
        p.stem_lds = {l.nrows, l.pitch, 2 * l.bytes};
    } else {
        p.stem = dtype == PLAN_BF16 ? STEM_MFMA_BF16 : STEM_MFMA_F32;
        p.nan = NAN_RESCAN;
    }
    bool head_done = false;
    for (int i = 0; i < 2; ++i) {
        BlockPlan& b = p.block[i];
        const bool fused_x3 = dtype == PLAN_BF16X3 && rbx_compiled(i, b.in.h, b.in.w);
        const bool fused_bf16 = dtype == PLAN_BF16 && rb_fits(RB_CFG[i], b.in, b.out);
        if (fused_x3) {
            b.kernel = BLOCK_X3;
            b.body = rbx_t16(NET_CH[i], NET_CH[i + 1], b.in.h) ? BODY_16X16X32 : BODY_32X32;
            b.clips = rbx_clips(i, b.in.h);
            b.row = rbx_row(i, b.in.h, b.in.w);
            if (i == 1) p.nan_in_block1 = p.nan == NAN_FLAG;
        } else if (fused_bf16) {
            b.kernel = b.in.h == RB_FIXED[i].h && b.in.w == RB_FIXED[i].w ? BLOCK_BF16_FIXED : BLOCK_BF16_RUNTIME;
            b.clips = RB_CFG[i].g;
            b.lds = rb_lds_bytes(RB_CFG[i], b.in.h, b.in.w, b.out.h, b.out.w);
        } else {
            b.kernel = dtype == PLAN_BF16 ? BLOCK_CONV_GEMM_BF16 : BLOCK_CONV_MFMA;
            b.nt = NET_CH[i + 1] == 64 ? 2 : 4;
        }
        if (i == 1 && (fused_x3 || fused_bf16)) {
            head_done = true;
            p.store_a3 = !stem_done;   // the activation tap, cough_resnet_read_activation, belongs to cough_resnet_forward
        }
    }
    p.head = head_done ? HEAD_FUSED : dtype == PLAN_BF16 ? HEAD_TAIL_BF16 : HEAD_TAIL_F32;
    return p;
}

// ------------------------------------------------------------------------------------------------ names
// the vocabulary of tests/resnet_layer_ref.py (plan_row, stage_path) and of profiles/resnet_layer_precision.txt
constexpr const char* plan_name(StemKernel k) {
    switch (k) {
        case STEM_FEATURIZER: return "featurize_kernel";
        case STEM_BF16: return "stem_bf16<bf16>";
        case STEM_X3: return "stem_bf16<x3>";
        case STEM_MFMA_F32: return "stem_mfma<float>";
        case STEM_MFMA_BF16: return "stem_mfma<bf16>";
    }
    return "?";
}
constexpr const char* plan_name(const BlockPlan& b) {
    switch (b.kernel) {
        case BLOCK_X3: return "resblock_x3";
        case BLOCK_BF16_FIXED: return "resblock_bf16:fixed";
        case BLOCK_BF16_RUNTIME: return "resblock_bf16:runtime";
        case BLOCK_CONV_MFMA: return b.nt == 1 ? "conv_mfma<float,1>" : b.nt == 2 ? "conv_mfma<float,2>" : "conv_mfma<float,4>";
        case BLOCK_CONV_GEMM_BF16: return b.nt == 2 ? "conv_gemm_bf16<2>" : "conv_gemm_bf16<4>";
    }
    return "?";
}
constexpr const char* plan_name(BlockBody b) { return b == BODY_16X16X32 ? "16x16x32" : "32x32"; }
constexpr const char* plan_name(HeadKernel h) {
    switch (h) {
        case HEAD_FUSED: return "fused";
        case HEAD_TAIL_F32: return "tail_kernel<float>";
        case HEAD_TAIL_BF16: return "tail_kernel<bf16>";
        case HEAD_TAIL_GENERIC: return "tail_generic_kernel";
    }
    return "?";
}
constexpr const char* plan_name(NanSource n) { return n == NAN_FLAG ? "flag" : "rescan"; }

}  // namespace
}  // namespace cough
