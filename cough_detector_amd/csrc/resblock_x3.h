// K3/K4, split-bf16 ("bf16x3") -- fused residual block for gfx950 whose logits stay within 1e-3 of the f32
// reference at a trained head's scale (plain bf16 operands: 5.5e-2, profiles/r02_precision_bf16_baseline.txt).
//
// Replaces ResidualBlock.forward (/root/reference/src/model.py:285-293) with the projection skip of :280-283,
// BatchNorm folded.  Every operand of every product -- activations and BN-folded weights -- is carried as a
// pair of bf16 values x = hi + lo (hi = bf16(x), lo = bf16(x - hi): 16 significant bits) and every k-step is
// three MFMAs into one f32 accumulator: hi*hi + hi*lo + lo*hi (the lo*lo term, 2^-18 relative, is dropped).
// Activations live in HBM as f32 (NHWC) and are split when they enter LDS.
//
// One 4-wave workgroup = G clips.  A workgroup takes <= 80 KB of LDS, so that at least TWO share a CU and one's staging /
// epilogue overlaps the other's MFMA phases, for block 0 up to 24 rows (images of up to 98 rows; the shipped 22 rows:
// 78 368 B) and block 1 at every height but 12 rows (the shipped 11x13, two clips: 81 440 B); block 0 at 26 / 27 rows
// (91 / 89 KB) and block 1 at 12 rows (88 KB, two clips) run one workgroup per CU.
//   * x is staged once into two LDS planes (hi, lo).  A plane is chunk-planar -- [8-channel chunk][pixel] of 16-byte
//     cells -- and its pixels are stored parity-split (even / odd image rows x even / odd columns, each sub-image with
//     the row pitch of the OUTPUT image), so the output pixels of a tile read, for any tap of the stride-2 conv1 as
//     for the stride-1 conv2 over h, CONSECUTIVE cells of one chunk plane, and a tap's address is the tile's base + a
//     compile-time constant.  No fragment is predicated; where a tap outside the image finds its zeros is a property of
//     the instantiation (resnet_plan.h: rbx_layout, rbx_border_x):
//       - bordered x planes (the 16x16x32 body of block 0 at 16, 17, 22 and 26 rows, where the LDS bound leaves room):
//         the zeros lie where those taps point -- the unused column of the odd-column sub-images of the odd-width image
//         and short zero runs in front of / behind the sub-images -- so conv1 and the projection read base + immediate
//         and nothing else (no tap mask, no select);
//       - everywhere else (block 0 at 23 / 24 rows and its 32x32x16 body, block 1, and h for conv2 in every body) the
//         planes carry no border: a select redirects such a tap to zero cells kept beside the planes.  In the
//         16x16x32 body the select is one v_cndmask_b32 per (tile, tap) pair whose 64-lane mask is a compile-time
//         constant (rbx_taps.h: rbx_tap_mask -- a lane's pixel is 16 t + (lane & 15)) held in a scalar register pair;
//         a pair with every lane inside the image (most of tap (1, 1)) takes none, and no per-lane tap mask exists.  h
//         stays so on purpose: a bordered h (row pitch OW + 1) puts two lanes of every ds_read_b128 lane group of
//         conv2 on one bank, and the LDS cycles that costs outweigh the selects (profiles/r10_block_borders.txt).
//   * conv1 (3x3 s2) accumulates into acc1; the 1x1 s2 projection of x then opens conv2's accumulator acc2, so x is
//     dead afterwards and h = ReLU(conv1 + b1) is written (split) OVER the x planes; conv2 (3x3 s1) runs out of h.
//   * MFMA operands are swapped (weights = A): a lane owns one pixel x 4 consecutive channels per accumulator quad,
//     so h and the output tile are written with 8 / 16-byte LDS stores.  Weight fragments (hi, lo) stream from L2 in
//     fragment order through a register ring.  Two bodies (RbxCfg::T16):
//       - block 0 up to 26 rows and block 1 (rbx_t16): v_mfma_f32_16x16x32_bf16 only.  Wave w owns CT = 1 (block 0) or
//         2 (block 1) 16-channel tiles of EVERY 16-pixel tile (block 0 at 22x25: 143 pixels = 9 tiles; block 1 at 11x13:
//         2 clips x 42 pixels = 6 tiles; no partial-tile code path), so CT (hi, lo) weight pairs per k32-step feed all
//         the tiles.  Activation fragments are fetched P tiles ahead.  A fragment read puts lanes 16c..16c+15 in chunk
//         plane c (+ 4 for block 1's second k32-step of a conv1 tap); planes are laid out so that the ds_read_b128
//         lane groups cover all 16 cell residues mod 16; border reads are bank-conflict-free too: in bordered planes
//         they are reads like any other, elsewhere the zeros come from rows of 16 cells read at the residue of the
//         lane's in-image cell (RbxCfg).
//       - block 0 at 27 rows: v_mfma_f32_32x32x16_bf16; wave (mg, ng) owns up to MW 32-pixel tiles x one 32-channel
//         tile; activation fragments are fetched one k-step ahead.  The 32 lanes of a chunk read 32 consecutive cells,
//         conflict-free at any plane alignment.
//   * epilogue: ReLU(acc2 + b2) -> f32 [pixel][COUT] tile in LDS -> one contiguous run of 16-byte global stores;
//     block 1 also finishes the head (global mean -> Linear(128, 2) -> softmax / argmax, model.py:242-265).
#pragma once
#include <utility>

#include "common.h"
#include "nn_common.h"
#include "resnet_plan.h"   // rbx_t16: which body a block runs; rbx_layout: where its pixels and zeros live in LDS
#include "rbx_taps.h"      // rbx_tap_mask: the lanes of a (tile, tap) whose tap lies inside the image; rbx_zero_cell

namespace cough {
namespace {

#ifdef COUGH_K1_STAMPS
// diagnostic build only (tools/rb_stamps.py, tools/rbx_stamps.py): per-workgroup s_memtime at phase boundaries, written to
// a buffer of its own that no other code reads.  Never compiled into libcough_amd.so.
__device__ unsigned long long* g_rb_stamp_buf = nullptr;
#define RB_STAMP(slot)                                                                        \
    do {                                                                                      \
        if (g_rb_stamp_buf && threadIdx.x == 0)                                               \
            g_rb_stamp_buf[(size_t)blockIdx.x * 8 + (slot)] = __builtin_amdgcn_s_memtime();   \
    } while (0)
#else
#define RB_STAMP(slot) do { } while (0)
#endif

struct RbxArgs {
    const float* x;       // [B][XH][XW][CIN] f32 NHWC
    int n_clips;
    const bf16_t* wf;     // MFMA fragments in k-step order, in the layout of the kernel's body (rbx_t16): conv1 (K = 9*CIN), projection (CIN), conv2 (9*COUT).
                          //   32x32x16 body: [K/16][COUT/32][2 = hi, lo][64 lanes][8]; lane (r, h) of (step s, tile t) holds
                          //   W[32t + r][16s + 8h .. +7] of its operand (pack_x3_fragments)
                          //   T16 body: [K/32][COUT/16][2][64 lanes][8]; lane l of (k32-step q, tile t) holds
                          //   W[16t + (l & 15)][32q + 8(l >> 4) .. +7] (pack_x3_t16_fragments)
    const float* b1;      // [COUT] folded conv1 bias
    const float* b2;      // [COUT] folded conv2 bias + projection bias
    float* out;           // [B][OH][OW][COUT] f32 NHWC, or nullptr (pipeline: only the fused head reads block 1's output)
    const float* fcw;     // fused head (block 1; nullptr: none): [2][COUT]
    const float* fcb;     // [2]
    float* logits;        // [B][2]
    float* probs;         // [B][2] or nullptr
    int* preds;           // [B] or nullptr
    const int* nanflag;   // fused head: [B] or nullptr; 1 = the clip's image holds a NaN -> NaN logits (nn_common.h: NaN rule)
};

template <int CIN, int COUT, int G, int XH, int XW>
struct RbxCfg {
    static constexpr int WAVES = 4, THREADS = 256;
    static constexpr bool T16 = rbx_t16(CIN, COUT, XH);
    static constexpr int OH = (XH - 1) / 2 + 1, OW = (XW - 1) / 2 + 1;
    static constexpr int NPX = XH * XW, PER = OH * OW, M = G * PER;
    // 32x32x16 body: NT 32-channel tiles, MG groups of MW 32-pixel tiles, 16-wide k-steps
    static constexpr int NT = COUT / 32, MG = WAVES / NT, TILES = (M + 31) / 32;
    static constexpr int MW = (TILES + MG - 1) / MG;
    static constexpr int KS1 = 9 * CIN / 16, KSP = CIN / 16, KS2 = 9 * COUT / 16, KS = KS1 + KSP + KS2;
    // T16 body: CT 16-channel tiles and NP 16-pixel tiles per wave, 32-wide k-steps
    static constexpr int CT = COUT / 16 / WAVES, NP = (M + 15) / 16;
    static constexpr int KQ1 = 9 * CIN / 32, KQP = CIN / 32, KQ2 = 9 * COUT / 32, KQ = KQ1 + KQP + KQ2;
    static_assert(!T16 || ((CT == 1 || CT == 2) && COUT == 16 * CT * WAVES && (CIN == 32 || CIN == 64) && G <= 2 &&
                           PER >= 16),
                  "T16: one or two 16-channel tiles per wave, one or two k32-steps per conv1 tap, at most one 16-pixel "
                  "tile straddling two clips");
    static constexpr int CHI = CIN / 8, CHO = COUT / 8;
    // ---- the LDS layout: resnet_plan.h (rbx_layout) holds the arithmetic and the description of the planes ----
    static constexpr RbxGeo L = rbx_geo(CIN, COUT, G, XH, XW);
    static_assert(L.t16 == T16 && L.m == M && L.np == NP && L.chi == CHI && L.cho == CHO, "rbx_layout describes this instantiation");
    // x planes: parity-split pixel order.  Sub-image (row parity a, column parity b) holds pixels (2i + a, 2j + b) at
    // i * OW + j; RE / RO = number of even / odd rows; the odd-column sub-images of an odd XW carry one unused column.
    // BX: bordered x planes (rbx_border_x) -- the zeros lie where conv1's taps outside the image point, and a tap's
    // address is the tile's base + a compile-time offset; else a tap outside the image is redirected to a zero cell.
    static constexpr bool BX = L.border_x;
    static constexpr int RE = L.re, RO = L.ro;
    static constexpr int NPP = L.npp;                                        // cells of one clip in one chunk plane
    static constexpr int PB01 = L.b01, PB10 = L.b10, PB11 = L.b11;           // sub-image bases (PB00 = 0)
    static constexpr int NZX = BX ? rbx_x_nzero(RE, RO, OW) : 0;             // bordered x: zero cells of a chunk plane
    // x cells between the starts of two clips in a chunk plane.  T16 with two clips: NPP rounded so that NPPC - PER is
    // a multiple of 16, and the 16 pixels of a tile that straddles the clips still read 16 distinct residues mod 16.
    static constexpr int NPPC = L.nppc;
    // Bytes of one x / h chunk plane and the zero cells that taps outside the image read.  32x32x16 body: one zero cell
    // at the end of each chunk plane (byte offset ZX / ZH inside the plane).
    // T16: a ds_read_b128 lane group (MI355X: lanes {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same in the upper
    // half) takes complementary pixels from chunk planes (lane >> 4) = 0 and 1 (2 and 3), so planes read by lanes 16
    // apart must lie a multiple of 256 B apart; where a select supplies the zeros they come from 256-B-aligned rows of 16
    // cells, and a lane whose tap lies outside the image reads the zero cell with the bank residue of its in-image cell.
    //   x, CIN = 32 (conv1 and the projection read chunk plane lane >> 4 only): planes padded to 256 B; un-bordered, one
    //     zero row after the four; bordered, the zeros are cells of the planes and a border read is as conflict-free as
    //     any other (16 consecutive cells of one chunk plane per 16 lanes).
    //   x, CIN = 64: a tap's second k32-step reads plane 4 + (lane >> 4) at the immediate offset KX.  Planes are padded to
    //     64 B only (so that four of them span a multiple of 256 B), in the order
    //       [zero row][x0][x2][zero row][x4][x6][x1][x3][256 B unused][x5][x7],
    //     which puts x1 / x3 / x5 / x7 4 planes + 256 B past x0 / x2 / x4 / x6, every plane c + 4 KX = 2 planes + 256 B
    //     past plane c, and the second zero row KX past the first.  Padding every plane to 256 B would take block 1 at
    //     11x13 past 80 KB, and one workgroup per CU.
    //   h: planes padded to 256 B, one zero row at the end of each (conv2's k32-step c of a tap reads chunk plane
    //     4c + (lane >> 4) at an immediate offset).
    static constexpr int ZC = L.zc;
    static constexpr int CPX = L.cpx;
    static constexpr int xoff(int c) { return rbx_xoff(T16, CHI, CPX, c); }   // byte offset of x chunk plane c
    static constexpr int ZX = L.zx;
    static constexpr int KX = L.kx;
    static constexpr int ZH = L.zh;
    static constexpr int CPH = L.cph;
    static constexpr int XBYTES = L.xbytes, HBYTES = L.hbytes;
    static_assert(!T16 || ((BX || ZX % 256 == 0) && CPX % (CHI == 4 ? 256 : 64) == 0 && CPH % 256 == 0 && (G == 1 || (NPPC - PER) % 16 == 0)),
                  "T16 bank residues");
    static_assert(!T16 || CHI == 4 || ((xoff(1) - xoff(0)) % 256 == 0 && (xoff(3) - xoff(2)) % 256 == 0 &&
                                       xoff(5) - xoff(1) == KX && xoff(6) - xoff(2) == KX && xoff(7) - xoff(3) == KX &&
                                       xoff(0) >= ZX + 256 && xoff(2) + CPX <= ZX + KX && xoff(4) >= ZX + KX + 256),
                  "T16 x layout, CIN = 64");
    // bordered x: four 256-B-padded chunk planes of one clip, odd XW; the largest cell any lane can form -- the last
    // tile's padding rows at tap (2, 2) included -- lies inside its chunk plane
    static_assert(!BX || (T16 && CHI == 4 && G == 1 && XW % 2 == 1 && (16 * NP - 1 + PB11 + 1) * 16 <= CPX &&
                          PB11 + RO * OW + (RE > RO ? OW : 0) <= NPP && PB01 % 8 >= 2 && (PB11 - PB10) % 8 >= 2),
                  "bordered x planes");
    static constexpr int PL = L.pl;                                          // pitch between the hi and lo planes
    static constexpr int BIAS = L.bias;                                      // b1[COUT], b2[COUT] f32
    static constexpr int HRED = L.hred;                                      // head reduction scratch [WAVES][2] f32
    static constexpr int LDS = L.lds;
    static constexpr int OP = COUT + 4;                                      // floats per row of the f32 output tile
    static_assert(T16 || (WAVES % NT == 0 && MG * MW * 32 >= M), "tile split");
    static_assert(OW == (XW + 1) / 2, "sub-image row pitch");
    static_assert(M * OP * 4 <= 2 * PL, "the output tile lies over the planes");
    static constexpr int STAGE_MAX = 18;                                     // 16-byte pieces per thread staged in one batch
    static_assert((G * NPX * CIN / 4 + THREADS - 1) / THREADS <= 2 * STAGE_MAX, "staging registers (f32 input, two batches)");
    static_assert(LDS <= 160 * 1024, "one workgroup must fit a CU");
    // two workgroups per CU (one's staging / epilogue overlaps the other's MFMA phases): block 0 up to 24 rows, block 1
    // at every compiled height but 12 rows (two clips of 6x7 outputs)
    static_assert(LDS <= 80 * 1024 || (CIN == 32 && XH > 24) || (CIN == 64 && XH == 12), "two workgroups per CU");
};

template <int CIN, int COUT, int G, int XH, int XW>
__global__ __launch_bounds__(256, 2) void resblock_x3_kernel(RbxArgs a) {
    using Cfg = RbxCfg<CIN, COUT, G, XH, XW>;
    constexpr int THREADS = Cfg::THREADS, OH = Cfg::OH, OW = Cfg::OW, NPX = Cfg::NPX, PER = Cfg::PER, M = Cfg::M;
    constexpr bool T16 = Cfg::T16;
    using f32x4 = __attribute__((ext_vector_type(4))) float;
    constexpr int CHI = Cfg::CHI, CHO = Cfg::CHO, PL = Cfg::PL, OP = Cfg::OP, CPX = Cfg::CPX, CPH = Cfg::CPH, NPP = Cfg::NPP;
    constexpr int ZX = Cfg::ZX, KX = Cfg::KX, ZH = Cfg::ZH, ZC = Cfg::ZC, NPPC = Cfg::NPPC;   // the zero cells (RbxCfg)
#ifndef RBX_D
#define RBX_D 4
#endif
#ifndef RBX_DQ
#define RBX_DQ 3
#endif
#ifndef RBX_P
#define RBX_P 2
#endif
#ifndef RBX_PRIO
#define RBX_PRIO 0
#endif
    extern __shared__ __attribute__((aligned(256))) char smem[];
    float* lbias = reinterpret_cast<float*>(smem + Cfg::BIAS);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int clip0 = blockIdx.x * G;
    const int nvalid = a.n_clips - clip0 < G ? a.n_clips - clip0 : G;
    RB_STAMP(0);

    // biases first: vector-memory loads return in issue order, so a bias loaded after the staging loads and stored
    // to LDS straight away would drain every load of wave 0 before its first piece is split
    float bv1 = 0.f, bv2 = 0.f;
    if (tid < COUT) { bv1 = a.b1[tid]; bv2 = a.b2[tid]; }

    // ---- weight fragment stream (hi, lo per k-step): the first DW k-steps are in flight during the staging ----
    // prefetch depth in k-steps (T16: one k32-step = NP x CT x 3 MFMAs >= 288 cycles).  Block 1 with one clip (13 / 14
    // rows, NP = 4) holds 2 k32-steps, so that it stays within 168 VGPRs and three workgroups per CU.
    constexpr int CT = T16 ? Cfg::CT : 1;      // channel tiles per wave and k-step in the ring
    constexpr int DW = !T16 ? RBX_D : CT == 2 && G == 1 ? 2 : RBX_DQ;
    // A fragment's address is a scalar base (the array + the k-step's bytes, formed on the scalar unit; the empty asm
    // keeps the compiler from folding the step into a 64-bit vector addition per load) + this lane's 32-bit offset + an
    // immediate (channel tile, plane): global_load_dwordx4 v, voff, s[base:base+1] offset:imm.
    // (The offset is extended to 64 bits next to the load only if it is defined in the load's basic block: WLANE_HERE,
    // an empty asm too, re-defines it at the head of each k-loop.)
    unsigned wlane = unsigned(T16 ? wave * CT : wave % Cfg::NT) * 2048u + lane * 16u;   // bytes
#define WLANE_HERE() asm("" : "+v"(wlane))
    constexpr int WSTEP = T16 ? COUT / 16 : Cfg::NT;   // channel tiles per k-step in the fragment array
    static_assert((CT * 2 - 1) * 1024 < 4096, "channel tile and plane inside the load's immediate offset");
    auto wfrag = [&](int s, int ct, int plane) -> bf16x8 {
        using gbytes = const __attribute__((address_space(1))) char*;
        using gfrag = const __attribute__((address_space(1))) bf16x8*;
        gbytes sb = (gbytes)a.wf + size_t(s) * WSTEP * 2048;
        asm("" : "+s"(sb));
        return *(gfrag)(sb + wlane + (ct * 2 + plane) * 1024);
    };
    bf16x8 ring[DW][CT][2];
#pragma unroll
    for (int i = 0; i < DW; ++i)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) { ring[i][ct][0] = wfrag(i, ct, 0); ring[i][ct][1] = wfrag(i, ct, 1); }

    // ---- stage: the clips' x (f32) is one linear run of 16-byte pieces = 4 channels of one pixel; all loads are
    // issued first, then each piece is split and its hi / lo halves go to the swizzled chunk of the two planes ----
    {
        constexpr int NPIECE = G * NPX * CIN / 4, UN = (NPIECE + THREADS - 1) / THREADS, QP = CIN / 4;
        // the shipped image stages in ONE batch (all loads in flight before the first split); a larger image (103- / 110-row
        // features) in two, so that the staging registers stay within the accumulators' budget
        constexpr int NB = UN <= Cfg::STAGE_MAX ? 1 : 2, UNB = (UN + NB - 1) / NB;
        const float4* src = reinterpret_cast<const float4*>(a.x + (long long)clip0 * NPX * CIN);
        if constexpr (Cfg::BX) {
            // the zero cells of every chunk plane, hi and lo: the unused column of the odd-column sub-images and the
            // runs in front of / behind the sub-images (rbx_x_zero)
            constexpr int NZX = Cfg::NZX;
            for (int z = tid; z < 2 * CHI * NZX; z += THREADS) {
                const int pl = z / NZX;
                const int cell = rbx_x_zero(Cfg::PB01, Cfg::PB10, Cfg::PB11, OW, Cfg::RE, Cfg::RO, z % NZX);
                *reinterpret_cast<uint4*>(smem + (pl / CHI) * PL + Cfg::xoff(pl % CHI) + cell * 16) = make_uint4(0, 0, 0, 0);
            }
        } else if constexpr (T16) {
            constexpr int NZ = CHI / 4;   // the zero rows (one per k32-step of a tap), hi and lo
            if (tid < 2 * NZ * ZC) {
                const int k = tid / ZC;
                *reinterpret_cast<uint4*>(smem + (k / NZ) * PL + ZX + (k % NZ) * KX + (tid % ZC) * 16) = make_uint4(0, 0, 0, 0);
            }
        } else if (tid < 2 * CHI) {   // the zero cell of every chunk plane, hi and lo
            *reinterpret_cast<uint4*>(smem + (tid / CHI) * PL + (tid % CHI) * CPX + ZX) = make_uint4(0, 0, 0, 0);
        }
        // FULL: every clip of the workgroup exists -- always with one clip per workgroup, and with two in every workgroup
        // but the last of a launch -- so the clamp and the zeroing below compare with the compile-time NPIECE and the
        // pieces carry no batch-end branch; the last workgroup of a two-clip launch takes the other instance.
        auto stage = [&](auto fullc) {
            constexpr bool FULL = decltype(fullc)::value;
            const int valid = FULL ? NPIECE : nvalid * NPX * QP;
#pragma unroll
            for (int b0 = 0; b0 < UN; b0 += UNB) {
                float4 v[UNB];
#pragma unroll
                for (int u = 0; u < UNB; ++u) {
                    // unconditional, index-clamped loads: a load under a branch makes the compiler drain vmcnt to 0 before the
                    // first piece is split; clamped, the pieces are processed as they arrive (vmcnt(UNB - 1 - u))
                    const int i = tid + (b0 + u) * THREADS;
                    v[u] = src[i < valid ? i : valid - 1];
                }
#pragma unroll
                for (int u = 0; u < UNB; ++u) {
                    const int i = tid + (b0 + u) * THREADS;
                    if (i < NPIECE) {
                        const int P = i / QP, q = i % QP;                      // raster pixel (clip, row, column), quarter-chunk
                        const int g = P / NPX, rem = P % NPX, ih = rem / XW, iw = rem % XW;
                        const int cell = RBX_X_CELL(g * NPPC, Cfg::PB01, Cfg::PB10, Cfg::PB11, OW, ih, iw);
                        uint2 hi, lo;
                        if (!FULL && i >= valid) v[u] = make_float4(0.f, 0.f, 0.f, 0.f);   // clips beyond the batch read as zeros
                        split4(v[u].x, v[u].y, v[u].z, v[u].w, hi, lo);
                        const int off = Cfg::xoff(q >> 1) + cell * 16 + (q & 1) * 8;
                        *reinterpret_cast<uint2*>(smem + off) = hi;
                        *reinterpret_cast<uint2*>(smem + off + PL) = lo;
                    }
                }
            }
        };
        if constexpr (G == 1) stage(std::true_type{});
        else if (nvalid == G) stage(std::true_type{});
        else stage(std::false_type{});
    }
    if (tid < COUT) { lbias[tid] = bv1; lbias[COUT + tid] = bv2; }
    float fw0 = 0.f, fw1 = 0.f, fb0 = 0.f, fb1 = 0.f;   // fused head (block 1): Linear(128, 2) weights of channel tid & 127
    if constexpr (COUT == 128) {
        if (a.fcw != nullptr) {
            fw0 = a.fcw[tid & 127]; fw1 = a.fcw[128 + (tid & 127)];
            fb0 = a.fcb[0]; fb1 = a.fcb[1];
        }
    }
    int nan_clip = 0;   // NaN rule (nn_common.h): the verdict on this thread's clip, fetched here so that its latency is long gone
    if constexpr (COUT == 128) {
        if (a.fcw != nullptr && a.nanflag != nullptr && (tid & 127) == 0 && (tid >> 7) < nvalid) nan_clip = a.nanflag[clip0 + (tid >> 7)];
    }

    // cell offset of conv1 tap (kh, kw) from cell (oh, ow) of sub-image (0, 0) (rbx_x_tap)
    auto tapx = [](int kh, int kw) constexpr -> int { return rbx_x_tap(Cfg::PB01, Cfg::PB10, Cfg::PB11, Cfg::OW, kh, kw); };

    constexpr int NT = Cfg::NT, MW = Cfg::MW, KS1 = Cfg::KS1, KSP = Cfg::KSP, KS = Cfg::KS, D = DW;
    const int r = lane & 31, h = lane >> 5, ng = wave % NT, mg = wave / NT;
    // ---- per-lane geometry: lane r owns output pixel R of each of its tiles ---------------------------------
    int goh[MW], gow[MW], px1[MW], ph1[MW];
    bool rok[MW];
#pragma unroll
    for (int mt = 0; mt < MW; ++mt) {
        const int R = (mg * MW + mt) * 32 + r;
        rok[mt] = R < M;
        const int Rc = rok[mt] ? R : 0;
        const int g = Rc / PER, rem = Rc % PER;
        goh[mt] = rok[mt] ? rem / OW : -4;   // -4: every tap of a padding row is out of range -> the zero pixel
        gow[mt] = rem % OW;
        px1[mt] = (g * NPP + rem) * 16 + h * CPX;   // byte offset of x cell (clip, oh, ow) of sub-image (0, 0), this lane's chunk
        ph1[mt] = Rc * 16 + h * CPH;                // byte offset of h cell R, this lane's chunk
    }

    // ---- T16 body: lane l owns pixel (l & 15) of every 16-pixel tile and chunk (l >> 4) of every 32-wide k-step;
    // its accumulator quads are channels n0 + 16 ct .. +3 (n0 = 16 CT wave + 4 (l >> 4), channel tile ct < CT) ----
    constexpr int NP = Cfg::NP, KQ1 = Cfg::KQ1, KQP = Cfg::KQP, KQ = Cfg::KQ, P = RBX_P, NB = P + 1;
    constexpr int NI = KQ * NP, I2 = (KQ1 + KQP) * NP;   // (k32-step, tile) pairs; the first pair of conv2
    const int px = lane & 15, tq = lane >> 4, n0 = 16 * CT * wave + 4 * tq;
    // Pixel R of clip g has x cell g * NPPC + R - g * PER of sub-image (0, 0): tile t's cells are this lane's base +
    // 256 t bytes, + DX from the tile past the clip boundary on; the one tile that straddles it takes its base from lbs.
    // Pixel R's h cell is R.
    // These bases are absolute LDS addresses: the workgroup's LDS base is folded in here, once, and what aaddr forms
    // from them is the operand of the ds_read itself.
    using lds_bytes = const __attribute__((address_space(3))) char*;
    using lds_frag = const __attribute__((address_space(3))) bf16x8*;
    const int lds0 = int(reinterpret_cast<size_t>((lds_bytes)smem));
    constexpr int DX = (NPPC - PER) * 16;
    const int lbx = lds0 + px * 16 + Cfg::xoff(tq), lbh = lds0 + px * 16 + tq * CPH, zh = lds0 + ZH + tq * CPH, zx = lds0 + ZX;
    const int lbs = lbx + (G > 1 && px >= PER % 16 ? DX : 0);
    // the zero cell a lane reads for a tap outside the image: the one with the bank residue (mod 16 cells) of its
    // in-image cell; rx is the residue of the lane's x cell of tile 0 (x planes with CIN = 64 are not 256-B aligned)
    const int rx = px + (CHI == 4 ? 0 : Cfg::xoff(tq) / 16);
    // Which lanes of a (tile, tap) pair read their cell and which a zero cell is known here: the pixel of lane l of tile t
    // is 16 t + (l & 15), so the 64-lane mask is a constant (rbx_taps.h: rbx_tap_mask; a padding row R >= M reads zeros at
    // every tap).  It reaches v_cndmask_b32 as a scalar register pair the compiler fills with s_mov; the statement holds
    // that one instruction, whose operands -- two vector registers written by vector instructions, a scalar pair
    // written by the scalar unit -- need no wait states.  A pair whose 64 lanes all lie inside takes no select at all.
    auto lane_select = [](unsigned long long inside, int cell, int zero) -> int {
        int r;
        asm("v_cndmask_b32 %0, %1, %2, %3" : "=v"(r) : "v"(zero), "v"(cell), "s"(inside));
        return r;
    };
    RB_STAMP(1);
    __syncthreads();
    RB_STAMP(2);
#if RBX_PRIO
    __builtin_amdgcn_s_setprio(1);   // MFMA phases outrank the co-resident workgroup's staging / epilogue VALU work
#endif

    // ---- T16 body ----
    auto body16 = [&]() {
        f32x4 acc1[CT][NP], acc2[CT][NP];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int t = 0; t < NP; ++t) { acc1[ct][t] = f32x4{0.f, 0.f, 0.f, 0.f}; acc2[ct][t] = f32x4{0.f, 0.f, 0.f, 0.f}; }

        // The zero cell a lane reads for a tap depends on the lane and the tap, not on the tile.  ZREG: the nine cells of
        // the operand stay in registers (made opaque, or the compiler forms each again at every select), so a select is
        // one v_add_u32 (the cell) and the v_cndmask_b32.  Else -- block 1 with one clip, which stays within 168 VGPRs --
        // the zero cell is formed from the cell's own residue with one v_and_or_b32 (the LDS base and the zero rows are
        // 256-B aligned).
        constexpr bool ZREG = !(CT == 2 && G == 1);
        int zxc[9], zhc[9];
        auto zero_cells = [&](auto opc) {
            constexpr int op = decltype(opc)::value;
            if constexpr (ZREG && !(op == RBX_OP_X && Cfg::BX)) {
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) {
                    int z = op == RBX_OP_X ? rbx_zero_cell(zx, rx + tapx(tap / 3, tap % 3)) : rbx_zero_cell(zh, px + rbx_h_tap(OW, tap / 3, tap % 3));
                    asm("" : "+v"(z));
                    (op == RBX_OP_X ? zxc : zhc)[tap] = z;
                }
            }
        };
        // Address of the hi fragment of pair i = (k32-step i / NP, tile i % NP), compile-time at every call site.  The
        // tap's cell (base + compile-time offset) or the zero cell is chosen at the tap's first k32-step; further
        // k32-steps of the tap (chunk planes) and the lo plane are immediate offsets.
        int tadr[NP];
        auto aaddr = [&](auto ic) -> int {
            constexpr int i = decltype(ic)::value, q = i / NP, t = i % NP;
            constexpr bool conv1 = q < KQ1, proj = !conv1 && q < KQ1 + KQP;
            constexpr int kt = (conv1 ? q : proj ? q - KQ1 : q - KQ1 - KQP) * 32;   // k inside this operand
            constexpr int C = (conv1 || proj) ? CIN : COUT;
            constexpr int tap = proj ? 4 : kt / C, c32 = (kt % C) / 32, kh = tap / 3, kw = tap % 3;
            if constexpr (Cfg::BX && (conv1 || proj)) {
                // bordered x (one clip, one k32-step per tap): the lane's base + an immediate, inside or outside the image
                return lbx + (256 * t + 16 * tapx(kh, kw));
            } else if constexpr (c32 == 0) {
                if constexpr (conv1 || proj) {
                    constexpr bool strad = G > 1 && 16 * t < PER && 16 * t + 16 > PER;
                    constexpr int off = 256 * t + (G > 1 && 16 * t >= PER ? DX : 0) + 16 * tapx(kh, kw);
                    constexpr unsigned long long in = rbx_tap_mask(Cfg::L, RBX_OP_X, t, tap);
                    const int cell = (strad ? lbs : lbx) + off;
                    if constexpr (in == ~0ull) tadr[t] = cell;
                    else tadr[t] = lane_select(in, cell, ZREG ? zxc[tap] : zx | (cell & 0xF0));
                } else {
                    constexpr int off = 256 * t + 16 * rbx_h_tap(OW, kh, kw);
                    constexpr unsigned long long in = rbx_tap_mask(Cfg::L, RBX_OP_H, t, tap);
                    const int cell = lbh + off;
                    if constexpr (in == ~0ull) tadr[t] = cell;
                    else tadr[t] = lane_select(in, cell, ZREG ? zhc[tap] : zh | (cell & 0xF0));
                }
            }
            return tadr[t] + c32 * ((conv1 || proj) ? KX : 4 * CPH);
        };
        auto ldsfrag = [](int addr) -> bf16x8 { return *reinterpret_cast<lds_frag>(addr); };
        zero_cells(std::integral_constant<int, RBX_OP_X>{});
        bf16x8 af[NB][2];
        WLANE_HERE();
        auto fetch = [&](auto ic) {
            constexpr int i = decltype(ic)::value;
            const int p = aaddr(ic);
            af[i % NB][0] = ldsfrag(p);
            af[i % NB][1] = ldsfrag(p + PL);
        };
        [&]<int... Js>(std::integer_sequence<int, Js...>) {
            (fetch(std::integral_constant<int, Js>{}), ...);
        }(std::make_integer_sequence<int, P>{});

        auto pair = [&]<int i>() {
            constexpr int q = i / NP, t = i % NP, j = i + P;
            if constexpr (i == I2) {
                // ---- x is dead: h = ReLU(conv1 + b1), split, goes over the x planes ----
                RB_STAMP(3);
#if RBX_PRIO
                __builtin_amdgcn_s_setprio(0);
#endif
                __syncthreads();
                for (int z = tid; z < 2 * CHO * ZC; z += THREADS) {   // the zero cells of every h chunk plane, hi and lo
                    const int pl = z / ZC;
                    *reinterpret_cast<uint4*>(smem + (pl / CHO) * PL + (pl % CHO) * CPH + ZH + (z % ZC) * 16) =
                        make_uint4(0, 0, 0, 0);
                }
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) {
                    const int n = n0 + 16 * ct;
                    const float4 bb = *reinterpret_cast<const float4*>(lbias + n);
#pragma unroll
                    for (int u = 0; u < NP; ++u) {
                        const int R = 16 * u + px;
                        uint2 hi, lo;
                        split4(fmaxf(acc1[ct][u][0] + bb.x, 0.f), fmaxf(acc1[ct][u][1] + bb.y, 0.f),
                               fmaxf(acc1[ct][u][2] + bb.z, 0.f), fmaxf(acc1[ct][u][3] + bb.w, 0.f), hi, lo);
                        if (R < M) {
                            const int off = (n >> 3) * CPH + R * 16 + ((n >> 2) & 1) * 8;
                            *reinterpret_cast<uint2*>(smem + off) = hi;
                            *reinterpret_cast<uint2*>(smem + off + PL) = lo;
                        }
                    }
                }
                __syncthreads();
                RB_STAMP(4);
                WLANE_HERE();
                zero_cells(std::integral_constant<int, RBX_OP_H>{});
#if RBX_PRIO
                __builtin_amdgcn_s_setprio(1);
#endif
                [&]<int... Js>(std::integer_sequence<int, Js...>) {
                    (fetch(std::integral_constant<int, I2 + Js>{}), ...);
                }(std::make_integer_sequence<int, P>{});
            }
            // The pair's 3 CT MFMAs, kind-major (whi * x_hi, whi * x_lo, wlo * x_hi; channel tiles inner), with one filler
            // group in front of each (~8 free issue cycles): the address of pair i + P; after the last kind-0 MFMA its hi
            // read, after the last kind-1 MFMA its lo read.  The step's last tile also re-fills the weight ring slot it
            // just finished with: a tile's hi weights after its kind-1 MFMA, its lo weights after its kind-2 MFMA.  A
            // prefetch never crosses into conv2: h is written in between.
            constexpr bool pf = j < NI && (j < I2) == (i < I2);
            constexpr bool wl = t == NP - 1 && q + DW < KQ;
            const bf16x8 cur_hi = af[i % NB][0], cur_lo = af[i % NB][1];
            int np = 0;
            if constexpr (pf) np = aaddr(std::integral_constant<int, j>{});
            [&]<int... Ms>(std::integer_sequence<int, Ms...>) {
                ([&] {
                    constexpr int m = Ms, kind = m / CT, ct = m % CT;
                    const bf16x8 w = ring[q % DW][ct][kind == 2 ? 1 : 0];
                    const bf16x8 x = kind == 1 ? cur_lo : cur_hi;
                    __builtin_amdgcn_sched_barrier(0);
                    if constexpr (q < KQ1) acc1[ct][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, x, acc1[ct][t], 0, 0, 0);
                    else acc2[ct][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, x, acc2[ct][t], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                    if constexpr (pf && m == CT - 1) af[j % NB][0] = ldsfrag(np);
                    if constexpr (pf && m == 2 * CT - 1) af[j % NB][1] = ldsfrag(np + PL);
                    if constexpr (wl && kind == 1) ring[q % DW][ct][0] = wfrag(q + DW, ct, 0);
                    if constexpr (wl && kind == 2) ring[q % DW][ct][1] = wfrag(q + DW, ct, 1);
                }(), ...);
            }(std::make_integer_sequence<int, 3 * CT>{});
            __builtin_amdgcn_sched_barrier(0);
        };
        [&]<int... Is>(std::integer_sequence<int, Is...>) {
            (pair.template operator()<Is>(), ...);
        }(std::make_integer_sequence<int, NI>{});

        // ---- epilogue: out = ReLU(conv2 + projection + b2) -> f32 [pixel][COUT] tile over the (dead) planes ----
        RB_STAMP(5);
#if RBX_PRIO
        __builtin_amdgcn_s_setprio(0);
#endif
        __syncthreads();
        float* otile = reinterpret_cast<float*>(smem);
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            const int n = n0 + 16 * ct;
            const float4 bb = *reinterpret_cast<const float4*>(lbias + COUT + n);
#pragma unroll
            for (int t = 0; t < NP; ++t) {
                const int R = 16 * t + px;
                const float4 o = make_float4(fmaxf(acc2[ct][t][0] + bb.x, 0.f), fmaxf(acc2[ct][t][1] + bb.y, 0.f),
                                             fmaxf(acc2[ct][t][2] + bb.z, 0.f), fmaxf(acc2[ct][t][3] + bb.w, 0.f));
                if (R < M) *reinterpret_cast<float4*>(otile + R * OP + n) = o;
            }
        }
    };

    auto body = [&]<int MWX>() {
        f32x16 acc1[MWX], acc2[MWX];
#pragma unroll
        for (int mt = 0; mt < MWX; ++mt) { acc1[mt] = f32x16{0}; acc2[mt] = f32x16{0}; }

        // Activation fragments of k-step s (compile-time at every call site).  A tap's address -- the tile's base cell +
        // a compile-time cell offset, or the zero cell -- is chosen when the first k-step of the tap is fetched; the
        // further k-steps (chunk planes) and the lo plane are immediate offsets.
        int tadr[MWX];
        auto afrag = [&](auto sc, int mt, bf16x8& fhi, bf16x8& flo) {
            constexpr int s = decltype(sc)::value;
            constexpr bool conv1 = s < KS1, proj = !conv1 && s < KS1 + KSP;
            constexpr int kt = conv1 ? s * 16 : proj ? (s - KS1) * 16 : (s - KS1 - KSP) * 16;   // k inside this operand
            constexpr int C = (conv1 || proj) ? CIN : COUT, CP = (conv1 || proj) ? CPX : CPH;
            constexpr int tap = proj ? 4 : kt / C, c16 = (kt % C) / 16, kh = tap / 3, kw = tap % 3;
            if constexpr (c16 == 0) {
                if constexpr (conv1 || proj) {
                    const int ih = 2 * goh[mt] - 1 + kh, iw = 2 * gow[mt] - 1 + kw;
                    const bool ok = unsigned(ih) < unsigned(XH) && unsigned(iw) < unsigned(XW);
                    tadr[mt] = ok ? px1[mt] + tapx(kh, kw) * 16 : ZX + h * CPX;
                } else {
                    const int ih = goh[mt] - 1 + kh, iw = gow[mt] - 1 + kw;
                    const bool ok = unsigned(ih) < unsigned(OH) && unsigned(iw) < unsigned(OW);
                    tadr[mt] = ok ? ph1[mt] + ((kh - 1) * OW + kw - 1) * 16 : ZH + h * CPH;
                }
            }
            const char* p = smem + tadr[mt] + 2 * c16 * CP;
            fhi = *reinterpret_cast<const bf16x8*>(p);
            flo = *reinterpret_cast<const bf16x8*>(p + PL);
        };
        // the address part of afrag alone (the k-loop issues the two reads separately, one in front of each MFMA)
        auto aaddr = [&](auto sc, int mt) -> const char* {
            constexpr int s = decltype(sc)::value;
            constexpr bool conv1 = s < KS1, proj = !conv1 && s < KS1 + KSP;
            constexpr int kt = conv1 ? s * 16 : proj ? (s - KS1) * 16 : (s - KS1 - KSP) * 16;
            constexpr int C = (conv1 || proj) ? CIN : COUT, CP = (conv1 || proj) ? CPX : CPH;
            constexpr int tap = proj ? 4 : kt / C, c16 = (kt % C) / 16, kh = tap / 3, kw = tap % 3;
            if constexpr (c16 == 0) {
                if constexpr (conv1 || proj) {
                    const int ih = 2 * goh[mt] - 1 + kh, iw = 2 * gow[mt] - 1 + kw;
                    const bool ok = unsigned(ih) < unsigned(XH) && unsigned(iw) < unsigned(XW);
                    tadr[mt] = ok ? px1[mt] + tapx(kh, kw) * 16 : ZX + h * CPX;
                } else {
                    const int ih = goh[mt] - 1 + kh, iw = gow[mt] - 1 + kw;
                    const bool ok = unsigned(ih) < unsigned(OH) && unsigned(iw) < unsigned(OW);
                    tadr[mt] = ok ? ph1[mt] + ((kh - 1) * OW + kw - 1) * 16 : ZH + h * CPH;
                }
            }
            return smem + tadr[mt] + 2 * c16 * CP;
        };

        bf16x8 af[2][MWX][2];
        WLANE_HERE();
#pragma unroll
        for (int mt = 0; mt < MWX; ++mt) afrag(std::integral_constant<int, 0>{}, mt, af[0][mt][0], af[0][mt][1]);

        auto step = [&]<int s>() {
            if constexpr (s == KS1 + KSP) {
                // ---- x is dead: h = ReLU(conv1 + b1), split, goes over the x planes ----
                RB_STAMP(3);
#if RBX_PRIO
                __builtin_amdgcn_s_setprio(0);
#endif
                __syncthreads();
                if (tid < 2 * CHO)   // the zero cell of every h chunk plane, hi and lo
                    *reinterpret_cast<uint4*>(smem + (tid / CHO) * PL + (tid % CHO) * CPH + ZH) = make_uint4(0, 0, 0, 0);
#pragma unroll
                for (int mt = 0; mt < MWX; ++mt) {
                    const int R = (mg * MW + mt) * 32 + r;
#pragma unroll
                    for (int gq = 0; gq < 4; ++gq) {
                        const int n0 = ng * 32 + 8 * gq + 4 * h;
                        const float4 bb = *reinterpret_cast<const float4*>(lbias + n0);
                        uint2 hi, lo;
                        split4(fmaxf(acc1[mt][4 * gq] + bb.x, 0.f), fmaxf(acc1[mt][4 * gq + 1] + bb.y, 0.f),
                               fmaxf(acc1[mt][4 * gq + 2] + bb.z, 0.f), fmaxf(acc1[mt][4 * gq + 3] + bb.w, 0.f), hi, lo);
                        if (rok[mt]) {
                            const int off = (n0 >> 3) * CPH + R * 16 + h * 8;
                            *reinterpret_cast<uint2*>(smem + off) = hi;
                            *reinterpret_cast<uint2*>(smem + off + PL) = lo;
                        }
                    }
                }
                __syncthreads();
                RB_STAMP(4);
                WLANE_HERE();
#if RBX_PRIO
                __builtin_amdgcn_s_setprio(1);
#endif
#pragma unroll
                for (int mt = 0; mt < MWX; ++mt)
                    afrag(std::integral_constant<int, s>{}, mt, af[s & 1][mt][0], af[s & 1][mt][1]);
            }
            // Software pipeline, pinned with scheduling barriers: ONE filler sits in front of EACH MFMA of tile mt -- the
            // address math of the next step's fragment, then its hi read (+ the hi weight load D steps ahead), then its lo
            // read (+ the lo weight load) -- so that no filler group is longer than the ~24 issue cycles an MFMA leaves
            // free.  Left alone, the scheduler sinks every ds_read next to its MFMA and each pays the LDS latency; one
            // filler group per MFMA triple (the first version) left the pipe idle behind every third MFMA (+2.3 %).
            const bf16x8 whi = ring[s % D][0][0], wlo = ring[s % D][0][1];
#pragma unroll
            for (int mt = 0; mt < MWX; ++mt) {
                constexpr bool pf = s + 1 < KS && s + 1 != KS1 + KSP;
                const bf16x8 cur_hi = af[s & 1][mt][0], cur_lo = af[s & 1][mt][1];
                const char* np = nullptr;
                if constexpr (pf) np = aaddr(std::integral_constant<int, s + 1>{}, mt);
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (s < KS1) acc1[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(whi, cur_hi, acc1[mt], 0, 0, 0);
                else acc2[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(whi, cur_hi, acc2[mt], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (pf) af[(s + 1) & 1][mt][0] = *reinterpret_cast<const bf16x8*>(np);
                if constexpr (s + D < KS) { if (mt == 0) ring[s % D][0][0] = wfrag(s + D, 0, 0); }
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (s < KS1) acc1[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(whi, cur_lo, acc1[mt], 0, 0, 0);
                else acc2[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(whi, cur_lo, acc2[mt], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (pf) af[(s + 1) & 1][mt][1] = *reinterpret_cast<const bf16x8*>(np + PL);
                if constexpr (s + D < KS) { if (mt == 0) ring[s % D][0][1] = wfrag(s + D, 0, 1); }
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (s < KS1) acc1[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wlo, cur_hi, acc1[mt], 0, 0, 0);
                else acc2[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wlo, cur_hi, acc2[mt], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        [&]<int... Ss>(std::integer_sequence<int, Ss...>) {
            (step.template operator()<Ss>(), ...);
        }(std::make_integer_sequence<int, KS>{});

        // ---- epilogue: out = ReLU(conv2 + projection + b2) -> f32 [pixel][COUT] tile over the (dead) planes ----
        RB_STAMP(5);
#if RBX_PRIO
        __builtin_amdgcn_s_setprio(0);
#endif
        __syncthreads();
        float* otile = reinterpret_cast<float*>(smem);
#pragma unroll
        for (int mt = 0; mt < MWX; ++mt) {
            const int R = (mg * MW + mt) * 32 + r;
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const int n0 = ng * 32 + 8 * gq + 4 * h;
                const float4 bb = *reinterpret_cast<const float4*>(lbias + COUT + n0);
                const float4 o = make_float4(fmaxf(acc2[mt][4 * gq] + bb.x, 0.f), fmaxf(acc2[mt][4 * gq + 1] + bb.y, 0.f),
                                             fmaxf(acc2[mt][4 * gq + 2] + bb.z, 0.f), fmaxf(acc2[mt][4 * gq + 3] + bb.w, 0.f));
                if (rok[mt]) *reinterpret_cast<float4*>(otile + R * OP + n0) = o;
            }
        }
    };
    // a wave whose last tile lies entirely beyond the M valid rows runs the shorter body (one wave-uniform choice)
    constexpr int TILES = Cfg::TILES;
    const int mytiles = TILES - mg * MW < MW ? TILES - mg * MW : MW;
    if constexpr (T16) {
        body16();
    } else if constexpr (MW > 1 && TILES % MW != 0) {
        if (mytiles < MW) body.template operator()<(TILES % MW)>();
        else body.template operator()<MW>();
    } else {
        body.template operator()<MW>();
    }
    __syncthreads();
    RB_STAMP(6);
    const float* otile = reinterpret_cast<const float*>(smem);
    if (a.out != nullptr) {
        const int nvec = nvalid * PER * (COUT / 4);
        float4* o = reinterpret_cast<float4*>(a.out + (long long)clip0 * PER * COUT);
        for (int p = tid; p < nvec; p += THREADS) {
            const int row = p / (COUT / 4), c4 = p % (COUT / 4);
            o[p] = *reinterpret_cast<const float4*>(otile + row * OP + 4 * c4);
        }
    }
    if constexpr (COUT == 128) {
        // ---- fused head (model.py:242-247, :257-265): same summation order as tail_kernel (pixels in order, then
        // the lanes of a wave, then the two waves of a clip) ----
        static_assert(G * 128 <= THREADS, "one thread per (clip, channel)");
        if (a.fcw != nullptr) {
            float* hred = reinterpret_cast<float*>(smem + Cfg::HRED);
            const int c = tid & 127, g = tid >> 7;
            float sum = 0.f;
            if (g < G) {
#pragma unroll 6
                for (int i = 0; i < PER; ++i) sum += otile[(g * PER + i) * OP + c];
            }
            const float mean = sum / float(PER);
            float l0 = wave_sum(mean * fw0), l1 = wave_sum(mean * fw1);
            if (lane == 0) { hred[wave * 2] = l0; hred[wave * 2 + 1] = l1; }
            __syncthreads();
            if (c == 0 && g < nvalid) {
                const int w0 = g * 2;   // the clip's two waves
                l0 = hred[w0 * 2] + hred[(w0 + 1) * 2] + fb0;
                l1 = hred[w0 * 2 + 1] + hred[(w0 + 1) * 2 + 1] + fb1;
                const long long b = clip0 + g;
                if (nan_clip) l0 = l1 = __builtin_nanf("");   // probs NaN, argmax 0 as torch.argmax
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
    RB_STAMP(7);
}
#undef WLANE_HERE

// Host: folded [N][K] weights of conv1, projection and conv2 -> split-bf16 32x32x16 fragments in stream order.
inline void pack_x3_fragments(std::vector<bf16_t>& wf, const std::vector<float>& w1, int K1, const std::vector<float>& wp,
                              int KP, const std::vector<float>& w2, int K2, int N) {
    const int nt = N / 32, ks1 = K1 / 16, ksp = KP / 16, ks2 = K2 / 16, ks = ks1 + ksp + ks2;
    wf.assign(size_t(ks) * nt * 2 * 512, 0);
    for (int s = 0; s < ks; ++s) {
        const std::vector<float>& w = s < ks1 ? w1 : s < ks1 + ksp ? wp : w2;
        const int K = s < ks1 ? K1 : s < ks1 + ksp ? KP : K2;
        const int sl = s < ks1 ? s : s < ks1 + ksp ? s - ks1 : s - ks1 - ksp;
        for (int t = 0; t < nt; ++t)
            for (int lane = 0; lane < 64; ++lane)
                for (int jj = 0; jj < 8; ++jj) {
                    const float v = w[size_t(32 * t + (lane & 31)) * K + 16 * sl + 8 * (lane >> 5) + jj];
                    const size_t base = ((size_t(s) * nt + t) * 2) * 512 + size_t(lane) * 8 + jj;
                    split_bf16_host(v, wf[base], wf[base + 512]);
                }
    }
}

// Host: the same weights as 16x16x32 fragments for the T16 body ([K/32][N/16][2][64 lanes][8], RbxArgs::wf).
inline void pack_x3_t16_fragments(std::vector<bf16_t>& wt, const std::vector<float>& w1, int K1, const std::vector<float>& wp,
                                   int KP, const std::vector<float>& w2, int K2, int N) {
    const int nt = N / 16, q1 = K1 / 32, qp = KP / 32, q2 = K2 / 32, nq = q1 + qp + q2;
    wt.assign(size_t(nq) * nt * 2 * 512, 0);
    for (int q = 0; q < nq; ++q) {
        const std::vector<float>& w = q < q1 ? w1 : q < q1 + qp ? wp : w2;
        const int K = q < q1 ? K1 : q < q1 + qp ? KP : K2;
        const int ql = q < q1 ? q : q < q1 + qp ? q - q1 : q - q1 - qp;
        for (int t = 0; t < nt; ++t)
            for (int lane = 0; lane < 64; ++lane)
                for (int jj = 0; jj < 8; ++jj) {
                    const float v = w[size_t(16 * t + (lane & 15)) * K + 32 * ql + 8 * (lane >> 4) + jj];
                    const size_t base = ((size_t(q) * nt + t) * 2) * 512 + size_t(lane) * 8 + jj;
                    split_bf16_host(v, wt[base], wt[base + 512]);
                }
    }
}

}  // namespace
}  // namespace cough
