// Checks the compile-time lane masks of resblock_x3_kernel's border selects (csrc/rbx_taps.h: rbx_tap_mask) and the zero
// cells a masked lane reads (rbx_zero_x / rbx_zero_h) for every compiled (block, input height).  Host C++17, nothing but the
// two headers: c++ -std=c++17 -I csrc rbx_tap_mask_check.cpp (tests/test_rbx_tap_masks_host.py builds and runs it, once more
// with -fsanitize=address,undefined).
//
// What the mask must say is restated here from the image geometry alone: the workgroup's output pixels are listed in the
// order the kernel numbers them (clip, output row, output column), a lane of tile t owns pixel 16 t + (lane & 15) (32 t +
// (lane & 31) in the 32x32x16 body), and a tap lies inside when its input row and column do.  Per instantiation, for conv1,
// the projection (tap 4 of the same operand) and conv2, and for every (tile, tap, lane):
//   * the mask bit is set exactly when the lane's pixel is one of the workgroup's M and the tap's input pixel lies inside
//     the operand's image;
//   * where the operand's planes carry no border, the zero cell of the lane lies inside the zero rows (the zero cells) that
//     rbx_layout reserves -- the first k-step's row of the x planes, the lane's own chunk plane of h -- and, in the 16x16x32
//     body, has the bank residue (mod 16 cells) of the cell the lane would read inside the image; the form the kernel uses
//     where it keeps no zero cells in registers, zero row | (cell & 0xF0), gives the same cell.
// `--shifted` runs the same checks on every mask moved up by one lane: they must fail (exit status 1).
// stdout: one line per instantiation; exit status 1 and the first failures on stderr if anything does not hold.
#include <cstdio>
#include <cstring>
#include <vector>

#include "resnet_plan.h"
#include "rbx_taps.h"

using namespace cough;

static int g_fail = 0;
#define CHECK(cond, ...)                                                        \
    do {                                                                        \
        if (!(cond)) {                                                          \
            if (++g_fail <= 20) { std::fprintf(stderr, "FAIL %s: ", #cond); std::fprintf(stderr, __VA_ARGS__); std::fputc('\n', stderr); } \
        }                                                                       \
    } while (0)

struct Pixel { int clip, row, col; };

static long check(int blk, const RbxGeo& L, bool shifted) {
    // the workgroup's output pixels, in the kernel's order
    std::vector<Pixel> pix;
    for (int g = 0; g < L.g; ++g)
        for (int r = 0; r < L.oh; ++r)
            for (int c = 0; c < L.ow; ++c) pix.push_back({g, r, c});
    CHECK(int(pix.size()) == L.m, "blk %d xh %d: %zu pixels, m = %d", blk, L.xh, pix.size(), L.m);
    const int lanes_per_tile = L.t16 ? 16 : 32, tiles = (L.m + lanes_per_tile - 1) / lanes_per_tile;
    CHECK(!L.t16 || tiles == L.np, "blk %d xh %d: %d tiles, np = %d", blk, L.xh, tiles, L.np);
    const int DX = (L.nppc - L.per) * 16;
    long bits = 0;
    for (int op = RBX_OP_X; op <= RBX_OP_H; ++op)
        for (int t = 0; t < tiles; ++t)
            for (int tap = 0; tap < 9; ++tap) {
                unsigned long long mask = rbx_tap_mask(L, op, t, tap);
                if (shifted) mask <<= 1;
                const int kh = tap / 3, kw = tap % 3;
                for (int lane = 0; lane < 64; ++lane, ++bits) {
                    const int R = lanes_per_tile * t + lane % lanes_per_tile;
                    bool inside = false;
                    if (R < int(pix.size())) {
                        const Pixel& p = pix[R];
                        if (op == RBX_OP_X) {   // 3x3, stride 2, padding 1 over the XH x XW input (the projection is tap 4)
                            const int ih = 2 * p.row + kh - 1, iw = 2 * p.col + kw - 1;
                            inside = ih >= 0 && ih <= L.xh - 1 && iw >= 0 && iw <= L.xw - 1;
                        } else {                // 3x3, stride 1, padding 1 over the OH x OW image h
                            const int jh = p.row + kh - 1, jw = p.col + kw - 1;
                            inside = jh >= 0 && jh <= L.oh - 1 && jw >= 0 && jw <= L.ow - 1;
                        }
                    }
                    const bool bit = (mask >> lane) & 1;
                    CHECK(bit == inside, "blk %d xh %d %s tile %d tap %d lane %d (pixel %d): mask bit %d, geometry says %d", blk, L.xh,
                          op == RBX_OP_X ? "conv1" : "conv2", t, tap, lane, R, int(bit), int(inside));
                    if (inside || (op == RBX_OP_X && L.border_x)) continue;
                    // ---- the zero cell of a masked lane ----
                    if (op == RBX_OP_X) {
                        const int z = rbx_zero_x(L, lane, tap);
                        if (L.t16) {
                            CHECK(z >= L.zx && z < L.zx + L.zc * 16 && z % 16 == 0 && z + 16 <= L.xbytes,
                                  "blk %d xh %d conv1 tap %d lane %d: zero cell %d outside the zero row at %d", blk, L.xh, tap, lane, z, L.zx);
                            const int px = lane & 15, tq = lane >> 4;
                            const bool strad = L.g > 1 && 16 * t < L.per && 16 * t + 16 > L.per;
                            const int lbx = px * 16 + rbx_xoff(true, L.chi, L.cpx, tq);
                            const int cell = lbx + (strad && px >= L.per % 16 ? DX : 0) + 256 * t + (L.g > 1 && 16 * t >= L.per ? DX : 0) +
                                             16 * rbx_x_tap(L.b01, L.b10, L.b11, L.ow, kh, kw);
                            CHECK(((z / 16) & 15) == ((cell >> 4) & 15), "blk %d xh %d conv1 tile %d tap %d lane %d: zero cell %d, cell %d: bank residues differ",
                                  blk, L.xh, t, tap, lane, z, cell);
                            CHECK(z == (L.zx | (cell & 0xF0)), "blk %d xh %d conv1 tile %d tap %d lane %d: zero row | residue gives %d, not %d", blk, L.xh, t,
                                  tap, lane, L.zx | (cell & 0xF0), z);
                        } else {
                            CHECK(z == (lane >> 5) * L.cpx + L.zx && z + 16 <= L.xbytes, "blk %d xh %d conv1 lane %d: zero cell %d", blk, L.xh, lane, z);
                        }
                    } else {
                        const int z = rbx_zero_h(L, lane, tap);
                        if (L.t16) {
                            const int px = lane & 15, tq = lane >> 4, row = tq * L.cph + L.zh;
                            CHECK(z >= row && z < row + L.zc * 16 && z % 16 == 0 && z + 16 <= L.hbytes,
                                  "blk %d xh %d conv2 tap %d lane %d: zero cell %d outside the zero row at %d", blk, L.xh, tap, lane, z, row);
                            const int cell = px * 16 + tq * L.cph + 256 * t + 16 * rbx_h_tap(L.ow, kh, kw);
                            CHECK(((z / 16) & 15) == ((cell >> 4) & 15), "blk %d xh %d conv2 tile %d tap %d lane %d: zero cell %d, cell %d: bank residues differ",
                                  blk, L.xh, t, tap, lane, z, cell);
                            CHECK(z == (row | (cell & 0xF0)), "blk %d xh %d conv2 tile %d tap %d lane %d: zero row | residue gives %d, not %d", blk, L.xh, t,
                                  tap, lane, row | (cell & 0xF0), z);
                        } else {
                            CHECK(z == (lane >> 5) * L.cph + L.zh && z + 16 <= L.hbytes, "blk %d xh %d conv2 lane %d: zero cell %d", blk, L.xh, lane, z);
                        }
                    }
                }
            }
    return bits;
}

int main(int argc, char** argv) {
    const bool shifted = argc > 1 && std::strcmp(argv[1], "--shifted") == 0;
    if (argc > 1 && !shifted) {
        std::fprintf(stderr, "usage: %s [--shifted]\n", argv[0]);
        return 2;
    }
    int n = 0;
    for (int blk = 0; blk < 2; ++blk)
        for (int i = 0; i < RBX_NROWS[blk]; ++i) {
            const int xh = rbx_rows(blk, i), g = rbx_clips(blk, xh);
            const RbxGeo L = rbx_geo(NET_CH[blk], NET_CH[blk + 1], g, xh, RBX_COLS[blk]);
            const long bits = check(blk, L, shifted);
            std::printf("block %d %2dx%d G%d %s x=%s m=%d mask bits=%ld\n", blk, xh, L.xw, g, L.t16 ? "16x16x32" : "32x32",
                        L.border_x ? "bordered" : "select", L.m, bits);
            ++n;
        }
    if (g_fail) {
        std::fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("ok %d instantiations\n", n);
    return 0;
}
