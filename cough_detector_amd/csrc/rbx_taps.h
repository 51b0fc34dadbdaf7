// Which lanes of a fragment read of resblock_x3_kernel find their tap inside the image, and which zero cell the others
// read: plain host C++17 on top of resnet_plan.h (tests/rbx_tap_mask_check.cpp enumerates it for every instantiation).
//
// A lane's pixel depends on the tile and on the lane alone -- 16x16x32 body: R = 16 t + (lane & 15), 32x32x16 body:
// R = 32 t + (lane & 31) -- so whether tap (kh, kw) of that pixel lies inside the image is known when the kernel is
// compiled: one 64-bit lane mask per (operand, tile, tap).  The 16x16x32 body hands it to v_cndmask_b32 as a scalar
// register pair (resblock_x3.h: body16); no per-lane tap mask is computed on the vector unit.
#pragma once
#include "resnet_plan.h"

namespace cough {
namespace {

enum RbxOperand { RBX_OP_X = 0 /* conv1 (3x3 s2) and the projection (tap 4) over x */, RBX_OP_H = 1 /* conv2 (3x3 s1) over h */ };

// the workgroup's output pixel that lane `lane` owns in tile t (may be >= L.m: a padding row of the last tile)
constexpr int rbx_lane_pixel(const RbxGeo L, int t, int lane) { return L.t16 ? 16 * t + (lane & 15) : 32 * t + (lane & 31); }

// bit l: tap `tap` = 3 kh + kw of lane l's pixel of tile t lies inside the operand's image, and the pixel is one of the
// workgroup's M (a padding row reads zeros at every tap).  A pixel of the second clip takes its row and column from
// R % PER.
constexpr unsigned long long rbx_tap_mask(const RbxGeo L, int op, int t, int tap) {
    const int kh = tap / 3, kw = tap % 3;
    unsigned long long m = 0;
    for (int l = 0; l < 64; ++l) {
        const int R = rbx_lane_pixel(L, t, l);
        if (R >= L.m) continue;
        const int rem = R % L.per, oh = rem / L.ow, ow = rem % L.ow;
        const int ih = op == RBX_OP_X ? 2 * oh - 1 + kh : oh - 1 + kh, iw = op == RBX_OP_X ? 2 * ow - 1 + kw : ow - 1 + kw;
        const int nh = op == RBX_OP_X ? L.xh : L.oh, nw = op == RBX_OP_X ? L.xw : L.ow;
        if (ih >= 0 && ih < nh && iw >= 0 && iw < nw) m |= 1ull << l;
    }
    return m;
}

// 16x16x32 body: the cell of a zero row (16 cells at byte offset zrow, 256-B aligned) with bank residue `res` mod 16 cells
constexpr int rbx_zero_cell(int zrow, int res) { return zrow + (res & 15) * 16; }

// Byte offset, inside a plane, of the zero cell lane `lane` reads at the first k-step of a tap outside the image (planes
// without borders).  16x16x32 body: the cell of the zero row with the bank residue of the lane's in-image cell -- that
// depends on the lane and the tap, not on the tile: tiles are 16 cells apart, clips a multiple of 16.  32x32x16 body:
// the one zero cell of the lane's chunk plane.
constexpr int rbx_zero_x(const RbxGeo L, int lane, int tap) {
    if (!L.t16) return L.zx + (lane >> 5) * L.cpx;
    const int px = lane & 15, tq = lane >> 4;
    const int rx = px + (L.chi == 4 ? 0 : rbx_xoff(true, L.chi, L.cpx, tq) / 16);   // x planes with CIN = 64 are not 256-B aligned
    return rbx_zero_cell(L.zx, rx + rbx_x_tap(L.b01, L.b10, L.b11, L.ow, tap / 3, tap % 3));
}
constexpr int rbx_zero_h(const RbxGeo L, int lane, int tap) {
    if (!L.t16) return L.zh + (lane >> 5) * L.cph;
    const int px = lane & 15, tq = lane >> 4;
    return rbx_zero_cell(L.zh + tq * L.cph, px + rbx_h_tap(L.ow, tap / 3, tap % 3));
}

}  // namespace
}  // namespace cough
