// Counter-based random numbers shared by the training-side kernels (augment.hip, and train_common.h's dropout keep).
#pragma once
#include <hip/hip_runtime.h>

namespace cough {
namespace {

// Philox4x32-10 (Salmon et al., SC'11): 128-bit counter c, 64-bit key k (the seed).  augment.hip counts (sample group, clip,
// 0, 0); the training steps count (unit group, clip, step offset lo, step offset hi).
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint2 k) {
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
        c = make_uint4(hi1 ^ c.y ^ k.x, lo1, hi0 ^ c.w ^ k.y, lo0);
        k.x += 0x9E3779B9u;
        k.y += 0xBB67AE85u;
    }
    return c;
}

}  // namespace
}  // namespace cough
