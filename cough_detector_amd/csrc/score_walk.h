// The walking rule of the offline scorer, shared by score.hip (the sweep and the event list) and scenes.hip (the event
// matcher): both libraries decide whether a window fires with literally these functions, so a recording's matched
// detections number its sweep count.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>

namespace cough {

// ------------------------------------------------------------------------------------------ the walking rule
// `next` is the first window index allowed to fire: 0 at the start of a recording, j + gap after window j fired.
__device__ __forceinline__ bool walk_fires(double s, double threshold, long long k, long long next) {
    return s >= threshold && k >= next;               // false for a NaN on either side
}
__device__ __forceinline__ long long walk_advance(long long k, int gap) { return k + gap; }

// recording c's windows inside [0, n_windows), whatever the offsets hold
__device__ __forceinline__ void clip_windows(const long long* __restrict__ offs, int c, long long n_windows, long long& first,
                                             int& count) {
    const long long lo = min(max(offs[c], 0LL), n_windows);
    const long long hi = min(max(offs[c + 1], lo), n_windows);
    first = lo;
    count = int(min(hi - lo, (long long)INT_MAX));
}

// a float64 of lane `src` (wave-uniform) in every lane
__device__ __forceinline__ double read_lane(double v, int src) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), src);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
    return __hiloint2double(hi, lo);
}

}  // namespace cough
