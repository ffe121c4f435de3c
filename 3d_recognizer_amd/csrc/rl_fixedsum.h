// The fixed-order fp64 sum shared by boxes.hip and outliers.hip (the numpy twin is randlanet/utils/boxes.py: fixed_sums): the
// terms of one id in chunks of FS_CHUNK = 64 * FS_TURNS consecutive members, lane l of the chunk's wavefront adding members
// l, l + 64, .. in turn from 0.0, the 64 lane sums folded in halves, and the chunk sums of the id through the same two steps
// once more.  Here: the two constants and the fold; the loads around them belong to the kernels.
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr int FS_TURNS = 16;                 // terms a lane adds per chunk (TURNS of utils/boxes.py)
constexpr int FS_CHUNK = 64 * FS_TURNS;      // members per chunk (CHUNK of utils/boxes.py)

// the 64 lane sums folded in halves by six xor-shuffles; lane 0 (every lane, in fact) ends with the chunk's sum
__device__ __forceinline__ double fs_fold64(double v) {
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) v = v + __shfl_xor(v, h, 64);      // lane l < h: s_l + s_(l + h)
    return v;
}

}  // namespace
