// Device-side Hamming distance of two 256-bit descriptors (16-byte aligned), shared by match_to_map.hip and map_merge.hip.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ int alva_hamming256_dev(const uint4 *a, const uint4 *b) {
    const uint4 a0 = a[0], a1 = a[1], b0 = b[0], b1 = b[1];
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) + __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) +
           __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}
