// Device-side pieces of the scene volume shared by mesh.hip (extraction) and mesh_raycast.hip (raycast): X4 of alva_mesh_extract
// (include/alvaar_hip.h).  Integers only, so the same corners give the same bits wherever it is inlined.
#pragma once
#include <hip/hip_runtime.h>

// X4: the gradient over a cell's eight corners, q[c] the corner (c & 1, (c >> 1) & 1, c >> 2); returns L2 = |g|^2
__device__ __forceinline__ long long mesh_cell_gradient(const int (&q)[8], int (&g)[3]) {
    g[0] = g[1] = g[2] = 0;
#pragma unroll
    for (int c = 0; c < 8; c++)
#pragma unroll
        for (int ax = 0; ax < 3; ax++) g[ax] += ((c >> ax) & 1) ? q[c] : -q[c];
    return ((long long) g[0] * g[0] + (long long) g[1] * g[1]) + (long long) g[2] * g[2];
}
