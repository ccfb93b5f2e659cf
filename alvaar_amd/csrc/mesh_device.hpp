// Device-side pieces of the scene volume shared by mesh.hip (extraction), mesh_raycast.hip (raycast) and mesh_color.hip (the colour
// sampler): X4 of alva_mesh_extract and the cell arithmetic of R3 of the raycast (include/alvaar_hip.h).  X4 is integers only and R3's
// cell is single IEEE operations in the written order, so the same inputs give the same bits wherever they are inlined.
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

// a double clamped to lo..hi and converted; a NaN gives lo.  The clamp comes first: the conversion of what an int cannot hold is undefined
__device__ __forceinline__ int mesh_clamp_int(double v, int lo, int hi) { return v >= (double) hi ? hi : v >= (double) lo ? (int) v : lo; }

// R3's cell along one axis: from the continuous voxel coordinate g (0 at the centre of voxel 0) the lower corner ic in 0..N - 2 and the
// fraction f in 0..256 of the way to the upper one.  No index leaves the volume, whatever g
__device__ __forceinline__ void mesh_cell_axis(double g, int N, int &ic, int &f) {
    ic = mesh_clamp_int(floor(g), 0, N - 2);
    f = mesh_clamp_int(rint((g - (double) ic) * 256.0), 0, 256);
}
