// Device-side pieces of the scene volume shared by mesh.hip (extraction), mesh_blocks.hip (extraction in blocks), mesh_raycast.hip
// (raycast) and mesh_color.hip (the colour sampler): X2 - X4 and X6 of alva_mesh_extract and the cell arithmetic of R3 of the raycast
// (include/alvaar_hip.h).  X2, X4 and X6 are integers only, X3's float is one written expression and R3's cell is single IEEE
// operations in the written order, so the same inputs give the same bits wherever they are inlined.
#pragma once
#include <hip/hip_runtime.h>

// X2: a cell's activity from its eight corners.  vs = the voxel strides along x, y, z in whatever array the caller keeps its voxels in;
// valid(o) / inside(o) = X1 of the voxel `o` array elements past the cell's minimum corner
template <class Valid, class Inside>
__device__ __forceinline__ bool mesh_cell_active_at(const int (&vs)[3], Valid valid, Inside inside) {
    bool all_valid = true;
    int n_in = 0;
#pragma unroll
    for (int c = 0; c < 8; c++) {
        const int o = (c & 1) * vs[0] + ((c >> 1) & 1) * vs[1] + (c >> 2) * vs[2];
        all_valid = all_valid && valid(o);
        n_in += inside(o) ? 1 : 0;
    }
    return all_valid && n_in > 0 && n_in < 8;
}

// X6: which of the three edges of the voxel at p (0 <= p < N per axis) emit a quad -- bit a = the edge p -> p + a, bit 3 = inside(p); 0 for
// an invalid voxel.  vs / cs = the strides of the caller's voxel and cell arrays; valid(o) / inside(o) = X1 of the voxel o elements past p,
// cell(o) = X2 of the cell o elements past p's own.  Nothing is asked of a voxel or a cell outside the grid
template <class Valid, class Inside, class Cell>
__device__ __forceinline__ int mesh_quad_mask(const int (&p)[3], int N, const int (&vs)[3], const int (&cs)[3], Valid valid, Inside inside, Cell cell) {
    if (!valid(0)) return 0;
    const bool in_v = inside(0);
    int mask = in_v ? 8 : 0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const int b = (a + 1) % 3, c = (a + 2) % 3;
        if (!(p[a] < N - 1 && p[b] >= 1 && p[b] < N - 1 && p[c] >= 1 && p[c] < N - 1)) continue;
        if (!valid(vs[a]) || inside(vs[a]) == in_v) continue;
        if (cell(-cs[b] - cs[c]) && cell(-cs[c]) && cell(0) && cell(-cs[b])) mask |= 1 << a;
    }
    return mask;
}

// X6's two triangles of one quad: Q0..Q3 the four cells' vertex indices, in_v = inside(v)
__device__ __forceinline__ void mesh_quad_triangles(int *t, bool in_v, int Q0, int Q1, int Q2, int Q3) {
    if (in_v) {
        t[0] = Q0; t[1] = Q1; t[2] = Q2; t[3] = Q0; t[4] = Q2; t[5] = Q3;
    } else {
        t[0] = Q0; t[1] = Q2; t[2] = Q1; t[3] = Q0; t[4] = Q3; t[5] = Q2;
    }
}

// X4: the gradient over a cell's eight corners, q[c] the corner (c & 1, (c >> 1) & 1, c >> 2); returns L2 = |g|^2
__device__ __forceinline__ long long mesh_cell_gradient(const int (&q)[8], int (&g)[3]) {
    g[0] = g[1] = g[2] = 0;
#pragma unroll
    for (int c = 0; c < 8; c++)
#pragma unroll
        for (int ax = 0; ax < 3; ax++) g[ax] += ((c >> ax) & 1) ? q[c] : -q[c];
    return ((long long) g[0] * g[0] + (long long) g[1] * g[1]) + (long long) g[2] * g[2];
}

// X3 and X4: the vertex and the normal of the active cell p from its eight corners' q (q[c] as for mesh_cell_gradient), o and voxel the
// volume's origin and voxel edge
__device__ __forceinline__ void mesh_cell_vertex(const int (&q)[8], const int (&p)[3], const double (&o)[3], double voxel, float (&vertex)[3],
                                                 float (&normal)[3]) {
    // X3
    int sum[3] = {0, 0, 0}, m = 0;
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int lo = 0; lo < 8; lo++) {
            if (lo & (1 << a)) continue;
            const int hi = lo | (1 << a);
            if ((q[lo] < 0) == (q[hi] < 0)) continue;
            const int qa = q[lo] < 0 ? -q[lo] : q[lo], qb = q[hi] < 0 ? -q[hi] : q[hi];
            const int D = qa + qb, f = (2048 * qa + D) / (2 * D);
#pragma unroll
            for (int ax = 0; ax < 3; ax++) sum[ax] += 1024 * (p[ax] + ((lo >> ax) & 1)) + (ax == a ? f : 0);
            m++;
        }
    // X4
    int g[3];
    const long long L2 = mesh_cell_gradient(q, g);
    const double len = sqrt((double) L2);
#pragma unroll
    for (int ax = 0; ax < 3; ax++) {
        const int X = (sum[ax] + m / 2) / m;
        vertex[ax] = (float) (o[ax] + ((double) X / 1024.0 + 0.5) * voxel);
        normal[ax] = L2 == 0 ? 0.f : (float) ((double) g[ax] / len);
    }
}

// a double clamped to lo..hi and converted; a NaN gives lo.  The clamp comes first: the conversion of what an int cannot hold is undefined
__device__ __forceinline__ int mesh_clamp_int(double v, int lo, int hi) { return v >= (double) hi ? hi : v >= (double) lo ? (int) v : lo; }

// R3's cell along one axis: from the continuous voxel coordinate g (0 at the centre of voxel 0) the lower corner ic in 0..N - 2 and the
// fraction f in 0..256 of the way to the upper one.  No index leaves the volume, whatever g
__device__ __forceinline__ void mesh_cell_axis(double g, int N, int &ic, int &f) {
    ic = mesh_clamp_int(floor(g), 0, N - 2);
    f = mesh_clamp_int(rint((g - (double) ic) * 256.0), 0, 256);
}
