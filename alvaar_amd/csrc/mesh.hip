// Scene mesh: depth images fused into a truncated signed distance volume (alva_mesh_integrate) and the volume's surface extracted as
// triangles (alva_mesh_extract) -- ARKit scene reconstruction (ARMeshGeometry), WebXR mesh-detection.  The reference has no counterpart,
// so the definitions in include/alvaar_hip.h (M1-M5, X1-X7) are pinned by the numpy restatement tests/mesh_cases.py.  Geometry is IEEE
// double in the written order (compile with -ffp-contract=off), every decision is made on integers or on single IEEE comparisons, and
// every sum whose order is not fixed is an integer sum, so the same inputs give the same bits.
//
// alva_mesh_integrate, one launch:
//   k_mesh_integrate  one thread per voxel and step, i on the lanes (the loads and stores of a wave are contiguous), at most 2048
//                     workgroups that stride over the volume; nothing but the thread's own voxels is written, the five counts go per
//                     thread, per wave, per workgroup, then one integer atomicAdd per workgroup and count.  alva_mesh_integrate_color is
//                     the same body with a compile-time flag: M1 - M4 exist once, the colour voxel is one more 32-bit load and store
//                     per lane and there is a sixth count
// alva_mesh_extract, five launches over the N^3 indices (k N + j) N + i, which are the voxels and -- for i, j, k < N - 1 -- the cells: both
// orders of X5 and X6 are ascending in that one index, so a rank is a prefix count along it.  A workgroup is 256 consecutive indices:
//   k_mesh_classify   per index: the voxel's validity and side, the cell's activity from its eight corners; the activity of a wave's 64
//                     cells is one ballot word; per workgroup the counts of active cells, valid and inside voxels
//   k_mesh_quads      per voxel: which of its three edges emit a quad (the ends from the volume, the four cells from the ballot words);
//                     per workgroup the count of quads
//   k_mesh_scan       one workgroup: the exclusive scan of the workgroups' two counts, the totals, the code
//   k_mesh_vertices   per active cell: its rank from the scanned count and the ballot words, the vertex and the normal
//   k_mesh_triangles  per emitting voxel: its quads' place from the scanned count, the four cells' ranks, two triangles per quad
// No workgroup waits for another: what one launch needs of all workgroups of the one before comes from the stream's order.
// The bodies of X2, X3 / X4, X6 and the winding are in mesh_device.hpp, over an accessor for "the voxel / cell o elements from here":
// mesh_blocks.hip runs the same ones on a block's box in LDS.
#include "common.hpp"
#include "camera_device.hpp"
#include "mesh_device.hpp"
#include "wave_utils.hpp"
#include <cmath>

namespace {

constexpr int MESH_SCRATCH_SLOT = 9;   // (shared with the other synchronous stages)
constexpr int MESH_N_MIN = 4, MESH_N_MAX = 256;
constexpr int MESH_INTEGRATE_GRID = 2048;   // workgroups at most: 8 per CU

// ---------------------------------------------------------------------------------------------------------------------- integrate
struct IntegrateArgs {
    int16_t *q;
    uint8_t *w;
    int N;
    double o[3], voxel, trunc;
    double R[9], t[3];   // X_cam = R X_world + t
    AlvaCam cam;
    int step, gw, gh;
    const float *depth;
    const uint8_t *conf, *code;
    int w_max;
    int *counts;   // updated, hidden, free, outside, no depth, coloured
    // alva_mesh_integrate_color only (K1 - K3)
    uint32_t *c;             // [N^3]: r | g << 8 | b << 16 | wc << 24
    const uint32_t *thumb;   // [th][tw], the same bytes
    int cstep, tw, th;
};

// one voxel: M1 - M5, and with COLOR K1 - K3.  Returns 0 updated, 1 hidden, 3 outside, 4 no depth; is_free and colored are set with 0
template <bool COLOR>
__device__ __forceinline__ int mesh_integrate_voxel(const IntegrateArgs &A, int idx, int &is_free, int &colored) {
    const int i = idx % A.N, j = (idx / A.N) % A.N, k = idx / (A.N * A.N);
    // M1
    const double x = A.o[0] + ((double) i + 0.5) * A.voxel;
    const double y = A.o[1] + ((double) j + 0.5) * A.voxel;
    const double z = A.o[2] + ((double) k + 0.5) * A.voxel;
    const double Px = ((A.R[0] * x + A.R[1] * y) + A.R[2] * z) + A.t[0];
    const double Py = ((A.R[3] * x + A.R[4] * y) + A.R[5] * z) + A.t[1];
    const double Pz = ((A.R[6] * x + A.R[7] * y) + A.R[8] * z) + A.t[2];
    if (!(Pz > 1e-9)) return 3;
    // M2
    float up, vp;
    alva_project_dist_dev(A.cam, Px, Py, Pz, up, vp);
    const float fu = floorf(up), fv = floorf(vp);
    if (!(0.f <= fu && fu < (float) (A.gw * A.step) && 0.f <= fv && fv < (float) (A.gh * A.step))) return 3;   // (a NaN fails every comparison)
    const int c = ((int) fv / A.step) * A.gw + (int) fu / A.step;
    // M3
    const float d = A.depth[c];
    if (!(A.code[c] == 0 && d > 0.f)) return 4;
    int w_m = (int) A.conf[c] >> 3;
    w_m = w_m > 1 ? w_m : 1;
    // M4
    const double s = (double) d - Pz;
    if (s < -A.trunc) return 1;
    const double t = s / A.trunc;
    int q_m = 32767;
    if (t >= 1.0) is_free = 1;
    else q_m = (int) rint(t * 32767.0);
    // M5
    const int q0 = A.q[idx], w0 = A.w[idx];
    const int a = q0 * w0 + q_m * w_m, S = w0 + w_m;
    const int num = 2 * a + S, den = 2 * S;
    int qn = num / den;
    if (num % den != 0 && num < 0) qn--;   // a true floor: C++ division truncates
    A.q[idx] = (int16_t) qn;
    A.w[idx] = (uint8_t) (S < A.w_max ? S : A.w_max);
    if constexpr (COLOR) {
        // K1 (fu, fv >= 0 here, so the quotients are too)
        const int tx = (int) fu / A.cstep, ty = (int) fv / A.cstep;
        if (!is_free && tx < A.tw && ty < A.th) {
            // K2, K3: one 32-bit load of the voxel, one of the thumbnail's cell, one 32-bit store
            const uint32_t m = A.thumb[ty * A.tw + tx], c0 = A.c[idx];
            const int wc = (int) (c0 >> 24), Sc = wc + w_m;
            uint32_t cn = (uint32_t) (Sc < A.w_max ? Sc : A.w_max) << 24;
#pragma unroll
            for (int ch = 0; ch < 3; ch++) {
                const int v0 = (int) ((c0 >> (8 * ch)) & 255u), vm = (int) ((m >> (8 * ch)) & 255u);
                cn |= (uint32_t) ((2 * (v0 * wc + vm * w_m) + Sc) / (2 * Sc)) << (8 * ch);   // a weighted mean of two bytes: <= 255
            }
            A.c[idx] = cn;
            colored = 1;
        }
    }
    return 0;
}

// A workgroup takes 256 consecutive voxels at a time, gridDim.x * 256 apart, and adds its counts up in registers: the atomic sums
// are one per workgroup, not one per wave -- all of them land on the same few words, and with a workgroup per 256 voxels and an atomic
// per wave they, not the voxels, were the launch's time (measured on an MI355X: 110 us at N = 64 and 760 us at N = 128, about 5 ns per
// atomic, against 19 and 34 us in this form).  COLOR: alva_mesh_integrate_color, with the sixth count
template <bool COLOR>
__global__ void __launch_bounds__(256) k_mesh_integrate(const IntegrateArgs A) {
    constexpr int NC = COLOR ? 6 : 5;
    __shared__ int s_n[4][NC];
    const int V = A.N * A.N * A.N;
    int n[NC];   // updated, hidden, free, outside, no depth, coloured
#pragma unroll
    for (int c = 0; c < NC; c++) n[c] = 0;
    for (int base = blockIdx.x * 256; base < V; base += gridDim.x * 256) {
        const int idx = base + threadIdx.x;
        if (idx >= V) continue;
        int is_free = 0, colored = 0;
        const int cat = mesh_integrate_voxel<COLOR>(A, idx, is_free, colored);
        n[0] += cat == 0;
        n[1] += cat == 1;
        n[2] += is_free;
        n[3] += cat == 3;
        n[4] += cat == 4;
        if constexpr (COLOR) n[5] += colored;
    }
    // (integers: the order of the additions does not matter)
#pragma unroll
    for (int c = 0; c < NC; c++) {
        const int v = wave_sum(n[c]);
        if ((threadIdx.x & 63) == 0) s_n[threadIdx.x >> 6][c] = v;
    }
    __syncthreads();
    if (threadIdx.x < NC) {
        const int v = (s_n[0][threadIdx.x] + s_n[1][threadIdx.x]) + (s_n[2][threadIdx.x] + s_n[3][threadIdx.x]);
        if (v) atomicAdd(&A.counts[threadIdx.x], v);
    }
}

// ---------------------------------------------------------------------------------------------------------------------- extract
struct ExtractArgs {
    const int16_t *q;
    const uint8_t *w;
    int N, n_blocks;
    double o[3], voxel;
    int min_weight, max_vertices, max_triangles;
    unsigned long long *bits;   // [4 n_blocks]: bit l of word W = the cell of index 64 W + l is active
    uint8_t *fmask;             // [256 n_blocks]: bit a = the edge v -> v + a emits a quad, bit 3 = inside(v)
    int *vsum, *fsum;           // [n_blocks]: the workgroup's active cells / quads; after the scan, those of the workgroups before it
    int *nvalid, *ninside;      // [n_blocks]
    int *info;                  // [8] on the device
    float *vertices, *normals;
    int *triangles;
};

// the sum of v over the workgroup's four waves, delivered to every thread
__device__ __forceinline__ int block_sum_256(int v, int *s4) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
    __syncthreads();
    const int r = (s4[0] + s4[1]) + (s4[2] + s4[3]);
    __syncthreads();
    return r;
}

__global__ void __launch_bounds__(256) k_mesh_classify(const ExtractArgs A) {
    __shared__ int s4[4];
    const int N = A.N, idx = blockIdx.x * 256 + threadIdx.x;
    bool valid = false, inside = false, active = false;
    if (idx < N * N * N) {
        const int i = idx % N, j = (idx / N) % N, k = idx / (N * N);
        // X1
        valid = A.w[idx] >= A.min_weight;
        inside = A.q[idx] < 0;
        // X2
        if (i < N - 1 && j < N - 1 && k < N - 1) {
            const int vs[3] = {1, N, N * N};
            active = mesh_cell_active_at(
                vs, [&](int o) { return A.w[idx + o] >= A.min_weight; }, [&](int o) { return A.q[idx + o] < 0; });
        }
    }
    const unsigned long long word = __ballot(active);
    if ((threadIdx.x & 63) == 0) A.bits[idx >> 6] = word;
    const int nv = block_sum_256(active ? 1 : 0, s4), na = block_sum_256(valid ? 1 : 0, s4), ni = block_sum_256(valid && inside ? 1 : 0, s4);
    if (threadIdx.x == 0) {
        A.vsum[blockIdx.x] = nv;
        A.nvalid[blockIdx.x] = na;
        A.ninside[blockIdx.x] = ni;
    }
}

__device__ __forceinline__ bool mesh_cell_active(const ExtractArgs &A, int L) { return (A.bits[L >> 6] >> (L & 63)) & 1ull; }

__global__ void __launch_bounds__(256) k_mesh_quads(const ExtractArgs A) {
    __shared__ int s4[4];
    const int N = A.N, idx = blockIdx.x * 256 + threadIdx.x;
    int mask = 0;
    if (idx < N * N * N) {
        const int p[3] = {idx % N, (idx / N) % N, idx / (N * N)};
        const int stride[3] = {1, N, N * N};
        // X6
        mask = mesh_quad_mask(
            p, N, stride, stride, [&](int o) { return A.w[idx + o] >= A.min_weight; }, [&](int o) { return A.q[idx + o] < 0; },
            [&](int o) { return mesh_cell_active(A, idx + o); });
    }
    A.fmask[idx] = (uint8_t) mask;   // (the array covers every thread of the grid)
    const int nq = block_sum_256(__popc(mask & 7), s4);
    if (threadIdx.x == 0) A.fsum[blockIdx.x] = nq;
}

// the exclusive scan of one value per thread over a workgroup of 1024; total = the sum of all
__device__ __forceinline__ int block_excl_scan_1024(int v, int *s16, int &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    if (lane == 63) s16[wave] = x;
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int u = 0; u < 16; u++) {
        base += u < wave ? s16[u] : 0;
        total += s16[u];
    }
    __syncthreads();
    return base + x - v;
}

__global__ void __launch_bounds__(1024) k_mesh_scan(const ExtractArgs A) {
    __shared__ int s16[16];
    const int n = A.n_blocks, per = (n + 1023) / 1024;
    const int b0 = threadIdx.x * per, b1 = b0 + per < n ? b0 + per : n;
    int sv = 0, sf = 0, sa = 0, si = 0;
    for (int b = b0; b < b1; b++) {
        sv += A.vsum[b];
        sf += A.fsum[b];
        sa += A.nvalid[b];
        si += A.ninside[b];
    }
    int tv, tf, ta, ti;
    int ov = block_excl_scan_1024(sv, s16, tv), of = block_excl_scan_1024(sf, s16, tf);
    (void) block_excl_scan_1024(sa, s16, ta);
    (void) block_excl_scan_1024(si, s16, ti);
    for (int b = b0; b < b1; b++) {
        const int cv = A.vsum[b], cf = A.fsum[b];
        A.vsum[b] = ov;
        A.fsum[b] = of;
        ov += cv;
        of += cf;
    }
    if (threadIdx.x == 0) {
        // X7
        A.info[0] = tv > A.max_vertices || 2 * tf > A.max_triangles ? 3 : tv == 0 ? 1 : 0;
        A.info[1] = tv;
        A.info[2] = 2 * tf;
        A.info[3] = ta;
        A.info[4] = ti;
        A.info[5] = A.N;
        A.info[6] = 0;
        A.info[7] = 0;
    }
}

// X5: the number of active cells of a lower index
__device__ __forceinline__ int mesh_cell_rank(const ExtractArgs &A, int L) {
    const int blk = L >> 8, wv = (L >> 6) & 3;
    int r = A.vsum[blk];
    for (int u = 0; u < wv; u++) r += __popcll(A.bits[4 * blk + u]);
    return r + __popcll(A.bits[L >> 6] & ((1ull << (L & 63)) - 1ull));
}

__global__ void __launch_bounds__(256) k_mesh_vertices(const ExtractArgs A) {
    if (A.info[0] == 3) return;
    const int N = A.N, idx = blockIdx.x * 256 + threadIdx.x;
    if (!mesh_cell_active(A, idx)) return;   // (the words cover every thread of the grid)
    const int rank = mesh_cell_rank(A, idx);
    const int p[3] = {idx % N, (idx / N) % N, idx / (N * N)};
    int q[8];
#pragma unroll
    for (int c = 0; c < 8; c++) q[c] = A.q[idx + (c & 1) + ((c >> 1) & 1) * N + (c >> 2) * N * N];
    // X3, X4
    float v[3], n[3];
    mesh_cell_vertex(q, p, A.o, A.voxel, v, n);
#pragma unroll
    for (int ax = 0; ax < 3; ax++) {
        A.vertices[3 * (size_t) rank + ax] = v[ax];
        A.normals[3 * (size_t) rank + ax] = n[ax];
    }
}

__global__ void __launch_bounds__(256) k_mesh_triangles(const ExtractArgs A) {
    __shared__ int s4[4];
    if (A.info[0] == 3) return;
    const int N = A.N, idx = blockIdx.x * 256 + threadIdx.x;
    const int mask = A.fmask[idx], lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // the quads of the lower threads of the workgroup: of the lower lanes by ballots, of the lower waves through LDS
    const unsigned long long lt = (1ull << lane) - 1ull;
    const unsigned long long b0 = __ballot(mask & 1), b1 = __ballot(mask & 2), b2 = __ballot(mask & 4);
    if (lane == 0) s4[wave] = __popcll(b0) + __popcll(b1) + __popcll(b2);
    __syncthreads();
    if (!(mask & 7)) return;
    int quad = A.fsum[blockIdx.x] + __popcll(b0 & lt) + __popcll(b1 & lt) + __popcll(b2 & lt);
    for (int u = 0; u < wave; u++) quad += s4[u];
    const int stride[3] = {1, N, N * N};
#pragma unroll
    for (int a = 0; a < 3; a++) {
        if (!(mask & (1 << a))) continue;
        const int sb = stride[(a + 1) % 3], sc = stride[(a + 2) % 3];
        const int Q0 = mesh_cell_rank(A, idx - sb - sc), Q1 = mesh_cell_rank(A, idx - sc), Q2 = mesh_cell_rank(A, idx),
                  Q3 = mesh_cell_rank(A, idx - sb);
        int *t = A.triangles + 6 * (size_t) quad;
        mesh_quad_triangles(t, (mask & 8) != 0, Q0, Q1, Q2, Q3);
        quad++;
    }
}

}  // namespace

// alva_mesh_integrate (d_c null) and alva_mesh_integrate_color: the same checks, the same launch but for the kernel's flag
static int mesh_integrate_run(alva_ctx *ctx, int16_t *d_q, uint8_t *d_w, uint8_t *d_c, int N, const double *h_origin3, double voxel, double trunc,
                              const double *h_T_cw12, const double *h_calib8, int width, int height, int step, const float *d_depth,
                              const uint8_t *d_conf, const uint8_t *d_code, const uint8_t *d_thumb, int cstep, int w_max, int *h_info8) {
    ALVA_ARG(ctx && d_q && d_w && h_origin3 && h_T_cw12 && h_calib8 && d_depth && d_conf && d_code && h_info8);
    ALVA_ARG(N >= MESH_N_MIN && N <= MESH_N_MAX);
    ALVA_ARG(std::isfinite(voxel) && voxel > 0 && std::isfinite(trunc) && trunc > 0);
    ALVA_ARG(width >= 1 && height >= 1 && width <= 16384 && height <= 16384);
    ALVA_ARG(step >= 1 && step <= 16 && width / step >= 1 && height / step >= 1);
    ALVA_ARG(w_max >= 1 && w_max <= 255);
    for (int i = 0; i < 3; i++) ALVA_ARG(std::isfinite(h_origin3[i]));
    for (int i = 0; i < 8; i++) ALVA_ARG(std::isfinite(h_calib8[i]));
    for (int i = 0; i < 12; i++) ALVA_ARG(std::isfinite(h_T_cw12[i]));
    ALVA_ARG(h_calib8[0] > 0 && h_calib8[1] > 0);
    IntegrateArgs A{};
    if (d_c) {
        ALVA_ARG(d_thumb && ((uintptr_t) d_c % 4) == 0 && ((uintptr_t) d_thumb % 4) == 0);
        ALVA_ARG(cstep >= 1 && cstep <= 16 && width / cstep >= 1 && height / cstep >= 1);
        A.c = (uint32_t *) d_c; A.thumb = (const uint32_t *) d_thumb;
        A.cstep = cstep; A.tw = width / cstep; A.th = height / cstep;
    }
    A.q = d_q; A.w = d_w; A.N = N;
    memcpy(A.o, h_origin3, sizeof(A.o));
    A.voxel = voxel; A.trunc = trunc;
    memcpy(A.R, h_T_cw12, sizeof(A.R));
    memcpy(A.t, h_T_cw12 + 9, sizeof(A.t));
    A.cam = AlvaCam{h_calib8[0], h_calib8[1], h_calib8[2], h_calib8[3], h_calib8[4], h_calib8[5], h_calib8[6], h_calib8[7]};
    A.step = step; A.gw = width / step; A.gh = height / step;
    A.depth = d_depth; A.conf = d_conf; A.code = d_code;
    A.w_max = w_max;
    int *pin = nullptr;
    int rc = alva_ctx_pinned(ctx, 64 * sizeof(int), (void **) &pin);
    if (rc) return rc;
    uint8_t *scr = nullptr;
    rc = alva_ctx_scratch(ctx, MESH_SCRATCH_SLOT, 256, (void **) &scr);
    if (rc) return rc;
    A.counts = (int *) scr;
    ALVA_HIP(hipMemsetAsync(A.counts, 0, 8 * sizeof(int), ctx->stream));
    const int blocks = alva_divup(N * N * N, 256), grid = blocks < MESH_INTEGRATE_GRID ? blocks : MESH_INTEGRATE_GRID;
    if (d_c) hipLaunchKernelGGL(k_mesh_integrate<true>, dim3(grid), dim3(256), 0, ctx->stream, A);
    else hipLaunchKernelGGL(k_mesh_integrate<false>, dim3(grid), dim3(256), 0, ctx->stream, A);
    ALVA_LAUNCH_CHECK();
    ALVA_HIP(hipMemcpyAsync(pin + 32, A.counts, 6 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    ALVA_HIP(alva_stream_sync(ctx->stream));
    memcpy(h_info8, pin + 32, 5 * sizeof(int));
    h_info8[5] = N;
    h_info8[6] = pin[32 + 5];   // (zero without colour: nothing adds to it)
    h_info8[7] = 0;
    return ALVA_OK;
}

extern "C" int alva_mesh_integrate(alva_ctx *ctx, int16_t *d_q, uint8_t *d_w, int N, const double *h_origin3, double voxel, double trunc,
                                   const double *h_T_cw12, const double *h_calib8, int width, int height, int step, const float *d_depth,
                                   const uint8_t *d_conf, const uint8_t *d_code, int w_max, int *h_info8) {
    return mesh_integrate_run(ctx, d_q, d_w, nullptr, N, h_origin3, voxel, trunc, h_T_cw12, h_calib8, width, height, step, d_depth, d_conf, d_code,
                              nullptr, 0, w_max, h_info8);
}

extern "C" int alva_mesh_integrate_color(alva_ctx *ctx, int16_t *d_q, uint8_t *d_w, uint8_t *d_c, int N, const double *h_origin3, double voxel,
                                         double trunc, const double *h_T_cw12, const double *h_calib8, int width, int height, int step,
                                         const float *d_depth, const uint8_t *d_conf, const uint8_t *d_code, const uint8_t *d_thumb, int cstep,
                                         int w_max, int *h_info8) {
    ALVA_ARG(d_c);
    return mesh_integrate_run(ctx, d_q, d_w, d_c, N, h_origin3, voxel, trunc, h_T_cw12, h_calib8, width, height, step, d_depth, d_conf, d_code,
                              d_thumb, cstep, w_max, h_info8);
}

extern "C" int alva_mesh_extract(alva_ctx *ctx, const int16_t *d_q, const uint8_t *d_w, int N, const double *h_origin3, double voxel,
                                 int min_weight, int max_vertices, int max_triangles, float *d_vertices, float *d_normals, int *d_triangles,
                                 int *h_info8) {
    ALVA_ARG(ctx && d_q && d_w && h_origin3 && d_vertices && d_normals && d_triangles && h_info8);
    ALVA_ARG(N >= MESH_N_MIN && N <= MESH_N_MAX);
    ALVA_ARG(std::isfinite(voxel) && voxel > 0);
    ALVA_ARG(min_weight >= 1 && min_weight <= 255 && max_vertices >= 1 && max_triangles >= 1);
    for (int i = 0; i < 3; i++) ALVA_ARG(std::isfinite(h_origin3[i]));
    ExtractArgs A{};
    A.q = d_q; A.w = d_w; A.N = N;
    A.n_blocks = alva_divup(N * N * N, 256);
    memcpy(A.o, h_origin3, sizeof(A.o));
    A.voxel = voxel;
    A.min_weight = min_weight; A.max_vertices = max_vertices; A.max_triangles = max_triangles;
    A.vertices = d_vertices; A.normals = d_normals; A.triangles = d_triangles;
    const size_t nb = (size_t) A.n_blocks;
    const size_t off_bits = 256, off_sums = off_bits + nb * 4 * sizeof(unsigned long long), off_fmask = off_sums + nb * 4 * sizeof(int);
    int *pin = nullptr;
    int rc = alva_ctx_pinned(ctx, 64 * sizeof(int), (void **) &pin);
    if (rc) return rc;
    uint8_t *scr = nullptr;
    rc = alva_ctx_scratch(ctx, MESH_SCRATCH_SLOT, off_fmask + nb * 256, (void **) &scr);
    if (rc) return rc;
    A.info = (int *) scr;
    A.bits = (unsigned long long *) (scr + off_bits);
    A.vsum = (int *) (scr + off_sums);
    A.fsum = A.vsum + nb;
    A.nvalid = A.fsum + nb;
    A.ninside = A.nvalid + nb;
    A.fmask = scr + off_fmask;
    hipLaunchKernelGGL(k_mesh_classify, dim3(A.n_blocks), dim3(256), 0, ctx->stream, A);
    ALVA_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mesh_quads, dim3(A.n_blocks), dim3(256), 0, ctx->stream, A);
    ALVA_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mesh_scan, dim3(1), dim3(1024), 0, ctx->stream, A);
    ALVA_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mesh_vertices, dim3(A.n_blocks), dim3(256), 0, ctx->stream, A);
    ALVA_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mesh_triangles, dim3(A.n_blocks), dim3(256), 0, ctx->stream, A);
    ALVA_LAUNCH_CHECK();
    ALVA_HIP(hipMemcpyAsync(pin + 40, A.info, 8 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    ALVA_HIP(alva_stream_sync(ctx->stream));
    memcpy(h_info8, pin + 40, 8 * sizeof(int));
    return ALVA_OK;
}
