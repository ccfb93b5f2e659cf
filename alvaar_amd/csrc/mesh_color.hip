// Mesh colour, the two stages that are not the integration (that one is k_mesh_integrate's colour instantiation, mesh.hip): the frame's
// colour reduced to a thumbnail (alva_color_thumb, T1) and the colour volume sampled at world points (alva_mesh_color_at, A0-A4).  The
// reference has no counterpart, so the definitions in include/alvaar_hip.h are pinned by the numpy restatement tests/mesh_color_cases.py.
// The thumbnail is integers only; the sampler's geometry is IEEE double in the written order (compile with -ffp-contract=off) up to the
// cell and its fractions -- R3's, one body with the raycast (mesh_device.hpp) -- and integers from there, so the same inputs give the
// same bits.
//
//   k_color_thumb    one thread per thumbnail cell, tx on the lanes: a wave reads 64 cstep consecutive pixels of a row at a time, one
//                    32-bit load per pixel, and writes 64 consecutive 32-bit cells.  Nothing past tw cstep / th cstep is read.  With a
//                    completion word (the session's per-frame call) the workgroups count their arrivals and the last one publishes it
//   k_mesh_color_at  one lane per point, 256 per workgroup: eight 32-bit loads of colour voxels, every index clamped into the volume
//                    before it is used; the four counts per lane, per wave, per workgroup, then one integer atomicAdd each
#include "common.hpp"
#include "mesh_device.hpp"
#include "wave_utils.hpp"
#include <cmath>

namespace {

constexpr int CA_SCRATCH_SLOT = 9;   // (shared with the other synchronous stages)
constexpr int CA_N_MIN = 4, CA_N_MAX = 256;
constexpr int CA_MAX_POINTS = 1 << 20;

// ---------------------------------------------------------------------------------------------------------------------- thumbnail
struct ThumbArgs {
    const uint8_t *rgba;
    size_t pitch;
    int cstep, tw, th;
    uint32_t *thumb;      // [th][tw]: r | g << 8 | b << 16 | 255 << 24
    unsigned *arrivals;   // with `done`: a device word, zero between launches
    unsigned *done;       // pinned: receives seq when every workgroup has read its pixels; or null
    unsigned seq;
};

__global__ void __launch_bounds__(256) k_color_thumb(const ThumbArgs A) {
    const int tx = blockIdx.x * 64 + threadIdx.x, ty = blockIdx.y * 4 + threadIdx.y;
    if (tx < A.tw && ty < A.th) {
        // T1
        unsigned sum[3] = {0, 0, 0};
        for (int dy = 0; dy < A.cstep; dy++) {
            const uint32_t *row = (const uint32_t *) (A.rgba + (size_t) (ty * A.cstep + dy) * A.pitch) + tx * A.cstep;
            for (int dx = 0; dx < A.cstep; dx++) {
                const uint32_t p = row[dx];   // (the alpha byte comes with the word and is dropped)
                sum[0] += p & 255u;
                sum[1] += (p >> 8) & 255u;
                sum[2] += (p >> 16) & 255u;
            }
        }
        const unsigned n = (unsigned) (A.cstep * A.cstep);
        A.thumb[(size_t) ty * A.tw + tx] = (2 * sum[0] + n) / (2 * n) | ((2 * sum[1] + n) / (2 * n)) << 8 | ((2 * sum[2] + n) / (2 * n)) << 16 | 255u << 24;
    }
    if (A.done) {   // every store above needed its loads: a workgroup that arrives has read its pixels
        __syncthreads();
        if (threadIdx.x == 0 && threadIdx.y == 0) {
            __threadfence();
            if (atomicAdd(A.arrivals, 1u) == gridDim.x * gridDim.y - 1) {
                __hip_atomic_store(A.arrivals, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(A.done, A.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------- colour at
struct ColorAtArgs {
    const uint32_t *c;   // [N^3]: r | g << 8 | b << 16 | wc << 24
    int N, n;
    double o[3], voxel;
    const float *points;
    uint32_t *rgba;
    uint8_t *code;
    int *counts;   // codes 0, 1, 2, 4
};

// A0 - A4 for one point: the code, and the colour r | g << 8 | b << 16 | 255 << 24 (zero unless the code is 0)
__device__ __forceinline__ int mesh_color_at_point(const ColorAtArgs &A, const float (&p)[3], uint32_t &out) {
    out = 0;
    const int N = A.N;
    // A0 (a NaN fails the comparison)
    if (!(fabsf(p[0]) <= 3.4028234663852886e38f && fabsf(p[1]) <= 3.4028234663852886e38f && fabsf(p[2]) <= 3.4028234663852886e38f)) return 4;
    // A1, A2
    int ic[3], f[3];
    bool in = true;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const double g = ((double) p[a] - A.o[a]) / A.voxel - 0.5;
        in = in && 0.0 <= g && g <= (double) (N - 1);
        mesh_cell_axis(g, N, ic[a], f[a]);
    }
    if (!in) return 1;
    // A3 (integers: the order of the sums does not matter)
    const int base = (ic[2] * N + ic[1]) * N + ic[0];   // 0 <= base and base + N N + N + 1 <= N^3 - 1: ic <= N - 2
    long long S = 0, sum[3] = {0, 0, 0};
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const uint32_t v = A.c[base + (k & 1) + ((k >> 1) & 1) * N + (k >> 2) * N * N];
        const int wx = (k & 1) ? f[0] : 256 - f[0], wy = (k & 2) ? f[1] : 256 - f[1], wz = (k & 4) ? f[2] : 256 - f[2];
        const long long Wt = (long long) (wx * wy) * (long long) (wz * (int) (v >> 24));
        S += Wt;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) sum[ch] += (long long) ((v >> (8 * ch)) & 255u) * Wt;
    }
    if (S == 0) return 2;
    // A4
    out = 255u << 24;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) out |= (uint32_t) ((2 * sum[ch] + S) / (2 * S)) << (8 * ch);
    return 0;
}

__global__ void __launch_bounds__(256) k_mesh_color_at(const ColorAtArgs A) {
    __shared__ int s_n[4][4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    int cnt[4] = {0, 0, 0, 0};   // codes 0, 1, 2, 4
    if (i < A.n) {
        const float p[3] = {A.points[3 * (size_t) i], A.points[3 * (size_t) i + 1], A.points[3 * (size_t) i + 2]};
        uint32_t out;
        const int code = mesh_color_at_point(A, p, out);
        A.rgba[i] = out;
        A.code[i] = (uint8_t) code;
        cnt[0] = code == 0;
        cnt[1] = code == 1;
        cnt[2] = code == 2;
        cnt[3] = code == 4;
    }
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const int v = wave_sum(cnt[c]);
        if ((threadIdx.x & 63) == 0) s_n[threadIdx.x >> 6][c] = v;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int v = (s_n[0][threadIdx.x] + s_n[1][threadIdx.x]) + (s_n[2][threadIdx.x] + s_n[3][threadIdx.x]);
        if (v) atomicAdd(&A.counts[threadIdx.x], v);
    }
}

}  // namespace

int alva_color_thumb_done(alva_ctx *ctx, const uint8_t *d_rgba, size_t pitch, int width, int height, int cstep, uint8_t *d_thumb,
                          uint32_t *d_arrivals, uint32_t *h_done, uint32_t seq) {
    ALVA_ARG(ctx && d_rgba && d_thumb && ((uintptr_t) d_rgba % 4) == 0 && pitch % 4 == 0 && ((uintptr_t) d_thumb % 4) == 0);
    ALVA_ARG(width >= 1 && height >= 1 && width <= 16384 && height <= 16384 && pitch >= (size_t) width * 4);
    ALVA_ARG(cstep >= 1 && cstep <= 16 && width / cstep >= 1 && height / cstep >= 1);
    ALVA_ARG(!h_done || d_arrivals);
    ThumbArgs A{};
    A.rgba = d_rgba; A.pitch = pitch; A.cstep = cstep; A.tw = width / cstep; A.th = height / cstep;
    A.thumb = (uint32_t *) d_thumb;
    A.arrivals = d_arrivals; A.done = h_done; A.seq = seq;
    hipLaunchKernelGGL(k_color_thumb, dim3(alva_divup(A.tw, 64), alva_divup(A.th, 4)), dim3(64, 4), 0, ctx->stream, A);
    ALVA_LAUNCH_CHECK();
    return ALVA_OK;
}

extern "C" int alva_color_thumb(alva_ctx *ctx, const uint8_t *d_rgba, size_t pitch, int width, int height, int cstep, uint8_t *d_thumb) {
    return alva_color_thumb_done(ctx, d_rgba, pitch, width, height, cstep, d_thumb, nullptr, nullptr, 0);
}

extern "C" int alva_mesh_color_at(alva_ctx *ctx, const uint8_t *d_c, int N, const double *h_origin3, double voxel, int n, const float *d_points3,
                                  uint8_t *d_rgba, uint8_t *d_code, int *h_info8) {
    ALVA_ARG(ctx && d_c && h_origin3 && d_points3 && d_rgba && d_code && h_info8);
    ALVA_ARG(((uintptr_t) d_c % 4) == 0 && ((uintptr_t) d_rgba % 4) == 0);
    ALVA_ARG(N >= CA_N_MIN && N <= CA_N_MAX);
    ALVA_ARG(std::isfinite(voxel) && voxel > 0);
    ALVA_ARG(n >= 1 && n <= CA_MAX_POINTS);
    for (int i = 0; i < 3; i++) ALVA_ARG(std::isfinite(h_origin3[i]));
    ColorAtArgs A{};
    A.c = (const uint32_t *) d_c; A.N = N; A.n = n;
    memcpy(A.o, h_origin3, sizeof(A.o));
    A.voxel = voxel;
    A.points = d_points3; A.rgba = (uint32_t *) d_rgba; A.code = d_code;
    int *pin = nullptr;
    int rc = alva_ctx_pinned(ctx, 64 * sizeof(int), (void **) &pin);
    if (rc) return rc;
    uint8_t *scr = nullptr;
    rc = alva_ctx_scratch(ctx, CA_SCRATCH_SLOT, 256, (void **) &scr);
    if (rc) return rc;
    A.counts = (int *) scr;
    ALVA_HIP(hipMemsetAsync(A.counts, 0, 8 * sizeof(int), ctx->stream));
    hipLaunchKernelGGL(k_mesh_color_at, dim3(alva_divup(n, 256)), dim3(256), 0, ctx->stream, A);
    ALVA_LAUNCH_CHECK();
    ALVA_HIP(hipMemcpyAsync(pin + 56, A.counts, 4 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    ALVA_HIP(alva_stream_sync(ctx->stream));
    h_info8[0] = n;
    memcpy(h_info8 + 1, pin + 56, 4 * sizeof(int));
    h_info8[5] = h_info8[6] = 0;
    h_info8[7] = N;
    return ALVA_OK;
}
