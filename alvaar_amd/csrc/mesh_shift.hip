// Scene volume shift: the volume translated by whole voxels into a second volume, zeros entering on the far side (alva_mesh_shift, S1-S4
// of include/alvaar_hip.h) -- what lets the session's volume follow the camera.  The reference has no counterpart; the definition is
// pinned by the numpy restatement tests/mesh_shift_cases.py.  Nothing is resampled and nothing is computed but integer counts: the
// output is the input's bytes where the two cubes overlap.
//
//   k_mesh_shift  one launch for q, w and the colour volume, on k_mesh_integrate's striding grid (at most 2048 workgroups).  A thread
//                 owns one UNIT of the index space, x on the lanes, and has two duties for it.  As a SOURCE: it loads the unit's w
//                 (which the counts need of every voxel, kept or lost) and, where the unit's destination lies inside the cube, its q
//                 and colour, and stores the three there.  As a DESTINATION: where the unit's own source lies outside, it stores
//                 zeros.  So every input byte is loaded at most once, every output byte is stored exactly once, and both the loads
//                 and the stores of a wave are contiguous.
//                 WIDE: a unit is 8 voxels of a row -- 16 bytes of q, 8 of w, 32 of colour per lane.  It needs N and s_x to be
//                 multiples of 8 (then a unit is wholly kept or wholly lost and every row offset is a multiple of 8 voxels) and the six
//                 arrays aligned to their access; otherwise a unit is one voxel.  Both give the same bytes.
//                 The four counts go per thread, per wave, per workgroup, then one integer atomicAdd per workgroup and count.
#include "common.hpp"
#include "wave_utils.hpp"
#include <climits>

namespace {

constexpr int SHIFT_SCRATCH_SLOT = 9;   // (shared with the other synchronous stages)
constexpr int SHIFT_N_MIN = 4, SHIFT_N_MAX = 256;
constexpr int SHIFT_GRID = 2048;   // workgroups at most: k_mesh_integrate's bound

struct ShiftArgs {
    const int16_t *q;
    const uint8_t *w;
    const uint32_t *c;   // [N^3]: r | g << 8 | b << 16 | wc << 24; or null (COLOR false)
    int16_t *q_out;
    uint8_t *w_out;
    uint32_t *c_out;
    int N;
    int s[3];   // every |s| < N; with `none` they are zero and not used
    int none;   // S3: nothing is copied
    int *counts;   // copied, copied with w > 0, lost with w > 0, copied with a colour weight > 0
};

// the number of non-zero bytes of a word
__device__ __forceinline__ int nonzero_bytes(uint32_t v) {
    v |= v >> 4;
    v |= v >> 2;
    v |= v >> 1;
    return __popc(v & 0x01010101u);
}

template <bool WIDE, bool COLOR>
__global__ void __launch_bounds__(256) k_mesh_shift(const ShiftArgs A) {
    constexpr int U = WIDE ? 8 : 1;   // voxels per unit
    __shared__ int s_n[4][4];
    const int N = A.N, V = N * N * N, units = V / U;   // (WIDE: N is a multiple of 8)
    const int delta = (A.s[2] * N + A.s[1]) * N + A.s[0];   // |delta| < N^3: S1's source index minus the destination's
    int n[4] = {0, 0, 0, 0};
    for (int base = blockIdx.x * 256; base < units; base += gridDim.x * 256) {
        const int u = base + threadIdx.x;
        if (u >= units) continue;
        const int idx = u * U;
        const int i = idx % N, j = (idx / N) % N, k = idx / (N * N);
        // S1, S2 as a source: the voxels idx .. idx + U - 1 go to idx - delta where (i - s_x, j - s_y, k - s_z) lies inside.  (unsigned)
        // makes a negative coordinate a large one; WIDE: i and s_x are multiples of 8, so the unit's eight voxels share the answer
        const bool to_in = !A.none && (unsigned) (i - A.s[0]) < (unsigned) N && (unsigned) (j - A.s[1]) < (unsigned) N &&
                           (unsigned) (k - A.s[2]) < (unsigned) N;
        // as a destination: the source of idx is (i + s_x, j + s_y, k + s_z)
        const bool from_in = !A.none && (unsigned) (i + A.s[0]) < (unsigned) N && (unsigned) (j + A.s[1]) < (unsigned) N &&
                             (unsigned) (k + A.s[2]) < (unsigned) N;
        if constexpr (WIDE) {
            const uint2 w8 = *(const uint2 *) (A.w + idx);
            const int weighted = nonzero_bytes(w8.x) + nonzero_bytes(w8.y);
            if (to_in) {
                const int dst = idx - delta;   // in [0, V - 8], a multiple of 8
                *(uint4 *) (A.q_out + dst) = *(const uint4 *) (A.q + idx);
                *(uint2 *) (A.w_out + dst) = w8;
                n[0] += 8;
                n[1] += weighted;
                if constexpr (COLOR) {
                    const uint4 c0 = *(const uint4 *) (A.c + idx), c1 = *(const uint4 *) (A.c + idx + 4);
                    *(uint4 *) (A.c_out + dst) = c0;
                    *(uint4 *) (A.c_out + dst + 4) = c1;
                    n[3] += ((c0.x >> 24) != 0) + ((c0.y >> 24) != 0) + ((c0.z >> 24) != 0) + ((c0.w >> 24) != 0) + ((c1.x >> 24) != 0) +
                            ((c1.y >> 24) != 0) + ((c1.z >> 24) != 0) + ((c1.w >> 24) != 0);
                }
            } else n[2] += weighted;
            if (!from_in) {
                const uint4 z = {0u, 0u, 0u, 0u};
                *(uint4 *) (A.q_out + idx) = z;
                *(uint2 *) (A.w_out + idx) = uint2{0u, 0u};
                if constexpr (COLOR) {
                    *(uint4 *) (A.c_out + idx) = z;
                    *(uint4 *) (A.c_out + idx + 4) = z;
                }
            }
        } else {
            const uint8_t w0 = A.w[idx];
            if (to_in) {
                const int dst = idx - delta;   // in [0, V)
                A.q_out[dst] = A.q[idx];
                A.w_out[dst] = w0;
                n[0]++;
                n[1] += w0 != 0;
                if constexpr (COLOR) {
                    const uint32_t c0 = A.c[idx];
                    A.c_out[dst] = c0;
                    n[3] += (c0 >> 24) != 0;
                }
            } else n[2] += w0 != 0;
            if (!from_in) {
                A.q_out[idx] = 0;
                A.w_out[idx] = 0;
                if constexpr (COLOR) A.c_out[idx] = 0u;
            }
        }
    }
    // S4 (integers: the order of the additions does not matter)
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const int v = wave_sum(n[c]);
        if ((threadIdx.x & 63) == 0) s_n[threadIdx.x >> 6][c] = v;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int v = (s_n[0][threadIdx.x] + s_n[1][threadIdx.x]) + (s_n[2][threadIdx.x] + s_n[3][threadIdx.x]);
        if (v) atomicAdd(&A.counts[threadIdx.x], v);
    }
}

bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t a0 = (uintptr_t) a, b0 = (uintptr_t) b;
    return a && b && a0 < b0 + nb && b0 < a0 + na;
}

}  // namespace

extern "C" int alva_mesh_shift(alva_ctx *ctx, const int16_t *d_q, const uint8_t *d_w, const uint8_t *d_c, int N, const int *h_shift3,
                               int16_t *d_q_out, uint8_t *d_w_out, uint8_t *d_c_out, int *h_info8) {
    ALVA_ARG(ctx && d_q && d_w && h_shift3 && d_q_out && d_w_out && h_info8);
    ALVA_ARG((d_c != nullptr) == (d_c_out != nullptr));
    ALVA_ARG(N >= SHIFT_N_MIN && N <= SHIFT_N_MAX);
    ALVA_ARG(((uintptr_t) d_q % 2) == 0 && ((uintptr_t) d_q_out % 2) == 0 && ((uintptr_t) d_c % 4) == 0 && ((uintptr_t) d_c_out % 4) == 0);
    const size_t V = (size_t) N * N * N;
    {   // out of place: no output may overlap an input, or another output
        const void *in[3] = {d_q, d_w, d_c}, *out[3] = {d_q_out, d_w_out, d_c_out};
        const size_t bytes[3] = {2 * V, V, 4 * V};
        for (int a = 0; a < 3; a++)
            for (int b = 0; b < 3; b++) {
                ALVA_ARG(!ranges_overlap(in[a], bytes[a], out[b], bytes[b]));
                ALVA_ARG(a == b || !ranges_overlap(out[a], bytes[a], out[b], bytes[b]));
            }
    }
    ShiftArgs A{};
    A.q = d_q; A.w = d_w; A.c = (const uint32_t *) d_c;
    A.q_out = d_q_out; A.w_out = d_w_out; A.c_out = (uint32_t *) d_c_out;
    A.N = N;
    // S3, before any index is formed: the comparisons hold for every int, INT_MIN included
    for (int a = 0; a < 3; a++) A.none = A.none || h_shift3[a] <= -N || h_shift3[a] >= N;
    for (int a = 0; a < 3; a++) A.s[a] = A.none ? 0 : h_shift3[a];
    bool wide = N % 8 == 0 && A.s[0] % 8 == 0;
    wide = wide && ((uintptr_t) d_q % 16) == 0 && ((uintptr_t) d_q_out % 16) == 0 && ((uintptr_t) d_w % 8) == 0 && ((uintptr_t) d_w_out % 8) == 0 &&
           ((uintptr_t) d_c % 16) == 0 && ((uintptr_t) d_c_out % 16) == 0;
    int *pin = nullptr;
    int rc = alva_ctx_pinned(ctx, 64 * sizeof(int), (void **) &pin);
    if (rc) return rc;
    uint8_t *scr = nullptr;
    rc = alva_ctx_scratch(ctx, SHIFT_SCRATCH_SLOT, 256, (void **) &scr);
    if (rc) return rc;
    A.counts = (int *) scr;
    ALVA_HIP(hipMemsetAsync(A.counts, 0, 8 * sizeof(int), ctx->stream));
    const int units = (int) (V / (wide ? 8 : 1)), blocks = alva_divup(units, 256), grid = blocks < SHIFT_GRID ? blocks : SHIFT_GRID;
    if (wide && d_c) hipLaunchKernelGGL((k_mesh_shift<true, true>), dim3(grid), dim3(256), 0, ctx->stream, A);
    else if (wide) hipLaunchKernelGGL((k_mesh_shift<true, false>), dim3(grid), dim3(256), 0, ctx->stream, A);
    else if (d_c) hipLaunchKernelGGL((k_mesh_shift<false, true>), dim3(grid), dim3(256), 0, ctx->stream, A);
    else hipLaunchKernelGGL((k_mesh_shift<false, false>), dim3(grid), dim3(256), 0, ctx->stream, A);
    ALVA_LAUNCH_CHECK();
    ALVA_HIP(hipMemcpyAsync(pin + 48, A.counts, 4 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    ALVA_HIP(alva_stream_sync(ctx->stream));
    memcpy(h_info8, pin + 48, 4 * sizeof(int));
    h_info8[4] = h_info8[5] = h_info8[6] = 0;
    h_info8[7] = N;
    return ALVA_OK;
}
