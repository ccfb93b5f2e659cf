// Light estimation: ambient intensity, second-order spherical harmonics and the primary directional light of the scene -- ARCore's
// LightEstimate, ARKit's ARLightEstimate / ARDirectionalLightEstimate, WebXR light-estimation.  The reference has no counterpart, so the
// definitions in include/alvaar_hip.h (B1-B5, F1-F3, E1-E5) are pinned by the numpy restatement tests/light_cases.py.  Every frame is
// binned by its rotation into a world-aligned cube map (8 x 8 cells per face) kept on the device, and the estimate is projected from
// that map.  Sums whose order is not fixed are integer sums; geometry and the projection are IEEE double in the written order (compile
// with -ffp-contract=off), so the same inputs give the same bits.
//
// alva_light_bin, one launch (k_light_bin), no host wait.  A workgroup takes a tile of whole blocks, at most 64 x L_TILE_H pixels:
//   pixels      a lane reads four pixels of one row with one 16-byte load (pixel by pixel where the address is not aligned or the tile
//               ends), sixteen rows per pass, looks the channels up in the table (LDS) and adds its run of pixels to the block's sums in
//               LDS
//   blocks      one lane per block: the frame's sums per wave, then one LDS add; with a rotation the block's direction (once per block,
//               not per pixel), its cell, and the cell's sums in LDS (uint32 is enough for a workgroup's pixels) -- per wave where the
//               whole wave has one cell, which is the usual case
//   flush       the cells the tile touched and the frame's sums, by 64-bit global atomics
// alva_light_fuse, one workgroup of 384 lanes (one per cell) queued right behind it; alva_light_estimate, one wave at call time, which
// writes its answer into pinned host memory.
#include "common.hpp"
#include "camera_device.hpp"
#include "wave_utils.hpp"
#include <cmath>

namespace {

constexpr int LN = ALVA_LIGHT_N, LCELLS = ALVA_LIGHT_CELLS;
constexpr int L_FRAME = 4 * LCELLS;               // the frame's words behind the cells' in the accumulators
constexpr int L_STATE_W = 12 * LCELLS;            // byte offsets into the state: E u32 [cell][3], W u8 [cell], latch u32 [8]
constexpr int L_STATE_LATCH = 13 * LCELLS;
static_assert(L_STATE_LATCH + 32 == ALVA_LIGHT_STATE_BYTES && L_FRAME + 8 == ALVA_LIGHT_ACC_WORDS, "layout");

__constant__ uint16_t c_light_lut[256] = {
#include "light_lut.inc"
};

// ---------------------------------------------------------------------------------------------------------------------- bin
struct BinArgs {
    const uint8_t *rgba;
    size_t pitch;
    int step, gw, gh, bx, by;   // the grid in blocks, a tile in blocks
    int has_R;
    AlvaCam cam;
    double R[9];
    unsigned long long *acc;
};

// B4: the cell of a direction, -1 for none
__device__ __forceinline__ int light_cell(double d0, double d1, double d2) {
    if (!(isfinite(d0) && isfinite(d1) && isfinite(d2))) return -1;
    const double a0 = fabs(d0), a1 = fabs(d1), a2 = fabs(d2);
    int axis = 0;
    double m = a0;
    if (a1 > m) { axis = 1; m = a1; }
    if (a2 > m) { axis = 2; m = a2; }
    if (!(m > 0.)) return -1;
    const double major = axis == 0 ? d0 : axis == 1 ? d1 : d2;
    const int face = 2 * axis + (major < 0. ? 1 : 0);
    const double a = (axis == 0 ? d1 : d0) / m, b = (axis == 2 ? d1 : d2) / m;
    const int fi = (int) floor((a + 1.) * 4.0), fj = (int) floor((b + 1.) * 4.0);
    const int i = fi < LN - 1 ? fi : LN - 1, j = fj < LN - 1 ? fj : LN - 1;
    return (face * LN + j) * LN + i;
}

// a tile in pixels, at most.  Measured (k_light_bin, HIP events, 640 x 480 / 1280 x 720): 11.4 / 19.0 us with 16 rows, 10.3 / 14.2 with 32,
// 10.8 / 12.6 with 64 -- a workgroup's fixed work (clearing and flushing 384 cells) wants more than four pixels per lane to pay for it
constexpr int L_TILE_W = 64, L_TILE_H = 64;
constexpr int L_TILE_BLOCKS = (L_TILE_W / 2) * (L_TILE_H / 2);           // blocks of a tile at step 2, the most
static_assert(L_TILE_H % 16 == 0 && L_TILE_W * L_TILE_H <= 65536, "uint32 sums per workgroup");

__global__ void __launch_bounds__(256) k_light_bin(const BinArgs A) {
    __shared__ uint16_t s_lut[256];
    __shared__ unsigned s_blk[L_TILE_BLOCKS * 4];   // per block of the tile: S_R, S_G, S_B, saturated
    __shared__ unsigned s_cell[LCELLS * 4];         // per cell: S_R, S_G, S_B, pixels
    __shared__ unsigned s_frame[8];                 // S_R, S_G, S_B, pixels, saturated, blocks
    const int t = threadIdx.x;
    const int step = A.step, nblk = A.bx * A.by;
    s_lut[t] = c_light_lut[t];
    for (int i = t; i < nblk * 4; i += 256) s_blk[i] = 0u;
    for (int i = t; i < LCELLS * 4; i += 256) s_cell[i] = 0u;
    if (t < 8) s_frame[t] = 0u;
    __syncthreads();
    const int gx0 = blockIdx.x * A.bx, gy0 = blockIdx.y * A.by;
    const int tile_w = A.bx * step, tile_h = A.by * step;   // <= L_TILE_W x L_TILE_H pixels
    // B1, B2: four pixels of one row per lane and pass, sixteen rows per pass
    {
        const int lx0 = (t & 15) * 4;
        int nvalid = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) nvalid += (lx0 + i < tile_w && gx0 + (lx0 + i) / step < A.gw) ? 1 : 0;   // (a prefix: both bounds grow with i)
        for (int r = t >> 4; r < tile_h && nvalid > 0; r += 16) {
            if (gy0 + r / step >= A.gh) break;
            const uint8_t *row = A.rgba + (size_t) (gy0 * step + r) * A.pitch + (size_t) (gx0 * step + lx0) * 4;
            unsigned px[4] = {0u, 0u, 0u, 0u};
            if (nvalid == 4 && (((uintptr_t) row) & 15) == 0) {
                const uint4 v = *(const uint4 *) row;
                px[0] = v.x; px[1] = v.y; px[2] = v.z; px[3] = v.w;
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++)
                    if (i < nvalid) px[i] = *(const unsigned *) (row + 4 * i);
            }
            int cur = -1;
            unsigned sr = 0, sg = 0, sb = 0, sat = 0;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                if (i >= nvalid) break;
                const int b = (r / step) * A.bx + (lx0 + i) / step;
                if (b != cur) {
                    if (cur >= 0) {
                        atomicAdd(&s_blk[4 * cur], sr);
                        atomicAdd(&s_blk[4 * cur + 1], sg);
                        atomicAdd(&s_blk[4 * cur + 2], sb);
                        if (sat) atomicAdd(&s_blk[4 * cur + 3], sat);
                    }
                    cur = b;
                    sr = sg = sb = sat = 0;
                }
                const unsigned R = px[i] & 255u, G = (px[i] >> 8) & 255u, B = (px[i] >> 16) & 255u;
                sr += s_lut[R];
                sg += s_lut[G];
                sb += s_lut[B];
                sat += (R >= 250u || G >= 250u || B >= 250u) ? 1u : 0u;
            }
            if (cur >= 0) {
                atomicAdd(&s_blk[4 * cur], sr);
                atomicAdd(&s_blk[4 * cur + 1], sg);
                atomicAdd(&s_blk[4 * cur + 2], sb);
                if (sat) atomicAdd(&s_blk[4 * cur + 3], sat);
            }
        }
    }
    __syncthreads();
    // B3 - B5: one lane per block of the tile.  The sums of a wave stay below 2^31 (64 blocks of at most 256 pixels of at most 65535)
    for (int b0 = 0; b0 < nblk; b0 += 256) {
        const int b = b0 + t;
        const int lbx = b % A.bx, lby = b / A.bx;
        const int gx = gx0 + lbx, gy = gy0 + lby;
        const bool live = b < nblk && gx < A.gw && gy < A.gh;
        const unsigned sr = live ? s_blk[4 * b] : 0u, sg = live ? s_blk[4 * b + 1] : 0u, sb = live ? s_blk[4 * b + 2] : 0u;
        const unsigned sat = live ? s_blk[4 * b + 3] : 0u, npx = live ? (unsigned) (step * step) : 0u;
        const int w_k = wave_sum(live ? 1 : 0);
        if (!w_k) continue;   // (wave-uniform)
        const int w_r = wave_sum((int) sr), w_g = wave_sum((int) sg), w_b = wave_sum((int) sb), w_n = wave_sum((int) npx);
        const int w_s = wave_sum((int) sat);
        if ((t & 63) == 0) {
            atomicAdd(&s_frame[0], (unsigned) w_r);
            atomicAdd(&s_frame[1], (unsigned) w_g);
            atomicAdd(&s_frame[2], (unsigned) w_b);
            atomicAdd(&s_frame[3], (unsigned) w_n);
            if (w_s) atomicAdd(&s_frame[4], (unsigned) w_s);
            atomicAdd(&s_frame[5], (unsigned) w_k);
        }
        if (!A.has_R) continue;
        int cell = -1;
        if (live) {
            const int u = gx * step + step / 2, v = gy * step + step / 2;
            float uu, vv;
            alva_undistort_dev(A.cam, (float) u, (float) v, uu, vv);
            const double x = ((double) uu - A.cam.cx) / A.cam.fx, y = ((double) vv - A.cam.cy) / A.cam.fy;
            const double d0 = (A.R[0] * x + A.R[1] * y) + A.R[2] * 1.;
            const double d1 = (A.R[3] * x + A.R[4] * y) + A.R[5] * 1.;
            const double d2 = (A.R[6] * x + A.R[7] * y) + A.R[8] * 1.;
            cell = light_cell(d0, d1, d2);
        }
        // a tile is much smaller than a cell: mostly the whole wave has one cell, and then one lane adds the wave's sums
        int cmax = cell;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const int o = __shfl_xor(cmax, d);
            cmax = o > cmax ? o : cmax;
        }
        if (cmax < 0) continue;
        if (__all(cell == cmax || cell < 0)) {
            const bool in = cell >= 0;
            const int c_r = wave_sum(in ? (int) sr : 0), c_g = wave_sum(in ? (int) sg : 0), c_b = wave_sum(in ? (int) sb : 0);
            const int c_n = wave_sum(in ? (int) npx : 0);
            if ((t & 63) == 0) {
                atomicAdd(&s_cell[4 * cmax], (unsigned) c_r);
                atomicAdd(&s_cell[4 * cmax + 1], (unsigned) c_g);
                atomicAdd(&s_cell[4 * cmax + 2], (unsigned) c_b);
                atomicAdd(&s_cell[4 * cmax + 3], (unsigned) c_n);
            }
        } else if (cell >= 0) {
            atomicAdd(&s_cell[4 * cell], sr);
            atomicAdd(&s_cell[4 * cell + 1], sg);
            atomicAdd(&s_cell[4 * cell + 2], sb);
            atomicAdd(&s_cell[4 * cell + 3], npx);
        }
    }
    __syncthreads();
    for (int c = t; c < LCELLS; c += 256) {
        if (s_cell[4 * c + 3]) {
#pragma unroll
            for (int k = 0; k < 4; k++) atomicAdd(&A.acc[4 * c + k], (unsigned long long) s_cell[4 * c + k]);
        }
    }
    if (t < 6 && s_frame[5]) atomicAdd(&A.acc[L_FRAME + t], (unsigned long long) s_frame[t]);
}

// ---------------------------------------------------------------------------------------------------------------------- fuse
__global__ void __launch_bounds__(LCELLS) k_light_fuse(unsigned long long *acc, uint8_t *state, unsigned min_pixels, unsigned w_new, unsigned w_max,
                                                       unsigned long long *acc_out, unsigned *started, unsigned seq) {
    __shared__ unsigned s_count[2];   // observed, touched
    const int c = threadIdx.x;
    // this launch runs: every bin queued before it on the stream has finished, so the frames they read belong to their owner again
    if (c == 0 && started) __hip_atomic_store(started, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (c < 2) s_count[c] = 0u;
    __syncthreads();
    unsigned *E = (unsigned *) state + 3 * c;
    uint8_t *W = state + L_STATE_W + c;
    unsigned *latch = (unsigned *) (state + L_STATE_LATCH);
    unsigned long long a[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        a[k] = acc[4 * c + k];
        if (acc_out) acc_out[4 * c + k] = a[k];
        acc[4 * c + k] = 0ull;
    }
    const unsigned long long n = a[3];
    if (n > 0ull) atomicAdd(&s_count[1], 1u);
    if (n >= (unsigned long long) min_pixels) {   // F1 (min_pixels >= 1)
        atomicAdd(&s_count[0], 1u);
        const unsigned long long w = *W;
#pragma unroll
        for (int k = 0; k < 3; k++) {             // F2
            const unsigned long long m = a[k] / n;
            E[k] = (unsigned) (w == 0ull ? m : ((unsigned long long) E[k] * w + m * (unsigned long long) w_new) / (w + (unsigned long long) w_new));
        }
        const unsigned long long wn = w + (unsigned long long) w_new;
        *W = (uint8_t) (w == 0ull ? w_new : wn < (unsigned long long) w_max ? (unsigned) wn : w_max);
    }
    __syncthreads();
    if (c == 0) {   // F3
        unsigned long long f[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            f[k] = acc[L_FRAME + k];
            if (acc_out) acc_out[L_FRAME + k] = f[k];
            acc[L_FRAME + k] = 0ull;
        }
        if (f[3] > 0ull) {
            latch[0] = (unsigned) (f[0] / f[3]);
            latch[1] = (unsigned) (f[1] / f[3]);
            latch[2] = (unsigned) (f[2] / f[3]);
            latch[3] = (unsigned) f[4];
            latch[4] = (unsigned) f[5];
            latch[5] = s_count[1];
            latch[7] += 1u;
        }
        if (s_count[0]) latch[6] += 1u;
    }
}

// ---------------------------------------------------------------------------------------------------------------------- estimate
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// one wave; out = sh [27], primary_dir [3], primary_rgb [3], ambient [4] (floats), then info [8] (ints)
__global__ void __launch_bounds__(64) k_light_estimate(const uint8_t *state, const double *table, float *out, int *info) {
    const int l = threadIdx.x;
    const unsigned *E = (const unsigned *) state;
    const uint8_t *W = state + L_STATE_W;
    const unsigned *latch = (const unsigned *) (state + L_STATE_LATCH);
    // E1
    int k_mine = 0;
    unsigned long long s_mine[3] = {0ull, 0ull, 0ull};
    for (int j = 0; j < LCELLS / 64; j++) {
        const int cell = l + 64 * j;
        if (W[cell]) {
            k_mine++;
#pragma unroll
            for (int c = 0; c < 3; c++) s_mine[c] += E[3 * cell + c];
        }
    }
    const int K = wave_sum(k_mine);
    unsigned A[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const unsigned long long s = wave_sum_u64(s_mine[c]);
        A[c] = K ? (unsigned) (s / (unsigned long long) K) : latch[c];
    }
    // E3
    double x[27];
#pragma unroll
    for (int i = 0; i < 27; i++) x[i] = 0.;
    for (int j = 0; j < LCELLS / 64; j++) {
        const int cell = l + 64 * j;
        const bool has = W[cell] != 0;
        double v[3];
#pragma unroll
        for (int c = 0; c < 3; c++) v[c] = (double) (has ? E[3 * cell + c] : A[c]) / 65535.0;
#pragma unroll
        for (int k = 0; k < 9; k++) {
            const double tb = table[k * LCELLS + cell];
#pragma unroll
            for (int c = 0; c < 3; c++) x[3 * k + c] += tb * v[c];
        }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
        for (int i = 0; i < 27; i++) x[i] += __shfl_down(x[i], s);   // lanes l < s hold x[l] + x[l + s]: lane 0 ends with the sum
    }
    if (l != 0) return;
    const int code = K ? 0 : latch[7] ? 1 : 5;
    if (!K) {
#pragma unroll
        for (int i = 3; i < 27; i++) x[i] = 0.;   // the ambient term in Y00 alone
    }
    // E4
    double lum[4];
#pragma unroll
    for (int k = 0; k < 4; k++) lum[k] = (0.2126 * x[3 * k] + 0.7152 * x[3 * k + 1]) + 0.0722 * x[3 * k + 2];
    const double g0 = lum[3], g1 = lum[1], g2 = lum[2];
    const double gg = (g0 * g0 + g1 * g1) + g2 * g2, thr = 1e-3 * lum[0];
    const bool valid = K && gg > thr * thr;
    for (int i = 0; i < 27; i++) out[i] = (float) x[i];
    if (valid) {
        const double nrm = sqrt(gg);
        const double d0 = g0 / nrm, d1 = g1 / nrm, d2 = g2 / nrm;
        out[27] = (float) d0;
        out[28] = (float) d1;
        out[29] = (float) d2;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double p = ((x[9 + c] * d0 + x[3 + c] * d1) + x[6 + c] * d2) / 0.488603;
            out[30 + c] = (float) (p > 0. ? p : 0.);
        }
    } else {
        for (int i = 27; i < 33; i++) out[i] = 0.f;
    }
    // E5
    const unsigned long long MR = latch[0], MG = latch[1], MB = latch[2];
    out[33] = (float) ((double) ((13933ull * MR + 46871ull * MG + 4732ull * MB) >> 16) / 65535.0);
    out[34] = MG ? (float) ((double) MR / (double) MG) : 1.f;
    out[35] = 1.f;
    out[36] = MG ? (float) ((double) MB / (double) MG) : 1.f;
    info[0] = code;
    info[1] = K;
    info[2] = (int) latch[5];
    info[3] = (int) latch[4];
    info[4] = (int) latch[3];
    info[5] = (int) latch[6];
    info[6] = valid ? 1 : 0;
    info[7] = 0;
}

// E2: the basis table, 9 x 384 doubles, with + - x / sqrt and the five literals only
void light_basis_table(double *T) {
    static const double PI = 3.141592653589793;
    double dir[LCELLS][3], om[LCELLS];
    double sum = 0.;
    for (int cell = 0; cell < LCELLS; cell++) {
        const int face = cell / (LN * LN), j = (cell / LN) % LN, i = cell % LN;
        const double a = (double) (2 * i + 1) / 8.0 - 1., b = (double) (2 * j + 1) / 8.0 - 1.;
        const double r2 = (1. + a * a) + b * b, r = sqrt(r2);
        const double major = (face & 1) ? -1. : 1.;
        const int axis = face >> 1;
        double d[3];
        d[axis] = major;
        d[axis == 0 ? 1 : 0] = a;
        d[axis == 2 ? 1 : 2] = b;
        for (int k = 0; k < 3; k++) dir[cell][k] = d[k] / r;
        om[cell] = 1. / (r2 * r);
        sum += om[cell];
    }
    const double scale = (4. * PI) / sum;
    for (int cell = 0; cell < LCELLS; cell++) {
        const double w = om[cell] * scale, x = dir[cell][0], y = dir[cell][1], z = dir[cell][2];
        T[0 * LCELLS + cell] = w * 0.282095;
        T[1 * LCELLS + cell] = w * (0.488603 * y);
        T[2 * LCELLS + cell] = w * (0.488603 * z);
        T[3 * LCELLS + cell] = w * (0.488603 * x);
        T[4 * LCELLS + cell] = w * (1.092548 * (x * y));
        T[5 * LCELLS + cell] = w * (1.092548 * (y * z));
        T[6 * LCELLS + cell] = w * (0.315392 * (3. * (z * z) - 1.));
        T[7 * LCELLS + cell] = w * (1.092548 * (x * z));
        T[8 * LCELLS + cell] = w * (0.546274 * (x * x - y * y));
    }
}

}  // namespace

extern "C" int alva_light_bin(alva_ctx *ctx, const uint8_t *d_rgba, size_t pitch, int width, int height, const double *h_calib8,
                              const double *h_R_wc9, int step, uint64_t *d_acc) {
    ALVA_ARG(ctx && d_rgba && h_calib8 && d_acc);
    ALVA_ARG(width >= 1 && height >= 1 && width <= 16384 && height <= 16384 && pitch >= (size_t) width * 4);
    ALVA_ARG(pitch % 4 == 0 && ((uintptr_t) d_rgba % 4) == 0 && ((uintptr_t) d_acc % 8) == 0);
    ALVA_ARG(step >= 2 && step <= 16);
    for (int i = 0; i < 8; i++) ALVA_ARG(std::isfinite(h_calib8[i]));
    ALVA_ARG(h_calib8[0] > 0 && h_calib8[1] > 0);
    BinArgs A{};
    A.rgba = d_rgba; A.pitch = pitch; A.step = step;
    A.gw = width / step; A.gh = height / step;
    if (A.gw == 0 || A.gh == 0) return ALVA_OK;   // no block: nothing is added
    A.bx = L_TILE_W / step; A.by = L_TILE_H / step;   // a tile of whole blocks
    A.has_R = h_R_wc9 != nullptr;
    A.cam = AlvaCam{h_calib8[0], h_calib8[1], h_calib8[2], h_calib8[3], h_calib8[4], h_calib8[5], h_calib8[6], h_calib8[7]};
    if (h_R_wc9) memcpy(A.R, h_R_wc9, sizeof(A.R));
    A.acc = (unsigned long long *) d_acc;
    hipLaunchKernelGGL(k_light_bin, dim3(alva_divup(A.gw, A.bx), alva_divup(A.gh, A.by)), dim3(256), 0, ctx->stream, A);
    ALVA_LAUNCH_CHECK();
    return ALVA_OK;
}

int alva_light_fuse_started(alva_ctx *ctx, uint64_t *d_acc, uint8_t *d_state, int min_pixels, int w_new, int w_max, uint64_t *d_acc_out,
                            uint32_t *h_started, uint32_t seq) {
    ALVA_ARG(ctx && d_acc && d_state && ((uintptr_t) d_acc % 8) == 0 && ((uintptr_t) d_state % 4) == 0 && ((uintptr_t) d_acc_out % 8) == 0);
    ALVA_ARG(min_pixels >= 1 && w_new >= 1 && w_new <= w_max && w_max <= 255 && d_acc_out != d_acc);
    hipLaunchKernelGGL(k_light_fuse, dim3(1), dim3(LCELLS), 0, ctx->stream, (unsigned long long *) d_acc, d_state, (unsigned) min_pixels,
                       (unsigned) w_new, (unsigned) w_max, (unsigned long long *) d_acc_out, (unsigned *) h_started, (unsigned) seq);
    ALVA_LAUNCH_CHECK();
    return ALVA_OK;
}

extern "C" int alva_light_fuse(alva_ctx *ctx, uint64_t *d_acc, uint8_t *d_state, int min_pixels, int w_new, int w_max, uint64_t *d_acc_out) {
    return alva_light_fuse_started(ctx, d_acc, d_state, min_pixels, w_new, w_max, d_acc_out, nullptr, 0);
}

extern "C" int alva_light_estimate(alva_ctx *ctx, const uint8_t *d_state, float *h_sh27, float *h_primary_dir3, float *h_primary_rgb3,
                                   float *h_ambient4, int *h_info8) {
    ALVA_ARG(ctx && d_state && ((uintptr_t) d_state % 4) == 0 && h_sh27 && h_primary_dir3 && h_primary_rgb3 && h_ambient4 && h_info8);
    if (!ctx->light_basis) {   // E2, once per context
        std::vector<double> T(9 * LCELLS);
        light_basis_table(T.data());
        double *d = nullptr;
        ALVA_HIP(hipMalloc((void **) &d, T.size() * sizeof(double)));
        if (hipMemcpy(d, T.data(), T.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
            (void) hipFree(d);
            alva_set_error("alva_light_estimate: the basis table could not be uploaded");
            return ALVA_ERR_HIP;
        }
        ctx->light_basis = d;
    }
    uint8_t *pin = nullptr;
    int rc = alva_ctx_pinned(ctx, 1024, (void **) &pin);
    if (rc) return rc;
    float *out = (float *) (pin + 512);
    int *info = (int *) (pin + 512 + 40 * sizeof(float));
    hipLaunchKernelGGL(k_light_estimate, dim3(1), dim3(64), 0, ctx->stream, d_state, (const double *) ctx->light_basis, out, info);
    ALVA_LAUNCH_CHECK();
    ALVA_HIP(alva_stream_sync(ctx->stream));
    memcpy(h_sh27, out, 27 * sizeof(float));
    memcpy(h_primary_dir3, out + 27, 3 * sizeof(float));
    memcpy(h_primary_rgb3, out + 30, 3 * sizeof(float));
    memcpy(h_ambient4, out + 33, 4 * sizeof(float));
    memcpy(h_info8, info, 8 * sizeof(int));
    return ALVA_OK;
}
