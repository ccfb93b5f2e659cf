// Dense depth: the depth image fused over time (alva_depth_fuse) and completed (alva_depth_fill) -- ARCore's acquireDepthImage16Bits /
// ARKit's smoothedSceneDepth beside the raw image of depth_sweep.hip.  The reference has no counterpart, so the definitions in
// include/alvaar_hip.h (F1-F5, P1-P4) are pinned by the numpy restatement tests/dense_cases.py.  Geometry is IEEE double in the written
// order (compile with -ffp-contract=off), every decision is made on integers or on single IEEE comparisons, and every sum whose order is
// not fixed is an integer sum, so the same inputs give the same bits.
//
// alva_depth_fuse, three launches:
//   k_dense_clear  the per-cell keys and the six counters to 0
//   k_dense_warp   one thread per cell of the previous state: its point in the current frame, one 64-bit atomicMax of (bits(rho') << 32) |
//                  (0xFFFFFFFF - i) on the target cell's key -- positive floats order as their bits, so the largest rho' (the nearest
//                  surface) wins and the lowest source index on a tie, in whatever order the sources arrive
//   k_dense_fuse   one thread per cell: the carried value from the key, the measurement, the fusion rule; the src counts per thread, then
//                  per wave, then one integer atomicAdd per wave and bin
// alva_depth_fill, push-pull over a pyramid whose launches do not grow with max_level (two for max_level <= 4, three above):
//   k_dense_pull   one workgroup per aligned 16 x 16 tile of its base level: up to four coarser levels in LDS, each written to the global
//                  pyramid (level 0 too: q, W and the guide).  Once from level 0, and for max_level > 4 once more from level 4
//   k_dense_push   one workgroup per aligned 2^min(max_level, 5) tile of level 0: per level, from the top down, the tile's cells and a halo
//                  of one cell (3 x 3 above the tile's own size) in LDS; the halo cells are recomputed exactly as the neighbouring tile
//                  computes them, because a cell's parents lie within the halo of the level above.  Writes level 0 and counts
#include "common.hpp"
#include "camera_device.hpp"
#include "wave_utils.hpp"
#include <cmath>

namespace {

constexpr int DD_SRCS = 6;
constexpr int DD_MAX_LEVEL = 8;
constexpr int DD_SCRATCH_SLOT = 9;
constexpr int DD_Q_MAX = (1 << 20) - 1;

// ---------------------------------------------------------------------------------------------------------------------- fuse
struct FuseArgs {
    const float *prev_rho;   // null: no previous state
    const uint8_t *prev_w;
    const float *m_depth;    // null: no measurement
    const uint8_t *m_conf, *m_code;
    int width, height, step, gw, gh;
    AlvaCam cam;
    double R[9], t[3];       // X_cur = R X_prev + t
    int decay, w_max;
    double rel_tol;
    unsigned long long *keys;
    int *counts;
    float *rho;
    uint8_t *w, *src;
};

__global__ void __launch_bounds__(256) k_dense_clear(unsigned long long *keys, int n, int *counts, int n_counts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) keys[i] = 0ull;
    if (i < n_counts) counts[i] = 0;
}

__global__ void __launch_bounds__(256) k_dense_warp(const FuseArgs A) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= A.gw * A.gh) return;
    const float rho_f = A.prev_rho[i];
    if (A.prev_w[i] == 0 || !(rho_f > 0.f)) return;
    const int gx = i % A.gw, gy = i / A.gw;
    const int u = gx * A.step + A.step / 2, v = gy * A.step + A.step / 2;
    float uu, vv;
    alva_undistort_dev(A.cam, (float) u, (float) v, uu, vv);
    const double x = ((double) uu - A.cam.cx) / A.cam.fx, y = ((double) vv - A.cam.cy) / A.cam.fy;
    const double rho = (double) rho_f;
    const double Px = ((A.R[0] * x + A.R[1] * y) + A.R[2] * 1.) + rho * A.t[0];
    const double Py = ((A.R[3] * x + A.R[4] * y) + A.R[5] * 1.) + rho * A.t[1];
    const double Pz = ((A.R[6] * x + A.R[7] * y) + A.R[8] * 1.) + rho * A.t[2];
    if (!(Pz > 1e-9)) return;
    float up, vp;
    alva_project_dist_dev(A.cam, Px, Py, Pz, up, vp);
    const float fu = floorf(up + 0.5f), fv = floorf(vp + 0.5f);
    if (!(0.f <= fu && fu < (float) (A.gw * A.step) && 0.f <= fv && fv < (float) (A.gh * A.step))) return;   // (a NaN fails every comparison)
    const float rho_n = (float) (rho / Pz);
    if (!(rho_n > 0.f && rho_n <= 3.402823466e+38f)) return;
    const int j = ((int) fv / A.step) * A.gw + (int) fu / A.step;
    const unsigned long long key = ((unsigned long long) __float_as_uint(rho_n) << 32) | (unsigned long long) (0xFFFFFFFFu - (unsigned) i);
    atomicMax(&A.keys[j], key);
}

__global__ void __launch_bounds__(256) k_dense_fuse(const FuseArgs A) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    int s = -1;
    if (j < A.gw * A.gh) {
        // F2 the carried value
        float rho_c = 0.f;
        int w_c = 0;
        if (A.prev_rho) {
            const unsigned long long key = A.keys[j];
            if (key) {
                const unsigned i = 0xFFFFFFFFu - (unsigned) (key & 0xFFFFFFFFull);
                w_c = ((int) A.prev_w[i] * A.decay) >> 8;
                rho_c = __uint_as_float((unsigned) (key >> 32));
            }
        }
        // F3 the measurement
        float rho_m = 0.f;
        int w_m = 0;
        if (A.m_depth && A.m_code[j] == 0 && A.m_depth[j] > 0.f) {
            rho_m = (float) (1.0 / (double) A.m_depth[j]);
            w_m = (int) A.m_conf[j] >> 3;
            w_m = w_m > 1 ? w_m : 1;
        }
        // F4
        float rho = 0.f;
        int w = 0;
        if (w_c == 0 && w_m == 0) {
            s = 0;
        } else if (w_c == 0) {
            s = 1; rho = rho_m; w = w_m;
        } else if (w_m == 0) {
            s = 2; rho = rho_c; w = w_c;
        } else {
            const double a = (double) rho_c, b = (double) rho_m;
            if (fabs(a - b) <= A.rel_tol * fmax(a, b)) {
                s = 3;
                rho = (float) (((double) w_c * a + (double) w_m * b) / (double) (w_c + w_m));
                w = w_c + w_m < A.w_max ? w_c + w_m : A.w_max;
            } else if (w_m >= w_c) {
                s = 4; rho = rho_m; w = w_m;
            } else {
                s = 5; rho = rho_c; w = w_c - w_m;
            }
        }
        A.rho[j] = rho;
        A.w[j] = (uint8_t) w;
        A.src[j] = (uint8_t) s;
    }
    // F5 (integers: the order of the additions does not matter)
#pragma unroll
    for (int k = 0; k < DD_SRCS; k++) {
        const int c = wave_sum(s == k ? 1 : 0);
        if ((threadIdx.x & 63) == 0 && c) atomicAdd(&A.counts[k], c);
    }
}

// ---------------------------------------------------------------------------------------------------------------------- fill
// the pyramid in global memory, levels 0..L: per cell pack = q | W << 20, and the guide
struct Pyr {
    int L;
    int w[DD_MAX_LEVEL + 1], h[DD_MAX_LEVEL + 1];
    unsigned off[DD_MAX_LEVEL + 2];
    unsigned *pack;
    uint8_t *guide;
};

struct FillArgs {
    const float *rho;
    const uint8_t *w;
    const uint8_t *gray;
    size_t pitch;
    int step;
    double rho_ref;
    Pyr P;
    int *counts;   // seeds, filled, empty, levels used
    float *depth;
    uint8_t *level;
};

__device__ __forceinline__ int dd_E(int d) {
    const int s = (d >> 3) < 6 ? (d >> 3) : 6;
    const int e = 64 >> s;
    return e > 1 ? e : 1;
}

// base = 0: P1 from the state, then up to four pulls; base = 4: from level 4 of the pyramid
__global__ void __launch_bounds__(256) k_dense_pull(const FillArgs A, int base, int nlev) {
    __shared__ unsigned s_pack[256 + 64 + 16 + 4 + 1];
    __shared__ uint8_t s_g[256 + 64 + 16 + 4 + 1];
    const Pyr &P = A.P;
    const int t = threadIdx.x;
    if (base == 0 && blockIdx.x == 0 && blockIdx.y == 0 && t < 4) A.counts[t] = 0;
    {
        const int lx = t & 15, ly = t >> 4;
        const int X = blockIdx.x * 16 + lx, Y = blockIdx.y * 16 + ly;
        unsigned pk = 0;
        int g = 0;
        if (X < P.w[base] && Y < P.h[base]) {
            const size_t c = (size_t) P.off[base] + (size_t) Y * P.w[base] + X;
            if (base == 0) {
                // P1
                const int wt = A.w[c];
                if (wt > 0) {
                    const double r = rint(((double) A.rho[c] / A.rho_ref) * 65536.0);
                    const int q = r >= (double) DD_Q_MAX ? DD_Q_MAX : r >= 0. ? (int) r : 0;   // (a NaN becomes 0)
                    pk = (unsigned) q | ((unsigned) wt << 20);
                }
                g = A.gray[(size_t) (Y * A.step + A.step / 2) * A.pitch + (size_t) (X * A.step + A.step / 2)];
                P.pack[c] = pk;
                P.guide[c] = (uint8_t) g;
            } else {
                pk = P.pack[c];
                g = P.guide[c];
            }
        }
        s_pack[t] = pk;
        s_g[t] = (uint8_t) g;
    }
    __syncthreads();
    // P2
    int src_off = 0, side = 16;
    for (int k = 1; k <= nlev; k++) {
        const int cs = side >> 1, dst_off = src_off + side * side;
        const int lf = base + k - 1, lc = base + k;
        if (t < cs * cs) {
            const int lx = t % cs, ly = t / cs;
            const int X = blockIdx.x * cs + lx, Y = blockIdx.y * cs + ly;
            unsigned pk = 0;
            int g = 0;
            if (X < P.w[lc] && Y < P.h[lc]) {
                int n = 0, gs = 0, ws = 0;
                long long qs = 0;
#pragma unroll
                for (int d = 0; d < 4; d++) {
                    const int fx = 2 * X + (d & 1), fy = 2 * Y + (d >> 1);
                    if (fx < P.w[lf] && fy < P.h[lf]) {
                        const int li = src_off + (2 * ly + (d >> 1)) * side + 2 * lx + (d & 1);
                        const unsigned c = s_pack[li];
                        const int wc = (int) (c >> 20) & 255;
                        n++;
                        gs += s_g[li];
                        ws += wc;
                        qs += (long long) wc * (long long) (c & DD_Q_MAX);
                    }
                }
                g = (gs + n / 2) / n;
                if (ws > 0) pk = (unsigned) ((qs + ws / 2) / ws) | ((unsigned) (ws < 255 ? ws : 255) << 20);
                const size_t c = (size_t) P.off[lc] + (size_t) Y * P.w[lc] + X;
                P.pack[c] = pk;
                P.guide[c] = (uint8_t) g;
            }
            s_pack[dst_off + t] = pk;
            s_g[dst_off + t] = (uint8_t) g;
        }
        __syncthreads();
        src_off = dst_off;
        side = cs;
    }
}

// The push of one tile.  At level l the tile covers x0 = tx0 >> l .. x1 = (tx0 + T - 1) >> l and the workgroup holds [x0 - 1, x1 + 1], per
// axis.  A cell's parents are x >> 1 and (x >> 1) + (x & 1 ? 1 : -1); for every cell of that range they lie in [(x0 >> 1) - 1, (x1 >> 1)
// + 1], the range held of the level above: for x = x0 - 1, x0 even gives (x0 >> 1) - 1 and x0 >> 1, x0 odd gives x0 >> 1 and (x0 >> 1) -
// 1; for x = x1 + 1, x1 odd gives (x1 >> 1) + 1 and x1 >> 1, x1 even gives x1 >> 1 and (x1 >> 1) + 1; the cells between have parents
// within [x0 >> 1, x1 >> 1] and one step beside.  So a halo of one cell per level is enough, and a halo cell gets the value its own
// tile gives it: the same integers from the same pulled pyramid.
// A cell in LDS: bit 31 = has a value (its own or filled), bits 20..23 its evidence level, bits 0..19 q
constexpr int DD_TILE_MAX = 32, DD_REG_MAX = DD_TILE_MAX + 2;

__global__ void __launch_bounds__(256) k_dense_push(const FillArgs A, int tile_log) {
    __shared__ unsigned s_val[2][DD_REG_MAX * DD_REG_MAX];
    __shared__ uint8_t s_g[2][DD_REG_MAX * DD_REG_MAX];
    const Pyr &P = A.P;
    const int T = 1 << tile_log;
    const int tx0 = blockIdx.x * T, ty0 = blockIdx.y * T;
    int n_seed = 0, n_fill = 0, n_empty = 0, max_lv = 0;
    int cur = 0;
    // the region of the level above: origin and size (set when that level is processed)
    int px0 = 0, py0 = 0, pnx = 0, pny = 0;
    for (int l = P.L; l >= 0; l--) {
        const int x0 = (tx0 >> l) - 1, y0 = (ty0 >> l) - 1;
        const int nx = ((tx0 + T - 1) >> l) - (tx0 >> l) + 3, ny = ((ty0 + T - 1) >> l) - (ty0 >> l) + 3;
        const int nxt = cur ^ 1;
        for (int c = threadIdx.x; c < nx * ny; c += 256) {
            const int ix = c % nx, iy = c / nx;
            const int X = x0 + ix, Y = y0 + iy;
            unsigned val = 0;
            int g = 0;
            const bool inside = X >= 0 && Y >= 0 && X < P.w[l] && Y < P.h[l];
            const bool halo = ix == 0 || iy == 0 || ix == nx - 1 || iy == ny - 1;
            if (inside && !(l == 0 && halo)) {   // (nothing lies below level 0 that would read its halo)
                const size_t gc = (size_t) P.off[l] + (size_t) Y * P.w[l] + X;
                const unsigned pk = P.pack[gc];
                g = P.guide[gc];
                if ((pk >> 20) & 255) {
                    val = 0x80000000u | ((unsigned) l << 20) | (pk & DD_Q_MAX);
                } else if (l < P.L) {
                    // P3
                    const int ax = X >> 1, ay = Y >> 1;
                    const int bx = ax + ((X & 1) ? 1 : -1), by = ay + ((Y & 1) ? 1 : -1);
                    int S = 0, ev = 255;
                    long long qs = 0;
#pragma unroll
                    for (int d = 0; d < 4; d++) {
                        const int PX = (d & 1) ? bx : ax, PY = (d >> 1) ? by : ay;
                        const int bil = ((d & 1) ? 1 : 3) * ((d >> 1) ? 1 : 3);
                        if (PX < 0 || PY < 0 || PX >= P.w[l + 1] || PY >= P.h[l + 1]) continue;
                        const int jx = PX - px0, jy = PY - py0;
                        if (jx < 0 || jy < 0 || jx >= pnx || jy >= pny) continue;   // (cannot happen: the parents lie within the halo)
                        const unsigned pv = s_val[cur][jy * pnx + jx];
                        if (!(pv & 0x80000000u)) continue;
                        const int dg = g - (int) s_g[cur][jy * pnx + jx];
                        const int wt = bil * dd_E(dg < 0 ? -dg : dg);
                        S += wt;
                        qs += (long long) wt * (long long) (pv & DD_Q_MAX);
                        const int pe = (int) (pv >> 20) & 15;
                        ev = pe < ev ? pe : ev;
                    }
                    if (S > 0) val = 0x80000000u | ((unsigned) ev << 20) | (unsigned) ((qs + S / 2) / S);
                }
                if (l == 0) {
                    // P4
                    const size_t o = (size_t) Y * P.w[0] + X;
                    const int q = (int) (val & DD_Q_MAX), ev = (int) (val >> 20) & 15;
                    if ((pk >> 20) & 255) {
                        A.depth[o] = (float) (1.0 / (double) A.rho[o]);
                        A.level[o] = 0;
                        n_seed++;
                    } else if ((val & 0x80000000u) && q > 0) {
                        A.depth[o] = (float) (65536.0 / ((double) q * A.rho_ref));
                        A.level[o] = (uint8_t) ev;
                        n_fill++;
                        max_lv = ev > max_lv ? ev : max_lv;
                    } else {
                        A.depth[o] = 0.f;
                        A.level[o] = 255;
                        n_empty++;
                    }
                }
            }
            if (l > 0) {
                s_val[nxt][c] = val;
                s_g[nxt][c] = (uint8_t) g;
            }
        }
        __syncthreads();
        cur = nxt;
        px0 = x0; py0 = y0; pnx = nx; pny = ny;
    }
    n_seed = wave_sum(n_seed);
    n_fill = wave_sum(n_fill);
    n_empty = wave_sum(n_empty);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int o = __shfl_xor(max_lv, d);
        max_lv = o > max_lv ? o : max_lv;
    }
    if ((threadIdx.x & 63) == 0) {
        if (n_seed) atomicAdd(&A.counts[0], n_seed);
        if (n_fill) atomicAdd(&A.counts[1], n_fill);
        if (n_empty) atomicAdd(&A.counts[2], n_empty);
        if (max_lv) atomicMax(&A.counts[3], max_lv);
    }
}

}  // namespace

extern "C" int alva_depth_fuse(alva_ctx *ctx, const float *d_prev_rho, const uint8_t *d_prev_w, const double *h_T_cp12, const double *h_calib8,
                               int width, int height, int step, const float *d_depth, const uint8_t *d_conf, const uint8_t *d_code, int decay,
                               int w_max, double rel_tol, float *d_rho, uint8_t *d_w, uint8_t *d_src, int *h_info8) {
    ALVA_ARG(ctx && h_T_cp12 && h_calib8 && d_rho && d_w && d_src && h_info8);
    ALVA_ARG((d_prev_rho != nullptr) == (d_prev_w != nullptr));
    ALVA_ARG((d_depth != nullptr) == (d_conf != nullptr) && (d_depth != nullptr) == (d_code != nullptr));
    ALVA_ARG(width >= 1 && height >= 1 && width <= 16384 && height <= 16384);
    ALVA_ARG(step >= 1 && step <= 16 && width / step >= 1 && height / step >= 1);
    ALVA_ARG(decay >= 0 && decay <= 256 && w_max >= 1 && w_max <= 255 && std::isfinite(rel_tol) && rel_tol > 0);
    for (int i = 0; i < 8; i++) ALVA_ARG(std::isfinite(h_calib8[i]));
    for (int i = 0; i < 12; i++) ALVA_ARG(std::isfinite(h_T_cp12[i]));
    ALVA_ARG(h_calib8[0] > 0 && h_calib8[1] > 0);
    ALVA_ARG(d_rho != d_prev_rho && d_w != d_prev_w);
    FuseArgs A{};
    A.prev_rho = d_prev_rho; A.prev_w = d_prev_w;
    A.m_depth = d_depth; A.m_conf = d_conf; A.m_code = d_code;
    A.width = width; A.height = height; A.step = step;
    A.gw = width / step; A.gh = height / step;
    A.cam = AlvaCam{h_calib8[0], h_calib8[1], h_calib8[2], h_calib8[3], h_calib8[4], h_calib8[5], h_calib8[6], h_calib8[7]};
    memcpy(A.R, h_T_cp12, sizeof(A.R));
    memcpy(A.t, h_T_cp12 + 9, sizeof(A.t));
    A.decay = decay; A.w_max = w_max; A.rel_tol = rel_tol;
    A.rho = d_rho; A.w = d_w; A.src = d_src;
    const int n = A.gw * A.gh;
    int *pin = nullptr;
    int rc = alva_ctx_pinned(ctx, 64 * sizeof(int), (void **) &pin);
    if (rc) return rc;
    uint8_t *scr = nullptr;
    rc = alva_ctx_scratch(ctx, DD_SCRATCH_SLOT, 256 + (size_t) n * sizeof(unsigned long long), (void **) &scr);
    if (rc) return rc;
    A.counts = (int *) scr;
    A.keys = (unsigned long long *) (scr + 256);
    const int blocks = alva_divup(n, 256);
    hipLaunchKernelGGL(k_dense_clear, dim3(d_prev_rho ? blocks : 1), dim3(256), 0, ctx->stream, A.keys, d_prev_rho ? n : 0, A.counts, DD_SRCS);
    ALVA_LAUNCH_CHECK();
    if (d_prev_rho) {
        hipLaunchKernelGGL(k_dense_warp, dim3(blocks), dim3(256), 0, ctx->stream, A);
        ALVA_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_dense_fuse, dim3(blocks), dim3(256), 0, ctx->stream, A);
    ALVA_LAUNCH_CHECK();
    ALVA_HIP(hipMemcpyAsync(pin + 16, A.counts, DD_SRCS * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    ALVA_HIP(alva_stream_sync(ctx->stream));
    memcpy(h_info8, pin + 16, DD_SRCS * sizeof(int));
    h_info8[6] = A.gw;
    h_info8[7] = A.gh;
    return ALVA_OK;
}

extern "C" int alva_depth_fill(alva_ctx *ctx, const float *d_rho, const uint8_t *d_w, const uint8_t *d_cur, size_t pitch, int width, int height,
                               int step, double rho_ref, int max_level, float *d_depth, uint8_t *d_level, int *h_info4) {
    ALVA_ARG(ctx && d_rho && d_w && d_cur && d_depth && d_level && h_info4);
    ALVA_ARG(width >= 1 && height >= 1 && width <= 16384 && height <= 16384 && pitch >= (size_t) width);
    ALVA_ARG(step >= 1 && step <= 16 && width / step >= 1 && height / step >= 1);
    ALVA_ARG(std::isfinite(rho_ref) && rho_ref > 0 && max_level >= 1 && max_level <= DD_MAX_LEVEL);
    FillArgs A{};
    A.rho = d_rho; A.w = d_w; A.gray = d_cur; A.pitch = pitch; A.step = step; A.rho_ref = rho_ref;
    A.depth = d_depth; A.level = d_level;
    Pyr &P = A.P;
    P.L = max_level;
    P.w[0] = width / step;
    P.h[0] = height / step;
    P.off[0] = 0;
    for (int l = 0; l <= max_level; l++) {
        if (l) {
            P.w[l] = (P.w[l - 1] + 1) / 2;
            P.h[l] = (P.h[l - 1] + 1) / 2;
        }
        P.off[l + 1] = P.off[l] + (unsigned) P.w[l] * (unsigned) P.h[l];
    }
    const size_t cells = P.off[max_level + 1], pack_bytes = (cells * 4 + 255) / 256 * 256;
    int *pin = nullptr;
    int rc = alva_ctx_pinned(ctx, 64 * sizeof(int), (void **) &pin);
    if (rc) return rc;
    uint8_t *scr = nullptr;
    rc = alva_ctx_scratch(ctx, DD_SCRATCH_SLOT, 256 + pack_bytes + cells, (void **) &scr);
    if (rc) return rc;
    A.counts = (int *) scr;
    P.pack = (unsigned *) (scr + 256);
    P.guide = scr + 256 + pack_bytes;
    const int n0 = max_level < 4 ? max_level : 4;
    hipLaunchKernelGGL(k_dense_pull, dim3(alva_divup(P.w[0], 16), alva_divup(P.h[0], 16)), dim3(256), 0, ctx->stream, A, 0, n0);
    ALVA_LAUNCH_CHECK();
    if (max_level > 4) {
        hipLaunchKernelGGL(k_dense_pull, dim3(alva_divup(P.w[4], 16), alva_divup(P.h[4], 16)), dim3(256), 0, ctx->stream, A, 4, max_level - 4);
        ALVA_LAUNCH_CHECK();
    }
    const int tile_log = max_level < 5 ? max_level : 5;
    hipLaunchKernelGGL(k_dense_push, dim3(alva_divup(P.w[0], 1 << tile_log), alva_divup(P.h[0], 1 << tile_log)), dim3(256), 0, ctx->stream, A,
                       tile_log);
    ALVA_LAUNCH_CHECK();
    ALVA_HIP(hipMemcpyAsync(pin + 24, A.counts, 4 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    ALVA_HIP(alva_stream_sync(ctx->stream));
    memcpy(h_info4, pin + 24, 4 * sizeof(int));
    return ALVA_OK;
}
