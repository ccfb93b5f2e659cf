// Raycasting the scene volume: rays marched through the truncated signed distance volume of mesh.hip to its zero crossing
// (alva_mesh_raycast: explicit world rays; alva_mesh_raycast_pixels: the rays of image pixels from a pose, as a grid -- a depth image of
// the volume -- or as a list -- taps).  ARKit's raycast against mesh geometry, WebXR hit test on mesh-detection geometry, the per-frame
// surface prediction of every KinectFusion-style pipeline.  The reference has no counterpart, so the definition in include/alvaar_hip.h
// (R0-R8) is pinned by the numpy restatement tests/raycast_cases.py.  Geometry is IEEE double in the written order (compile with
// -ffp-contract=off); from the sample's fractions on everything is an integer, so the same inputs give the same bits.
//
// One launch, k_mesh_raycast, one lane per ray, 256 threads per workgroup:
//   rays     world rays and listed pixels in index order; in grid mode a wave is an 8 x 8 tile of grid pixels (partial tiles masked), so
//            that neighbouring lanes walk neighbouring cells and a wave's corner loads share cache lines
//   march    per sample the cell's eight corners are four rows of two adjacent voxels: four 16-bit loads of w, and only for a cell seen
//            whole four 32-bit loads of q.  The loop ends per lane; its length is bounded by the integer 2 N + 2, whatever the ray
//   counts   per lane, per wave, per workgroup, then one integer atomicAdd per count and one atomicMax per workgroup (as k_mesh_integrate)
// No LDS beyond the 24 words of that fold, and no workgroup waits for another.  Every index is clamped into the volume before it is used.
#include "common.hpp"
#include "camera_device.hpp"
#include "mesh_device.hpp"
#include "wave_utils.hpp"
#include <cmath>

namespace {

constexpr int RC_SCRATCH_SLOT = 9;   // (shared with the other synchronous stages)
constexpr int RC_N_MIN = 4, RC_N_MAX = 256;
constexpr int RC_MAX_RAYS = 1 << 20, RC_MAX_GRID = 1 << 22;
constexpr double RC_MIN_COS = 0.0872;   // the hit test's grazing gate

enum { RC_WORLD = 0, RC_LIST = 1, RC_GRID = 2 };

struct RaycastArgs {
    const int16_t *q;
    const uint8_t *w;
    int N, min_weight;
    double o[3], voxel;
    int mode, n;             // n: the rays (grid mode: gw gh)
    const double *rays;      // RC_WORLD: [n][6] = O, D
    const float *uv;         // RC_LIST: [n][2] raw pixels
    double R[9], t[3];       // X_world = R X_cam + t
    AlvaCam cam;
    int step, gw, gh, tiles_x;
    double t_near, t_far;
    float *t_out, *point, *normal;
    uint8_t *code;
    float *pose;             // [n][16] or null
    uint8_t *pose_ok;        // [n] or null
    int *counts;             // codes 0..4, then the largest sample count
};

struct RayResult {
    int code, samples;
    float t, p[3], n[3];
    double nd[3];   // R6's quotient before it is rounded to float (R7's y)
    bool has_n;     // code 0 with L2 > 0
};

__device__ __forceinline__ bool rc_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // (a NaN fails the comparison)

// R0 - R6 for one ray
__device__ __forceinline__ void mesh_march(const RaycastArgs &A, const double (&O)[3], const double (&D)[3], RayResult &r) {
    r.code = 2;
    r.samples = 0;
    r.t = 0.f;
    r.has_n = false;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        r.p[a] = r.n[a] = 0.f;
        r.nd[a] = 0.;
    }
    const int N = A.N;
    // R0
    const double m01 = fabs(D[0]) > fabs(D[1]) ? fabs(D[0]) : fabs(D[1]), dmax = m01 > fabs(D[2]) ? m01 : fabs(D[2]);
    if (!(rc_finite(O[0]) && rc_finite(O[1]) && rc_finite(O[2]) && rc_finite(D[0]) && rc_finite(D[1]) && rc_finite(D[2])) || dmax == 0.) {
        r.code = 4;
        return;
    }
    // R1
    double t0 = A.t_near, t1 = A.t_far;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const double lo = A.o[a] + 0.5 * A.voxel, hi = A.o[a] + ((double) N - 0.5) * A.voxel;
        if (D[a] == 0.) {
            if (!(lo <= O[a] && O[a] <= hi)) {
                r.code = 1;
                return;
            }
            continue;
        }
        const double ta = (lo - O[a]) / D[a], tb = (hi - O[a]) / D[a];
        const double tmin = ta < tb ? ta : tb, tmax = ta < tb ? tb : ta;
        t0 = t0 > tmin ? t0 : tmin;
        t1 = t1 < tmax ? t1 : tmax;
    }
    if (!(t0 <= t1)) {
        r.code = 1;
        return;
    }
    // R2
    const double dt = (0.5 * A.voxel) / dmax;
    const int NN = N * N, n_last = 2 * N + 1;
    bool have_prev = false;
    long long Fp = 0;
    for (int n = 0; n <= n_last; n++) {
        const double tn = t0 + (double) n * dt;
        if (!(tn <= t1)) break;
        r.samples = n + 1;
        // R3
        int ic[3], f[3];
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const double P = O[a] + tn * D[a];
            const double g = (P - A.o[a]) / A.voxel - 0.5;
            mesh_cell_axis(g, N, ic[a], f[a]);
        }
        const int base = (ic[2] * N + ic[1]) * N + ic[0];   // 0 <= base and base + NN + N + 1 <= N^3 - 1: ic <= N - 2
        const int row[4] = {base, base + N, base + NN, base + NN + N};
        bool valid = true;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            unsigned short ww;
            __builtin_memcpy(&ww, A.w + row[k], 2);
            valid = valid && (int) (ww & 255) >= A.min_weight && (int) (ww >> 8) >= A.min_weight;
        }
        if (!valid) {   // R4: unknown space is passed through, and no crossing is taken across it
            have_prev = false;
            continue;
        }
        int q[8];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            unsigned int qq;
            __builtin_memcpy(&qq, A.q + row[k], 4);
            q[2 * k] = (int) (short) (qq & 0xffffu);
            q[2 * k + 1] = (int) (short) (qq >> 16);
        }
        const int fx = f[0], gx = 256 - f[0];
        const long long fy = f[1], gy = 256 - f[1], fz = f[2], gz = 256 - f[2];
        const long long r00 = q[0] * gx + q[1] * fx, r10 = q[2] * gx + q[3] * fx, r01 = q[4] * gx + q[5] * fx, r11 = q[6] * gx + q[7] * fx;
        const long long F = (r00 * gy + r10 * fy) * gz + (r01 * gy + r11 * fy) * fz;   // (integers: the order of the sum does not matter)
        // R4
        if (have_prev && Fp > 0 && F <= 0) {
            // R5
            const double tp = t0 + (double) (n - 1) * dt;
            const double th = tp + dt * ((double) Fp / (double) (Fp - F));
            r.code = 0;
            r.t = (float) th;
#pragma unroll
            for (int a = 0; a < 3; a++) r.p[a] = (float) (O[a] + th * D[a]);
            // R6
            int g[3];
            const long long L2 = mesh_cell_gradient(q, g);
            if (L2 != 0) {
                const double len = sqrt((double) L2);
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    r.nd[a] = (double) g[a] / len;
                    r.n[a] = (float) r.nd[a];
                }
                r.has_n = true;
            }
            return;
        }
        if (have_prev && Fp <= 0 && F > 0) {
            r.code = 3;
            return;
        }
        have_prev = true;
        Fp = F;
    }
}

// R7: the pose of a hit (alva_hit_test's pose step with y = n); false when the gate refuses it, and then nothing is written
__device__ __forceinline__ bool mesh_ray_pose(const RaycastArgs &A, const double (&D)[3], const RayResult &r, float *pose) {
    if (!r.has_n) return false;
    const double *y = r.nd;
    const double nD = (y[0] * D[0] + y[1] * D[1]) + y[2] * D[2], Dl = sqrt((D[0] * D[0] + D[1] * D[1]) + D[2] * D[2]);
    if (!(fabs(nD) / Dl >= RC_MIN_COS)) return false;
    double x[3] = {0, 0, 0}, xl = 0;
    for (int col = 0; col < 2 && !(xl >= 1e-6); col++) {   // the camera's x axis in the surface; its y axis when x is along the normal
        const double a[3] = {A.R[col], A.R[3 + col], A.R[6 + col]};
        const double an = (a[0] * y[0] + a[1] * y[1]) + a[2] * y[2];
#pragma unroll
        for (int k = 0; k < 3; k++) x[k] = a[k] - an * y[k];
        xl = sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]);
    }
    if (!(xl >= 1e-6)) return false;   // (R_wc is not a rotation)
#pragma unroll
    for (int k = 0; k < 3; k++) x[k] = x[k] / xl;
    const double z[3] = {x[1] * y[2] - x[2] * y[1], x[2] * y[0] - x[0] * y[2], x[0] * y[1] - x[1] * y[0]};
#pragma unroll
    for (int k = 0; k < 3; k++) {
        pose[k] = (float) x[k];
        pose[4 + k] = (float) y[k];
        pose[8 + k] = (float) z[k];
        pose[12 + k] = r.p[k];
    }
    pose[3] = pose[7] = pose[11] = 0.f;
    pose[15] = 1.f;
    return true;
}

__global__ void __launch_bounds__(256) k_mesh_raycast(const RaycastArgs A) {
    __shared__ int s_n[4][6];
    // which ray, if any
    int ray = -1;
    float pu = 0.f, pv = 0.f;
    if (A.mode == RC_GRID) {
        const int tile = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
        const int gx = (tile % A.tiles_x) * 8 + (lane & 7), gy = (tile / A.tiles_x) * 8 + (lane >> 3);
        if (gx < A.gw && gy < A.gh) {
            ray = gy * A.gw + gx;
            pu = (float) (gx * A.step + A.step / 2);
            pv = (float) (gy * A.step + A.step / 2);
        }
    } else {
        const int i = blockIdx.x * 256 + threadIdx.x;
        if (i < A.n) {
            ray = i;
            if (A.mode == RC_LIST) {
                pu = A.uv[2 * (size_t) i];
                pv = A.uv[2 * (size_t) i + 1];
            }
        }
    }
    int cnt[6] = {0, 0, 0, 0, 0, 0};   // codes 0..4, samples
    if (ray >= 0) {
        double O[3], D[3];
        if (A.mode == RC_WORLD) {
            const double *p = A.rays + 6 * (size_t) ray;
#pragma unroll
            for (int a = 0; a < 3; a++) {
                O[a] = p[a];
                D[a] = p[3 + a];
            }
        } else {   // step 3 of alva_depth_sweep
            float uu, vv;
            alva_undistort_dev(A.cam, pu, pv, uu, vv);
            const double x = ((double) uu - A.cam.cx) / A.cam.fx, y = ((double) vv - A.cam.cy) / A.cam.fy;
#pragma unroll
            for (int a = 0; a < 3; a++) {
                D[a] = (A.R[3 * a] * x + A.R[3 * a + 1] * y) + A.R[3 * a + 2] * 1.;
                O[a] = A.t[a];
            }
        }
        RayResult r;
        mesh_march(A, O, D, r);
        A.t_out[ray] = r.t;
        A.code[ray] = (uint8_t) r.code;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            A.point[3 * (size_t) ray + a] = r.p[a];
            A.normal[3 * (size_t) ray + a] = r.n[a];
        }
        if (A.pose) {
            float pose[16];
#pragma unroll
            for (int k = 0; k < 16; k++) pose[k] = 0.f;
            const bool ok = r.code == 0 && mesh_ray_pose(A, D, r, pose);
#pragma unroll
            for (int k = 0; k < 16; k++) A.pose[16 * (size_t) ray + k] = pose[k];
            if (A.pose_ok) A.pose_ok[ray] = ok ? 1 : 0;
        }
#pragma unroll
        for (int c = 0; c < 5; c++) cnt[c] = r.code == c;
        cnt[5] = r.samples;
    }
    // R8 (integers: the order of the additions does not matter)
#pragma unroll
    for (int c = 0; c < 5; c++) {
        const int v = wave_sum(cnt[c]);
        if ((threadIdx.x & 63) == 0) s_n[threadIdx.x >> 6][c] = v;
    }
    int mx = cnt[5];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int o = __shfl_xor(mx, d);
        mx = o > mx ? o : mx;
    }
    if ((threadIdx.x & 63) == 0) s_n[threadIdx.x >> 6][5] = mx;
    __syncthreads();
    if (threadIdx.x < 5) {
        const int v = (s_n[0][threadIdx.x] + s_n[1][threadIdx.x]) + (s_n[2][threadIdx.x] + s_n[3][threadIdx.x]);
        if (v) atomicAdd(&A.counts[threadIdx.x], v);
    } else if (threadIdx.x == 5) {
        const int a = s_n[0][5] > s_n[1][5] ? s_n[0][5] : s_n[1][5], b = s_n[2][5] > s_n[3][5] ? s_n[2][5] : s_n[3][5];
        const int v = a > b ? a : b;
        if (v) atomicMax(&A.counts[5], v);
    }
}

// the volume's arguments, checked and copied; ALVA_ERR_ARG on a bad one
int raycast_volume(RaycastArgs &A, alva_ctx *ctx, const int16_t *d_q, const uint8_t *d_w, int N, const double *h_origin3, double voxel,
                   int min_weight, double t_near, double t_far, float *d_t, float *d_point3, float *d_normal3, uint8_t *d_code, int *h_info8) {
    ALVA_ARG(ctx && d_q && d_w && h_origin3 && d_t && d_point3 && d_normal3 && d_code && h_info8);
    ALVA_ARG(N >= RC_N_MIN && N <= RC_N_MAX);
    ALVA_ARG(std::isfinite(voxel) && voxel > 0);
    ALVA_ARG(min_weight >= 1 && min_weight <= 255);
    ALVA_ARG(std::isfinite(t_near) && !std::isnan(t_far) && t_near <= t_far);
    for (int i = 0; i < 3; i++) ALVA_ARG(std::isfinite(h_origin3[i]));
    A.q = d_q; A.w = d_w; A.N = N; A.min_weight = min_weight;
    memcpy(A.o, h_origin3, sizeof(A.o));
    A.voxel = voxel;
    A.t_near = t_near; A.t_far = t_far;
    A.t_out = d_t; A.point = d_point3; A.normal = d_normal3; A.code = d_code;
    return ALVA_OK;
}

// one launch, one wait; h_info8 (R8)
int raycast_run(alva_ctx *ctx, RaycastArgs &A, int blocks, int *h_info8) {
    int *pin = nullptr;
    int rc = alva_ctx_pinned(ctx, 64 * sizeof(int), (void **) &pin);
    if (rc) return rc;
    uint8_t *scr = nullptr;
    rc = alva_ctx_scratch(ctx, RC_SCRATCH_SLOT, 256, (void **) &scr);
    if (rc) return rc;
    A.counts = (int *) scr;
    ALVA_HIP(hipMemsetAsync(A.counts, 0, 8 * sizeof(int), ctx->stream));
    hipLaunchKernelGGL(k_mesh_raycast, dim3(blocks), dim3(256), 0, ctx->stream, A);
    ALVA_LAUNCH_CHECK();
    ALVA_HIP(hipMemcpyAsync(pin + 48, A.counts, 6 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    ALVA_HIP(alva_stream_sync(ctx->stream));
    h_info8[0] = A.n;
    memcpy(h_info8 + 1, pin + 48, 6 * sizeof(int));
    h_info8[7] = A.N;
    return ALVA_OK;
}

}  // namespace

extern "C" int alva_mesh_raycast(alva_ctx *ctx, const int16_t *d_q, const uint8_t *d_w, int N, const double *h_origin3, double voxel,
                                 int min_weight, int n_rays, const double *d_rays6, double t_near, double t_far, float *d_t, float *d_point3,
                                 float *d_normal3, uint8_t *d_code, int *h_info8) {
    RaycastArgs A{};
    const int rc = raycast_volume(A, ctx, d_q, d_w, N, h_origin3, voxel, min_weight, t_near, t_far, d_t, d_point3, d_normal3, d_code, h_info8);
    if (rc) return rc;
    ALVA_ARG(d_rays6 && n_rays >= 1 && n_rays <= RC_MAX_RAYS);
    A.mode = RC_WORLD;
    A.n = n_rays;
    A.rays = d_rays6;
    return raycast_run(ctx, A, alva_divup(n_rays, 256), h_info8);
}

extern "C" int alva_mesh_raycast_pixels(alva_ctx *ctx, const int16_t *d_q, const uint8_t *d_w, int N, const double *h_origin3, double voxel,
                                        int min_weight, const double *h_T_wc12, const double *h_calib8, int width, int height, int step,
                                        int n_px, const float *d_uv, double t_near, double t_far, float *d_t, float *d_point3,
                                        float *d_normal3, uint8_t *d_code, float *d_pose16, uint8_t *d_pose_ok, int *h_info8) {
    RaycastArgs A{};
    const int rc = raycast_volume(A, ctx, d_q, d_w, N, h_origin3, voxel, min_weight, t_near, t_far, d_t, d_point3, d_normal3, d_code, h_info8);
    if (rc) return rc;
    ALVA_ARG(h_T_wc12 && h_calib8);
    ALVA_ARG(width >= 1 && height >= 1 && width <= 16384 && height <= 16384);
    ALVA_ARG(step >= 1 && step <= 16 && width / step >= 1 && height / step >= 1);
    ALVA_ARG(d_pose16 || !d_pose_ok);
    for (int i = 0; i < 8; i++) ALVA_ARG(std::isfinite(h_calib8[i]));
    for (int i = 0; i < 12; i++) ALVA_ARG(std::isfinite(h_T_wc12[i]));
    ALVA_ARG(h_calib8[0] > 0 && h_calib8[1] > 0);
    memcpy(A.R, h_T_wc12, sizeof(A.R));
    memcpy(A.t, h_T_wc12 + 9, sizeof(A.t));
    A.cam = AlvaCam{h_calib8[0], h_calib8[1], h_calib8[2], h_calib8[3], h_calib8[4], h_calib8[5], h_calib8[6], h_calib8[7]};
    A.step = step; A.gw = width / step; A.gh = height / step;
    A.pose = d_pose16; A.pose_ok = d_pose_ok;
    int blocks;
    if (d_uv) {
        ALVA_ARG(n_px >= 1 && n_px <= RC_MAX_RAYS);
        A.mode = RC_LIST;
        A.n = n_px;
        A.uv = d_uv;
        blocks = alva_divup(n_px, 256);
    } else {
        ALVA_ARG((long long) A.gw * A.gh <= RC_MAX_GRID);
        A.mode = RC_GRID;
        A.n = A.gw * A.gh;
        A.tiles_x = alva_divup(A.gw, 8);
        blocks = alva_divup(A.tiles_x * alva_divup(A.gh, 8), 4);
    }
    return raycast_run(ctx, A, blocks, h_info8);
}
