// Depth from motion: a per-frame depth image for occlusion (the depth of ARCore's Depth API on a phone without a depth sensor; the
// reference has no counterpart, so the definition in include/alvaar_hip.h is pinned by the numpy restatement tests/depth_cases.py).
//
// A plane sweep over inverse depth: every grid pixel's patch of the current image is compared, under D depth hypotheses, with the patch
// the reference image shows where the hypothesis says it must be (zero-mean SAD on integers).  The geometry is IEEE double in the
// written operation order (compile with -ffp-contract=off), the costs are integers, so the same inputs give the same bits.
//
// One launch, one wave per grid pixel:
//   patch       the N = (2r+1)^2 gray values, their sum, N c_i - sum C and the texture measure (lanes over patch pixels, integer sums)
//   rays        q_i = R_rc K^-1 (undistorted pixel i, 1), once per wave, in LDS (3 x 81 doubles); every hypothesis reads them as a
//               broadcast (all lanes the same address)
//   hypotheses  lane l takes k = l, l + 64, ...: N projections into the reference image, the bilinear samples go to LDS as bytes
//               ([i][lane]: a lane's own column, no conflicts between lanes beyond the four that share a bank word), then the cost,
//               which needs the samples' sum first; costs stay in LDS for the neighbours the refinement reads
//   winner      argmin as a 64-bit (cost, k) key through the wave, then the second minimum away from it
// A second one-workgroup launch counts the codes into pinned memory.
#include "common.hpp"
#include "camera_device.hpp"
#include "wave_utils.hpp"
#include <cmath>

namespace {

constexpr int DS_MAX_N = 81, DS_MAX_D = 256, DS_CODES = 6;

struct DepthArgs {
    const uint8_t *cur, *ref;
    size_t pitch;
    int width, height, step, D, r, gw, gh;
    AlvaCam cam;
    double R[9], t[3];   // X_ref = R X_cur + t
    double rho_min, rho_max;
    int tex_thr;         // min_texture N N
    int min_conf;
    float *depth;
    uint8_t *conf, *code;
    int *best;           // [gh gw 4] or null
};

__device__ __forceinline__ void depth_write(const DepthArgs &A, int g, int code, float depth, int conf, int kb, int best, int second, int T) {
    A.depth[g] = depth;
    A.conf[g] = (uint8_t) conf;
    A.code[g] = (uint8_t) code;
    if (A.best) {
        int *b = A.best + 4 * (size_t) g;
        b[0] = kb; b[1] = best; b[2] = second; b[3] = T;
    }
}

__global__ void __launch_bounds__(64) k_depth_sweep(const DepthArgs A) {
    __shared__ double s_q[3][DS_MAX_N];
    __shared__ int s_cdev[DS_MAX_N];
    __shared__ int s_cost[DS_MAX_D];
    __shared__ uint8_t s_smp[DS_MAX_N * 64];
    const int lane = threadIdx.x, g = blockIdx.x;
    const int gx = g % A.gw, gy = g / A.gw;
    const int u = gx * A.step + A.step / 2, v = gy * A.step + A.step / 2;
    const int r = A.r, side = 2 * r + 1, N = side * side, D = A.D;

    // ---- 1 patch
    if (u - r < 0 || u + r > A.width - 1 || v - r < 0 || v + r > A.height - 1) {
        if (lane == 0) depth_write(A, g, 1, 0.f, 0, -1, -1, -1, 0);
        return;
    }
    int part = 0;
    for (int i = lane; i < N; i += 64) {
        const int c = A.cur[(size_t) (v + i / side - r) * A.pitch + (u + i % side - r)];
        s_cdev[i] = c;
        part += c;
    }
    const int sumC = wave_sum(part);
    // ---- 2 texture
    part = 0;
    for (int i = lane; i < N; i += 64) {
        const int d = N * s_cdev[i] - sumC;
        s_cdev[i] = d;
        part += d < 0 ? -d : d;
    }
    const int T = wave_sum(part);
    if (T < A.tex_thr) {
        if (lane == 0) depth_write(A, g, 2, 0.f, 0, -1, -1, -1, T);
        return;
    }
    // ---- 3 rays
    for (int i = lane; i < N; i += 64) {
        float uu, vv;
        alva_undistort_dev(A.cam, (float) (u + i % side - r), (float) (v + i / side - r), uu, vv);
        const double x = ((double) uu - A.cam.cx) / A.cam.fx, y = ((double) vv - A.cam.cy) / A.cam.fy;
        s_q[0][i] = (A.R[0] * x + A.R[1] * y) + A.R[2] * 1.;
        s_q[1][i] = (A.R[3] * x + A.R[4] * y) + A.R[5] * 1.;
        s_q[2][i] = (A.R[6] * x + A.R[7] * y) + A.R[8] * 1.;
    }
    __syncthreads();

    // ---- 4 hypotheses
    const float wmax = (float) (A.width - 1), hmax = (float) (A.height - 1);
    unsigned long long mine = ~0ull;
    for (int k = lane; k < D; k += 64) {
        const double rho = A.rho_min + ((A.rho_max - A.rho_min) * (double) k) / (double) (D - 1);
        const double tx = rho * A.t[0], ty = rho * A.t[1], tz = rho * A.t[2];
        bool valid = true;
        int sumS = 0;
        for (int i = 0; i < N && valid; i++) {
            const double Px = s_q[0][i] + tx, Py = s_q[1][i] + ty, Pz = s_q[2][i] + tz;
            if (!(Pz > 1e-9)) {
                valid = false;
                break;
            }
            float up, vp;
            alva_project_dist_dev(A.cam, Px, Py, Pz, up, vp);
            const float fu = floorf(up), fv = floorf(vp);
            if (!(0.f <= fu && fu + 1.f <= wmax && 0.f <= fv && fv + 1.f <= hmax)) {   // (a NaN fails every comparison)
                valid = false;
                break;
            }
            const int a = (int) rintf((up - fu) * 32.f), b = (int) rintf((vp - fv) * 32.f);
            const uint8_t *p = A.ref + (size_t) (int) fv * A.pitch + (int) fu;
            const int g00 = p[0], g01 = p[1], g10 = p[A.pitch], g11 = p[A.pitch + 1];
            const int s = (g00 * (32 - a) * (32 - b) + g01 * a * (32 - b) + g10 * (32 - a) * b + g11 * a * b + 512) >> 10;
            s_smp[i * 64 + lane] = (uint8_t) s;
            sumS += s;
        }
        int cost = -1;
        if (valid) {
            cost = 0;
            for (int i = 0; i < N; i++) {
                const int d = s_cdev[i] - (N * (int) s_smp[i * 64 + lane] - sumS);
                cost += d < 0 ? -d : d;
            }
            const unsigned long long key = argmin_key(cost, k);
            mine = key < mine ? key : mine;
        }
        s_cost[k] = cost;
    }
    __syncthreads();

    // ---- 5 winner
    const unsigned long long win = wave_min(mine);
    if (win == ~0ull) {
        if (lane == 0) depth_write(A, g, 3, 0.f, 0, -1, -1, -1, T);
        return;
    }
    const int kb = (int) (unsigned) (win & 0xffffffffull), best = (int) (unsigned) (win >> 32);
    unsigned long long other = ~0ull;
    for (int k = lane; k < D; k += 64) {
        const int c = s_cost[k];
        if (c >= 0 && (k - kb >= 2 || kb - k >= 2)) {
            const unsigned long long key = argmin_key(c, 0);
            other = key < other ? key : other;
        }
    }
    other = wave_min(other);
    if (lane != 0) return;
    const int second = other == ~0ull ? -1 : (int) (unsigned) (other >> 32);
    const int conf = second < 0 ? 0 : 255 - (255 * best) / (second > 1 ? second : 1);
    // ---- 6 refinement
    double off = 0.;
    if (kb > 0 && kb < D - 1) {
        const int cm = s_cost[kb - 1], cp = s_cost[kb + 1];
        if (cm >= 0 && cp >= 0) {
            const int den = cm - 2 * best + cp;
            if (den > 0) off = (double) (cm - cp) / (double) (2 * den);
        }
    }
    const double rho = A.rho_min + ((A.rho_max - A.rho_min) * ((double) kb + off)) / (double) (D - 1);
    // ---- 7 codes
    const int code = (kb == 0 || kb == D - 1) ? 5 : conf < A.min_conf ? 4 : 0;
    depth_write(A, g, code, code == 0 ? (float) (1.0 / rho) : 0.f, conf, kb, best, second, T);
}

// the count of every code over the n grid pixels, into pinned memory
__global__ void __launch_bounds__(1024) k_depth_count(const uint8_t *code, int n, int *out) {
    __shared__ int s_cnt[DS_CODES];
    if (threadIdx.x < DS_CODES) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    int cnt[DS_CODES] = {0, 0, 0, 0, 0, 0};   // per thread in registers, then per wave: the bins are few, LDS atomics on them would queue up
    for (int i = threadIdx.x; i < n; i += 1024) {
        const int c = code[i];
#pragma unroll
        for (int k = 0; k < DS_CODES; k++) cnt[k] += c == k;
    }
#pragma unroll
    for (int k = 0; k < DS_CODES; k++) {
        const int w = wave_sum(cnt[k]);
        if ((threadIdx.x & 63) == 0 && w) atomicAdd(&s_cnt[k], w);
    }
    __syncthreads();
    if (threadIdx.x < DS_CODES) out[threadIdx.x] = s_cnt[threadIdx.x];
}

}  // namespace

extern "C" int alva_depth_sweep(alva_ctx *ctx, const uint8_t *d_cur, const uint8_t *d_ref, size_t pitch, int width, int height,
                                const double *h_calib8, const double *h_T_rc12, int step, int num_hyp, double rho_min, double rho_max,
                                int patch_radius, int min_texture, int min_conf, float *d_depth, uint8_t *d_conf, uint8_t *d_code, int *h_info8,
                                int *d_best) {
    ALVA_ARG(ctx && d_cur && d_ref && h_calib8 && h_T_rc12 && d_depth && d_conf && d_code && h_info8);
    ALVA_ARG(width >= 4 && width % 4 == 0 && height >= 1 && width <= 16384 && height <= 16384 && pitch >= (size_t) width);
    ALVA_ARG(step >= 1 && step <= 16 && width / step >= 1 && height / step >= 1);
    ALVA_ARG(num_hyp >= 8 && num_hyp <= DS_MAX_D && patch_radius >= 1 && patch_radius <= 4);
    ALVA_ARG(std::isfinite(rho_min) && std::isfinite(rho_max) && rho_min > 0 && rho_min < rho_max);
    ALVA_ARG(min_texture >= 0 && min_texture <= 255 && min_conf >= 0 && min_conf <= 255);
    for (int i = 0; i < 8; i++) ALVA_ARG(std::isfinite(h_calib8[i]));
    for (int i = 0; i < 12; i++) ALVA_ARG(std::isfinite(h_T_rc12[i]));
    ALVA_ARG(h_calib8[0] > 0 && h_calib8[1] > 0);
    int *pin = nullptr;
    const int rc = alva_ctx_pinned(ctx, 8 * sizeof(int), (void **) &pin);
    if (rc) return rc;
    DepthArgs A{};
    A.cur = d_cur; A.ref = d_ref; A.pitch = pitch;
    A.width = width; A.height = height; A.step = step; A.D = num_hyp; A.r = patch_radius;
    A.gw = width / step; A.gh = height / step;
    A.cam = AlvaCam{h_calib8[0], h_calib8[1], h_calib8[2], h_calib8[3], h_calib8[4], h_calib8[5], h_calib8[6], h_calib8[7]};
    memcpy(A.R, h_T_rc12, sizeof(A.R));
    memcpy(A.t, h_T_rc12 + 9, sizeof(A.t));
    A.rho_min = rho_min; A.rho_max = rho_max;
    const int N = (2 * patch_radius + 1) * (2 * patch_radius + 1);
    A.tex_thr = min_texture * N * N;
    A.min_conf = min_conf;
    A.depth = d_depth; A.conf = d_conf; A.code = d_code; A.best = d_best;
    const int n = A.gw * A.gh;
    hipLaunchKernelGGL(k_depth_sweep, dim3(n), dim3(64), 0, ctx->stream, A);
    ALVA_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_depth_count, dim3(1), dim3(1024), 0, ctx->stream, d_code, n, pin);
    ALVA_LAUNCH_CHECK();
    ALVA_HIP(alva_stream_sync(ctx->stream));
    memcpy(h_info8, pin, DS_CODES * sizeof(int));
    h_info8[6] = A.gw;
    h_info8[7] = A.gh;
    return ALVA_OK;
}
