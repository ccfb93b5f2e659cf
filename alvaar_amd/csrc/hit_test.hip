// Hit test: the anchor pose on the surface under an image point (the hit test of WebXR / ARCore; the reference has no counterpart, so
// the definition in include/alvaar_hip.h is pinned by the numpy restatement tests/hit_cases.py).
//
// Per ray (= tap): undistort the tap, select the map points that project within radius_px of it (camera-front only, ascending index,
// at most HIT_CAP), LMedS over planes through 3 hashed samples of the selection (score = the rank m/2 distance, scale-free), inliers
// within 2.5 x 1.4826 x that score, and the inliers' moments about the winning sample's first point.  The 3 x 3 eigenvector, the ray /
// plane intersection and the pose are host work on those ten sums.  All decisions are IEEE double in the written operation order
// (compile with -ffp-contract=off), so a given map, pose and seed give the same bits on every call.
//
// One launch per call, one 512-thread workgroup per ray:
//   selection   strided pass over the n points, ballot + prefix into LDS (SoA, 3 x 2048 doubles = 48 KB), index order kept
//   hypotheses  striped over the 8 waves; a wave holds its m distances in registers (32 per lane) and finds the rank-k one exactly by
//               radix select over the bit patterns of the non-negative doubles (8 byte passes, a 256-bin LDS histogram per wave)
//   winner      argmin over (score, iteration) of the waves' bests
//   moments     strided pass over the selection, 10 sums reduced with __shfl_xor, then over the waves in a fixed order
// The distances are not staged in LDS: 8 waves x 2048 doubles (128 KB) beside the points would pass the 160 KB of a CU.
#include "common.hpp"
#include "camera_device.hpp"
#include "plane_fit.hpp"
#include "slam/se3.hpp"
#include <cmath>

namespace {

constexpr int HIT_NT = 512, HIT_WAVES = HIT_NT / 64, HIT_CAP = 2048, HIT_PER_LANE = HIT_CAP / 64, HIT_MAX_RAYS = 16;
constexpr int HIT_MIN_SELECTED = 24, HIT_MIN_INLIERS = 16;
constexpr double HIT_INLIER_FACTOR = 3.7065;   // 2.5 x 1.4826, the LMedS scale
constexpr double HIT_MIN_COS = 0.0872;         // cos 85 deg: a ray under 5 deg from grazing

struct HitRecord {   // one per ray, in pinned memory
    double mom[10];  // n_in | sum x (3) | sum x x^T upper triangle (6), x = Q_i - q0
    double q0[3];
    double score;
    float uu, vv;    // the undistorted tap
    int m, n_sel, best_it, pad;
};

struct HitArgs {
    const double *pts;   // [n][3]
    int n, iters;
    double t[3], R[9];   // Twc: translation, R_wc row-major
    AlvaCam cam;
    float uv[2 * HIT_MAX_RAYS];
    double radius2;
    uint32_t seed;
    const uint32_t *rand3;   // [iters][3] explicit sample words (pinned), or null
    HitRecord *out;
};

// the plane of hypothesis `it` through three of the m selected points: false when two indices coincide or the points are collinear
__device__ __forceinline__ bool hit_hypothesis(const HitArgs &A, int it, int m, const double *Qx, const double *Qy, const double *Qz,
                                               double (&q0)[3], double (&nr)[3]) {
    int idx[3];
    if (!alva_sample3(A.rand3, A.seed, (uint32_t) it, m, idx)) return false;
    const double p0[3] = {Qx[idx[0]], Qy[idx[0]], Qz[idx[0]]}, p1[3] = {Qx[idx[1]], Qy[idx[1]], Qz[idx[1]]};
    const double p2[3] = {Qx[idx[2]], Qy[idx[2]], Qz[idx[2]]};
    return plane_through3(p0, p1, p2, q0, nr);
}

__global__ void __launch_bounds__(HIT_NT) k_hit_test(const HitArgs A) {
    __shared__ double Qx[HIT_CAP], Qy[HIT_CAP], Qz[HIT_CAP];
    __shared__ int s_hist[HIT_WAVES][256];
    __shared__ int s_wcnt[2][HIT_WAVES];
    __shared__ double s_score[HIT_WAVES];
    __shared__ int s_it[HIT_WAVES];
    __shared__ double s_red[HIT_WAVES][10];
    __shared__ float s_uv[2];
    const int ray = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform for the compiler too: a hypothesis is scalar control flow
    HitRecord *out = A.out + ray;
    if (tid == 0) {
        float uu, vv;
        alva_undistort_dev(A.cam, A.uv[2 * ray], A.uv[2 * ray + 1], uu, vv);
        s_uv[0] = uu;
        s_uv[1] = vv;
    }
    __syncthreads();
    const double uu = (double) s_uv[0], vv = (double) s_uv[1];

    // ---- selection, compacted in index order; what lies past HIT_CAP is counted and not kept
    int total = 0;
    for (int base = 0, par = 0; base < A.n; base += HIT_NT, par ^= 1) {
        const int i = base + tid;
        bool sel = false;
        double px = 0, py = 0, pz = 0;
        if (i < A.n) {
            const double *p = A.pts + 3 * (size_t) i;
            px = p[0]; py = p[1]; pz = p[2];
            const double d0 = px - A.t[0], d1 = py - A.t[1], d2 = pz - A.t[2];
            const double cx = (A.R[0] * d0 + A.R[3] * d1) + A.R[6] * d2;   // R_wc^T (P - t)
            const double cy = (A.R[1] * d0 + A.R[4] * d1) + A.R[7] * d2;
            const double cz = (A.R[2] * d0 + A.R[5] * d1) + A.R[8] * d2;
            if (cz > 0) {
                const double eu = (A.cam.fx * cx / cz + A.cam.cx) - uu, ev = (A.cam.fy * cy / cz + A.cam.cy) - vv;
                sel = eu * eu + ev * ev <= A.radius2;
            }
        }
        const int pos = block_compact_in_order<HIT_WAVES>(sel, s_wcnt, par, total);
        if (sel && pos < HIT_CAP) {
            Qx[pos] = px; Qy[pos] = py; Qz[pos] = pz;
        }
    }
    const int m = total < HIT_CAP ? total : HIT_CAP;
    // the last 64-point slice is filled up with NaNs: a wave computes its distances a whole slice at a time, and a NaN distance sorts
    // behind every real one, where the rank m / 2 never reaches
    if (tid < 64 && m + tid < (m + 63) / 64 * 64) Qx[m + tid] = Qy[m + tid] = Qz[m + tid] = __longlong_as_double(0x7ff8000000000000ll);
    __syncthreads();
    if (tid == 0) {
        out->uu = s_uv[0]; out->vv = s_uv[1];
        out->m = m; out->n_sel = total; out->best_it = -1; out->pad = 0;
        out->score = 0;
        out->q0[0] = out->q0[1] = out->q0[2] = 0;
    }
    if (tid < 10) out->mom[tid] = 0;
    if (m < HIT_MIN_SELECTED) return;

    // ---- hypotheses: iteration base + wave on wave `wave`; every wave runs every round (the barriers are workgroup-wide)
    const int k = m / 2;
    double best_score = INFINITY;
    int best_it = -1;
    for (int base = 0; base < A.iters; base += HIT_WAVES) {
        const int it = base + wave;
        double q0[3] = {0, 0, 0}, nr[3] = {0, 0, 0};
        const bool ok = it < A.iters && hit_hypothesis(A, it, m, Qx, Qy, Qz, q0, nr);
        unsigned long long key[HIT_PER_LANE];
#pragma unroll
        for (int j = 0; j < HIT_PER_LANE; j++) {
            const int i = lane + 64 * j;
            key[j] = ~0ull;
            if (ok && 64 * j < m) {
                const double d = fabs(((Qx[i] - q0[0]) * nr[0] + (Qy[i] - q0[1]) * nr[1]) + (Qz[i] - q0[2]) * nr[2]);
                key[j] = (unsigned long long) __double_as_longlong(d);
            }
        }
        // rank k among the m distances: radix select, one byte per pass from the top (non-negative doubles order like their bit patterns;
        // the NaNs of the padding are counted too, behind them all)
        unsigned long long prefix = 0, mask = 0;
        int kk = k;
        for (int pass = 7; pass >= 0; pass--) {
            const int sh = 8 * pass;
#pragma unroll
            for (int q = 0; q < 4; q++) s_hist[wave][lane + 64 * q] = 0;
            __syncthreads();
            if (ok) {
#pragma unroll
                for (int j = 0; j < HIT_PER_LANE; j++)
                    if (64 * j < m && (key[j] & mask) == prefix) atomicAdd(&s_hist[wave][(int) ((key[j] >> sh) & 255ull)], 1);
            }
            __syncthreads();
            if (ok) {   // the lane whose bins hold rank kk names the byte
                int bin;
                wave_radix_locate(s_hist[wave], lane, kk, bin, kk);
                prefix |= (unsigned long long) bin << sh;
            }
            mask |= 255ull << sh;
        }
        const double score = __longlong_as_double((long long) prefix);
        if (ok && score < best_score) {   // a wave's iterations ascend: the first of equal scores stays
            best_score = score;
            best_it = it;
        }
    }
    if (lane == 0) {
        s_score[wave] = best_score;
        s_it[wave] = best_it;
    }
    __syncthreads();
    double win_score = INFINITY;
    int win_it = -1;
#pragma unroll
    for (int w = 0; w < HIT_WAVES; w++) {
        const double sc = s_score[w];
        const int iw = s_it[w];
        if (iw >= 0 && (sc < win_score || (sc == win_score && iw < win_it))) {
            win_score = sc;
            win_it = iw;
        }
    }
    if (win_it < 0) return;   // no hypothesis survived: the record says best_it = -1

    // ---- inliers of the winner and their moments about its first sample
    double q0[3], nr[3];
    (void) hit_hypothesis(A, win_it, m, Qx, Qy, Qz, q0, nr);
    const double thr = HIT_INLIER_FACTOR * win_score;
    double acc[10];
#pragma unroll
    for (int c = 0; c < 10; c++) acc[c] = 0;
    for (int i = tid; i < m; i += HIT_NT) {
        const double x = Qx[i] - q0[0], y = Qy[i] - q0[1], z = Qz[i] - q0[2];
        if (fabs((x * nr[0] + y * nr[1]) + z * nr[2]) <= thr) moments_accumulate(x, y, z, acc);
    }
    const double v = block_sum_in_wave_order<10, HIT_WAVES>(acc, s_red);
    if (tid < 10) out->mom[tid] = v;
    if (tid == 0) {
        out->best_it = win_it;
        out->score = win_score;
        out->q0[0] = q0[0]; out->q0[1] = q0[1]; out->q0[2] = q0[2];
    }
}

// refit, intersection and pose of one ray from its record; returns the code
int hit_finish(const HitRecord &r, const double t[3], const double R[9], const double *calib, float *pose16, int *n_in_out) {
    *n_in_out = 0;
    if (r.m < HIT_MIN_SELECTED) return 1;
    if (r.best_it < 0) return 2;
    const int n_in = (int) r.mom[0];
    *n_in_out = n_in;
    if (n_in < HIT_MIN_INLIERS) return 3;
    double mu[3], S[6], nrm[3];
    moments_to_centroid_cov(r.mom, mu, S);
    const double C[9] = {S[0], S[1], S[2], S[1], S[3], S[4], S[2], S[4], S[5]};
    smallest_eigvec<3>(C, nrm);
    const double c[3] = {r.q0[0] + mu[0], r.q0[1] + mu[1], r.q0[2] + mu[2]};
    face_towards(nrm, c, t);
    const double fx = calib[0], fy = calib[1], cx = calib[2], cy = calib[3];
    double dc[3] = {((double) r.uu - cx) / fx, ((double) r.vv - cy) / fy, 1.0};
    const double dl = std::sqrt(dc[0] * dc[0] + dc[1] * dc[1] + dc[2] * dc[2]);
    for (double &v: dc) v /= dl;
    double dw[3], den = 0, num = 0;
    for (int i = 0; i < 3; i++) {
        dw[i] = R[3 * i] * dc[0] + R[3 * i + 1] * dc[1] + R[3 * i + 2] * dc[2];
        den += nrm[i] * dw[i];
        num += nrm[i] * (c[i] - t[i]);
    }
    if (!(std::fabs(den) >= HIT_MIN_COS)) return 4;
    const double lam = num / den;
    if (!(lam > 0)) return 4;
    double x[3], xl = 0;
    for (int col = 0; col < 2 && !(xl >= 1e-6); col++) {   // the camera's x axis in the plane; its y axis when x is along the normal
        const double a[3] = {R[col], R[3 + col], R[6 + col]};
        const double an = a[0] * nrm[0] + a[1] * nrm[1] + a[2] * nrm[2];
        for (int k = 0; k < 3; k++) x[k] = a[k] - an * nrm[k];
        xl = std::sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
    }
    for (double &v: x) v /= xl;
    const double z[3] = {x[1] * nrm[2] - x[2] * nrm[1], x[2] * nrm[0] - x[0] * nrm[2], x[0] * nrm[1] - x[1] * nrm[0]};
    for (int row = 0; row < 3; row++) {
        pose16[row] = (float) x[row];
        pose16[4 + row] = (float) nrm[row];
        pose16[8 + row] = (float) z[row];
        pose16[12 + row] = (float) (t[row] + lam * dw[row]);
    }
    pose16[3] = pose16[7] = pose16[11] = 0.f;
    pose16[15] = 1.f;
    return 0;
}

}  // namespace

extern "C" int alva_hit_test(alva_ctx *ctx, const double *d_points, int n, const double *h_pose7_twc, const double *h_calib8, int n_rays,
                             const float *h_uv, float radius_px, int num_iterations, uint32_t seed, const uint32_t *h_rand3, float *h_pose16,
                             int *h_info8, double *h_moments) {
    ALVA_ARG(ctx && h_pose7_twc && h_calib8 && h_uv && h_pose16 && h_info8);
    ALVA_ARG(n_rays >= 1 && n_rays <= HIT_MAX_RAYS && num_iterations >= 1 && num_iterations <= 4096 && radius_px > 0 && n >= 0);
    ALVA_ARG(d_points || n == 0);
    memset(h_info8, 0, (size_t) n_rays * 8 * sizeof(int));
    if (h_moments) memset(h_moments, 0, (size_t) n_rays * 10 * sizeof(double));
    if (n == 0) {
        for (int r = 0; r < n_rays; r++) {
            h_info8[8 * r] = 1;
            h_info8[8 * r + 2] = -1;
        }
        return ALVA_OK;
    }
    // pinned: explicit sample words (tests) | one record per ray
    const size_t off_rec = h_rand3 ? ((size_t) num_iterations * 12 + 255) / 256 * 256 : 0;
    uint8_t *pin = nullptr;
    const int rc = alva_ctx_pinned(ctx, off_rec + (size_t) n_rays * sizeof(HitRecord), (void **) &pin);
    if (rc) return rc;
    if (h_rand3) memcpy(pin, h_rand3, (size_t) num_iterations * 12);
    HitArgs A{};
    A.pts = d_points;
    A.n = n;
    A.iters = num_iterations;
    memcpy(A.t, h_pose7_twc, sizeof(A.t));
    alva_slam::quat_to_rot(h_pose7_twc + 3, A.R);
    A.cam = AlvaCam{h_calib8[0], h_calib8[1], h_calib8[2], h_calib8[3], h_calib8[4], h_calib8[5], h_calib8[6], h_calib8[7]};
    memcpy(A.uv, h_uv, (size_t) n_rays * 2 * sizeof(float));
    A.radius2 = (double) radius_px * (double) radius_px;
    A.seed = seed;
    A.rand3 = h_rand3 ? (const uint32_t *) pin : nullptr;
    A.out = (HitRecord *) (pin + off_rec);
    hipLaunchKernelGGL(k_hit_test, dim3(n_rays), dim3(HIT_NT), 0, ctx->stream, A);
    ALVA_LAUNCH_CHECK();
    ALVA_HIP(alva_stream_sync(ctx->stream));
    for (int r = 0; r < n_rays; r++) {
        HitRecord rec;
        memcpy(&rec, A.out + r, sizeof(rec));
        int *info = h_info8 + 8 * r, n_in = 0;
        info[0] = hit_finish(rec, A.t, A.R, h_calib8, h_pose16 + 16 * r, &n_in);
        info[1] = rec.m;
        info[2] = rec.best_it;
        info[3] = n_in;
        info[4] = rec.n_sel;
        if (h_moments) memcpy(h_moments + 10 * r, rec.mom, sizeof(rec.mom));
    }
    return ALVA_OK;
}
