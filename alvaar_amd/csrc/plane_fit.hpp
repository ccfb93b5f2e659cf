// The pieces that the plane fitters share: alva_find_plane (find_plane.hip), alva_hit_test (hit_test.hip), alva_detect_planes
// (detect_planes.hip) and alva_track_planes (track_planes.hip).  Every one of them is order-sensitive -- the tests hold discrete outputs exactly and identical calls to the bit,
// and the hit test and plane detection draw from ONE sample stream (tests/plane_cases.py) -- so each has one definition, here.
// The host-compilable part (no HIP needed) is checked by tests/cpp/plane_fit_host.cpp.
//
// What deliberately stays with its caller:
//   plane_of, plane_dist (find_plane.hip)   they replay the reference's float arithmetic and its 4-vector normalisation, and are pinned
//                                           against the repaired reference
//   the two radix-select drivers            different key widths and storage: workgroup-wide over float keys in LDS (k_plane_hyp), per
//                                           wave over double keys in registers (k_hit_test).  They share wave_radix_locate only
// pl_rotate and plane_frame_from_moments (the 12-sweep Jacobi and the frame built from it) are shared by k_plane_round and
// k_track_claim: register-resident, a fixed sweep count -- another algorithmic form than smallest_eigvec by design; merging the two
// would change bits
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PLANE_FIT_HD __host__ __device__ inline
#else
#define PLANE_FIT_HD inline
#endif

// ---- the sample stream
PLANE_FIT_HD uint32_t alva_hash32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du;
    x ^= x >> 15; x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
// a 32-bit word to an index in [0, m)
PLANE_FIT_HD int alva_sample_index(uint32_t w, int m) { return (int) (((uint64_t) w * (uint64_t) m) >> 32); }

// the three indices in [0, m) of hypothesis k of the stream: from the explicit words rand3[3 k ..] when given, otherwise hashed from the
// seed.  False when two of them coincide
PLANE_FIT_HD bool alva_sample3(const uint32_t *rand3, uint32_t seed, uint32_t k, int m, int (&idx)[3]) {
    for (int j = 0; j < 3; j++) {
        const uint32_t w = rand3 ? rand3[3 * (size_t) k + j] : alva_hash32(seed ^ ((3u * k + (uint32_t) j) * 0x9E3779B9u));
        idx[j] = alva_sample_index(w, m);
    }
    return !(idx[0] == idx[1] || idx[0] == idx[2] || idx[1] == idx[2]);
}

// ---- the plane through three points: q0 = p0 and the unit normal nh of (p1 - p0) x (p2 - p0); false when the points are collinear
PLANE_FIT_HD bool plane_through3(const double (&p0)[3], const double (&p1)[3], const double (&p2)[3], double (&q0)[3], double (&nh)[3]) {
    q0[0] = p0[0]; q0[1] = p0[1]; q0[2] = p0[2];
    const double u0 = p1[0] - q0[0], u1 = p1[1] - q0[1], u2 = p1[2] - q0[2];
    const double w0 = p2[0] - q0[0], w1 = p2[1] - q0[1], w2 = p2[2] - q0[2];
    const double c0 = u1 * w2 - u2 * w1, c1 = u2 * w0 - u0 * w2, c2 = u0 * w1 - u1 * w0;
    const double nn = sqrt((c0 * c0 + c1 * c1) + c2 * c2);
    if (!(nn > 0)) return false;
    nh[0] = c0 / nn; nh[1] = c1 / nn; nh[2] = c2 / nn;
    return true;
}

// ---- the ten moments of a point set: n | sum x (3) | sum x x^T upper triangle (6)
PLANE_FIT_HD void moments_accumulate(double x, double y, double z, double (&acc)[10]) {
    acc[0] += 1.0;
    acc[1] += x; acc[2] += y; acc[3] += z;
    acc[4] += x * x; acc[5] += x * y; acc[6] += x * z;
    acc[7] += y * y; acc[8] += y * z; acc[9] += z * z;
}
// centroid mu and covariance S (upper triangle: 00 01 02 11 12 22) of the set
PLANE_FIT_HD void moments_to_centroid_cov(const double *mom, double (&mu)[3], double (&S)[6]) {
    const double inv = 1.0 / mom[0];
    mu[0] = mom[1] * inv; mu[1] = mom[2] * inv; mu[2] = mom[3] * inv;
    S[0] = mom[4] * inv - mu[0] * mu[0]; S[1] = mom[5] * inv - mu[0] * mu[1]; S[2] = mom[6] * inv - mu[0] * mu[2];
    S[3] = mom[7] * inv - mu[1] * mu[1]; S[4] = mom[8] * inv - mu[1] * mu[2]; S[5] = mom[9] * inv - mu[2] * mu[2];
}
// nrm normalised, and turned so that it points from the plane's point c to the side of `eye`
PLANE_FIT_HD void face_towards(double (&nrm)[3], const double *c, const double *eye) {
    const double nl = sqrt(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2]);
    double facing = 0;
    for (int k = 0; k < 3; k++) {
        nrm[k] /= nl;
        facing += nrm[k] * (eye[k] - c[k]);
    }
    if (!(facing > 0))
        for (int k = 0; k < 3; k++) nrm[k] = -nrm[k];
}

// ---- the plane's frame from the ten moments (detection's steps 4 and 6, tracking's T3 and T5), on one lane
// one Jacobi rotation in the plane (p, q) of a symmetric 3 x 3 held in scalars (k is the third index): zeroes a_pq, and rotates the
// eigenvector columns p and q.  Scalars only, so that the solve stays in registers
PLANE_FIT_HD void pl_rotate(double &app, double &aqq, double &apq, double &akp, double &akq, double &v0p, double &v0q, double &v1p, double &v1q,
                            double &v2p, double &v2q) {
    if (fabs(apq) < 1e-300) return;
    const double th = (aqq - app) / (2 * apq);
    const double t = (th >= 0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1)), c = 1 / sqrt(t * t + 1), s = t * c;
    app -= t * apq;
    aqq += t * apq;
    apq = 0;
    const double kp = akp, kq = akq;
    akp = c * kp - s * kq;
    akq = s * kp + c * kq;
    const double a0 = v0p, b0 = v0q, a1 = v1p, b1 = v1q, a2 = v2p, b2 = v2q;
    v0p = c * a0 - s * b0; v0q = s * a0 + c * b0;
    v1p = c * a1 - s * b1; v1q = s * a1 + c * b1;
    v2p = c * a2 - s * b2; v2q = s * a2 + c * b2;
}

constexpr double PL_AXIS_SWITCH = 0.9;   // |R_wc[:,0] . nrm| above this (under 26 deg between them): x is oriented by R_wc[:,1]

struct PlaneFit {
    double c[3], nrm[3], x[3], z[3];
};

// mom: the ten moments of x = P_i - q0; eye: the camera centre; a, b: R_wc[:, 0], R_wc[:, 1].  F.c = q0 + centroid, F.nrm = the unit
// eigenvector of the covariance's smallest eigenvalue, facing the camera; F.x = that of the largest, made perpendicular to nrm, unit and
// oriented by a (by b when |a . nrm| > PL_AXIS_SWITCH); F.z = x cross nrm
PLANE_FIT_HD void plane_frame_from_moments(const double *mom, const double *q0, const double *eye, const double *a, const double *b, PlaneFit &F) {
    double mu[3], cov[6];
    moments_to_centroid_cov(mom, mu, cov);
    double a00 = cov[0], a01 = cov[1], a02 = cov[2], a11 = cov[3], a12 = cov[4], a22 = cov[5];
    double v00 = 1, v01 = 0, v02 = 0, v10 = 0, v11 = 1, v12 = 0, v20 = 0, v21 = 0, v22 = 1;   // v_kc: component k of eigenvector c
    for (int sweep = 0; sweep < 12; sweep++) {   // cyclic Jacobi converges quadratically: a 3 x 3 is at the last bit after 5 or 6 sweeps
        pl_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
        pl_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
        pl_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
    }
    const int lo = a11 < a00 ? (a22 < a11 ? 2 : 1) : (a22 < a00 ? 2 : 0), hi = a11 > a00 ? (a22 > a11 ? 2 : 1) : (a22 > a00 ? 2 : 0);
    double nrm[3] = {lo == 0 ? v00 : lo == 1 ? v01 : v02, lo == 0 ? v10 : lo == 1 ? v11 : v12, lo == 0 ? v20 : lo == 1 ? v21 : v22};
    double x[3] = {hi == 0 ? v00 : hi == 1 ? v01 : v02, hi == 0 ? v10 : hi == 1 ? v11 : v12, hi == 0 ? v20 : hi == 1 ? v21 : v22};
    const double c[3] = {q0[0] + mu[0], q0[1] + mu[1], q0[2] + mu[2]};
    face_towards(nrm, c, eye);
    const double xn = x[0] * nrm[0] + x[1] * nrm[1] + x[2] * nrm[2];
    for (int k = 0; k < 3; k++) x[k] -= xn * nrm[k];
    const double xl = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
    // the axis that orients x: the camera's x axis, or its y axis for a plane that faces along the camera's x axis (every in-plane
    // direction is then perpendicular to it, and the sign would be decided by noise)
    const double an = a[0] * nrm[0] + a[1] * nrm[1] + a[2] * nrm[2];
    const bool use_b = fabs(an) > PL_AXIS_SWITCH;
    double xa = 0;
    for (int k = 0; k < 3; k++) {
        x[k] /= xl;
        xa += x[k] * (use_b ? b[k] : a[k]);
    }
    if (xa < 0)
        for (int k = 0; k < 3; k++) x[k] = -x[k];
    const double z[3] = {x[1] * nrm[2] - x[2] * nrm[1], x[2] * nrm[0] - x[0] * nrm[2], x[0] * nrm[1] - x[1] * nrm[0]};
    for (int k = 0; k < 3; k++) {
        F.c[k] = c[k]; F.nrm[k] = nrm[k]; F.x[k] = x[k]; F.z[k] = z[k];
    }
}

// the record of a found plane (detection's step 7, tracking's T5): ext = lo_x hi_x lo_z hi_z over the final set, in F's frame about F.c
PLANE_FIT_HD void plane_record(const PlaneFit &F, const double (&ext)[4], float *o) {
    const double hx = (ext[0] + ext[1]) / 2, hz = (ext[2] + ext[3]) / 2;
    const double p[3] = {F.c[0] + hx * F.x[0] + hz * F.z[0], F.c[1] + hx * F.x[1] + hz * F.z[1], F.c[2] + hx * F.x[2] + hz * F.z[2]};
    o[0] = (float) F.x[0]; o[1] = (float) F.x[1]; o[2] = (float) F.x[2]; o[3] = 0.f;
    o[4] = (float) F.nrm[0]; o[5] = (float) F.nrm[1]; o[6] = (float) F.nrm[2]; o[7] = 0.f;
    o[8] = (float) F.z[0]; o[9] = (float) F.z[1]; o[10] = (float) F.z[2]; o[11] = 0.f;
    o[12] = (float) p[0]; o[13] = (float) p[1]; o[14] = (float) p[2]; o[15] = 1.f;
    o[16] = (float) (ext[1] - ext[0]);
    o[17] = (float) (ext[3] - ext[2]);
    o[18] = (float) ((F.nrm[0] * p[0] + F.nrm[1] * p[1]) + F.nrm[2] * p[2]);
}

// ---- host: eigenvector of the smallest eigenvalue of a symmetric N x N, row-major (cyclic Jacobi)
template <int N>
inline void smallest_eigvec(const double *M, double *v) {
    double A[N][N], V[N][N];
    for (int i = 0; i < N; i++)
        for (int j = 0; j < N; j++) {
            A[i][j] = M[N * i + j];
            V[i][j] = i == j;
        }
    for (int sweep = 0; sweep < 60; sweep++) {
        double off = 0;
        for (int p = 0; p < N - 1; p++)
            for (int q = p + 1; q < N; q++) off += A[p][q] * A[p][q];
        if (off < 1e-300) break;
        for (int p = 0; p < N - 1; p++)
            for (int q = p + 1; q < N; q++) {
                if (std::fabs(A[p][q]) < 1e-300) continue;
                const double th = (A[q][q] - A[p][p]) / (2 * A[p][q]);
                const double t = (th >= 0 ? 1.0 : -1.0) / (std::fabs(th) + std::sqrt(th * th + 1)), c = 1 / std::sqrt(t * t + 1), s = t * c;
                for (int k = 0; k < N; k++) {
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - s * akq;
                    A[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < N; k++) {
                    const double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - s * aqk;
                    A[q][k] = s * apk + c * aqk;
                }
                for (int k = 0; k < N; k++) {
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
            }
    }
    int m = 0;
    for (int i = 1; i < N; i++)
        if (A[i][i] < A[m][m]) m = i;
    for (int k = 0; k < N; k++) v[k] = V[k][m];
}

#if defined(__HIPCC__)
// ---- workgroup-wide helpers for workgroups of WAVES x 64 threads; every thread calls them (they hold a barrier)

// N per-lane sums over the workgroup in a fixed order: __shfl_xor from 32 down to 1 within a wave, then the waves in ascending order.
// Thread c < N returns the total of acc[c], the others 0.  s_red: [WAVES][N] in LDS
template <int N, int WAVES>
__device__ __forceinline__ double block_sum_in_wave_order(double (&acc)[N], double (*s_red)[N]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
#pragma unroll
    for (int c = 0; c < N; c++) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) acc[c] += __shfl_xor(acc[c], o);
        if (lane == 0) s_red[wave][c] = acc[c];
    }
    __syncthreads();
    double v = 0;
    if (tid < N)
        for (int w = 0; w < WAVES; w++) v += s_red[w][tid];
    return v;
}

// In-order compaction, one item per thread and round: the output position of this thread's item (meaningful where pred holds) among all
// items kept so far, thread order within the round.  `total` is the same in every thread and is advanced by the round's count.  The wave
// counts s_wcnt[2][WAVES] are double-buffered -- the caller flips par every round -- so this one barrier per round is enough (a wave
// can be at most one round ahead of the slowest reader)
template <int WAVES>
__device__ __forceinline__ int block_compact_in_order(bool pred, int (*s_wcnt)[WAVES], int par, int &total) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned long long b = __ballot(pred);
    if (lane == 0) s_wcnt[par][wave] = __popcll(b);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < WAVES; w++) {
        const int c = s_wcnt[par][w];
        before += w < wave ? c : 0;
        all += c;
    }
    const int pos = total + before + __popcll(b & ((1ull << lane) - 1ull));
    total += all;
    return pos;
}

// The radix select's locate step, by one whole wave: hist[256] counts the keys per byte value, rank k lies among them.  4 bins per lane,
// an inclusive scan over the wave, and the lane whose bins hold rank k names the byte: every lane gets that bin and the rank r left
// within it.  Integers only, so exact
__device__ __forceinline__ void wave_radix_locate(const int *hist, int lane, int k, int &bin, int &r) {
    const int h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
    int incl = h0 + h1 + h2 + h3;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
    }
    const int excl = incl - (h0 + h1 + h2 + h3);
    r = k - excl;
    bin = 4 * lane;
    const bool mine = k >= excl && k < incl;
    if (r >= h0) { r -= h0; bin++;
        if (r >= h1) { r -= h1; bin++;
            if (r >= h2) { r -= h2; bin++; } } }
    const unsigned long long who = __ballot(mine);   // exactly one lane: rank k lies among the keys counted
    const int src = who ? __ffsll((long long) who) - 1 : 0;
    bin = __shfl(bin, src);
    r = __shfl(r, src);
}
#endif
