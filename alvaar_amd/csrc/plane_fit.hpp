// The pieces that the three plane fitters share: alva_find_plane (find_plane.hip), alva_hit_test (hit_test.hip) and alva_detect_planes
// (detect_planes.hip).  Every one of them is order-sensitive -- the tests hold discrete outputs exactly and identical calls to the bit,
// and the hit test and plane detection draw from ONE sample stream (tests/plane_cases.py) -- so each has one definition, here.
// The host-compilable part (no HIP needed) is checked by tests/cpp/plane_fit_host.cpp.
//
// What deliberately stays with its caller:
//   plane_of, plane_dist (find_plane.hip)   they replay the reference's float arithmetic and its 4-vector normalisation, and are pinned
//                                           against the repaired reference
//   the two radix-select drivers            different key widths and storage: workgroup-wide over float keys in LDS (k_plane_hyp), per
//                                           wave over double keys in registers (k_hit_test).  They share wave_radix_locate only
//   pl_rotate and the 12-sweep Jacobi       (detect_planes.hip) register-resident, a fixed sweep count: another algorithmic form than
//                                           smallest_eigvec by design; merging the two would change bits
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
