// Anchors: poses that stay attached to the map as it is refined (ARCore HitResult.createAnchor / Anchor.getPose, ARKit ARAnchor, WebXR
// XRAnchor; the reference has no counterpart, so the definitions in include/alvaar_hip.h -- A1 to A3, U0 to U5 -- are pinned by the numpy
// restatement tests/anchor_cases.py).  An anchor is tied to the map points around it (its support), and its pose is recomputed from where
// those points are now.  Two stages, one launch each, records in pinned memory, the host waits once:
//
// k_anchor_attach   the support: the K nearest points of an anchor's position.  One 512-thread workgroup per anchor.  A thread holds the
//                   distances of its 32 points (index tid + 512 j) in registers -- a distance array of 16384 doubles is 128 KB of LDS --
//                   and the workgroup finds the distance of rank K - 1 exactly by a radix select over the doubles' bit patterns (they are
//                   >= 0, so bit order is value order): 8 byte passes over ONE 256-bin LDS histogram, located by every wave alike
//                   (wave_radix_locate: integers, so every wave names the same bin).  The points below the threshold, and the first of
//                   those equal to it, are compacted in index order (block_compact_in_order); one wave sorts the <= 64 survivors by
//                   (distance, index) with a rank count.  Everything after the distance is a comparison of bit patterns.
// k_anchor_update   the rigid motion of a support, robustly: Horn's closed form (the largest eigenvector of a symmetric 4 x 4, cyclic
//                   Jacobi, 12 sweeps) and one trim round at 3.7065 x the median residual.  One wave per anchor, one support per lane,
//                   four anchors per 256-thread workgroup.  Every sum is a __shfl_xor butterfly (masks 1, 2, 4 .. 32) that leaves the same
//                   bits in every lane -- IEEE addition commutes -- so the eigen-solve runs uniformly on all lanes and nothing is
//                   broadcast.  No LDS, no barrier, no scratch; no workgroup waits for another.
// All decisions are IEEE double in the written operation order (compile with -ffp-contract=off).
#include "common.hpp"
#include "plane_fit.hpp"
#include <cmath>

namespace {

constexpr int AN_NT = 512, AN_WAVES = AN_NT / 64, AN_N_CAP = 16384, AN_PER_THREAD = AN_N_CAP / AN_NT, AN_MAX_ATTACH = 16;
constexpr int AN_K_MIN = 8, AN_K_MAX = 64;   // the support: one point per lane of a wave64 at most
constexpr int AU_NT = 256, AU_WAVES = AU_NT / 64, AU_MAX_ANCHORS = 64, AU_STRIDE = 64;
constexpr double AU_TRIM_FACTOR = 3.7065;    // 2.5 x 1.4826, the hit test's LMedS scale
constexpr double AU_TRIM_FLOOR = 1e-9;       // x rho: keeps every point of a map that did not move (med = 0)
constexpr double AU_GAP = 1e-4;              // x sqrt(Spp Sqq): below it the two largest eigenvalues do not determine a rotation

struct AttachRecord {   // one per anchor, in pinned memory
    double d[AN_K_MAX];
    int idx[AN_K_MAX];
    int count, pad[15];
};

struct AttachArgs {
    const double *pts;   // [n][3]
    int n, K;
    double pos[AN_MAX_ATTACH][3];
    AttachRecord *out;
};

__global__ void __launch_bounds__(AN_NT) k_anchor_attach(const AttachArgs A) {
    __shared__ int s_hist[256];
    __shared__ int s_wless[2][AN_WAVES], s_weq[2][AN_WAVES];
    __shared__ unsigned long long s_key[AN_K_MAX];
    __shared__ int s_idx[AN_K_MAX];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = A.n;
    const double ax = A.pos[blockIdx.x][0], ay = A.pos[blockIdx.x][1], az = A.pos[blockIdx.x][2];
    AttachRecord *out = A.out + blockIdx.x;

    // ---- A1: the distances, 32 per thread; a thread's point j is tid + 512 j
    unsigned long long key[AN_PER_THREAD];
#pragma unroll
    for (int j = 0; j < AN_PER_THREAD; j++) {
        const int i = tid + AN_NT * j;
        key[j] = ~0ull;
        if (i < n) {
            const double dx = A.pts[3 * (size_t) i] - ax, dy = A.pts[3 * (size_t) i + 1] - ay, dz = A.pts[3 * (size_t) i + 2] - az;
            key[j] = (unsigned long long) __double_as_longlong((dx * dx + dy * dy) + dz * dz);
        }
    }

    // ---- A2: the key of rank count - 1 among the n, one byte per pass from the top.  Whether a slot holds a point is asked of its index,
    // never of its key: a distance may have any bit pattern
    const int count = A.K < n ? A.K : n;
    unsigned long long prefix = 0, mask = 0;
    int kk = count - 1;
    for (int pass = 7; pass >= 0; pass--) {
        const int sh = 8 * pass;
        if (tid < 256) s_hist[tid] = 0;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < AN_PER_THREAD; j++)
            if (tid + AN_NT * j < n && (key[j] & mask) == prefix) atomicAdd(&s_hist[(int) ((key[j] >> sh) & 255ull)], 1);
        __syncthreads();
        int bin;
        wave_radix_locate(s_hist, lane, kk, bin, kk);   // every wave reads the same counts and names the same byte
        prefix |= (unsigned long long) bin << sh;
        mask |= 255ull << sh;
        __syncthreads();   // the histogram is zeroed again only after every wave has read it
    }
    // prefix: the threshold key; kk: the rank left among the keys equal to it, so the support is every key below the threshold -- there
    // are n_less = count - 1 - kk of them -- and the kk + 1 lowest indices among the equal ones
    const int n_less = count - 1 - kk;

    // ---- in-order compaction: round j holds the indices 512 j .. 512 j + 511 in thread order
    int total_less = 0, total_eq = 0;
#pragma unroll
    for (int j = 0; j < AN_PER_THREAD; j++) {
        if (AN_NT * j >= n) break;   // the same in every thread
        const int i = tid + AN_NT * j;
        const bool less = i < n && key[j] < prefix, eq = i < n && key[j] == prefix;
        const int pl = block_compact_in_order<AN_WAVES>(less, s_wless, j & 1, total_less);
        const int pe = block_compact_in_order<AN_WAVES>(eq, s_weq, j & 1, total_eq);
        const int slot = less ? pl : eq && pe <= kk ? n_less + pe : -1;   // pl < n_less and n_less + pe <= count - 1 by the counts above
        if (slot >= 0 && slot < AN_K_MAX) {
            s_key[slot] = key[j];
            s_idx[slot] = i;
        }
    }
    __syncthreads();

    // ---- A3: one wave sorts the survivors by (key, index): a lane's rank is the number of survivors before it
    if (wave == 0) {
        if (lane < count) {
            const unsigned long long mk = s_key[lane];
            const int mi = s_idx[lane];
            int rank = 0;
            for (int m = 0; m < count; m++) {
                const unsigned long long ok = s_key[m];
                rank += ok < mk || (ok == mk && s_idx[m] < mi);
            }
            out->d[rank] = __longlong_as_double((long long) mk);
            out->idx[rank] = mi;
        } else {
            out->d[lane] = 0;
            out->idx[lane] = -1;
        }
        if (lane == 0) out->count = count;
    }
}

// ---------------------------------------------------------------------------------------------------------------- update
struct UpdateRecord {   // one per anchor, in pinned memory
    double rt[12];      // R row-major, t
    float pose[16];
    int info[8];
};

struct UpdateArgs {
    int n_anchors;
    const int *count;        // [n_anchors]                        (pinned)
    const double *ref;       // [n_anchors][AU_STRIDE][3]
    const double *cur;       // [n_anchors][AU_STRIDE][3]
    const float *pose_ref;   // [n_anchors][16]
    UpdateRecord *out;
};

// the sum over the wave's 64 lanes in the butterfly order, masks 1, 2, 4, 8, 16, 32: a balanced tree over the lanes, the same bits in
// every lane (a + b == b + a)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ double dot3(double a0, double a1, double a2, double b0, double b1, double b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }

// U1 - U3 over the lanes `in` (c of them, c >= 1): centroids, spreads and, when c >= 4 and the gap test passes, Horn's rotation.  R, t:
// the fit, or I and cq - cp when the function returns false.  Every lane computes the same bits
__device__ __forceinline__ bool rigid_fit(bool in, int c, const double (&p)[3], const double (&q)[3], double (&R)[9], double (&t)[3], double &rho) {
    double cp[3], cq[3], pc[3], qc[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        cp[k] = wave_sum(in ? p[k] : 0.0) / (double) c;
        cq[k] = wave_sum(in ? q[k] : 0.0) / (double) c;
        pc[k] = p[k] - cp[k];
        qc[k] = q[k] - cq[k];
    }
    const double Spp = wave_sum(in ? (pc[0] * pc[0] + pc[1] * pc[1]) + pc[2] * pc[2] : 0.0);
    const double Sqq = wave_sum(in ? (qc[0] * qc[0] + qc[1] * qc[1]) + qc[2] * qc[2] : 0.0);
    rho = sqrt(Spp / (double) c);
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = k % 4 == 0 ? 1.0 : 0.0;
#pragma unroll
    for (int k = 0; k < 3; k++) t[k] = cq[k] - cp[k];
    if (c < 4) return false;   // U2

    double S[3][3];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) S[a][b] = wave_sum(in ? pc[a] * qc[b] : 0.0);
    // Horn's N (J. Opt. Soc. Am. A 4, 1987, eq. 25 -- as written in include/alvaar_hip.h); the unit quaternion (w, x, y, z) of the rotation is
    // the eigenvector of its largest eigenvalue
    double M[4][4], V[4][4];
    M[0][0] = (S[0][0] + S[1][1]) + S[2][2];
    M[1][1] = (S[0][0] - S[1][1]) - S[2][2];
    M[2][2] = (S[1][1] - S[0][0]) - S[2][2];
    M[3][3] = (S[2][2] - S[0][0]) - S[1][1];
    M[0][1] = M[1][0] = S[1][2] - S[2][1];
    M[0][2] = M[2][0] = S[2][0] - S[0][2];
    M[0][3] = M[3][0] = S[0][1] - S[1][0];
    M[1][2] = M[2][1] = S[0][1] + S[1][0];
    M[1][3] = M[3][1] = S[2][0] + S[0][2];
    M[2][3] = M[3][2] = S[1][2] + S[2][1];
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) V[a][b] = a == b ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 12; sweep++) {   // the project's fixed sweep count (plane_frame_from_moments); every index below is static
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int b = a + 1; b < 4; b++) {
                const double apq = M[a][b];
                if (fabs(apq) < 1e-300) continue;
                const double th = (M[b][b] - M[a][a]) / (2 * apq);
                const double tt = (th >= 0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1)), cs = 1 / sqrt(tt * tt + 1), sn = tt * cs;
                M[a][a] -= tt * apq;
                M[b][b] += tt * apq;
                M[a][b] = M[b][a] = 0;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    if (k == a || k == b) continue;
                    const double kp = M[k][a], kq = M[k][b];
                    M[k][a] = M[a][k] = cs * kp - sn * kq;
                    M[k][b] = M[b][k] = sn * kp + cs * kq;
                }
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const double vp = V[k][a], vq = V[k][b];
                    V[k][a] = cs * vp - sn * vq;
                    V[k][b] = sn * vp + cs * vq;
                }
            }
    }
    // the two largest eigenvalues; the lowest index on ties
    int i1 = 0;
#pragma unroll
    for (int k = 1; k < 4; k++)
        if (M[k][k] > (i1 == 0 ? M[0][0] : i1 == 1 ? M[1][1] : i1 == 2 ? M[2][2] : M[3][3])) i1 = k;
    double l1 = 0, l2 = -INFINITY, e[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (k == i1) {
            l1 = M[k][k];
#pragma unroll
            for (int r = 0; r < 4; r++) e[r] = V[r][k];
        } else if (M[k][k] > l2) {
            l2 = M[k][k];
        }
    }
    if (l1 - l2 <= AU_GAP * sqrt(Spp * Sqq)) return false;   // (a NaN anywhere fails the comparison and goes on as a rotation of NaNs)
    const double nq = sqrt(((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) + e[3] * e[3]);
    const double w = e[0] / nq, x = e[1] / nq, y = e[2] / nq, z = e[3] / nq;
    R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - w * z);     R[2] = 2 * (x * z + w * y);
    R[3] = 2 * (x * y + w * z);     R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - w * x);
    R[6] = 2 * (x * z - w * y);     R[7] = 2 * (y * z + w * x);     R[8] = 1 - 2 * (x * x + y * y);
#pragma unroll
    for (int k = 0; k < 3; k++) t[k] = cq[k] - dot3(R[3 * k], R[3 * k + 1], R[3 * k + 2], cp[0], cp[1], cp[2]);
    return true;
}

__global__ void __launch_bounds__(AU_NT) k_anchor_update(const UpdateArgs A) {
    const int lane = threadIdx.x & 63;
    const int a = (int) blockIdx.x * AU_WAVES + __builtin_amdgcn_readfirstlane((int) threadIdx.x >> 6);
    if (a >= A.n_anchors) return;   // a whole wave; there is no barrier in this kernel
    const int m = __builtin_amdgcn_readfirstlane(A.count[a]);
    UpdateRecord *out = A.out + a;
    const float *pr = A.pose_ref + 16 * a;

    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0};
    int code = 2, kept = m;
    if (m > 0) {
        double p[3] = {0, 0, 0}, q[3] = {0, 0, 0};
        if (lane < m) {
            const size_t o = ((size_t) a * AU_STRIDE + lane) * 3;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                p[k] = A.ref[o + k];
                q[k] = A.cur[o + k];
            }
        }
        bool in = lane < m;
        int c = m;
        double rho = 0;
        for (int round = 0; round < 2; round++) {
            double Rn[9], tn[3], rho_n;
            const bool det = rigid_fit(in, c, p, q, Rn, tn, rho_n);
            if (round == 0 || det) {   // an undetermined refit leaves the first fit standing
#pragma unroll
                for (int k = 0; k < 9; k++) R[k] = Rn[k];
#pragma unroll
                for (int k = 0; k < 3; k++) t[k] = tn[k];
            }
            if (round == 1) break;
            code = det ? 0 : 1;
            rho = rho_n;
            if (!det) break;   // the trim judges a rigid fit only
            // ---- U4: residuals, their median by a rank count under (r, lane), the trim
            double e[3];
#pragma unroll
            for (int k = 0; k < 3; k++) e[k] = q[k] - (dot3(R[3 * k], R[3 * k + 1], R[3 * k + 2], p[0], p[1], p[2]) + t[k]);
            const double r = sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
            int rank = 0;
            for (int l = 0; l < m; l++) {
                const double rl = __shfl(r, l);
                rank += rl < r || (rl == r && l < lane);
            }
            const unsigned long long who = __ballot(in && rank == m / 2);
            const double med = __shfl(r, who ? __ffsll((long long) who) - 1 : 0);
            const bool keep = in && (r <= AU_TRIM_FACTOR * med || r <= AU_TRIM_FLOOR * rho);
            kept = __popcll(__ballot(keep));
            if (!(kept >= 4 && kept < m)) break;
            in = keep;
            c = kept;
        }
    }

    // ---- U5: [R | t] o the reference pose; every lane holds the same values, lanes 0 .. 11 write rt, lanes 0 .. 15 the pose
    double P[16];
#pragma unroll
    for (int col = 0; col < 4; col++) {
        const double v0 = (double) pr[4 * col], v1 = (double) pr[4 * col + 1], v2 = (double) pr[4 * col + 2];
#pragma unroll
        for (int row = 0; row < 3; row++) {
            const double rv = dot3(R[3 * row], R[3 * row + 1], R[3 * row + 2], v0, v1, v2);
            P[4 * col + row] = col == 3 ? rv + t[row] : rv;
        }
        P[4 * col + 3] = col == 3 ? 1.0 : 0.0;
    }
    if (code == 2) {   // U0: no support, the reference pose as it is
#pragma unroll
        for (int k = 0; k < 16; k++) P[k] = (double) pr[k];
    }
    double mine_rt = 0, mine_p = 0;
#pragma unroll
    for (int k = 0; k < 12; k++) mine_rt = lane == k ? (k < 9 ? R[k] : t[k - 9]) : mine_rt;
#pragma unroll
    for (int k = 0; k < 16; k++) mine_p = lane == k ? P[k] : mine_p;
    if (lane < 12) out->rt[lane] = mine_rt;
    if (lane < 16) out->pose[lane] = code == 2 ? pr[lane] : (float) mine_p;
    if (lane < 8) out->info[lane] = lane == 0 ? code : lane == 1 ? m : lane == 2 ? kept : 0;
}

}  // namespace

extern "C" int alva_anchor_attach(alva_ctx *ctx, const double *d_points, int n, int n_anchors, const double *h_pos3, int max_support,
                                  int *h_index, double *h_dist2, int *h_count) {
    ALVA_ARG(ctx && h_pos3 && h_index && h_dist2 && h_count);
    ALVA_ARG(n >= 0 && n <= AN_N_CAP && (d_points || n == 0));
    ALVA_ARG(n_anchors >= 1 && n_anchors <= AN_MAX_ATTACH && max_support >= AN_K_MIN && max_support <= AN_K_MAX);
    for (int i = 0; i < n_anchors * max_support; i++) {
        h_index[i] = -1;
        h_dist2[i] = 0;
    }
    memset(h_count, 0, (size_t) n_anchors * sizeof(int));
    if (n == 0) return ALVA_OK;
    AttachRecord *pin = nullptr;
    const int rc = alva_ctx_pinned(ctx, (size_t) n_anchors * sizeof(AttachRecord), (void **) &pin);
    if (rc) return rc;
    AttachArgs A{};
    A.pts = d_points;
    A.n = n;
    A.K = max_support;
    memcpy(A.pos, h_pos3, (size_t) n_anchors * 3 * sizeof(double));
    A.out = pin;
    hipLaunchKernelGGL(k_anchor_attach, dim3(n_anchors), dim3(AN_NT), 0, ctx->stream, A);
    ALVA_LAUNCH_CHECK();
    ALVA_HIP(alva_stream_sync(ctx->stream));
    for (int a = 0; a < n_anchors; a++) {
        const int count = pin[a].count;
        if (count < 0 || count > max_support) {
            alva_set_error("alva_anchor_attach: anchor %d came back with %d supports", a, count);
            return ALVA_ERR_STATE;
        }
        h_count[a] = count;
        memcpy(h_index + (size_t) a * max_support, pin[a].idx, (size_t) count * sizeof(int));
        memcpy(h_dist2 + (size_t) a * max_support, pin[a].d, (size_t) count * sizeof(double));
    }
    return ALVA_OK;
}

extern "C" int alva_anchor_update(alva_ctx *ctx, int n_anchors, const int *h_count, const double *h_ref, const double *h_cur,
                                  const float *h_pose16_ref, float *h_pose16, double *h_rt12, int *h_info8) {
    ALVA_ARG(ctx && h_count && h_pose16_ref && h_pose16 && h_info8);
    ALVA_ARG(n_anchors >= 1 && n_anchors <= AU_MAX_ANCHORS);
    bool any = false;
    for (int a = 0; a < n_anchors; a++) {
        ALVA_ARG(h_count[a] >= 0 && h_count[a] <= AU_STRIDE);
        any = any || h_count[a] > 0;
    }
    ALVA_ARG(!any || (h_ref && h_cur));
    // pinned: counts | reference poses | ref | cur | one record per anchor
    const size_t na = (size_t) n_anchors, set_bytes = na * AU_STRIDE * 3 * sizeof(double);
    const size_t off_pose = (na * sizeof(int) + 255) / 256 * 256, off_ref = off_pose + (na * 16 * sizeof(float) + 255) / 256 * 256;
    const size_t off_cur = off_ref + set_bytes, off_rec = off_cur + set_bytes;
    uint8_t *pin = nullptr;
    const int rc = alva_ctx_pinned(ctx, off_rec + na * sizeof(UpdateRecord), (void **) &pin);
    if (rc) return rc;
    memcpy(pin, h_count, na * sizeof(int));
    memcpy(pin + off_pose, h_pose16_ref, na * 16 * sizeof(float));
    for (int a = 0; a < n_anchors; a++) {   // the rows past an anchor's count are not read
        const size_t o = (size_t) a * AU_STRIDE * 3, bytes = (size_t) h_count[a] * 3 * sizeof(double);
        if (!bytes) continue;
        memcpy((double *) (pin + off_ref) + o, h_ref + o, bytes);
        memcpy((double *) (pin + off_cur) + o, h_cur + o, bytes);
    }
    UpdateArgs A{};
    A.n_anchors = n_anchors;
    A.count = (const int *) pin;
    A.pose_ref = (const float *) (pin + off_pose);
    A.ref = (const double *) (pin + off_ref);
    A.cur = (const double *) (pin + off_cur);
    A.out = (UpdateRecord *) (pin + off_rec);
    hipLaunchKernelGGL(k_anchor_update, dim3(alva_divup(n_anchors, AU_WAVES)), dim3(AU_NT), 0, ctx->stream, A);
    ALVA_LAUNCH_CHECK();
    ALVA_HIP(alva_stream_sync(ctx->stream));
    for (int a = 0; a < n_anchors; a++) {
        UpdateRecord rec;
        memcpy(&rec, A.out + a, sizeof(rec));
        memcpy(h_pose16 + 16 * a, rec.pose, sizeof(rec.pose));
        memcpy(h_info8 + 8 * a, rec.info, sizeof(rec.info));
        if (h_rt12) memcpy(h_rt12 + 12 * a, rec.rt, sizeof(rec.rt));
    }
    return ALVA_OK;
}
