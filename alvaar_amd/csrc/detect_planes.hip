// Plane detection: the map's planes, bounded and oriented, several per call (ARCore Plane / ARKit ARPlaneAnchor / WebXR plane detection;
// the reference has no counterpart, so the definition in include/alvaar_hip.h is pinned by the numpy restatement tests/plane_cases.py).
//
// Sequential RANSAC with removal: per round, hypotheses through 3 hashed samples of the LIVE points (those no earlier round took), the
// one with the most points within `thickness` wins, the plane is refitted to that consensus set (ten moments, a 3 x 3 eigen-solve), the
// points within `thickness` of the refitted plane get the round's label and leave the live set, and their bounding rectangle along the
// principal axes is the plane's extent.  All decisions are IEEE double in the written operation order (compile with -ffp-contract=off),
// so a given point set, pose and seed give the same bits on every call.
//
// One launch of k_plane_round per round, queued back to back (plane_rounds_enqueue; the host side of alva_detect_planes is the launcher
// it shares with alva_track_planes, track_planes.hip): no host round trip between rounds, the host waits once per call for the records
// in pinned memory.  Within a round:
//   scoring     a grid of 512-thread workgroups stripes the hypotheses, one per wave at a time; a workgroup walks the live list once per
//               batch in LDS tiles of 2048 points (SoA, 48 KB) and counts with __popcll(__ballot()) -- integers, so order-free
//   hand-over   every workgroup publishes its counts (agent-scope stores), releases and adds to an arrival counter; the one that arrives
//               last acquires and goes on alone (plane_last_arriver).  No workgroup waits for another
//   last one    argmax over (count, lowest it); the consensus set's moments (per-lane strided sums, __shfl_xor, the waves in order); the
//               eigen-solve on one lane (fixed-sweep cyclic Jacobi); the final set's size and extents (min / max: exact, order-free);
//               labels; the NEXT round's live list, compacted in index order (ballot + prefix) as SoA coordinates and indices; the record
// A round that stops sets a device word; the launches queued behind it read it and return at once.
#include "common.hpp"
#include "plane_fit.hpp"
#include "plane_round.hpp"
#include <cmath>

namespace {

// the live list of round r: the input itself for r = 0
struct PlaneLive {
    const double *x, *y, *z;
    const int *idx;
    int stride;
    __device__ __forceinline__ void get(int i, double &px, double &py, double &pz) const {
        const size_t o = (size_t) i * stride;
        px = x[o]; py = y[o]; pz = z[o];
    }
    __device__ __forceinline__ int index(int i) const { return idx ? idx[i] : i; }
};

// the plane of hypothesis `it` of round r through three of the m live points: false when two indices coincide or the points are collinear
__device__ __forceinline__ bool pl_hypothesis(const PlaneArgs &A, const PlaneLive &L, int r, int it, int m, double (&q0)[3], double (&nh)[3]) {
    int idx[3];
    if (!alva_sample3(A.rand3, A.seed, (uint32_t) (r * A.iters + it), m, idx)) return false;
    double p0[3], p1[3], p2[3];
    L.get(idx[0], p0[0], p0[1], p0[2]);
    L.get(idx[1], p1[0], p1[1], p1[2]);
    L.get(idx[2], p2[0], p2[1], p2[2]);
    return plane_through3(p0, p1, p2, q0, nh);
}

__global__ void __launch_bounds__(PL_NT) k_plane_round(const PlaneArgs A, const int r) {
    __shared__ double Tx[PL_TILE], Ty[PL_TILE], Tz[PL_TILE];
    __shared__ double s_red[PL_WAVES][10];
    __shared__ int s_wcnt[2][PL_WAVES];
    __shared__ int s_key[PL_WAVES];
    __shared__ PlaneFit s_fit;
    __shared__ int s_last;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    PlaneState *S = A.state;
    if (S->stopped) return;   // written by an earlier launch
    const bool from_pts = r == 0 && !A.seeded;   // round 0 of a detection reads the input itself
    const int m = from_pts ? A.n : S->m;
    PlaneRecord *out = A.out + A.slot_base + r;
    if (m < A.min_inliers) {   // every workgroup sees the same m: the first one reports, nobody scores
        if (blockIdx.x == 0 && tid == 0) {
            out->info[0] = 1; out->info[1] = m; out->info[2] = -1; out->info[3] = 0; out->info[4] = 0;
            S->stopped = 1;
        }
        return;
    }
    PlaneLive L;
    if (from_pts) L = PlaneLive{A.pts, A.pts + 1, A.pts + 2, nullptr, 3};
    else {
        const double *b = r & 1 ? A.live[1] : A.live[0];
        L = PlaneLive{b, b + A.cap, b + 2 * (size_t) A.cap, r & 1 ? A.live_idx[1] : A.live_idx[0], 1};
    }
    const double thick = A.thickness;

    // ---- scoring: hypothesis (batch * grid + block) * 8 + wave on wave `wave`
    for (int base_it = 0; base_it < A.iters; base_it += A.grid * PL_WAVES) {
        const int it = base_it + (int) blockIdx.x * PL_WAVES + wave;
        double q0[3] = {0, 0, 0}, nh[3] = {0, 0, 0};
        const bool ok = it < A.iters && pl_hypothesis(A, L, r, it, m, q0, nh);
        int cnt = 0;
        for (int base = 0; base < m; base += PL_TILE) {
            const int tn = m - base < PL_TILE ? m - base : PL_TILE;
            __syncthreads();   // the previous tile has been scored by every wave
            for (int i = tid; i < tn; i += PL_NT) L.get(base + i, Tx[i], Ty[i], Tz[i]);
            __syncthreads();
            if (ok) {
                for (int i0 = 0; i0 < tn; i0 += 64) {
                    const int i = i0 + lane;
                    bool in = false;
                    if (i < tn) in = fabs(((Tx[i] - q0[0]) * nh[0] + (Ty[i] - q0[1]) * nh[1]) + (Tz[i] - q0[2]) * nh[2]) <= thick;
                    cnt += __popcll(__ballot(in));
                }
            }
        }
        if (lane == 0 && it < A.iters) __hip_atomic_store(A.counts + it, ok ? cnt : -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }

    // ---- hand-over: release, arrive; the last one acquires, and has the counter ready for the next round's launch
    if (!plane_last_arriver(&S->counter, A.grid, s_last)) return;

    // ---- winner: the largest count, the lowest `it` on ties.  key = count * 4096 + (4095 - it), -1: none
    int key = -1;
    for (int it = tid; it < A.iters; it += PL_NT) {
        const int c = __hip_atomic_load(A.counts + it, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int k = c < 0 ? -1 : c * PL_MAX_ITERS + (PL_MAX_ITERS - 1 - it);
        key = k > key ? k : key;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const int k = __shfl_xor(key, o);
        key = k > key ? k : key;
    }
    if (lane == 0) s_key[wave] = key;
    __syncthreads();
    key = -1;
#pragma unroll
    for (int w = 0; w < PL_WAVES; w++) key = s_key[w] > key ? s_key[w] : key;
    const int best_count = key < 0 ? 0 : key / PL_MAX_ITERS, best_it = key < 0 ? -1 : PL_MAX_ITERS - 1 - key % PL_MAX_ITERS;
    if (key < 0 || best_count < A.min_inliers) {
        if (tid == 0) {
            out->info[0] = key < 0 ? 2 : 3; out->info[1] = m; out->info[2] = best_it; out->info[3] = best_count; out->info[4] = 0;
            S->stopped = 1;
        }
        return;
    }

    // ---- refit: the ten moments of x = P_i - Q0 over the winner's consensus set, in a fixed order
    double q0[3], nh[3];
    (void) pl_hypothesis(A, L, r, best_it, m, q0, nh);
    double acc[10];
#pragma unroll
    for (int c = 0; c < 10; c++) acc[c] = 0;
    for (int i = tid; i < m; i += PL_NT) {
        double px, py, pz;
        L.get(i, px, py, pz);
        const double x = px - q0[0], y = py - q0[1], z = pz - q0[2];
        if (fabs((x * nh[0] + y * nh[1]) + z * nh[2]) <= thick) moments_accumulate(x, y, z, acc);
    }
    const double mom_c = block_sum_in_wave_order<10, PL_WAVES>(acc, s_red);
    if (tid < 10) {
        s_red[0][tid] = mom_c;   // each column is read and written by its own lane only
        out->mom[tid] = mom_c;
    }
    __syncthreads();
    if (tid == 0) plane_frame_from_moments(s_red[0], q0, A.t, A.a, A.b, s_fit);   // centroid, covariance, the three eigenvectors: one lane
    __syncthreads();
    const double c0 = s_fit.c[0], c1 = s_fit.c[1], c2 = s_fit.c[2], n0 = s_fit.nrm[0], n1 = s_fit.nrm[1], n2 = s_fit.nrm[2];
    const double x0 = s_fit.x[0], x1 = s_fit.x[1], x2 = s_fit.x[2], z0 = s_fit.z[0], z1 = s_fit.z[1], z2 = s_fit.z[2];

    // ---- final set: its size and its extent along x and z (counts and min / max: exact whatever the order)
    int n_in = 0;
    double ext[4] = {INFINITY, -INFINITY, INFINITY, -INFINITY};   // lo_x hi_x lo_z hi_z
    for (int i = tid; i < m; i += PL_NT) {
        double px, py, pz;
        L.get(i, px, py, pz);
        const double dx = px - c0, dy = py - c1, dz = pz - c2;
        if (fabs((dx * n0 + dy * n1) + dz * n2) <= thick) {
            n_in++;
            const double ex = (dx * x0 + dy * x1) + dz * x2, ez = (dx * z0 + dy * z1) + dz * z2;
            ext[0] = fmin(ext[0], ex); ext[1] = fmax(ext[1], ex);
            ext[2] = fmin(ext[2], ez); ext[3] = fmax(ext[3], ez);
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) n_in += __shfl_xor(n_in, o);
    plane_ext_wave(ext);
    if (lane == 0) {
        s_key[wave] = n_in;
#pragma unroll
        for (int k = 0; k < 4; k++) s_red[wave][k] = ext[k];
    }
    __syncthreads();
    n_in = 0;
#pragma unroll
    for (int w = 0; w < PL_WAVES; w++) {
        n_in += s_key[w];
        ext[0] = w ? fmin(ext[0], s_red[w][0]) : s_red[0][0]; ext[1] = w ? fmax(ext[1], s_red[w][1]) : s_red[0][1];
        ext[2] = w ? fmin(ext[2], s_red[w][2]) : s_red[0][2]; ext[3] = w ? fmax(ext[3], s_red[w][3]) : s_red[0][3];
    }
    if (n_in < A.min_inliers) {   // nothing is labelled in this round
        if (tid == 0) {
            out->info[0] = 4; out->info[1] = m; out->info[2] = best_it; out->info[3] = best_count; out->info[4] = n_in;
            S->stopped = 1;
        }
        return;
    }

    // ---- labels, and the next round's live list compacted in index order
    double *nb = r & 1 ? A.live[0] : A.live[1];
    int *ni = r & 1 ? A.live_idx[0] : A.live_idx[1];
    int total = 0;
    for (int base = 0, par = 0; base < m; base += PL_NT, par ^= 1) {
        const int i = base + tid;
        bool keep = false;
        double px = 0, py = 0, pz = 0;
        int idx = 0;
        if (i < m) {
            L.get(i, px, py, pz);
            idx = L.index(i);
            const double dx = px - c0, dy = py - c1, dz = pz - c2;
            keep = !(fabs((dx * n0 + dy * n1) + dz * n2) <= thick);
            if (!keep && A.labels) A.labels[idx] = A.slot_base + r;
        }
        const int pos = block_compact_in_order<PL_WAVES>(keep, s_wcnt, par, total);   // pos < m - (labelled so far) <= cap
        if (keep) {
            nb[pos] = px; nb[A.cap + pos] = py; nb[2 * (size_t) A.cap + pos] = pz;
            ni[pos] = idx;
        }
    }

    // ---- record
    if (tid == 0) {
        plane_record(s_fit, ext, out->plane);
        out->info[0] = 0; out->info[1] = m; out->info[2] = best_it; out->info[3] = best_count; out->info[4] = n_in;
        S->m = total;
    }
}

}  // namespace

int plane_rounds_enqueue(alva_ctx *ctx, const PlaneArgs &A, int rounds) {
    for (int r = 0; r < rounds; r++) {
        hipLaunchKernelGGL(k_plane_round, dim3(A.grid), dim3(PL_NT), 0, ctx->stream, A, r);
        ALVA_LAUNCH_CHECK();
    }
    return ALVA_OK;
}

