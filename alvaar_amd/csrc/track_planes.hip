// Plane tracking: the planes of an earlier call, refitted to the points of this one, in their own slots; new planes among the points
// that no kept plane claims (ARCore Plane trackables / ARKit ARPlaneAnchor updates / the WebXR XRPlane set; the reference has no
// counterpart, so the definition in include/alvaar_hip.h -- T0 to T6 -- is pinned by the numpy restatement tests/track_cases.py).
//
// One launch of k_track_claim in front of the rounds of detection (k_plane_round, detect_planes.hip), all queued back to back: no host
// round trip, the host waits once per call for the records in pinned memory.  The launcher here is alva_detect_planes' too: without
// priors there is no claim launch, and round 0 reads the input itself.  With one prior k_track_claim is ONE 512-thread
// workgroup.  With two or more it is one workgroup per prior: every workgroup makes the whole claim (it needs every prior), workgroup j
// refits prior j alone, publishes the frame (agent-scope stores), releases and adds to an arrival counter; the one that arrives last
// acquires, reads the frames and settles alone -- k_plane_round's hand-over, no workgroup waits for another.  The steps:
//   claim       every point against every usable prior (at most 8, held in LDS); the point-to-slot assignment is one byte per point in
//               LDS (16 KB at the bound of 16384 points); the per-prior counts are __popcll(__ballot()) sums -- integers, order-free
//   refit       per prior with enough points, the ten moments of its claimed set (per-lane strided sums, __shfl_xor, the waves in order:
//               block_sum_in_wave_order) and the eigen-solve on one lane: prior after prior in the one workgroup (the solves then side by
//               side, wave w's lane 0 for prior w), or each in the workgroup of its own
//   settle      the claim again, against the refitted planes; sizes, then per kept plane the extents (min / max: exact, order-free)
//   hand-over   labels, and the points that no kept plane holds compacted in index order (block_compact_in_order) into live[0] /
//               live_idx[0] / PlaneState::m: the live list that k_plane_round's round 0 reads when PlaneArgs::seeded is set
// All decisions are IEEE double in the written operation order (compile with -ffp-contract=off).
#include "common.hpp"
#include "plane_fit.hpp"
#include "plane_round.hpp"
#include "slam/se3.hpp"
#include <cmath>

namespace {

constexpr int TP_NONE = 255;   // the assignment byte of a point that no plane claims

struct TrackArgs {
    PlaneArgs R;                          // the rounds' block: pts, n, cap, live, live_idx, state, labels, out, min_inliers, thickness, t, a, b
    int n_prior;
    unsigned usable;                      // bit j: prior j is usable (T0)
    double prior[PL_MAX_PLANES][6];       // c_j (3), n_j (3): the records' floats cast to double
    int split;                            // 1: a grid of n_prior workgroups, workgroup j refits prior j (T1 - T3), the last to arrive finishes
    double *fits;                         // [PL_MAX_PLANES][12] (split only): the refitted frames c, nrm, x, z, handed to the finisher
};

// T1 / T4: every point to the plane of `mask` with the smallest |d| among those within `thick`, the lowest j on ties; the assignment
// goes to s_assign, the planes' sizes to s_tot (valid after the barrier this ends with)
__device__ __forceinline__ void tp_claim(const double *pts, int n, unsigned mask, const double (*s_pl)[6], double thick, uint8_t *s_assign,
                                         int (*s_cnt)[PL_MAX_PLANES], int *s_tot) {
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int cnt[PL_MAX_PLANES];
#pragma unroll
    for (int j = 0; j < PL_MAX_PLANES; j++) cnt[j] = 0;
    for (int base = 0; base < n; base += PL_NT) {   // every lane runs every trip: the ballots need whole waves
        const int i = base + tid;
        int best = TP_NONE;
        if (i < n) {
            const double px = pts[3 * (size_t) i], py = pts[3 * (size_t) i + 1], pz = pts[3 * (size_t) i + 2];
            double bd = INFINITY;
#pragma unroll
            for (int j = 0; j < PL_MAX_PLANES; j++) {
                if (!((mask >> j) & 1u)) continue;
                const double d = fabs(((px - s_pl[j][0]) * s_pl[j][3] + (py - s_pl[j][1]) * s_pl[j][4]) + (pz - s_pl[j][2]) * s_pl[j][5]);
                if (d <= thick && d < bd) {
                    bd = d;
                    best = j;
                }
            }
            s_assign[i] = (uint8_t) best;
        }
#pragma unroll
        for (int j = 0; j < PL_MAX_PLANES; j++) cnt[j] += __popcll(__ballot(best == j));
    }
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < PL_MAX_PLANES; j++) s_cnt[wave][j] = cnt[j];
    }
    __syncthreads();
    if (tid < PL_MAX_PLANES) {
        int t = 0;
        for (int w = 0; w < PL_WAVES; w++) t += s_cnt[w][tid];
        s_tot[tid] = t;
    }
    __syncthreads();
}

__global__ void __launch_bounds__(PL_NT) k_track_claim(const TrackArgs T) {
    __shared__ uint8_t s_assign[PL_N_CAP];
    __shared__ double s_pl[PL_MAX_PLANES][6];
    __shared__ double s_red[PL_WAVES][10];
    __shared__ double s_mom[PL_MAX_PLANES][10];
    __shared__ double s_ext[PL_MAX_PLANES][4];
    __shared__ PlaneFit s_fit[PL_MAX_PLANES];
    __shared__ int s_cnt[PL_WAVES][PL_MAX_PLANES];
    __shared__ int s_tot[2][PL_MAX_PLANES];   // claimed (T1), inliers (T4)
    __shared__ int s_wcnt[2][PL_WAVES];
    __shared__ int s_last;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const PlaneArgs &A = T.R;
    const int n = A.n, np = T.n_prior;
    const double *pts = A.pts;
    const double thick = A.thickness;

    // ---- T0, T1: the priors as handed in
    if (tid < np * 6) s_pl[tid / 6][tid % 6] = T.prior[tid / 6][tid % 6];
    __syncthreads();
    tp_claim(pts, n, T.usable, s_pl, thick, s_assign, s_cnt, s_tot[0]);

    // ---- T2: the priors that go on
    unsigned active = 0;
#pragma unroll
    for (int j = 0; j < PL_MAX_PLANES; j++)
        if (j < np && ((T.usable >> j) & 1u) && s_tot[0][j] >= A.min_inliers) active |= 1u << j;

    // ---- T3: the ten moments of x = P_i - c_j over prior j's claimed set, in a fixed order; then the eight solves side by side
    for (int j = 0; j < np; j++) {
        if (!((active >> j) & 1u) || (T.split && j != (int) blockIdx.x)) continue;
        const double c0 = s_pl[j][0], c1 = s_pl[j][1], c2 = s_pl[j][2];
        double acc[10];
#pragma unroll
        for (int c = 0; c < 10; c++) acc[c] = 0;
        for (int i = tid; i < n; i += PL_NT)
            if (s_assign[i] == j) moments_accumulate(pts[3 * (size_t) i] - c0, pts[3 * (size_t) i + 1] - c1, pts[3 * (size_t) i + 2] - c2, acc);
        const double mom_c = block_sum_in_wave_order<10, PL_WAVES>(acc, s_red);
        if (tid < 10) {
            s_mom[j][tid] = mom_c;
            A.out[j].mom[tid] = mom_c;
        }
        __syncthreads();   // s_red is free again, s_mom[j] is visible
    }
    if (!T.split) {
        if (lane == 0 && wave < np && ((active >> wave) & 1u)) plane_frame_from_moments(s_mom[wave], s_pl[wave], A.t, A.a, A.b, s_fit[wave]);
        __syncthreads();
    } else {
        // ---- split: this workgroup's prior only; publish its frame, release, arrive; the last one acquires and goes on alone
        const int jb = blockIdx.x;
        const bool mine = (active >> jb) & 1u;
        if (tid == 0 && mine) plane_frame_from_moments(s_mom[jb], s_pl[jb], A.t, A.a, A.b, s_fit[jb]);
        __syncthreads();
        if (tid < 12 && mine) __hip_atomic_store(T.fits + 12 * jb + tid, (&s_fit[jb].c[0])[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (!plane_last_arriver(&A.state->counter, (int) gridDim.x, s_last)) return;   // the rounds behind count from 0
        if (tid < np * 12 && ((active >> (tid / 12)) & 1u))
            (&s_fit[tid / 12].c[0])[tid % 12] = __hip_atomic_load(T.fits + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
    }
    if (tid < np * 6 && ((active >> (tid / 6)) & 1u)) s_pl[tid / 6][tid % 6] = tid % 6 < 3 ? s_fit[tid / 6].c[tid % 6] : s_fit[tid / 6].nrm[tid % 6 - 3];
    __syncthreads();

    // ---- T4: the claim again, against the refitted planes
    tp_claim(pts, n, active, s_pl, thick, s_assign, s_cnt, s_tot[1]);
    unsigned kept = 0;
#pragma unroll
    for (int j = 0; j < PL_MAX_PLANES; j++)
        if (((active >> j) & 1u) && s_tot[1][j] >= A.min_inliers) kept |= 1u << j;

    // ---- T5: the extents of the kept planes over their T4 sets (min / max: exact whatever the order)
    for (int j = 0; j < np; j++) {
        if (!((kept >> j) & 1u)) continue;
        const double c0 = s_fit[j].c[0], c1 = s_fit[j].c[1], c2 = s_fit[j].c[2];
        const double x0 = s_fit[j].x[0], x1 = s_fit[j].x[1], x2 = s_fit[j].x[2], z0 = s_fit[j].z[0], z1 = s_fit[j].z[1], z2 = s_fit[j].z[2];
        double ext[4] = {INFINITY, -INFINITY, INFINITY, -INFINITY};   // lo_x hi_x lo_z hi_z
        for (int i = tid; i < n; i += PL_NT)
            if (s_assign[i] == j) {
                const double dx = pts[3 * (size_t) i] - c0, dy = pts[3 * (size_t) i + 1] - c1, dz = pts[3 * (size_t) i + 2] - c2;
                const double ex = (dx * x0 + dy * x1) + dz * x2, ez = (dx * z0 + dy * z1) + dz * z2;
                ext[0] = fmin(ext[0], ex); ext[1] = fmax(ext[1], ex);
                ext[2] = fmin(ext[2], ez); ext[3] = fmax(ext[3], ez);
            }
        plane_ext_wave(ext);
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 4; k++) s_red[wave][k] = ext[k];
        }
        __syncthreads();
        if (tid < 4) {
            double v = s_red[0][tid];
            for (int w = 1; w < PL_WAVES; w++) v = tid & 1 ? fmax(v, s_red[w][tid]) : fmin(v, s_red[w][tid]);
            s_ext[j][tid] = v;
        }
        __syncthreads();
    }

    // ---- labels, and round 0's live list: the points that no kept plane holds, compacted in index order
    double *nb = A.live[0];
    int *ni = A.live_idx[0];
    int total = 0;
    for (int base = 0, par = 0; base < n; base += PL_NT, par ^= 1) {
        const int i = base + tid;
        bool keep = false;
        if (i < n) {
            const int a = s_assign[i];
            keep = a == TP_NONE || !((kept >> a) & 1u);
            if (!keep && A.labels) A.labels[i] = a;
        }
        const int pos = block_compact_in_order<PL_WAVES>(keep, s_wcnt, par, total);   // pos < n <= cap
        if (keep) {
            nb[pos] = pts[3 * (size_t) i]; nb[A.cap + pos] = pts[3 * (size_t) i + 1]; nb[2 * (size_t) A.cap + pos] = pts[3 * (size_t) i + 2];
            ni[pos] = i;
        }
    }

    // ---- records: thread j writes slot j
    if (tid < np) {
        PlaneRecord *out = A.out + tid;
        const bool us = (T.usable >> tid) & 1u, ac = (active >> tid) & 1u, kp = (kept >> tid) & 1u;
        if (kp) {
            const double ext[4] = {s_ext[tid][0], s_ext[tid][1], s_ext[tid][2], s_ext[tid][3]};
            plane_record(s_fit[tid], ext, out->plane);
        }
        out->info[0] = kp ? 0 : ac ? 8 : us ? 7 : 9;
        out->info[1] = n; out->info[2] = -1; out->info[3] = us ? s_tot[0][tid] : 0; out->info[4] = ac ? s_tot[1][tid] : 0; out->info[5] = 1;
    }
    if (tid == 0) A.state->m = total;
}

// The one host body of alva_detect_planes (n_prior = 0: no claim launch, round 0 reads the input itself) and alva_track_planes
int planes_run(alva_ctx *ctx, const double *d_points, int n, const double *h_pose7_twc, double thickness, int min_inliers, int max_planes,
               int num_iterations, uint32_t seed, const uint32_t *h_rand3, int n_prior, const float *h_prior24, float *h_planes24, int *h_info8,
               int *d_labels, double *h_moments) {
    ALVA_ARG(ctx && h_pose7_twc && h_planes24 && h_info8);
    ALVA_ARG(n >= 0 && n <= PL_N_CAP && (d_points || n == 0));
    ALVA_ARG(thickness > 0 && std::isfinite(thickness));
    ALVA_ARG(min_inliers >= 8 && min_inliers <= PL_N_CAP && max_planes >= 1 && max_planes <= PL_MAX_PLANES);
    ALVA_ARG(num_iterations >= 1 && num_iterations <= PL_MAX_ITERS);
    ALVA_ARG(n_prior >= 0 && n_prior <= max_planes && (h_prior24 || n_prior == 0));
    const int rounds = max_planes - n_prior;
    TrackArgs T{};
    PlaneArgs &A = T.R;
    T.n_prior = n_prior;
    for (int j = 0; j < n_prior; j++) {   // T0
        const float *rec = h_prior24 + 24 * j;
        bool ok = rec[15] == 1.f;
        for (int k = 0; k < 24; k++) ok = ok && std::isfinite(rec[k]);
        if (ok) T.usable |= 1u << j;
        for (int k = 0; k < 3; k++) {
            T.prior[j][k] = (double) rec[12 + k];
            T.prior[j][3 + k] = (double) rec[4 + k];
        }
    }
    memset(h_planes24, 0, (size_t) max_planes * 24 * sizeof(float));
    memset(h_info8, 0, (size_t) max_planes * 8 * sizeof(int));
    if (h_moments) memset(h_moments, 0, (size_t) max_planes * 10 * sizeof(double));
    for (int r = n_prior; r < max_planes; r++) {   // not run, until a round says otherwise
        h_info8[8 * r] = 5;
        h_info8[8 * r + 2] = -1;
    }
    if (n == 0) {   // nothing is launched: no prior claims a point, and the first round has too few
        for (int j = 0; j < n_prior; j++) {
            h_info8[8 * j] = (T.usable >> j) & 1u ? 7 : 9;
            h_info8[8 * j + 2] = -1;
            h_info8[8 * j + 5] = 1;
        }
        if (rounds > 0) h_info8[8 * n_prior] = 1;
        return 0;
    }
    // pinned: explicit sample words (tests) | one record per slot
    const size_t words_bytes = h_rand3 ? (size_t) rounds * num_iterations * 12 : 0, off_rec = (words_bytes + 255) / 256 * 256;
    uint8_t *pin = nullptr;
    int rc = alva_ctx_pinned(ctx, off_rec + (size_t) max_planes * sizeof(PlaneRecord), (void **) &pin);
    if (rc) return rc;
    // device: state | counts | two live lists (SoA coordinates, indices) | the refitted frames (split only)
    const size_t cap = (size_t) (n + 63) / 64 * 64;
    const size_t off_counts = 256, off_live = off_counts + ((size_t) num_iterations * 4 + 255) / 256 * 256, live_bytes = cap * (3 * 8 + 4);
    uint8_t *dev = nullptr;
    const size_t off_fits = off_live + 2 * live_bytes;   // (a multiple of 256: cap is one of 64, live_bytes of 28 x 64)
    const bool split = n_prior >= 2;   // one prior: nothing to share out, and the hand-over would only cost (1.8 us measured)
    rc = alva_ctx_scratch(ctx, PL_SCRATCH_SLOT, off_fits + (split ? sizeof(double) * PL_MAX_PLANES * 12 : 0), (void **) &dev);
    if (rc) return rc;
    if (h_rand3) memcpy(pin, h_rand3, words_bytes);
    A.pts = d_points;
    for (int b = 0; b < 2; b++) {
        A.live[b] = (double *) (dev + off_live + b * live_bytes);
        A.live_idx[b] = (int *) (dev + off_live + b * live_bytes + cap * 24);
    }
    A.counts = (int *) (dev + off_counts);
    A.state = (PlaneState *) dev;
    A.labels = d_labels;
    A.rand3 = h_rand3 ? (const uint32_t *) pin : nullptr;
    A.out = (PlaneRecord *) (pin + off_rec);
    A.n = n;
    A.cap = (int) cap;
    A.iters = num_iterations;
    A.min_inliers = min_inliers;
    A.grid = alva_divup(num_iterations, PL_WAVES) < PL_MAX_GRID ? alva_divup(num_iterations, PL_WAVES) : PL_MAX_GRID;
    A.seeded = n_prior > 0;   // without priors round 0 reads the input itself
    A.slot_base = n_prior;
    A.seed = seed;
    A.thickness = thickness;
    double R[9];
    memcpy(A.t, h_pose7_twc, sizeof(A.t));
    alva_slam::quat_to_rot(h_pose7_twc + 3, R);
    for (int k = 0; k < 3; k++) {
        A.a[k] = R[3 * k];
        A.b[k] = R[3 * k + 1];
    }
    memset(A.out, 0, (size_t) max_planes * sizeof(PlaneRecord));
    for (int r = n_prior; r < max_planes; r++) {
        A.out[r].info[0] = 5;
        A.out[r].info[2] = -1;
    }
    ALVA_HIP(hipMemsetAsync(dev, 0, sizeof(PlaneState), ctx->stream));
    if (d_labels) ALVA_HIP(hipMemsetAsync(d_labels, 0xff, (size_t) n * sizeof(int), ctx->stream));   // -1
    if (n_prior > 0) {
        T.split = split;
        T.fits = split ? (double *) (dev + off_fits) : nullptr;
        hipLaunchKernelGGL(k_track_claim, dim3(T.split ? n_prior : 1), dim3(PL_NT), 0, ctx->stream, T);
        ALVA_LAUNCH_CHECK();
    }
    rc = plane_rounds_enqueue(ctx, A, rounds);
    if (rc) return rc;
    ALVA_HIP(alva_stream_sync(ctx->stream));
    int found = 0;
    for (int r = 0; r < max_planes; r++) {
        PlaneRecord rec;
        memcpy(&rec, A.out + r, sizeof(rec));
        memcpy(h_info8 + 8 * r, rec.info, sizeof(rec.info));
        const bool refit_ran = r < n_prior ? rec.info[0] == 0 || rec.info[0] == 8 : rec.info[0] == 0 || rec.info[0] == 4;
        if (h_moments && refit_ran) memcpy(h_moments + 10 * r, rec.mom, sizeof(rec.mom));
        if (rec.info[0] != 0) continue;
        memcpy(h_planes24 + 24 * r, rec.plane, sizeof(rec.plane));
        found++;
    }
    return found;
}

}  // namespace

extern "C" int alva_detect_planes(alva_ctx *ctx, const double *d_points, int n, const double *h_pose7_twc, double thickness, int min_inliers,
                                  int max_planes, int num_iterations, uint32_t seed, const uint32_t *h_rand3, float *h_planes24, int *h_info8,
                                  int *d_labels, double *h_moments) {
    return planes_run(ctx, d_points, n, h_pose7_twc, thickness, min_inliers, max_planes, num_iterations, seed, h_rand3, 0, nullptr, h_planes24,
                      h_info8, d_labels, h_moments);
}

extern "C" int alva_track_planes(alva_ctx *ctx, const double *d_points, int n, const double *h_pose7_twc, double thickness, int min_inliers,
                                 int max_planes, int num_iterations, uint32_t seed, const uint32_t *h_rand3, int n_prior,
                                 const float *h_prior24, float *h_planes24, int *h_info8, int *d_labels, double *h_moments) {
    return planes_run(ctx, d_points, n, h_pose7_twc, thickness, min_inliers, max_planes, num_iterations, seed, h_rand3, n_prior, h_prior24,
                      h_planes24, h_info8, d_labels, h_moments);
}
