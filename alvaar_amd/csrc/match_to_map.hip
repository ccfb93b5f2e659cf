// f1: Mapper::matchToMap -- re-association of the local map with a new keyframe.
//
// Replaces the loops of Mapper::matchToMap (src/slam/src/mapper.cpp:354-588) for a CONSISTENT map (every keypoint id has
// its map point, every observing keyframe exists and holds the keypoint; the reference's repair branches :459-463, :500-509
// stay on the host).  Per local map point (:389-553): project into the frame (Sophus SE3 * point = Eigen quaternion rotation,
// CameraCalibration::projectCamToImageDist), visibility gates, the 2x2-cell keypoint neighbourhood of
// Frame::getSurroundingKeypoints (frame.cpp:313-341), and for each neighbouring keypoint: pixel distance, "never observed in
// the same keyframe", mean re-projection error of the map point in the keypoint's keyframes, minimum Hamming distance
// between the two descriptor sets (MapPoint::computeMinDescDist, map_point.cpp:206-222); best / second best with the 0.9
// ratio test.  Then per keypoint the closest map point wins, the last one on ties (:555-586).
//
// ONE matcher body (match_point) serves two forms of the map through a small view type that says where a map point's
// observations and descriptors are read from:
//   FlatView   the flattened arrays of alva_match_to_map / alva_match_to_map_flags (observation ranges obsPtr, descriptors per
//              observation, optional "has a descriptor" flags)
//   RowView    the rows gathered from the map layer's RECORDS (slam/mp_rec.hpp) by alva_match_to_map_records: the host names one
//              record slot per table row instead of flattening its map per keyframe; descriptors are read in place from the map
//              point's descriptor table (medoid_table.hpp, resident on the device: mapKeyframeDescriptors_ itself)
//
//   k_frame_obs     flat form: map point -> its observation in the frame (or -1)
//   k_mtm_gather    record form: ONE WAVE per row reads the record's header + live entries straight out of pinned host memory
//                   (zero-copy; the only bytes that cross PCIe are the ones the call needs: ~64 + 24 n_entries per row), keeps the
//                   observations whose keyframe exists and holds the keypoint (ballot compaction, ascending keyframe =
//                   observedKeyframeIds_ order), finds the row's observation in the frame, and lists the live slots of the descriptor
//                   table (what MapPoint::computeMinDescDist iterates)
//   k_match_local   match_point over FlatView
//   k_match_rows    match_point over RowView
//                   ONE WAVE per local map point; lane i evaluates the i-th neighbouring keypoint; the reference's sequential
//                   two-minimum scan (<=) is reproduced with ballots: best = LAST lane holding the minimum, second = minimum
//                   of the rest
//   k_arbitrate     both forms: per keypoint the closest map point, the LAST one in list order on ties: match_point folds
//                   (distance, list position) into one 64-bit key per keypoint with atomicMax -- an order-independent
//                   maximum, so the result does not depend on which wave gets there first -- and this kernel decodes it
// Everything is integer / IEEE double / float in the reference's operation order (compile with -ffp-contract=off), so the
// result is the reference's, not an approximation of it.
#include "common.hpp"
#include "camera_device.hpp"
#include "hamming_device.hpp"
#include "slam/medoid_table.hpp"
#include "slam/mp_rec.hpp"
#include <cmath>

namespace {

using alva_slam::MpRec;
using alva_slam::ObsEnt;
using alva_slam::MP_ENT_CAP;

// what both forms share
struct MtmCommon {
    AlvaCam cam;
    double imgW, imgH;
    int cellSize, numCellsW, gridCells;
    const int *cellPtr, *cellMp;
    const double *kfQ, *kfT;
    int frameKf, nMp, nLocal;
    const int *local;
    float maxPxDist, minDist, viewTh;
    unsigned long long *arb;  // [nMp] per keypoint: ((~distance bits) << 32) | list position of the best claim, 0 = none
    int *matchOfMp;  // [nMp]
};

struct MtmArgs {
    MtmCommon c;
    const double *mpWpt;
    const uint8_t *mpIs3d, *mpHasDesc;  // mpHasDesc / obsHasDesc may be NULL: every observation carries a descriptor
    const int *obsPtr, *obsKf;
    const float *obsPx;
    const uint8_t *obsDesc, *obsHasDesc;
    int *frameObs;   // [nMp]
};

struct MtmRow {
    double X[3];
    int slot, n_obs, frame_obs, n_desc;
    uint8_t is3d, has_desc, pad[6];
    struct Obs {
        int kf;            // index into the keyframe table
        float px[2];
    } obs[MP_ENT_CAP];
    uint8_t desc_slot[alva_medoid::CAP];   // live slots of the descriptor table
};
static_assert(sizeof(MtmRow) == 576, "MtmRow layout");

struct MtmRecArgs {
    MtmCommon c;
    int nKf;
    const int *kfIds;
    const int *mpSlot;
    const MpRec *const *chunks;          // arena chunk table (device-readable; the chunks are pinned host memory)
    const alva_medoid::Table *tables;
    int frameKfId;
    MtmRow *rows;
};

// The views: a map point is its row index; an observation index is the view's own (obsBegin .. obsEnd, frameObs); Descs is where a
// map point's descriptors lie, which the body reads once per local map point, not once per candidate.
struct FlatView {
    const MtmArgs &A;
    __device__ bool matchable(int M) const {
        return A.frameObs[M] < 0 && A.mpIs3d[M] && (A.mpHasDesc ? A.mpHasDesc[M] != 0 : A.obsPtr[M] != A.obsPtr[M + 1]);
    }
    __device__ void world(int M, double *X) const {
#pragma unroll
        for (int k = 0; k < 3; k++) X[k] = A.mpWpt[3 * (size_t) M + k];
    }
    __device__ int frameObs(int K) const { return A.frameObs[K]; }
    __device__ bool hasDesc(int K) const { return !A.mpHasDesc || A.mpHasDesc[K]; }
    __device__ int obsBegin(int M) const { return A.obsPtr[M]; }
    __device__ int obsEnd(int M) const { return A.obsPtr[M + 1]; }
    __device__ int obsKf(int, int o) const { return A.obsKf[o]; }
    __device__ float2 obsPx(int, int o) const { return make_float2(A.obsPx[2 * (size_t) o], A.obsPx[2 * (size_t) o + 1]); }
    struct Descs {
        int a, b;   // the map point's observations
    };
    __device__ Descs descs(int M) const { return {A.obsPtr[M], A.obsPtr[M + 1]}; }
    __device__ int minDescDist(const Descs &m, int K) const {
        const Descs k = descs(K);
        int dmin = 1000;
        for (int a = m.a; a < m.b; a++)
            for (int b = k.a; b < k.b; b++)
                if (!A.obsHasDesc || (A.obsHasDesc[a] && A.obsHasDesc[b]))
                    dmin = min(dmin, alva_hamming256_dev(reinterpret_cast<const uint4 *>(A.obsDesc + 32 * (size_t) a),
                                                         reinterpret_cast<const uint4 *>(A.obsDesc + 32 * (size_t) b)));
        return dmin;
    }
};

struct RowView {
    const MtmRecArgs &A;
    __device__ bool matchable(int M) const { return A.rows[M].frame_obs < 0 && A.rows[M].is3d && A.rows[M].has_desc; }
    __device__ void world(int M, double *X) const {
#pragma unroll
        for (int k = 0; k < 3; k++) X[k] = A.rows[M].X[k];
    }
    __device__ int frameObs(int K) const { return A.rows[K].frame_obs; }
    __device__ bool hasDesc(int K) const { return A.rows[K].has_desc; }
    __device__ int obsBegin(int) const { return 0; }
    __device__ int obsEnd(int M) const { return A.rows[M].n_obs; }
    __device__ int obsKf(int M, int o) const { return A.rows[M].obs[o].kf; }
    __device__ float2 obsPx(int M, int o) const { return make_float2(A.rows[M].obs[o].px[0], A.rows[M].obs[o].px[1]); }
    struct Descs {
        const alva_medoid::Table *t;
        const uint8_t *live;   // the table's live slots
        int n;
    };
    __device__ Descs descs(int M) const { return {A.tables + A.rows[M].slot, A.rows[M].desc_slot, A.rows[M].n_desc}; }
    __device__ int minDescDist(const Descs &m, int K) const {   // every pair of the two descriptor tables
        const Descs k = descs(K);
        int dmin = 1000;
        for (int a = 0; a < m.n; a++) {
            const uint4 *da = reinterpret_cast<const uint4 *>(m.t->slot[m.live[a]].desc);
            for (int b = 0; b < k.n; b++)
                dmin = min(dmin, alva_hamming256_dev(da, reinterpret_cast<const uint4 *>(k.t->slot[k.live[b]].desc)));
        }
        return dmin;
    }
};

__device__ __forceinline__ float norm2f(float dx, float dy) { return (float) sqrt((double) dx * (double) dx + (double) dy * (double) dy); }

__global__ void __launch_bounds__(256) k_frame_obs(MtmArgs A) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= A.c.nMp) return;
    int fo = -1;
    for (int o = A.obsPtr[m]; o < A.obsPtr[m + 1]; o++)
        if (A.obsKf[o] == A.c.frameKf) fo = o;
    A.frameObs[m] = fo;
    A.c.arb[m] = 0ull;
}

__global__ void __launch_bounds__(256) k_mtm_gather(MtmRecArgs A) {
    __shared__ int s_kf[64];
    if ((int) threadIdx.x < A.nKf && threadIdx.x < 64) s_kf[threadIdx.x] = A.kfIds[threadIdx.x];
    __syncthreads();
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= A.c.nMp) return;
    const int slot = A.mpSlot[row];
    const MpRec *r = A.chunks[slot >> alva_slam::MP_CHUNK_SHIFT] + (slot & (alva_slam::MP_CHUNK - 1));
    // header: 6 x 8 bytes (X, inverse depth, id | anchor, flags)
    const unsigned long long *h8 = reinterpret_cast<const unsigned long long *>(r);
    const unsigned long long hv = lane < 6 ? __builtin_nontemporal_load(h8 + lane) : 0ull;
    const unsigned long long fl = __shfl(hv, 5);
    const int n_ent = (int) ((fl >> 24) & 0xffu);
    MtmRow *g = A.rows + row;
    // entries: kf | flags, px -- the first 16 of an entry's 24 bytes
    int kf = -1, kfi = -1;
    unsigned flags = 0;
    float px0 = 0.f, px1 = 0.f;
    if (lane < n_ent && lane < MP_ENT_CAP) {
        const unsigned long long *e8 = reinterpret_cast<const unsigned long long *>(r->ent + lane);
        const unsigned long long a = __builtin_nontemporal_load(e8), b = __builtin_nontemporal_load(e8 + 1);
        kf = (int) (unsigned) (a & 0xffffffffull);
        flags = (unsigned) ((a >> 32) & 0xffu);
        px0 = __uint_as_float((unsigned) (b & 0xffffffffull));
        px1 = __uint_as_float((unsigned) (b >> 32));
        for (int i = 0; i < A.nKf && i < 64; i++)
            if (s_kf[i] == kf) kfi = i;
    }
    const bool keep = (flags & alva_slam::MPF_OBS) && (flags & alva_slam::MPF_INKF) && kfi >= 0;
    const unsigned long long km = __ballot(keep);
    const int pos = __popcll(km & ((1ull << lane) - 1ull));
    if (keep) {
        g->obs[pos].kf = kfi;
        g->obs[pos].px[0] = px0;
        g->obs[pos].px[1] = px1;
    }
    const unsigned long long fm = __ballot(keep && kf == A.frameKfId);
    // the descriptor table's live slots
    const alva_medoid::Table *t = A.tables + slot;
    const int used = t->used;
    const bool live = lane < used && lane < alva_medoid::CAP && t->slot[lane].key != alva_medoid::FREE_KEY;
    const unsigned long long lm = __ballot(live);
    if (live) g->desc_slot[__popcll(lm & ((1ull << lane) - 1ull))] = (uint8_t) lane;
    if (lane < 3) g->X[lane] = __longlong_as_double((long long) hv);
    if (lane == 0) {
        g->slot = slot;
        g->n_obs = __popcll(km);
        g->frame_obs = fm ? __popcll(km & ((1ull << (63 - __clzll((long long) fm))) - 1ull)) : -1;
        g->n_desc = __popcll(lm);
        g->is3d = (uint8_t) (fl & 0xffu);
        g->has_desc = (uint8_t) ((fl >> 8) & 0xffu);
        A.c.arb[row] = 0ull;
    }
}

// One wave per local map point: Mapper::matchToMap's body for list position li, on the map as View presents it.
template <class View>
__device__ __forceinline__ void match_point(const MtmCommon &C, const View &V) {
    const int li = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (li >= C.nLocal) return;
    const int M = C.local[li];
    int outKp = -1;
    float outDist = 0.f;
    // wave-uniform gates (:393-433)
    bool go = V.matchable(M);
    double wpt[3] = {0, 0, 0}, campt[3];
    float pu = 0.f, pv = 0.f;
    if (go) {
        V.world(M, wpt);
        alva_se3_apply_dev(C.kfQ + 4 * (size_t) C.frameKf, C.kfT + 3 * (size_t) C.frameKf, wpt, campt);
        go = !(campt[2] < 0.1);
        if (go) {
            const float view_angle = (float) (campt[2] / sqrt((campt[0] * campt[0] + campt[1] * campt[1]) + campt[2] * campt[2]));
            go = !(fabsf(view_angle) < C.viewTh);
        }
        if (go) {
            alva_project_dist_dev(C.cam, campt[0], campt[1], campt[2], pu, pv);
            go = pu >= 0 && pv >= 0 && (double) pu < C.imgW && (double) pv < C.imgH;
        }
    }
    if (go) {
        // the 2 x 2 cells of Frame::getSurroundingKeypoints, in its loop order; their stored keypoints, flattened
        const int rkp = (int) floorf(pv / (float) C.cellSize), ckp = (int) floorf(pu / (float) C.cellSize);
        int cb[4], cn[4], total = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int r = rkp - 1 + (j >> 1), c = ckp - 1 + (j & 1), idx = r * C.numCellsW + c;
            const bool ok = !(r < 0 || c < 0 || idx > C.gridCells) && idx < C.gridCells;
            cb[j] = ok ? C.cellPtr[idx] : 0;
            cn[j] = ok ? C.cellPtr[idx + 1] - cb[j] : 0;
            total += cn[j];
        }
        const int ma = V.obsBegin(M), mb = V.obsEnd(M);
        const typename View::Descs md = V.descs(M);
        // running state of the reference's scan: (bestDist, bestId), (secDist, secId valid?)
        float bestD = C.minDist, secD = C.minDist;
        int bestK = -1, nValid = 0;
        for (int base = 0; base < total; base += 64) {
            const int i = base + lane;
            bool valid = false;
            float dist = 0.f;
            int K = -1;
            if (i < total) {
                int j = 0, off = i;
                while (off >= cn[j]) {
                    off -= cn[j];
                    j++;
                }
                K = C.cellMp[cb[j] + off];
                // (a grid entry whose map point does not observe the frame keyframe -- the host's guard against it runs only under
                // ALVA_CHECK_OBS_MIRROR -- is no candidate.  Compared with the -1 that k_frame_obs / k_mtm_gather write, not `>= 0`:
                // told that the index is non-negative the compiler keeps a zero high word live across the loop, 2 VGPRs in k_match_local)
                const int ko = V.frameObs(K), ka = V.obsBegin(K), kb = V.obsEnd(K);
                float pxDist = 0.f;
                if (ko != -1) {
                    const float2 kp = V.obsPx(K, ko);
                    pxDist = norm2f(pu - kp.x, pv - kp.y);
                }
                bool cand = ko != -1 && !(pxDist > C.maxPxDist);
                if (!V.hasDesc(K)) cand = false;  // kpMapPoint->desc_.empty() (:465-468)
                if (cand)  // never both observed in one keyframe (:474-485)
                    for (int a = ka; a < kb && cand; a++)
                        for (int b = ma; b < mb; b++)
                            if (V.obsKf(K, a) == V.obsKf(M, b)) {
                                cand = false;
                                break;
                            }
                if (cand) {  // mean re-projection error of the map point in the keypoint's keyframes (:487-515)
                    float coProj = 0.f;
                    int nCo = 0;
                    for (int a = ka; a < kb; a++) {
                        double cp[3];
                        float qu, qv;
                        const int kf = V.obsKf(K, a);
                        alva_se3_apply_dev(C.kfQ + 4 * (size_t) kf, C.kfT + 3 * (size_t) kf, wpt, cp);
                        alva_project_dist_dev(C.cam, cp[0], cp[1], cp[2], qu, qv);
                        const float2 op = V.obsPx(K, a);
                        const float dx = op.x - qu, dy = op.y - qv;
                        coProj = (float) ((double) coProj + sqrt((double) dx * (double) dx + (double) dy * (double) dy));
                        nCo++;
                    }
                    cand = !(coProj / (float) nCo > C.maxPxDist);
                }
                if (cand) {  // MapPoint::computeMinDescDist (map_point.cpp:206-222)
                    dist = (float) V.minDescDist(md, K);
                    valid = dist <= C.minDist;  // larger distances fail both `<=` tests of the scan (:519-531)
                }
            }
            // fold this chunk into the scan state: best = LAST minimum, second = minimum of everything else seen
            const unsigned long long vm = __ballot(valid);
            if (vm) {
                float cmin = valid ? dist : 3.0e38f;
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) cmin = fminf(cmin, __shfl_xor(cmin, off));
                const unsigned long long mm = __ballot(valid && dist == cmin);
                const int lastLane = 63 - __clzll((long long) mm);
                float rest = (valid && lane != lastLane) ? dist : 3.0e38f;
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) rest = fminf(rest, __shfl_xor(rest, off));
                const int cK = __shfl(K, lastLane);
                // merge (bestD, secD) [earlier] with (cmin @ cK, rest) [later]
                if (cmin <= bestD) {
                    const float oldBest = nValid > 0 ? bestD : 3.0e38f, oldSec = nValid > 1 ? secD : 3.0e38f;
                    secD = fminf(fminf(oldBest, oldSec), rest);
                    bestD = cmin;
                    bestK = cK;
                } else {
                    const float oldSec = nValid > 1 ? secD : 3.0e38f;
                    secD = fminf(oldSec, cmin);
                }
                nValid += __popcll(vm);
            }
        }
        if (bestK != -1 && nValid > 1)
            if (0.9 * (double) secD < (double) bestD) bestK = -1;  // :534-540
        outKp = bestK;
        outDist = bestD;
    }
    if (lane == 0 && outKp >= 0) {
        // smaller distance wins, then the later list position (the reference scans the claims in push order with <=, :563-578)
        const unsigned long long key = ((unsigned long long) (0xffffffffu - __float_as_uint(outDist)) << 32) | (unsigned) (li + 1);
        atomicMax(&C.arb[outKp], key);
    }
}

__global__ void __launch_bounds__(256) k_match_local(MtmArgs A) { match_point(A.c, FlatView{A}); }

__global__ void __launch_bounds__(256) k_match_rows(MtmRecArgs A) { match_point(A.c, RowView{A}); }

__global__ void __launch_bounds__(256) k_arbitrate(const unsigned long long *__restrict__ arb, const int *__restrict__ local,
                                                   int *__restrict__ matchOfMp, int nMp) {
    const int K = blockIdx.x * 256 + threadIdx.x;
    if (K >= nMp) return;
    const unsigned li1 = (unsigned) (arb[K] & 0xffffffffull);
    matchOfMp[K] = li1 ? local[li1 - 1] : -1;
}

// What the entry points share: the common block with the thresholds, and scratch slot 7 = [front bytes of the form | arb [n_mp]].
int mtm_common(alva_ctx *ctx, const double *h_calib10, int cell_size, int num_cells_w, int grid_cells, const int *d_cell_ptr, const int *d_cell_mp,
               const double *d_kf_q, const double *d_kf_t, int frame_kf, int n_mp, int num_keypoints_3d, int n_local, const int *d_local,
               float max_proj_err, float dist_ratio, int *d_match_of_mp, size_t off_arb, MtmCommon &C, uint8_t **base) {
    C.cam = {h_calib10[0], h_calib10[1], h_calib10[2], h_calib10[3], h_calib10[4], h_calib10[5], h_calib10[6], h_calib10[7]};
    C.imgW = h_calib10[8]; C.imgH = h_calib10[9];
    C.cellSize = cell_size; C.numCellsW = num_cells_w; C.gridCells = grid_cells;
    C.cellPtr = d_cell_ptr; C.cellMp = d_cell_mp; C.kfQ = d_kf_q; C.kfT = d_kf_t;
    C.frameKf = frame_kf; C.nMp = n_mp; C.nLocal = n_local; C.local = d_local;
    // thresholds exactly as the reference forms them (:364-387, :439): floats, atanf / cosf of the host libm
    const float fovV = 0.5 * h_calib10[9] / h_calib10[1], fovH = 0.5 * h_calib10[8] / h_calib10[0];
    const float maxRadFov = fovH > fovV ? std::atan(fovH) : std::atan(fovV);
    C.viewTh = std::cos(maxRadFov);
    float maxPxDist = max_proj_err;
    if (num_keypoints_3d < 30) maxPxDist *= 2.;
    C.maxPxDist = maxPxDist;
    C.minDist = 32 * dist_ratio * 8.;
    int rc = alva_ctx_scratch(ctx, 7, off_arb + (size_t) n_mp * 8, (void **) base);
    if (rc) return rc;
    C.arb = (unsigned long long *) (*base + off_arb);
    C.matchOfMp = d_match_of_mp;
    return ALVA_OK;
}

// the match kernel of the form, then the arbitration
template <class Args>
int mtm_match(alva_ctx *ctx, void (*k_match)(Args), const Args &A) {
    const MtmCommon &C = A.c;
    if (C.nLocal > 0) hipLaunchKernelGGL(k_match, dim3(alva_divup(C.nLocal, 4)), dim3(256), 0, ctx->stream, A);
    hipLaunchKernelGGL(k_arbitrate, dim3(alva_divup(C.nMp, 256)), dim3(256), 0, ctx->stream, C.arb, C.local, C.matchOfMp, C.nMp);
    ALVA_LAUNCH_CHECK();
    return ALVA_OK;
}

}  // namespace

extern "C" int alva_match_to_map(alva_ctx *ctx, const double *h_calib10, int cell_size, int num_cells_w, int grid_cells, const int *d_cell_ptr,
                                 const int *d_cell_mp, int n_kf, const double *d_kf_q, const double *d_kf_t, int n_mp, const double *d_mp_wpt,
                                 const uint8_t *d_mp_is3d, const int *d_obs_ptr, const int *d_obs_kf, const float *d_obs_px,
                                 const uint8_t *d_obs_desc, int frame_kf, int num_keypoints_3d, int n_local, const int *d_local,
                                 float max_proj_err, float dist_ratio, int *d_match_of_mp) {
    return alva_match_to_map_flags(ctx, h_calib10, cell_size, num_cells_w, grid_cells, d_cell_ptr, d_cell_mp, n_kf, d_kf_q, d_kf_t, n_mp, d_mp_wpt,
                                   d_mp_is3d, nullptr, d_obs_ptr, d_obs_kf, d_obs_px, d_obs_desc, nullptr, frame_kf, num_keypoints_3d, n_local,
                                   d_local, max_proj_err, dist_ratio, d_match_of_mp);
}

extern "C" int alva_match_to_map_flags(alva_ctx *ctx, const double *h_calib10, int cell_size, int num_cells_w, int grid_cells,
                                       const int *d_cell_ptr, const int *d_cell_mp, int n_kf, const double *d_kf_q, const double *d_kf_t, int n_mp,
                                       const double *d_mp_wpt, const uint8_t *d_mp_is3d, const uint8_t *d_mp_has_desc, const int *d_obs_ptr,
                                       const int *d_obs_kf, const float *d_obs_px, const uint8_t *d_obs_desc, const uint8_t *d_obs_has_desc,
                                       int frame_kf, int num_keypoints_3d, int n_local, const int *d_local, float max_proj_err,
                                       float dist_ratio, int *d_match_of_mp) {
    ALVA_ARG(ctx && h_calib10 && cell_size > 0 && num_cells_w > 0 && grid_cells > 0 && n_kf > 0 && n_mp >= 0 && n_local >= 0);
    ALVA_ARG(frame_kf >= 0 && frame_kf < n_kf);
    if (n_mp == 0) return ALVA_OK;
    ALVA_ARG(d_cell_ptr && d_cell_mp && d_kf_q && d_kf_t && d_mp_wpt && d_mp_is3d && d_obs_ptr && d_obs_kf && d_obs_px && d_obs_desc &&
             d_match_of_mp && (n_local == 0 || d_local) && ((uintptr_t) d_obs_desc % 16) == 0);
    MtmArgs A{};
    uint8_t *base = nullptr;
    int rc = mtm_common(ctx, h_calib10, cell_size, num_cells_w, grid_cells, d_cell_ptr, d_cell_mp, d_kf_q, d_kf_t, frame_kf, n_mp, num_keypoints_3d,
                        n_local, d_local, max_proj_err, dist_ratio, d_match_of_mp, ((size_t) n_mp * 4 + 255) / 256 * 256, A.c, &base);
    if (rc) return rc;
    A.mpWpt = d_mp_wpt; A.mpIs3d = d_mp_is3d; A.mpHasDesc = d_mp_has_desc;
    A.obsPtr = d_obs_ptr; A.obsKf = d_obs_kf; A.obsPx = d_obs_px; A.obsDesc = d_obs_desc; A.obsHasDesc = d_obs_has_desc;
    A.frameObs = (int *) base;
    hipLaunchKernelGGL(k_frame_obs, dim3(alva_divup(n_mp, 256)), dim3(256), 0, ctx->stream, A);
    return mtm_match(ctx, k_match_local, A);
}

extern "C" int alva_match_to_map_records(alva_ctx *ctx, const double *h_calib10, int cell_size, int num_cells_w, int grid_cells,
                                         const int *d_cell_ptr, const int *d_cell_mp, int n_kf, const int *d_kf_ids, const double *d_kf_q,
                                         const double *d_kf_t, int frame_kf_index, int frame_kf_id, int n_mp, const int *d_mp_slot,
                                         const void *const *d_record_chunks, const void *d_desc_tables, int num_keypoints_3d, int n_local,
                                         const int *d_local, float max_proj_err, float dist_ratio, int *d_match_of_mp) {
    ALVA_ARG(ctx && h_calib10 && cell_size > 0 && num_cells_w > 0 && grid_cells > 0 && n_kf > 0 && n_kf <= 64 && n_mp >= 0 && n_local >= 0);
    ALVA_ARG(frame_kf_index >= 0 && frame_kf_index < n_kf);
    if (n_mp == 0) return ALVA_OK;
    ALVA_ARG(d_cell_ptr && d_cell_mp && d_kf_ids && d_kf_q && d_kf_t && d_mp_slot && d_record_chunks && d_desc_tables && d_match_of_mp &&
             (n_local == 0 || d_local));
    MtmRecArgs A{};
    uint8_t *base = nullptr;
    int rc = mtm_common(ctx, h_calib10, cell_size, num_cells_w, grid_cells, d_cell_ptr, d_cell_mp, d_kf_q, d_kf_t, frame_kf_index, n_mp,
                        num_keypoints_3d, n_local, d_local, max_proj_err, dist_ratio, d_match_of_mp, (size_t) n_mp * sizeof(MtmRow), A.c, &base);
    if (rc) return rc;
    A.nKf = n_kf; A.kfIds = d_kf_ids; A.mpSlot = d_mp_slot;
    A.chunks = reinterpret_cast<const MpRec *const *>(d_record_chunks);
    A.tables = static_cast<const alva_medoid::Table *>(d_desc_tables);
    A.frameKfId = frame_kf_id;
    A.rows = (MtmRow *) base;
    hipLaunchKernelGGL(k_mtm_gather, dim3(alva_divup(n_mp, 4)), dim3(256), 0, ctx->stream, A);
    return mtm_match(ctx, k_match_rows, A);
}
