// Image detection, the device stages: where a planar picture the app knows (a poster, a marker) lies in the frame (ARCore Augmented
// Images / ARKit ARImageAnchor / WebXR image-tracking; the reference has no counterpart, so the definitions in include/alvaar_hip.h are
// pinned by the numpy restatement tests/image_cases.py).
//
//   alva_image_match       the descriptors of up to 8 images (<= 512 each) against one frame's (<= 2048, the count read on the device): top-2
//                          with a ratio test, one-to-one, the kept pairs compacted per image in ascending query index with their
//                          coordinates.  The layout is reloc.hip's -- partial top-2 over (query block x row chunk), merge + claim, ordered
//                          emit -- and the scan of a chunk is the same function (hamming_device.hpp); here the tie-break id of a row is
//                          its index, and all images travel in one launch set.
//   alva_image_homography  counted-consensus RANSAC over 4-pair homographies, one launch for all images.  All decisions are IEEE double
//                          in the written operation order (compile with -ffp-contract=off).
//
// k_image_homography: one 256-thread workgroup per image.  The image's pairs (<= 512 x 4 doubles = 16 KB) are normalised into LDS once;
// then a LANE owns a whole hypothesis -- the 8 x 8 solve in registers (fully unrolled, the row exchange as selects, no scratch) and the
// count over the m pairs, which every lane reads at the same index (an LDS broadcast) -- so there is no cross-lane traffic until the
// winner: a max over the key (count, -it) through __shfl_xor and four LDS words.  The winning lane still holds its model; it hands the
// eight numbers over through LDS for the mask (one pair per thread) and the pose (one lane).  8 images x 4096 iterations is 128
// hypotheses per lane at the very most; the call is a few-Hz one and is bound by its launch and its wait, not by this.
#include "common.hpp"
#include "hamming_device.hpp"
#include "plane_fit.hpp"
#include <climits>
#include <cmath>

namespace {

constexpr int IMG_MAX = ALVA_IMAGE_MAX, IMG_QCAP = ALVA_IMAGE_QUERY_CAP, IMG_TCAP = ALVA_IMAGE_TRAIN_CAP;
constexpr int MQ = 256;   // queries per workgroup (four waves): an image is two workgroups wide
constexpr int MC = 64;    // train rows per workgroup (one LDS chunk)
constexpr int QBLOCKS = IMG_QCAP / MQ;

struct MatchArgs {
    const uint4 *qdesc;     // [n_images][IMG_QCAP][2]
    const float *qxy;       // [n_images][IMG_QCAP][2]
    const uint4 *tdesc;     // [train_cap][2]
    const float *txy;       // [train_cap][2]
    const int *ntrain;      // device: the frame's count
    int nq[IMG_MAX];
    int n_images, train_cap, max_dist;
    float ratio;
    AlvaTop2 *partial;              // [chunks][n_images * IMG_QCAP]
    int *cand;                      // [n_images * IMG_QCAP][2]: row, dist
    unsigned long long *claim;      // [n_images][train_cap]
    int *match;                     // [n_images][IMG_QCAP][3]
    double *xy;                     // [n_images][IMG_QCAP][4]
    int *count;                     // [n_images]
};

__device__ __forceinline__ int match_ntrain(const MatchArgs &A) {
    const int n = *A.ntrain;
    return n < 0 ? 0 : (n > A.train_cap ? A.train_cap : n);
}

__global__ void __launch_bounds__(MQ) k_image_partial(const MatchArgs A) {
    __shared__ uint4 s_d[MC * 2];
    __shared__ int s_id[MC];
    const int tid = threadIdx.x, img = blockIdx.x / QBLOCKS, qb = blockIdx.x % QBLOCKS;
    const int nt = match_ntrain(A), r0 = blockIdx.y * MC;
    if (r0 >= nt) return;   // (uniform) past the frame's rows: the merge does not read this chunk
    const int rcount = min(MC, nt - r0);
    if (tid < rcount) {
        s_id[tid] = r0 + tid;   // ties go to the lower train index
        s_d[2 * tid] = A.tdesc[2 * (size_t) (r0 + tid)];
        s_d[2 * tid + 1] = A.tdesc[2 * (size_t) (r0 + tid) + 1];
        if (qb == 0) A.claim[(size_t) img * A.train_cap + r0 + tid] = ~0ull;   // the merge's one-to-one claims start empty
    }
    const int qi = qb * MQ + tid, nq = A.nq[img];
    uint4 qa = make_uint4(0, 0, 0, 0), qbv = qa;
    if (qi < nq) {
        qa = A.qdesc[2 * ((size_t) img * IMG_QCAP + qi)];
        qbv = A.qdesc[2 * ((size_t) img * IMG_QCAP + qi) + 1];
    }
    __syncthreads();
    int bd = ALVA_TOP2_NO_DIST, bid = INT_MAX, brow = -1, bs = ALVA_TOP2_NO_DIST;
    alva_top2_scan(qa, qbv, s_d, s_id, rcount, r0, bd, bid, brow, bs);
    if (qi < nq) A.partial[(size_t) blockIdx.y * (A.n_images * IMG_QCAP) + img * IMG_QCAP + qi] = AlvaTop2{bd, bid, brow, bs};
}

__global__ void __launch_bounds__(MQ) k_image_merge(const MatchArgs A) {
    const int img = blockIdx.x / QBLOCKS, qi = (blockIdx.x % QBLOCKS) * MQ + threadIdx.x;
    if (qi >= A.nq[img]) return;
    const int nt = match_ntrain(A), chunks = (nt + MC - 1) / MC;
    const int slot = img * IMG_QCAP + qi;
    int bd = ALVA_TOP2_NO_DIST, bid = INT_MAX, brow = -1, bs = ALVA_TOP2_NO_DIST;
    for (int c = 0; c < chunks; c++) {
        const AlvaTop2 p = A.partial[(size_t) c * (A.n_images * IMG_QCAP) + slot];
        alva_top2_merge(bd, bid, brow, bs, p.d, p.id, p.row, p.second);
    }
    const bool ok = brow >= 0 && bd <= A.max_dist && (float) bd < A.ratio * (float) bs;
    A.cand[2 * slot] = ok ? brow : -1;
    A.cand[2 * slot + 1] = bd;
    if (ok) atomicMin(&A.claim[(size_t) img * A.train_cap + brow], ((unsigned long long) (unsigned) bd << 32) | (unsigned) qi);
}

// per image: the kept pairs in ascending query index (a ballot prefix per wave, wave offsets in LDS), coordinates gathered as doubles
__global__ void __launch_bounds__(IMG_QCAP) k_image_emit(const MatchArgs A) {
    constexpr int NW = IMG_QCAP / 64;
    __shared__ int s_w[NW];
    const int img = blockIdx.x, qi = threadIdx.x, lane = qi & 63, wave = qi >> 6;
    int row = -1, dist = 0;
    if (qi < A.nq[img]) {
        const int slot = img * IMG_QCAP + qi;
        row = A.cand[2 * slot];
        dist = A.cand[2 * slot + 1];
        if (row >= 0 && A.claim[(size_t) img * A.train_cap + row] != (((unsigned long long) (unsigned) dist << 32) | (unsigned) qi)) row = -1;
    }
    const unsigned long long bal = __ballot(row >= 0);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) s_w[wave] = __popcll(bal);
    __syncthreads();
    int off = 0, total = 0;
    for (int w = 0; w < NW; w++) {
        if (w < wave) off += s_w[w];
        total += s_w[w];
    }
    if (row >= 0) {
        const size_t o = (size_t) img * IMG_QCAP + off + before;
        A.match[3 * o] = qi;
        A.match[3 * o + 1] = row;
        A.match[3 * o + 2] = dist;
        const float *q = A.qxy + 2 * ((size_t) img * IMG_QCAP + qi), *t = A.txy + 2 * (size_t) row;
        A.xy[4 * o] = (double) q[0];
        A.xy[4 * o + 1] = (double) q[1];
        A.xy[4 * o + 2] = (double) t[0];
        A.xy[4 * o + 3] = (double) t[1];
    }
    if (qi == 0) A.count[img] = total;
}

// ---- the homography stage

constexpr int HOM_NT = 256, HOM_WAVES = HOM_NT / 64;

struct HomRecord {   // one per image, in pinned memory (zeroed by the host before the launch)
    double H[9], R[9], t[3];
    int info[8];
    uint8_t mask[IMG_QCAP];
};

struct HomArgs {
    const double *xy;    // [n_images][IMG_QCAP][4]: x, y (image pixels), u, v (undistorted frame pixels)
    const int *count;    // [n_images], device
    int wh[2 * IMG_MAX];
    double half_w, half_h, s;   // W / 2, H / 2, max(W, H) / 2
    double fx, fy, cx, cy;
    double thr2;
    int iters, min_inliers;
    uint32_t seed;
    const uint32_t *rand4;   // [iters][4] explicit sample words (pinned), or null
    HomRecord *out;
};

// h11 .. h32 (h33 = 1) through four pairs: rows (u-row, v-row) per pair in sample order, Gaussian elimination with partial pivoting (the
// largest |a| of the column, the lowest row on ties), false when a pivot is not > 1e-12, then back substitution
__device__ __forceinline__ bool hom_solve(const double (&px)[4], const double (&py)[4], const double (&qx)[4], const double (&qy)[4],
                                          double (&h)[8]) {
    double a[8][9];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const double x = px[i], y = py[i], u = qx[i], v = qy[i];
        a[2 * i][0] = x; a[2 * i][1] = y; a[2 * i][2] = 1.0; a[2 * i][3] = 0.0; a[2 * i][4] = 0.0; a[2 * i][5] = 0.0;
        a[2 * i][6] = -(x * u); a[2 * i][7] = -(y * u); a[2 * i][8] = u;
        a[2 * i + 1][0] = 0.0; a[2 * i + 1][1] = 0.0; a[2 * i + 1][2] = 0.0; a[2 * i + 1][3] = x; a[2 * i + 1][4] = y; a[2 * i + 1][5] = 1.0;
        a[2 * i + 1][6] = -(x * v); a[2 * i + 1][7] = -(y * v); a[2 * i + 1][8] = v;
    }
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        int piv = k;
        double best = fabs(a[k][k]);
#pragma unroll
        for (int r = k + 1; r < 8; r++) {
            const double v = fabs(a[r][k]);
            if (v > best) {
                best = v;
                piv = r;
            }
        }
        ok = ok && best > 1e-12;
#pragma unroll
        for (int r = k + 1; r < 8; r++) {
            const bool sw = piv == r;
#pragma unroll
            for (int c = k; c < 9; c++) {
                const double top = a[k][c], low = a[r][c];
                a[k][c] = sw ? low : top;
                a[r][c] = sw ? top : low;
            }
        }
#pragma unroll
        for (int r = k + 1; r < 8; r++) {
            const double f = a[r][k] / a[k][k];
#pragma unroll
            for (int c = k + 1; c < 9; c++) a[r][c] = a[r][c] - f * a[k][c];
        }
    }
    if (!ok) return false;   // (the arithmetic past a rejected pivot is discarded)
#pragma unroll
    for (int k = 7; k >= 0; k--) {
        double sum = a[k][8];
#pragma unroll
        for (int c = k + 1; c < 8; c++) sum = sum - a[k][c] * h[c];
        h[k] = sum / a[k][k];
    }
    return true;
}

__device__ __forceinline__ double hom_w(const double (&h)[8], double x, double y) { return (h[6] * x + h[7] * y) + 1.0; }

// the pair counts for h: w > 0 and the squared forward transfer error, in pixels, <= thr2
__device__ __forceinline__ bool hom_inlier(const double (&h)[8], double x, double y, double u, double v, double s, double thr2) {
    const double w = hom_w(h, x, y);
    const double X = (h[0] * x + h[1] * y) + h[2], Y = (h[3] * x + h[4] * y) + h[5];
    const double dx = (X / w - u) * s, dy = (Y / w - v) * s;
    return w > 0 && dx * dx + dy * dy <= thr2;
}

__global__ void __launch_bounds__(HOM_NT) k_image_homography(const HomArgs A) {
    __shared__ double Px[IMG_QCAP], Py[IMG_QCAP], Qx[IMG_QCAP], Qy[IMG_QCAP];
    __shared__ int s_key[HOM_WAVES];
    __shared__ double s_h[8];
    const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    HomRecord *out = A.out + img;
    int m = A.count[img];
    m = m < 0 ? 0 : (m > IMG_QCAP ? IMG_QCAP : m);
    if (tid == 0) {
        out->info[1] = m;
        out->info[2] = -1;
    }
    if (m < 4 || m < A.min_inliers) {   // (uniform)
        if (tid == 0) out->info[0] = 1;
        return;
    }
    const double w = (double) A.wh[2 * img], hh = (double) A.wh[2 * img + 1];
    for (int i = tid; i < m; i += HOM_NT) {
        const double *p = A.xy + 4 * ((size_t) img * IMG_QCAP + i);
        Px[i] = (p[0] - w / 2) / w;
        Py[i] = (p[1] - hh / 2) / w;
        Qx[i] = (p[2] - A.half_w) / A.s;
        Qy[i] = (p[3] - A.half_h) / A.s;
    }
    __syncthreads();

    // ---- hypotheses: iteration tid, tid + 256, ... on this lane; the first of equal counts stays
    int best_key = -1;
    double hb[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int it = tid; it < A.iters; it += HOM_NT) {
        int idx[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t word = A.rand4 ? A.rand4[4 * (size_t) it + j] : alva_hash32(A.seed ^ ((4u * (uint32_t) it + (uint32_t) j) * 0x9E3779B9u));
            idx[j] = alva_sample_index(word, m);
        }
        if (idx[0] == idx[1] || idx[0] == idx[2] || idx[0] == idx[3] || idx[1] == idx[2] || idx[1] == idx[3] || idx[2] == idx[3]) continue;
        double px[4], py[4], qx[4], qy[4], h[8];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            px[j] = Px[idx[j]]; py[j] = Py[idx[j]]; qx[j] = Qx[idx[j]]; qy[j] = Qy[idx[j]];
        }
        if (!hom_solve(px, py, qx, qy, h)) continue;
        bool front = true;
#pragma unroll
        for (int j = 0; j < 4; j++) front = front && hom_w(h, px[j], py[j]) > 0;
        if (!front) continue;
        int cnt = 0;
        for (int i = 0; i < m; i++) cnt += hom_inlier(h, Px[i], Py[i], Qx[i], Qy[i], A.s, A.thr2) ? 1 : 0;
        const int key = cnt * 4096 + (4095 - it);   // count <= 512, it < 4096: the largest count, then the lowest iteration
        if (key > best_key) {
            best_key = key;
#pragma unroll
            for (int c = 0; c < 8; c++) hb[c] = h[c];
        }
    }
    int wkey = best_key;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) wkey = max(wkey, __shfl_xor(wkey, d));
    if (lane == 0) s_key[wave] = wkey;
    __syncthreads();
    int win = s_key[0];
#pragma unroll
    for (int k = 1; k < HOM_WAVES; k++) win = max(win, s_key[k]);
    if (win < 0) {   // (uniform) no hypothesis survived
        if (tid == 0) out->info[0] = 2;
        return;
    }
    if (best_key == win) {   // one lane: an iteration belongs to one lane
#pragma unroll
        for (int c = 0; c < 8; c++) s_h[c] = hb[c];
    }
    __syncthreads();
    double h[8];
#pragma unroll
    for (int c = 0; c < 8; c++) h[c] = s_h[c];
    const int win_cnt = win / 4096, win_it = 4095 - win % 4096;
    for (int i = tid; i < m; i += HOM_NT) out->mask[i] = hom_inlier(h, Px[i], Py[i], Qx[i], Qy[i], A.s, A.thr2) ? 1 : 0;
    if (tid != 0) return;
    for (int c = 0; c < 8; c++) out->H[c] = h[c];
    out->H[8] = 1.0;
    out->info[2] = win_it;
    out->info[3] = win_cnt;
    if (win_cnt < A.min_inliers) {
        out->info[0] = 3;
        return;
    }
    // ---- pose: A = K^-1 (the frame normalisation undone) H; columns a1, a2 span the image, a3 is its centre
    const double sx = A.s / A.fx, sy = A.s / A.fy, ox = (A.half_w - A.cx) / A.fx, oy = (A.half_h - A.cy) / A.fy;
    double a[3][3];   // a[c] = column c
    for (int c = 0; c < 3; c++) {
        const double h0 = h[c], h1 = h[3 + c], h2 = c < 2 ? h[6 + c] : 1.0;
        a[c][0] = sx * h0 + ox * h2;
        a[c][1] = sy * h1 + oy * h2;
        a[c][2] = h2;
    }
    const double n1 = sqrt((a[0][0] * a[0][0] + a[0][1] * a[0][1]) + a[0][2] * a[0][2]);
    const double n2 = sqrt((a[1][0] * a[1][0] + a[1][1] * a[1][1]) + a[1][2] * a[1][2]);
    const double dot = (a[0][0] * a[1][0] + a[0][1] * a[1][1]) + a[0][2] * a[1][2];
    const double rat = n1 / n2;
    if (!(rat >= 0.5 && rat <= 2.0) || !(fabs(dot) / (n1 * n2) <= 0.5)) {
        out->info[0] = 4;
        return;
    }
    const double lam = 1.0 / sqrt(n1 * n2);
    const double r1[3] = {a[0][0] / n1, a[0][1] / n1, a[0][2] / n1};
    const double d = (r1[0] * a[1][0] + r1[1] * a[1][1]) + r1[2] * a[1][2];
    const double v[3] = {a[1][0] - d * r1[0], a[1][1] - d * r1[1], a[1][2] - d * r1[2]};
    const double nv = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    const double r2[3] = {v[0] / nv, v[1] / nv, v[2] / nv};
    const double r3[3] = {r1[1] * r2[2] - r1[2] * r2[1], r1[2] * r2[0] - r1[0] * r2[2], r1[0] * r2[1] - r1[1] * r2[0]};
    for (int r = 0; r < 3; r++) {
        out->R[3 * r] = r1[r];
        out->R[3 * r + 1] = r2[r];
        out->R[3 * r + 2] = r3[r];
        out->t[r] = lam * a[2][r];
    }
    out->info[0] = 0;
}

}  // namespace

extern "C" int alva_image_match(alva_ctx *ctx, int n_images, const uint8_t *d_qdesc, const float *d_qxy, const int *h_nq, const uint8_t *d_tdesc,
                                const float *d_txy, const int *d_ntrain, int train_cap, int max_dist, float ratio, int *d_match, double *d_xy,
                                int *d_count) {
    ALVA_ARG(ctx && n_images >= 1 && n_images <= IMG_MAX && h_nq && d_ntrain && d_match && d_xy && d_count);
    ALVA_ARG(train_cap >= 0 && train_cap <= IMG_TCAP && ratio >= 0.f && max_dist >= 0);
    ALVA_ARG(d_qdesc && ((uintptr_t) d_qdesc % 16) == 0 && d_qxy);
    ALVA_ARG(train_cap == 0 || (d_tdesc && ((uintptr_t) d_tdesc % 16) == 0 && d_txy));
    for (int j = 0; j < n_images; j++) ALVA_ARG(h_nq[j] >= 0 && h_nq[j] <= IMG_QCAP);
    const int chunks = alva_divup(train_cap, MC), slots = n_images * IMG_QCAP;
    const size_t part_bytes = ((size_t) chunks * slots * sizeof(AlvaTop2) + 255) / 256 * 256;
    const size_t cand_bytes = (size_t) slots * 8;
    uint8_t *scr = nullptr;
    const int rc = alva_ctx_scratch(ctx, 0, part_bytes + cand_bytes + (size_t) n_images * train_cap * 8 + 256, (void **) &scr);
    if (rc) return rc;
    MatchArgs A{};
    A.qdesc = (const uint4 *) d_qdesc;
    A.qxy = d_qxy;
    A.tdesc = (const uint4 *) d_tdesc;
    A.txy = d_txy;
    A.ntrain = d_ntrain;
    memcpy(A.nq, h_nq, (size_t) n_images * sizeof(int));
    A.n_images = n_images;
    A.train_cap = train_cap;
    A.max_dist = max_dist;
    A.ratio = ratio;
    A.partial = (AlvaTop2 *) scr;
    A.cand = (int *) (scr + part_bytes);
    A.claim = (unsigned long long *) (scr + part_bytes + cand_bytes);
    A.match = d_match;
    A.xy = d_xy;
    A.count = d_count;
    if (chunks > 0) {
        hipLaunchKernelGGL(k_image_partial, dim3(n_images * QBLOCKS, chunks), dim3(MQ), 0, ctx->stream, A);
        ALVA_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_image_merge, dim3(n_images * QBLOCKS), dim3(MQ), 0, ctx->stream, A);
    ALVA_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_image_emit, dim3(n_images), dim3(IMG_QCAP), 0, ctx->stream, A);
    ALVA_LAUNCH_CHECK();
    return ALVA_OK;
}

extern "C" int alva_image_homography(alva_ctx *ctx, int n_images, const double *d_xy, const int *d_count, const int *h_wh, int frame_w,
                                     int frame_h, const double *h_calib4, int num_iterations, float threshold_px, int min_inliers, uint32_t seed,
                                     const uint32_t *h_rand4, double *h_H9, int *h_info8, uint8_t *h_mask, double *h_R9, double *h_t3) {
    ALVA_ARG(ctx && n_images >= 1 && n_images <= IMG_MAX && d_xy && d_count && h_wh && h_calib4 && h_H9 && h_info8 && h_mask && h_R9 && h_t3);
    ALVA_ARG(frame_w >= 1 && frame_h >= 1 && num_iterations >= 1 && num_iterations <= 4096 && threshold_px >= 0.f && min_inliers >= 0);
    for (int j = 0; j < n_images; j++) ALVA_ARG(h_wh[2 * j] >= 1 && h_wh[2 * j + 1] >= 1);
    // pinned: explicit sample words (tests) | one record per image
    const size_t off_rec = h_rand4 ? ((size_t) num_iterations * 16 + 255) / 256 * 256 : 0;
    uint8_t *pin = nullptr;
    const int rc = alva_ctx_pinned(ctx, off_rec + (size_t) n_images * sizeof(HomRecord), (void **) &pin);
    if (rc) return rc;
    if (h_rand4) memcpy(pin, h_rand4, (size_t) num_iterations * 16);
    HomArgs A{};
    A.xy = d_xy;
    A.count = d_count;
    memcpy(A.wh, h_wh, (size_t) n_images * 2 * sizeof(int));
    A.half_w = (double) frame_w / 2;
    A.half_h = (double) frame_h / 2;
    A.s = (double) (frame_w > frame_h ? frame_w : frame_h) / 2;
    A.fx = h_calib4[0]; A.fy = h_calib4[1]; A.cx = h_calib4[2]; A.cy = h_calib4[3];
    A.thr2 = (double) threshold_px * (double) threshold_px;
    A.iters = num_iterations;
    A.min_inliers = min_inliers;
    A.seed = seed;
    A.rand4 = h_rand4 ? (const uint32_t *) pin : nullptr;
    A.out = (HomRecord *) (pin + off_rec);
    memset(A.out, 0, (size_t) n_images * sizeof(HomRecord));
    hipLaunchKernelGGL(k_image_homography, dim3(n_images), dim3(HOM_NT), 0, ctx->stream, A);
    ALVA_LAUNCH_CHECK();
    ALVA_HIP(alva_stream_sync(ctx->stream));
    for (int j = 0; j < n_images; j++) {
        const HomRecord *r = A.out + j;
        memcpy(h_H9 + 9 * j, r->H, sizeof(r->H));
        memcpy(h_R9 + 9 * j, r->R, sizeof(r->R));
        memcpy(h_t3 + 3 * j, r->t, sizeof(r->t));
        memcpy(h_info8 + 8 * j, r->info, sizeof(r->info));
        memcpy(h_mask + (size_t) IMG_QCAP * j, r->mask, IMG_QCAP);
    }
    return ALVA_OK;
}
