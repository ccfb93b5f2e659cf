// Relocalization: a global k = 2 Hamming match of a frame's descriptors against the map's record block, with a ratio test and a
// one-to-one resolution (no reference counterpart: the reference resets its map when tracking is lost; ORB-SLAM2 / OV²SLAM recover by
// matching against the map they have and solving an absolute pose, which is what this feeds).
//
// Rows are the 64-byte records alva_pack_map_records writes: {int32 stream, int32 id, f64 xyz[3], u8 desc[32]}, id = -1 = unused, in no
// particular order.  Every tie is broken by the map-point id, never by the row position, so the result does not depend on the row order:
//   best(q)   = the row minimising (popcount(q ^ desc_r), id_r) over rows with id >= 0
//   second(q) = the smallest distance over all other such rows (257 when there is none)
//   accepted  = best <= max_dist && (float) best < ratio * (float) second
//   one-to-one: of the accepted queries that share a best row, the smallest (distance, query index) keeps it
//   output    = the kept (query, row) pairs in ascending query index, with the pose solve's correspondences gathered beside them.
//
// Like a7 (hamming.hip) this is VALU-bound (24 N M integer operations against 32 (N + M) bytes), so the layout is the same:
// one wave holds 64 queries in registers (8 dwords per lane), a chunk of 64 train rows is staged in LDS and read back as wave-uniform
// broadcasts, the N x M rectangle is cut over a 2-D grid (query blocks x row chunks) so all CUs get work, and each workgroup leaves a
// mergeable top-2 record per query.  Three launches: partial top-2 -> merge + ratio test + claim -> ordered compaction + gather.
#include "common.hpp"
#include "hamming_device.hpp"
#include <climits>

namespace {

constexpr int RQ = 256;   // queries per workgroup (four waves)
constexpr int RC = 64;    // rows per workgroup (one LDS chunk): short chunks, so that a 2 000 x 10 000 match has ~2 waves per SIMD
constexpr int EMIT_NT = 1024;
constexpr int NO_DIST = ALVA_TOP2_NO_DIST;

// the top-2 record, its merge and the scan of a staged chunk are hamming_device.hpp's (shared with image_detect.hip)
using Top2 = AlvaTop2;

__global__ void __launch_bounds__(RQ) k_reloc_partial(const uint4 *__restrict__ q, int nq, const uint8_t *__restrict__ rows,
                                                      int nr, Top2 *__restrict__ partial /* [chunks][nq_pad] */, int nq_pad,
                                                      unsigned long long *__restrict__ claim /* [nr] */) {
    __shared__ uint4 s_d[RC * 2];
    __shared__ int s_id[RC];
    const int tid = threadIdx.x;
    const int r0 = blockIdx.y * RC;
    const int rcount = min(RC, nr - r0);
    if (tid < rcount) {
        const uint8_t *rec = rows + 64 * (size_t) (r0 + tid);
        s_id[tid] = reinterpret_cast<const int *>(rec)[1];
        s_d[2 * tid] = reinterpret_cast<const uint4 *>(rec + 32)[0];
        s_d[2 * tid + 1] = reinterpret_cast<const uint4 *>(rec + 32)[1];
        if (blockIdx.x == 0) claim[r0 + tid] = ~0ull;   // the merge's one-to-one claims start empty
    }
    const int qi = blockIdx.x * RQ + tid;
    uint4 qa = make_uint4(0, 0, 0, 0), qb = qa;
    if (qi < nq) {
        qa = q[2 * (size_t) qi];
        qb = q[2 * (size_t) qi + 1];
    }
    __syncthreads();
    int bd = NO_DIST, bid = INT_MAX, brow = -1, bs = NO_DIST;
    alva_top2_scan(qa, qb, s_d, s_id, rcount, r0, bd, bid, brow, bs);
    if (qi < nq) partial[(size_t) blockIdx.y * nq_pad + qi] = Top2{bd, bid, brow, bs};
}

// per query: the chunks' records merged, the acceptance tests, and a claim on the best row (smallest (distance, query index) wins)
__global__ void __launch_bounds__(256) k_reloc_merge(const Top2 *__restrict__ partial, int chunks, int nq, int nq_pad, const uint8_t *__restrict__ qvalid,
                                                     int max_dist, float ratio, int *__restrict__ cand /* [nq][2]: row, dist */,
                                                     unsigned long long *__restrict__ claim) {
    const int qi = blockIdx.x * 256 + threadIdx.x;
    if (qi >= nq) return;
    int bd = NO_DIST, bid = INT_MAX, brow = -1, bs = NO_DIST;
    for (int c = 0; c < chunks; c++) {
        const Top2 p = partial[(size_t) c * nq_pad + qi];
        alva_top2_merge(bd, bid, brow, bs, p.d, p.id, p.row, p.second);
    }
    const bool ok = (!qvalid || qvalid[qi]) && brow >= 0 && bd <= max_dist && (float) bd < ratio * (float) bs;
    cand[2 * qi] = ok ? brow : -1;
    cand[2 * qi + 1] = bd;
    if (ok) atomicMin(&claim[brow], ((unsigned long long) (unsigned) bd << 32) | (unsigned) qi);
}

// the kept pairs in ascending query index (one workgroup: a ballot prefix per wave, wave offsets in LDS), the correspondences gathered
__global__ void __launch_bounds__(EMIT_NT) k_reloc_emit(const int *__restrict__ cand, int nq, const unsigned long long *__restrict__ claim,
                                                        const uint8_t *__restrict__ rows, const double *__restrict__ qbv, const float *__restrict__ qunpx,
                                                        int *__restrict__ match /* [nq][4]: query, row, id, dist */, int *__restrict__ count,
                                                        double *__restrict__ obv, double *__restrict__ ouv, double *__restrict__ owpt) {
    constexpr int NW = EMIT_NT / 64;
    __shared__ int s_w[NW];
    __shared__ int s_base;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (int q0 = 0; q0 < nq; q0 += EMIT_NT) {
        const int qi = q0 + tid;
        int row = -1, dist = 0;
        if (qi < nq) {
            row = cand[2 * qi];
            dist = cand[2 * qi + 1];
            if (row >= 0 && claim[row] != (((unsigned long long) (unsigned) dist << 32) | (unsigned) qi)) row = -1;
        }
        const unsigned long long bal = __ballot(row >= 0);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) s_w[wave] = __popcll(bal);
        __syncthreads();
        int off = s_base;
        for (int w = 0; w < wave; w++) off += s_w[w];
        if (row >= 0) {
            const int o = off + before;
            const uint8_t *rec = rows + 64 * (size_t) row;
            match[4 * o] = qi;
            match[4 * o + 1] = row;
            match[4 * o + 2] = reinterpret_cast<const int *>(rec)[1];
            match[4 * o + 3] = dist;
            const double *x = reinterpret_cast<const double *>(rec + 8);
            if (owpt)
                for (int c = 0; c < 3; c++) owpt[3 * o + c] = x[c];
            if (obv && qbv)
                for (int c = 0; c < 3; c++) obv[3 * o + c] = qbv[3 * (size_t) qi + c];
            if (ouv && qunpx)
                for (int c = 0; c < 2; c++) ouv[2 * o + c] = (double) qunpx[2 * (size_t) qi + c];
        }
        __syncthreads();
        if (tid == 0) {
            int t = 0;
            for (int w = 0; w < NW; w++) t += s_w[w];
            s_base += t;
        }
        __syncthreads();
    }
    if (tid == 0) *count = s_base;
}

}  // namespace

extern "C" int alva_reloc_match(alva_ctx *ctx, const uint8_t *d_qdesc, const uint8_t *d_qvalid, int n_query, const double *d_qbv, const float *d_qunpx,
                                const uint8_t *d_rows, int n_rows, int max_dist, float ratio, int *d_match, int *d_count, double *d_bv, double *d_uv,
                                double *d_wpt) {
    ALVA_ARG(ctx && n_query >= 0 && n_rows >= 0 && d_count && ratio >= 0.f);
    ALVA_ARG(n_query == 0 || (d_qdesc && ((uintptr_t) d_qdesc % 16) == 0 && d_match));
    ALVA_ARG(n_rows == 0 || (d_rows && ((uintptr_t) d_rows % 16) == 0));
    const int nq_pad = alva_divup(n_query, RQ) * RQ, chunks = alva_divup(n_rows, RC);
    const size_t part_bytes = ((size_t) chunks * nq_pad * sizeof(Top2) + 255) / 256 * 256;
    const size_t cand_bytes = ((size_t) n_query * 8 + 255) / 256 * 256;
    uint8_t *scr = nullptr;
    int rc = alva_ctx_scratch(ctx, 0, part_bytes + cand_bytes + (size_t) n_rows * 8 + 256, (void **) &scr);
    if (rc) return rc;
    Top2 *partial = (Top2 *) scr;
    int *cand = (int *) (scr + part_bytes);
    unsigned long long *claim = (unsigned long long *) (scr + part_bytes + cand_bytes);
    const int live_chunks = n_query > 0 ? chunks : 0;
    if (live_chunks > 0) {
        hipLaunchKernelGGL(k_reloc_partial, dim3(nq_pad / RQ, chunks), dim3(RQ), 0, ctx->stream, (const uint4 *) d_qdesc, n_query, d_rows,
                           n_rows, partial, nq_pad, claim);
        ALVA_LAUNCH_CHECK();
    }
    if (n_query > 0) {
        hipLaunchKernelGGL(k_reloc_merge, dim3(alva_divup(n_query, 256)), dim3(256), 0, ctx->stream, (const Top2 *) partial, live_chunks, n_query, nq_pad,
                           d_qvalid, max_dist, ratio, cand, claim);
        ALVA_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_reloc_emit, dim3(1), dim3(EMIT_NT), 0, ctx->stream, (const int *) cand, n_query, (const unsigned long long *) claim, d_rows, d_qbv,
                       d_qunpx, d_match, d_count, d_bv, d_uv, d_wpt);
    ALVA_LAUNCH_CHECK();
    return ALVA_OK;
}
