// Device-side Hamming distance of two 256-bit descriptors (16-byte aligned), shared by match_to_map.hip and map_merge.hip, and the top-2
// scan of one query over a staged chunk of rows, shared by reloc.hip (map records) and image_detect.hip (a frame's descriptors).
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ int alva_hamming256_dev(const uint4 *a, const uint4 *b) {
    const uint4 a0 = a[0], a1 = a[1], b0 = b[0], b1 = b[1];
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) + __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) +
           __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// ---- top-2 of one query over rows: the best row under (distance, id) and the smallest distance over all other rows
constexpr int ALVA_TOP2_NO_DIST = 257;   // "no such row": one more than the largest distance of 256 bits

// a mergeable record: the best row of a set of rows under (distance, id), its row index, and the second-smallest distance in the set
struct AlvaTop2 {
    int d, id, row, second;
};

__device__ __forceinline__ void alva_top2_merge(int &bd, int &bid, int &brow, int &bs, int pd, int pid, int prow, int ps) {
    if (pd < bd || (pd == bd && pid < bid)) {
        bs = min(min(bs, ps), bd);
        bd = pd;
        bid = pid;
        brow = prow;
    } else {
        bs = min(bs, min(pd, ps));
    }
}

// the query (qa, qb) held in registers against the rcount rows staged in LDS (s_d: two uint4 per row, s_id: the row's tie-break id, < 0 =
// unused row), rows r0 .. r0 + rcount - 1 of the caller's numbering; the running record (bd, bid, brow, bs) is updated in place
__device__ __forceinline__ void alva_top2_scan(const uint4 qa, const uint4 qb, const uint4 *s_d, const int *s_id, int rcount, int r0, int &bd,
                                               int &bid, int &brow, int &bs) {
#pragma unroll 4
    for (int j = 0; j < rcount; j++) {
        const int id = s_id[j];
        if (id < 0) continue;   // (uniform: an unused row)
        const uint4 ta = s_d[2 * j], tb = s_d[2 * j + 1];
        int d = __popc(qa.x ^ ta.x);
        d += __popc(qa.y ^ ta.y);
        d += __popc(qa.z ^ ta.z);
        d += __popc(qa.w ^ ta.w);
        d += __popc(qb.x ^ tb.x);
        d += __popc(qb.y ^ tb.y);
        d += __popc(qb.z ^ tb.z);
        d += __popc(qb.w ^ tb.w);
        const bool better = d < bd || (d == bd && id < bid);
        bs = better ? bd : min(bs, d);
        bd = better ? d : bd;
        bid = better ? id : bid;
        brow = better ? r0 + j : brow;
    }
}
