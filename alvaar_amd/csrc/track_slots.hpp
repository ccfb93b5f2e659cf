// The tracking step of one frame, slot-wise (shared by klt.hip, which tracks, and stages_hip.hip, which drives it).
//
// VisualFrontend::kltTrackingFromMotionPrior (src/slam/src/visual_frontend.cpp:152-243) builds two keypoint lists -- 3-D keypoints
// whose projection under the predicted pose falls into the image (one pyramid level, from that projection) and everything else
// (full pyramid, from the keypoint's own position), the failures of the first list joining the second.  What fbKltTracking
// computes for a keypoint does not depend on the keypoint's position in a list, so no list is built here: one workgroup per SLOT
// of the frame container decides by itself which of the two it is, and re-tracks its keypoint on the full pyramid at once when the
// one-level pass fails -- from where that pass left it, which is what the reference does unless fewer than 33 % of the one-level
// passes succeeded (p3pReq_, :193-203: then the retry starts from the keypoint's own position).  That count is known only after the
// launch: the compaction kernel puts it into the header, and in that (rare) case the host launches the retry kernel, which redoes the
// retried slots from their own positions, and the compaction once more.  The compaction kernel gathers the correspondences of the
// pose solve in slot order (:275-298) and copies the per-slot results to pinned host memory ITSELF, behind its own system-scope
// fences and in front of the completion word the host polls.  (Results written to host memory by the tracker's workgroups -- an
// earlier kernel, on other XCDs -- are not ordered against that word: kernels of one stream are separated by agent-scope releases
// only.  With the tracker writing them the host read a stale value about once in 10^5 slots.)
#pragma once
#include "camera_device.hpp"
#include <cstdint>

#include <cstddef>

// The step's 1024-byte block of device counters (TrackSlots::cnt), zero between steps: the compaction's last workgroup resets it.
constexpr int TRK_STRIPES = 64;   // arrival stripes of the wave-per-slot tracker launch
struct TrackCounters {
    int pad0_[4];
    unsigned long long packed;   // the tracker launch's ONE packed counter: arrivals << 48 | tracked 3-D slots << 32 | slots tracked from
                                 // their projection << 16 | successes of those (one atomic per workgroup; counts fit 16 bits: a frame holds
                                 // < 65536 slots)
    int pad1_[2];
    int compact_arrivals;        // the compaction's workgroups
    int pad2_;
    int gathered_seq;            // the fused pose launch (GATHER_FIRST): seq once every slice's correspondences are gathered
    int gather_arrivals;         //                                       its compaction workgroups, arriving with their slice gathered
    int pad3_[20];
    unsigned long long stripes[TRK_STRIPES];   // the tracker's arrival stripes (klt.hip k_track_klt), summed into `packed`
    int pad4_[(1024 - 128 - 8 * TRK_STRIPES) / 4];
};
static_assert(offsetof(TrackCounters, packed) == 2 * 8 && offsetof(TrackCounters, compact_arrivals) == 8 * 4 &&
                  offsetof(TrackCounters, gathered_seq) == 10 * 4 && offsetof(TrackCounters, gather_arrivals) == 11 * 4 &&
                  offsetof(TrackCounters, stripes) == 16 * 8 && sizeof(TrackCounters) == 1024,
              "the counter block's layout");

// The step's two 8-byte words in pinned host memory, int offsets into TrackSlots::o_hdr, both [seq : 32 | p3pReq_ : 1 | n_pose : 31]:
//   TRK_HDR_EARLY  the tracker's counts, published by the LAST workgroup of the tracker launch itself -- the host learns the size of the
//                  pose problem one kernel earlier and enqueues the pose solve (sample draw + two launches) while the compaction runs
//   TRK_HDR_DONE   the compaction's completion word (system scope), after everything else: the host may poll it instead of waiting on
//                  the stream
constexpr int TRK_HDR_EARLY = 10, TRK_HDR_DONE = 12;
struct TrackWord {
    int seq, req, n_pose;
};
__host__ __device__ __forceinline__ unsigned long long track_word_pack(int seq, int req, int n_pose) {
    return ((unsigned long long) (unsigned) seq << 32) | ((unsigned long long) req << 31) | (unsigned) n_pose;
}
__host__ __device__ inline TrackWord track_word_unpack(unsigned long long w) {
    return TrackWord{(int) (w >> 32), (int) ((w >> 31) & 1), (int) (w & 0x7fffffffu)};
}
struct TrackSlots {
    int n, use_prior, width, height;
    const float *in_px;        // pinned host, [n][2]
    const uint8_t *in_is3d;    // pinned host, [n]
    const double *in_wpt;      // pinned host, [n][3]
    double q[4], t[3];         // T_cw (predicted)
    AlvaCam cam;
    const double *invK;        // device, 9
    TrackCounters *cnt;        // device, zeroed by the compaction kernel
    float *d_pts;              // [n][2] device copies of the three inputs (one coalesced pass over the bus; a workgroup per slot reading
                               // its 33 bytes from host memory by itself is bound by the number of outstanding PCIe reads)
    uint8_t *d_code;           // per slot: 0 lost | 1 tracked from the projection | 2 tracked on the full pyramid | 3 re-tracked
    uint8_t *d_retried;        // per slot: 1 = the one-level pass failed and the slot was re-tracked from where that pass left it
    uint8_t *d_is3d;           // copy of in_is3d
    float *d_px, *d_unpx;      // [n][2] tracked position | undistorted
    double *d_bv, *d_wpt;      // [n][3]; d_wpt = copy of in_wpt
    uint8_t *o_code;           // pinned host outputs
    float *o_px, *o_unpx;
    double *o_bv;
    int *o_hdr;                // TRK_HDR_EARLY / TRK_HDR_DONE
    int seq;                   // the step's sequence number, in both of o_hdr's words
    double *Pbv, *Puv, *Pwpt;  // device: correspondences of the pose solve
    unsigned long long *dbg;   // null, or the per-slot stamp buffer of ALVA_KLT_STAMPS=1 (microbench.hip)
    // The table CARRIED from the previous frame (round 6): a frame that only lost slots since the previous tracker launch -- every frame
    // between two keyframes -- is the previous frame's table without the lost rows, with the tracked positions as the new positions.  All
    // of that is on the device already: the host names, per slot, the slot it was (carry, 2 bytes per slot in host-written device memory
    // instead of 33 + the walk over the map points that fetched them), the tracker's workgroup reads its row through that index from the
    // previous frame's buffers (p_*) and writes it to this frame's (d_pts / d_is3d / d_wpt: what the retry launch, the compaction and the
    // next frame read).  The two frames' buffers alternate.  null: d_pts / d_is3d / d_wpt were written by the host (or k_track_stage_in).
    const uint16_t *carry;     // [n]
    const float *p_px;         // previous frame: d_px
    const uint8_t *p_is3d;     //                 d_is3d
    const double *p_wpt;       //                 d_wpt
};

struct alva_ctx;
struct alva_pyramid;
// enqueue only (klt.hip): the first launch over all slots, the retry launch
int alva_track_slots_klt(alva_ctx *ctx, const alva_pyramid *prev, const alva_pyramid *curr, const TrackSlots &D, int levels_prior, int levels_full,
                         float err_thresh, float fb_dist, int max_iters, float eps, int retry);
