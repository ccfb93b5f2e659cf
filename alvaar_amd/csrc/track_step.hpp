// The memory and the state of the fused tracking step (HipStages::track_begin, stages_hip.hip; the kernels' view of the same memory is
// TrackSlots, track_slots.hpp).  The step keeps three blocks, grown together when a frame outgrows them (track_reserve); each is described
// ONCE here, by the constructor that carves it: the field pointers and the block's size both come from that one walk.  The layouts are
// plain C++ -- a host-only test restates them for every capacity (tests/cpp/track_layout.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

struct TrackCounters;   // track_slots.hpp
constexpr size_t TRK_COUNTERS_BYTES = 1024, TRK_HDR_BYTES = 256;   // sizeof(TrackCounters) | o_hdr: the two completion words live in it

// Walks a block: typed pointers at running OFFSETS from the base.  Every base is 256-byte aligned (hipMalloc, hipHostMalloc and
// hipExtMallocWithFlags give that; track_reserve checks it once per allocation), so an offset's alignment is the pointer's.
struct TrackCarve {
    uintptr_t base;
    size_t off = 0;
    template <class T> T *take(size_t bytes) {
        T *p = reinterpret_cast<T *>(base + off);
        off += bytes;
        return p;
    }
    // on to the next multiple of a (a power of two) PAST off: a whole `a` when off is a multiple already
    void past(size_t a) { off += a - (off & (a - 1)); }
};
inline bool track_block_aligned(const void *base) { return ((uintptr_t) base & 255) == 0; }

// a slot table: positions [c][2] | 3-D flags [c] | world points [c][3]
struct TrackTable {
    float *px;
    uint8_t *is3d;
    double *wpt;
    TrackTable() = default;
    TrackTable(TrackCarve &k, size_t c, size_t flag_pad) {
        px = k.take<float>(c * 8);
        is3d = k.take<uint8_t>(c);
        k.past(flag_pad);
        wpt = k.take<double>(c * 24);
    }
};

// The DEVICE block: counters | code is3d | pts retried px unpx bv wpt | Pbv Puv Pwpt | the second px.  Capacities are multiples of 1024, so
// every array starts 16-byte aligned (k_track_stage_in copies in 16-byte units); pts and the second px start a 256-byte line of their own.
struct TrackDevBlock {
    TrackCounters *cnt;
    uint8_t *code, *is3d;      // (is3d, pts, wpt: the copy kernel's table; a host-written or carried table replaces them, TrackInBlock)
    float *pts;
    uint8_t *retried;
    float *px[2];              // the tracked positions of consecutive frames alternate (a carried table reads the previous frame's)
    float *unpx;
    double *bv, *wpt;
    double *Pbv, *Puv, *Pwpt;  // the gathered correspondences of the pose solve
    size_t end;
    TrackDevBlock(const void *base, size_t c) {
        TrackCarve k{(uintptr_t) base};
        cnt = k.take<TrackCounters>(TRK_COUNTERS_BYTES);
        code = k.take<uint8_t>(c);
        is3d = k.take<uint8_t>(c);
        k.past(256);
        pts = k.take<float>(c * 8);
        retried = k.take<uint8_t>(c);
        px[0] = k.take<float>(c * 8);
        unpx = k.take<float>(c * 8);
        bv = k.take<double>(c * 24);
        wpt = k.take<double>(c * 24);
        Pbv = k.take<double>(c * 24);
        Puv = k.take<double>(c * 16);
        Pwpt = k.take<double>(c * 24);
        k.past(256);
        px[1] = k.take<float>(c * 8);
        end = k.off;
    }
    static size_t bytes(size_t c) { return TrackDevBlock(nullptr, c).end; }
};

// The PINNED block: the slot table in (the map layer writes it there directly where there is no host-written device table; copied by
// k_track_stage_in) | the header with the two completion words | the per-slot results out, written by the kernels, read in place.
struct TrackPinBlock {
    TrackTable in;
    int *o_hdr;
    uint8_t *o_code;
    float *o_px, *o_unpx;
    double *o_bv;
    size_t end;
    TrackPinBlock(const void *base, size_t c) {
        TrackCarve k{(uintptr_t) base};
        in = TrackTable(k, c, 64);
        o_hdr = k.take<int>(TRK_HDR_BYTES);
        o_code = k.take<uint8_t>(c);
        k.past(64);
        o_px = k.take<float>(c * 8);
        o_unpx = k.take<float>(c * 8);
        o_bv = k.take<double>(c * 24);
        end = k.off;
    }
    static size_t bytes(size_t c) { return TrackPinBlock(nullptr, c).end + 256; }
};

// The HOST-WRITTEN block, device memory the host stores into over the bus: TWO tables -- a frame's table is either written by the host or
// built by the tracker from the previous frame's (the carried table, track_slots.hpp), so consecutive frames alternate between them -- and
// behind them the carry index the host writes instead (2 bytes per slot).
inline size_t track_in_bytes(size_t c) {
    TrackCarve k{0};
    (void) TrackTable(k, c, 256);
    return k.off;
}
struct TrackInBlock {
    TrackTable table[2];
    uint16_t *carry;
    size_t end;
    TrackInBlock(const void *base, size_t c) {
        TrackCarve k{(uintptr_t) base};
        table[0] = TrackTable(k, c, 256);
        table[1] = TrackTable(k, c, 256);
        carry = k.take<uint16_t>(c * 2);
        end = k.off;
    }
    static size_t bytes(size_t c) { return TrackInBlock(nullptr, c).end + 256; }
};

#ifdef __HIPCC__   // the step's state holds HIP-side types
#include "stage_arena.hpp"
#include "stages_hip.hpp"
#include "track_slots.hpp"

static_assert(sizeof(TrackCounters) == TRK_COUNTERS_BYTES, "the counter block");
static_assert(TRK_HDR_EARLY % 2 == 0 && TRK_HDR_DONE % 2 == 0 && TRK_HDR_EARLY != TRK_HDR_DONE &&
                  (size_t) (TRK_HDR_EARLY + 2) * 4 <= TRK_HDR_BYTES && (size_t) (TRK_HDR_DONE + 2) * 4 <= TRK_HDR_BYTES,
              "two 8-byte words inside o_hdr");

namespace alva_slam {

// how a step's slot table reached the device (the values HipStages::TrackStepInfo::route reports)
enum TrackRoute { TRACK_ROUTE_PINNED = 0, TRACK_ROUTE_DEVICE = 1, TRACK_ROUTE_CARRIED = 2 };
// the fused pose launch (k_pose_all) within one step: every queued launch must be answered by exactly one of go / abort
enum class PoseAll { not_queued, awaiting, go, aborted };

// Everything the fused tracking step keeps between calls.  Written by the session's own thread only, in the functions named.
struct TrackStepState {
    // -- the blocks: track_reserve allocates, grows and releases them; valid while cap > 0
    Arena dev, pin;             // TrackDevBlock, TrackPinBlock (pin.pinned is set by init)
    uint8_t *in = nullptr;      // TrackInBlock; null where there is no host-written device memory (then bar_table is false too)
    int cap = 0;                // slots all three are carved for: a multiple of 1024, only grows
    // -- switches: init (track_reserve clears bar_table when the allocation is refused)
    bool bar_table = true;      // the slot table in host-written device memory; ALVA_NO_BAR_TABLE=1: pinned table + k_track_stage_in
    bool carry_ok = true;       // ALVA_NO_CARRY=1: every frame's table assembled by the host (A/B)
    // -- the alternation of tables and px buffers: track_begin, once the step's tail is queued, on the device routes only
    int par = 0;                // the table (and px buffer) of the LAST tracker launch; the next one takes the other
    int valid_n = -1;           // slots of that launch if its table + tracked positions are complete on the device (a carried table may
                                // follow), else -1: track_begin clears it on entry, track_reserve when the blocks move
    int seq = 0;                // the last sequence number given out: track_begin per tracker launch, and again for a retry's compaction
    // -- the pose solve behind the step: track_begin sets, track_pose_collect consumes
    bool fused_active = false;  // the last track_begin took the fused path: track_pose_collect answers for it (else the composed default)
    bool pose_pending = false;  // a pose solve is enqueued and not collected yet
    int pose_n = 0;             // its correspondences (clamped to ALVA_P3P_MAX_N), 0 without a solve
    int pose_total = 0;         // the step's n_pose: the length of the outlier masks track_pose_collect returns
    // -- what the last fused track_begin did and where it gathered the pose correspondences (the test-only step probe reads them):
    //    written on the host, beside the launches they describe; rows are cleared when the blocks move
    HipStages::TrackStepInfo info{};
    const double *rows[3] = {nullptr, nullptr, nullptr};

    TrackDevBlock dev_block() const { return TrackDevBlock(dev.base, (size_t) cap); }
    TrackPinBlock pin_block() const { return TrackPinBlock(pin.base, (size_t) cap); }
    TrackInBlock in_block() const { return TrackInBlock(in, (size_t) cap); }
};

}  // namespace alva_slam
#endif
