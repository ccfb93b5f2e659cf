// The numeric stages of the map layer (slam/stages.hpp) on the GPU: every method is one or more calls through
// include/alvaar_hip.h on this object's HIP stream.  This is the only `Stages` implementation in libalvaar_hip.so; there is no
// CPU path -- creation fails when no HIP device is present.
//
// Host arrays cross into device memory through two bump arenas that are reset per call (stage_arena.hpp).  One stream
// synchronisation per method.  The scene features (hit test, depth, light, pictures, planes, anchors) are no stages of the map layer:
// they live in scene_stages.hip and see this object through HipStages::frame and HipStages::carve.
#include "common.hpp"
#include "stage_arena.hpp"
#include "multi_kernel.hpp"
#include <algorithm>
#include "camera_device.hpp"
#include "pose_internal.hpp"
#include "track_slots.hpp"
#include "stages_hip.hpp"
#include "track_step.hpp"
#include <cmath>
#include <cstdlib>

namespace alva_slam {

namespace {

// Frame::computeKeypoint's second half (frame.cpp:109-112)
__global__ void __launch_bounds__(256) k_bearing(const float *unpx, int n, const double *invK, double *bv) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    alva_bearing_dev(invK, unpx[2 * i], unpx[2 * i + 1], bv + 3 * (size_t) i);
}

// ---- the fused tracking step: the compaction behind the slot-wise tracker (track_slots.hpp) ----------------------------------------
#include "track_compact_device.hpp"
__global__ void __launch_bounds__(CMP_NT) k_track_compact(TrackSlots D) { (void) track_compact_body<CMP_NT>(D, (int) blockIdx.x, (int) gridDim.x); }
ALVA_MULTI_KERNEL(MK_TRACK_COMPACT, k_track_compact_multi, TrackSlots, dim3(CMP_NT), CMP_NT, (void) track_compact_body<CMP_NT>(A, bx, (int) gx));

}  // namespace

struct HipStages::Impl {
    int device = 0;
    alva_medoid_store *med = nullptr;   // the map points' descriptor tables (medoid.hip), created with the first replay
    alva_ctx *ctx = nullptr;
    hipStream_t st = nullptr;
    Camera cam;
    bool clahe = false;
    // Three pyramids / two gray images in rotation: the current frame's, the previous frame's (the tracker reads both) and the one a
    // look-ahead build may be filling for the next frame (hint_next_frame_device).  d_gray always names the CURRENT frame's image.
    alva_pyramid *pyr[3] = {nullptr, nullptr, nullptr};
    int cur = 0, prev = 1, nxt = 2;
    uint8_t *d_rgba = nullptr, *d_gray = nullptr, *d_gray_next = nullptr, *d_eq = nullptr, *h_rgba = nullptr;
    // look-ahead: the hinted source, whether its build has been enqueued (same stream, behind the pose kernels)
    const uint8_t *ahead_src = nullptr;
    bool ahead_enqueued = false;
    double *d_invK = nullptr;
    const uint8_t *registered = nullptr, *registered_dev = nullptr;  // caller buffer locked + mapped by register_frame_buffer
    size_t registered_bytes = 0;
    uint8_t *bar_frame = nullptr;   // alloc_frame_buffer: the caller's frame buffer in device memory, written by the host over the BAR
    size_t bar_frame_bytes = 0;
    bool upload_in_flight = false;
    hipEvent_t upload_done = nullptr;
    double max_quality = 0.001;  // state.hpp:57; lives as long as the reference's FeatureExtractor object (system.cpp:31)
    Arena dev, pin;
    // the map layer's record arena (slam/mp_rec.hpp): chunks of pinned host memory + the device-resident table of their addresses
    std::vector<MpRec *> rec_chunks;
    const MpRec **d_rec_tab = nullptr;
    // relocalize: the map's record block (alva_pack_map_records layout), packed once per LOST episode
    uint8_t *reloc_rows = nullptr;
    int reloc_cap = 0, reloc_n_rows = 0;
    // the device-visible source of the current frame's images (what build_from was given: the staging copy, the caller's frame buffer in
    // device memory, its registered buffer or its device frame)
    const uint8_t *frame_src = nullptr;
    static constexpr int REC_TAB_CAP = 4096;   // 16.7 M map points
    // the fused tracking step: its persistent blocks (grown when the keypoint count outgrows them) and what it keeps between calls
    TrackStepState trk;
    bool fused = true;       // ALVA_TRACK_UNFUSED=1: compose the tracking step from the fine-grained stages instead (A/B testing)
    bool poll = true;        // wait for the tracking step by polling its completion word in pinned memory (ALVA_NO_POLL=1: stream synchronisation)
    SessionPose pose() const { return SessionPose(cam.fx, cam.fy, cam.cx, cam.cy); }
    // Device memory that the HOST is going to write over the BAR must not have a previous life left in an L2: the allocator recycles
    // pages, and a line that an earlier owner's kernel wrote may still sit DIRTY in an L2 (device-local memory is only written back when
    // the line is evicted) -- evicted later, it would overwrite what the host stored in the meantime (seen as a tracker reading last
    // frame's slot table, once in a few hundred session starts).  One device-wide synchronisation behind a fill: its system-scope
    // release writes every dirty line back; nothing on the device writes the block afterwards.
    // FINE-GRAINED device memory (coherent with the host by definition; the device does not keep its lines in an L2 across kernels).
    // hipDeviceMallocUncached looked equivalent and is not: with BOTH the slot table and the caller's frame buffer allocated that way,
    // test_group_sessions_equal_their_solo_runs[one_lane] failed in 8 of 13 runs of tests/test_gpu_system.py (a session's second tracking
    // frame tracked from its first frame's table); either one alone, or the table fine-grained, never did (3 / 3, 3 / 3, and every run
    // since).  What the HIP memory model
    // promises: fine-grained allocations are coherent between host and device at system scope WHILE kernels run; "uncached" only selects
    // a cache policy for the device's own accesses and promises nothing about host stores that arrive over the BAR -- so the shipped flag
    // is the documented one, and the failing one was never covered by a rule.  tests/test_gpu_bar_buffers.py starts 32 sessions (and 30
    // one-lane groups) back to back under the shipped flag and compares every one with the first, bit for bit.
    static constexpr unsigned bar_alloc_flag = hipDeviceMallocFinegrained;
    // Host stores into device memory need the whole of it mapped into the CPU's address space (a "large" / resizable BAR).  On a small-BAR
    // host -- many passthrough VMs -- hipExtMallocWithFlags still succeeds, the pointer is simply not CPU-mapped and the first host store
    // faults: ask the driver instead of finding out (both paths then fall back: pinned slot table + copy kernel, registered frame buffer).
    static bool host_can_store_to_device_memory(int device) {
        int large = 0;
        if (hipDeviceGetAttribute(&large, hipDeviceAttributeIsLargeBar, device) != hipSuccess) {
            (void) hipGetLastError();
            return false;
        }
        return large != 0;
    }
    static hipError_t scrub_host_written(void *p, size_t bytes) {
        hipError_t e = hipMemset(p, 0, bytes);
        if (e != hipSuccess) return e;
        return hipDeviceSynchronize();
    }
    // the step's three blocks (track_step.hpp) for n slots; a multiple of 1024 slots with at least 1024 to spare
    int track_reserve(int n) {
        TrackStepState &T = trk;
        if (n <= T.cap) return ALVA_OK;
        const int cap = ((n + 1023) / 1024 + 1) * 1024;
        const size_t c = (size_t) cap;
        int rc = T.dev.grow(TrackDevBlock::bytes(c), st);
        if (rc) return rc;
        rc = T.pin.grow(TrackPinBlock::bytes(c), st);
        if (rc) return rc;
        // the slot table (positions | 3-D flags | world points) in DEVICE memory that the host writes directly: the whole of the device's
        // memory is visible to the CPU (large BAR; tools/probes/bar_probe.cpp: 128 KB of ordinary stores in 2.6 us, write-combined and
        // posted), so the map layer assembles the table where the tracker reads it and the copy kernel of rounds 2 - 4 (k_track_stage_in:
        // 7 us + a launch gap in front of every frame's tracker) is gone.  Fine-grained memory (bar_alloc_flag): an L2 must not answer with
        // last frame's line.  The host never READS this memory (a load over the bus costs ~1 us).
        T.valid_n = -1;   // no complete table is left: the buffers move
        T.rows[0] = T.rows[1] = T.rows[2] = nullptr;
        if (T.in) {
            ALVA_HIP(alva_stream_sync(st));
            ALVA_HIP(hipFree(T.in));
            T.in = nullptr;
        }
        if (T.bar_table) {
            const size_t in_bytes = TrackInBlock::bytes(c);
            if (hipExtMallocWithFlags((void **) &T.in, in_bytes, bar_alloc_flag) != hipSuccess) {
                (void) hipGetLastError();
                T.in = nullptr;
                T.bar_table = false;   // no such memory here: the pinned table + the copy kernel
            } else {
                ALVA_HIP(scrub_host_written(T.in, in_bytes));
            }
        }
        if (!track_block_aligned(T.dev.base) || !track_block_aligned(T.pin.base) || !track_block_aligned(T.in)) {
            alva_set_error("tracking step: a block's base is not 256-byte aligned (the layouts of track_step.hpp count on it)");
            return ALVA_ERR_STATE;
        }
        T.cap = cap;
        ALVA_HIP(hipMemsetAsync(T.dev.base, 0, sizeof(TrackCounters), st));  // the slot-wise step's counters start at zero
        // fresh (or recycled) pinned memory: the completion word must not equal a sequence number the host is about to wait for.  The
        // stream is idle here (both grows synchronised it), so a plain host store cannot race a kernel's publication.
        ALVA_HIP(alva_stream_sync(st));
        memset(T.pin_block().o_hdr + TRK_HDR_EARLY, 0, 8);
        memset(T.pin_block().o_hdr + TRK_HDR_DONE, 0, 8);
        return ALVA_OK;
    }

    // ---- one fused step, in the order track_begin calls them ---------------------------------------------------------------------
    // what the helpers hand to one another
    struct Step {
        const TrackJob &job;
        TrackRoute route = TRACK_ROUTE_PINNED;
        TrackSlots D{};
        PoseAll pose_all = PoseAll::not_queued;
        bool pose_early = false;   // the pose solve went out on the tracker's early word
        int early_n_pose = -1;     // that word's count
        TrackWord word{};          // the step's header, out of its last completion word
        int p3p_req = 0;           // the first completion word asked for the retry
    };

    // The composed path (ALVA_TRACK_UNFUSED=1, or a pose wanted with p3pEnabled_ off): the fine-grained stages, no table left behind.
    int track_composed(HipStages &hs, const TrackJob &job, TrackKlt &out) {
        trk.valid_n = -1;
        if (job.carry) {
            alva_set_error("tracking step: a carried slot table on the composed path");
            return ALVA_ERR_STATE;
        }
        if (trk.in && job.n > 0 && job.px == trk.in_block().table[trk.par ^ 1].px) {
            // the composed step READS the slot table on the host, and this one was written into device memory (track_slot_buffers): one
            // copy back instead of a load over the bus per element (p3pEnabled_ off: not the shipped configuration)
            static thread_local std::vector<uint8_t> back;
            const size_t n = (size_t) job.n;
            back.resize(n * 40);
            ALVA_HIP(hipSetDevice(device));
            __builtin_ia32_sfence();
            ALVA_HIP(hipMemcpy(back.data(), job.px, n * 8, hipMemcpyDeviceToHost));
            ALVA_HIP(hipMemcpy(back.data() + n * 8, job.wpt, n * 24, hipMemcpyDeviceToHost));
            ALVA_HIP(hipMemcpy(back.data() + n * 32, job.is3d, n, hipMemcpyDeviceToHost));
            TrackJob j2 = job;
            j2.px = (const float *) back.data();
            j2.wpt = (const double *) (back.data() + n * 8);
            j2.is3d = back.data() + n * 32;
            return hs.Stages::track_begin(j2, out);
        }
        return hs.Stages::track_begin(job, out);
    }

    // How the job's slot table reaches the device, from its pointers: carried from the previous frame's n_prev slots (track_carry_buffer
    // said yes and the map layer filled the index: nothing to read on the host), written into this frame's device table (track_slot_buffers
    // handed it out: it is written, never read here), or anything else, through the pinned table and the copy kernel.
    int track_route(const TrackJob &job, int n_prev, int par, TrackRoute *route) const {
        const bool have_in = trk.bar_table && trk.in;
        const TrackInBlock in = trk.in_block();
        if (job.carry) {
            if (!(have_in && job.carry == in.carry && n_prev >= job.n && !g_alva_lane)) {
                alva_set_error("tracking step: a carried slot table without a previous frame's table to carry it from");
                return ALVA_ERR_STATE;
            }
            *route = TRACK_ROUTE_CARRIED;
            return ALVA_OK;
        }
        const TrackTable &t = in.table[par];
        *route = have_in && job.px == t.px && job.is3d == t.is3d && job.wpt == t.wpt ? TRACK_ROUTE_DEVICE : TRACK_ROUTE_PINNED;
        return ALVA_OK;
    }

    // The kernels' view of the step (TrackSlots) from the layouts, the route and the job; the step's sequence number; the probe's account.
    void track_fill_slots(Step &s, int par) {
        const TrackJob &job = s.job;
        const TrackDevBlock dev = trk.dev_block();
        const TrackPinBlock pin = trk.pin_block();
        TrackSlots &D = s.D;
        D.cnt = dev.cnt;
        D.d_code = dev.code; D.d_retried = dev.retried;
        D.d_px = dev.px[par]; D.d_unpx = dev.unpx; D.d_bv = dev.bv;
        D.Pbv = dev.Pbv; D.Puv = dev.Puv; D.Pwpt = dev.Pwpt;
        if (s.route == TRACK_ROUTE_PINNED) {
            D.in_px = pin.in.px; D.in_is3d = pin.in.is3d; D.in_wpt = pin.in.wpt;
            D.d_pts = dev.pts; D.d_is3d = dev.is3d; D.d_wpt = dev.wpt;
        } else {   // the table is where the tracker reads it: no copy kernel (in_px == nullptr tells alva_track_slots_klt)
            const TrackInBlock in = trk.in_block();
            D.d_pts = in.table[par].px; D.d_is3d = in.table[par].is3d; D.d_wpt = in.table[par].wpt;
            if (s.route == TRACK_ROUTE_CARRIED) {   // ... built by the tracker from the previous frame's table and tracked positions
                D.carry = in.carry;
                D.p_px = dev.px[par ^ 1];
                D.p_is3d = in.table[par ^ 1].is3d;
                D.p_wpt = in.table[par ^ 1].wpt;
            }
        }
        D.o_hdr = pin.o_hdr; D.o_code = pin.o_code; D.o_px = pin.o_px; D.o_unpx = pin.o_unpx; D.o_bv = pin.o_bv;
        D.n = job.n;
        D.use_prior = job.use_prior;
        D.width = cam.width;
        D.height = cam.height;
        memcpy(D.q, job.Tcw_q, 32);
        memcpy(D.t, job.Tcw_t, 24);
        static_assert(sizeof(AlvaCam) == sizeof(std::array<double, 8>), "AlvaCam is the eight values of a calib8, in its order");
        memcpy(&D.cam, camera_calib8(cam).data(), sizeof(D.cam));
        D.invK = d_invK;
        D.dbg = alva_klt_stamp_buffer();
        D.seq = ++trk.seq;   // the tracker launch publishes its counts under this number too (TRK_HDR_EARLY)
        trk.info.route = s.route;
        trk.info.stage_in = D.in_px != nullptr;
        trk.info.seq = D.seq;
        trk.rows[0] = D.Pbv; trk.rows[1] = D.Puv; trk.rows[2] = D.Pwpt;
    }

    // the tracker over all slots (retry = 0) | over the retried slots again, from their own positions (retry = 1)
    int track_launch(const Step &s, int retry) {
        // state.hpp:50-56 constants; the prior pass works on one pyramid level (visual_frontend.cpp:166)
        return alva_track_slots_klt(ctx, pyr[prev], pyr[cur], s.D, 1, s.job.klt_levels, 30.f, 0.5f, 30, 0.01f, retry);
    }

    // The frame's tail -- compaction -> P3P-LMedS -> refinement -- as ONE launch queued right here, behind the tracker (pnp.hip
    // k_pose_all): its first workgroups are the compaction, the others wait for the host's word, which goes out (track_answer_early) as
    // soon as the tracker's early word has told the host how many correspondences there are.  A session of its own, polling, that wants
    // a pose; everything else keeps the compaction kernel.
    int track_queue_tail(Step &s) {
        const TrackSlots &D = s.D;
        if (poll && s.job.want_pose && s.job.do_p3p && alva_pose_all_possible(D.n, SessionPose::p3p_iters)) {
            const int rc = pose().enqueue_fused(ctx, D, s.job.do_random);
            if (rc) return rc;
            s.pose_all = PoseAll::awaiting;
            trk.info.pose_all_queued = 1;
        } else if (!alva_lane_defer(MK_TRACK_COMPACT, ctx, (unsigned) track_compact_grid(D.n), 0, &D, sizeof(D))) {
            hipLaunchKernelGGL(k_track_compact, dim3(track_compact_grid(D.n)), dim3(CMP_NT), 0, st, D);
            ALVA_LAUNCH_CHECK();
            trk.info.compact_launches++;
        }
        return ALVA_OK;
    }

    // The tracker launch's last workgroup has published the step's counts one kernel EARLIER (TRK_HDR_EARLY, track_slots.hpp): in the
    // normal case (no p3pReq_) the pose solve goes out NOW -- the queued k_pose_all gets its go, or host-side sample draw + two launches
    // are queued behind the compaction kernel in stream order -- instead of after the compaction's completion word: the GPU goes from the
    // compaction straight into P3P.
    int track_answer_early(HipStages &hs, Step &s) {
        if (!poll || !s.job.want_pose) return ALVA_OK;
        const volatile unsigned long long *early_word = reinterpret_cast<const volatile unsigned long long *>(s.D.o_hdr + TRK_HDR_EARLY);
        // (no stream wait behind the polls: a queued k_pose_all behind the tracker waits for this host's answer)
        TrackWord early{};
        const bool seen = alva_poll_until([&] { return (early = track_word_unpack(*early_word)).seq == s.D.seq; });
        s.early_n_pose = early.n_pose;
        if (!seen || early.req || early.n_pose < 4) {
            if (s.pose_all == PoseAll::awaiting) {
                (void) alva_pose_all_abort(ctx);   // p3pReq_, fewer than four correspondences, or no word at all: the queued launch ends after its compaction
                s.pose_all = PoseAll::aborted;
                trk.info.pose_all_answer = 2;
            }
            return ALVA_OK;
        }
        trk.pose_n = early.n_pose > ALVA_P3P_MAX_N ? ALVA_P3P_MAX_N : early.n_pose;   // (the first ones, in slot order)
        int rc;
        if (s.pose_all == PoseAll::awaiting) {
            trk.info.pose_all_answer = 1;
            rc = alva_pose_all_go(ctx, trk.pose_n);   // the queued launch's second phase: samples for this n, go
            s.pose_all = PoseAll::go;
        } else {
            rc = pose().enqueue(ctx, s.D.Pbv, s.D.Puv, s.D.Pwpt, trk.pose_n, s.job.do_random);
        }
        if (rc) return rc;
        s.pose_early = true;
        rc = hs.build_ahead();   // a hinted next frame: its images are queued behind the pose kernels
        if (rc) return rc;
        alva_lane_yield();       // in a group: the thread's other sessions deposit their pose solves before this one starts its bookkeeping
        return ALVA_OK;
    }

    // the step's header, out of the completion word published under D.seq
    int track_wait(Step &s) {
        const volatile unsigned long long *done_word = reinterpret_cast<const volatile unsigned long long *>(s.D.o_hdr + TRK_HDR_DONE);
        if (poll) {
            // the compaction kernel publishes [seq | p3pReq_ | n_pose] as one word after all results; spinning on it in pinned memory
            // returns a few microseconds before hipStreamSynchronize would
            if (!alva_wait_until([&] { return (s.word = track_word_unpack(*done_word)).seq == s.D.seq; }, st)) {
                alva_set_error("tracking step %d: the compaction never published its completion word", s.D.seq);
                return ALVA_ERR_STATE;
            }
        } else {
            ALVA_HIP(alva_stream_sync(st));
            s.word = track_word_unpack(*done_word);
        }
        return ALVA_OK;
    }

    // p3pReq_: fewer than 33 % of the one-level passes held (visual_frontend.cpp:193-203): the retries must start from the keypoints' own
    // positions instead -- redo them and compact again (rare: tracking is about to be lost)
    int track_retry(Step &s) {
        s.p3p_req = 1;
        int rc = track_launch(s, 1);
        if (rc) return rc;
        s.D.seq = ++trk.seq;   // the retry publishes under a new number, and the probe's account follows it
        hipLaunchKernelGGL(k_track_compact, dim3(track_compact_grid(s.D.n)), dim3(CMP_NT), 0, st, s.D);
        ALVA_LAUNCH_CHECK();
        trk.info.retry = 1;
        trk.info.compact_launches++;
        trk.info.seq = s.D.seq;
        return track_wait(s);
    }

    // the tracker's results to the caller; the pose solve's bookkeeping for track_pose_collect
    int track_publish(const Step &s, TrackKlt &out) {
        out.code_v = s.D.o_code;   // read in place (pinned host memory, written by the kernels; stays until the next track_begin)
        out.px_v = s.D.o_px;
        out.unpx_v = s.D.o_unpx;
        out.bv_v = s.D.o_bv;
        out.p3p_req = s.p3p_req;
        out.n_pose = s.word.n_pose;
        if (s.pose_early) {
            if (s.p3p_req || out.n_pose != s.early_n_pose) {   // cannot happen: both kernels count the same flags
                alva_set_error("tracking step: the tracker's early counts (%d) disagree with the compaction (%d)", s.early_n_pose, out.n_pose);
                return ALVA_ERR_STATE;
            }
            trk.pose_pending = true;
        } else if (s.job.want_pose && out.n_pose >= 4) {   // the solve did not go out on the early word (stream waits, p3pReq_, no word seen)
            trk.pose_n = out.n_pose > ALVA_P3P_MAX_N ? ALVA_P3P_MAX_N : out.n_pose;
            const int rc = pose().enqueue(ctx, s.D.Pbv, s.D.Puv, s.D.Pwpt, trk.pose_n, s.job.do_random);
            if (rc) return rc;
            trk.pose_pending = true;
        }
        trk.pose_n = out.n_pose >= 4 ? trk.pose_n : 0;
        trk.pose_total = out.n_pose;
        trk.fused_active = true;
        if (!trk.pose_pending) alva_lane_clean();   // in a group: the compaction's word was the chain's last (lane.hpp); with a pose solve, its own is
        return ALVA_OK;
    }

    alva_detect_pending det_pending{};   // detect_begin -> detect_end
    int dsc_n = 0;                       // describe_begin -> describe_end: count, where the results will be (pinned staging)
    const uint8_t *dsc_desc = nullptr, *dsc_valid = nullptr;
    const uint8_t *det_h = nullptr;
    int det_cap = 0;
    // a call plans its buffers first (StagePlan), then the arenas are grown once and carved
    int carve(StagePlan &p, std::vector<uint8_t *> &d, std::vector<uint8_t *> &h) {
        size_t total = 0;
        for (size_t s: p.sizes) total += s;
        int rc = dev.grow(total, st);
        if (rc) return rc;
        rc = pin.grow(total, st);
        if (rc) return rc;
        d.resize(p.sizes.size());
        h.resize(p.sizes.size());
        size_t off = 0;
        for (size_t i = 0; i < p.sizes.size(); i++) {
            d[i] = dev.base + off;
            h[i] = pin.base + off;
            off += p.sizes[i];
        }
        return ALVA_OK;
    }
    // planned buffers i0 .. i1 (consecutive in both arenas, same offsets) with ONE copy command instead of one per buffer: a copy
    // command costs ~5 us of host time and ~5-10 us of queue latency, and the small keyframe stages issued 4 - 10 of them each
    int up_span(const StagePlan &p, const std::vector<uint8_t *> &d, const std::vector<uint8_t *> &h, size_t i0, size_t i1) {
        ALVA_HIP(hipMemcpyAsync(d[i0], h[i0], (size_t) (h[i1] - h[i0]) + p.sizes[i1], hipMemcpyHostToDevice, st));
        return ALVA_OK;
    }
    int down_span(const StagePlan &p, const std::vector<uint8_t *> &d, const std::vector<uint8_t *> &h, size_t i0, size_t i1) {
        ALVA_HIP(hipMemcpyAsync(h[i0], d[i0], (size_t) (h[i1] - h[i0]) + p.sizes[i1], hipMemcpyDeviceToHost, st));
        return ALVA_OK;
    }
};

HipStages::HipStages() : m(new Impl()) {}

HipStages::~HipStages() {
    if (!m) return;
    (void) hipSetDevice(m->device);
    if (m->ctx) (void) alva_ctx_sync(m->ctx);
    for (auto &p: m->pyr) alva_pyramid_destroy(p);
    void *bufs[] = {m->d_rgba, m->d_gray, m->d_gray_next, m->d_eq, m->d_invK};
    for (void *b: bufs)
        if (b) (void) hipFree(b);
    if (m->h_rgba) (void) hipHostFree(m->h_rgba);
    if (m->registered) (void) hipHostUnregister((void *) m->registered);
    if (m->upload_done) (void) hipEventDestroy(m->upload_done);
    m->dev.release();
    m->pin.release();
    m->trk.dev.release();
    m->trk.pin.release();
    if (m->trk.in) (void) hipFree(m->trk.in);
    if (m->bar_frame) (void) hipFree(m->bar_frame);
    alva_medoid_store_destroy(m->med);
    for (MpRec *c: m->rec_chunks) (void) hipHostFree(c);
    if (m->d_rec_tab) (void) hipFree(m->d_rec_tab);
    if (m->reloc_rows) (void) hipFree(m->reloc_rows);
    alva_ctx_destroy(m->ctx);
    delete m;
}

int HipStages::init(int device, const Camera &cam, bool clahe, const double *invK, void *hip_stream) {
    m->device = device;
    m->cam = cam;
    m->clahe = clahe;
    m->pin.pinned = true;
    m->trk.pin.pinned = true;
    m->fused = getenv("ALVA_TRACK_UNFUSED") == nullptr;
    m->poll = alva_poll_enabled();
    // the slot table in host-written device memory (track_reserve): ALVA_NO_BAR_TABLE=1 keeps the pinned table + k_track_stage_in (A/B)
    m->trk.bar_table = getenv("ALVA_NO_BAR_TABLE") == nullptr && Impl::host_can_store_to_device_memory(m->device);
    m->trk.carry_ok = getenv("ALVA_NO_CARRY") == nullptr;
    int rc = hip_stream ? alva_ctx_create(device, hip_stream, 0, &m->ctx) : alva_ctx_create(device, nullptr, 1, &m->ctx);
    if (rc) return rc;
    m->st = (hipStream_t) alva_ctx_stream(m->ctx);
    const size_t P = (size_t) cam.width * cam.height;
    ALVA_HIP(hipMalloc((void **) &m->d_rgba, P * 4));
    ALVA_HIP(hipMalloc((void **) &m->d_gray, P));
    ALVA_HIP(hipMalloc((void **) &m->d_gray_next, P));
    if (clahe) ALVA_HIP(hipMalloc((void **) &m->d_eq, P));
    ALVA_HIP(hipMalloc((void **) &m->d_invK, 9 * sizeof(double)));
    ALVA_HIP(hipMemcpy(m->d_invK, invK, 9 * sizeof(double), hipMemcpyHostToDevice));
    ALVA_HIP(hipHostMalloc((void **) &m->h_rgba, P * 4, hipHostMallocDefault));
    ALVA_HIP(hipEventCreateWithFlags(&m->upload_done, hipEventDisableTiming));
    for (auto &p: m->pyr) {
        rc = alva_pyramid_create(m->ctx, cam.width, cam.height, 9, 3, &p);  // state.hpp:51-53: 9 x 9 window, 3 levels
        if (rc) return rc;
    }
    return ALVA_OK;
}

int HipStages::warm_up(int cell) {
    const Camera &k = m->cam;
    const int W = k.width, H = k.height;
    uint32_t lcg = 12345u;
    auto rnd = [&]() {
        lcg = lcg * 1664525u + 1013904223u;
        return (float) (lcg >> 8) * (1.f / 16777216.f);
    };
    int rc;
    // two frames: gray + pyramid (+ CLAHE)
    {
        std::vector<uint8_t> img((size_t) W * H * 4);
        for (size_t i = 0; i < img.size(); i += 4) {  // a smooth pattern with some texture: trackable, detectable
            const size_t p = i / 4, x = p % (size_t) W, y = p / (size_t) W;
            const uint8_t v = (uint8_t) (128 + 60 * std::sin(0.13 * (double) x) * std::cos(0.11 * (double) y) + 30 * ((x / 7 + y / 5) & 1));
            img[i] = img[i + 1] = img[i + 2] = v;
            img[i + 3] = 255;
        }
        for (int f = 0; f < 2; f++) {
            rc = new_frame(img.data());
            if (rc) return rc;
            rc = frame_done();
            if (rc) return rc;
        }
        ALVA_HIP(alva_stream_sync(m->st));
    }
    const int cw = (W + cell - 1) / cell, chh = (H + cell - 1) / cell, n = cw * chh;
    // the tracking step (stage-in, tracker, retry, compaction) and the pose solve behind it
    {
        float *px;
        uint8_t *is3d;
        double *wpt;
        std::vector<float> vpx;
        std::vector<uint8_t> v3;
        std::vector<double> vw;
        if (!track_slot_buffers(n + n / 4, &px, &is3d, &wpt)) {
            vpx.resize((size_t) (n + n / 4) * 2); v3.resize((size_t) (n + n / 4)); vw.resize((size_t) (n + n / 4) * 3);
            px = vpx.data(); is3d = v3.data(); wpt = vw.data();
        }
        for (int i = 0; i < n; i++) {
            const float x = 12.f + rnd() * (float) (W - 24), y = 12.f + rnd() * (float) (H - 24);
            px[2 * i] = x; px[2 * i + 1] = y;
            is3d[i] = (i % 8) != 0;
            const double z = 3.0 + 2.0 * rnd();
            wpt[3 * i] = ((double) x - k.cx) / k.fx * z; wpt[3 * i + 1] = ((double) y - k.cy) / k.fy * z; wpt[3 * i + 2] = z;
        }
        TrackJob job;
        job.n = n;
        job.px = px; job.is3d = is3d; job.wpt = wpt;
        job.want_pose = 1;
        job.do_random = 0;
        TrackKlt kl;
        TrackPose po;
        rc = track_begin(job, kl);
        if (!rc) rc = track_pose_collect(po);
        if (rc) return rc;
    }
    // keyframe stages
    {
        std::vector<float> pts((size_t) n * 2), un((size_t) n * 2), np((size_t) (n + 8) * 2);
        std::vector<double> bv((size_t) n * 3);
        std::vector<uint8_t> desc((size_t) n * 32), valid((size_t) n);
        for (int i = 0; i < n; i++) {
            pts[2 * (size_t) i] = 40.f + rnd() * (float) (W - 80);
            pts[2 * (size_t) i + 1] = 40.f + rnd() * (float) (H - 80);
        }
        rc = describe(n, pts.data(), desc.data(), valid.data());
        if (!rc) rc = compute_keypoints(n, pts.data(), un.data(), bv.data());
        if (rc) return rc;
        const double q = m->max_quality;
        int count = 0;
        rc = detect(cell, n / 2, pts.data(), n + 8, np.data(), &count);
        m->max_quality = q;
        if (rc) return rc;
    }
    {   // triangulation
        const int nt = n / 4 + 8;
        std::vector<double> T(36, 0.), bl((size_t) nt * 3), br((size_t) nt * 3), w((size_t) nt * 3), inv((size_t) nt), par((size_t) nt);
        std::vector<float> ul((size_t) nt * 2), ur((size_t) nt * 2);
        std::vector<int> grp((size_t) nt, 0);
        std::vector<uint8_t> st((size_t) nt);
        for (int b = 0; b < 3; b++) {   // R = I, t = (0.3, 0, 0) / its inverse / the keyframe's pose
            T[12 * b] = T[12 * b + 4] = T[12 * b + 8] = 1.;
        }
        T[9] = 0.3; T[21] = -0.3;
        for (int i = 0; i < nt; i++) {
            const double x = -0.3 + 0.6 * rnd(), y = -0.2 + 0.4 * rnd(), z = 4.;
            const double l[3] = {x, y, z}, r[3] = {x - 0.3, y, z};
            const double nl = std::sqrt(l[0] * l[0] + l[1] * l[1] + l[2] * l[2]), nr = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
            for (int c = 0; c < 3; c++) {
                bl[3 * (size_t) i + c] = l[c] / nl;
                br[3 * (size_t) i + c] = r[c] / nr;
            }
            ul[2 * (size_t) i] = (float) (k.fx * l[0] / z + k.cx); ul[2 * (size_t) i + 1] = (float) (k.fy * l[1] / z + k.cy);
            ur[2 * (size_t) i] = (float) (k.fx * r[0] / z + k.cx); ur[2 * (size_t) i + 1] = (float) (k.fy * r[1] / z + k.cy);
        }
        rc = triangulate(nt, 1, T.data(), grp.data(), bl.data(), br.data(), ul.data(), ur.data(), w.data(), inv.data(), st.data(), par.data());
        if (rc) return rc;
    }
    const int n_kf = 14;
    {   // matchToMap: the frame's keypoints (one per cell) + a local map of 3 n points with 6 observations each
        const int n_local = 3 * n, n_mp = n + n_local, per = 6;
        std::vector<int> cell_ptr((size_t) n + 1), cell_mp((size_t) n), obs_ptr((size_t) n_mp + 1), obs_kf, local((size_t) n_local), match((size_t) n_mp);
        std::vector<double> kq((size_t) n_kf * 4, 0.), kt((size_t) n_kf * 3, 0.), X((size_t) n_mp * 3);
        std::vector<uint8_t> m3((size_t) n_mp, 1), mhd((size_t) n_mp, 1), od, ohd;
        std::vector<float> opx;
        for (int f = 0; f < n_kf; f++) {
            kq[4 * (size_t) f + 3] = 1.;
            kt[3 * (size_t) f] = -0.05 * f;
        }
        for (int i = 0; i <= n; i++) cell_ptr[(size_t) i] = i;
        for (int i = 0; i < n; i++) cell_mp[(size_t) i] = i;
        for (int i = 0; i < n_local; i++) local[(size_t) i] = n + i;
        for (int p = 0; p < n_mp; p++) {
            const int c = p % n;
            const double x = ((c % cw) + 0.5 + 0.3 * (p / n)) * cell, y = ((c / cw) + 0.5) * cell, z = 4.;
            X[3 * (size_t) p] = (x - k.cx) / k.fx * z; X[3 * (size_t) p + 1] = (y - k.cy) / k.fy * z; X[3 * (size_t) p + 2] = z;
            obs_ptr[(size_t) p] = (int) obs_kf.size();
            for (int o = 0; o < per; o++) {
                obs_kf.push_back((p + o) % n_kf);
                opx.push_back((float) x);
                opx.push_back((float) y);
                for (int b = 0; b < 32; b++) od.push_back((uint8_t) (rnd() * 255.f));
                ohd.push_back(1);
            }
        }
        obs_ptr[(size_t) n_mp] = (int) obs_kf.size();
        rc = match_to_map(cell, cw, n, cell_ptr.data(), cell_mp.data(), n_kf, kq.data(), kt.data(), n_mp, X.data(), m3.data(), mhd.data(), obs_ptr.data(),
                          obs_kf.data(), opx.data(), od.data(), ohd.data(), n_kf - 1, n, n_local, local.data(), 2.0f, 0.2f, match.data());
        if (rc) return rc;
    }
    {   // local BA: 14 keyframes, 3 n points anchored round-robin, 6 further observations each
        const int n_pt = 3 * n, per = 6, n_obs = n_pt * per;
        std::vector<double> poses((size_t) n_kf * 7, 0.), auv((size_t) n_pt * 2), inv((size_t) n_pt, 0.25), ouv((size_t) n_obs * 2), chi2((size_t) n_obs);
        std::vector<uint8_t> kc((size_t) n_kf, 0), dp((size_t) n_obs);
        std::vector<int> pa((size_t) n_pt), okf((size_t) n_obs), opt((size_t) n_obs);
        kc[0] = kc[1] = 1;
        for (int f = 0; f < n_kf; f++) {
            poses[7 * (size_t) f] = 0.05 * f;   // Twc: camera f sits at x = 0.05 f
            poses[7 * (size_t) f + 6] = 1.;
        }
        for (int p = 0; p < n_pt; p++) {
            const int a = p % n_kf;
            const double u = 40. + rnd() * (W - 80), v = 40. + rnd() * (H - 80), z = 4.;
            pa[(size_t) p] = a;
            auv[2 * (size_t) p] = u; auv[2 * (size_t) p + 1] = v;
            const double xw = (u - k.cx) / k.fx * z + 0.05 * a, yw = (v - k.cy) / k.fy * z;
            for (int o = 0; o < per; o++) {
                const int f = (a + 1 + o) % n_kf;
                const size_t e = (size_t) p * per + (size_t) o;
                okf[e] = f;
                opt[e] = p;
                ouv[2 * e] = k.fx * (xw - 0.05 * f) / z + k.cx + 0.4 * (rnd() - 0.5);
                ouv[2 * e + 1] = k.fy * yw / z + k.cy + 0.4 * (rnd() - 0.5);
            }
        }
        rc = local_ba(n_kf, poses.data(), kc.data(), n_pt, pa.data(), auv.data(), inv.data(), n_obs, okf.data(), opt.data(), ouv.data(), 5, chi2.data(),
                      dp.data());
        if (rc) return rc;
    }
    pending_.active = false;
    m->trk.fused_active = false;
    m->trk.pose_pending = false;
    return ALVA_OK;
}

int HipStages::build_from(const uint8_t *d_src) {
    Impl &M = *m;
    const bool hit = M.ahead_enqueued && M.ahead_src == d_src;
    M.frame_src = d_src;   // (the scene stages' light binning reads the colour frame itself)
    M.ahead_enqueued = false;
    M.ahead_src = nullptr;
    // rotate: previous <- current <- next; the old previous becomes the free slot
    const int freed = M.prev;
    M.prev = M.cur;
    M.cur = M.nxt;
    M.nxt = freed;
    std::swap(M.d_gray, M.d_gray_next);
    if (hit) return ALVA_OK;
    if (!m->clahe) return alva_pyramid_build_from_rgba(m->ctx, m->pyr[m->cur], d_src, (size_t) m->cam.width * 4, m->d_gray, (size_t) m->cam.width);
    int rc = alva_rgba2gray(m->ctx, d_src, (size_t) m->cam.width * 4, m->cam.width, m->cam.height, m->d_gray, (size_t) m->cam.width);
    if (rc) return rc;
    // visual_frontend.cpp:16-18: clip limit 3, grid = image size / 50 (state.hpp:45-46)
    rc = alva_clahe(m->ctx, m->d_gray, (size_t) m->cam.width, m->cam.width, m->cam.height, 3.0, m->cam.width / 50, m->cam.height / 50, m->d_eq,
                    (size_t) m->cam.width);
    if (rc) return rc;
    rc = alva_pyramid_build_from_gray(m->ctx, m->pyr[m->cur], m->d_eq, (size_t) m->cam.width);
    if (rc) return rc;
    if (g_alva_lane) ALVA_HIP(alva_stream_sync(m->st));   // in a group the tracker runs on the lane's stream: these images are on the session's own
    return ALVA_OK;
}

// Look-ahead (no reference counterpart; the reference receives one frame per call): the caller names the frame of its NEXT call, and its
// gray image + LK pyramid are enqueued on the SAME stream right behind this frame's pose kernels, into the rotation's free slot: they run
// while the host does its pose bookkeeping, the keyframe decision and the next frame's slot table -- a window in which the GPU is otherwise
// idle -- instead of at the start of the next call.  (First version: a second stream beside the pose solve, ordered by two events.  The
// cross-queue waits cost what the overlap gained: 2 721 vs 2 742 frames/s sustained, `profiles/r3j_bench_n1.json`.)  The next
// new_frame_device takes the slot over when its pointer is the hinted one, and rebuilds as usual when it is not: results never depend
// on hints.  A frame that enqueues no pose solve builds ahead at the end of the call.
void HipStages::hint_next_frame_device(const uint8_t *d_rgba) {
    if (m->clahe) return;   // (the CLAHE chain shares d_eq / context scratch with the current frame: no look-ahead there)
    m->ahead_src = d_rgba;
    m->ahead_enqueued = false;
}

int HipStages::build_ahead() {
    Impl &M = *m;
    if (!M.ahead_src || M.ahead_enqueued) return ALVA_OK;
    const int rc = alva_pyramid_build_from_rgba(M.ctx, M.pyr[M.nxt], M.ahead_src, (size_t) M.cam.width * 4, M.d_gray_next, (size_t) M.cam.width);
    if (rc) return rc;
    M.ahead_enqueued = true;
    return ALVA_OK;
}

// The caller's frame buffer is pageable memory (the reference's wasm heap): by default a frame goes through a pinned staging copy
// (one memcpy + one DMA).  A caller that reuses ONE buffer -- src/system.js allocates memImg once and writes every frame into it
// (:63-67, :175) -- registers it explicitly (register_frame_buffer = alva_system_register_frame_buffer): the pages are locked and
// mapped, and k_level0 (gray + pyramid level 0) then reads the frame straight out of host memory over PCIe -- no staging copy, no
// copy command, no separate device RGBA buffer.  Registration is the caller's statement about the buffer's lifetime; nothing is
// inferred from pointer values (an address seen twice says nothing about the pages behind it).
int HipStages::register_frame_buffer(const uint8_t *buf, size_t bytes) {
    ALVA_HIP(hipSetDevice(m->device));
    const int urc = unregister_frame_buffer();
    if (urc) return urc;
    if (!buf) return ALVA_OK;
    ALVA_ARG(bytes >= (size_t) m->cam.width * m->cam.height * 4 && ((uintptr_t) buf & 15) == 0);
    ALVA_HIP(hipHostRegister((void *) buf, bytes, hipHostRegisterMapped));
    void *dp = nullptr;
    if (hipHostGetDevicePointer(&dp, (void *) buf, 0) != hipSuccess || !dp) {
        (void) hipGetLastError();
        (void) hipHostUnregister((void *) buf);
        alva_set_error("alva_system_register_frame_buffer: the registered buffer has no device mapping");
        return ALVA_ERR_HIP;
    }
    m->registered = buf;
    m->registered_dev = (const uint8_t *) dp;
    m->registered_bytes = bytes;
    return ALVA_OK;
}

int HipStages::alloc_frame_buffer(size_t bytes, uint8_t **h_writable) {
    ALVA_HIP(hipSetDevice(m->device));
    ALVA_ARG(h_writable && bytes >= (size_t) m->cam.width * m->cam.height * 4);
    if (m->bar_frame) {
        ALVA_HIP(alva_stream_sync(m->st));
        ALVA_HIP(hipFree(m->bar_frame));
        m->bar_frame = nullptr;
        m->bar_frame_bytes = 0;
    }
    if (!Impl::host_can_store_to_device_memory(m->device) || getenv("ALVA_NO_BAR_FRAME")) {
        alva_set_error("alva_system_alloc_frame_buffer: device memory is not host-writable on this system (no large BAR)");
        return ALVA_ERR_STATE;   // the caller falls back to its registered host buffer (alvaar_amd/system.py)
    }
    // fine-grained (bar_alloc_flag): every frame rewrites the buffer from the host, an L2 must not answer with the previous frame's line
    if (hipExtMallocWithFlags((void **) &m->bar_frame, bytes, Impl::bar_alloc_flag) != hipSuccess) {
        (void) hipGetLastError();
        m->bar_frame = nullptr;
        alva_set_error("alva_system_alloc_frame_buffer: no host-writable device memory on this system");
        return ALVA_ERR_STATE;
    }
    ALVA_HIP(Impl::scrub_host_written(m->bar_frame, bytes));
    m->bar_frame_bytes = bytes;
    *h_writable = m->bar_frame;
    return ALVA_OK;
}

int HipStages::unregister_frame_buffer() {
    if (!m->registered) return ALVA_OK;
    ALVA_HIP(hipSetDevice(m->device));
    ALVA_HIP(alva_stream_sync(m->st));   // no kernel may still be reading the pages
    m->upload_in_flight = false;
    const uint8_t *b = m->registered;
    m->registered = m->registered_dev = nullptr;
    m->registered_bytes = 0;
    ALVA_HIP(hipHostUnregister((void *) b));
    return ALVA_OK;
}

int HipStages::new_frame(const uint8_t *rgba) {
    ALVA_HIP(hipSetDevice(m->device));
    // a HOST frame inside a group (no group entry point takes one): the upload, its completion event and the kernels that read it belong on
    // the session's own stream -- the images are built there and waited for, so that the lane's tracker may read them
    struct NoLane {
        alva_lane *saved = g_alva_lane;
        NoLane() { g_alva_lane = nullptr; }
        ~NoLane() { g_alva_lane = saved; }
    } no_lane;
    const bool in_group = no_lane.saved != nullptr;
    const size_t bytes = (size_t) m->cam.width * m->cam.height * 4;
    if (m->bar_frame && rgba >= m->bar_frame && rgba + bytes <= m->bar_frame + m->bar_frame_bytes && (((uintptr_t) rgba) & 15) == 0) {
        // the caller stored the frame into device memory itself (alloc_frame_buffer): it IS a device frame; its write-combined stores
        // leave the core before the launch's doorbell does
        __builtin_ia32_sfence();
        const int rc = build_from(rgba);
        if (rc) return rc;
        if (in_group) ALVA_HIP(alva_stream_sync(m->st));
        else {
            // the buffer is the caller's again when the call returns (frame_done waits): a frame that makes no later stream wait -- too
            // few tracks, a reset -- must not leave the image kernels reading what the caller's next memImg.write overwrites
            m->upload_in_flight = true;
            ALVA_HIP(hipEventRecord(m->upload_done, m->st));
        }
        return ALVA_OK;
    }
    if (m->registered && rgba >= m->registered && rgba + bytes <= m->registered + m->registered_bytes && (((uintptr_t) rgba) & 15) == 0) {
        // zero-copy: the image kernels read the caller's pages; frame_done() waits for them before the call returns the buffer
        const int rc = build_from(m->registered_dev + (rgba - m->registered));
        if (rc) return rc;
        m->upload_in_flight = true;
        ALVA_HIP(hipEventRecord(m->upload_done, m->st));
        if (in_group) ALVA_HIP(alva_stream_sync(m->st));
        return ALVA_OK;
    }
    memcpy(m->h_rgba, rgba, bytes);
    ALVA_HIP(hipMemcpyAsync(m->d_rgba, m->h_rgba, bytes, hipMemcpyHostToDevice, m->st));
    const int rc = build_from(m->d_rgba);
    if (rc) return rc;
    if (in_group) ALVA_HIP(alva_stream_sync(m->st));
    return ALVA_OK;
}

int HipStages::new_frame_device(const uint8_t *d_rgba) {
    ALVA_HIP(hipSetDevice(m->device));
    return build_from(d_rgba);
}

int HipStages::frame_done() {
    if (m->ahead_src && !m->ahead_enqueued) {   // a frame that tracked nothing: the look-ahead goes out now
        const int rc = build_ahead();
        if (rc) return rc;
    }
    if (m->upload_in_flight) {
        m->upload_in_flight = false;
        ALVA_HIP(alva_event_sync(m->upload_done));
    }
    return ALVA_OK;
}

void HipStages::reset_images() {}  // the pyramids are rebuilt before they are read again (frame 0 tracks nothing)

// One tracking step as ONE device-side chain: glue -> tracker (one level, from the projected priors) -> glue -> tracker (full pyramid)
// -> glue, one host wait; then the pose solve (P3P-LMedS -> PnP, alva_compute_pose) is enqueued and collected by track_pose_collect
// after the map layer has done its tracker bookkeeping.  Inputs are read from and per-slot results written to pinned host memory
// by the kernels themselves: no copy commands.  The steps are Impl's track_* helpers, in this order.
int HipStages::track_begin(const TrackJob &job, TrackKlt &out) {
    TrackStepState &T = m->trk;
    T.info = TrackStepInfo{};
    if (!m->fused || (job.want_pose && !job.do_p3p)) return m->track_composed(*this, job, out);
    T.pose_pending = false;
    pending_.active = false;
    out.code_v = nullptr;
    out.px_v = out.unpx_v = nullptr;
    out.bv_v = nullptr;
    out.p3p_req = 0;
    out.n_pose = 0;
    const int n_prev = T.valid_n;
    T.valid_n = -1;   // (set again below by a launch that leaves a complete table behind: not by n == 0, not by an error)
    if (job.n == 0) return ALVA_OK;
    ALVA_HIP(hipSetDevice(m->device));
    int rc = m->track_reserve(job.n);
    if (rc) return rc;
    const int par = T.par ^ 1;   // this frame's table and d_px
    Impl::Step s{job};
    rc = m->track_route(job, n_prev, par, &s.route);
    if (rc) return rc;
    if (s.route != TRACK_ROUTE_PINNED) {
        __builtin_ia32_sfence();   // the table's write-combined stores leave the core before the launch's doorbell does
    } else {
        const TrackTable pin = T.pin_block().in;
        if (!(job.px == pin.px && job.is3d == pin.is3d && job.wpt == pin.wpt)) {   // (else track_slot_buffers was used: it is there already)
            memcpy(pin.px, job.px, (size_t) job.n * 8);
            memcpy(pin.is3d, job.is3d, (size_t) job.n);
            memcpy(pin.wpt, job.wpt, (size_t) job.n * 24);
        }
    }
    m->track_fill_slots(s, par);
    rc = m->track_launch(s, 0);   // the tracker launch precedes the tail's
    if (rc) return rc;
    rc = m->track_queue_tail(s);
    if (rc) return rc;
    // only now that the tail is queued, and only on the device routes: this frame's table and (once the launch is through) its tracked
    // positions are complete on the device
    if (s.route != TRACK_ROUTE_PINNED) {
        T.par = par;
        T.valid_n = job.n;
    }
    rc = m->track_answer_early(*this, s);
    if (rc) return rc;
    rc = m->track_wait(s);
    if (rc) return rc;
    if (s.word.req) {
        rc = m->track_retry(s);
        if (rc) return rc;
    }
    return m->track_publish(s, out);
}

bool HipStages::track_slot_buffers(int n, float **px, uint8_t **is3d, double **wpt) {
    if (!m->fused || n <= 0) return false;
    if (hipSetDevice(m->device) != hipSuccess || m->track_reserve(n) != ALVA_OK) return false;
    const TrackStepState &T = m->trk;
    // device memory, written in place (track_reserve): the table the NEXT launch takes | the pinned table
    const TrackTable t = T.bar_table && T.in ? T.in_block().table[T.par ^ 1] : T.pin_block().in;
    *px = t.px;
    *is3d = t.is3d;
    *wpt = t.wpt;
    return true;
}

bool HipStages::track_table_on_device() const { return m->fused && m->trk.bar_table && m->trk.in != nullptr; }

HipStages::TrackStepInfo HipStages::track_step_info() const { return m->trk.info; }

void HipStages::track_pose_rows(const double **Pbv, const double **Puv, const double **Pwpt) const {
    *Pbv = m->trk.rows[0];
    *Puv = m->trk.rows[1];
    *Pwpt = m->trk.rows[2];
}

uint16_t *HipStages::track_carry_buffer(int n_prev, int n) {
    const TrackStepState &T = m->trk;
    if (!m->fused || !T.carry_ok || !T.bar_table || !T.in || g_alva_lane) return nullptr;
    if (n <= 0 || n > n_prev || n_prev != T.valid_n || n_prev >= 65536 || n + 1 > T.cap) return nullptr;   // (the caller may write entry n: room for n + 1)
    return T.in_block().carry;
}

int HipStages::track_pose_collect(TrackPose &out) {
    TrackStepState &T = m->trk;
    if (!T.fused_active) return Stages::track_pose_collect(out);
    T.fused_active = false;
    out.status = -1;
    out.p3p_outlier.assign((size_t) T.pose_total, 0);
    out.pnp_outlier.assign((size_t) T.pose_total, 0);
    if (!T.pose_pending) return ALVA_OK;
    T.pose_pending = false;
    int status = 0;
    int rc = alva_compute_pose_collect_p3p(m->ctx, out.pose7, out.pose7_p3p, out.p3p_outlier.data(), out.pnp_outlier.data(), &status);
    if (rc) return rc;
    alva_lane_clean();   // the refinement's completion word has been seen: nothing of this session is left on the lane
    out.status = status;
    return ALVA_OK;
}

int HipStages::fbklt(int levels, int n, const float *pts, float *prior, uint8_t *status) {
    if (n <= 0) return ALVA_OK;
    StagePlan p;
    const size_t a = p.add((size_t) n * 8), b = p.add((size_t) n * 8), c = p.add((size_t) n);
    std::vector<uint8_t *> d, h;
    int rc = m->carve(p, d, h);
    if (rc) return rc;
    UP(m->st, a, pts, (size_t) n * 8);
    UP(m->st, b, prior, (size_t) n * 8);
    // state.hpp:50-56: kltError_ 30, kltMaxFbDistance_ 0.5, 30 iterations, 0.01 px
    rc = alva_fbklt_track(m->ctx, m->pyr[m->prev], m->pyr[m->cur], levels, 30.f, 0.5f, 30, 0.01f, (const float *) d[a], (float *) d[b], d[c], n);
    if (rc) return rc;
    DOWN(m->st, b, (size_t) n * 8);
    DOWN(m->st, c, (size_t) n);
    ALVA_HIP(alva_stream_sync(m->st));
    memcpy(prior, h[b], (size_t) n * 8);
    memcpy(status, h[c], (size_t) n);
    return ALVA_OK;
}

int HipStages::compute_keypoints(int n, const float *px, float *unpx, double *bv) {
    if (n <= 0) return ALVA_OK;
    StagePlan p;
    const size_t a = p.add((size_t) n * 8), b = p.add((size_t) n * 8), c = p.add((size_t) n * 24);
    std::vector<uint8_t *> d, h;
    int rc = m->carve(p, d, h);
    if (rc) return rc;
    UP(m->st, a, px, (size_t) n * 8);
    const Camera &k = m->cam;
    rc = alva_undistort_points(m->ctx, (const float *) d[a], n, k.fx, k.fy, k.cx, k.cy, k.k1, k.k2, k.p1, k.p2, (float *) d[b]);
    if (rc) return rc;
    hipLaunchKernelGGL(k_bearing, dim3(alva_divup(n, 256)), dim3(256), 0, m->st, (const float *) d[b], n, m->d_invK, (double *) d[c]);
    ALVA_LAUNCH_CHECK();
    rc = m->down_span(p, d, h, b, c);
    if (rc) return rc;
    ALVA_HIP(alva_stream_sync(m->st));
    memcpy(unpx, h[b], (size_t) n * 8);
    memcpy(bv, h[c], (size_t) n * 24);
    return ALVA_OK;
}

int HipStages::project_dist(int n, const double *cam_pts, float *px) {
    if (n <= 0) return ALVA_OK;
    StagePlan p;
    const size_t a = p.add((size_t) n * 24), b = p.add((size_t) n * 8);
    std::vector<uint8_t *> d, h;
    int rc = m->carve(p, d, h);
    if (rc) return rc;
    UP(m->st, a, cam_pts, (size_t) n * 24);
    const Camera &k = m->cam;
    rc = alva_project_dist(m->ctx, (const double *) d[a], n, k.fx, k.fy, k.cx, k.cy, k.k1, k.k2, k.p1, k.p2, (float *) d[b]);
    if (rc) return rc;
    DOWN(m->st, b, (size_t) n * 8);
    ALVA_HIP(alva_stream_sync(m->st));
    memcpy(px, h[b], (size_t) n * 8);
    return ALVA_OK;
}

int HipStages::p3p(int n, const double *bv, const double *wpt, int do_random, double *pose7, int *outliers, int *n_outliers, int *ok) {
    *ok = 0;
    *n_outliers = 0;
    if (n < 4) return ALVA_OK;  // multi_view_geometry.cpp:40-43
    // the LMedS median lives in LDS: at most ALVA_P3P_MAX_N correspondences per call; a larger frame is solved on its first keypoints
    // (container order) and the rest is left to the PnP's chi2 sweep
    const int nn = n > ALVA_P3P_MAX_N ? ALVA_P3P_MAX_N : n;
    StagePlan p;
    const size_t a = p.add((size_t) nn * 24), b = p.add((size_t) nn * 24);
    std::vector<uint8_t *> d, h;
    int rc = m->carve(p, d, h);
    if (rc) return rc;
    UP(m->st, a, bv, (size_t) nn * 24);
    UP(m->st, b, wpt, (size_t) nn * 24);
    double R[9], t[3];
    rc = m->pose().p3p(m->ctx, (const double *) d[a], (const double *) d[b], nn, do_random, R, t, outliers, n_outliers, ok);
    if (rc) return rc;
    if (*ok) {
        SE3 T;
        rot_to_quat(R, T.q);  // Twc.setRotationMatrix (multi_view_geometry.cpp:104-105)
        for (int i = 0; i < 3; i++) T.t[i] = t[i];
        se3_to_pose7(T, pose7);
    } else {
        *n_outliers = 0;
    }
    return ALVA_OK;
}

int HipStages::pnp(int n, const double *unpx_d, const double *wpt, double *pose7, int *outliers, int *n_outliers, int *ok) {
    *ok = 0;
    *n_outliers = 0;
    if (n <= 0) return ALVA_OK;
    StagePlan p;
    const size_t a = p.add((size_t) n * 16), b = p.add((size_t) n * 24);
    std::vector<uint8_t *> d, h;
    int rc = m->carve(p, d, h);
    if (rc) return rc;
    UP(m->st, a, unpx_d, (size_t) n * 16);
    UP(m->st, b, wpt, (size_t) n * 24);
    double info[8];
    return m->pose().refine(m->ctx, (const double *) d[a], (const double *) d[b], n, pose7, outliers, n_outliers, info, ok);
}

int HipStages::five_point(int n, const double *bv_kf, const double *bv_cur, int do_random, double *R, double *t, int *outliers, int *n_outliers,
                          int *ok) {
    *ok = 0;
    *n_outliers = 0;
    if (n < 8) return ALVA_OK;
    StagePlan p;
    const size_t a = p.add((size_t) n * 24), b = p.add((size_t) n * 24);
    std::vector<uint8_t *> d, h;
    int rc = m->carve(p, d, h);
    if (rc) return rc;
    UP(m->st, a, bv_kf, (size_t) n * 24);
    UP(m->st, b, bv_cur, (size_t) n * 24);
    std::vector<uint8_t> inl((size_t) n);
    rc = alva_compute_5pt_essential(m->ctx, (const double *) d[a], (const double *) d[b], n, 100, 3.0f, 1, do_random, 12345u, (float) m->cam.fx,
                                    (float) m->cam.fy, R, t, inl.data(), nullptr, ok);
    if (rc) return rc;
    if (*ok)
        for (int i = 0; i < n; i++)
            if (!inl[(size_t) i]) outliers[(*n_outliers)++] = i;
    return ALVA_OK;
}

int HipStages::detect(int cell, int n_occ, const float *occupied, int cap, float *pts, int *count) {
    const int rc = detect_begin(cell, n_occ, occupied, cap);
    return rc ? rc : detect_end(pts, count);
}

// the detector enqueued on the stream (all its launches + the copy of the whole output buffer back: the count is not known yet); the
// map layer updates its descriptor medoids meanwhile
int HipStages::detect_begin(int cell, int n_occ, const float *occupied, int cap) {
    StagePlan p;
    const size_t a = p.add((size_t) (n_occ > 0 ? n_occ : 1) * 8), b = p.add((size_t) cap * 8);
    std::vector<uint8_t *> d, h;
    int rc = m->carve(p, d, h);
    if (rc) return rc;
    // Small keyframe stages read their inputs from and write their results to the PINNED mirror of the plan directly (h[], device-
    // accessible, uncached by the GPU): a copy command is a blit kernel of its own (~9 us on the GPU + a launch + two queue gaps), and these
    // stages move 3 - 80 KB.  The wait that ends each stage is a stream synchronisation, which makes the kernels' writes visible.
    if (n_occ > 0) memcpy(h[a], occupied, (size_t) n_occ * 8);
    const Camera &k = m->cam;
    const uint8_t *img = m->clahe ? m->d_eq : m->d_gray;  // detection runs on currImage_ (map_manager.cpp:213)
    // roi = CameraCalibration::roi_rect_ (camera_calibration.cpp:20): the image minus a border of 20 px
    rc = alva_detect_grid_enqueue(m->ctx, img, (size_t) k.width, k.width, k.height, cell, (const float *) h[a], n_occ, k.border, k.border,
                                  k.width - 2 * k.border, k.height - 2 * k.border, m->max_quality, (float *) h[b], cap, &m->det_pending);
    if (rc) return rc;
    m->det_h = h[b];
    m->det_cap = cap;
    return ALVA_OK;
}

int HipStages::detect_end(float *pts, int *count) {
    const int rc = alva_detect_grid_collect(m->ctx, &m->det_pending, &m->max_quality, count);   // waits for the stream: the copy above is done too
    if (rc) return rc;
    if (*count > m->det_cap) *count = m->det_cap;
    if (*count > 0) memcpy(pts, m->det_h, (size_t) *count * 8);
    return ALVA_OK;
}

int HipStages::describe(int n, const float *pts, uint8_t *desc, uint8_t *valid) {
    const int rc = describe_begin(n, pts);
    return rc ? rc : describe_end(desc, valid);
}

// the description enqueued on the stream (results land in the pinned mirror of the plan); the map layer enters the new keyframe into its
// map points' records meanwhile (no stage call in between: the next one carves the same staging)
int HipStages::describe_begin(int n, const float *pts) {
    m->dsc_n = n > 0 ? n : 0;
    if (n <= 0) return ALVA_OK;
    StagePlan p;
    const size_t a = p.add((size_t) n * 8), b = p.add((size_t) n * 32), c = p.add((size_t) n);
    std::vector<uint8_t *> d, h;
    int rc = m->carve(p, d, h);
    if (rc) return rc;
    memcpy(h[a], pts, (size_t) n * 8);
    rc = alva_describe(m->ctx, m->d_gray, (size_t) m->cam.width, m->cam.width, m->cam.height, (const float *) h[a], n, h[b], h[c]);
    if (rc) return rc;
    m->dsc_desc = h[b];
    m->dsc_valid = h[c];
    return ALVA_OK;
}

int HipStages::describe_end(uint8_t *desc, uint8_t *valid) {
    const int n = m->dsc_n;
    m->dsc_n = 0;
    if (n <= 0) return ALVA_OK;
    ALVA_HIP(alva_stream_sync(m->st));
    memcpy(desc, m->dsc_desc, (size_t) n * 32);
    memcpy(valid, m->dsc_valid, (size_t) n);
    return ALVA_OK;
}

int HipStages::describe_and_compute(int n, const float *pts, uint8_t *desc, uint8_t *valid, float *unpx, double *bv) {
    if (n <= 0) return ALVA_OK;
    StagePlan p;
    const size_t a = p.add((size_t) n * 8), b = p.add((size_t) n * 32), c = p.add((size_t) n), u = p.add((size_t) n * 8), v = p.add((size_t) n * 24);
    std::vector<uint8_t *> d, h;
    int rc = m->carve(p, d, h);
    if (rc) return rc;
    memcpy(h[a], pts, (size_t) n * 8);
    rc = alva_describe(m->ctx, m->d_gray, (size_t) m->cam.width, m->cam.width, m->cam.height, (const float *) h[a], n, h[b], h[c]);
    if (rc) return rc;
    const Camera &k = m->cam;
    rc = alva_undistort_points(m->ctx, (const float *) h[a], n, k.fx, k.fy, k.cx, k.cy, k.k1, k.k2, k.p1, k.p2, (float *) h[u]);
    if (rc) return rc;
    hipLaunchKernelGGL(k_bearing, dim3(alva_divup(n, 256)), dim3(256), 0, m->st, (const float *) h[u], n, m->d_invK, (double *) h[v]);
    ALVA_LAUNCH_CHECK();
    ALVA_HIP(alva_stream_sync(m->st));   // descriptors | validity | undistorted positions | bearings: one wait
    memcpy(desc, h[b], (size_t) n * 32);
    memcpy(valid, h[c], (size_t) n);
    memcpy(unpx, h[u], (size_t) n * 8);
    memcpy(bv, h[v], (size_t) n * 24);
    return ALVA_OK;
}

int HipStages::triangulate(int n, int n_groups, const double *T36, const int *group, const double *bv_l, const double *bv_r, const float *unpx_l,
                           const float *unpx_r, double *wpt, double *inv_depth, uint8_t *status, double *parallax) {
    if (n <= 0) return ALVA_OK;
    StagePlan p;
    const size_t iT = p.add((size_t) n_groups * 288), ig = p.add((size_t) n * 4), il = p.add((size_t) n * 24), ir = p.add((size_t) n * 24),
                 iul = p.add((size_t) n * 8), iur = p.add((size_t) n * 8), ilp = p.add((size_t) n * 24), iw = p.add((size_t) n * 24),
                 iid = p.add((size_t) n * 8), ist = p.add((size_t) n), ipar = p.add((size_t) n * 8);
    std::vector<uint8_t *> d, h;
    int rc = m->carve(p, d, h);
    if (rc) return rc;
    memcpy(h[iT], T36, (size_t) n_groups * 288);
    memcpy(h[ig], group, (size_t) n * 4);
    memcpy(h[il], bv_l, (size_t) n * 24);
    memcpy(h[ir], bv_r, (size_t) n * 24);
    memcpy(h[iul], unpx_l, (size_t) n * 8);
    memcpy(h[iur], unpx_r, (size_t) n * 8);
    const Camera &k = m->cam;
    rc = alva_triangulate(m->ctx, n, (const double *) h[iT], n_groups, (const int *) h[ig], (const double *) h[il], (const double *) h[ir],
                          (const float *) h[iul], (const float *) h[iur], k.fx, k.fy, k.cx, k.cy, 3.0f /* mapMaxReprojectionError_ */,
                          (double *) d[ilp], (double *) h[iw], (double *) h[iid], h[ist], (double *) h[ipar]);
    if (rc) return rc;
    ALVA_HIP(alva_stream_sync(m->st));
    memcpy(wpt, h[iw], (size_t) n * 24);
    memcpy(inv_depth, h[iid], (size_t) n * 8);
    memcpy(status, h[ist], (size_t) n);
    memcpy(parallax, h[ipar], (size_t) n * 8);
    return ALVA_OK;
}

uint8_t *HipStages::stage_scratch(size_t bytes) {
    // the call that follows carves [0, bytes) of both arenas: its arrays are already in place in the pinned one
    if (m->dev.grow(bytes, m->st) != ALVA_OK || m->pin.grow(bytes, m->st) != ALVA_OK) return nullptr;
    return m->pin.base;
}

int HipStages::match_to_map(int cell_size, int num_cells_w, int grid_cells, const int *cell_ptr, const int *cell_mp, int n_kf, const double *kf_q,
                            const double *kf_t, int n_mp, const double *mp_wpt, const uint8_t *mp_is3d, const uint8_t *mp_has_desc,
                            const int *obs_ptr, const int *obs_kf, const float *obs_px, const uint8_t *obs_desc, const uint8_t *obs_has_desc,
                            int frame_kf, int num_keypoints_3d, int n_local, const int *local, float max_proj_err, float dist_ratio,
                            int *match_of_mp) {
    if (n_mp <= 0) return ALVA_OK;
    const int n_obs = obs_ptr[n_mp], n_cell = cell_ptr[grid_cells];
    const Camera &k = m->cam;
    const double calib[10] = {k.fx, k.fy, k.cx, k.cy, k.k1, k.k2, k.p1, k.p2, (double) k.width, (double) k.height};
    StagePlan p;
    const size_t icp = p.add((size_t) (grid_cells + 1) * 4), icm = p.add((size_t) (n_cell > 0 ? n_cell : 1) * 4), iq = p.add((size_t) n_kf * 32),
                 it = p.add((size_t) n_kf * 24), iw = p.add((size_t) n_mp * 24), i3 = p.add((size_t) n_mp), ihd = p.add((size_t) n_mp),
                 iop = p.add((size_t) (n_mp + 1) * 4), iok = p.add((size_t) (n_obs > 0 ? n_obs : 1) * 4),
                 iox = p.add((size_t) (n_obs > 0 ? n_obs : 1) * 8), iod = p.add((size_t) (n_obs > 0 ? n_obs : 1) * 32),
                 ioh = p.add((size_t) (n_obs > 0 ? n_obs : 1)), il = p.add((size_t) (n_local > 0 ? n_local : 1) * 4), im = p.add((size_t) n_mp * 4);
    std::vector<uint8_t *> d, h;
    int rc = m->carve(p, d, h);
    if (rc) return rc;
    UP(m->st, icp, cell_ptr, (size_t) (grid_cells + 1) * 4);
    UP(m->st, icm, cell_mp, (size_t) n_cell * 4);
    UP(m->st, iq, kf_q, (size_t) n_kf * 32);
    UP(m->st, it, kf_t, (size_t) n_kf * 24);
    UP(m->st, iw, mp_wpt, (size_t) n_mp * 24);
    UP(m->st, i3, mp_is3d, (size_t) n_mp);
    UP(m->st, ihd, mp_has_desc, (size_t) n_mp);
    UP(m->st, iop, obs_ptr, (size_t) (n_mp + 1) * 4);
    UP(m->st, iok, obs_kf, (size_t) n_obs * 4);
    UP(m->st, iox, obs_px, (size_t) n_obs * 8);
    UP(m->st, iod, obs_desc, (size_t) n_obs * 32);
    UP(m->st, ioh, obs_has_desc, (size_t) n_obs);
    UP(m->st, il, local, (size_t) n_local * 4);
    rc = alva_match_to_map_flags(m->ctx, calib, cell_size, num_cells_w, grid_cells, (const int *) d[icp], (const int *) d[icm], n_kf,
                                 (const double *) d[iq], (const double *) d[it], n_mp, (const double *) d[iw], d[i3], d[ihd], (const int *) d[iop],
                                 (const int *) d[iok], (const float *) d[iox], d[iod], d[ioh], frame_kf, num_keypoints_3d, n_local,
                                 (const int *) d[il], max_proj_err, dist_ratio, (int *) d[im]);
    if (rc) return rc;
    DOWN(m->st, im, (size_t) n_mp * 4);
    ALVA_HIP(alva_stream_sync(m->st));
    memcpy(match_of_mp, h[im], (size_t) n_mp * 4);
    return ALVA_OK;
}

// The record arena: pinned, zero-filled, never moved.  The kernels find a record through the device-resident table of chunk addresses.
MpRec *HipStages::mp_arena_chunk(int chunk) {
    if (chunk < 0 || chunk >= Impl::REC_TAB_CAP) return nullptr;
    if (hipSetDevice(m->device) != hipSuccess) return nullptr;
    if (!m->d_rec_tab) {
        if (hipMalloc((void **) &m->d_rec_tab, (size_t) Impl::REC_TAB_CAP * sizeof(void *)) != hipSuccess) return nullptr;
        if (hipMemset(m->d_rec_tab, 0, (size_t) Impl::REC_TAB_CAP * sizeof(void *)) != hipSuccess) return nullptr;
    }
    if (m->rec_chunks.capacity() < (size_t) Impl::REC_TAB_CAP) m->rec_chunks.reserve((size_t) Impl::REC_TAB_CAP);
    while ((int) m->rec_chunks.size() <= chunk) {
        MpRec *c = nullptr;
        if (hipHostMalloc((void **) &c, (size_t) MP_CHUNK * sizeof(MpRec), hipHostMallocDefault) != hipSuccess) return nullptr;
        memset(c, 0, (size_t) MP_CHUNK * sizeof(MpRec));
        const MpRec *cc = c;
        // (rare: once per 4096 map points) a blocking 8-byte copy: the kernels of later calls read the entry
        if (hipMemcpy(m->d_rec_tab + m->rec_chunks.size(), &cc, sizeof(cc), hipMemcpyHostToDevice) != hipSuccess) {
            (void) hipHostFree(c);
            return nullptr;
        }
        m->rec_chunks.push_back(c);
    }
    return m->rec_chunks[(size_t) chunk];
}

// Mapper::matchToMap on the records: the job's own arrays (cells, keyframe table, row slots, local list) lie in stage_scratch() and go
// up with ONE copy; the map itself is gathered by the kernels (alva_match_to_map_records)
int HipStages::match_to_map_rec(const MatchJob &J, int *match_of_mp) {
    if (J.n_mp <= 0) return ALVA_OK;
    if (!m->med || !alva_medoid_tables(m->med) || !m->d_rec_tab) return ALVA_ERR_STATE;   // (map points exist => their tables were replayed)
    int frame_kf = -1;
    for (int i = 0; i < J.n_kf; i++)
        if (J.kf_ids[i] == J.frame_kfid) frame_kf = i;
    if (frame_kf < 0) return ALVA_ERR_ARG;
    const int n_cell = J.cell_ptr[J.grid_cells];
    const Camera &k = m->cam;
    const double calib[10] = {k.fx, k.fy, k.cx, k.cy, k.k1, k.k2, k.p1, k.p2, (double) k.width, (double) k.height};
    const uint8_t *pb = m->pin.base, *pe = pb ? pb + m->pin.cap : nullptr;
    const uint8_t *ptrs[] = {(const uint8_t *) J.cell_ptr, (const uint8_t *) J.cell_mp, (const uint8_t *) J.kf_ids, (const uint8_t *) J.kf_q,
                             (const uint8_t *) J.kf_t, (const uint8_t *) J.mp_slot, (const uint8_t *) J.local, (const uint8_t *) match_of_mp};
    const size_t lens[] = {(size_t) (J.grid_cells + 1) * 4, (size_t) n_cell * 4, (size_t) J.n_kf * 4, (size_t) J.n_kf * 32, (size_t) J.n_kf * 24,
                           (size_t) J.n_mp * 4, (size_t) J.n_local * 4, (size_t) J.n_mp * 4};
    size_t lo = (size_t) -1, hi = 0;
    for (int i = 0; i < 8; i++) {
        if (lens[i] == 0) continue;
        if (!pb || ptrs[i] < pb || ptrs[i] + lens[i] > pe) return ALVA_ERR_ARG;   // the map layer assembles the job in stage_scratch()
        if (i < 7) {
            lo = std::min(lo, (size_t) (ptrs[i] - pb));
            hi = std::max(hi, (size_t) (ptrs[i] - pb) + lens[i]);
        }
    }
    if (m->dev.cap < m->pin.cap) return ALVA_ERR_STATE;
    auto dv = [&](const void *hp) { return m->dev.base + ((const uint8_t *) hp - pb); };
    ALVA_HIP(hipMemcpyAsync(m->dev.base + lo, pb + lo, hi - lo, hipMemcpyHostToDevice, m->st));
    const int rc = alva_match_to_map_records(m->ctx, calib, J.cell_size, J.num_cells_w, J.grid_cells, (const int *) dv(J.cell_ptr), (const int *) dv(J.cell_mp),
                                             J.n_kf, (const int *) dv(J.kf_ids), (const double *) dv(J.kf_q), (const double *) dv(J.kf_t), frame_kf,
                                             J.frame_kfid, J.n_mp, (const int *) dv(J.mp_slot), (const void *const *) m->d_rec_tab,
                                             alva_medoid_tables(m->med), J.num_keypoints_3d, J.n_local, (const int *) dv(J.local), J.max_proj_err,
                                             J.dist_ratio, match_of_mp);   // (pinned, written once per entry by the last kernel: no copy back)
    if (rc) return rc;
    ALVA_HIP(alva_stream_sync(m->st));
    return ALVA_OK;
}

int HipStages::local_ba(int n_kf, double *poses7, const uint8_t *kf_const, int n_pt, const int *pt_anchor_kf, const double *pt_anchor_uv,
                        double *pt_inv_depth, int n_obs, const int *obs_kf, const int *obs_pt, const double *obs_uv, int max_iters, double *chi2,
                        uint8_t *depth_pos) {
    const Camera &k = m->cam;
    const double calib[4] = {k.fx, k.fy, k.cx, k.cy};
    double info[4];
    int ok = 0;
    // optimizer.cpp:251-262: function tolerance 1e-3, Huber on sqrt(robustCostThreshold_) -- a float in the reference (:8, :22)
    return alva_local_ba(m->ctx, n_kf, poses7, kf_const, calib, 1, n_pt, pt_anchor_kf, pt_anchor_uv, pt_inv_depth, n_obs, obs_kf, obs_pt, obs_uv,
                         max_iters, 0.001, (double) 5.9915f, chi2, depth_pos, info, &ok);
}

int HipStages::local_ba_csr(int n_kf, double *poses7, const uint8_t *kf_const, int n_pt, const int *pt_ptr, const int *pt_anchor_kf,
                            const double *pt_anchor_uv, double *pt_inv_depth, int n_obs, const int *obs_kf, const double *obs_uv, int max_iters,
                            double chi2_threshold, uint64_t *bad_bits, int *n_bad) {
    const Camera &k = m->cam;
    const double calib[4] = {k.fx, k.fy, k.cx, k.cy};
    double info[4];
    int ok = 0;
    if (n_kf > 32) {   // (the device-side pair grouping is sized for the mapper's window; larger problems take the host-structured solve)
        return Stages::local_ba_csr(n_kf, poses7, kf_const, n_pt, pt_ptr, pt_anchor_kf, pt_anchor_uv, pt_inv_depth, n_obs, obs_kf, obs_uv, max_iters,
                                    chi2_threshold, bad_bits, n_bad);
    }
    // optimizer.cpp:251-262: function tolerance 1e-3, Huber on sqrt(robustCostThreshold_) -- a float in the reference (:8, :22)
    return alva_local_ba_csr(m->ctx, n_kf, poses7, kf_const, calib, n_pt, pt_ptr, pt_anchor_kf, pt_anchor_uv, pt_inv_depth, n_obs, obs_kf, obs_uv,
                             max_iters, 0.001, (double) 5.9915f, chi2_threshold, (unsigned long long *) bad_bits, n_bad, info, &ok);
}

// f1: the map points' descriptor tables live on the device (medoid.hip); the replay is enqueued behind the keyframe's other work on the
// session's stream and nothing waits for it -- only an export does
int HipStages::medoid_replay(int n_ops, const alva_medoid::MedoidOp *ops, int n_mp, const int *mp_slot, const int *first_op, int slots) {
    ALVA_HIP(hipSetDevice(m->device));
    if (!m->med) {
        const int rc = alva_medoid_store_create(m->ctx, &m->med);
        if (rc) return rc;
    }
    return alva_medoid_replay(m->med, n_ops, ops, n_mp, mp_slot, first_op, slots);
}
int HipStages::medoid_export(int n, const int *mp_slot, uint8_t *desc32, uint8_t *valid, int *info3) {
    if (!m->med) {   // nothing was ever replayed: every table is a fresh one
        if (desc32) memset(desc32, 0, 32 * (size_t) n);
        if (valid) memset(valid, 0, (size_t) n);
        if (info3)
            for (int i = 0; i < n; i++) { info3[3 * i] = 0; info3[3 * i + 1] = -1; info3[3 * i + 2] = 0; }
        return ALVA_OK;
    }
    return alva_medoid_export(m->med, n, mp_slot, desc32, valid, info3);
}
int HipStages::pack_map_records(int n_slots, int stream_id, int capacity, uint8_t *d_out, int *count) {
    if (!m->med || !m->d_rec_tab) return ALVA_ERR_STATE;
    return alva_pack_map_records(m->med, (const void *const *) m->d_rec_tab, n_slots, stream_id, capacity, d_out, count);
}
// One relocalization attempt (Stages::relocalize): the detector on the whole image (host wait: its count sizes the description), then
// description, undistortion, bearings and the global match (alva_reloc_match, which also gathers the pose solve's correspondences) queued
// on the session's stream with one wait, then the tracker's pose chain (alva_compute_pose: P3P-LMedS -> robust PnP) on the gathered
// device arrays.  The map's rows are packed on the device from the resident records when the job says the map changed.
int HipStages::relocalize(const RelocJob &job, RelocResult &out) {
    out = RelocResult();
    ALVA_HIP(hipSetDevice(m->device));
    const Camera &k = m->cam;
    if (job.cell <= 0) return ALVA_ERR_ARG;
    const int cap = ((k.width + job.cell - 1) / job.cell) * ((k.height + job.cell - 1) / job.cell) + 8;
    std::vector<float> pts((size_t) cap * 2);
    int n = 0;
    const double quality = m->max_quality;   // an attempt leaves the detector's adaptive threshold (state of the keyframe path) as it was
    int rc = detect(job.cell, 0, nullptr, cap, pts.data(), &n);
    m->max_quality = quality;
    if (rc) return rc;
    n = n > cap ? cap : n;
    out.n_detect = n;
    if (job.repack || !m->reloc_rows) {
        m->reloc_n_rows = 0;
        if (m->med && m->d_rec_tab && job.n_slots > 0) {
            if (job.n_slots > m->reloc_cap) {
                ALVA_HIP(alva_stream_sync(m->st));
                if (m->reloc_rows) ALVA_HIP(hipFree(m->reloc_rows));
                m->reloc_rows = nullptr;
                m->reloc_cap = 0;
                const int want = job.n_slots + job.n_slots / 2 + 256;
                ALVA_HIP(hipMalloc((void **) &m->reloc_rows, (size_t) want * 64));
                m->reloc_cap = want;
            }
            int count = 0;
            rc = alva_pack_map_records(m->med, (const void *const *) m->d_rec_tab, job.n_slots, 0, m->reloc_cap, m->reloc_rows, &count);
            if (rc) return rc;
            m->reloc_n_rows = count < m->reloc_cap ? count : m->reloc_cap;
        }
    }
    if (n <= 0 || m->reloc_n_rows <= 0) return ALVA_OK;
    StagePlan p;
    const size_t a = p.add((size_t) n * 8), b = p.add((size_t) n * 32), c = p.add((size_t) n), u = p.add((size_t) n * 8), v = p.add((size_t) n * 24),
                 mt = p.add((size_t) n * 16), cn = p.add(4), pb = p.add((size_t) n * 24), pu = p.add((size_t) n * 16), pw = p.add((size_t) n * 24);
    std::vector<uint8_t *> d, h;
    rc = m->carve(p, d, h);
    if (rc) return rc;
    memcpy(h[a], pts.data(), (size_t) n * 8);
    rc = alva_describe(m->ctx, m->d_gray, (size_t) k.width, k.width, k.height, (const float *) h[a], n, d[b], d[c]);
    if (rc) return rc;
    rc = alva_undistort_points(m->ctx, (const float *) h[a], n, k.fx, k.fy, k.cx, k.cy, k.k1, k.k2, k.p1, k.p2, (float *) d[u]);
    if (rc) return rc;
    hipLaunchKernelGGL(k_bearing, dim3(alva_divup(n, 256)), dim3(256), 0, m->st, (const float *) d[u], n, m->d_invK, (double *) d[v]);
    ALVA_LAUNCH_CHECK();
    rc = alva_reloc_match(m->ctx, d[b], d[c], n, (const double *) d[v], (const float *) d[u], m->reloc_rows, m->reloc_n_rows, job.max_dist, job.ratio,
                          (int *) d[mt], (int *) d[cn], (double *) d[pb], (double *) d[pu], (double *) d[pw]);
    if (rc) return rc;
    rc = m->down_span(p, d, h, b, cn);   // descriptors | validity | undistorted | bearings | matches | count: one copy, one wait
    if (rc) return rc;
    ALVA_HIP(alva_stream_sync(m->st));
    const int nm = *(const int *) h[cn];
    if (nm < 0 || nm > n) {
        alva_set_error("relocalize: match count %d of %d queries", nm, n);
        return ALVA_ERR_STATE;
    }
    out.n_match = nm;
    if (nm < 4 || nm < job.min_matches) return ALVA_OK;
    std::vector<uint8_t> p3p_out((size_t) nm), pnp_out((size_t) nm);
    int status = 0;
    double pose7[7] = {0, 0, 0, 0, 0, 0, 1};
    rc = m->pose().solve(m->ctx, (const double *) d[pb], (const double *) d[pu], (const double *) d[pw], nm, job.do_random, pose7, p3p_out.data(),
                         pnp_out.data(), &status);
    if (rc) return rc;
    out.status = status;
    if (status != 2) return ALVA_OK;
    memcpy(out.pose7, pose7, sizeof(pose7));
    const int *match = (const int *) h[mt];
    const uint8_t *desc = h[b];
    const float *unpx = (const float *) h[u];
    const double *bv = (const double *) h[v];
    for (int i = 0; i < nm; i++) {
        if (p3p_out[(size_t) i] || pnp_out[(size_t) i]) continue;
        const size_t q = (size_t) match[4 * i];
        out.px.insert(out.px.end(), &pts[2 * q], &pts[2 * q] + 2);
        out.unpx.insert(out.unpx.end(), unpx + 2 * q, unpx + 2 * q + 2);
        out.bv.insert(out.bv.end(), bv + 3 * q, bv + 3 * q + 3);
        out.desc.insert(out.desc.end(), desc + 32 * q, desc + 32 * q + 32);
        out.mp_id.push_back(match[4 * i + 2]);
    }
    out.n_inliers = (int) out.mp_id.size();
    return ALVA_OK;
}

int HipStages::medoid_dump(int mp_slot, alva_medoid::Table *out) {
    if (!m->med) return ALVA_ERR_STATE;
    return alva_medoid_dump(m->med, mp_slot, out, sizeof(*out));
}

int HipStages::find_plane(int n, const double *pts, const double *pose7_twc, int iterations, float *pose16, int *found) {
    *found = 0;
    if (n < 32) return ALVA_OK;  // system.cpp:181
    StagePlan p;
    const size_t a = p.add((size_t) n * 24);
    std::vector<uint8_t *> d, h;
    int rc = m->carve(p, d, h);
    if (rc) return rc;
    UP(m->st, a, pts, (size_t) n * 24);
    // the reference seeds a fresh generator from std::random_device in every iteration (system.cpp:210)
    return alva_find_plane(m->ctx, (const double *) d[a], n, pose7_twc, iterations, 1, 0u, nullptr, pose16, found);
}

HipStages::Frame HipStages::frame() const {
    return Frame{m->ctx, m->st, &m->cam, m->poll, &m->pyr[m->cur]->lv[0], m->frame_src, m->frame_src == m->d_rgba};
}

int HipStages::carve(StagePlan &p, std::vector<uint8_t *> &d, std::vector<uint8_t *> &h) { return m->carve(p, d, h); }

}  // namespace alva_slam
