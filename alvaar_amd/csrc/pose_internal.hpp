// Shared between p3p.hip and pnp.hip: device-side hand-off of the P3P-LMedS result to the PnP refinement
// (VisualFrontend::computePose chains them, src/slam/src/visual_frontend.cpp:245-417).
#pragma once
#include "common.hpp"
#include "pose_layout.hpp"   // the limits, the draw schedule and the memory blocks of the pose solve

struct P3pSelectOut {
    double model[12];  // R row-major (cam -> world) | t
    int best, n_valid_used, n_inliers, have_model;
};
static_assert(sizeof(P3pSelectOut) == 112 && sizeof(P3pSelectOut) <= POSE_REC_BYTES, "the selection record's slot");

// Enqueues the P3P-LMedS kernels on ctx->stream WITHOUT synchronising and without copy commands.
//   pin_samples : H*4 ints of PINNED host memory (alva_ctx_pinned); filled here, read by the hypothesis kernel over the bus
//   out/inlier  : where the selection result and the n-byte inlier mask are written: context scratch when another kernel
//                 consumes them (alva_compute_pose), pinned host memory when the host does (alva_p3p_lmeds)
int alva_p3p_enqueue(alva_ctx *ctx, const double *d_bearings, const double *d_wpts, int n, int max_iters, float err_threshold,
                     int do_random, uint32_t seed, float fx, float fy, int n_draws, int *pin_samples, P3pSelectOut *out,
                     uint8_t *inlier);

// the same in two steps (pnp.hip's fused P3P -> PnP launch takes the prepared arguments and launches them itself): samples drawn into
// pin_samples, scratch carved, *args filled | the launch alva_p3p_enqueue makes (lane deposit, or k_p3p_s / k_p3p on ctx->stream)
struct P3pArgs;
int alva_p3p_prepare(alva_ctx *ctx, const double *d_bearings, const double *d_wpts, int n, int max_iters, float err_threshold, int do_random,
                     uint32_t seed, float fx, float fy, int n_draws, int *pin_samples, P3pSelectOut *out, uint8_t *inlier, P3pArgs *args);
int alva_p3p_launch(alva_ctx *ctx, const P3pArgs &args);
int alva_p3p_raw_draws(int count, int do_random, uint32_t seed, int *h_raw);

// The fused tail of the single session's tracking frame (pnp.hip k_pose_all: compaction -> P3P -> PnP in one launch, queued right behind
// the tracker): enqueue | the host's answer once the tracker's early word gave it n (go: draws the samples; abort: the launch ends after
// its compaction phase).  Every enqueue MUST be answered by exactly one of the two; alva_compute_pose_collect_p3p collects a "go".
struct TrackSlots;
bool alva_pose_all_possible(int n_slots, int p3p_iters);
int alva_pose_all_enqueue(alva_ctx *ctx, const TrackSlots &D, int p3p_iters, float p3p_err, int do_random, uint32_t seed,
                          int pnp_iters, float chi2_th, float fx, float fy, float cx, float cy);
int alva_pose_all_go(alva_ctx *ctx, int n);
int alva_pose_all_abort(alva_ctx *ctx);

// alva_compute_pose_collect that also returns the accepted P3P pose (pnp.hip)
int alva_compute_pose_collect_p3p(alva_ctx *ctx, double *h_pose7, double *h_pose7_p3p, uint8_t *h_p3p_outlier, uint8_t *h_pnp_outlier,
                                  int *h_status);

// A batch of problems, one launch per stage for all of them (track_batch.hip; p3p.hip / pnp.hip define them).  An item is the kernel's
// argument block of one problem, filled into the caller's staging; scratch_bytes: the device scratch one problem needs, 64-byte granular
// (P3pScratch without masks | PnpScratch::BATCH).
size_t alva_p3p_batch_item_size();
size_t alva_p3p_batch_scratch_bytes(int H);
int alva_p3p_batch_item_fill(void *dst, const double *d_bearings, const double *d_wpts, int n, int max_iters, float err_threshold, float fx,
                             float fy, int H, const int *d_samples, uint8_t *d_scratch, int *d_counter, P3pSelectOut *d_out,
                             uint8_t *d_inlier);
int alva_p3p_batch_enqueue(alva_ctx *ctx, const void *d_items, int count, int H_max, int n_max);
size_t alva_pnp_batch_item_size();
size_t alva_pnp_out_size();
size_t alva_pnp_batch_scratch_bytes(int n);
int alva_pnp_batch_item_fill(void *dst, const double *d_uv, const double *d_wpts, int n, int pnp_iters, float chi2_th, float fx, float fy,
                             float cx, float cy, uint8_t *d_scratch, void *out, const P3pSelectOut *d_sel, const uint8_t *d_inlier0);
int alva_pnp_batch_enqueue(alva_ctx *ctx, const void *d_items, int count);
int alva_pnp_out_decode(const void *out, int p3p_iters, int H, int max_draws, double *h_pose7, int *h_status, int *needs_more_draws);

// The pose solve of a SESSION (the map layer's stages, the scene features, the step probe): the reference's constants and the camera's
// intrinsics as the kernels take them, said once.  frontend.hip and track_batch.hip get the intrinsics through their own ABI and take
// the constants from here.
struct SessionPose {
    static constexpr int p3p_iters = 100;      // multiViewRansacNumIterations_ (state.hpp:69)
    static constexpr float p3p_err = 3.0f;     // multiViewRansacError_, px (state.hpp:68)
    static constexpr uint32_t seed = 12345u;   // the sample generator's, unless multiViewRandomEnabled_ (state.hpp:67) asks for do_random
    static constexpr int pnp_iters = 5;        // maxIterations (visual_frontend.cpp:361, passed on at :363-375)
    static constexpr float chi2 = 5.9915f;     // robustCostThreshold_ (state.hpp:78); robust + L2 refinement (robustCostRefineWithL2_, :77)
    float fx, fy, cx, cy;
    SessionPose(double fx_, double fy_, double cx_, double cy_) : fx((float) fx_), fy((float) fy_), cx((float) cx_), cy((float) cy_) {}
    // the fused launch behind the tracker (to be answered: alva_pose_all_go / alva_pose_all_abort)
    int enqueue_fused(alva_ctx *ctx, const TrackSlots &D, int do_random) const {
        return alva_pose_all_enqueue(ctx, D, p3p_iters, p3p_err, do_random, seed, pnp_iters, chi2, fx, fy, cx, cy);
    }
    // the separate P3P -> PnP launches (collected by alva_compute_pose_collect_p3p)
    int enqueue(alva_ctx *ctx, const double *d_bv, const double *d_uv, const double *d_wpt, int n, int do_random) const {
        return alva_compute_pose_enqueue(ctx, d_bv, d_uv, d_wpt, n, p3p_iters, p3p_err, do_random, seed, pnp_iters, chi2, fx, fy, cx, cy);
    }
    int solve(alva_ctx *ctx, const double *d_bv, const double *d_uv, const double *d_wpt, int n, int do_random, double *h_pose7,
              uint8_t *h_p3p_outlier, uint8_t *h_pnp_outlier, int *h_status) const {
        return alva_compute_pose(ctx, d_bv, d_uv, d_wpt, n, p3p_iters, p3p_err, do_random, seed, pnp_iters, chi2, fx, fy, cx, cy, h_pose7,
                                 h_p3p_outlier, h_pnp_outlier, h_status);
    }
    // the two halves on their own
    int p3p(alva_ctx *ctx, const double *d_bv, const double *d_wpt, int n, int do_random, double *h_R, double *h_t, int *h_outliers,
            int *h_n_outliers, int *h_ok) const {
        return alva_p3p_lmeds(ctx, d_bv, d_wpt, n, p3p_iters, p3p_err, do_random, seed, fx, fy, h_R, h_t, h_outliers, h_n_outliers, h_ok);
    }
    int refine(alva_ctx *ctx, const double *d_uv, const double *d_wpt, int n, double *h_pose7, int *h_outliers, int *h_n_outliers,
               double *h_info, int *h_ok) const {
        return alva_pnp_refine(ctx, d_uv, d_wpt, n, h_pose7, pnp_iters, chi2, 1, 1, fx, fy, cx, cy, h_outliers, h_n_outliers, h_info, h_ok);
    }
};
