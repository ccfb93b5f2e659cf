/*
 * alvaar_hip.h -- C ABI of the MI355X (gfx950) hot path of AlvaAR's visual-SLAM
 * front-end and local bundle adjustment.
 *
 * This is the drop-in seam: each entry point replaces one L1 -> L0 call of the
 * reference (array in / array out, SURVEY.md §8(a), §8(b) "internal seam for
 * HIP").  Plain pointers and sizes only; no C++/torch types.  Pointers named
 * d_* are DEVICE pointers (HBM, on the context's device); h_* are host
 * pointers.  All work is enqueued on the context's HIP stream; functions that
 * return results through h_* pointers synchronise that stream before returning,
 * all others are asynchronous.
 *
 * Return value: ALVA_OK (0) or a negative ALVA_ERR_* code; alva_last_error()
 * gives a thread-local message.  There is NO CPU fallback anywhere behind this
 * header: if no gfx950 device is usable the calls fail.
 */
#ifndef ALVAAR_HIP_H
#define ALVAAR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    ALVA_OK = 0,
    ALVA_ERR_ARG = -1,   /* bad argument */
    ALVA_ERR_HIP = -2,   /* HIP runtime error (see alva_last_error) */
    ALVA_ERR_NOMEM = -3, /* allocation failed */
    ALVA_ERR_STATE = -4  /* object not in a usable state */
};

typedef struct alva_ctx alva_ctx;
typedef struct alva_pyramid alva_pyramid;

/* ---- context -------------------------------------------------------------------------------- */
/* own_stream != 0: the context creates and owns a non-blocking stream (hip_stream ignored).
 * own_stream == 0: enqueue on the caller's hipStream_t `hip_stream` as given -- NULL is the
 * legacy default stream (e.g. torch's current stream handle, which is 0 for the default stream). */
int alva_ctx_create(int device, void *hip_stream, int own_stream, alva_ctx **out);
/* Context with its own non-blocking stream in one of the device's priority classes: -1 high, 0 normal, +1 low.  The HIP runtime
 * multiplexes the streams of a class onto a few hardware queues (GPU_MAX_HW_QUEUES, default 4); streams sharing a queue run
 * strictly one after the other, so lanes that must overlap (alva_frontend's tracker / detector / look-ahead lanes) are
 * created in different classes. */
int alva_ctx_create_with_priority(int device, int priority_class, alva_ctx **out);
void alva_ctx_destroy(alva_ctx *ctx);
int alva_ctx_sync(alva_ctx *ctx);
/* Per-kernel timing for bench.py's roofline line: while enabled every kernel launch of the library is bracketed by two
 * HIP events on its own stream.  alva_prof_report waits for them and writes one line per kernel,
 * "name<TAB>launches<TAB>average microseconds", into buf.  (Measurement plumbing; no reference counterpart.) */
int alva_prof_enable(int on);
int alva_prof_report(char *buf, size_t cap);
/* Stream-order dependency without a host wait: work enqueued on `ctx` after this call starts only after everything
 * enqueued so far on `producer` has completed.  (The reference is single-threaded; this is what lets one frame run
 * detection and tracking+pose on two HIP streams.) */
int alva_ctx_wait(alva_ctx *ctx, alva_ctx *producer);
void *alva_ctx_stream(alva_ctx *ctx);
const char *alva_last_error(void);
const char *alva_version(void);

/* ---- a2: RGBA -> gray ------------------------------------------------------------------------
 * Replaces cv::cvtColor(image, image, COLOR_RGBA2GRAY) at src/slam/src/system.cpp:112
 * (Y = (9798 R + 19235 G + 3735 B + 16384) >> 15; imgproc/src/color_rgb.simd.hpp:646-664).
 * Pitches in bytes; rgba_pitch % 16 == 0, gray_pitch % 4 == 0, width % 4 == 0.
 *
 * Row pitches and alignment, for every call of this header that takes an image (anything else is ALVA_ERR_ARG before a launch):
 *   an RGBA frame (d_rgba)      pitch >= 4 * width, pitch % 16 == 0, the pointer 16-byte aligned (rows are read with 16-byte loads);
 *   a gray image with a "% 4"   pitch >= width, pitch % 4 == 0, the pointer 4-byte aligned: alva_rgba2gray's d_gray,
 *   rule                        alva_pyramid_build_from_gray's d_gray and the d_gray_out of the two RGBA pyramid builders;
 *   any other gray image        pitch >= width and nothing else -- any pointer, any pitch (read and written by bytes): alva_fast,
 *                               alva_orb_detect_and_compute(_batch), alva_orb_blur (input and output), alva_describe,
 *                               alva_detect_grid(_enqueue).
 * An image may be a view into a larger buffer: nothing outside width x height pixels of the rows is read or written. */
int alva_rgba2gray(alva_ctx *ctx, const uint8_t *d_rgba, size_t rgba_pitch, int width, int height,
                   uint8_t *d_gray, size_t gray_pitch);

/* ---- a3: LK pyramid with Scharr derivatives --------------------------------------------------
 * Replaces cv::buildOpticalFlowPyramid(img, pyr, Size(win,win), max_level) at
 * src/slam/src/visual_frontend.cpp:696 (video/src/lkpyramid.cpp:726-822; pyrDown
 * imgproc/src/pyramids.cpp:746-; ScharrDerivInvoker lkpyramid.cpp:70-151).
 * Every level is stored padded by `win` pixels on each side: gray REFLECT_101, derivatives
 * (interleaved int16 Ix,Iy) constant 0 -- the layout the LK tracker reads. */
typedef struct alva_pyr_level {
    int width, height;   /* interior size of this level */
    uint8_t *d_gray;     /* device pointer to interior pixel (0,0); valid for x,y in [-win, size+win) */
    size_t gray_pitch;   /* bytes */
    int16_t *d_deriv;    /* device pointer to interior element (0,0), 2 x int16 per pixel */
    size_t deriv_pitch;  /* bytes */
} alva_pyr_level;

/* width % 4 == 0, 3 <= win <= 15, 0 <= max_level <= 7, and width > win && height > win: a level 0 not larger than the window is
 * ALVA_ERR_ARG (its REFLECT_101 border would have to be reflected more than once; the stop rule below never produces such a level). */
int alva_pyramid_create(alva_ctx *ctx, int width, int height, int win, int max_level, alva_pyramid **out);
void alva_pyramid_destroy(alva_pyramid *pyr);
/* number of levels actually built (OpenCV stops when the next level would be <= win in either
 * dimension, lkpyramid.cpp:811-816) */
int alva_pyramid_num_levels(const alva_pyramid *pyr);
int alva_pyramid_level(const alva_pyramid *pyr, int level, alva_pyr_level *out);
/* d_gray: width x height of level 0, gray_pitch >= width, gray_pitch % 4 == 0, d_gray 4-byte aligned. */
int alva_pyramid_build_from_gray(alva_ctx *ctx, alva_pyramid *pyr, const uint8_t *d_gray, size_t gray_pitch);
/* Copies one padded level to host (synchronises): h_gray (h+2win) x (w+2win) u8 contiguous,
 * h_deriv same x 2 int16.  Either may be NULL. */
int alva_pyramid_download_level(alva_ctx *ctx, const alva_pyramid *pyr, int level, uint8_t *h_gray, int16_t *h_deriv);
/* fused a2+a3: level 0 is converted straight from the RGBA frame (also the entry of
 * System::findCameraPose, system.cpp:106-112).  d_gray_out may be NULL.
 * d_rgba: rgba_pitch >= 4 * width, rgba_pitch % 16 == 0, 16-byte aligned.  d_gray_out (un-padded, width x height): gray_out_pitch >=
 * width, gray_out_pitch % 4 == 0, 4-byte aligned; only its width x height pixels are written, whatever the pitch. */
int alva_pyramid_build_from_rgba(alva_ctx *ctx, alva_pyramid *pyr, const uint8_t *d_rgba, size_t rgba_pitch,
                                 uint8_t *d_gray_out, size_t gray_out_pitch);
/* The same for `count` cameras of one geometry in FIVE launches (one grid layer per camera) instead of 5 x count: one 640x480
 * frame is 1.2 MB and every launch above is bound by launch latency; many frames per launch is what lets the same kernels run at
 * HBM speed (bench.py "batched_preprocess").  Results are identical to `count` calls of alva_pyramid_build_from_rgba.
 * pyrs / d_rgba / d_gray_out (may be NULL) are HOST arrays of `count` handles / device pointers.  Enqueue only.
 * One rgba_pitch and one gray_out_pitch for all cameras, each under the single call's rule; every d_rgba[c] 16-byte and every
 * d_gray_out[c] 4-byte aligned; pyramids of another geometry than pyrs[0]'s are ALVA_ERR_ARG. */
int alva_pyramid_build_from_rgba_batch(alva_ctx *ctx, alva_pyramid *const *pyrs, const uint8_t *const *d_rgba, size_t rgba_pitch,
                                       uint8_t *const *d_gray_out, size_t gray_out_pitch, int count);

/* ---- a4: forward-backward pyramidal KLT ------------------------------------------------------
 * alva_lk_track replaces one cv::calcOpticalFlowPyrLK(prevPyr, nextPyr, pts, next, status, err,
 * Size(win,win), num_levels, {COUNT+EPS,max_iters,eps}, USE_INITIAL_FLOW|LK_GET_MIN_EIGENVALS)
 * (video/src/lkpyramid.cpp:183-724,1239-1404).  d_next is in/out (initial flow), d_status u8,
 * d_err = min eigenvalue (float).
 * alva_fbklt_track replaces FeatureTracker::fbKltTracking (src/slam/src/feature_tracker.cpp:5-111):
 * forward LK on num_levels, gate (status && err <= err_thresh && inBorder), backward LK on level 0
 * only, keep if |p - back| <= fb_dist.  d_prior in/out, d_status out (1 = tracked). */
int alva_lk_track(alva_ctx *ctx, const alva_pyramid *prev, const alva_pyramid *next, int num_levels,
                  int max_iters, float eps, const float *d_pts, float *d_next, uint8_t *d_status,
                  float *d_err, int n);
int alva_fbklt_track(alva_ctx *ctx, const alva_pyramid *prev, const alva_pyramid *curr, int num_levels,
                     float err_thresh, float fb_dist, int max_iters, float eps, const float *d_pts,
                     float *d_prior, uint8_t *d_status, int n);

/* ---- a6: 256-bit steered-BRIEF (ORB) description of given points ------------------------------
 * Replaces FeatureExtractor::describeFeaturePoints (src/slam/src/feature_extractor.cpp:160-214) =
 * cv::ORB::create(500,1.,0)->compute(): border-32 REFLECT_101 copy, 7x7 sigma=2 Gaussian
 * (features2d/src/orb.cpp:1188), 256 tests at round(R(angle) * pattern) with angle = -1 deg
 * (orb.cpp:219-284; core/src/types.cpp:93-101).  Points within 31 px of the image edge get
 * d_valid[i] = 0 and a zero descriptor (the reference returns an empty Mat for them).
 * d_desc: n x 32 bytes. */
int alva_describe(alva_ctx *ctx, const uint8_t *d_gray, size_t gray_pitch, int width, int height,
                  const float *d_pts, int n, uint8_t *d_desc, uint8_t *d_valid);
/* The 7x7 sigma-2 blur ORB samples from, of the image itself (REFLECT_101 at its edge; for stage-level parity tests):
 * d_out is height x width, rows out_pitch >= width apart; gray_pitch >= width.  Neither has an alignment rule. */
int alva_orb_blur(alva_ctx *ctx, const uint8_t *d_gray, size_t gray_pitch, int width, int height,
                  uint8_t *d_out, size_t out_pitch);

/* ---- a5': FAST-9/16 + NMS, and the full ORB detector -------------------------------------------
 * alva_fast replaces cv::FAST(img, kps, threshold, true, TYPE_9_16) (features2d/src/fast.cpp:56-292,
 * score fast_score.cpp:120-): keypoints are emitted in row-major order; d_xy int32 x,y pairs,
 * d_score int32.  *h_count receives the total found (may exceed cap; only cap are written).
 * gray_pitch >= width, no alignment rule (the image is read by bytes). */
int alva_fast(alva_ctx *ctx, const uint8_t *d_gray, size_t gray_pitch, int width, int height, int threshold,
              int *d_xy, int *d_score, int cap, int *h_count);

typedef struct alva_orb alva_orb;
/* Replaces cv::ORB::create(nfeatures, scale, nlevels, 31, 0, 2, HARRIS_SCORE, 31, fast_threshold)
 * ->detectAndCompute (features2d/src/orb.cpp:784-1218). */
int alva_orb_create(alva_ctx *ctx, int width, int height, int nfeatures, float scale_factor, int nlevels,
                    int fast_threshold, alva_orb **out);
void alva_orb_destroy(alva_orb *orb);
/* d_kp: cap x 6 floats {x, y, size, angle, response, octave}; d_desc: cap x 32 bytes (may be NULL for
 * detect-only).  Keypoint ORDER within a level is canonical (row-major by y then x) rather than
 * nth_element's unspecified order; the SET equals the reference's (SURVEY.md §8a a5').
 * Launch bound: candidates that tie exactly at a level's Harris cut are all kept (KeyPointsFilter::retainBest), so a level with a
 * budget of n_l keypoints (orb.cpp:799-813) can keep more than n_l.  The emit and descriptor launches are sized for
 * max(4 n_l + 64, 1024) keypoints per level; a level that keeps more (a periodic scene: every repeat of a corner has the same
 * response; a lattice of identical dots with nfeatures = 1 keeps every dot) makes this call, alva_orb_collect and
 * alva_orb_collect_batch return ALVA_ERR_STATE with a message naming the level and "above the launch bound".  The count is then
 * not returned and the output buffers hold no usable result; nothing is written past cap, and the detector object and the context
 * stay valid for the next image.  A level that keeps exactly the bound is returned in full.
 * d_gray: gray_pitch >= width (a smaller one is ALVA_ERR_ARG), no alignment rule for the pointer or the pitch: the image is read by
 * bytes, and by unaligned dwords that never pass the end of a row's width pixels. */
int alva_orb_detect_and_compute(alva_ctx *ctx, alva_orb *orb, const uint8_t *d_gray, size_t gray_pitch,
                                float *d_kp, uint8_t *d_desc, int cap, int *h_count);
/* h_count == NULL above only enqueues the work (no host wait); this call then waits for it and returns the count. */
int alva_orb_collect(alva_ctx *ctx, alva_orb *orb, int *h_count);
/* cv::ORB::detectAndCompute of `count` cameras in one set of launches: every camera has its own detector object (all of one geometry:
 * image size, nfeatures, scale, nlevels), gray image (non-NULL, rows gray_pitch >= width apart), keypoint and descriptor buffer (both
 * non-NULL, each of capacity cap >= 0); each camera's output equals its own alva_orb_detect_and_compute.  A camera that finds more
 * than cap keypoints gets the first cap records and descriptors of its (octave, y, x) order; rows from cap on are not written (cap = 0
 * writes nothing).  Enqueue-only; alva_orb_collect_batch waits and returns per camera the number of keypoints FOUND, which may
 * therefore exceed cap (as *h_count of alva_orb_detect_and_compute may): the caller clamps it to cap before reading the buffers. */
int alva_orb_detect_and_compute_batch(alva_ctx *ctx, alva_orb *const *orbs, int count, const uint8_t *const *d_gray,
                                      size_t gray_pitch, float *const *d_kp, uint8_t *const *d_desc, int cap);
int alva_orb_collect_batch(alva_ctx *ctx, alva_orb *const *orbs, int count, int *h_counts);
/* Number of keypoints (since the last reset) whose rBRIEF rotation (float) cos / sin could not be PROVEN to round like the host C
 * library's (features2d/src/orb.cpp:230-232): the kernel decides the two floats from a ~100-bit evaluation and only a true value
 * within 2^-50 of a float rounding boundary is left unproven (probability ~3e-8 per keypoint).  Synchronous. */
int alva_orb_ambiguous_rotations(int *h_count, int reset);
/* One level of the detector's pyramid as the last run left it (which = 0: orb.cpp:1086-1099's resize chain; which = 1: its 7x7 sigma-2
 * blur, orb.cpp:1188) copied to d_out (w x h bytes, rows out_pitch apart; d_out NULL only returns the size).  For stage-level parity tests.
 * ALVA_ORB_PYRAMID=chain (read at alva_orb_create) builds the pyramid with one resize launch per level instead of the fused launch. */
int alva_orb_debug_level(alva_ctx *ctx, alva_orb *orb, int level, int which, uint8_t *d_out, size_t out_pitch, int *w, int *h);
/* device-resident keypoint count of the detector's last run (what alva_orb_collect copies to the host) */
const int *alva_orb_device_count(const alva_orb *orb);

/* ---- a5: the reference's grid Shi-Tomasi detector ---------------------------------------------
 * Replaces FeatureExtractor::detectFeaturePoints (src/slam/src/feature_extractor.cpp:11-158).
 * h_max_quality is the detector's adaptive threshold, in/out (stateful across calls, :138-145).
 * d_occupied: n_occ x 2 floats (already-tracked keypoints).  d_out_pts: cap x 2 floats,
 * sub-pixel refined (cornerSubPix win 3, 30 it, eps 0.01).  *h_count = number of points.
 * d_gray: gray_pitch >= width (a smaller one is ALVA_ERR_ARG), no alignment rule (read by bytes); the same for _enqueue. */
int alva_detect_grid(alva_ctx *ctx, const uint8_t *d_gray, size_t gray_pitch, int width, int height,
                     int cell_size, const float *d_occupied, int n_occ, int roi_x, int roi_y, int roi_w,
                     int roi_h, double *h_max_quality, float *d_out_pts, int cap, int *h_count);
/* The same call split at its only host wait: _enqueue launches the detection on the context's stream with the threshold `max_quality`
 * and returns at once; _collect waits, reports the count and applies the adaptive-threshold rule (:138-145) to *h_max_quality.  The
 * caller does host work in between (the map layer updates its descriptor medoids while the detector runs).  No other call on the
 * context between the two. */
typedef struct alva_detect_pending {
    void *h_cnt;
    int n_cells;
    int reserved;
} alva_detect_pending;
int alva_detect_grid_enqueue(alva_ctx *ctx, const uint8_t *d_gray, size_t gray_pitch, int width, int height, int cell_size,
                             const float *d_occupied, int n_occ, int roi_x, int roi_y, int roi_w, int roi_h, double max_quality,
                             float *d_out_pts, int cap, alva_detect_pending *pending);
int alva_detect_grid_collect(alva_ctx *ctx, const alva_detect_pending *pending, double *h_max_quality, int *h_count);
/* The lambda_min plane of the context's last detection copied to d_out: n_cells x cell_size^2 floats, cell after cell in row-major cell
 * order, as the detector left it (the cells of that call which were occupied or fail x0 + cell < w - 1 hold nothing of it).  n_cells and
 * cell_size are those of that call.  For stage-level parity tests.  Synchronous. */
int alva_detect_grid_debug_eig(alva_ctx *ctx, int n_cells, int cell_size, float *d_out);

/* ---- a7: Hamming brute-force matcher ----------------------------------------------------------
 * Replaces cv::BFMatcher(NORM_HAMMING).match(query, train) (core/src/batch_distance.cpp:199-251,
 * norm.cpp:99-): per query the smallest distance, LOWEST train index on ties.
 * Descriptors are 32 bytes each, rows 32-byte aligned. */
int alva_bf_match_hamming(alva_ctx *ctx, const uint8_t *d_query, int n_query, const uint8_t *d_train,
                          int n_train, int *d_idx, int *d_dist);
/* `count` independent matches in one pair of launches.  Match c: queries d_query[c], whose number is read from device memory
 * (*d_n_query[c], clamped to cap_query) so that the call can be enqueued behind the detector that produces them; train set
 * d_train[c] with n_train[c] rows (0 = skip that match); rows of d_idx[c] / d_dist[c] beyond the query count stay untouched.
 * expected_queries sizes the grid (larger counts are covered by a loop).  Enqueue-only. */
int alva_bf_match_hamming_batch(alva_ctx *ctx, int count, const uint8_t *const *d_query, const int *const *d_n_query,
                                int cap_query, const uint8_t *const *d_train, const int *n_train, int *const *d_idx,
                                int *const *d_dist, int expected_queries);

/* ---- a8: P3P + LMedS absolute pose ------------------------------------------------------------
 * Replaces MultiViewGeometry::p3pRansac(obs, wpts, max_iters, err_thr, optimize=false, doRandom,
 * fx, fy, Twc, outliers) (src/slam/src/multi_view_geometry.cpp:24-127) = opengv::sac::Lmeds<
 * AbsolutePoseSacProblem(KNEIP)> (opengv/sac/implementation/Lmeds.hpp:43-195).
 * Sampling runs on the host with the reference's own sampler classes (std::mt19937 +
 * std::uniform_int_distribution, prefix Fisher-Yates; SampleConsensusProblem.hpp:40-120): do_random = 0
 * seeds with `seed` (the reference's fixed seed is 12345u), do_random != 0 seeds from the clock like
 * the reference's default.  alva_p3p_draw_samples exposes that index stream (count x 4 int32).
 * Outputs (host): R row-major 3x3 + t (Twc), outlier index list (capacity n); *h_ok = 1 on success
 * (>= 5 inliers and an orthogonal R, multi_view_geometry.cpp:82-91).  n <= 19000 (the LMedS median is LDS-resident). */
int alva_p3p_draw_samples(int n_points, int count, int do_random, uint32_t seed, int *h_samples);
int alva_p3p_lmeds(alva_ctx *ctx, const double *d_bearings, const double *d_wpts, int n, int max_iters,
                   float err_threshold, int do_random, uint32_t seed, float fx, float fy, double *h_R,
                   double *h_t, int *h_outliers, int *h_n_outliers, int *h_ok);
/* The hypothesis stage made visible (the instrument of tests/test_gpu_p3p_hypotheses.py; alva_relpose_hypotheses is its
 * two-view counterpart): `count` problems with CALLER-SUPPLIED samples go through the production launches and everything the
 * selection decides on comes back, per hypothesis.
 *   route 0: one problem after the other through the single-problem launch of alva_p3p_lmeds (samples in the kernel arguments
 *            up to H = 192, in pinned host memory above; the raised dynamic-LDS limit above n = 7168)
 *   route 1: all problems in ONE batch (the three launches of the batched tracker), n <= 7168
 * In: device bearings / world points (n x 3 doubles), host samples (H x 4 indices < n), max_iters = the cap on VALID hypotheses
 * the selection may use.  Out (host, caller-allocated): h_models[H x 12] (R row-major | t), h_valid[H], h_penalty[H] (the LMedS
 * median; +inf where the sample has no model, whose model row and mask are zero), h_masks[H x ceil(n / 64)] 64-bit words, bit i of
 * row h = point i is an inlier of hypothesis h (route 0 only: the batch keeps no masks, the pointer may be NULL there),
 * h_inlier[n] and the selection record: best (-1: none), n_valid_used, n_inliers, have_model, model[12].  counter_after is the
 * selection's arrival counter as the launch left it (0 unless something is wrong).  Synchronous. */
typedef struct alva_p3p_hyp_problem {
    const double *d_bearings, *d_wpts;
    const int *h_samples;
    int n, H, max_iters;
    double *h_models;
    int *h_valid;
    double *h_penalty;
    unsigned long long *h_masks;
    uint8_t *h_inlier;
    int best, n_valid_used, n_inliers, have_model, counter_after;
    double model[12];
} alva_p3p_hyp_problem;
int alva_p3p_hypotheses(alva_ctx *ctx, alva_p3p_hyp_problem *problems, int count, float err_threshold, float fx, float fy,
                        int route);

/* ---- a9: robust PnP refinement (motion-only BA) -----------------------------------------------
 * Replaces MultiViewGeometry::ceresPnP (src/slam/src/multi_view_geometry.cpp:129-223): Huber LM on
 * the 6-DoF pose (Ceres trust_region_minimizer.cc / levenberg_marquardt_strategy.cc semantics,
 * wall-clock cap removed), chi2 outlier sweep, optional L2 re-solve.
 * h_pose7 = [tx,ty,tz,qx,qy,qz,qw] (Twc) in/out.  h_info[8]: iterations/cost of both solves. */
int alva_pnp_refine(alva_ctx *ctx, const double *d_uv, const double *d_wpts, int n, double *h_pose7,
                    int max_iters, float chi2_th, int use_robust, int apply_l2_after_robust, float fx,
                    float fy, float cx, float cy, int *h_outliers, int *h_n_outliers, double *h_info,
                    int *h_ok);

/* ---- a8 + a9 chained: VisualFrontend::computePose (src/slam/src/visual_frontend.cpp:245-417) -----------------
 * P3P-LMedS, its acceptance tests, removal of its outliers and the robust PnP refinement of the inliers run as one
 * device-side chain with ONE host synchronisation.  d_uv are the undistorted pixel observations of the same n points.
 * Outputs: h_pose7 (written when *h_status >= 1 and PnP produced a pose), per-point masks in the caller's
 * indexing (either may be NULL), *h_status: 0 = P3P rejected (the reference resets the frame), 1 = P3P pose accepted
 * but the refinement failed its checks (:383-399), 2 = refined pose accepted. */
int alva_compute_pose(alva_ctx *ctx, const double *d_bearings, const double *d_uv, const double *d_wpts, int n,
                      int p3p_iters, float p3p_err, int do_random, uint32_t seed, int pnp_iters, float chi2_th,
                      float fx, float fy, float cx, float cy, double *h_pose7, uint8_t *h_p3p_outlier,
                      uint8_t *h_pnp_outlier, int *h_status);
/* The same in two halves: _enqueue launches the chain without waiting, _collect waits and returns the results.  No other
 * call may be made on `ctx` in between (other contexts / streams are free to run: that is the point).  _collect waits on a completion
 * word the last kernel publishes in pinned host memory after all results (ALVA_NO_POLL=1: on the stream instead); later calls on `ctx`
 * are stream-ordered behind the chain either way. */
int alva_compute_pose_enqueue(alva_ctx *ctx, const double *d_bearings, const double *d_uv, const double *d_wpts, int n,
                              int p3p_iters, float p3p_err, int do_random, uint32_t seed, int pnp_iters, float chi2_th,
                              float fx, float fy, float cx, float cy);
int alva_compute_pose_collect(alva_ctx *ctx, double *h_pose7, uint8_t *h_p3p_outlier, uint8_t *h_pnp_outlier,
                              int *h_status);

/* ---- f2b: two-view map initialisation ----------------------------------------------------------------
 * Replaces MultiViewGeometry::compute5ptEssentialMatrix(bvs1, bvs2, maxIterations, errorThreshold, optimize, doRandom, fx, fy,
 * Rwc, twc, outliers) (src/slam/src/multi_view_geometry.cpp:225-320; caller VisualFrontend::checkReadyForInit,
 * visual_frontend.cpp:517-528 with state.hpp:67-69: 100 iterations, 3 px, optimize = true): OpenGV RANSAC (99 % confidence,
 * adaptive iteration count) over Nister's five-point solver with 8-index samples, then Levenberg-Marquardt refinement of
 * (t, Cayley(R)) on the inliers.  d_bv1 / d_bv2: n x 3 unit bearings in the previous keyframe / the current frame (device);
 * the model is X1 = R X2 + t.  Outputs (host): h_R (3 x 3 row-major), h_t (as the reference, NOT normalised), h_inlier[n]
 * (1 = inlier; the reference's outlier list is its complement; may be NULL), *h_ok = the reference's return value
 * (0: n < 8, no model, or fewer than 10 inliers).  do_random = 0 draws the reference's deterministic sample stream
 * (std::mt19937 seeded 12345u when seed = 12345).  Synchronous.
 * The refinement is a forward-difference optimiser working at its rounding-noise floor: the reference's own result moves by
 * 1e-6 .. 1e-4 when one input changes by one ulp, and agreement with it is of that size. */
typedef struct alva_relpose_info {
    int iterations;      /* RANSAC iterations the reference would have run (Ransac::iterations_) */
    int n_inliers;
    int draws;           /* samples consumed (iterations + samples without a real root) */
    int lm_iterations, lm_status, lm_nfev; /* Eigen::LevenbergMarquardt iter / status code / function evaluations */
    double ransac_model[12]; /* R (row-major) | t before the refinement */
} alva_relpose_info;
int alva_compute_5pt_essential(alva_ctx *ctx, const double *d_bv1, const double *d_bv2, int n, int max_iters,
                               float error_threshold, int optimize, int do_random, uint32_t seed, float fx, float fy,
                               double *h_R, double *h_t, uint8_t *h_inlier, alva_relpose_info *h_info, int *h_ok);
/* The sample stream (count x 8 int32, SampleConsensusProblem.hpp:65-84) and the hypothesis stage alone: one
 * CentralRelativePoseSacProblem::computeModelCoefficients (CentralRelativePoseSacProblem.cpp:38-247) + countWithinDistance per
 * sample; h_counts[k] = -1 when sample k has no model. */
int alva_relpose_draw_samples(int n_points, int count, int do_random, uint32_t seed, int *h_samples8);
int alva_relpose_hypotheses(alva_ctx *ctx, const double *d_bv1, const double *d_bv2, int n, const int *h_samples8, int n_samples,
                            float error_threshold, float fx, float fy, double *h_models12, int *h_counts);

/* ---- f3: plane under the map points -------------------------------------------------------------------
 * The INTENDED algorithm of System::processPlane(mapPoints, Twc, numIterations) (src/slam/src/system.cpp:177-342, caller
 * findPlane :123-137): RANSAC over planes through 3 sampled points (orientation test, k-th smallest distance as the score),
 * inliers within 1.4 x the best score, least-squares refit, pose = [Rodrigues(...) Rodrigues((1,0,0)) | mean of the inliers]
 * in the layout of Utils::toPoseArray(cv::Mat).  As shipped the reference function has no defined behaviour;
 * parity is pinned against the reference's own function compiled with its four defects repaired (oracle/ref_shim_plane.cpp) and
 * against the CPU restatement oracle/alva_oracle_plane.c, which is pinned to the same (tests/test_plane.py).
 * d_points: n x 3 world points (device, f64); h_pose7_twc: current pose; h_samples3 (num_iterations x 3 int32, may be NULL):
 * the sample indices, otherwise drawn from std::mt19937(seed) (clock-seeded when do_random).  *h_found = 0 when n < 32 or
 * fewer than 32 inliers.  n <= 12288; every index of h_samples3 must lie in [0, n) (ALVA_ERR_ARG otherwise, before anything is
 * launched; the context stays usable); an index may repeat within a triple (the iteration is then skipped).  Synchronous.
 * Everything up to and including the inlier set is a fixed sequence of single-rounded float and double operations, pinned bit for
 * bit by the numpy restatement tests/findplane_cases.py; the refit's sums and the eigenvector are toleranced there. */
int alva_find_plane(alva_ctx *ctx, const double *d_points, int n, const double *h_pose7_twc, int num_iterations, int do_random,
                    uint32_t seed, const int *h_samples3, float *h_plane_pose16, int *h_found);
/* alva_find_plane -- the same two launches, the same arithmetic, the same bits in h_plane_pose16 and *h_found -- with its
 * intermediate results.  Each of the following may be NULL; for tests:
 *   h_scores[num_iterations]      the score of every iteration (the k-th smallest distance), +inf where the iteration was skipped
 *                                 (collinear or repeated sample, or the orientation test)
 *   h_planes4[num_iterations][4]  its plane (a, b, c, d), the unit 4-vector; meaningful only where the score is finite (zero
 *                                 elsewhere when h_scores is given too)
 *   h_inlier[n]                   uint8, 1 where the point's distance to the winning plane is < 1.4f x the best score (every point
 *                                 when no iteration survived)
 *   h_info4                       {best iteration (-1: none survived), n_inliers, k = max((int)(0.2 n), 20), 0}
 *   h_best_score                  the winning score (1e10f when none survived)
 *   h_moments13                   over the inliers, of the float-cast coordinates as doubles: the upper triangle of the sum of
 *                                 [x y z 1]^T [x y z 1], row by row (10), then the sums of x, y, z (3)
 * When nothing is launched (n < 32) or an argument is rejected after the first check: scores +inf, planes, flags and moments 0,
 * info {-1, 0, k, 0}, best score 1e10f. */
int alva_find_plane_trace(alva_ctx *ctx, const double *d_points, int n, const double *h_pose7_twc, int num_iterations, int do_random,
                          uint32_t seed, const int *h_samples3, float *h_plane_pose16, int *h_found, float *h_scores, float *h_planes4,
                          uint8_t *h_inlier, int *h_info4, float *h_best_score, double *h_moments13);

/* ---- hit test: the anchor pose on the surface under an image point ------------------------------------------------------
 * The hit test of WebXR / ARCore; no reference counterpart (parity is pinned by the numpy restatement tests/hit_cases.py).
 * d_points: n x 3 world points (device, f64); h_pose7_twc: camera pose (t, q = x y z w); h_calib8: fx fy cx cy k1 k2 p1 p2;
 * h_uv: n_rays taps in RAW image pixels.  All arithmetic is IEEE double in the written order; one launch for all rays.  Per ray:
 *   ray         (uu, vv) = undistorted tap (CameraCalibration::undistortImagePoint, float), dc = ((uu - cx) / fx, (vv - cy) / fy, 1),
 *               dw = R_wc dc / |dc|
 *   selection   Pc = R_wc^T (P_i - t); selected iff Pc.z > 0 and (fx Pc.x / Pc.z + cx - uu)^2 + (fy Pc.y / Pc.z + cy - vv)^2 <=
 *               radius_px^2; kept in ascending index order, at most the first 2048; m = kept count; m < 24: code 1
 *   hypotheses  it = 0 .. num_iterations - 1: words w_j = h(seed ^ ((3 it + j) * 0x9E3779B9)), j = 0 1 2 (or h_rand3[it][j]) with
 *               h(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16 (uint32); index i_j = (w_j * m) >> 32
 *               (64-bit product); skipped when two indices coincide or |(Q1 - Q0) x (Q2 - Q0)| is not > 0; n = that cross product,
 *               normalised; score = the element of rank m / 2 (0-based) among |(Q_i - Q0) . n| over the m selected points (LMedS:
 *               scale-free, as a monocular map needs); the smallest score wins, the lowest `it` on ties; none survived: code 2
 *   inliers     |(Q_i - Q0) . n| <= 3.7065 * score (2.5 x 1.4826; <= keeps the points of an exact plane); fewer than 16: code 3
 *   refit       centroid c and covariance of the inliers, n = eigenvector of the smallest eigenvalue, flipped to face the camera
 *               (n . (t - c) > 0)
 *   hit         den = n . dw; |den| < 0.0872 (under 5 deg from grazing) or lambda = n . (c - t) / den <= 0: code 4; p = t + lambda dw
 *   pose        y = n, x = normalize(a - (a . n) n) with a = R_wc[:,0] (R_wc[:,1] when that norm is < 1e-6), z = x cross y;
 *               h_pose16 in alva_find_plane's layout: out[4 c + r] = Rot[r][c], out[12..14] = p, out[15] = 1
 * h_info8 per ray: {code, m, best_it (-1: none), n_in, selected before the cap, 0, 0, 0}; code 0 = found, and only then is the
 * ray's pose written.  h_moments (may be NULL; for tests) per ray: n_in as a double, the sum of x (3) and the upper triangle of the
 * sum of x x^T (6) over the inliers with x = Q_i - Q0 of the winning hypothesis.  The plane is UNBOUNDED: a hit may lie on a plane's
 * extension beyond the points that support it.  n_rays 1..16, num_iterations 1..4096, radius_px > 0; n = 0 is legal (code 1 for
 * every ray, nothing is launched).  A given map, pose and seed give the same bits on every call.  Synchronous. */
int alva_hit_test(alva_ctx *ctx, const double *d_points, int n, const double *h_pose7_twc, const double *h_calib8, int n_rays,
                  const float *h_uv, float radius_px, int num_iterations, uint32_t seed, const uint32_t *h_rand3, float *h_pose16,
                  int *h_info8, double *h_moments);

/* ---- plane detection: the planes among a set of points, bounded and oriented, several per call ---------------------------
 * ARCore Plane / ARKit ARPlaneAnchor / WebXR plane detection; no reference counterpart (parity is pinned by the numpy restatement
 * tests/plane_cases.py).  Sequential multi-plane RANSAC with removal.  d_points: n x 3 world points (device, f64), n 0..16384;
 * h_pose7_twc: camera pose (t, q = x y z w), used only to orient the result; thickness > 0, finite: half the slab's width, in map
 * units.  All arithmetic is IEEE double in the written order.  Every point starts with label -1.  Rounds r = 0 .. max_planes - 1; the
 * live list L_r is the points still labelled -1, in ascending index, m = |L_r|:
 *   1 too few     m < min_inliers: stop, code 1
 *   2 hypotheses  it = 0 .. num_iterations - 1: words w_j = h(seed ^ ((3 (r * num_iterations + it) + j) * 0x9E3779B9)), j = 0 1 2, uint32
 *                 arithmetic, h as for alva_hit_test (or h_rand3[r * num_iterations + it][j]); index i_j = (w_j * m) >> 32 (64-bit
 *                 product) INTO THE LIVE LIST, Q_j = L_r[i_j]; skipped when two indices coincide or |(Q1 - Q0) x (Q2 - Q0)| is not > 0;
 *                 nh = that cross product, normalised; count = #{i in L_r : |(P_i - Q0) . nh| <= thickness}, the dot product
 *                 associated (dx nx + dy ny) + dz nz as everywhere below
 *   3 winner      the largest count, the lowest `it` on ties; none survived: stop, code 2; count < min_inliers: stop, code 3
 *   4 refit       over the winner's consensus set (the points counted), in live order, the ten sums of x = P_i - Q0: the count, the
 *                 sum of x (3), the upper triangle of the sum of x x^T (6); mu = sum x / count, covariance S_ab = sum x_a x_b / count -
 *                 mu_a mu_b, centroid c = Q0 + mu; nrm = the unit eigenvector of S's smallest eigenvalue, negated unless
 *                 nrm . (t - c) > 0 (it faces the camera)
 *   5 final set   F = {i in L_r : |(P_i - c) . nrm| <= thickness}, n_in = |F|; n_in < min_inliers: stop, code 4, nothing is labelled
 *                 in this round; otherwise the points of F get label r and leave the live list
 *   6 extent      x = the eigenvector of the LARGEST eigenvalue of the same covariance S (step 4's; F's own is not computed), minus its
 *                 component along nrm, normalised, negated when x . a < 0 with a = R_wc[:,0] -- or a = R_wc[:,1] when
 *                 |R_wc[:,0] . nrm| > 0.9: a plane that faces along the camera's x axis has every in-plane direction perpendicular
 *                 to it, and noise would pick the sign (as alva_hit_test falls back to R_wc[:,1]); z = x cross nrm; lo_x, hi_x, lo_z, hi_z =
 *                 min / max over F of (P_i - c) . x and (P_i - c) . z; centre p = c + ((lo_x + hi_x) / 2) x + ((lo_z + hi_z) / 2) z
 *   7 record      h_planes24[r]: a pose16 in alva_find_plane's layout (out[4 c + r] = Rot[r][c]) with the columns x, nrm, z and the
 *                 translation p, out[15] = 1; then extent_x = hi_x - lo_x, extent_z = hi_z - lo_z, the plane's offset nrm . p, five zeros
 * h_info8[r] = {code, m, best_it (-1: none), the winner's count, n_in, 0, 0, 0}; code 0 = found.  The round that stops writes its code;
 * every later round's info is {5, 0, -1, 0, 0, 0, 0, 0} (not run).  A plane record is written only for code 0, the rest stays zero.
 * d_labels (device int32[n], may be NULL): the plane index of every point, or -1.  h_rand3 ([max_planes * num_iterations][3] words, may
 * be NULL; for tests) replaces the hashed words.  h_moments ([max_planes][10], may be NULL; for tests): step 4's ten sums of the rounds
 * that reached it with a large enough count (codes 0 and 4).  min_inliers 8..16384, max_planes 1..8, num_iterations 1..4096; n = 0 is
 * legal (round 0 stops with code 1, nothing is launched).  Returns the number of planes found (>= 0) or a negative error; after
 * ALVA_ERR_ARG the context stays usable.  One launch per round, queued back to back; the 3 x 3 eigen-solve runs on the device (cyclic
 * Jacobi, 12 sweeps); the host waits once.  The same points, pose and seed give the same bits on every call.  Synchronous. */
int alva_detect_planes(alva_ctx *ctx, const double *d_points, int n, const double *h_pose7_twc, double thickness, int min_inliers,
                       int max_planes, int num_iterations, uint32_t seed, const uint32_t *h_rand3, float *h_planes24, int *h_info8,
                       int *d_labels, double *h_moments);

/* ---- plane tracking: the planes of an earlier call kept in their slots, refitted, grown; new planes among the rest ----------
 * ARCore Plane trackables / ARKit ARPlaneAnchor updates / the WebXR XRPlane set; no reference counterpart (parity is pinned by the numpy
 * restatement tests/track_cases.py).  The arguments, their bounds and the arithmetic (IEEE double in the written order, the dot product
 * associated (dx nx + dy ny) + dz nz) are alva_detect_planes'; in addition h_prior24: n_prior records of an earlier call
 * (alva_detect_planes' or this function's layout), 0 <= n_prior <= max_planes, non-null when n_prior > 0.  Prior j keeps slot j:
 *   T0 priors     n_j = (double) rec[4..6], c_j = (double) rec[12..14], as handed in, not renormalised.  A prior with a non-finite number
 *                 among its 24, or with rec[15] != 1, is unusable: code 9, it claims nothing
 *   T1 claim      d_ij = ((P_i - c_j)_x n_x + (P_i - c_j)_y n_y) + (P_i - c_j)_z n_z; point i is claimed by the usable prior with the
 *                 smallest |d_ij| among those with |d_ij| <= thickness, the lowest j on ties; otherwise it is unclaimed
 *   T2 too few    claimed_j < min_inliers: code 7 (lost)
 *   T3 refit      the ten sums of x = P_i - c_j over prior j's claimed set (the count, the sum of x, the upper triangle of the sum of
 *                 x x^T); centroid mu, covariance, nrm'_j = the unit eigenvector of the smallest eigenvalue, negated unless it faces the
 *                 camera -- exactly alva_detect_planes' step 4 with Q0 = c_j; c'_j = c_j + mu.  (No code of its own: every prior that
 *                 passed T2 passes T3)
 *   T4 settle     T1 again, against the refitted planes (c'_j, nrm'_j) of the priors that passed T2, and only those;
 *                 inliers_j < min_inliers: code 8, and the points it claimed end up unclaimed (they are not offered to another plane)
 *   T5 record     a kept prior gets a record as in alva_detect_planes' steps 6 and 7 over its T4 set: the long axis from T3's covariance,
 *                 the same sign rule with the 0.9 switch, centre = the rectangle's, extents and offset alike
 *   T6 new planes the points unclaimed after T4, in ascending index, are the live list of max_planes - n_prior rounds: exactly
 *                 alva_detect_planes' steps 1 to 7 on that list with the same seed, the round index r in the sample hash counting
 *                 from 0 (h_rand3: [(max_planes - n_prior) * num_iterations][3], rows from 0); round r writes slot n_prior + r and the
 *                 label n_prior + r
 * d_labels[i]: the slot, or -1.  h_info8[slot] = {code, n (tracked slot) or the round's live count (new), -1 or the winning iteration,
 * claimed_j or the winner's count, inliers, origin (1: tracked, 0: new), 0, 0}; a new slot's info is alva_detect_planes' (codes 0 .. 5).
 * A record is written only for code 0.  h_moments (may be NULL; for tests): T3's sums for tracked slots with codes 0 and 8, step 4's for
 * new slots with codes 0 and 4.  n = 0 launches nothing: usable priors get code 7 (unusable ones 9) with n = 0, the first new slot code 1.
 * With n_prior = 0 every output byte equals alva_detect_planes' for the same arguments.  Returns the number of code-0 slots, or a
 * negative error; after ALVA_ERR_ARG the context stays usable.  One claim-and-settle launch (skipped when n_prior = 0; one workgroup for
 * one prior, from two priors on one workgroup per prior and the last to arrive settles -- the same bits either way), then one launch
 * per round, queued back to back; the host waits once.  The same points, pose, priors and seed give the same bits on
 * every call.  Synchronous. */
int alva_track_planes(alva_ctx *ctx, const double *d_points, int n, const double *h_pose7_twc, double thickness, int min_inliers,
                      int max_planes, int num_iterations, uint32_t seed, const uint32_t *h_rand3, int n_prior, const float *h_prior24,
                      float *h_planes24, int *h_info8, int *d_labels, double *h_moments);

/* ---- plane outlines: the convex boundary polygon of each detected plane ---------------------------------------------------
 * ARCore Plane.getPolygon / ARKit ARPlaneGeometry / WebXR XRPlane.polygon; no reference counterpart (parity is pinned by the numpy
 * restatement tests/outline_cases.py).  The outline is a SET FUNCTION of the plane's points with EXACT predicates: any correct
 * algorithm gives the same bits, and the order of the points does not matter.  d_points: n x 3 world points (device, f64), n 0..16384;
 * d_labels: the plane index of every point (device, int32[n]; alva_detect_planes' labels).  For plane k of n_planes (1..8) the frame is
 * the record rec = h_planes24[k] (alva_detect_planes' layout), its floats cast to double: x = rec[0..2], z = rec[8..10],
 * p = rec[12..14], s = max(rec[16], rec[17]):
 *   frame     rec[15] != 1: code 5 (no plane record: the detection's code was not 0); s not finite or not > 0 (a NaN extent makes s NaN),
 *             or one of the nine numbers of x, z, p not finite: code 4
 *   grid      inv = 1048576.0 / s, cell = s / 1048576.0 (host, double: the device divides nothing that decides)
 *   points    every i in 0 .. n - 1 with d_labels[i] == k (labels < 0 or >= n_planes belong to no plane): d = P_i - p,
 *             u = (d.x x0 + d.y x1) + d.z x2, v likewise with z, IEEE double in the written order;
 *             qu = clamp(rint(u * inv), -2^21, 2^21) as int32 (rint rounds half to even), qv likewise: every cross product of
 *             differences stays below 2^45, so int64 is exact.  Fewer than 3 such points: code 1
 *   hull      the vertices of the convex hull of the set of distinct (qu, qv); strictly convex vertices only (a grid point on an edge
 *             is no vertex); ordered so that consecutive vertices a, b, c satisfy cross(b - a, c - b) > 0 (counter-clockwise in (u, v));
 *             the first one is the lexicographically smallest (qu, qv).  No area (one grid point, or all collinear): code 2; more than
 *             max_vertices vertices: code 3
 *   area      A2 = sum over the vertices of qu_i qv_(i+1) - qu_(i+1) qv_i (int64, > 0); h_area[k] = (((double) A2 * 0.5) * cell) * cell
 *   vertices  h_outline[k][j] = ((float) (qu_j * cell), (float) (qv_j * cell)): plane-local; the world point is p + u x + v z.  The
 *             entries after the last vertex are zero
 * h_outline [n_planes][max_vertices][2]; h_outline_q (the same shape, int32, may be NULL; for tests): the grid coordinates;
 * h_info8[k] = {code, vertices, points labelled k, 0, 0, 0, 0, 0}; for a code other than 0 the vertex count is 0 and only the codes
 * 1 .. 3 report the point count; nothing else is written for that plane (outline, area stay zero).  max_vertices 8..1024; n = 0 is legal
 * (code 1, or 5, or 4 for every plane, nothing is launched).  Returns the number of planes with code 0, or a negative error; after
 * ALVA_ERR_ARG the context stays usable.  One launch for all planes, one workgroup per plane (gather + octagon prune + gift wrapping,
 * at most max_vertices wrapping steps whatever the input); the host waits once.  Synchronous. */
int alva_plane_outlines(alva_ctx *ctx, const double *d_points, int n, const int *d_labels, int n_planes, const float *h_planes24,
                        int max_vertices, float *h_outline, int *h_outline_q, int *h_info8, double *h_area);

/* ---- anchors, stage 1: an anchor's support, the K nearest points ------------------------------------------------------------
 * ARCore HitResult.createAnchor / ARKit ARAnchor / WebXR XRAnchor tie a pose to the map around it; no reference counterpart (parity is
 * pinned by the numpy restatement tests/anchor_cases.py).  d_points: n x 3 world points (device, f64), n 0..16384; n_anchors 1..16 (the
 * hit test's bound); h_pos3[a][3]: the anchors' world positions; max_support = K, 8..64.  Per anchor a, position (ax, ay, az):
 *   A1 distance   d_i = ((x_i - ax)^2 + (y_i - ay)^2) + (z_i - az)^2: each difference first, then the products, then the two sums in the
 *                 written order, IEEE double
 *   A2 support    the min(K, n) points that come first under the total order (bits(d_i), i): the doubles' bit patterns compared as
 *                 unsigned 64-bit integers (d_i >= 0, so that is value order), ties by the lower index
 *   A3 record     h_index[a][0 .. count) = their indices in ascending (bits(d), i), h_dist2[a][..] = their d, h_count[a] = count =
 *                 min(K, n); the entries past count are -1 and 0
 * h_index, h_dist2: [n_anchors][max_support].  Everything after A1 compares bit patterns, so the result is a function of the point SET
 * and any correct algorithm gives the same bytes.  n = 0 is legal (count 0, nothing is launched).  Returns 0 or a negative error; after
 * ALVA_ERR_ARG the context stays usable.  One launch for all anchors, one 512-thread workgroup per anchor (distances in registers, a
 * radix select over their bit patterns, an in-order compaction, one wave sorts the survivors); the host waits once.  Synchronous. */
int alva_anchor_attach(alva_ctx *ctx, const double *d_points, int n, int n_anchors, const double *h_pos3, int max_support, int *h_index,
                       double *h_dist2, int *h_count);

/* ---- anchors, stage 2: the rigid motion of a support, robustly, and the anchor's pose carried along ------------------------------
 * n_anchors 1..64.  Per anchor a: m = h_count[a] (0..64) pairs at a FIXED stride of 64: h_ref[a][j][3], where support j was when the
 * anchor was attached, and h_cur[a][j][3], where it is now (both [n_anchors][64][3]; rows j >= m are not read; both may be NULL when
 * every m is 0); h_pose16_ref[a][16]: the anchor's pose at attach time in alva_find_plane's layout (in[4 c + r] = Rot[r][c],
 * in[12..14] = the translation).  IEEE double in the written order, no contraction; dot(u, v) = (u0 v0 + u1 v1) + u2 v2.
 * SUMS: every "sum over L" below is taken over the 64 lanes j = 0..63 of one wave, lane j contributing its term when j is in the lane
 * set L and +0.0 otherwise, in the __shfl_xor butterfly order with the masks 1, 2, 4, 8, 16, 32: s0[j] = term_j; s_(k+1)[j] = s_k[j] +
 * s_k[j ^ 2^k]; the sum is s6[0] (all 64 are equal: IEEE addition commutes) -- i.e. a balanced binary tree over adjacent pairs.
 *   U0 no support  m = 0: code 2, R = I, t = 0, the pose is the reference pose, byte for byte
 *   U1 spreads     for a lane set L with c lanes (first L = {0 .. m-1}, c = m): cp = (sum p) / c, cq = (sum q) / c per component;
 *                  p' = p - cp, q' = q - cq; Spp = sum ((p'x p'x + p'y p'y) + p'z p'z), Sqq likewise; rho = sqrt(Spp / c)
 *   U2 too few     c < 4: the fit is undetermined: R = I, t = cq - cp
 *   U3 rotation    S_ab = sum p'_a q'_b (a, b in x y z); Horn's symmetric 4 x 4
 *                      N = | (Sxx + Syy) + Szz   Syz - Szy             Szx - Sxz             Sxy - Syx           |
 *                          | .                   (Sxx - Syy) - Szz     Sxy + Syx             Szx + Sxz           |
 *                          | .                   .                     (Syy - Sxx) - Szz     Syz + Szy           |
 *                          | .                   .                     .                     (Szz - Sxx) - Syy   |
 *                  diagonalised by a cyclic Jacobi of exactly 12 sweeps over the pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), V = I at the
 *                  start; a pair with |N_pq| < 1e-300 is skipped, otherwise th = (N_qq - N_pp) / (2 N_pq), tt = sign(th) / (|th| +
 *                  sqrt(th th + 1)) with sign(0) = +1, cs = 1 / sqrt(tt tt + 1), sn = tt cs; N_pp -= tt N_pq, N_qq += tt N_pq, N_pq = 0;
 *                  for k other than p, q: (N_kp, N_kq) <- (cs N_kp - sn N_kq, sn N_kp + cs N_kq), mirrored; for every k: (V_kp, V_kq)
 *                  <- (cs V_kp - sn V_kq, sn V_kp + cs V_kq).  l1 = the largest diagonal entry (the lowest index on ties), l2 = the
 *                  largest of the other three.  l1 - l2 <= 1e-4 sqrt(Spp Sqq): undetermined (a collinear support): R = I, t = cq - cp.
 *                  Otherwise e = column l1's of V, (w, x, y, z) = e / sqrt(((e0 e0 + e1 e1) + e2 e2) + e3 e3), and
 *                      R = | 1 - 2 (yy + zz)   2 (xy - wz)       2 (xz + wy)     |
 *                          | 2 (xy + wz)       1 - 2 (xx + zz)   2 (yz - wx)     |    (R(e) = R(-e): no sign rule is needed)
 *                          | 2 (xz - wy)       2 (yz + wx)       1 - 2 (xx + yy) |
 *                  t_a = cq_a - dot(R row a, cp)
 *   the first fit  U1 - U3 over {0 .. m-1}: code 0 when determined, code 1 (translation only) otherwise; kept = m
 *   U4 trim        only after a determined first fit: r_j = sqrt((e0 e0 + e1 e1) + e2 e2) with e_a = q_a - (dot(R row a, p) + t_a);
 *                  med = the r_j of rank m / 2 (0-based) under the order (r, j); support j is kept iff r_j <= 3.7065 med (2.5 x 1.4826,
 *                  the hit test's) or r_j <= 1e-9 rho (rho of the first fit: keeps every point of a map that did not move, med = 0);
 *                  kept = their number.  If 4 <= kept < m: U1 - U3 over the kept lanes; determined: that fit replaces the first;
 *                  undetermined: the first fit stands.  One round only
 *   U5 pose        column c of the result = (dot(R row 0, v), dot(R row 1, v), dot(R row 2, v)) with v = (double) column c of the
 *                  reference pose, c = 0 1 2; the translation likewise from the reference translation, + t_a per component; cast to
 *                  float; out[3] = out[7] = out[11] = 0, out[15] = 1
 * h_pose16[a][16]; h_rt12[a][12] (may be NULL; for tests) = R row-major, then t, in double; h_info8[a] = {code, m, kept, 0, 0, 0, 0, 0}:
 * code 0 a rigid update, 1 translation only, 2 no support.  The pose is always derived from the attach-time reference, never from an
 * earlier answer: nothing accumulates.  Returns 0 or a negative error; after ALVA_ERR_ARG the context stays usable.  One launch for all
 * anchors: one wave per anchor (one support per lane), four anchors per 256-thread workgroup, no LDS, no barrier; the host waits once.
 * Synchronous. */
int alva_anchor_update(alva_ctx *ctx, int n_anchors, const int *h_count, const double *h_ref, const double *h_cur,
                       const float *h_pose16_ref, float *h_pose16, double *h_rt12, int *h_info8);

/* ---- depth from motion: a per-frame depth image for occlusion -----------------------------------------------------------
 * ARCore Depth API / ARKit sceneDepth / WebXR depth sensing, without a depth sensor; no reference counterpart (parity is pinned by the
 * numpy restatement tests/depth_cases.py).  A plane sweep over inverse depth between two gray images of one geometry: d_cur the current
 * frame, d_ref an earlier one (device u8, `pitch` bytes per row for both, width % 4 == 0).  h_calib8 = fx fy cx cy k1 k2 p1 p2;
 * h_T_rc12 = R_rc row-major (9) then t_rc, X_ref = R_rc X_cur + t_rc.  step 1..16, num_hyp D 8..256, 0 < rho_min < rho_max (inverse
 * depths, finite), patch_radius r 1..4 with N = (2r+1)^2, min_texture and min_conf 0..255.  The grid is gw = width / step by gh =
 * height / step (integer division).  Geometry is IEEE double in the written order, costs are integers.  Per grid pixel (gx, gy), centre
 * (u, v) = (gx step + step / 2, gy step + step / 2) in integers:
 *   1 patch       the N pixels (u + dx, v + dy), dy outer and dx inner, both -r..r; any outside the image: code 1.  c_i their gray
 *                 values in the current image, sum C their sum
 *   2 texture     T = sum |N c_i - sum C|; T < min_texture N N: code 2
 *   3 rays        per patch pixel (uu, vv) = alva_undistort_points' result for ((float) (u + dx), (float) (v + dy)); dc = ((uu - cx) / fx,
 *                 (vv - cy) / fy, 1); q = R_rc dc, each row associated (r0 x + r1 y) + r2 1
 *   4 hypotheses  k = 0..D-1: rho_k = rho_min + ((rho_max - rho_min) k) / (D - 1); P = q + rho_k t_rc per component (the point at depth
 *                 1 / rho_k, scaled by rho_k).  The hypothesis is invalid when, for any patch pixel, P.z is not > 1e-9, or (u', v') =
 *                 alva_project_points_dist's result for P (floats) with fu = floorf(u'), fv = floorf(v') fails 0 <= fu, fu + 1 <=
 *                 width - 1, 0 <= fv, fv + 1 <= height - 1 (float comparisons).  a = (int) rintf((u' - fu) 32.f), b likewise from v';
 *                 s_i = (g00 (32 - a)(32 - b) + g01 a (32 - b) + g10 (32 - a) b + g11 a b + 512) >> 10 with g00 = ref(fu, fv), g01 =
 *                 ref(fu + 1, fv), g10 = ref(fu, fv + 1), g11 = ref(fu + 1, fv + 1); cost_k = sum |(N c_i - sum C) - (N s_i - sum S)|,
 *                 a zero-mean SAD on integers
 *   5 winner      kb = the valid k of the smallest cost (= best), the lowest k on ties; no valid k: code 3.  second = the smallest cost
 *                 over valid k with |k - kb| >= 2; conf = 255 - (255 best) / max(second, 1) in integer division, 0 without such a k
 *   6 refinement  when 0 < kb < D - 1, both neighbours are valid and den = cost[kb-1] - 2 best + cost[kb+1] > 0: off = (double)
 *                 (cost[kb-1] - cost[kb+1]) / (2 den), otherwise 0; rho = rho_min + ((rho_max - rho_min) (kb + off)) / (D - 1); depth =
 *                 (float) (1.0 / rho)
 *   7 codes       in precedence 1, 2, 3, then 5: kb is 0 or D - 1 (the surface is outside the swept range), 4: conf < min_conf, 0: a depth
 * Depth is the camera-space z of the surface, in the units of t_rc, at the raw pixel (u, v) of the current frame.  d_depth f32, d_conf
 * u8, d_code u8, each gh x gw on the device: depth is written for code 0 and is 0 otherwise, conf for codes 0, 4 and 5 and is 0
 * otherwise.  h_info8 = the count of each code 0..5, then gw, gh.  d_best (device int32 [gh gw 4], may be NULL; for tests) = {kb,
 * best, second, T}: -1 for what does not exist (kb, best and second of codes 1 2 3; second without a k two steps from kb), T = 0 for
 * code 1.  The same inputs give the same bits.  Returns 0 or a negative error; after ALVA_ERR_ARG the context stays usable.  One launch,
 * one wave per grid pixel with its lanes over the hypotheses, and a second small launch that counts the codes.  Synchronous. */
int alva_depth_sweep(alva_ctx *ctx, const uint8_t *d_cur, const uint8_t *d_ref, size_t pitch, int width, int height,
                     const double *h_calib8, const double *h_T_rc12, int step, int num_hyp, double rho_min, double rho_max,
                     int patch_radius, int min_texture, int min_conf, float *d_depth, uint8_t *d_conf, uint8_t *d_code, int *h_info8,
                     int *d_best);

/* ---- dense depth: the depth image fused over time and completed ------------------------------------------------------------
 * ARCore acquireDepthImage16Bits beside acquireRawDepthImage16Bits (which alva_depth_sweep is), ARKit smoothedSceneDepth; no reference
 * counterpart (parity is pinned by the numpy restatement tests/dense_cases.py).  Two stages on the sweep's grid gw = width / step by gh =
 * height / step.  Geometry is IEEE double in the written order, float roundings exactly where the camera model has them, every decision
 * is an integer or a single IEEE comparison, every sum of more than two terms is an integer sum.  The same inputs give the same bits.
 *
 * alva_depth_fuse carries a previous fused image into the current frame and fuses the current measurement into it.  A state is, per
 * grid pixel, an inverse depth rho (f32, 0 = none) and a weight w (u8, 0 = none), each gh x gw on the device.  d_prev_rho / d_prev_w: the
 * previous state (both NULL: none); h_T_cp12 = R_cp row-major (9) then t_cp, X_cur = R_cp X_prev + t_cp; h_calib8 as for the sweep;
 * d_depth / d_conf / d_code: the sweep's outputs for the current frame (all three NULL: no measurement); decay 0..256, w_max 1..255,
 * rel_tol > 0 (finite).  Outputs d_rho, d_w, d_src (u8), each gh x gw, which must not overlap the previous state.
 *   F1 warp         per previous grid pixel i = gy gw + gx with w > 0 and rho > 0: centre (u, v) = (gx step + step / 2, gy step + step / 2);
 *                   (uu, vv) = alva_undistort_points' result for ((float) u, (float) v); dc = ((uu - cx) / fx, (vv - cy) / fy, 1); P = R_cp dc
 *                   + rho t_cp, each row ((r0 x + r1 y) + r2 1) + (double) rho t (the point scaled by rho: nothing is divided).  Dropped
 *                   when P.z is not > 1e-9.  (u', v') = alva_project_points_dist's result for P (floats); fu = floorf(u' + 0.5f), fv =
 *                   floorf(v' + 0.5f); dropped unless 0 <= fu < gw step and 0 <= fv < gh step (float comparisons, so a NaN is dropped);
 *                   tu = (int) fu, tv = (int) fv, the target cell is (tu / step, tv / step).  rho' = (float) ((double) rho / P.z); dropped
 *                   unless 0 < rho' <= FLT_MAX.  Of the sources that land in one cell the largest rho' wins (the nearest surface), the
 *                   lowest i on a tie: the maximum over the sources of the 64-bit key (bits(rho') << 32) | (0xFFFFFFFF - i)
 *   F2 carried      w' = (w_src decay) >> 8 of the winning source; w' == 0 or no source: the cell has no carried value
 *   F3 measurement  where code == 0 and depth > 0: rho_m = (float) (1.0 / (double) depth), w_m = max(1, conf >> 3)
 *   F4 fusion       neither: rho = 0, w = 0, src 0.  Measurement only: (rho_m, w_m), src 1.  Carried only: (rho', w'), src 2.  Both, and
 *                   |rho' - rho_m| <= rel_tol max(rho', rho_m) in double: rho = (float) (((double) w' rho' + (double) w_m rho_m) / (double)
 *                   (w' + w_m)), w = min(w_max, w' + w_m), src 3.  Both, disagreeing, w_m >= w': (rho_m, w_m), src 4.  Both, disagreeing,
 *                   w_m < w': (rho', w' - w_m), src 5.  (w_max bounds the weight of src 3 only.)
 *   F5 info         h_info8 = the count of each src 0..5, then gw, gh
 * Three launches (clear the keys, warp: one 64-bit atomicMax per source, fuse and count) and one host wait.
 *
 * alva_depth_fill completes a state by push-pull over a pyramid, guided by the gray image so that a fill does not cross an intensity
 * edge.  d_rho / d_w: the state; d_cur: the current gray image (u8, `pitch` bytes per row); rho_ref > 0 (finite) the fixed-point scale,
 * max_level L 1..8.
 *   P1 level 0      per cell with w > 0: q = clip((int) rint(((double) rho / rho_ref) 65536.0), 0, 2^20 - 1) (a NaN gives 0), W = w; else
 *                   q = 0, W = 0.  The guide G = the gray value at the cell's centre pixel (gx step + step / 2, gy step + step / 2)
 *   P2 pull         L times: level l + 1 is ceil(h_l / 2) x ceil(w_l / 2); cell (x, y) has the children (2x + dx, 2y + dy), dx, dy in {0, 1},
 *                   that lie inside level l (n of them).  Wsum = sum W_c; q = (sum W_c q_c + Wsum / 2) / Wsum, 0 when Wsum = 0; W = min(255,
 *                   Wsum); G = (sum G_c + n / 2) / n.  Integer division throughout
 *   P3 push         from level L - 1 down to 0, for the cells without a value (W = 0; a cell with W > 0 keeps its own q): per axis the
 *                   parents are x >> 1 with weight 3 and (x >> 1) + (x & 1 ? 1 : -1) with weight 1, so four parents with the bilinear
 *                   weights 9, 3, 3, 1.  A parent counts when it lies inside level l + 1 and has a value, its own or a filled one; its
 *                   weight wt = the bilinear weight times E[|G_cell - G_parent|], E[d] = max(1, 64 >> min(d >> 3, 6)).  S = sum wt; S > 0:
 *                   the cell is filled with q = (sum wt q_p + S / 2) / S, else it has no value at this level.  The evidence level of a
 *                   cell with its own value at level l is l; of a filled cell the smallest evidence level among the parents that counted
 *   P4 output       at level 0: w > 0 (a seed, never altered): depth = (float) (1.0 / (double) rho), d_level = 0.  Filled with q > 0: depth
 *                   = (float) (65536.0 / ((double) q rho_ref)), d_level = its evidence level 1..L.  Otherwise depth = 0, d_level = 255.
 *                   The nearest evidence of a filled cell is about 2^d_level grid cells away, so max_level bounds the extrapolation
 * d_depth f32 (camera-space z, 0 = none) and d_level u8, each gh x gw; h_info4 = {seeds, filled, empty, the largest d_level of a filled
 * cell (0 without one)}.  Two launches for max_level <= 4 and three above, whatever the grid, and one host wait.
 * Both return 0 or a negative error; after ALVA_ERR_ARG the context stays usable.  Synchronous. */
int alva_depth_fuse(alva_ctx *ctx, const float *d_prev_rho, const uint8_t *d_prev_w, const double *h_T_cp12, const double *h_calib8,
                    int width, int height, int step, const float *d_depth, const uint8_t *d_conf, const uint8_t *d_code, int decay,
                    int w_max, double rel_tol, float *d_rho, uint8_t *d_w, uint8_t *d_src, int *h_info8);
int alva_depth_fill(alva_ctx *ctx, const float *d_rho, const uint8_t *d_w, const uint8_t *d_cur, size_t pitch, int width, int height,
                    int step, double rho_ref, int max_level, float *d_depth, uint8_t *d_level, int *h_info4);

/* ---- scene mesh: depth fused into a truncated signed distance volume, its surface extracted as triangles --------------------
 * ARKit scene reconstruction (ARMeshAnchor / ARMeshGeometry), WebXR mesh-detection (XRMesh), what ARCore's raw depth image is for; no
 * reference counterpart (parity is pinned by the numpy restatement tests/mesh_cases.py).  The volume is a cube of N^3 voxels, 4 <= N <=
 * 256, on the device as d_q (int16) and d_w (uint8), each [N][N][N] with the index (k N + j) N + i, i along world x, j along y, k along
 * z.  q is the truncated signed distance in units of trunc / 32767, positive in front of the surface; w is the weight, 0 = never seen.  A
 * fresh volume is all zero bytes.  h_origin3 = the world position of the volume's minimum corner, voxel = the edge of a voxel (> 0,
 * finite).  Geometry is IEEE double in the written order, float roundings exactly where the camera model has them, every decision is an
 * integer or a single IEEE comparison, every sum of more than two terms is an integer sum.  The same inputs give the same bits.
 *
 * alva_mesh_integrate fuses one depth image into the volume, in place.  trunc > 0 (finite); h_T_cw12 = R_cw row-major (9) then t_cw,
 * X_cam = R_cw X_world + t_cw; h_calib8, width, height, step as for the sweep; d_depth / d_conf / d_code the sweep's outputs on the grid
 * gw = width / step by gh = height / step; w_max 1..255.  Per voxel (i, j, k):
 *   M1 centre       Pw = (o_x + ((double) i + 0.5) voxel, o_y + ((double) j + 0.5) voxel, o_z + ((double) k + 0.5) voxel); Pc = R_cw Pw +
 *                   t_cw, each row ((r0 x + r1 y) + r2 z) + t.  Dropped (outside) when Pc.z is not > 1e-9
 *   M2 pixel        (u', v') = alva_project_points_dist's result for Pc (floats); fu = floorf(u'), fv = floorf(v'); dropped (outside)
 *                   unless 0 <= fu < gw step and 0 <= fv < gh step (float comparisons, so a NaN is dropped); the grid cell is ((int) fu /
 *                   step, (int) fv / step)
 *   M3 measurement  the cell counts where code == 0 and depth > 0, with w_m = max(1, conf >> 3) (F3 of alva_depth_fuse); otherwise the
 *                   voxel is dropped (no depth)
 *   M4 distance     s = (double) depth - Pc.z, projective along the camera's z.  s < -trunc: dropped (hidden).  t = s / trunc; t >= 1: q_m
 *                   = 32767 (free: free space is carved), otherwise q_m = (int) rint(t 32767.0)
 *   M5 update       A = q w + q_m w_m (int32), S = w + w_m; q' = floor((2 A + S) / (2 S)), a true floor (A may be negative); w' =
 *                   min(w_max, S)
 * h_info8 = {updated, hidden, free (a subset of updated), outside, no depth, N, 0, 0}.  One launch, one thread per voxel with i on the
 * lanes, nothing written but the thread's own voxel (so the order of execution cannot matter), integer atomic sums for the counts, and
 * one host wait.
 *
 * alva_mesh_extract is surface nets: one vertex per cell the surface crosses, one quad per voxel edge it crosses; no case table, and
 * the result is a set function of the volume.  min_weight 1..255, max_vertices and max_triangles >= 1.
 *   X1 voxels       valid = w >= min_weight, inside = q < 0 (q == 0 counts as outside)
 *   X2 cells        cell (i, j, k), 0 <= i, j, k < N - 1, has the corners (i + dx, j + dy, k + dz); it is active when all eight are valid
 *                   and they are not all on one side
 *   X3 vertex       over the cell's 12 edges whose ends a (the lower coordinate) and b differ in inside: D = |q_a| + |q_b|, f = (2048
 *                   |q_a| + D) / (2 D) in integer division (0..1024); the crossing point in 1/1024 voxel is 1024 index(a) plus f along
 *                   the edge's axis.  Per axis X = (sum + m / 2) / m over the m crossing edges, integer division; the world coordinate
 *                   = (float) (o + ((double) X / 1024.0 + 0.5) voxel)
 *   X4 normal       g_x = sum q(dx = 1) - sum q(dx = 0) over the eight corners (int), g_y and g_z likewise; L2 = g_x^2 + g_y^2 + g_z^2
 *                   (int64); n = (float) ((double) g / sqrt((double) L2)), zero when L2 == 0.  It points to the free side
 *   X5 order        the vertices in ascending (k (N - 1) + j) (N - 1) + i of their cells; every active cell emits one, also one that no
 *                   face uses (at the border of the observed region)
 *   X6 faces        per voxel v and axis a = 0, 1, 2 with (b, c) the next two axes cyclically: the edge v -> v + a emits a quad when it
 *                   lies inside the grid, both ends are valid and differ in inside, and the four cells Q0..Q3 = v - b - c, v - c, v, v -
 *                   b exist and are active (counter-clockwise about +a).  inside(v): the triangles (Q0, Q1, Q2), (Q0, Q2, Q3), otherwise
 *                   (Q0, Q2, Q1), (Q0, Q3, Q2): the geometric normal points to the free side, as X4's.  Order: ascending (k N + j) N + i
 *                   of v, then a, two triangles each
 *   X7 info         h_info8 = {code, vertices, triangles, valid voxels, inside valid voxels, N, 0, 0}.  Code 0: a mesh; 1: no active
 *                   cell; 3: more vertices than max_vertices or more triangles than max_triangles -- the two counts are still the
 *                   true ones and the three arrays are not written
 * d_vertices and d_normals f32 [max_vertices][3] (world coordinates), d_triangles int32 [max_triangles][3] (vertex indices), on the
 * device.  Five launches whatever N -- classify (the activity of a wave's 64 cells is one ballot word, counts per workgroup), quads,
 * a one-workgroup scan of the workgroups' counts, vertices, triangles -- and one host wait; no workgroup waits for another inside a
 * launch.  Both return 0 or a negative error; after ALVA_ERR_ARG the context stays usable.  Synchronous. */
int alva_mesh_integrate(alva_ctx *ctx, int16_t *d_q, uint8_t *d_w, int N, const double *h_origin3, double voxel, double trunc,
                        const double *h_T_cw12, const double *h_calib8, int width, int height, int step, const float *d_depth,
                        const uint8_t *d_conf, const uint8_t *d_code, int w_max, int *h_info8);
int alva_mesh_extract(alva_ctx *ctx, const int16_t *d_q, const uint8_t *d_w, int N, const double *h_origin3, double voxel, int min_weight,
                      int max_vertices, int max_triangles, float *d_vertices, float *d_normals, int *d_triangles, int *h_info8);

/* ---- raycasting the scene volume: rays marched to the zero crossing of the signed distance -------------------------------------
 * ARKit's raycast against mesh geometry, WebXR hit test on mesh-detection geometry, the depth image ARKit and HoloLens derive from their
 * reconstruction, the surface prediction of KinectFusion; no reference counterpart (parity is pinned by the numpy restatement
 * tests/raycast_cases.py).  The volume (d_q, d_w, N, h_origin3 = o, voxel) and min_weight 1..255 are as for alva_mesh_extract.  A ray is
 * an origin O and a direction D of any length, both in world coordinates; t is in units of D.  t_near <= t_far per call: t_near finite,
 * t_far finite or +inf.  Geometry is IEEE double in the written order; everything from R3's fractions on is an integer.  The same
 * inputs give the same bits.  Per ray:
 *   R0 reject   any component of O or D not finite, or max(|D_x|, |D_y|, |D_z|) == 0: code 4
 *   R1 clip     against the box of the voxel centres, lo_a = o_a + 0.5 voxel, hi_a = o_a + ((double) N - 0.5) voxel: t0 = t_near, t1 =
 *               t_far, then per axis a = x, y, z: D_a == 0: code 1 unless lo_a <= O_a <= hi_a; otherwise ta = (lo_a - O_a) / D_a, tb =
 *               (hi_a - O_a) / D_a, t0 = max(t0, min(ta, tb)), t1 = min(t1, max(ta, tb)).  Code 1 unless t0 <= t1
 *   R2 samples  dt = (0.5 voxel) / max|D_a| (no axis moves more than half a voxel per step); t_n = t0 + (double) n dt (never
 *               accumulated), n = 0, 1, .. while t_n <= t1 and n <= 2 N + 1.  The second condition never binds for finite input -- a ray
 *               crosses the box in at most 2 N - 1 samples -- and makes the loop's length an integer fact.  P_a = O_a + t_n D_a
 *   R3 value    g_a = (P_a - o_a) / voxel - 0.5; i_a = clamp(floor(g_a), 0, N - 2), f_a = clamp(rint((g_a - (double) i_a) 256.0), 0,
 *               256), each clamped as a double and then converted to int, a NaN giving the lower bound (so no index leaves the volume,
 *               whatever the ray).  The sample is valid when all eight corners (i_x + dx, i_y + dy, i_z + dz) have w >= min_weight; its
 *               value is F = sum over the corners of q wx wy wz (int64, |F| < 2^42) with wx = f_x where dx = 1 and 256 - f_x where dx = 0,
 *               wy and wz likewise
 *   R4 march    prev = none.  An invalid sample: prev = none (unknown space is passed through, and no crossing is taken across it).  A
 *               valid sample with prev valid, F_prev > 0 and F <= 0: a hit.  A valid sample with prev valid, F_prev <= 0 and F > 0: code 3,
 *               the surface was met from behind, and the ray ends.  Any other valid sample becomes prev.  Samples exhausted: code 2
 *   R5 hit      code 0: t_hit = t_prev + dt ((double) F_prev / (double) (F_prev - F)) with t_prev = t0 + (double) (n - 1) dt; p_a = O_a +
 *               t_hit D_a; the outputs are (float) t_hit and (float) p
 *   R6 normal   X4's integer gradient g over the eight corners of the HIT sample's cell (all valid); L2 as there; nd = (double) g /
 *               sqrt((double) L2), n = (float) nd; zero when L2 == 0.  It points to the free side
 *   R7 pose     (alva_mesh_raycast_pixels, where d_pose16 is given) for code 0 with L2 > 0 and |(nd_x D_x + nd_y D_y) + nd_z D_z| /
 *               sqrt((D_x D_x + D_y D_y) + D_z D_z) >= 0.0872 (alva_hit_test's grazing gate): alva_hit_test's pose step with y = nd --
 *               a = R_wc[:,0], x' = a - ((a_x y_x + a_y y_y) + a_z y_z) y, |x'| = sqrt((x'_x x'_x + x'_y x'_y) + x'_z x'_z); |x'| < 1e-6:
 *               the same from a = R_wc[:,1]; x = x' / |x'|, z = x cross y -- in alva_find_plane's layout: out[0..2] = (float) x, out[4..6]
 *               = (float) y, out[8..10] = (float) z, out[12..14] = R5's p, out[15] = 1, and pose_ok = 1.  Otherwise (also when both |x'| <
 *               1e-6: R_wc is no rotation) sixteen zeros and pose_ok = 0
 *   R8 info     h_info8 = {rays, the count of each code 0..4, the largest number of samples any ray took, N}; integer atomic sums and an
 *               integer atomic maximum, folded per workgroup first
 * Codes: 0 a hit, 1 the ray misses the box (or [t_near, t_far] does), 2 no surface on the ray, 3 the surface from behind, 4 rejected.
 * d_t f32 [n], d_point3 and d_normal3 f32 [n][3], d_code u8 [n], all on the device; t, p and n are zero unless the code is 0.
 *
 * alva_mesh_raycast takes n_rays (1..2^20) explicit rays d_rays6 (device, f64 [n][6] = O then D).
 *
 * alva_mesh_raycast_pixels takes the rays of image pixels seen from a pose: h_T_wc12 = R_wc row-major (9) then t_wc, X_world = R_wc
 * X_cam + t_wc; h_calib8, width, height, step as for alva_depth_sweep.  d_uv == NULL: the sweep's grid, gw = width / step by gh = height /
 * step (at most 2^22 pixels), pixel (gx, gy) at the raw pixel ((float) (gx step + step / 2), (float) (gy step + step / 2)), outputs at
 * index gy gw + gx, n_px not read.  Otherwise d_uv (device, f32 [n_px][2]) holds n_px (1..2^20) raw pixels.  A pixel's ray is step 3 of
 * alva_depth_sweep: (uu, vv) = alva_undistort_points' result; dc = (((double) uu - cx) / fx, ((double) vv - cy) / fy, 1); D = R_wc dc,
 * each row associated (r0 x + r1 y) + r2 1; O = t_wc.  Because dc.z = 1, t_hit is the camera-space z: d_t is a depth image in
 * alva_depth_sweep's convention, 0 where the code is not 0.  d_pose16 (f32 [n][16]) and d_pose_ok (u8 [n]) may be NULL (d_pose_ok only
 * with d_pose16).  The grid, the list of the grid's pixels and alva_mesh_raycast fed those pixels' rays give the same bits.
 *
 * Unknown space is TRANSPARENT (a ray passes through what was never seen, and finds what lies behind it), and every ray takes every
 * sample up to its hit: there is no empty-space skipping.  Both return 0 or a negative error; after ALVA_ERR_ARG the context stays
 * usable.  One launch -- one lane per ray; in grid mode a wave is an 8 x 8 tile of grid pixels -- and one host wait.  Synchronous. */
int alva_mesh_raycast(alva_ctx *ctx, const int16_t *d_q, const uint8_t *d_w, int N, const double *h_origin3, double voxel, int min_weight,
                      int n_rays, const double *d_rays6, double t_near, double t_far, float *d_t, float *d_point3, float *d_normal3,
                      uint8_t *d_code, int *h_info8);
int alva_mesh_raycast_pixels(alva_ctx *ctx, const int16_t *d_q, const uint8_t *d_w, int N, const double *h_origin3, double voxel,
                             int min_weight, const double *h_T_wc12, const double *h_calib8, int width, int height, int step, int n_px,
                             const float *d_uv, double t_near, double t_far, float *d_t, float *d_point3, float *d_normal3, uint8_t *d_code,
                             float *d_pose16, uint8_t *d_pose_ok, int *h_info8);

/* ---- mesh colour: the frame's colour fused into the scene volume beside the distance, and sampled at world points ---------------
 * What ARKit / ARCore / WebXR apps paint a scan preview, a minimap or a raycast hit with; what KinectFusion, Open3D's
 * ScalableTSDFVolume and InfiniTAM carry beside the distance; no reference counterpart (parity is pinned by the numpy restatement
 * tests/mesh_color_cases.py).  The colour volume d_c is u8 [N^3][4] = (r, g, b, colour weight wc) at the index of d_q; a fresh one is all
 * zero bytes.  Geometry is IEEE double in the written order, every decision is an integer or a single IEEE comparison, every sum of more
 * than two terms is an integer sum.  The same inputs give the same bits.  There is no exposure metadata and nothing is linearised:
 * every colour is a mean **in the PIXEL-VALUE domain** (a mean of sRGB-encoded bytes, as they arrive), so it follows the camera's
 * exposure and white balance and is slightly darker than the linear-light mean across a strong edge.
 *
 * alva_color_thumb reduces one RGBA frame (d_rgba, `pitch` bytes per row, both multiples of 4) to a thumbnail: cstep 1..16, tw = width /
 * cstep, th = height / cstep, both >= 1; d_thumb u8 [th][tw][4] on the device, 4-byte aligned.
 *   T1 mean         for cell (tx, ty) and channel c of R, G, B: sum = the integer sum of the cstep^2 bytes of the block at (tx cstep, ty
 *                   cstep); out_c = (2 sum + cstep^2) / (2 cstep^2) in integer division (the mean, rounded half up); out[3] = 255.  The
 *                   input's alpha is not used, and no column past tw cstep or row past th cstep is read
 * It only enqueues (one launch), as alva_light_bin.
 *
 * alva_mesh_integrate_color is alva_mesh_integrate with colour: the same arguments, and d_c, d_thumb (alva_color_thumb's output for this
 * frame and `width`, `height`, cstep).  Per voxel M1 - M5 run exactly as there -- it is the same kernel body with a compile-time flag, and
 * d_q and d_w afterwards are byte for byte what alva_mesh_integrate leaves -- and then
 *   K1 coloured     when M5 ran, the voxel is not free (t < 1: it lies in the truncation band -trunc <= s < trunc), and tx = (int) fu /
 *                   cstep < tw and ty = (int) fv / cstep < th with M2's fu, fv
 *   K2 measurement  (r_m, g_m, b_m) = thumb[ty][tx]; the weight is M3's w_m
 *   K3 update       per channel S = wc + w_m, c' = (2 (c wc + c_m w_m) + S) / (2 S) in integer division (everything is non-negative); wc'
 *                   = min(w_max, S)
 * h_info8 = alva_mesh_integrate's with [6] = voxels coloured.  One launch on the same striding grid of at most 2048 workgroups; the
 * colour voxel is one 32-bit load and one 32-bit store per lane, contiguous over the wave; one host wait.
 *
 * alva_mesh_color_at samples the colour volume at n (1..2^20) world points d_points3 (device, f32 [n][3]); d_rgba u8 [n][4] (4-byte
 * aligned) and d_code u8 [n] on the device.  Per point p:
 *   A0 reject       a component that is not finite: code 4
 *   A1 inside       g_a = ((double) p_a - o_a) / voxel - 0.5; code 1 unless 0 <= g_a <= N - 1 on every axis (double comparisons): the box of
 *                   the voxel centres, R1's
 *   A2 cell         i_a and f_a from g_a exactly as R3 of the raycast, with its clamps (one body for both kernels): no index leaves the
 *                   volume, whatever the point
 *   A3 weights      over the eight corners (i_x + dx, i_y + dy, i_z + dz): Wt = wx wy wz wc (int64) with wx = f_x where dx = 1 and 256 -
 *                   f_x where dx = 0, wy and wz likewise, wc the corner's colour weight; S = sum Wt.  S == 0: code 2, no colour was ever
 *                   fused there
 *   A4 colour       per channel (2 sum(c Wt) + S) / (2 S) in integer division; d_rgba = (r, g, b, 255).  Four zeros unless the code is 0
 * h_info8 = {n, the count of code 0, 1, 2, 4, 0, 0, N}, integer atomic sums folded per workgroup first.  A corner without colour (wc = 0)
 * takes no part, so the colour of a cell at the border of what was seen is the mean of the corners that have one.  One launch -- one
 * lane per point -- and one host wait.  All three return 0 or a negative error; after ALVA_ERR_ARG the context stays usable. */
int alva_color_thumb(alva_ctx *ctx, const uint8_t *d_rgba, size_t pitch, int width, int height, int cstep, uint8_t *d_thumb);
int alva_mesh_integrate_color(alva_ctx *ctx, int16_t *d_q, uint8_t *d_w, uint8_t *d_c, int N, const double *h_origin3, double voxel,
                              double trunc, const double *h_T_cw12, const double *h_calib8, int width, int height, int step,
                              const float *d_depth, const uint8_t *d_conf, const uint8_t *d_code, const uint8_t *d_thumb, int cstep,
                              int w_max, int *h_info8);
int alva_mesh_color_at(alva_ctx *ctx, const uint8_t *d_c, int N, const double *h_origin3, double voxel, int n, const float *d_points3,
                       uint8_t *d_rgba, uint8_t *d_code, int *h_info8);

/* ---- shifting the scene volume by whole voxels: what lets it follow the camera ---------------------------------------------------
 * Kintinuous' shifting volume, InfiniTAM's swapping, Open3D's scalable volume; no reference counterpart (parity is pinned by the numpy
 * restatement tests/mesh_shift_cases.py).  The volume (d_q, d_w, N) is as for alva_mesh_integrate, d_c the colour volume of
 * alva_mesh_integrate_color or NULL (then d_c_out is NULL too).  h_shift3 = (s_x, s_y, s_z) in voxels.  The stage is OUT OF PLACE: no
 * output may overlap an input (or another output); a call where one does is ALVA_ERR_ARG.  Nothing is resampled:
 *   S1 source       the destination voxel (i, j, k) -- i fastest, as everywhere -- has the source (i + s_x, j + s_y, k + s_z)
 *   S2 copy / empty where the source lies in [0, N)^3 the voxel's q, w and four colour bytes are the source's; otherwise the voxel is
 *                   empty: all of its bytes are zero
 *   S3 large shifts any |s_a| >= N leaves everything empty.  That is decided before any index is formed: every int is a legal shift
 *                   component, INT_MIN and INT_MAX included
 *   S4 counts       h_info8 = {voxels copied, copied voxels with w > 0, source voxels with w > 0 that were not copied (what the shift
 *                   lost), copied voxels with a colour weight > 0 (0 without d_c), 0, 0, 0, N}; integer sums, folded per workgroup
 * The world origin that goes with the output is origin + s voxel: a world point keeps its voxel's bytes.  The shift (0, 0, 0) is a plain
 * copy.  One launch for the three volumes on k_mesh_integrate's striding grid (at most 2048 workgroups): every input byte is loaded at
 * most once, every output byte stored exactly once, contiguous over the wave.  Where N and s_x are multiples of 8 and the arrays are
 * aligned (q and c to 16 bytes, w to 8) a lane moves 8 voxels -- 16, 8 and 32 bytes; otherwise one voxel.  Both give the same bytes.  One
 * host wait.  Returns 0 or a negative error; after ALVA_ERR_ARG the context stays usable.  Synchronous. */
int alva_mesh_shift(alva_ctx *ctx, const int16_t *d_q, const uint8_t *d_w, const uint8_t *d_c, int N, const int *h_shift3, int16_t *d_q_out,
                    uint8_t *d_w_out, uint8_t *d_c_out, int *h_info8);

/* ---- the scene mesh in blocks: a world-fixed lattice of blocks, a digest per block, the meshes of selected blocks ---------------
 * ARKit's ARMeshAnchors (chunks with an identity that are added, updated and removed), WebXR mesh-detection's XRMesh objects with
 * lastChangedTime, HoloLens' surface observers; no reference counterpart (parity is pinned by the numpy restatement
 * tests/mesh_block_cases.py).  The volume (d_q, d_w, N, h_origin3, voxel) and min_weight are as for alva_mesh_extract; it is not
 * written.  alva_mesh_shift moves a world point's bytes by whole voxels, so a caller that keeps the sum of its shifts has a lattice in
 * which a world point keeps its index:
 *   L1 lattice      h_lattice3 (|lattice_a| <= 2^30) is the global index of the local voxel (0, 0, 0): voxel (i, j, k) has g = lattice +
 *                   (i, j, k).  The block edge B is 8, 16 or 32 voxels; the block key is b_a = floor(g_a / B), a true floor (keys may be
 *                   negative).  The local block grid covers floor(lattice_a / B) .. floor((lattice_a + N - 1) / B) per axis -- h_nb3 blocks
 *                   -- and is enumerated in ascending (b_z, b_y, b_x).  Blocks at the cube's faces may be partial
 *   L2 ownership    a quad of X6 belongs to the block of its voxel v.  A block's vertices are all active cells (X2) whose minimum corner
 *                   d = g - B b lies in [-1, B - 1]^3: its own cells and one layer on the low side, which its quads reference.  They are
 *                   ordered by ascending cell index; the triangles are X6's order restricted to the block's voxels, their indices local
 *                   to the block, 0 .. nv - 1.  A boundary vertex is therefore repeated in the neighbouring blocks with identical
 *                   floats: adjacent block meshes are watertight against each other.  The floats are X3 / X4 on the same local
 *                   indices and the same origin: byte for byte what alva_mesh_extract writes for the same cell
 *   L3 digest       a block's mesh is a function of the (B + 2)^3 voxels with d in [-1, B]^3, those outside the cube counting as
 *                   invalid, and of each only `valid` (X1) and, where valid, q.  For a valid voxel p = ((d_z + 1) (B + 2) + (d_y + 1)) (B
 *                   + 2) + (d_x + 1), x = ((uint64) p << 17) | 0x10000 | (uint16) q, and the splitmix64 finaliser z = x +
 *                   0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) 0x94D049BB133111EB; z ^= z >> 31.
 *                   The digest is the sum of z over the box's valid voxels mod 2^64 -- an integer sum, so the order of execution
 *                   cannot matter; an unseen block has digest 0.  p is relative to the block: a shift does not change the digest
 *                   of a block whose box stays inside the cube, nor does a weight that changes without crossing min_weight.  It is a
 *                   HASH: two different boxes share a digest with a chance of about 2^-64, and a caller that cannot accept that
 *                   extracts without asking (the session call's ALL flag)
 *   L4 counts       per block nv = the active cells in L2's range, nq = the quads owned (2 nq triangles); a block is PRESENT when nq > 0
 * alva_mesh_block_digest writes d_digest (u64 [nb]) and d_counts (i32 [nb][2] = nv, nq), nb = h_nb3[0] h_nb3[1] h_nb3[2], both on the
 * device.  One launch whatever N: one workgroup per block keeps the box in LDS as two bits per voxel, loads contiguous along i, and
 * stores its own sum -- no atomics -- and one host wait.
 *
 * alva_mesh_extract_blocks extracts the n_sel (>= 0) blocks h_sel_keys [n_sel][3] = (b_x, b_y, b_z) -- strictly ascending in (z, y, x) and
 * inside the block grid; otherwise ALVA_ERR_ARG -- packed in selection order into d_vertices / d_normals (f32 [max_vertices][3]) and
 * d_triangles (i32 [max_triangles][3]) on the device; h_ranges [n_sel][4] = {v0, nv, t0, nt}: the block's vertices are v0 .. v0 + nv - 1,
 * its triangles t0 .. t0 + nt - 1, with indices 0 .. nv - 1.  h_info8 = {code, vertices, triangles, n_sel, selected blocks that are present,
 * N, B, 0}, codes as X7: 0 meshes; 1 no selected block has an active cell; 3 over a cap -- the two counts are still the true ones and
 * neither the three arrays nor h_ranges are written.  Three launches whatever n_sel -- counts, a one-workgroup scan, vertices and
 * triangles -- and one host wait; no workgroup waits for another inside a launch.  Both return 0 or a negative error; after
 * ALVA_ERR_ARG the context stays usable.  Synchronous. */
int alva_mesh_block_digest(alva_ctx *ctx, const int16_t *d_q, const uint8_t *d_w, int N, const int *h_lattice3, int min_weight, int B,
                           int *h_nb3, unsigned long long *d_digest, int *d_counts);
int alva_mesh_extract_blocks(alva_ctx *ctx, const int16_t *d_q, const uint8_t *d_w, int N, const double *h_origin3, double voxel,
                             const int *h_lattice3, int min_weight, int B, int n_sel, const int *h_sel_keys, int max_vertices,
                             int max_triangles, float *d_vertices, float *d_normals, int *d_triangles, int *h_ranges, int *h_info8);

/* ---- light estimation: ambient intensity, spherical harmonics, primary light -----------------------------------------------
 * ARCore LightEstimate, ARKit ARLightEstimate / ARDirectionalLightEstimate, WebXR light-estimation; no reference counterpart (parity is
 * pinned by the numpy restatement tests/light_cases.py).  A camera sees a small part of the sphere, so every frame is binned by its
 * rotation into a world-aligned cube map kept on the device, N = ALVA_LIGHT_N cells per face edge, ALVA_LIGHT_CELLS in all, and the
 * estimate is projected from that map.  The environment is treated as DISTANT: only the frame's rotation places it, never its position.
 * There is no exposure metadata, so every value is in the PIXEL-INTENSITY domain (pixel value 255 = 1.0 after linearisation): the
 * estimate follows the camera's exposure and is not photometric.  Decisions are made on integers or on single IEEE double operations in
 * the written order; a sum whose order is not written down is an integer sum.  The same inputs give the same bits.
 *
 * The frame accumulators: ALVA_LIGHT_ACC_WORDS uint64 on the device -- per cell {S_R, S_G, S_B, pixels}, then for the frame as a whole
 * {S_R, S_G, S_B, pixels, pixels with a channel >= 250, blocks, 0, 0}; all zero before the first bin.  The environment state:
 * ALVA_LIGHT_STATE_BYTES bytes on the device -- E u32 [cell][3] (R, G, B in the table's scale), W u8 [cell], then the latch u32 [8] = {M_R,
 * M_G, M_B, saturated pixels, blocks, cells touched, frames fused, frames latched}; all zero = empty.
 *
 * alva_light_bin adds one RGBA frame (d_rgba, `pitch` bytes per row, both multiples of 4) to the accumulators.  h_calib8 = fx fy cx cy k1
 * k2 p1 p2; h_R_wc9 = the camera-to-world rotation, row-major, or NULL (not tracking); step 2..16; the grid is gw = width / step by gh =
 * height / step blocks (none: nothing is added).
 *   B1 linearise    a channel value v becomes lut[v], the 256-entry uint16 table of alvaar_amd/csrc/light_lut.inc: round(65535 x the sRGB
 *                   transfer function of v / 255)
 *   B2 block sums   per block (gx, gy): S_R, S_G, S_B = the sums of lut[.] over its step x step pixels, and the count of its pixels with
 *                   any of R, G, B >= 250.  (A block's luminance would be Y = (13933 S_R + 46871 S_G + 4732 S_B) >> 16 in 64-bit integers,
 *                   the form E5 uses; no output depends on it per block.)
 *   B3 direction    centre (u, v) = (gx step + step / 2, gy step + step / 2); (uu, vv) = alva_undistort_points' result for ((float) u,
 *                   (float) v), exactly as F1 of alva_depth_fuse; dc = ((uu - cx) / fx, (vv - cy) / fy, 1); dw = R_wc dc, each row (r0 x +
 *                   r1 y) + r2 1
 *   B4 cell         the major axis is the component of dw of largest magnitude, x before y before z on a tie; face = 2 axis + (component <
 *                   0); (a, b) = the other two components in axis order, each divided by the major component's magnitude; i = min(N - 1,
 *                   (int) floor((a + 1) 4.0)), j likewise from b; cell = (face N + j) N + i.  A block whose dw has a non-finite component,
 *                   or whose major component is zero, joins no cell
 *   B5 accumulate   per cell the sums of S_R, S_G, S_B and of step^2 pixels over its blocks; for the frame the three channel sums, the
 *                   pixels, the >= 250 count and the blocks, over all blocks.  With h_R_wc9 == NULL only the frame's words are added to.
 *                   Integer additions: consecutive bins add up
 * alva_light_fuse folds the accumulators into the state and zeroes them.  min_pixels >= 1, 1 <= w_new <= w_max <= 255; d_acc_out (may be
 * NULL): ALVA_LIGHT_ACC_WORDS words that receive the accumulators as they were.
 *   F1 observed     a cell with pixels n >= min_pixels; its means m_c = S_c / n (integer division)
 *   F2 blend        W = 0: E = m, W = w_new.  Otherwise E_c = (E_c W + m_c w_new) / (W + w_new) in 64-bit integers and W = min(w_max, W +
 *                   w_new).  An unobserved cell keeps E and W: what is behind the user is still there
 *   F3 latch        when the frame's pixels n_f > 0: M_c = S_c / n_f, the saturated pixels, the blocks, the number of cells with n > 0,
 *                   and `frames latched` goes up; n_f = 0 keeps the previous latch.  `frames fused` goes up when a cell was observed.
 *                   All accumulators are zero afterwards
 * alva_light_estimate projects the state.
 *   E1 fill         K = the cells with W > 0; A_c = (sum of their E_c) / K (integers); a cell with W = 0 takes A_c.  K = 0: A_c = M_c, code
 *                   1 when a frame was latched, else 5
 *   E2 basis        a table of 9 x 384 doubles, built on the host by the context's first estimate, with + - x / sqrt only.  Per cell (face,
 *                   j, i): a = (2 i + 1) / 8.0 - 1, b likewise from j; r2 = (1 + a a) + b b, r = sqrt(r2); direction d = the vector with
 *                   +1 (face even) or -1 on the face's axis and (a, b) on the other two in axis order, each component divided by r; omega
 *                   = 1 / (r2 r); omega is scaled by (4 pi) / (sum of omega in ascending cell order), pi = 3.141592653589793.  table[k][cell]
 *                   = omega' x Y_k(d): Y0 = 0.282095, Y1 = 0.488603 y, Y2 = 0.488603 z, Y3 = 0.488603 x, Y4 = 1.092548 (x y), Y5 =
 *                   1.092548 (y z), Y6 = 0.315392 (3 (z z) - 1), Y7 = 1.092548 (x z), Y8 = 0.546274 (x x - y y)
 *   E3 projection   L[k][c] = sum over the cells of table[k][cell] x ((double) E_c[cell] / 65535.0): lane l of 64 starts from 0 and adds
 *                   its cells l, l + 64, ..., l + 320 in ascending order, then x[l] += x[l + s] for s = 32, 16, 8, 4, 2, 1.  With K = 0
 *                   L[k] = 0 for k >= 1 (the ambient term in Y00 alone).  h_sh27[3 k + c] = (float) L[k][c]: real spherical harmonics of
 *                   the linear radiance in the world frame, no Condon-Shortley sign (a positive band-1 coefficient = more light from the
 *                   positive axis), c = R, G, B
 *   E4 primary      lum_k = (0.2126 L[k][R] + 0.7152 L[k][G]) + 0.0722 L[k][B]; g = (lum_3, lum_1, lum_2); valid when K > 0 and (g0 g0 + g1
 *                   g1) + g2 g2 > (1e-3 lum_0)^2; d = g / sqrt(that sum): the unit vector towards the strongest directional component;
 *                   h_primary_rgb3[c] = max(0, ((L[3][c] d_x + L[1][c] d_y) + L[2][c] d_z) / 0.488603).  Otherwise all six values are 0.
 *                   The primary light stays inside h_sh27, as in WebXR
 *   E5 frame values h_ambient4 = {(float) (((13933 M_R + 46871 M_G + 4732 M_B) >> 16) / 65535.0), (float) (M_R / M_G), 1, (float) (M_B /
 *                   M_G)} with the divisions in double: the mean linear luminance of the last latched frame (ARCore's ambient-intensity
 *                   mode) and its colour correction, (1, 1, 1) when M_G = 0
 * h_info8 = {code (0 an estimate, 1 no environment yet: only h_ambient4 is meaningful, 5 no frame latched), K, cells the last frame
 * touched, its blocks, its pixels with a channel >= 250, frames fused, primary valid 0 / 1, 0}.
 * alva_light_bin (one launch) and alva_light_fuse (one workgroup) only enqueue; alva_light_estimate is one launch and one host wait. */
#define ALVA_LIGHT_N 8
#define ALVA_LIGHT_CELLS 384
#define ALVA_LIGHT_ACC_WORDS 1544
#define ALVA_LIGHT_STATE_BYTES 5024
int alva_light_bin(alva_ctx *ctx, const uint8_t *d_rgba, size_t pitch, int width, int height, const double *h_calib8,
                   const double *h_R_wc9, int step, uint64_t *d_acc);
int alva_light_fuse(alva_ctx *ctx, uint64_t *d_acc, uint8_t *d_state, int min_pixels, int w_new, int w_max, uint64_t *d_acc_out);
int alva_light_estimate(alva_ctx *ctx, const uint8_t *d_state, float *h_sh27, float *h_primary_dir3, float *h_primary_rgb3,
                        float *h_ambient4, int *h_info8);

/* ---- image detection: where a planar picture the app knows lies in the frame ---------------------------------------------
 * ARCore Augmented Images / ARKit ARImageAnchor / WebXR image-tracking; no reference counterpart (parity is pinned by the numpy
 * restatement tests/image_cases.py).  Two device stages for up to ALVA_IMAGE_MAX images at once; an image j is its ORB keypoints (level-0
 * pixels of the picture) and descriptors, slot j of two device blocks: d_qdesc [n_images][ALVA_IMAGE_QUERY_CAP][32] (16-byte aligned) and
 * d_qxy [n_images][ALVA_IMAGE_QUERY_CAP][2] float, with h_nq[j] <= ALVA_IMAGE_QUERY_CAP rows in use.
 *
 * alva_image_match -- the images' descriptors are the queries, the frame's the train set: d_tdesc [train_cap][32] (16-byte aligned),
 * d_txy [train_cap][2] float (the keypoints, undistorted), train_cap <= ALVA_IMAGE_TRAIN_CAP, of which n_t = clamp(*d_ntrain, 0, train_cap)
 * rows are used -- *d_ntrain is read ON THE DEVICE, so the call queues behind the detector that writes it.  Per image, per query:
 *   best      the train row minimising (popcount(q ^ t), train index)
 *   second    the smallest distance over all other rows (257 when there is none)
 *   accepted  best <= max_dist and (float) best < ratio * (float) second
 *   one-to-one  of the accepted queries of ONE image that share a best row, only the smallest (distance, query index) is kept
 * Output per image j, in ascending query index, k_j pairs: d_match [j][i] = {query, train, distance}, d_xy [j][i] = {x, y of the query
 * keypoint, u, v of the train keypoint} as doubles, d_count [j] = k_j (all device memory, blocks of ALVA_IMAGE_QUERY_CAP rows per image;
 * rows past k_j are not written).  The result depends on nothing but these rules.  Enqueue-only, three launches for all images (the
 * first is skipped when train_cap = 0).
 *
 * alva_image_homography -- counted-consensus RANSAC over 4-pair homographies, then the pose of the picture's plane; one launch for all
 * images, IEEE double in the written order.  Per image j with size (w, h) = h_wh[j] and m = clamp(d_count[j], 0, ALVA_IMAGE_QUERY_CAP)
 * pairs of d_xy [j] (read on the device), W = frame_w, H = frame_h, s = max(W, H) / 2, h_calib4 = fx fy cx cy:
 *   pairs       p_i = ((x - w / 2) / w, (y - h / 2) / w)  (the picture's unit-width frame, origin at its centre),
 *               q_i = ((u - W / 2) / s, (v - H / 2) / s)
 *   too few     m < 4 or m < min_inliers: code 1, nothing else is computed
 *   samples     it = 0 .. num_iterations - 1: words w_j = h(seed ^ ((4 it + j) * 0x9E3779B9)), j = 0 .. 3, uint32 arithmetic, h as for
 *               alva_hit_test (or h_rand4[it][j]); index i_j = (w_j * m) >> 32 (64-bit product); skipped when two indices coincide
 *   model       the 8 x 9 system for (h11 h12 h13 h21 h22 h23 h31 h32), h33 = 1: per sampled pair, in sample order, the u-row
 *               [x y 1 0 0 0 -(x u) -(y u) | u] then the v-row [0 0 0 x y 1 -(x v) -(y v) | v].  Gaussian elimination, for column
 *               k = 0 .. 7: the pivot is the row r >= k with the largest |a[r][k]| (scanned upwards from k, replaced only by a strictly
 *               larger value: the lowest row on ties); the hypothesis is skipped when that |a| is not > 1e-12; rows k and pivot are
 *               exchanged; for r > k: f = a[r][k] / a[k][k], a[r][c] = a[r][c] - f * a[k][c] for c > k.  Back substitution, k = 7 .. 0:
 *               sum = a[k][8], then sum = sum - a[k][c] * h[c] for c = k + 1 .. 7 ascending, h[k] = sum / a[k][k]
 *   sign        skipped unless w = (h31 x + h32 y) + 1 > 0 at all four samples
 *   count       the pairs with w > 0 and dx dx + dy dy <= (double) threshold_px ^ 2, where X = (h11 x + h12 y) + h13,
 *               Y = (h21 x + h22 y) + h23, dx = (X / w - u) * s, dy = (Y / w - v) * s  (the forward transfer error in pixels)
 *   winner      the largest count, the lowest `it` on ties; none survived: code 2.  h_H9 = H row-major, h_mask [i] = 1 for the pairs
 *               the winner counts; count < min_inliers: code 3
 *   pose        column c of A: (sx H[0][c] + ox H[2][c], sy H[1][c] + oy H[2][c], H[2][c]) with sx = s / fx, sy = s / fy,
 *               ox = (W / 2 - cx) / fx, oy = (H / 2 - cy) / fy; n1 = |a1|, n2 = |a2| (each sqrt((x x + y y) + z z), dot products
 *               associated the same way); code 4 unless 0.5 <= n1 / n2 <= 2 and |a1 . a2| / (n1 n2) <= 0.5 (not a rigid view of a
 *               plane); lambda = 1 / sqrt(n1 n2); r1 = a1 / n1; v = a2 - (r1 . a2) r1, r2 = v / |v|; r3 = r1 x r2; t = lambda a3.
 *               h_R9 row-major with the columns r1 r2 r3, h_t3: X_cam = R (p.x, p.y, 0) + t in units of the picture's width
 * h_info8 per image = {code, m, winning iteration (-1: none), its count, 0, 0, 0, 0}; code 0 = a pose.  H and the mask are written for
 * codes 0, 3 and 4, R and t for code 0 only; the rest is zero.  h_mask is [n_images][ALVA_IMAGE_QUERY_CAP].  n_images 1..8,
 * num_iterations 1..4096, threshold_px >= 0.  One workgroup per image, a lane per hypothesis.  Synchronous: one launch, one host wait. */
#define ALVA_IMAGE_MAX 8
#define ALVA_IMAGE_QUERY_CAP 512
#define ALVA_IMAGE_TRAIN_CAP 2048
int alva_image_match(alva_ctx *ctx, int n_images, const uint8_t *d_qdesc, const float *d_qxy, const int *h_nq, const uint8_t *d_tdesc,
                     const float *d_txy, const int *d_ntrain, int train_cap, int max_dist, float ratio, int *d_match, double *d_xy,
                     int *d_count);
int alva_image_homography(alva_ctx *ctx, int n_images, const double *d_xy, const int *d_count, const int *h_wh, int frame_w, int frame_h,
                          const double *h_calib4, int num_iterations, float threshold_px, int min_inliers, uint32_t seed,
                          const uint32_t *h_rand4, double *h_H9, int *h_info8, uint8_t *h_mask, double *h_R9, double *h_t3);

/* ---- f4a: CLAHE ------------------------------------------------------------------------------
 * Replaces cv::createCLAHE(clip_limit, Size(tiles_x, tiles_y))->apply(src, dst) for 8-bit images
 * (imgproc/src/clahe.cpp:120-420), which VisualFrontend::preprocessImage runs when claheEnabled_
 * (src/slam/src/visual_frontend.cpp:16-18 with clip 3 and tiles = size / 50, :678-681; off in the shipped
 * configuration, system.cpp:17).  Bit-exact, including the REFLECT_101 extension for sizes that the grid does not divide.
 * d_dst may not alias d_src.  Enqueue only. */
int alva_clahe(alva_ctx *ctx, const uint8_t *d_src, size_t src_pitch, int width, int height, double clip_limit,
               int tiles_x, int tiles_y, uint8_t *d_dst, size_t dst_pitch);

/* ---- f1: Mapper::matchToMap on a flattened map ----------------------------------------------------
 * Replaces the loops of Mapper::matchToMap(frame, maxProjectionError, distRatio, localMapPointIds)
 * (src/slam/src/mapper.cpp:354-588; caller matchingToLocalMap :334 with state.hpp:62-63) for a consistent map.  The host
 * flattens its containers once per keyframe:
 *   h_calib10        fx fy cx cy k1 k2 p1 p2 imgWidth imgHeight (the shared CameraCalibration)
 *   grid             the frame's keypoint grid as Frame stores it (frame.cpp:250-260, :313-341): cell_size, num_cells_w,
 *                    grid_cells, d_cell_ptr[grid_cells + 1], d_cell_mp = map point INDEX of each stored keypoint, stored order
 *   keyframes        d_kf_q[n_kf][4] (x y z w) and d_kf_t[n_kf][3]: T_cw of every keyframe; frame_kf = the one being matched
 *   map points       d_mp_wpt[n_mp][3], d_mp_is3d[n_mp], observations d_obs_ptr[n_mp + 1] -> d_obs_kf (ascending keyframe
 *                    index = MapPoint::observedKeyframeIds_ order), d_obs_px (the keypoint's px_ in that keyframe),
 *                    d_obs_desc (32 B each, 16-B aligned: MapPoint::mapKeyframeDescriptors_)
 *   d_local          indices of the local map points in the iteration order of frame.localMapPointIds_
 * Output d_match_of_mp[n_mp]: for the map point m of a frame keypoint, the index of the local map point that
 * matchToMap pairs with it (the reference's mapPrevIdNewId[keypointId] = mapPointId), else -1.  Enqueue only. */
int alva_match_to_map(alva_ctx *ctx, const double *h_calib10, int cell_size, int num_cells_w, int grid_cells,
                      const int *d_cell_ptr, const int *d_cell_mp, int n_kf, const double *d_kf_q, const double *d_kf_t,
                      int n_mp, const double *d_mp_wpt, const uint8_t *d_mp_is3d, const int *d_obs_ptr,
                      const int *d_obs_kf, const float *d_obs_px, const uint8_t *d_obs_desc, int frame_kf,
                      int num_keypoints_3d, int n_local, const int *d_local, float max_proj_err, float dist_ratio,
                      int *d_match_of_mp);
/* The same for a LIVE map, in which a keyframe may hold a keypoint it could not describe (within 31 px of the border,
 * src/slam/src/feature_extractor.cpp:191-209): d_mp_has_desc[m] = !MapPoint::desc_.empty() (the gates at mapper.cpp:404, :465),
 * d_obs_has_desc[o] = MapPoint::mapKeyframeDescriptors_ has an entry for that observation's keyframe (its 32-byte slot is ignored
 * otherwise).  NULL flags = every observation carries a descriptor (alva_match_to_map). */
int alva_match_to_map_flags(alva_ctx *ctx, const double *h_calib10, int cell_size, int num_cells_w, int grid_cells,
                            const int *d_cell_ptr, const int *d_cell_mp, int n_kf, const double *d_kf_q, const double *d_kf_t, int n_mp,
                            const double *d_mp_wpt, const uint8_t *d_mp_is3d, const uint8_t *d_mp_has_desc, const int *d_obs_ptr,
                            const int *d_obs_kf, const float *d_obs_px, const uint8_t *d_obs_desc, const uint8_t *d_obs_has_desc,
                            int frame_kf, int num_keypoints_3d, int n_local, const int *d_local, float max_proj_err, float dist_ratio,
                            int *d_match_of_mp);

/* The same call on the map layer's RECORDS instead of a flattened map (round 5; csrc/slam/mp_rec.hpp states the layout: one
 * 1024-byte record per map point -- worldPoint_, is3d_, !desc_.empty(), and per keyframe an entry {keyframe id, flags
 * observed-by / holds-the-keypoint / has-a-descriptor, the keypoint's px_ and unpx_ in that keyframe}, i.e.
 * MapPoint::observedKeyframeIds_ + what Frame::getKeypointById returns for it (src/slam/src/mapper.cpp:487-515) -- in chunks of
 * 4096 records of PINNED host memory that the host edits in place).  The caller names one record slot per table row
 * (d_mp_slot); a gather kernel reads the rows' records out of host memory (d_record_chunks: device-readable table of the chunks'
 * addresses), keeps the observations whose keyframe is listed in d_kf_ids (ascending ids; d_kf_q / d_kf_t their T_cw;
 * frame_kf_index / frame_kf_id name the keyframe being matched) and holds the keypoint, and takes the descriptors from the
 * device-resident descriptor tables of the same slots (d_desc_tables = alva_medoid_tables(): mapKeyframeDescriptors_, what
 * MapPoint::computeMinDescDist iterates, map_point.cpp:206-222).  Grid, local list, thresholds and output as above.  Enqueue only. */
int alva_match_to_map_records(alva_ctx *ctx, const double *h_calib10, int cell_size, int num_cells_w, int grid_cells,
                              const int *d_cell_ptr, const int *d_cell_mp, int n_kf, const int *d_kf_ids, const double *d_kf_q,
                              const double *d_kf_t, int frame_kf_index, int frame_kf_id, int n_mp, const int *d_mp_slot,
                              const void *const *d_record_chunks, const void *d_desc_tables, int num_keypoints_3d, int n_local,
                              const int *d_local, float max_proj_err, float dist_ratio, int *d_match_of_mp);

/* ---- f4b: lens distortion paths of CameraCalibration --------------------------------------
 * alva_undistort_points replaces CameraCalibration::undistortImagePoint (src/slam/src/camera_calibration.cpp:56-72) =
 * cv::undistortPoints(pts, out, K, D, R = K) with D = (k1, k2, p1, p2), 5 fixed iterations
 * (calib3d/src/undistort.dispatch.cpp:384-556): pixel in, undistorted pixel out (n x 2 f32 each).
 * alva_project_dist replaces CameraCalibration::projectCamToImageDist (:34-54) = cv::projectPoints of (x/z, y/z, 1)
 * rounded to float, zero rvec / tvec (calib3d/src/calibration.cpp:522-): camera-frame points (n x 3 f64) in, distorted
 * pixels (n x 2 f32) out.  Both bit-exact; both are used by the reference even when the coefficients are zero.
 * Enqueue only. */
int alva_undistort_points(alva_ctx *ctx, const float *d_px, int n, double fx, double fy, double cx, double cy, double k1,
                          double k2, double p1, double p2, float *d_out);
int alva_project_dist(alva_ctx *ctx, const double *d_cam_pts, int n, double fx, double fy, double cx, double cy,
                      double k1, double k2, double p1, double p2, float *d_out);

/* ---- f2a: triangulation of a new keyframe's 2-D keypoints -------------------------------------
 * Replaces the per-keypoint arithmetic of Mapper::triangulateTemporal (src/slam/src/mapper.cpp:222-287):
 * MultiViewGeometry::triangulate (= opengv::triangulation::triangulate2, opengv/src/triangulation/methods.cpp:67-90),
 * the rotation-compensated parallax (:246-248), the cheirality gate z < 0.1 (:256) and the reprojection gate (:266-272).
 * The caller groups the points by the keyframe that first observed them: d_T holds one block of 36 doubles per group,
 * { R_lr[9], t_lr[3], R_rl[9], t_rl[3], R_wl[9], t_wl[3] } row-major (l = that keyframe, r = the new keyframe,
 * w = world; T_lr = T_lw * T_wr, :226-228), d_group[i] selects the block of point i.  d_bv_*: unit bearings (n x 3 f64),
 * d_unpx_*: undistorted pixels (n x 2 f32).  Outputs per point: point in the l camera, world point, inverse depth
 * 1 / z_l, status (0 = accepted, 1 = behind a camera, 2 = reprojection error), parallax in pixels (the reference drops
 * the observation of rejected points whose parallax exceeds 20, :258-262/:274-278 -- host bookkeeping).  Enqueue only. */
int alva_triangulate(alva_ctx *ctx, int n, const double *d_T, int n_groups, const int *d_group, const double *d_bv_l,
                     const double *d_bv_r, const float *d_unpx_l, const float *d_unpx_r, double fx, double fy, double cx,
                     double cy, float max_reproj_err, double *d_lpt, double *d_wpt, double *d_inv_depth,
                     uint8_t *d_status, double *d_parallax);

/* ---- per-frame driver: the caller of a2-a9 -------------------------------------------------------------------
 * Mirrors the order of VisualFrontend::trackMono (src/slam/src/visual_frontend.cpp:83-150): preprocessImage (:672-698)
 * -> kltTracking (:152-243) -> computePose (:245-417), plus the keyframe branch's feature work
 * (MapManager::extractKeypoints, map_manager.cpp:196-231, with the detector the north_star names, and BFMatcher
 * matching against the previous frame, map_point.cpp:106-212).  The reference runs them back to back on one CPU
 * thread; here the detector + matcher run on a second HIP stream while the first tracks and solves the pose.  One host
 * wait for the pose, one for the keypoint count.  All inputs are device pointers: d_rgba the frame; d_pts n_pts x 2
 * float keypoints to track from the previous frame; d_bearings / d_uv / d_wpts n_corr 2-D/3-D correspondences for the
 * pose (doubles, as alva_compute_pose).  *h_pose_status as alva_compute_pose.
 * d_rgba (and d_rgba_next, which shares rgba_pitch): as alva_pyramid_build_from_rgba -- rgba_pitch >= 4 * width, rgba_pitch % 16 == 0,
 * 16-byte aligned; the same for every d_rgba[c] of alva_track_batch_step / _step_detect with their one rgba_pitch. */
typedef struct alva_frontend alva_frontend;
int alva_frontend_create(int device, int width, int height, int max_tracked, int orb_features, alva_frontend **out);
void alva_frontend_destroy(alva_frontend *fe);
int alva_frontend_track(alva_frontend *fe, const uint8_t *d_rgba, size_t rgba_pitch, const float *d_pts, int n_pts,
                        const double *d_bearings, const double *d_uv, const double *d_wpts, int n_corr, float fx,
                        float fy, float cx, float cy, double *h_pose7, int *h_pose_status, int *h_n_keypoints);
/* The same with one frame of look-ahead: d_rgba_next (may be NULL) is the frame the NEXT call will pass as d_rgba; its gray
 * image and pyramid are built on a third HIP stream while this frame is tracked, so preprocessImage leaves the dependent chain
 * pyramid -> KLT -> P3P -> PnP.  Contract: d_rgba_next is read asynchronously from now until the NEXT alva_frontend_track* call on this
 * object has returned, so its contents must not change in between, and "the same pointer" on that next call means "the same, unchanged
 * contents" (the look-ahead result is used as is).  A next call with any other d_rgba waits for the pending look-ahead build and
 * rebuilds.  Results are identical to alva_frontend_track. */
int alva_frontend_track_ahead(alva_frontend *fe, const uint8_t *d_rgba, size_t rgba_pitch, const uint8_t *d_rgba_next,
                              const float *d_pts, int n_pts, const double *d_bearings, const double *d_uv, const double *d_wpts,
                              int n_corr, float fx, float fy, float cx, float cy, double *h_pose7, int *h_pose_status,
                              int *h_n_keypoints);
/* Device-resident results of the last alva_frontend_track: tracked positions (n_pts x 2) + status, ORB keypoints
 * (n x 6) + descriptors (n x 32), matches of the n descriptors against the previous frame's.  Any may be NULL.
 * Call alva_frontend_sync first if anything but later alva_frontend_* calls is going to read them. */
int alva_frontend_results(alva_frontend *fe, const float **d_tracked, const uint8_t **d_track_status,
                          const float **d_keypoints, const uint8_t **d_descriptors, const int **d_match_idx,
                          const int **d_match_dist);
int alva_frontend_sync(alva_frontend *fe);
/* Measurement helper: n_streams independent camera streams on one GPU, one host thread per stream, each running `steps`
 * alva_frontend_track calls on its own alva_frontend (d_frames[s * ring + k] = frame k of stream s; the other inputs are
 * per-stream arrays of device pointers).  *h_seconds = wall time from the common start to the last stream's finish. */
int alva_frontend_run_many(alva_frontend **fes, int n_streams, int steps, int warmup, const uint8_t *const *d_frames,
                           int ring, size_t rgba_pitch, const float *const *d_pts, int n_pts,
                           const double *const *d_bearings, const double *const *d_uv, const double *const *d_wpts,
                           int n_corr, float fx, float fy, float cx, float cy, double *h_seconds, int *h_accepted);

/* a4 for many cameras: FeatureTracker::fbKltTracking (src/slam/src/feature_tracker.cpp:5-111) of `count` independent
 * (previous, current) pyramid pairs in ONE launch; arguments per pair as alva_fbklt_track (d_prior[c] in/out), pyramids may differ
 * in size.  lanes_per_keypoint selects the wave layout: 5 (a lane per column pair of the 9x9 window, 12 keypoints per wave: the
 * fastest for large batches), 8 (the same with 8 keypoints per wave) or 64 (alva_fbklt_track's layout); results are bit-identical
 * for all three, any other value is ALVA_ERR_ARG.  Enqueue-only, like alva_fbklt_track. */
int alva_fbklt_track_batch(alva_ctx *ctx, const alva_pyramid *const *prev, const alva_pyramid *const *curr, int count,
                           int num_levels, float err_thresh, float fb_dist, int max_iters, float eps,
                           const float *const *d_pts, float *const *d_prior, uint8_t *const *d_status, const int *n,
                           int lanes_per_keypoint);

/* ---- a1 for a rig: VisualFrontend::trackMono of B lock-step cameras, one launch per stage for all of them ----------------
 * The per-frame path of src/slam/src/visual_frontend.cpp:83-150 -- preprocessImage (:672-698), kltTracking (:152-243),
 * computePose (:245-417); the detector is the keyframe branch's, not this path's -- for `cameras` independent cameras that deliver
 * their frames together: 5 launches build all gray images + LK pyramids, 1 launch tracks every camera's keypoints, 4 launches solve
 * every camera's P3P-LMedS -> PnP behind it, and one host synchronisation returns the poses.  Each camera has its own frame, keypoints
 * (n_pts[c] <= max_tracked), correspondences (n_corr[c] <= max_corr <= 7168) and state; results are identical to `cameras`
 * alva_frontend_track calls.  d_rgba / d_pts / d_bearings / d_uv / d_wpts are host arrays of `cameras` device pointers;
 * h_pose7 is [cameras][7] (written where status >= 1 and the solver produced a pose), h_pose_status [cameras] as alva_compute_pose. */
typedef struct alva_track_batch alva_track_batch;
int alva_track_batch_create(int device, int width, int height, int cameras, int max_tracked, int max_corr, alva_track_batch **out);
void alva_track_batch_destroy(alva_track_batch *tb);
int alva_track_batch_step(alva_track_batch *tb, const uint8_t *const *d_rgba, size_t rgba_pitch, const float *const *d_pts,
                          const int *n_pts, const double *const *d_bearings, const double *const *d_uv,
                          const double *const *d_wpts, const int *n_corr, float fx, float fy, float cx, float cy, double *h_pose7,
                          int *h_pose_status);
/* Optional: the keyframe branch's feature work for every camera, as alva_frontend_track does for one -- cv::ORB::detectAndCompute
 * (orb_features, 1.2, 8 levels, FAST 20) on the frame's gray image and a brute-force Hamming match against the camera's previous
 * descriptors, batched over the cameras on a third HIP stream (12 + 2 launches for all cameras).  Enable before the first step;
 * alva_track_batch_step_detect then also returns the per-camera keypoint counts, alva_track_batch_detections the device-resident
 * keypoints [n][6], descriptors [n][32] and matches (index / distance into the camera's previous descriptor set). */
int alva_track_batch_enable_detector(alva_track_batch *tb, int orb_features);
int alva_track_batch_step_detect(alva_track_batch *tb, const uint8_t *const *d_rgba, size_t rgba_pitch, const float *const *d_pts,
                                 const int *n_pts, const double *const *d_bearings, const double *const *d_uv,
                                 const double *const *d_wpts, const int *n_corr, float fx, float fy, float cx, float cy,
                                 double *h_pose7, int *h_pose_status, int *h_n_keypoints);
int alva_track_batch_detections(alva_track_batch *tb, int cam, const float **d_keypoints, const uint8_t **d_descriptors,
                                const int **d_match_idx, const int **d_match_dist);
/* device-resident kltTracking result of one camera from the last step: [n_pts][2] positions, [n_pts] status */
int alva_track_batch_results(alva_track_batch *tb, int cam, const float **d_tracked, const uint8_t **d_track_status);
/* Tuning knob of the tracking launch: lanes of a wavefront per keypoint, 5 (default, see alva_fbklt_track_batch), 8 or 64 (the
 * single-camera kernel's layout).  Results are identical for all three.  The environment variable ALVA_KLT_BATCH_LANES sets the
 * default at creation. */
int alva_track_batch_set_klt_lanes(alva_track_batch *tb, int lanes);
/* steps done, and how often a camera had to be re-solved by the single-camera call because the first 128 samples of its P3P
 * stream held fewer than 100 non-degenerate ones (the reference keeps drawing, Lmeds.hpp:67-92) */
int alva_track_batch_stats(alva_track_batch *tb, long *frames, long *single_camera_fallbacks);
/* the context (stream) the batch runs on, e.g. for alva_prof_* or alva_ctx_sync */
alva_ctx *alva_track_batch_ctx(alva_track_batch *tb);

/* ---- a10-a13: local bundle adjustment ---------------------------------------------------------
 * Replaces the solve inside Optimizer::localBA (src/slam/src/optimizer.cpp:251-262 on the problem
 * built at :20-247): Levenberg-Marquardt + Huber, Schur complement on the point blocks,
 * anchored-inverse-depth (inv_depth=1, state.hpp:74 default) or XYZ points; cost functions
 * src/slam/src/ceres_parametrization.cpp:6-94,157-268.  Flat problem description (host arrays):
 *   h_poses[n_kf][7] in/out, h_kf_const[n_kf], h_calib[4],
 *   inv_depth=1: h_pt_anchor_kf[n_pt], h_pt_anchor_uv[n_pt][2], h_pt_param[n_pt]    in/out
 *   inv_depth=0: h_pt_param[n_pt][3] in/out
 *   h_obs_kf[n_obs], h_obs_pt[n_obs], h_obs_uv[n_obs][2]
 * Outputs: h_chi2[n_obs], h_depth_pos[n_obs] at the last evaluated point (what the reference's
 * outlier sweep reads, optimizer.cpp:266-309), h_info[0..3] = {#iterations, initial cost, final cost,
 * #successful steps}.
 * n_kf <= ALVA_LOCAL_BA_MAX_KF for alva_local_ba and alva_local_ba_batch (alva_local_ba_csr: 32): more is refused with ALVA_ERR_ARG
 * before anything is launched.  n_pt == 0 and n_obs == 0 are accepted (nothing moves, *h_ok = 1), and so is a problem without a free
 * keyframe (only the points move). */
#define ALVA_LOCAL_BA_MAX_KF 128
int alva_local_ba(alva_ctx *ctx, int n_kf, double *h_poses, const uint8_t *h_kf_const, const double *h_calib,
                  int inv_depth, int n_pt, const int *h_pt_anchor_kf, const double *h_pt_anchor_uv,
                  double *h_pt_param, int n_obs, const int *h_obs_kf, const int *h_obs_pt,
                  const double *h_obs_uv, int max_iters, double function_tolerance, double huber_chi2,
                  double *h_chi2, uint8_t *h_depth_pos, double *h_info, int *h_ok);

/* The same solve for a caller that holds its observations GROUPED BY POINT (round 5: the map layer's localBA build emits them that
 * way): h_pt_ptr[n_pt + 1] delimits each point's residual blocks in h_obs_kf / h_obs_uv (anchored inverse depth only).  The
 * (observing keyframe, anchor keyframe) grouping that the camera-block assembly needs is built on the DEVICE (a stable counting
 * sort, identical to the host-built one: results are bit-identical to alva_local_ba on the same problem), and the outlier sweep's
 * test of Optimizer::localBA (src/slam/src/optimizer.cpp:266-309: chi2 > chi2_threshold, or the point behind the camera) comes back as
 * one BIT per residual block (h_bad_bits: (n_obs + 63) / 64 words; *h_n_bad their count) instead of the chi2 / depth arrays.
 * n_kf <= 32.  Synchronous. */
int alva_local_ba_csr(alva_ctx *ctx, int n_kf, double *h_poses, const uint8_t *h_kf_const, const double *h_calib, int n_pt,
                      const int *h_pt_ptr, const int *h_pt_anchor_kf, const double *h_pt_anchor_uv, double *h_pt_inv_depth, int n_obs,
                      const int *h_obs_kf, const double *h_obs_uv, int max_iters, double function_tolerance, double huber_chi2,
                      double chi2_threshold, unsigned long long *h_bad_bits, int *h_n_bad, double *h_info, int *h_ok);

/* `count` independent local-BA problems (anchored inverse depth) with ONE set of launches per LM iteration: a rig's cameras or a
 * server's sessions, each with its own keyframes / points / observations (ragged sizes).  Every kernel carries the problem in a grid
 * dimension -- the reduced camera systems are factored on `count` compute units at once, the Schur-complement GEMMs form one grouped
 * FP64-MFMA launch -- and every problem has its own minimiser state on the device, which steps its trust region separately (problems
 * stop at different iterations; the host enqueues iterations until all have stopped).  Every problem's result is BIT-IDENTICAL to its own alva_local_ba call.  Arguments: arrays of
 * `count` sizes / host pointers with alva_local_ba's meaning; h_calib[4] shared; h_info [count][4]; h_ok [count].  At most 21 free
 * keyframes per problem (the reduced system is factored in LDS: 6 x free, rounded up to a multiple of 16, <= 128); n_pt > 0 and n_obs > 0
 * for every problem.  Anything else is refused with ALVA_ERR_ARG before anything is launched. */
int alva_local_ba_batch(alva_ctx *ctx, int count, const int *n_kf, double *const *h_poses, const uint8_t *const *h_kf_const,
                        const double *h_calib, const int *n_pt, const int *const *h_pt_anchor_kf, const double *const *h_pt_anchor_uv,
                        double *const *h_pt_param, const int *n_obs, const int *const *h_obs_kf, const int *const *h_obs_pt,
                        const double *const *h_obs_uv, int max_iters, double function_tolerance, double huber_chi2, double *const *h_chi2,
                        uint8_t *const *h_depth_pos, double *h_info, int *h_ok);

/* ---- measured ceilings for the roofline lines of bench.py (MI355X_MICROARCH.md lists neither): the FP64 matrix rate of
 * v_mfma_f64_16x16x4_f64 in TFLOP/s and the plain integer VALU rate (xor / popcount-accumulate / add) in 1e12 lane-operations/s. */
int alva_microbench_peaks(alva_ctx *ctx, double *h_tflops_mfma_f64, double *h_tops_valu_int);
/* Launch latency for the end-to-end bound of a frame (bench.py "bounds"): microseconds per kernel of `chain` dependent empty
 * launches on the context's stream, and the round trip of one empty launch + stream synchronisation.  Synchronous. */
int alva_microbench_launch(alva_ctx *ctx, int chain, double *h_us_per_dependent_launch, double *h_us_launch_sync_roundtrip);
/* Debug (no reference counterpart): phase stamps of the pose kernels (100 MHz wall clock), recorded only when the process runs with
 * ALVA_KSTAMPS=1: 4096 x u64 -- k_p3p 8 per workgroup from entry 0, k_pnp sequentially from entry 2048; cleared by the call. */
int alva_debug_kstamps(unsigned long long *h_out);
/* Debug: with ALVA_KLT_STAMPS=1 in the environment the tracker launch of the System path (k_track_klt) records, per slot of the frame
 * container, its wall time in the kernel (100 MHz ticks, bits 0-31) | result code << 32 | tracked-from-projection << 36 | retried << 37;
 * copies the 16384 entries of the last launch to the host.  ALVA_ERR_STATE without the variable. */
int alva_debug_klt_stamps(unsigned long long *h_out16384);

/* f1: MapPoint's descriptor tables -- mapKeyframeDescriptors_, mapDescriptorsDist_, desc_ -- on the device, edited by
 * REPLAYING a log of MapPoint::addDesc (map_point.cpp:131-181), the descriptor half of MapPoint::removeObservedKeyframeId (:93-128),
 * the release when the last observation goes (:80-91) and "new map point" operations.  A store holds one fixed-size table per map point
 * SLOT (alva_medoid_table_bytes()); operations are 64-byte records (alva_medoid_op_bytes(): int op {0 add, 1 remove, 2 clear, 3 reset},
 * int keyframe, int rehash_to (bucket count of the rehash this insert triggers in the reference's unordered_map, 0 = none), int next
 * (index of the same map point's next operation, -1 = last), uint8 descriptor[32], 16 bytes padding).  alva_medoid_replay ENQUEUES
 * the log on the context's stream (one wavefront per listed map point: mp_slot[i] with its chain head first_op[i]; `slots` = highest
 * slot in use + 1); alva_medoid_export waits and returns per requested slot desc_ (32 B), !desc_.empty(), {#descriptors, keyframe
 * desc_ was taken from, overflow flag}; alva_medoid_dump copies one raw table (tests; layout in csrc/slam/medoid_table.hpp). */
typedef struct alva_medoid_store alva_medoid_store;
size_t alva_medoid_table_bytes(void);
size_t alva_medoid_op_bytes(void);
int alva_medoid_store_create(alva_ctx *ctx, alva_medoid_store **out);
void alva_medoid_store_destroy(alva_medoid_store *store);
int alva_medoid_replay(alva_medoid_store *store, int n_ops, const void *ops, int n_mp, const int *mp_slot, const int *first_op, int slots);
int alva_medoid_export(alva_medoid_store *store, int n, const int *mp_slot, uint8_t *h_desc32, uint8_t *h_valid, int *h_info3);
int alva_medoid_dump(alva_medoid_store *store, int mp_slot, void *h_table, size_t bytes);
/* the device array of tables (valid until the next alva_medoid_replay grows it; NULL before the first replay): kernels that read the
 * descriptors in place (alva_match_to_map_records) */
const void *alva_medoid_tables(alva_medoid_store *store);
/* The shared-map exchange's record block from the resident data (round 5): one thread per record slot 0 .. n_slots - 1 reads the
 * map-point record's header (csrc/slam/mp_rec.hpp; d_record_chunks as in alva_match_to_map_records) and the descriptor medoid of the
 * same slot's table; every 3-D point with a descriptor becomes one 64-byte row {int32 stream, int32 point id, f64 xyz[3], u8 desc[32]}
 * of d_out [capacity][64] (device), in no particular order; unused rows get point id -1.  *h_count = points found (> capacity: only
 * `capacity` of them were written -- an arbitrary subset).  Semantics of the exchange: MapManager::mergeMapPoints,
 * src/slam/src/map_manager.cpp:428-513 (parity unpinned: the reference has one map).  Synchronous. */
int alva_pack_map_records(alva_medoid_store *store, const void *const *d_record_chunks, int n_slots, int stream_id, int capacity,
                          uint8_t *d_out, int *h_count);

/* ---- relocalization after tracking loss (no reference counterpart: the reference resets its map; ORB-SLAM2 / OV²SLAM match against
 * the map they keep).  A global k = 2 Hamming match of n_query frame descriptors (d_qdesc [n][32], 16-byte aligned; d_qvalid [n] or
 * NULL = all valid) against n_rows map rows in alva_pack_map_records' 64-byte layout (id = -1: unused row; any row order).  Per valid
 * query: best = the row minimising (distance, map-point id) over rows with id >= 0, second = the smallest distance over all other such
 * rows (257 when none); accepted when best <= max_dist and (float) best < ratio * (float) second.  One-to-one: of the accepted queries
 * sharing a best row only the smallest (distance, query index) is kept.  Output in ascending query index: d_match [n_query][4] =
 * {query, row, id, distance}, *d_count (device memory) = the number of pairs, and -- each where non-NULL -- the pose solve's
 * correspondences gathered per pair: d_bv [3] from d_qbv, d_uv [2] (double) from d_qunpx, d_wpt [3] = the row's xyz (the inputs of
 * alva_compute_pose).  The result does not depend on the row order.  Enqueue-only, three launches. */
int alva_reloc_match(alva_ctx *ctx, const uint8_t *d_qdesc, const uint8_t *d_qvalid, int n_query, const double *d_qbv, const float *d_qunpx,
                     const uint8_t *d_rows, int n_rows, int max_dist, float ratio, int *d_match, int *d_count, double *d_bv, double *d_uv,
                     double *d_wpt);

/* ---- §8(e) optional shared-map merge (north_star extension, PARITY UNPINNED: the reference has one map) -----------------------
 * n records sorted by (stream, point id): a record is absorbed by the earliest SURVIVING record of another stream within max_dist
 * (metres) whose descriptor is within max_hamming bits (smallest distance wins, earliest record on ties) -- the intent of
 * MapManager::mergeMapPoints (src/slam/src/map_manager.cpp:428-513) with mapMaxDescriptorDistance_ (state.hpp:60).  d_keep[i] = 1 for
 * survivors, d_absorbed_by[i] = index of the absorbing record or -1.  *h_rounds = fixed-point rounds taken.  0 <= max_hamming <= 256;
 * n <= 2^22 records (a candidate is one int: nine bits of distance above the record index); more than 32 candidates for one record
 * is ALVA_ERR_STATE.  Synchronous. */
int alva_fuse_map_points(alva_ctx *ctx, int n, const int *d_stream, const double *d_xyz, const uint8_t *d_desc, double max_dist,
                         int max_hamming, uint8_t *d_keep, int *d_absorbed_by, int *h_rounds);

#ifdef __cplusplus
}
#endif
#endif /* ALVAAR_HIP_H */
