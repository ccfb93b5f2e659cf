/*
 * alvaar_system.h -- the reference's public surface (src/slam/src/system.hpp:24-38, bound to JS at
 * src/slam/src/embind.cpp:9-19) as a C ABI with POINTER-typed arguments, plus `alva::System`, a header-only C++
 * class with the reference's method names whose `int`-typed twins keep the wasm32 calling convention
 * (src/slam/src/system.cpp:59-61,108-109: heap byte offsets passed as int).
 *
 * Status codes of find_camera_pose (system.cpp:163-174): 1 = pose valid, 2 = tracker reset this frame,
 * 3 = still initialising, 4 = tracking lost, relocalizing against the kept map (only with alva_system_set_relocalization; the pose
 * written is that of the last status-1 frame).  The pose is written even when the status is not 1 (system.cpp:118).
 * Pose layout (src/slam/src/utils.cpp:3-27): p[0..2] = R row 0, p[4..6] = R row 1, p[8..10] = R row 2,
 * p[12..14] = t, p[3] = p[7] = p[11] = 0, p[15] = 1 (Twc).
 *
 * Scope (DESIGN.md "System surface"): the WHOLE per-frame path of System::processCameraPose (system.cpp:156-175) --
 * VisualFrontend::track/process (motion-model priors, two-pass forward-backward KLT, P3P-LMedS + robust PnP, pose-failure
 * handling, five-point initialisation, keyframe policy), MapManager::createKeyframe (grid detection + ORB description, descriptor
 * medoids), Mapper::processNewKeyframe (triangulation, covisibility, guided matching to the local map + map-point merging,
 * local bundle adjustment with outlier sweep and write-back, map-point and keyframe culling).  The bookkeeping is host code
 * (alvaar_amd/csrc/slam/), every numeric stage runs on the GPU through include/alvaar_hip.h.  Lens distortion (k1 k2 p1 p2) and CLAHE
 * are wired (camera_calibration.cpp:34-72, visual_frontend.cpp:678-681).  find_plane runs the plane fit the reference intends
 * (alva_find_plane; the reference function itself computes on reinterpreted memory, so its parity is unpinned).
 * Known deviations: a timestamp older than the previous one resets the tracker (status 2) instead of exit(-1)
 * (visual_frontend.hpp:46-50); P3P-LMedS is solved on the first 19000 3-D keypoints of a frame when there are more (a 3840x2160 frame has ~10 k).
 */
#ifndef ALVAAR_SYSTEM_H
#define ALVAAR_SYSTEM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct alva_system alva_system;

int alva_system_create(int device, alva_system **out);
void alva_system_destroy(alva_system *sys);
/* System::configure (system.cpp:13-40): cell size 40, CLAHE off, clock-seeded sampling.  A failed call leaves the object
 * unconfigured (every later call returns ALVA_ERR_ARG) and alva_system_last_error() says why. */
int alva_system_configure(alva_system *sys, int width, int height, double fx, double fy, double cx, double cy, double k1,
                          double k2, double p1, double p2);
/* The same with the three settings System::configure hard-codes (system.cpp:15-19; state.hpp:67): the keypoint cell size
 * (12 at 640x480 = the 2000-keypoint workload of BASELINE configs[1]), CLAHE, and random_sampling = 0 for the fixed sample
 * streams of OpenGV (seed 12345) that the differential tests use. */
int alva_system_configure_ex(alva_system *sys, int width, int height, double fx, double fy, double cx, double cy, double k1,
                             double k2, double p1, double p2, int cell_size, int clahe_enabled, int random_sampling);
void alva_system_reset(alva_system *sys);
/* Relocalization after tracking loss (no reference counterpart; off by default, and off changes nothing).  Enabled, the fourth
 * consecutive pose failure (visual_frontend.cpp:73-92) no longer resets the map: the system enters LOST, the map is frozen, and every
 * frame returns status 4 while it is matched globally against the map's 3-D points (k = 2 Hamming with a ratio test, alva_reloc_match)
 * and an absolute pose is solved (P3P-LMedS -> robust PnP).  A pose with >= 30 inliers makes that frame a keyframe of the SAME map
 * (status 1: keyframe and map-point ids continue, anchors keep their world frame).  max_lost_frames > 0: after that many frames with
 * status 4 the next failed attempt resets as the reference would (status 2); 0 = stay LOST until relocalized or alva_system_reset.
 * Every other reset trigger (failed initialisation, a timestamp going back) still resets.  Allowed before or after configure; turning it
 * off while LOST resets. */
int alva_system_set_relocalization(alva_system *sys, int enabled, int max_lost_frames);
/* out4 = {frames in the current LOST episode (0 when tracking), relocalization attempts, successes, inliers of the last attempt} */
int alva_system_relocalization_stats(alva_system *sys, long *out4);
/* System::findCameraPose (system.cpp:106-121).  h_rgba: width*height*4 bytes, caller-owned, read-only to the callee and not retained
 * beyond the call; h_pose: float[16].  By default the frame is copied through a pinned staging buffer. */
int alva_system_find_camera_pose(alva_system *sys, const uint8_t *h_rgba, float *h_pose);
/* ---- many sessions on a few host threads (no reference counterpart: the reference is one System per process / worker).  A group
 * owns n_threads worker threads; alva_system_group_find_camera_pose_device runs ONE frame of each of `count` configured systems
 * (session i: frame d_rgba[i] in device memory, pose -> h_poses[16 i ..], status / error code -> h_status[i]) and returns when all are
 * done.  Sessions are fibers on the workers: a session's waits for the GPU hand the thread to the worker's next session, so the
 * threads only execute map-layer work and the GPU sees the sessions' streams side by side.  Every session's results equal its solo run
 * bit for bit.  Systems must not be used from other threads during the call. */
typedef struct alva_system_group alva_system_group;
int alva_system_group_create(int n_threads, alva_system_group **out);
void alva_system_group_destroy(alva_system_group *group);
/* Streams for sessions to SHARE: the GPU's command processor slows down sharply beyond a handful of concurrently active hardware queues
 * (measured: empty launches 2.5 us each on 1 - 4 streams, 26 us each on 8), so a group's sessions run on a few streams rather than one
 * each.  alva_system_group_stream returns (creating it on first use) the group's stream number `index`; alva_system_set_stream makes a
 * system build its stages on that stream at its next alva_system_configure*.  The systems must be destroyed before the group. */
int alva_system_group_stream(alva_system_group *group, int device, int index, void **out_stream);
int alva_system_set_stream(alva_system *sys, void *hip_stream);
int alva_system_group_find_camera_pose_device(alva_system_group *group, int count, alva_system *const *systems, const uint8_t *const *d_rgba,
                                              double timestamp_ms, float *h_poses, int *h_status);
/* LOCK-STEP LAUNCHES (default on; ALVA_GROUP_LOCKSTEP=0 or alva_system_group_set_lockstep(group, 0) turns them off).  The group owns
 * `lanes` streams of its own (default 4; ALVA_GROUP_LANES / alva_system_group_set_lanes; 0 = none); session i of a call runs on worker
 * i % n_threads and belongs to lane (i + i / n_threads) % lanes.  The seven launches of a tracking frame -- gray + pyramid level 0, pyramid,
 * slot table, fb-KLT, compaction, P3P-LMedS, PnP -- are issued ONCE PER KIND for all sessions of a lane (blockIdx.y = session; the
 * argument blocks ride in the kernel arguments) on the lane's stream, by the thread whose session completes the set, instead of seven per
 * session: S side-by-side chains of small kernels saturate the GPU's command path and wave slots long before its arithmetic.  A worker
 * holds sessions of different lanes and does the host half of one lane's sessions while another lane's launches run.  Everything else a
 * session launches (keyframe stages, local BA) stays on the session's own stream.  Results are unchanged bit for bit (same arithmetic
 * per slot / hypothesis / correspondence).  alva_system_group_launch_stats: out2 = {combined launches issued, session launches they
 * carried}. */
int alva_system_group_set_lanes(alva_system_group *group, int lanes);
/* summed over the workers since the last reset: out4 = {seconds inside group steps, seconds inside session slices that did more than
 * look at a completion word, slices, slices that did work} -- how much of the workers' time is map-layer work and how much is waiting */
int alva_system_group_time_stats(alva_system_group *group, double *out4, int reset);
int alva_system_group_set_lockstep(alva_system_group *group, int on);
int alva_system_group_launch_stats(alva_system_group *group, long *out2);
/* Optional, for a caller that reuses ONE frame buffer the way src/system.js reuses its memImg (:63-67, :175): page-lock and map
 * `bytes` (>= width*height*4, 16-byte aligned) at h_rgba.  Frames passed from inside the registered range are then read in place
 * over PCIe by the gray / pyramid kernel (no staging copy, no copy command); every find_camera_pose* call still returns only after the
 * GPU has finished reading the buffer.  The registration is the caller's promise that the memory stays allocated until
 * alva_system_unregister_frame_buffer / alva_system_configure / alva_system_destroy; one buffer per system (a second call replaces
 * the first).  Must be called after alva_system_configure. */
int alva_system_register_frame_buffer(alva_system *sys, const uint8_t *h_rgba, size_t bytes);
int alva_system_unregister_frame_buffer(alva_system *sys);
/* The ONE frame buffer of src/system.js (memImg, :63-67) placed in DEVICE memory that the host can write (round 5): the whole of an
 * MI355X's memory is visible to the CPU over the PCIe BAR, write-combined, so memImg.write(frame) (:175) -- one copy of the frame, which
 * the caller performs anyway -- IS the upload: *h_writable receives a pointer the caller stores the frame through (ordinary stores /
 * memcpy; never read through it: a load crosses the bus), and a frame passed to alva_system_find_camera_pose* from inside this buffer
 * is read by the gray / pyramid kernel straight out of HBM, exactly like alva_system_find_camera_pose_device's.  Freed by
 * alva_system_configure / alva_system_destroy.  ALVA_ERR_STATE where such memory cannot be had (use alva_system_register_frame_buffer). */
int alva_system_alloc_frame_buffer(alva_system *sys, size_t bytes, uint8_t **h_writable);
/* The same with the frame's timestamp (milliseconds) as an argument instead of the system clock (system.cpp:114): the
 * constant-velocity motion model (visual_frontend.hpp:11-68) is the only consumer. */
int alva_system_find_camera_pose_ts(alva_system *sys, const uint8_t *h_rgba, double timestamp_ms, float *h_pose);
/* The same for a frame that already lives in DEVICE memory of the system's GPU (width*height*4 bytes, 16-byte aligned): no PCIe
 * upload.  For capture pipelines that deliver into HBM, and for bench.py's timed loop (frames resident in HBM).  The frame is PACKED:
 * its rows are width*4 bytes apart, there is no pitch argument (a padded frame goes through the stage calls of alvaar_hip.h). */
int alva_system_find_camera_pose_device(alva_system *sys, const uint8_t *d_rgba, double timestamp_ms, float *h_pose);
/* Look-ahead for frames in device memory (no reference counterpart: the reference is handed one frame per call).  Called BEFORE
 * alva_system_find_camera_pose_device(frame k), it names frame k+1 (device memory that stays valid and unchanged until that call): the
 * gray image and LK pyramid of frame k+1 are then enqueued right behind frame k's pose kernels (they run while the host does call k's
 * bookkeeping and builds call k+1's slot table, a window in which the GPU is otherwise idle), and call k+1 finds them
 * ready when it passes the same pointer (any other pointer: the look-ahead is dropped and the frame is built as usual).  Results are
 * identical with and without hints.  One hint per call; NULL cancels. */
int alva_system_hint_next_frame_device(alva_system *sys, const uint8_t *d_rgba_next);
/* System::findCameraPoseWithIMU (system.cpp:57-104).  h_imu: [qw,qx,qy,qz,n, n x {ts,gx,gy,gz,ax,ay,az}]. Always returns 1. */
int alva_system_find_camera_pose_with_imu(alva_system *sys, const uint8_t *h_rgba, const double *h_imu, float *h_pose);
/* the same with the caller's timestamp in milliseconds instead of the wall clock (system.cpp:87), as alva_system_find_camera_pose_ts */
int alva_system_find_camera_pose_with_imu_ts(alva_system *sys, const uint8_t *h_rgba, const double *h_imu, double timestamp_ms, float *h_pose);
/* System::findPlane (system.cpp:123-137): 1 on success, 0 otherwise (needs >= 32 observed 3-D points). */
int alva_system_find_plane(alva_system *sys, float *h_pose, int num_iterations);
/* Hit test (no reference counterpart; alva_hit_test in alvaar_hip.h defines it): for each of n_rays (1..16) taps h_uv (raw image
 * pixels) the anchor pose h_pose16[ray][16] on the surface under the tap, fitted to the observed 3-D map points of the current frame
 * that project within radius_px of it (alva_system_find_plane's points, in the same order), from the current pose and the system's
 * own calibration.  h_info8[ray][8] = {code, selected, winning iteration, inliers, selected before the cap, 0, 0, 0}; code 0 found,
 * 1 fewer than 24 points selected, 2 no hypothesis survived, 3 fewer than 16 inliers, 4 grazing ray or surface behind the camera,
 * 5 not tracking (the last alva_system_find_camera_pose* did not return 1: nothing runs).  A pose is written only for code 0.  The
 * seed is fixed: the same map, pose and taps give the same bits, so a reticle does not jitter.  Changes no state of the session.
 * Returns the number of rays with code 0, or a negative error. */
int alva_system_hit_test(alva_system *sys, int n_rays, const float *h_uv, float radius_px, int num_iterations, float *h_pose16,
                         int *h_info8);
/* Depth from motion (no reference counterpart; alva_depth_sweep in alvaar_hip.h defines the stage): a depth image of the current frame
 * for occlusion, on the grid gw = width / step by gh = height / step, matched against an earlier frame of the session under the two
 * frames' poses.  Opt-in: alva_system_set_depth(sys, 1), before or after configure (it holds across alva_system_configure*); while it
 * is off nothing is kept, launched or allocated and alva_system_depth returns ALVA_ERR_STATE.
 * Reference frames: after a frame that returns 1 through alva_system_find_camera_pose* (not through a group), level 0 of its LK pyramid
 * and its pose are kept in a ring of 4 when the ring is empty or the camera centre is at least 0.03 x the median depth (camera z of the
 * frame's observed 3-D points) away from the newest entry; the copy is device to device on the session's stream.  configure,
 * alva_system_reset, a new map (any reset of the tracker) and turning depth off empty the ring; a LOST episode keeps it.
 * alva_system_depth: h_depth f32, h_conf u8, h_code u8, each gh x gw with room for cap >= gw gh elements; h_info8 = the count of each
 * code 0..5, then gw, gh.  Codes 0..5 as alva_depth_sweep (0 a depth, 1 border, 2 no texture, 3 not seen by the reference frame, 4
 * low confidence, 5 outside the swept range), and for the whole image, with all six counts 0 and nothing launched:
 *   6  not tracking: the last alva_system_find_camera_pose* did not return 1, or the frame sees fewer than 8 3-D points
 *   7  no reference frame: none of the ring has a baseline of 0.03 x the median depth and an optical axis within cos >= 0.9
 * The reference is the newest ring entry that qualifies; the swept range is rho_max = 1 / (0.5 z[5 %]), rho_min = 1 / (2 z[95 %]) of
 * the frame's points' sorted camera z (z[p %] = entry (n - 1) p / 100, integer division).  Depth is the camera-space z in map units
 * at the raw pixel (gx step + step / 2, gy step + step / 2).  step 1..16, num_hyp 8..256, patch_radius 1..4, min_texture and min_conf
 * 0..255.  Changes no state of the session; the same frame gives the same bits.  Returns the number of code-0 pixels or a negative
 * error. */
int alva_system_set_depth(alva_system *sys, int enabled);
int alva_system_depth(alva_system *sys, int step, int num_hyp, int patch_radius, int min_texture, int min_conf, float *h_depth,
                      uint8_t *h_conf, uint8_t *h_code, int cap, int *h_info8);
/* Dense depth (no reference counterpart; alva_depth_fuse and alva_depth_fill in alvaar_hip.h define the stages): the depth image fused
 * over the session's frames and completed, as ARCore acquireDepthImage16Bits beside the raw image of alva_system_depth.  Needs
 * alva_system_set_depth(sys, 1).  A call
 *   1  picks the reference frame and the range exactly as alva_system_depth does (the same code; codes 6 and 7 as there),
 *   2  sweeps on the device (the raw images are not downloaded),
 *   3  fuses the measurement with the session's state, warped by T_cp from the pose stored with the state to the current frame's pose
 *      (decay, w_max and rel_tol are the constants below),
 *   4  stores the new state and the current pose,
 *   5  fills it with rho_ref = 2 x the sweep range's rho_max and level 0 of the current LK pyramid as the guide,
 *   6  downloads depth, weight, src and level once.
 * h_depth f32 (camera-space z in map units, 0 = none), h_weight u8 (the state's w: 0 for a filled or empty cell), h_src u8 (F4's case
 * of the cell, 0..5), h_level u8 (0 a fused value, 1..max_level the evidence level of a filled cell, 255 none), each gh x gw with room
 * for cap >= gw gh elements.  h_info16 = the fuse counts of src 0..5, filled, empty, gw, gh, the whole-image code (0, 6 or 7), the
 * sweep's count of code 0, warp used (0 or 1), 0, 0, 0.  max_level 1..8; the other arguments as for alva_system_depth.
 * The state is per session and on the device, allocated by the first dense call; with depth off, or no dense call made, nothing is
 * allocated, kept or launched.  It is emptied by configure, alva_system_reset, a new map (any reset of the tracker), turning depth off,
 * alva_system_reset_depth_dense, and a call whose step or grid size differs from the state's.  Not tracking (code 6): nothing runs and
 * the state is kept, so it survives a LOST episode with relocalization on, as the ring does; all of depth is 0 and level 255.  No
 * reference frame (code 7): with a state, it is warped, stored and filled without a measurement; without one nothing is launched.  A
 * second call for the same frame (the tracker's frame counter, which a frame fed through a group advances too) does not fuse again: it
 * fills the stored state and returns the same bytes.  The call changes nothing else in the session, and alva_system_depth returns the same bytes whether or not dense calls happen.
 * Returns the number of grid pixels with a depth, or a negative error. */
#define ALVA_DEPTH_DENSE_DECAY 230      /* of 256: the weight a carried value keeps per call */
#define ALVA_DEPTH_DENSE_W_MAX 128      /* the ceiling of a fused weight */
#define ALVA_DEPTH_DENSE_REL_TOL 0.05   /* carried value and measurement agree within this share of the larger inverse depth */
int alva_system_depth_dense(alva_system *sys, int step, int num_hyp, int patch_radius, int min_texture, int min_conf, int max_level,
                            float *h_depth, uint8_t *h_weight, uint8_t *h_src, uint8_t *h_level, int cap, int *h_info16);
int alva_system_reset_depth_dense(alva_system *sys);
/* Scene mesh (no reference counterpart; alva_mesh_integrate and alva_mesh_extract in alvaar_hip.h define the stages): the geometry of the
 * scene as triangles, as ARKit scene reconstruction (ARMeshGeometry) and WebXR mesh-detection (XRMesh).  The depth of alva_system_depth is
 * fused, frame by frame, into a truncated signed distance volume of resolution^3 voxels kept on the device in WORLD coordinates, and
 * the volume's surface is extracted on request.  Needs alva_system_set_depth(sys, 1).
 * alva_system_mesh_update integrates the current frame.  resolution 32, 64, 128 or 256; rel_extent > 0; step, num_hyp, patch_radius,
 * min_texture, min_conf as for alva_system_depth.  It picks the reference frame and the range exactly as alva_system_depth does: code
 * 6 (not tracking) and 7 (no reference frame) run nothing and keep the volume.  With no volume, or with a resolution or rel_extent
 * other than the volume's, the volume is placed and zeroed: m = the median depth of the frame's map points, the cube's side = rel_extent
 * m, voxel = side / resolution, its centre = the camera centre + m x the optical axis, trunc = ALVA_MESH_TRUNC_VOXELS voxel.  THE
 * PLACEMENT'S SIZE THEN STAYS FIXED (a monocular map has no metric scale to size it by), and so does its position unless the app asks for
 * the volume to follow the camera (alva_system_set_mesh_follow, alva_system_mesh_move, below).  A second call
 * on the same frame (the tracker's frame counter) integrates nothing: code 8.  The sweep runs against the kept reference image on the
 * device and its outputs are integrated there with w_max = ALVA_MESH_W_MAX: no depth image crosses to the host.  h_info16 = {code, updated,
 * hidden, free, outside, no depth (alva_mesh_integrate's counts), resolution of the volume (0: none), the sweep's count of code 0,
 * frames integrated, placed by this call (0 or 1), voxels coloured, colour fused by this call (0 or 1; both 0 without mesh colour, below),
 * shifted by this call (0 or 1), this call's shift in voxels x, y, z (all 0 with follow off, below)}; h_geometry5 = {origin x, y, z (the volume's minimum corner), voxel, trunc},
 * zeros without a volume.  Returns the number of voxels updated, or a negative error (ALVA_ERR_STATE with depth off).
 * alva_system_mesh extracts the whole volume: h_vertices and h_normals f32 [max_vertices][3] (world coordinates; the normal points to
 * the free side), h_triangles int32 [max_triangles][3]; h_info8 as alva_mesh_extract's (code 0 a mesh, 1 no surface yet, 3 over a cap:
 * the counts are the true ones and nothing is written) and code 5: no volume yet.  It answers whether or not the tracker tracks right
 * now.  Returns the number of triangles, or a negative error.
 * The volume is per session, allocated by the first update; without one nothing is allocated, kept or launched.  It is emptied by
 * configure, alva_system_reset, a new map (any reset of the tracker), turning depth off, alva_system_reset_mesh, and an update whose
 * resolution or rel_extent differs.  The calls change nothing else in the session.  The volume is NOT re-fused when local BA moves the
 * poses it was integrated from: new evidence outweighs old only through ALVA_MESH_W_MAX. */
#define ALVA_MESH_W_MAX 128          /* the ceiling of a voxel's weight */
#define ALVA_MESH_TRUNC_VOXELS 3.0   /* the truncation distance, in voxels */
int alva_system_mesh_update(alva_system *sys, int resolution, double rel_extent, int step, int num_hyp, int patch_radius, int min_texture,
                            int min_conf, int *h_info16, double *h_geometry5);
int alva_system_mesh(alva_system *sys, int min_weight, int max_vertices, int max_triangles, float *h_vertices, float *h_normals,
                     int *h_triangles, int *h_info8, double *h_geometry5);
int alva_system_reset_mesh(alva_system *sys);
/* Following the camera (no reference counterpart; alva_mesh_shift in alvaar_hip.h defines the stage): the volume translated by whole
 * voxels so that it stays in front of a user who walks, as Kintinuous, InfiniTAM and Open3D's scalable volume move theirs.  Nothing is
 * resampled: where the old and the new cube overlap the volume keeps its bytes, zeros (never-seen voxels) enter on the far side, and
 * WHAT LEAVES THE CUBE IS GONE from the volume -- it is not kept or paged out; alva_system_mesh_blocks (below) tells the app which blocks
 * of the mesh left, so that it can keep its copy of them.  Opt-in: alva_system_set_mesh_follow(sys, block),
 * block 0 (off, the default) or 1, 2, 4, 8, 16, 32 voxels, before or after configure (it holds across alva_system_configure*).  While it
 * is off nothing is allocated or launched and every answer of the session keeps its bytes.  The switch itself does not touch the volume.
 * The session keeps the placement's origin0, side and median depth m0 and an integer offset in voxels; the volume's origin is always
 * origin0 + (double) offset voxel, computed afresh from the integers (offset 0: origin0's bits), and voxel and trunc never change.
 * The rule runs inside alva_system_mesh_update when follow is on, there is a volume, the call does not place it and the frame is not
 * already integrated (code 8) -- before the frame is integrated, so the frame lands in the shifted volume:
 *   V1 target        c_i = t_wc,i + m0 R_wc[i][2]: the placement's own expression with the placement's own m0, so the volume does not
 *                    breathe with the per-frame median
 *   V2 displacement  d_i = (c_i - (origin_i + side / 2)) / voxel
 *   V3 shift         s_i = block (int) trunc(d_i / block), 0 where d_i is not finite; |trunc(d_i / block)| is limited to
 *                    ALVA_MESH_FOLLOW_MAX_SHIFT / block first (such a shift empties any volume).  The volume moves only once the target is
 *                    a whole block away and the remainder stays under a block: hysteresis without extra state
 *   V4 apply         any s_i != 0: alva_mesh_shift with s into the second volume block (and the second colour block, with mesh colour),
 *                    each allocated by the first shift and not before; the blocks swap; offset += s.  h_info16[12..15] and h_geometry5
 *                    (the new origin) report it.  No s_i != 0: nothing is launched
 * alva_system_mesh_move is V2 - V4 with the caller's centre h_centre3 (world coordinates) and block (1, 2, 4, 8, 16 or 32), whatever the
 * switch says: the app decides where the volume should be.  It answers whether or not the tracker tracks, as alva_system_mesh.  h_info8 =
 * alva_mesh_shift's {copied, copied weighted, weighted voxels lost, copied coloured, code, 0, 0, resolution}: code 5 = no volume yet;
 * without a shift the counts are zero.  h_geometry5 as alva_system_mesh_update's, after the move.  Returns 1 when it shifted, 0 when
 * not, or a negative error.
 * alva_system_mesh_follow_stats: h_stats8 = {block, shifts of this volume so far, its offset x, y, z in voxels, weighted voxels lost so
 * far, 0, 0}.  Everything that empties or replaces the volume -- configure, alva_system_reset, a new map, depth off,
 * alva_system_reset_mesh, an update whose resolution or rel_extent differs -- clears the offset and the two tallies; a LOST episode with
 * relocalization on keeps them.  The raycast, the extraction and the colour sampler read the shifted volume with the new origin and
 * need no notice.  The group drivers do not follow. */
#define ALVA_MESH_FOLLOW_MAX_SHIFT (1 << 24)
int alva_system_set_mesh_follow(alva_system *sys, int block);
int alva_system_mesh_move(alva_system *sys, const double *h_centre3, int block, int *h_info8, double *h_geometry5);
int alva_system_mesh_follow_stats(alva_system *sys, long *h_stats8);
/* The mesh in blocks (no reference counterpart; alva_mesh_block_digest and alva_mesh_extract_blocks in alvaar_hip.h define the stages and
 * the lattice L1 - L4): the scene mesh as chunks with a stable identity of which only those that changed are handed out -- ARKit's
 * ARMeshAnchors (added, updated, removed), WebXR mesh-detection's XRMesh with lastChangedTime, HoloLens' surface observers.  The
 * volume moves in whole voxels and the session keeps the offset, so a block of `block` (8, 16 or 32) voxels has a key (b_x, b_y, b_z)
 * that stays the same across shifts, and while its box lies inside the cube its content is bit for bit the same.  Opt-in by calling
 * it: without a call nothing is allocated or launched, and the calls change nothing else in the session (alva_system_mesh, the
 * raycasts, the volume and the tracker keep their bytes).  min_weight as for alva_system_mesh; flags 0 or ALVA_MESH_BLOCKS_ALL.
 *   G1 volume      no volume: code 5 and nothing runs.  The call answers whether or not the tracker tracks, as alva_system_mesh
 *   G2 table       the session keeps key -> digest (L3) of the PRESENT blocks (L4) of the last successful call.  The table is cleared
 *                  and `epoch` incremented when the volume has been emptied, placed or replaced since -- configure,
 *                  alva_system_reset, a new map, depth off, alva_system_reset_mesh, an update whose resolution or rel_extent differs
 *                  -- or when min_weight or block differ from the table's, and by alva_system_reset_mesh_blocks.  A shift does not
 *                  clear it.  An app drops all its chunks when epoch changes
 *   G3 digests     alva_mesh_block_digest with lattice = the follow offset (zeros without follow), and one download
 *   G4 states      the present blocks in ascending (b_z, b_y, b_x): a key not in the table is state 1 (new), a digest that differs
 *                  state 2 (changed), an equal one state 0 -- reported, with its mesh, only with ALVA_MESH_BLOCKS_ALL.  Then the
 *                  table's keys that are not present now, in ascending order, with zero ranges: state 3, inside the block grid but
 *                  without a surface any more; state 4, left the cube -- the app may keep its last copy, which is how it holds a mesh
 *                  larger than the volume
 *   G5 caps        more blocks reported than max_blocks, or more vertices or triangles in the blocks to extract than max_vertices /
 *                  max_triangles: code 3, the true counts in h_info8, nothing else written and THE TABLE UNTOUCHED, so the same call
 *                  with larger buffers gives the answer a single call would have
 *   G6 meshes      alva_mesh_extract_blocks on the state 1 / 2 blocks (and the state 0 ones with ALL), packed in that order; with
 *                  h_colors (u8 [max_vertices][4]; ALVA_ERR_STATE with mesh colour off) the colour sampler of
 *                  alva_system_mesh_colored on the packed vertices before the download.  The table then becomes the present blocks'
 *                  digests
 * h_keys [max_blocks][3]; h_block_info [max_blocks][8] = {state, v0, nv, t0, nt, digest low word, high word, 0}: the block's vertices are
 * rows v0 .. v0 + nv - 1 of h_vertices / h_normals (f32 [max_vertices][3], world coordinates) / h_colors, its triangles rows t0 .. t0 + nt -
 * 1 of h_triangles (i32 [max_triangles][3]) with indices 0 .. nv - 1 LOCAL to the block; a vertex on a block boundary is repeated in the
 * neighbouring blocks with identical floats (L2), so adjacent chunks are watertight against each other.  h_lattice3 = the lattice used;
 * h_info8 = {code 0 / 3 / 5, blocks reported, vertices, triangles, blocks gone (states 3 and 4), epoch, present blocks, block};
 * h_geometry5 as alva_system_mesh's.  Returns the number of blocks reported, or a negative error.
 * Change detection is on GEOMETRY alone: colour weights move with every integrated frame and would mark every visible block on every
 * call; an app that wants refreshed colours asks with ALVA_MESH_BLOCKS_ALL.  The digest is a hash: a changed block keeps its digest with
 * a chance of about 2^-64, and ALL is the way around that too.  With the resolution and the follow block both multiples of `block`
 * every block is whole.  Otherwise the blocks at the cube's faces are partial: voxels outside the cube count as invalid, so a block that
 * enters or leaves the border is reported as changed -- choose block <= the follow block.  The group drivers do not get the call. */
#define ALVA_MESH_BLOCKS_ALL 1
int alva_system_mesh_blocks(alva_system *sys, int min_weight, int block, int flags, int max_blocks, int max_vertices, int max_triangles,
                            int *h_keys, int *h_block_info, float *h_vertices, float *h_normals, uint8_t *h_colors, int *h_triangles,
                            int *h_lattice3, int *h_info8, double *h_geometry5);
int alva_system_reset_mesh_blocks(alva_system *sys);   /* forget the list: epoch + 1, everything is reported anew */
/* Mesh colour (no reference counterpart; alva_color_thumb, alva_mesh_integrate_color and alva_mesh_color_at in alvaar_hip.h define the
 * stages): the frames' colour fused into the volume beside the distance, for painting the mesh of a scan preview, a minimap or a room
 * capture, colouring a raycast hit, tinting a virtual object by the surface it stands on.  Opt-in: alva_system_set_mesh_color(sys, 1),
 * before or after configure (it holds across alva_system_configure*); it has an effect only with depth on.  While it is off nothing is
 * kept, launched or allocated, and alva_system_mesh_colored and alva_system_mesh_color_at return ALVA_ERR_STATE.  While it is on the
 * distance volume, the mesh, the tracker and every other answer of the session keep their bytes.
 * Every alva_system_find_camera_pose* that returns 1 reduces its colour frame to a thumbnail (the means of blocks of ALVA_MESH_COLOR_STEP
 * pixels, kept on the device and stamped with the frame): the frame may be the caller's memory, which it may overwrite once the call
 * returns, and the update comes later.  One launch per frame, enqueued behind the frame's kernels; a frame in the caller's own memory
 * has been read when the call returns (light's wait covers it when light is on too; else the call waits for that launch), the
 * session's staging copy is not waited for.  alva_system_mesh_update then fuses the thumbnail of ITS frame together with the distance,
 * in the same launch (h_info16[10], [11]); with no thumbnail of the current frame (colour was turned on after it) it fuses geometry
 * only.  The colour volume is allocated, placed, replaced and emptied with the distance volume, and emptied by alva_system_set_mesh_color
 * changing; a LOST episode with relocalization on keeps it.  The group drivers (alva_system_group_*) do not feed it.  Colours are means
 * of PIXEL VALUES as they arrive (not linearised, no exposure compensation), and they are not re-fused when local BA moves poses.
 * alva_system_mesh_colored is alva_system_mesh -- the same bytes in everything they share -- with h_colors u8 [max_vertices][4]: the colour
 * volume sampled at every vertex on the device, before the download; alpha 255 where the vertex has a colour, four zeros where it has
 * none (no colour was fused near it); h_info8[6] = vertices with a colour.
 * alva_system_mesh_color_at samples the colour volume at n (1..2^20) world points h_points3 [n][3], for example alva_system_mesh_raycast's
 * h_points: h_rgba u8 [n][4], h_codes u8 [n] (alva_mesh_color_at's: 0 a colour, 1 outside the volume, 2 no colour fused there, 4 not
 * finite; 5 for every point without a volume or a colour volume, and then nothing is launched), h_info8 = {n, the count of each code 0,
 * 1, 2, 4, 0, 0, resolution}.  It answers whether or not the tracker tracks right now.  Returns the number of colours, or a negative
 * error. */
#define ALVA_MESH_COLOR_STEP 4
int alva_system_set_mesh_color(alva_system *sys, int enabled);
int alva_system_mesh_colored(alva_system *sys, int min_weight, int max_vertices, int max_triangles, float *h_vertices, float *h_normals,
                             uint8_t *h_colors, int *h_triangles, int *h_info8, double *h_geometry5);
int alva_system_mesh_color_at(alva_system *sys, int n, const float *h_points3, uint8_t *h_rgba, uint8_t *h_codes, int *h_info8);
/* Raycasting the scene volume (no reference counterpart; alva_mesh_raycast and alva_mesh_raycast_pixels in alvaar_hip.h define the stages
 * and the per-ray codes 0..4): rays against the session's kept volume, as ARKit's raycast against mesh geometry and WebXR hit test on
 * mesh-detection geometry; the depth image of the reconstruction, for occlusion.  min_weight 1..255 as for alva_system_mesh.  The three
 * calls only read the volume and change nothing in the session.  Without a volume every ray's code is 5 and nothing is launched; a call
 * that needs the current frame's pose answers code 6 for every ray while the tracker does not track (as alva_system_depth).  h_info8 =
 * {rays, the count of each code 0..4, the largest number of samples any ray took, resolution}, the counts zero under codes 5 and 6.
 * alva_system_mesh_raycast: n (1..2^20) world rays h_rays6 [n][6] = origin then direction (any length; t is in its units), t_near <=
 * t_far (t_far may be +inf); h_t [n], h_points and h_normals [n][3] (world coordinates, zero unless the code is 0), h_codes u8 [n].  It
 * answers whether or not the tracker tracks right now, as alva_system_mesh.  Returns the number of hits, or a negative error.
 * alva_system_mesh_depth: the depth image of the volume on alva_system_depth's grid, gw = width / step by gh = height / step, from h_T_wc12
 * (R_wc row-major, then t_wc; any pose, tracking or not) or, with NULL, from the current frame's pose.  h_depth [cap] is the camera-space
 * z in alva_system_depth's convention (0 where the code is not 0), h_normals [cap][3] the surface normals in world coordinates, h_codes u8
 * [cap]; cap >= gw gh.  It is the VOLUME's depth, not the current frame's: an object that has moved lags until new evidence outweighs the
 * old (ALVA_MESH_W_MAX), and what was never seen is transparent.  Returns the number of pixels with a depth, or a negative error.
 * alva_system_mesh_hit_test: n_taps (1..16) taps h_uv in raw image pixels from the current frame's pose; h_poses16 in alva_system_hit_test's
 * layout (y the surface normal, the translation the hit), zeros where there is no pose; h_info8 per tap = {code, pose_ok, the call's
 * largest sample count, resolution, 0 ...} -- a pose needs code 0, a non-zero gradient and a ray at least 5 degrees from grazing.
 * Returns the number of poses, or a negative error. */
int alva_system_mesh_raycast(alva_system *sys, int n, const double *h_rays6, int min_weight, double t_near, double t_far, float *h_t,
                             float *h_points, float *h_normals, uint8_t *h_codes, int *h_info8);
int alva_system_mesh_depth(alva_system *sys, const double *h_T_wc12, int step, int min_weight, float *h_depth, float *h_normals,
                           uint8_t *h_codes, int cap, int *h_info8);
int alva_system_mesh_hit_test(alva_system *sys, int n_taps, const float *h_uv, int min_weight, float *h_poses16, int *h_info8);
/* Light estimation (no reference counterpart; alva_light_bin, alva_light_fuse and alva_light_estimate in alvaar_hip.h define the stages):
 * the ambient intensity, second-order spherical harmonics and the primary directional light of the scene, as ARCore's LightEstimate,
 * ARKit's ARLightEstimate / ARDirectionalLightEstimate and WebXR light-estimation.  Opt-in: alva_system_set_light(sys, 1), before or after
 * configure (it holds across alva_system_configure*); while it is off nothing is kept, launched or allocated and alva_system_light returns
 * ALVA_ERR_STATE.
 * A camera sees about 60 degrees of the sphere, so one frame cannot give the lighting of a scene; a tracked session that looks around
 * can.  While light is on, every alva_system_find_camera_pose* bins its colour frame (blocks of ALVA_LIGHT_STEP pixels) by the frame's
 * ROTATION into a world-aligned cube map of 6 x 8 x 8 cells kept on the device, and blends it in with weight ALVA_LIGHT_W_NEW against a cell's
 * weight of at most ALVA_LIGHT_W_MAX (a cell needs ALVA_LIGHT_MIN_PIXELS pixels of a frame to count); cells the camera does not see keep
 * their value.  A frame that is not tracked (initialising, LOST) contributes its own mean values only.  One launch and one small workgroup
 * per frame, enqueued behind the frame's kernels; a frame in the caller's own memory (its frame buffer in device memory, its registered
 * buffer, a device frame) has been read when the call returns (the call waits for that launch), the session's staging copy is not waited for.
 * The environment is treated as DISTANT (only the rotation places a frame; the position is not used), and there is no exposure metadata:
 * all values are in the PIXEL-INTENSITY domain (pixel value 255 = 1.0 after the sRGB curve), they follow the camera's exposure and are
 * NOT photometric.
 * alva_system_light: h_sh27[3 k + c] = the real spherical harmonics of the environment's linear radiance in the world frame, k = 0..8 in
 * the order Y00, Y1-1 (y), Y10 (z), Y11 (x), Y2-2 (xy), Y2-1 (yz), Y20, Y21 (xz), Y22, without the Condon-Shortley sign (a positive band-1
 * coefficient = more light from the positive axis), c = R, G, B; h_primary_dir3 = the unit vector, in the world frame, towards the
 * strongest directional component (zero when there is none) and h_primary_rgb3 its intensity (it stays inside h_sh27, as in WebXR);
 * h_ambient4 = {mean linear luminance of the last frame 0..1, colour correction r, g, b}: ARCore's ambient-intensity mode; h_info8 = {code,
 * cells of the environment with a value, cells the last frame touched, blocks of the last frame, pixels of the last frame with a channel
 * >= 250, frames fused so far, primary valid 0 / 1, 0}.  Codes, also the return value:
 *   0  an estimate
 *   1  no environment yet (no tracked frame): only h_ambient4 is meaningful, h_sh27 holds the ambient term in Y00 alone, no primary light
 *   5  no frame seen since light was turned on (or since the environment was emptied): nothing is launched
 * The environment is per session, allocated by the first frame with light on.  It is emptied by configure, alva_system_reset, a new map
 * (any reset of the tracker), turning light off and alva_system_reset_light (which keeps the switch); a LOST episode with relocalization
 * on keeps it.  The group drivers (alva_system_group_*) do not feed it.  The call changes nothing else in the session.
 * Returns the code, or a negative error. */
#define ALVA_LIGHT_STEP 4
#define ALVA_LIGHT_MIN_PIXELS 64
#define ALVA_LIGHT_W_NEW 32
#define ALVA_LIGHT_W_MAX 224
int alva_system_set_light(alva_system *sys, int enabled);
int alva_system_light(alva_system *sys, float *h_sh27, float *h_primary_dir3, float *h_primary_rgb3, float *h_ambient4, int *h_info8);
int alva_system_reset_light(alva_system *sys);
/* Image detection (no reference counterpart; alva_image_match and alva_image_homography in alvaar_hip.h define the device stages): pose and
 * size of planar pictures the app knows -- a poster, a marker, a product box -- as ARCore's Augmented Images, ARKit's ARImageAnchor and
 * WebXR image-tracking.  A picture whose printed width is known is also the one way a monocular session learns its metric scale.
 * alva_system_add_image: gray, width x height pixels, rows `pitch` bytes apart, in host memory; width_m = the printed width in metres (0 =
 * unknown).  Sides 96 .. 1024, at most ALVA_IMAGE_MAX pictures per session.  The picture is described once, here: ORB with 500 features,
 * scale 1.2, FAST threshold 20 and L levels, L <= 8 the largest with short side / 1.2^(L-1) >= 64; a picture with fewer than 32 keypoints is
 * refused (the error text says so).  Returns its id (>= 0, never reused within the object's life) or a negative error.  Needs a configured
 * session (the descriptor runs on its device).  The pictures are the app's data, not the scene's: they outlive alva_system_configure*,
 * alva_system_reset and a new map; alva_system_remove_image, alva_system_reset_images and alva_system_destroy drop them.  With no picture
 * added nothing is allocated or launched; the frame-size ORB object (1500 features, 1.2, 8 levels, threshold 20) and the device block
 * come with the first detection after configure.
 * alva_system_detect_images answers every picture (at most `cap` of them), in ascending id, from the session's current frame -- level 0 of
 * the pyramid it holds: ORB on the frame, its keypoints undistorted, alva_image_match (max distance 64, ratio 0.8), alva_image_homography
 * (num_iterations, threshold_px, min_inliers, seed 12345), then per picture with a pose the winner's inliers through alva_pnp_refine with
 * the tracker's own parameters, as points (p.x, p.y, 0) of the picture's unit-width frame, a re-count of all its pairs at threshold_px
 * under the refined pose, and on the host (csrc/slam/image_place.hpp) the scale: every 3-D map point the frame observes, in front of the
 * camera, whose ray meets the picture inside its borders gives the ratio map depth / unit-width depth; the element of rank c / 2 of the
 * c ratios is the picture's width in map units.  Per picture k:
 *   h_ids[k]       its id
 *   h_info8[k]     {code, pairs, winning iteration or -1, its count, inliers after the refinement, map points used for the scale, frame
 *                  keypoints, 0}
 *   h_quads8[k]    the four corners in undistorted frame pixels: top-left, top-right, bottom-right, bottom-left (codes 0, 5, 6)
 *   h_poses16[k]   in alva_system_find_plane's layout, world (map) coordinates, at the picture's centre: x = the picture's right, y = its
 *                  normal towards the viewer, z = down the picture (ARCore's convention, right-handed)  (code 0)
 *   h_extents2[k]  the picture's width and height in map units  (code 0)
 *   h_scale1[k]    metres per map unit = width_m / width in map units, 0 when width_m is 0  (code 0)
 * Codes: 0 found; 1 fewer than min_inliers pairs; 2 no hypothesis survived; 3 the best count is below min_inliers; 4 not a rigid view of
 * a plane (a gate of alva_image_homography failed, the refinement failed or kept fewer than min_inliers); 5 found in the frame but not
 * placed: fewer than 8 map points lie on it, so there is no scale; 6 the same because the last alva_system_find_camera_pose* did not return
 * 1 -- the 2-D part still runs, so a picture is seen before the map exists; 7 no frame yet.  What is not listed for a code is zero.
 * The call changes nothing in the session: a session that calls it tracks bit for bit like one that never does.  A pose is NOT smoothed or
 * remembered between calls; an app that wants it to stick hands it to alva_system_create_anchors.  A few-Hz call: the host waits for the
 * frame's ORB, once after alva_image_homography and once per refined picture.  The group drivers do not have it.
 * Returns the number of pictures with code 0, or a negative error. */
#define ALVA_SYSTEM_IMAGE_MIN_KEYPOINTS 32
int alva_system_add_image(alva_system *sys, const uint8_t *h_gray, int width, int height, size_t pitch, double width_m);
int alva_system_remove_image(alva_system *sys, int id);
int alva_system_reset_images(alva_system *sys);
int alva_system_detect_images(alva_system *sys, int num_iterations, float threshold_px, int min_inliers, int cap, int *h_ids, float *h_poses16,
                              float *h_extents2, float *h_scale1, float *h_quads8, int *h_info8);
/* Plane detection (no reference counterpart; alva_detect_planes in alvaar_hip.h defines it): up to max_planes (1..8) planes of the MAP
 * -- all its 3-D points, observed by the current frame or not, in ascending id; of a map with more than 16384 of them the 16384 with
 * the highest ids.  h_planes24[k][24] = pose16 (columns: long axis -- pointing along the camera's x axis, or along its y axis for a plane that faces along the camera's x --, normal
 * facing the camera, short axis; translation: the centre of
 * the bounding rectangle), the extents along the long and the short axis, the plane's offset normal . centre, five zeros.
 * h_info8[k][8] = {code, live points, winning iteration, its count, inliers, 0, 0, 0}; code 0 found, 1 fewer than min_inliers live
 * points, 2 no hypothesis survived, 3 / 4 fewer than min_inliers points on the best / the refitted plane, 5 not run (an earlier round
 * stopped), 6 not tracking (the last alva_system_find_camera_pose* did not return 1: nothing runs).  A frame that tracks but observes
 * no 3-D point yet gives no D: the call answers as for an empty map (code 1, then 5).  A plane is written only for code 0.  The slab's half thickness is rel_thickness x D, D = the camera-frame depth of rank
 * n / 2 among the current frame's n observed 3-D points (alva_system_find_plane's points), since a monocular map has no metric scale.
 * h_point_ids / h_labels (each may be NULL; otherwise cap >= 16384 entries): the ids of the points looked at and the plane index of
 * each, or -1; both lists are filled up to cap with -1.  The seed is fixed: the same map and pose give the same bits.  Changes no state
 * of the session.  Returns the number of planes found, or a negative error. */
int alva_system_detect_planes(alva_system *sys, double rel_thickness, int min_inliers, int max_planes, int num_iterations,
                              float *h_planes24, int *h_info8, int *h_point_ids, int *h_labels, int cap);
/* Plane detection with outlines (no reference counterpart; alva_plane_outlines in alvaar_hip.h defines the outline): what
 * alva_system_detect_planes does, with the same arguments and -- on the same session state -- the same bytes in h_planes24, h_info8,
 * h_point_ids, h_labels and the return value, and for every plane its convex boundary polygon, computed from the same upload of the
 * points.  h_outline[k][max_vertices][2] (max_vertices 8..1024): the polygon's vertices in the plane's own frame, counter-clockwise in
 * (u, v) from the lexicographically smallest one; the world point of a vertex is centre + u x long axis + v x short axis of
 * h_planes24[k]; entries past the last vertex are zero.  The vertices lie on a grid of max(extent) / 2^20.
 * h_outline_info8[k][8] = {code, vertices, points of the plane, 0, 0, 0, 0, 0}; code 0 an outline, 1 fewer than 3 points, 2 no area (all
 * the plane's points on one line of the grid), 3 more than max_vertices vertices, 4 the plane's record cannot serve as a frame, 5 no plane
 * k (h_info8[k][0] is not 0), 6 not tracking.  h_area[k]: the polygon's area in map units squared.  Outline and area are written only
 * for code 0.  The outline depends on the plane's points as a set only.  Changes no state of the session.  Returns the number of planes
 * found, or a negative error. */
int alva_system_detect_plane_outlines(alva_system *sys, double rel_thickness, int min_inliers, int max_planes, int num_iterations,
                                      float *h_planes24, int *h_info8, int *h_point_ids, int *h_labels, int cap, int max_vertices,
                                      float *h_outline, int *h_outline_info8, double *h_area);
/* Plane tracking (no reference counterpart; alva_track_planes in alvaar_hip.h defines the stage, slam/plane_tracks.hpp the ids and the
 * merge): alva_system_detect_planes' inputs -- the map's 3-D points, the slab's half thickness rel_thickness x D, the 16384-point cap, the
 * fixed seed -- but the planes PERSIST between calls: the session keeps the records of the planes it returned (at most 8) and hands
 * them to the next call as priors.  A kept plane stays in the list's order (ascending id) in the first slots, is refitted to the points
 * now within the slab around it and grows with the map; new planes are looked for among the points that no kept plane holds, and fill
 * the slots after the kept ones.  h_planes24, h_info8, h_point_ids, h_labels, cap as for alva_system_detect_planes, with
 * h_info8[k][8] = {code, points (tracked slot) or live points (new), -1 or winning iteration, claimed or the winner's count, inliers,
 * origin (1 tracked, 0 new), 0, 0}; code 0 a plane; 1 .. 5 alva_system_detect_planes' for a new slot; 6 not tracking; 7 a tracked plane
 * that fewer than min_inliers points lie on now (lost), 8 the same after its refit, 9 its record is unusable.  A tracked plane with a code
 * other than 0 leaves the list.  h_plane_ids[k]: the plane's id (code 0), else -1 -- a tracked plane keeps its id, a new one gets the
 * next id; ids are never reused.  h_merged_into[k]: -1, or the id of the earlier plane of this call that plane k turned out to be part of
 * (normals within 10 degrees, each centre within the other's slab): plane k is delivered once more and then leaves the list, its points
 * go to that plane from the next call on.  max_planes below the number of planes tracked is an argument error.  While the last
 * alva_system_find_camera_pose* did not return 1 (or the frame gives no D) nothing runs: code 6 in every slot, ids -1, and the list stays
 * as it is -- planes survive a LOST episode when relocalization is on.  The list is emptied by alva_system_reset_planes, by
 * alva_system_configure* and whenever the map is thrown away (alva_system_reset, a failed initialisation, LOST without relocalization).
 * max_vertices > 0 (8..1024): the planes' outlines as for alva_system_detect_plane_outlines (a slot without a plane: outline code 5);
 * max_vertices = 0: no outlines, the three arrays may be NULL.  Changes nothing else in the session.  Returns the number of code-0
 * slots, or a negative error. */
int alva_system_track_planes(alva_system *sys, double rel_thickness, int min_inliers, int max_planes, int num_iterations,
                             float *h_planes24, int *h_info8, int *h_plane_ids, int *h_merged_into, int *h_point_ids, int *h_labels, int cap,
                             int max_vertices, float *h_outline, int *h_outline_info8, double *h_area);
void alva_system_reset_planes(alva_system *sys);
/* Anchors (no reference counterpart; alva_anchor_attach and alva_anchor_update in alvaar_hip.h define the stages, slam/anchors.hpp the
 * list): poses that stay attached to the map as it is refined.  The pose that alva_system_hit_test, alva_system_find_plane or
 * alva_system_detect_planes returned is a matrix in world coordinates, and the map under it keeps moving: local BA rewrites points, matching
 * merges them, culling removes them.  An anchor is tied to the map points around it -- its support, the max_support nearest 3-D points of
 * the map when it is created -- and alva_system_update_anchors recomputes its pose from where those points are now: the rigid motion of
 * the support since then (robust: one trim round), applied to the pose it was created with.  At most 64 anchors, in ascending id; ids
 * are never reused.
 * alva_system_create_anchors: n poses (1..16, alva_system_find_plane's layout: what the three calls above return), max_support 8..64.
 * The candidates are the map's 3-D points in ascending id, of a map past 16384 points the newest.  h_anchor_ids[k]: the new anchor's id,
 * or -1 unless the code is 0; h_info8[k][8] = {code, supports, points looked at, 0, 0, 0, 0, 0}: code 0 created, 1 fewer than four 3-D
 * points in the map, 3 the list is full, 4 a non-finite number in the pose, 6 not tracking (the last alva_system_find_camera_pose* did not
 * return 1).  Returns the number created, or a negative error.
 * alva_system_update_anchors: fills h_anchor_ids[k], h_pose16[k][16] and h_info8[k][8] for every anchor of the list, in ascending id, and
 * returns their number; cap (the arrays' rows) below the list's length is an argument error.  h_info8[k] = {code, supports alive, supports
 * kept by the trim, re-attached, age, supports at attach, 0, 0}: code 0 a rigid update, 1 translation only (fewer than four supports
 * alive, or supports on one line), 2 no support alive (the pose is the one it was attached with), 6 not tracking.  A support whose map
 * point is no longer a 3-D point of the map (culled, or absorbed by a merge) is dropped for good.  An anchor left with fewer than half its
 * supports -- alive < (supports at attach + 1) / 2 -- is re-attached after the update: the pose just delivered becomes its reference
 * pose, the max_support nearest points of the map as it is now its supports (re-attached = 1, supports at attach = the new number); with
 * fewer than four 3-D points in the map it keeps what it has.  age counts the updates that ran.  While the last
 * alva_system_find_camera_pose* did not return 1 nothing runs: every anchor answers code 6 with the pose delivered last, and the list
 * stays as it is -- anchors survive a LOST episode when relocalization is on.
 * alva_system_remove_anchor: 1 when the anchor existed, else 0.  The list is emptied by alva_system_reset_anchors, by
 * alva_system_configure* and whenever the map is thrown away (alva_system_reset, a failed initialisation, LOST without relocalization).
 * None of the four changes anything else in the session. */
int alva_system_create_anchors(alva_system *sys, int n, const float *h_pose16, int max_support, int *h_anchor_ids, int *h_info8);
int alva_system_update_anchors(alva_system *sys, int cap, int *h_anchor_ids, float *h_pose16, int *h_info8);
int alva_system_remove_anchor(alva_system *sys, int anchor_id);
void alva_system_reset_anchors(alva_system *sys);
/* System::getFramePoints (system.cpp:139-154): writes x,y int pairs of the current 2-D (not yet triangulated)
 * keypoints, at most 2048 points (the caller's buffer is uint32[4096], src/system.js:64); returns their count. */
int alva_system_get_frame_points(alva_system *sys, int *h_points);

/* ids + pixel positions + 3-D flag of the current frame's keypoints, in the frame container's order; returns their number */
int alva_system_get_keypoints(alva_system *sys, int *h_ids, float *h_px, uint8_t *h_is3d, int cap);

/* ---- inspection (tests, tools): flat views of the map layer's state, same layouts as oracle/ref_shim_system.cpp produces for
 * the reference's System.  out16: frame id, keyframe id, #keypoints, #2-D, #3-D, occupied cells, #keyframes, #map points, map
 * initialised, p3pReq_, poseFailedCounter_, next keyframe id, next map point id, |local map|, |covisible|, frameMaxNumKeypoints_. */
int alva_system_debug_state(alva_system *sys, int *out16);
int alva_system_debug_pose7(alva_system *sys, double *pose7_twc, double *init_pose7);
int alva_system_debug_frame_keypoints(alva_system *sys, int cap, int *ids, float *px, float *unpx, uint8_t *is3d, uint8_t *has_desc);
int alva_system_debug_keyframe_ids(alva_system *sys, int cap, int *ids);
int alva_system_debug_keyframe(alva_system *sys, int kfid, double *pose7, int *info6, int cap, int *ids, float *px, uint8_t *is3d);
int alva_system_debug_covisibility(alva_system *sys, int kfid, int cap, int *pairs);
int alva_system_debug_map_points(alva_system *sys, int cap, int *ids, double *xyz, int *flags5, double *inv_depth, uint8_t *desc);
/* ids of the observed 3-D map points of the current frame in the map container's order: the points, in the order, that
 * alva_system_find_plane and alva_system_hit_test hand to their kernels; returns their number */
int alva_system_debug_frame_map_point_ids(alva_system *sys, int cap, int *ids);
int alva_system_debug_counters(alva_system *sys, long *out3 /* local-BA solves, map-point merges, culled keyframes */);
/* alva_system_depth with what it handed to alva_depth_sweep (each may be NULL): h_images2 [2][height][width] the current and the
 * reference image, h_T_rc12, h_rho2 = {rho_min, rho_max}; written only when the sweep ran.  alva_system_debug_depth_ring: the poses
 * (t, q = x y z w) of the kept reference frames, newest first, into h_pose7x4 [4][7] (may be NULL); returns their number. */
int alva_system_debug_depth(alva_system *sys, int step, int num_hyp, int patch_radius, int min_texture, int min_conf, float *h_depth,
                            uint8_t *h_conf, uint8_t *h_code, int cap, int *h_info8, uint8_t *h_images2, double *h_T_rc12, double *h_rho2);
int alva_system_debug_depth_ring(alva_system *sys, double *h_pose7x4);
/* alva_system_depth_dense with what it handed to alva_depth_fuse and alva_depth_fill (each may be NULL): the state before and after the
 * call (h_rho_before f32, h_w_before u8, h_rho_after f32, each [cap]; the weight after is h_weight; before is zeros when there was no
 * state), the sweep's raw outputs (h_raw_depth, h_raw_conf, h_raw_code; zeros and code 255 when nothing was swept), h_gray [height][width]
 * the guide image, h_pose7x2 the pose (t, q = x y z w) stored with the state and the current frame's, h_T_cp12, h_rho_ref, and h_flags4 =
 * {what ran: -1 nothing, 0 fill of the stored state only, 1 fuse without a previous state, 2 warp and fuse; swept (0 or 1); 0; 0}. */
int alva_system_debug_depth_dense(alva_system *sys, int step, int num_hyp, int patch_radius, int min_texture, int min_conf, int max_level,
                                  float *h_depth, uint8_t *h_weight, uint8_t *h_src, uint8_t *h_level, int cap, int *h_info16,
                                  float *h_rho_before, uint8_t *h_w_before, float *h_rho_after, float *h_raw_depth, uint8_t *h_raw_conf,
                                  uint8_t *h_raw_code, uint8_t *h_gray, double *h_pose7x2, double *h_T_cp12, double *h_rho_ref,
                                  int *h_flags4);
/* alva_system_mesh_update with what the call saw, for replaying the stages (each may be NULL): the sweep's raw outputs (h_raw_depth f32,
 * h_raw_conf u8, h_raw_code u8, each [gh][gw]), h_T_cw12 the pose handed to alva_mesh_integrate, and the volume after the update (h_q
 * int16, h_w u8, each [resolution]^3); written only when the integration ran (code 0). */
int alva_system_debug_mesh_update(alva_system *sys, int resolution, double rel_extent, int step, int num_hyp, int patch_radius,
                                  int min_texture, int min_conf, int *h_info16, double *h_geometry5, float *h_raw_depth,
                                  uint8_t *h_raw_conf, uint8_t *h_raw_code, double *h_T_cw12, int16_t *h_q, uint8_t *h_w);
/* Mesh colour's kept state, for replaying the stages (each may be NULL): h_thumb u8 [height / ALVA_MESH_COLOR_STEP][width /
 * ALVA_MESH_COLOR_STEP][4] the thumbnail of the last coloured frame, h_c u8 [resolution^3][4] the colour volume; zeros where there is none
 * (h_c is not written without a volume).  Returns bit 0: the thumbnail is the current frame's, bit 1: there is a colour volume; or a
 * negative error (ALVA_ERR_STATE with mesh colour off). */
int alva_system_debug_mesh_color(alva_system *sys, uint8_t *h_thumb, uint8_t *h_c);
/* alva_system_light with what the last frame handed to the stages (each may be NULL): h_acc [ALVA_LIGHT_ACC_WORDS] the frame accumulators
 * alva_light_bin left and alva_light_fuse folded in, h_R_wc9 the rotation it was binned with (row-major; zeros when it was not tracked),
 * h_flags4 = {a frame was fed 0 / 1, it was binned with a rotation 0 / 1, frames fed since the environment was emptied, 0}, h_state
 * [ALVA_LIGHT_STATE_BYTES] the environment state alva_light_estimate projected.  Zeros where no frame was fed. */
int alva_system_debug_light(alva_system *sys, float *h_sh27, float *h_primary_dir3, float *h_primary_rgb3, float *h_ambient4, int *h_info8,
                            uint64_t *h_acc, double *h_R_wc9, int *h_flags4, uint8_t *h_state);
/* alva_system_detect_images with what the call saw, so that the stages can be replayed on it (every pointer may be NULL; the blocks are
 * sized for ALVA_IMAGE_MAX pictures, ALVA_IMAGE_QUERY_CAP rows each, and ALVA_IMAGE_TRAIN_CAP frame keypoints):
 *   n_frame      the frame's ORB keypoint count; kp / unpx [n_frame][2] their raw and undistorted positions, desc [n_frame][32]
 *   nq [k], wh [k][2], qxy [k][512][2], qdesc [k][512][32]   the pictures as they were described when they were added
 *   match [k][512][3], xy [k][512][4], count [k]             alva_image_match's outputs
 *   H [k][9], mask [k][512], stage_info [k][8], stage_R [k][9], stage_t [k][3]   alva_image_homography's outputs (before the refinement)
 *   R [k][9], t [k][3]    the picture's pose in the camera after the refinement, in units of its width (code 0, 5, 6)
 *   pose7                 the frame's Twc (t, q = x y z w) the placement used; tracked = 1 when the last frame returned status 1 */
typedef struct alva_image_debug {
    int *n_frame;
    float *kp, *unpx;
    uint8_t *desc;
    int *nq, *wh;
    float *qxy;
    uint8_t *qdesc;
    int *match;
    double *xy;
    int *count;
    double *H;
    uint8_t *mask;
    int *stage_info;
    double *stage_R, *stage_t, *R, *t, *pose7;
    int *tracked;
} alva_image_debug;
int alva_system_debug_detect_images(alva_system *sys, int num_iterations, float threshold_px, int min_inliers, int cap, int *h_ids,
                                    float *h_poses16, float *h_extents2, float *h_scale1, float *h_quads8, int *h_info8,
                                    const alva_image_debug *dbg);
/* ---- the optional SHARED-MAP MERGE across sessions, applied to a session (north_star's extra; the reference has one map: parity unpinned).
 * A merge round (alvaar_amd/multi.py: pack -> ONE all_gather over the process group -> alva_fuse_map_points) decides, for map points of
 * DIFFERENT streams that coincide -- same world position within 5 cm, descriptors within 51 bits; this presumes that the streams' maps live
 * in ONE world frame (a rig with known extrinsics, a shared initialisation, or maps registered beforehand), which the round verifies with
 * a similarity fit over the fused pairs before it applies anything -- which point of the shared map each absorbed point IS.  Applying it:
 *   alva_system_set_shared_ids      map point `local_id[i]` of this session is point (shared_stream[i], shared_id[i]) of the shared map;
 *                                   returns how many of the ids exist.  The table follows MapManager::mergeMapPoints (the survivor
 *                                   inherits it) and forgets culled points; alva_system_get_shared_ids reads it (ascending local id).
 *   alva_system_merge_map_points    MapManager::mergeMapPoints(prev_id, new_id) (map_manager.cpp:428-513) on this session's own map: two
 *                                   of its points that the round found to be the SAME shared point become one; 1 = merged, 0 = not
 *                                   merged: the reference's early return (a point is gone or the survivor is not 3-D), or the two
 *                                   points are observed together by the current frame or by a keyframe -- the reference's routine
 *                                   only ever meets points that are not (a new keyframe's keypoint against a local-map point the
 *                                   frame does not see) and would leave that frame with a keypoint of a vanished map point; such a
 *                                   pair keeps its two ids and the same shared id. */
int alva_system_merge_map_points(alva_system *sys, int prev_id, int new_id);
int alva_system_set_shared_ids(alva_system *sys, int n, const int *local_id, const int *shared_stream, const int *shared_id);
int alva_system_get_shared_ids(alva_system *sys, int cap, int *local_id, int *shared_stream, int *shared_id);
/* This session's 3-D map points as the exchange's record block, written ON THE DEVICE from the resident map (alva_pack_map_records):
 * d_out [capacity][64] in the system's GPU memory; *h_count = 3-D points with a descriptor (when it exceeds `capacity` the block holds an
 * arbitrary subset: export through alva_system_debug_map_points instead, which keeps the oldest).  Pending descriptor edits are replayed
 * first.  ALVA_ERR_STATE without a device-resident map (nothing was ever mapped). */
int alva_system_pack_map_records(alva_system *sys, int stream_id, int capacity, uint8_t *d_out, int *h_count);
/* fb-KLT work since the last reset: out2[0] = keypoint-levels (LK passes over one pyramid level, forwards + the backward pass, from
 * the per-slot result codes), out2[1] = slots handed to the tracking steps */
int alva_system_debug_klt_work(alva_system *sys, long *out2, int reset);
/* wall-clock seconds per section of the frame loop since the last reset: upload + pyramid enqueue, slot gathering, tracking step,
 * tracker bookkeeping, wait for the pose, pose bookkeeping + keyframe decision, keyframe creation, mapping (incl. local BA) */
int alva_system_debug_timing(alva_system *sys, double *out8, int reset);
/* finer laps of the keyframe path + element counts (profiling aid; indices documented in alvaar_amd/system.py: timing_fine) */
int alva_system_debug_timing_fine(alva_system *sys, double *out32, int reset);
/* finer split of the keyframe sections: [0] prepareFrame [1] describe tracked keypoints [2] grid detection [3] describe + undistort new
 * keypoints [4] map insertion + keyframe copy | [5] triangulation [6] covisibility [7] local-map matching incl. flattening and merges
 * [8] optimize (local BA + culling) ; inside them: [9] the matchToMap stage call [10] the local-BA stage calls */
int alva_system_debug_timing_keyframe(alva_system *sys, double *out16, int reset);
/* (the differential tests' one behaviour-changing hook, alva_system_debug_set_init_pose, is declared in alvaar_system_testing.h, not here) */
const char *alva_system_last_error(void);

#ifdef __cplusplus
}

namespace alva {
/* Drop-in for the reference's `class System` (same method names and argument order). */
class System {
public:
    System() { status_ = alva_system_create(0, &s_); }
    ~System() { alva_system_destroy(s_); }
    System(const System &) = delete;
    System &operator=(const System &) = delete;
    void configure(int imageWidth, int imageHeight, double fx, double fy, double cx, double cy, double k1, double k2, double p1,
                   double p2) {
        status_ = s_ ? alva_system_configure(s_, imageWidth, imageHeight, fx, fy, cx, cy, k1, k2, p1, p2) : status_;
    }
    /* 0 when construction and the last configure succeeded (the reference's methods are void; errors surface here) */
    int status() const { return status_; }
    void reset() { alva_system_reset(s_); }
    /* relocalization after tracking loss (status 4 while lost; see alva_system_set_relocalization) */
    int setRelocalization(bool enabled, int maxLostFrames = 0) { return alva_system_set_relocalization(s_, enabled ? 1 : 0, maxLostFrames); }
    /* depth from motion (no reference counterpart, so no wasm twin): depth / conf / code [cap] with cap >= (width / step) (height / step),
     * info[8]; returns the number of pixels with a depth (see alva_system_depth) */
    int setDepth(bool enabled) { return alva_system_set_depth(s_, enabled ? 1 : 0); }
    int depth(int step, int numHyp, int patchRadius, int minTexture, int minConf, float *depth, uint8_t *conf, uint8_t *code, int cap,
              int *info) {
        return alva_system_depth(s_, step, numHyp, patchRadius, minTexture, minConf, depth, conf, code, cap, info);
    }
    /* dense depth: the fused and completed image; depth / weight / src / level [cap], info[16] (see alva_system_depth_dense) */
    int depthDense(int step, int numHyp, int patchRadius, int minTexture, int minConf, int maxLevel, float *depth, uint8_t *weight,
                   uint8_t *src, uint8_t *level, int cap, int *info) {
        return alva_system_depth_dense(s_, step, numHyp, patchRadius, minTexture, minConf, maxLevel, depth, weight, src, level, cap, info);
    }
    int resetDepthDense() { return alva_system_reset_depth_dense(s_); }
    /* scene mesh: info[16], geometry[5]; vertices / normals [maxVertices][3], triangles [maxTriangles][3], info[8] (see
     * alva_system_mesh_update / alva_system_mesh) */
    int meshUpdate(int resolution, double relExtent, int step, int numHyp, int patchRadius, int minTexture, int minConf, int *info,
                   double *geometry) {
        return alva_system_mesh_update(s_, resolution, relExtent, step, numHyp, patchRadius, minTexture, minConf, info, geometry);
    }
    int mesh(int minWeight, int maxVertices, int maxTriangles, float *vertices, float *normals, int *triangles, int *info, double *geometry) {
        return alva_system_mesh(s_, minWeight, maxVertices, maxTriangles, vertices, normals, triangles, info, geometry);
    }
    int resetMesh() { return alva_system_reset_mesh(s_); }
    /* following the camera: block 0 (off), 1, 2, 4, 8, 16 or 32 voxels; centre [3], info[8], geometry[5]; stats[8] (see
     * alva_system_set_mesh_follow) */
    int setMeshFollow(int block) { return alva_system_set_mesh_follow(s_, block); }
    int meshMove(const double *centre, int block, int *info, double *geometry) { return alva_system_mesh_move(s_, centre, block, info, geometry); }
    int meshFollowStats(long *stats) { return alva_system_mesh_follow_stats(s_, stats); }
    /* the mesh in blocks: block 8, 16 or 32; keys [maxBlocks][3], blockInfo [maxBlocks][8], vertices / normals [maxVertices][3], colors
     * [maxVertices][4] or null, triangles [maxTriangles][3], lattice[3], info[8], geometry[5] (see alva_system_mesh_blocks) */
    int meshBlocks(int minWeight, int block, bool all, int maxBlocks, int maxVertices, int maxTriangles, int *keys, int *blockInfo,
                   float *vertices, float *normals, uint8_t *colors, int *triangles, int *lattice, int *info, double *geometry) {
        return alva_system_mesh_blocks(s_, minWeight, block, all ? ALVA_MESH_BLOCKS_ALL : 0, maxBlocks, maxVertices, maxTriangles, keys, blockInfo,
                                       vertices, normals, colors, triangles, lattice, info, geometry);
    }
    int resetMeshBlocks() { return alva_system_reset_mesh_blocks(s_); }
    /* mesh colour: colors [maxVertices][4]; points [n][3], rgba [n][4], codes [n], info[8] (see alva_system_mesh_colored /
     * alva_system_mesh_color_at) */
    int setMeshColor(bool enabled) { return alva_system_set_mesh_color(s_, enabled ? 1 : 0); }
    int meshColored(int minWeight, int maxVertices, int maxTriangles, float *vertices, float *normals, uint8_t *colors, int *triangles,
                    int *info, double *geometry) {
        return alva_system_mesh_colored(s_, minWeight, maxVertices, maxTriangles, vertices, normals, colors, triangles, info, geometry);
    }
    int meshColorAt(const float *points, int n, uint8_t *rgba, uint8_t *codes, int *info) {
        return alva_system_mesh_color_at(s_, n, points, rgba, codes, info);
    }
    /* raycasting the scene volume: rays [n][6]; t [n], points / normals [n][3], codes [n], info[8]; Twc [12] or null: the current pose,
     * depth / codes [cap], normals [cap][3]; uv [nTaps][2], poses [nTaps][16], info [nTaps][8] (see alva_system_mesh_raycast) */
    int meshRaycast(const double *rays, int n, int minWeight, double tNear, double tFar, float *t, float *points, float *normals,
                    uint8_t *codes, int *info) {
        return alva_system_mesh_raycast(s_, n, rays, minWeight, tNear, tFar, t, points, normals, codes, info);
    }
    int meshDepth(const double *Twc, int step, int minWeight, float *depth, float *normals, uint8_t *codes, int cap, int *info) {
        return alva_system_mesh_depth(s_, Twc, step, minWeight, depth, normals, codes, cap, info);
    }
    int meshHitTest(const float *uv, int nTaps, int minWeight, float *poses, int *info) {
        return alva_system_mesh_hit_test(s_, nTaps, uv, minWeight, poses, info);
    }
    /* light estimation: sh[27], primaryDir[3], primaryRgb[3], ambient[4], info[8]; returns the code (see alva_system_light) */
    int setLight(bool enabled) { return alva_system_set_light(s_, enabled ? 1 : 0); }
    int light(float *sh, float *primaryDir, float *primaryRgb, float *ambient, int *info) {
        return alva_system_light(s_, sh, primaryDir, primaryRgb, ambient, info);
    }
    int resetLight() { return alva_system_reset_light(s_); }
    /* image detection: see alva_system_add_image / alva_system_detect_images */
    int addImage(const uint8_t *gray, int width, int height, size_t pitch, double widthMetres) {
        return alva_system_add_image(s_, gray, width, height, pitch, widthMetres);
    }
    int removeImage(int id) { return alva_system_remove_image(s_, id); }
    int resetImages() { return alva_system_reset_images(s_); }
    int detectImages(int numIterations, float thresholdPx, int minInliers, int cap, int *ids, float *poses, float *extents, float *scale,
                     float *quads, int *info) {
        return alva_system_detect_images(s_, numIterations, thresholdPx, minInliers, cap, ids, poses, extents, scale, quads, info);
    }
    /* native, pointer-typed */
    int findCameraPose(const uint8_t *imageRGBA, float *pose) { return alva_system_find_camera_pose(s_, imageRGBA, pose); }
    int findCameraPoseWithIMU(const uint8_t *imageRGBA, const double *imu, float *pose) {
        return alva_system_find_camera_pose_with_imu(s_, imageRGBA, imu, pose);
    }
    int findPlane(float *location, int numIterations) { return alva_system_find_plane(s_, location, numIterations); }
    int getFramePoints(int *points) { return alva_system_get_frame_points(s_, points); }
    /* hit test (no reference counterpart, so no wasm twin): nRays taps uv[nRays][2] -> poses[nRays][16], info[nRays][8];
     * returns the number of hits (see alva_system_hit_test) */
    int hitTest(const float *uv, int nRays, float radiusPx, int numIterations, float *poses, int *info) {
        return alva_system_hit_test(s_, nRays, uv, radiusPx, numIterations, poses, info);
    }
    /* plane detection (no reference counterpart, so no wasm twin): planes[maxPlanes][24], info[maxPlanes][8], pointIds / labels [cap] or
     * null; returns the number of planes found (see alva_system_detect_planes) */
    int detectPlanes(double relThickness, int minInliers, int maxPlanes, int numIterations, float *planes, int *info, int *pointIds,
                     int *labels, int cap) {
        return alva_system_detect_planes(s_, relThickness, minInliers, maxPlanes, numIterations, planes, info, pointIds, labels, cap);
    }
    /* detectPlanes and each plane's convex outline: outlines[maxPlanes][maxVertices][2] in the plane's frame, outlineInfo[maxPlanes][8],
     * areas[maxPlanes] (see alva_system_detect_plane_outlines) */
    int detectPlaneOutlines(double relThickness, int minInliers, int maxPlanes, int numIterations, float *planes, int *info, int *pointIds,
                            int *labels, int cap, int maxVertices, float *outlines, int *outlineInfo, double *areas) {
        return alva_system_detect_plane_outlines(s_, relThickness, minInliers, maxPlanes, numIterations, planes, info, pointIds, labels, cap,
                                                 maxVertices, outlines, outlineInfo, areas);
    }
    /* plane tracking: detectPlanes' planes kept between calls, with ids (planeIds[maxPlanes]) and merges (mergedInto[maxPlanes]);
     * maxVertices 0: no outlines (see alva_system_track_planes) */
    int trackPlanes(double relThickness, int minInliers, int maxPlanes, int numIterations, float *planes, int *info, int *planeIds,
                    int *mergedInto, int *pointIds, int *labels, int cap, int maxVertices = 0, float *outlines = nullptr,
                    int *outlineInfo = nullptr, double *areas = nullptr) {
        return alva_system_track_planes(s_, relThickness, minInliers, maxPlanes, numIterations, planes, info, planeIds, mergedInto, pointIds,
                                        labels, cap, maxVertices, outlines, outlineInfo, areas);
    }
    void resetPlanes() { alva_system_reset_planes(s_); }
    /* anchors: poses[n][16] -> anchorIds[n], info[n][8], returns the number created; updateAnchors fills up to cap rows in ascending
     * id and returns their number (see alva_system_create_anchors) */
    int createAnchors(const float *poses, int n, int maxSupport, int *anchorIds, int *info) {
        return alva_system_create_anchors(s_, n, poses, maxSupport, anchorIds, info);
    }
    int updateAnchors(int cap, int *anchorIds, float *poses, int *info) { return alva_system_update_anchors(s_, cap, anchorIds, poses, info); }
    int removeAnchor(int anchorId) { return alva_system_remove_anchor(s_, anchorId); }
    void resetAnchors() { alva_system_reset_anchors(s_); }
    /* wasm32 calling convention of the reference (pointers as int heap offsets) */
    int findCameraPose(int imageRGBADataPtr, int posePtr) {
        return findCameraPose(reinterpret_cast<const uint8_t *>((uintptr_t) (uint32_t) imageRGBADataPtr),
                              reinterpret_cast<float *>((uintptr_t) (uint32_t) posePtr));
    }
    int findCameraPoseWithIMU(int imageRGBADataPtr, int imuDataPtr, int posePtr) {
        return findCameraPoseWithIMU(reinterpret_cast<const uint8_t *>((uintptr_t) (uint32_t) imageRGBADataPtr),
                                     reinterpret_cast<const double *>((uintptr_t) (uint32_t) imuDataPtr),
                                     reinterpret_cast<float *>((uintptr_t) (uint32_t) posePtr));
    }
    int findPlane(int locationPtr, int numIterations) {
        return findPlane(reinterpret_cast<float *>((uintptr_t) (uint32_t) locationPtr), numIterations);
    }
    int getFramePoints(int pointsPtr) { return getFramePoints(reinterpret_cast<int *>((uintptr_t) (uint32_t) pointsPtr)); }
    alva_system *handle() { return s_; }

private:
    alva_system *s_ = nullptr;
    int status_ = 0;
};
}  // namespace alva
#endif
#endif /* ALVAAR_SYSTEM_H */
