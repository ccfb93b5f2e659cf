// The device side of the scene features (hit test, depth from motion, dense depth, light estimation, image detection, planes,
// anchors): none has a counterpart in the reference, and none is a stage of the map layer -- the session (system_scene.hip) calls them
// directly.  One object per configured session, made after its HipStages and destroyed before it: the calls run on the stages' context
// and stream, on the frame the stages hold (HipStages::frame), through the stages' one pair of staging arenas (HipStages::carve).  The
// state the features keep on the device between calls lives here, each block allocated by the first call that needs it: every one a
// DeviceBlock (device_block.hpp) -- the volumes a Volume, block and resolution in one value -- that frees itself, so a feature adds a
// member and a method and nothing to the destructor.  The two launches that read a frame that may be the caller's own memory share
// one wait (FrameRead), the three calls that sweep share one sweep (SweepParams, sweep()).
//
// All pointers are HOST pointers; arrays are flat.  Every method returns 0 on success, a negative alva error code otherwise.
#pragma once
#include "device_block.hpp"
#include "stages_hip.hpp"
#include <vector>

namespace alva_slam {

// the depth sweep's parameters that the session's callers choose, and the ranges the session accepts
struct SweepParams {
    int step, num_hyp, patch_radius, min_texture, min_conf;
    bool ok() const {
        return step >= 1 && step <= 16 && num_hyp >= 8 && num_hyp <= 256 && patch_radius >= 1 && patch_radius <= 4 && min_texture >= 0 &&
               min_texture <= 255 && min_conf >= 0 && min_conf <= 255;
    }
};

// a device block and the resolution N it was made for (0: none), `per_voxel` bytes for each of N^3 voxels: the value that is tested,
// replaced and swapped is the pair, so a block never meets another block's N
struct Volume {
    DeviceBlock block;
    int N = 0;
    bool is(int n) const { return block && N == n; }
    size_t voxels() const { return (size_t) N * N * N; }
    int replace(int n, size_t per_voxel, hipStream_t st) {
        N = 0;
        const int rc = block.replace(per_voxel * (size_t) n * n * n, st);
        if (rc == ALVA_OK) N = n;
        return rc;
    }
    int release(hipStream_t st) {
        const int rc = block.release(st);
        if (!block) N = 0;
        return rc;
    }
};

// A launch reads the frame's source.  The staging copy is the session's own, and the next upload is ordered behind the launch; any
// other source is the caller's memory, which it may overwrite as soon as the call returns: the launch must have read it by then.  It
// says so in a word in pinned memory -- it publishes `seq`, which never takes the word's first value 0 -- that is polled like the
// tracking step's; a session that does not poll waits for the stream instead.  One object per launch that publishes
struct FrameRead {
    uint32_t *word = nullptr, seq = 0;   // pinned, made by the first arm()
    FrameRead() = default;
    FrameRead(const FrameRead &) = delete;
    ~FrameRead() {
        if (word) (void) hipHostFree(word);
    }
    static bool owed(const HipStages::Frame &f) { return !f.src_is_staging; }
    // before the launch: the next seq, and *publish = the word to hand to the launch, null where nobody will poll it (the frame is
    // the session's own, the session does not poll, or -- wait_here false -- a later wait on the same stream covers this launch)
    int arm(const HipStages::Frame &f, bool wait_here, uint32_t **publish) {
        if (!word) {
            ALVA_HIP(hipHostMalloc((void **) &word, 64, hipHostMallocDefault));
            *word = 0;
        }
        if (++seq == 0) ++seq;
        *publish = owed(f) && wait_here && f.poll ? word : nullptr;
        return ALVA_OK;
    }
    // after the launch, where the wait is owed: -> ALVA_OK, the stream's error, or 1: the word was never published (the caller says
    // so in its own words)
    int wait(const HipStages::Frame &f) const {
        if (!f.poll) ALVA_HIP(alva_stream_sync(f.st));
        else if (!alva_wait_until([&] { return *(volatile uint32_t *) word == seq; }, f.st)) return 1;
        return ALVA_OK;
    }
};

class SceneStages {
public:
    explicit SceneStages(HipStages &stages) : hs(stages) {}
    ~SceneStages();
    SceneStages(const SceneStages &) = delete;   // (it owns device memory)

    // the hit test (alva_hit_test): n_rays taps uv against the n points
    int hit_test(int n, const double *pts, const double *pose7_twc, const double *calib8, int n_rays, const float *uv, float radius_px,
                 int iterations, uint32_t seed, float *pose16, int *info8);

    // depth from motion (alva_depth_sweep).  depth_keep: level 0 of the current frame's pyramid is copied into slot 0..3 of the ring of
    // reference images (device to device, on the stages' stream).  depth_sweep: the current frame's level 0 swept against that slot;
    // depth, conf, code [gh][gw] and info8 come back to the host, and with images2 (may be null; for tests) the two images, current then
    // reference, [2][height][width]
    int depth_keep(int slot);
    int depth_sweep(int slot, const double *calib8, const double *T_rc12, const SweepParams &p, double rho_min, double rho_max, float *depth,
                    uint8_t *conf, uint8_t *code, int *info8, uint8_t *images2);

    // dense depth (alva_depth_fuse / alva_depth_fill): the fused state (rho, w, src per grid pixel) lives on the device, allocated by the
    // first depth_dense call.  mode 2: sweep against ring slot `slot` (slot < 0: no measurement), fuse with the kept state warped by
    // T_cp12, keep the result, fill it; mode 1: the same without a kept state (one of another grid size is dropped); mode 0: fill the kept
    // state as it is.  The guide is level 0 of the current pyramid.  Nothing but the final images comes back to the host: depth, weight,
    // src, level [gh][gw]; info16 gets the fuse counts [0..5] (modes 1, 2), filled [6], empty [7], gw, gh [8, 9] and the sweep's count of
    // code 0 [11].  The debug pointers (each may be null; for tests) receive the state before and after (before: zeros in mode 1), the raw
    // sweep outputs (zeros / code 255 without a sweep) and the gray image [height][width].  Whether there is a state to warp or fill, and
    // of which frame, is the caller's to know: this object holds the buffers and the grid they were last written on, and refuses modes 0
    // and 2 on another grid
    struct DepthDense {
        int mode, slot;
        const double *calib8, *T_rc12, *T_cp12;
        SweepParams sweep;
        int max_level, decay, w_max;
        double rho_min, rho_max, rel_tol, rho_ref;
        float *depth;
        uint8_t *weight, *src, *level;
        int *info16;
        float *dbg_rho_before, *dbg_rho_after, *dbg_raw_depth;
        uint8_t *dbg_w_before, *dbg_raw_conf, *dbg_raw_code, *dbg_gray;
    };
    int depth_dense(const DepthDense &c);

    // scene mesh (alva_mesh_integrate / alva_mesh_extract): the volume (q int16, w uint8, each [N][N][N]) lives on the device, allocated
    // by the first mesh_update, the extraction's device-side outputs by the first mesh_extract; a session that never asks has neither
    // (the extraction's scratch is the context's, shared with the other synchronous stages).  mesh_update: sweep
    // against ring slot `slot` exactly as depth_dense does and integrate the sweep's DEVICE outputs with (origin3, voxel, trunc, T_cw12,
    // w_max) -- no depth image crosses to the host; `zero` empties the volume first (a new placement), and a volume of another N is
    // replaced by an empty one.  info8 = the stage's, *swept0 the sweep's count of code 0.  The debug pointers (each may be null; for
    // tests) receive the raw sweep outputs [gh][gw] and the volume after the update [N][N][N].  mesh_extract: the volume extracted with
    // (origin3, voxel, min_weight) into the caller's arrays, vertices / normals [max_vertices][3], triangles [max_triangles][3], of which
    // only the first info8[1] / info8[2] rows are written, and nothing unless info8[0] == 0; ALVA_ERR_STATE without a volume.
    // mesh_clear zeroes the volume (the memory is kept).  Where the volume lies in the world is the caller's to know
    // Mesh colour (alva_color_thumb / alva_mesh_integrate_color / alva_mesh_color_at): the thumbnail of the last coloured frame and the
    // colour volume (u8 [N^3][4]) live on the device, each allocated by the first call that needs it -- a session that never turns mesh
    // colour on has neither.  color_frame: the current frame's device-visible source reduced with `cstep` into the kept thumbnail; it
    // only enqueues, and where the source is the caller's own memory it either waits until the launch has read it (wait = true: a
    // polled completion word, or the stream) or leaves that to the caller, who has a wait of its own coming on the same stream (wait =
    // false; *pending says whether one is owed).  frame_wait is that wait where nothing else supplied it.  mesh_update with color_on keeps
    // the colour volume beside the distance volume -- allocated, replaced and zeroed with it -- and with color_fuse integrates through
    // alva_mesh_integrate_color with the kept thumbnail (info8[6] = voxels coloured).  mesh_extract with `colors` ([max_vertices][4])
    // samples the colour volume at the extraction's device-side vertices before the download (alpha 255 where a vertex has a colour, 0
    // where it has none, all zero without a colour volume; *n_colored the count).  mesh_color_at: n world points points3 [n][3] ->
    // rgba [n][4], codes [n], info8; ALVA_ERR_STATE without a colour volume.  mesh_color_debug: the kept thumbnail [th][tw][4] and the
    // colour volume [N^3][4] (each may be null; zeros where there is none).  mesh_color_drop frees both
    int color_frame(int cstep, bool wait, bool *pending);
    int frame_wait();
    bool has_mesh_color() const { return mesh.block && mesh_color.is(mesh.N); }
    int mesh_color_at(const double *origin3, double voxel, int n, const float *points3, uint8_t *rgba, uint8_t *codes, int *info8);
    int mesh_color_debug(uint8_t *thumb, uint8_t *c);
    int mesh_color_drop();

    struct MeshUpdate {
        int slot, N;
        bool zero;
        bool color_on, color_fuse;
        int cstep;
        const double *calib8, *T_rc12, *origin3, *T_cw12;
        double voxel, trunc, rho_min, rho_max;
        SweepParams sweep;
        int w_max;
        int *info8, *swept0;
        float *dbg_raw_depth;
        uint8_t *dbg_raw_conf, *dbg_raw_code;
        int16_t *dbg_q;
        uint8_t *dbg_w;
    };
    int mesh_update(const MeshUpdate &c);
    int mesh_extract(const double *origin3, double voxel, int min_weight, int max_vertices, int max_triangles, float *vertices, float *normals,
                     int *triangles, int *info8, uint8_t *colors = nullptr, int *n_colored = nullptr);
    int mesh_clear();
    // following the camera (alva_mesh_shift): the volume -- and the colour volume, where there is one -- shifted by shift3 voxels into
    // a second block, which then takes the first one's place: every reader goes through mesh_q / mesh_w / mesh_color and sees
    // the shifted volume from the next call on.  The second volume block and the second colour block are each allocated by the first
    // shift that needs them: a session that never shifts has neither.  info8 = the stage's; ALVA_ERR_STATE without a volume
    int mesh_shift(const int *shift3, int *info8);
    // the mesh in blocks (alva_mesh_block_digest / alva_mesh_extract_blocks), the volume only read.  mesh_block_digest: the digest pass
    // with (lattice3, min_weight, B) and one download: digest [nb], counts [nb][2], nb3.  mesh_extract_blocks: the n_sel (>= 1) blocks
    // sel_keys extracted into the extraction's device block -- n_vertices and n_triangles are the selection's sums, which the caller
    // has from the digest pass, and the caps -- then, with `colors`, the colour sampler on the packed vertices (zeros without a colour
    // volume), then one set of downloads: vertices / normals [n_vertices][3], colors [n_vertices][4], triangles [n_triangles][3],
    // ranges [n_sel][4], info8 the stage's.  The digest pass's device block is allocated by its first call: a session that never
    // asks has none.  ALVA_ERR_STATE without a volume
    int mesh_block_digest(const int *lattice3, int min_weight, int B, std::vector<uint64_t> &digest, std::vector<int> &counts, int *nb3);
    int mesh_extract_blocks(const double *origin3, double voxel, const int *lattice3, int min_weight, int B, int n_sel, const int *sel_keys,
                            int n_vertices, int n_triangles, float *vertices, float *normals, uint8_t *colors, int *triangles, int *ranges,
                            int *info8);

    // raycasting the kept volume (alva_mesh_raycast / alva_mesh_raycast_pixels) with (origin3, voxel, min_weight, t_near, t_far); the
    // volume is only read.  T_wc12 null: the n world rays rays6 [n][6].  Otherwise the pixels of a width x height image seen from T_wc12
    // with calib8: uv null: the grid of `step`, n = (width / step) (height / step); else the n raw pixels uv [n][2].  t [n], points and
    // normals [n][3], codes [n], poses [n][16], pose_ok [n] (each may be null; poses only for pixels) come back to the host, and info8.
    // The rays and the outputs have one device block that is allocated by the first call and grows with n: a session that never asks
    // has none.  ALVA_ERR_STATE without a volume
    struct MeshRaycast {
        const double *origin3;
        double voxel;
        int min_weight, n;
        const double *rays6, *T_wc12, *calib8;
        int width, height, step;
        const float *uv;
        double t_near, t_far;
        float *t, *points, *normals;
        uint8_t *codes;
        float *poses;
        uint8_t *pose_ok;
        int *info8;
    };
    int mesh_raycast(const MeshRaycast &c);

    // light estimation (alva_light_bin / alva_light_fuse / alva_light_estimate): the frame accumulators and the environment state live on
    // the device, allocated by the first light_frame.  light_frame: the current frame -- the device-visible source its images were built
    // from -- is binned with R_wc9 (row-major; null: not tracking, the frame's own values only) on the grid of `step` and fused into the
    // state with (min_pixels, w_new, w_max); it only enqueues, and waits (for the bin, not for the fuse) only where the source is the
    // caller's own memory, which the caller may overwrite once the call returns.  light_estimate: the state projected, one launch and one
    // download; dbg_acc (ALVA_LIGHT_ACC_WORDS) and dbg_state (ALVA_LIGHT_STATE_BYTES), each may be null, receive the last frame's
    // accumulators and the state.  light_clear empties the state
    int light_frame(const double *R_wc9, int step, int min_pixels, int w_new, int w_max);
    int light_estimate(float *sh27, float *primary_dir3, float *primary_rgb3, float *ambient4, int *info8, uint64_t *dbg_acc, uint8_t *dbg_state);
    int light_clear();

    // image detection (alva_image_match / alva_image_homography).  image_describe: a picture (gray, host memory, rows `pitch` apart)
    // through ORB with nfeatures 500, scale 1.2, `nlevels` levels, FAST threshold 20 -> at most 512 keypoints (level-0 pixels, xy
    // [512][2]) and descriptors (desc [512][32]); the detector object lives for the call only.  image_detect: see ImageDetectCall
    struct ImageDetectCall {
        int n_images = 0;
        const uint8_t *desc = nullptr;   // [n_images][512][32]
        const float *xy = nullptr;       // [n_images][512][2]
        const int *nq = nullptr, *wh = nullptr;   // [n_images], [n_images][2]
        long version = 0;                // changes whenever the set of pictures does: the device copy is kept until then
        int iterations = 256, min_inliers = 20;
        float threshold_px = 3.f;
        // per image: stage 2's H, mask and info {code, pairs, winning iteration, its count, inliers after the refinement, 0, frame
        // keypoints, 0}, and (R, t) AFTER alva_pnp_refine for code 0 (code 4 when the refinement fails or keeps fewer than min_inliers)
        double *H9 = nullptr, *R9 = nullptr, *t3 = nullptr;
        int *info8 = nullptr;
        uint8_t *mask = nullptr;         // [n_images][512]
        // what the call saw, for replaying the stages (each may be null): the frame's keypoints [2048][2], undistorted [2048][2],
        // descriptors [2048][32], their count; stage 1's pairs [n_images][512][3], coordinates [n_images][512][4], counts; stage 2's own
        // info, R and t (before the refinement)
        float *dbg_kp = nullptr, *dbg_unpx = nullptr;
        uint8_t *dbg_desc = nullptr;
        int *dbg_n_frame = nullptr, *dbg_match = nullptr, *dbg_count = nullptr, *dbg_stage_info8 = nullptr;
        double *dbg_xy = nullptr, *dbg_stage_R9 = nullptr, *dbg_stage_t3 = nullptr;
    };
    int image_describe(const uint8_t *gray, int width, int height, size_t pitch, int nlevels, float *xy, uint8_t *desc, int *count);
    int image_detect(const ImageDetectCall &c);

    // planes (alva_detect_planes where n_prior = 0, else alva_track_planes): the n_prior records prior24 keep their slots, up to
    // max_planes - n_prior new planes among the other points follow; labels [n] may be null.  max_vertices > 0: the planes' outlines too
    // (alva_plane_outlines on the same upload: points and labels stay on the device between the two) -- outline
    // [max_planes][max_vertices][2], outline_info8 [max_planes][8], area [max_planes]; max_vertices = 0: none, and the three are not
    // touched
    struct PlaneCall {
        int n;
        const double *pts, *pose7_twc;
        double thickness;
        int min_inliers, max_planes, iterations;
        uint32_t seed;
        int n_prior;
        const float *prior24;
        float *planes24;
        int *info8, *labels;
        int max_vertices;
        float *outline;
        int *outline_info8;
        double *area;
    };
    int planes(const PlaneCall &c);

    // anchors (alva_anchor_attach): per anchor position pos3[a] the max_support nearest of the n points; index, dist2
    // [n_anchors][max_support], count [n_anchors]
    int anchor_attach(int n, const double *pts, int n_anchors, const double *pos3, int max_support, int *index, double *dist2, int *count);
    // anchors (alva_anchor_update): the rigid motion of each anchor's supports ref -> cur ([n_anchors][64][3], count [n_anchors]) applied
    // to its reference pose; pose16 [n_anchors][16], info8 [n_anchors][8]
    int anchor_update(int n_anchors, const int *count, const double *ref, const double *cur, const float *pose16_ref, float *pose16, int *info8);

private:
    HipStages &hs;
    // depth from motion: the ring of reference images (DEPTH_SLOTS copies of a pyramid's level 0, in its pitch), allocated by the first
    // depth_keep -- a session that never turns depth on never has it.  sweep: alva_depth_sweep of the current level 0 against ring
    // slot `slot` into three DEVICE buffers [gh][gw]; ALVA_ERR_ARG for a slot the ring does not have
    static constexpr int DEPTH_SLOTS = 4;
    DeviceBlock depth_ring;
    size_t depth_slot_bytes = 0;
    int sweep(int slot, const double *calib8, const double *T_rc12, const SweepParams &p, double rho_min, double rho_max, float *d_depth,
              uint8_t *d_conf, uint8_t *d_code, int *info8);
    // dense depth: the fused state, two copies of (rho f32, w u8) that take turns as a fuse's input and output, and the src image of the
    // last fuse; one block of 11 bytes per grid pixel, allocated by the first depth_dense and again when a call's grid has more pixels
    // -- a session that never asks for dense depth never has it
    DeviceBlock dense_block;
    size_t dense_cap() const { return dense_block.bytes / 11; }   // grid pixels the block holds
    int dense_gw = 0, dense_gh = 0, dense_cur = 0;   // the grid of the last fuse (0 x 0: none yet) and which copy it wrote
    float *dense_rho(int k) const { return (float *) (dense_block.ptr + (size_t) k * 5 * dense_cap()); }
    uint8_t *dense_w(int k) const { return dense_block.ptr + (size_t) k * 5 * dense_cap() + 4 * dense_cap(); }
    uint8_t *dense_src() const { return dense_block.ptr + 10 * dense_cap(); }
    // scene mesh: the volume (q int16 [N^3], then w uint8 [N^3]) allocated by the first mesh_update and again when N changes, and the
    // extraction's outputs, one block (vertices, normals, triangles, colours) that grows with the caps asked for
    Volume mesh;
    DeviceBlock mesh_out;
    DeviceBlock mesh_digest_out;   // the digest pass's outputs (u64 [nb], then i32 [nb][2]), grow-only
    int16_t *mesh_q() const { return (int16_t *) mesh.block.ptr; }
    uint8_t *mesh_w() const { return mesh.block.ptr + 2 * mesh.voxels(); }
    // mesh colour: the colour volume (u8 [N^3][4]); the kept thumbnail (rounded up to 256, then 256 bytes for the launch's arrival
    // counter; color_thumb_exact = [th][tw][4]) and the wait for the launch that reduces a frame into it
    Volume mesh_color;
    DeviceBlock color_thumb;
    size_t color_thumb_exact = 0;
    FrameRead color_read;
    // following the camera: the volumes a shift writes into and then swaps with mesh / mesh_color
    Volume mesh_alt, mesh_color_alt;
    // raycast: one block for ray_cap() rays -- the rays (48 bytes each: world rays, or pixels in the first 8), t, point, normal, pose, code,
    // pose_ok -- allocated by the first mesh_raycast, and again when a call has more rays
    DeviceBlock ray_block;
    static constexpr size_t RAY_BYTES = 48 + 4 + 12 + 12 + 64 + 1 + 1;
    size_t ray_cap() const { return ray_block.bytes / RAY_BYTES; }
    int ray_reserve(size_t n);
    // light estimation: one block -- the frame accumulators, their copy of the last fuse, the environment state -- allocated by the
    // first light_frame: a session with light off never has it
    DeviceBlock light_block;
    FrameRead light_read;   // the word the fuse publishes when it starts (the bin before it is done)
    static constexpr size_t LIGHT_ACC_BYTES = (ALVA_LIGHT_ACC_WORDS * 8 + 255) / 256 * 256;
    uint64_t *light_acc() const { return (uint64_t *) light_block.ptr; }
    uint64_t *light_acc_last() const { return (uint64_t *) (light_block.ptr + LIGHT_ACC_BYTES); }
    uint8_t *light_state() const { return light_block.ptr + 2 * LIGHT_ACC_BYTES; }
    static constexpr size_t LIGHT_BLOCK_BYTES = 2 * LIGHT_ACC_BYTES + ALVA_LIGHT_STATE_BYTES;
    // image detection: the frame-size ORB object (1500 features, 1.2, 8 levels, threshold 20) and one device block -- the frame's
    // keypoints, descriptors and points, the pictures' descriptors and keypoints, the stages' outputs, the refinement's inputs -- both
    // made by the first image_detect: a session that never adds a picture has neither
    alva_orb *img_orb = nullptr;
    DeviceBlock img_block;
    long img_version = -1;
    static constexpr size_t IMG_KP = 0, IMG_DESC = IMG_KP + (size_t) ALVA_IMAGE_TRAIN_CAP * 24, IMG_XY = IMG_DESC + (size_t) ALVA_IMAGE_TRAIN_CAP * 32,
                            IMG_UNPX = IMG_XY + (size_t) ALVA_IMAGE_TRAIN_CAP * 8, IMG_QDESC = IMG_UNPX + (size_t) ALVA_IMAGE_TRAIN_CAP * 8,
                            IMG_QXY = IMG_QDESC + (size_t) ALVA_IMAGE_MAX * ALVA_IMAGE_QUERY_CAP * 32,
                            IMG_MATCH = IMG_QXY + (size_t) ALVA_IMAGE_MAX * ALVA_IMAGE_QUERY_CAP * 8,
                            IMG_PAIRS = IMG_MATCH + (size_t) ALVA_IMAGE_MAX * ALVA_IMAGE_QUERY_CAP * 16,
                            IMG_COUNT = IMG_PAIRS + (size_t) ALVA_IMAGE_MAX * ALVA_IMAGE_QUERY_CAP * 32, IMG_UV = IMG_COUNT + 256,
                            IMG_WPT = IMG_UV + (size_t) ALVA_IMAGE_QUERY_CAP * 16, IMG_BLOCK_BYTES = IMG_WPT + (size_t) ALVA_IMAGE_QUERY_CAP * 24;
};

}  // namespace alva_slam
