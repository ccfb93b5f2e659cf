// What the two halves of the session share: system.hip (create / configure / reset, the frame path, find-plane, inspection, shared ids,
// groups) and system_scene.hip (the scene features' entry points).  Internal to the library; no logic of its own.
#pragma once
#include "common.hpp"
#include "scene_stages.hpp"
#include "slam/slam.hpp"
#include "slam/anchors.hpp"
#include "slam/mesh_blocks.hpp"
#include "slam/plane_tracks.hpp"
#include "slam/stage_trace.hpp"
#include "../../include/alvaar_system.h"
#include "../../include/alvaar_system_testing.h"
#include <memory>
#include <vector>

using namespace alva_slam;

// the session's own error text (alva_system_last_error falls back to the library's when it is empty); defined in system.hip
extern thread_local char g_sys_err[256];
inline int sys_fail(int rc, const char *what) {
    snprintf(g_sys_err, sizeof(g_sys_err), "%s: %s", what, alva_last_error());
    return rc;
}

struct alva_system {
    int device = 0;
    std::unique_ptr<HipStages> stages;
    std::unique_ptr<SceneStages> scene;  // the scene features' device side: of one configuration, made after `stages` and destroyed before it
    std::unique_ptr<TraceStages> trace;  // ALVA_STAGE_TRACE=<file>: log every stage call (debugging aid, see slam/stage_trace.hpp)
    std::unique_ptr<Slam> slam;
    void *hip_stream = nullptr;   // alva_system_set_stream: the stream the next configure builds the stages on (null: a stream of its own)
    // findCameraPoseWithIMU (system.cpp:57-104)
    double imu_translation[3] = {0, 0, 0}, prev_translation[3] = {0, 0, 0};
    // alva_system_set_relocalization: kept here too, so that it holds across alva_system_configure*
    bool reloc_enabled = false;
    int reloc_max_lost = 0;
    // what the last find_camera_pose* returned (0: none since configure / reset): alva_system_hit_test answers only while it is 1
    int last_status = 0;
    bool frame_seen = false;   // a frame has been processed since configure: the pyramid holds one

    // ---- the scene features' session state: one member per feature.  What belongs to one map (Slam::map_generation) and one
    // configuration has clear(), sync(map_generation) and generation; each entry point syncs its own feature before it reads it ----
    // alva_system_track_planes: the planes kept between its calls
    PlaneTracks plane_tracks;
    // alva_system_create_anchors / alva_system_update_anchors: the anchors kept between calls
    Anchors anchors;
    // alva_system_set_depth: kept here, so that it holds across alva_system_configure* (as relocalization)
    bool depth_enabled = false;
    struct Depth {
        // depth from motion: the poses of the reference frames whose images the scene stages keep (entry i = their ring slot i); seq 0 =
        // free, the largest seq is the newest
        struct Ref {
            SE3 Twc;
            long seq = 0;
        };
        Ref ring[4];
        long seq = 0, generation = 0;
        // alva_system_depth_dense: what the session knows of the fused state the scene stages keep on the device -- the grid it is on, the
        // pose and the frame it was last fused in, and that fuse's part of h_info16 for a second call on the same frame.  Emptied with the ring
        struct Dense {
            bool valid = false;
            int gw = 0, gh = 0, step = 0;
            SE3 Twc;
            int frame = -1;   // the tracker's frame id (FrameRec::id, advanced by every processed frame, through a group too)
            int counts[6] = {0, 0, 0, 0, 0, 0}, swept0 = 0, warped = 0;
        };
        Dense dense;
        void clear() {
            for (Ref &e: ring) e.seq = 0;
            dense.valid = false;
        }
        void sync(long map_generation) {
            if (map_generation != generation) clear();
            generation = map_generation;
        }
    } depth;
    // alva_system_mesh_update / alva_system_mesh: the volume itself lives in the scene stages, on the device; here is what the session
    // knows of it -- that there is one, where it lies in the world (placed by the call that made it, then moved only in whole voxels:
    // alva_system_set_mesh_follow, alva_system_mesh_move), the frame last integrated and how many were.  Of one map and one
    // configuration; emptied with the depth ring too (the mesh is made of depth).  The placement chose origin0, side and the median
    // depth m0; `offset` counts the voxels the volume has been shifted by since, and origin is ALWAYS origin0 + (double) offset voxel,
    // computed afresh (place_origin) so that nothing accumulates -- with offset 0 that is origin0's bits.  Whatever empties or replaces
    // the volume clears offset and the two tallies
    struct Mesh {
        bool valid = false;
        int N = 0;
        double rel_extent = 0, origin[3] = {0, 0, 0}, voxel = 0, trunc = 0;
        double origin0[3] = {0, 0, 0}, m0 = 0, side = 0;
        long long offset[3] = {0, 0, 0}, shifts = 0, lost = 0;   // lost: weighted voxels that left the cube
        int frame = -1;   // the tracker's frame id of the last integration (FrameRec::id)
        int frames = 0;
        long generation = 0;
        long long volume = 0;   // moves on whenever the volume is emptied, placed or replaced (never by a shift): alva_system_mesh_blocks' G2
        void place_origin() {
            for (int i = 0; i < 3; i++) origin[i] = origin0[i] + (double) offset[i] * voxel;
        }
        void clear() {
            valid = false;
            volume++;
            frame = -1;
            frames = 0;
            offset[0] = offset[1] = offset[2] = 0;
            shifts = lost = 0;
        }
        void sync(long map_generation) {
            if (map_generation != generation) clear();
            generation = map_generation;
        }
    } mesh;
    // alva_system_mesh_blocks: the present blocks of the last successful call (G2 - G6); empty until the first call
    alva_slam::MeshBlockList mesh_blocks;
    // alva_system_set_mesh_follow: the block in voxels, 0 = off; kept here, so that it holds across alva_system_configure* (as depth)
    int mesh_follow = 0;
    // alva_system_set_mesh_color: kept here, so that it holds across alva_system_configure* (as depth).  The thumbnail of the last
    // coloured frame and the colour volume live in the scene stages, on the device; here is the frame the thumbnail was taken from (the
    // tracker's frame id, -1: none).  The colour volume shares the mesh's validity: what empties the volume empties the colour
    bool mesh_color_enabled = false;
    struct MeshColor {
        int thumb_frame = -1;
        void clear() { thumb_frame = -1; }
    } mesh_color;
    // alva_system_set_light: kept here, so that it holds across alva_system_configure* (as depth)
    bool light_enabled = false;
    // The environment itself lives in the scene stages, on the device; here is what the session knows of it: whether a frame has been fed
    // since it was last emptied, the map it belongs to, and the rotation the last frame was binned with (for alva_system_debug_light).
    // clear and sync take the scene stages that hold the environment (null: unconfigured, nothing on a device to empty)
    struct Light {
        bool fed = false, has_R = false;
        long generation = 0;
        int frames = 0;
        double R[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        void clear(SceneStages *scene) {
            if (fed && scene) (void) scene->light_clear();
            fed = has_R = false;
            frames = 0;
        }
        void sync(long map_generation, SceneStages *scene) {
            if (map_generation != generation) clear(scene);
            generation = map_generation;
        }
    } light;
    // alva_system_add_image: the pictures are the app's data and are kept HERE, on the host, as they were described -- the scene stages keep
    // a device copy that goes with them at every configure and is made again from this (version tells them when).  Of no map and of no
    // configuration: the list and its id counter hold across alva_system_configure* and alva_system_reset
    struct ImageTarget {
        int id = 0, w = 0, h = 0, nq = 0;
        double width_m = 0;
        std::vector<float> xy;       // [nq][2] level-0 pixels
        std::vector<uint8_t> desc;   // [nq][32]
    };
    struct Images {
        std::vector<ImageTarget> list;   // ascending id
        int next_id = 0;
        long version = 0;
        void clear() {
            list.clear();
            version++;
        }
    } images;
};

// No C++ exception may cross the C ABI (the reference's contract: "no exceptions"): the map layer keeps the reference's
// .at() look-ups (std::out_of_range on an inconsistent map) and its containers can throw std::bad_alloc.  Every entry point that runs
// the map layer goes through guarded(): the error text is kept, the tracker is asked to reset (what the reference's own failure paths
// do, visual_frontend.cpp:73-92) and ALVA_ERR_STATE is returned.
template <class F>
int guarded(alva_system *s, const char *what, F &&body) {
    try {
        return body();
    } catch (const std::exception &e) {
        snprintf(g_sys_err, sizeof(g_sys_err), "%s: %s", what, e.what());
    } catch (...) {
        snprintf(g_sys_err, sizeof(g_sys_err), "%s: unknown C++ exception", what);
    }
    if (s && s->stages) (void) s->stages->frame_done();   // no kernel keeps reading a caller-owned frame buffer behind an error return
    if (s && s->slam) s->slam->reset_requested = true;
    return ALVA_ERR_STATE;
}

// MapManager::getCurrentFrameMapPoints (map_manager.cpp:340-357): observed 3-D map points, in the map's container order
inline void frame_map_points(const Slam &S, std::vector<double> *xyz, std::vector<int> *ids) {
    for (const auto &e: S.map_points)
        if (e.second->r->observed && e.second->r->is3d) {
            if (xyz) xyz->insert(xyz->end(), e.second->r->X, e.second->r->X + 3);
            if (ids) ids->push_back(e.first);
        }
}

// system_scene.hip.  After every frame that was processed: the features that follow the frames (depth, light) take theirs
void scene_after_frame(alva_system *s);
// what alva_system_configure* and alva_system_reset do to the scene features' state (the one list of each)
void scene_configured(alva_system *s);
void scene_reset(alva_system *s);
