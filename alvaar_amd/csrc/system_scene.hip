// The scene features of a session as a C ABI (include/alvaar_system.h; none has a counterpart in the reference): hit test, depth from
// motion, dense depth, scene mesh and its raycast and colour, light estimation, image detection, planes, anchors.  Each entry point reads the map layer's state (system_impl.hpp:
// the session object), runs the feature's device side (scene_stages.hip) and keeps the feature's own session state -- which belongs to one
// map and one configuration, and is brought up to date (sync) by the entry point that reads it.
#include "system_impl.hpp"
#include "slam/image_place.hpp"
#include <algorithm>
#include <cmath>

// The two refusals most entry points share (every entry point clears g_sys_err first, then checks)
static int bad_argument(const char *what, const char *text = "not configured or bad argument") {
    snprintf(g_sys_err, sizeof(g_sys_err), "%s: %s", what, text);
    return ALVA_ERR_ARG;
}
static int switched_off(const char *what, const char *feature, const char *its_switch) {
    snprintf(g_sys_err, sizeof(g_sys_err), "%s: %s is off (%s)", what, feature, its_switch);
    return ALVA_ERR_STATE;
}

// ---- depth from motion (alva_depth_sweep in alvaar_hip.h defines the stage; the reference frames are kept here and in the scene stages) ----
constexpr double DEPTH_MIN_BASELINE = 0.03;   // of the median depth of the frame's 3-D points
constexpr double DEPTH_MIN_COS = 0.9;         // between the optical axes of the current and the reference frame
constexpr int DEPTH_MIN_POINTS = 8;

// the camera-space z of the current frame's observed 3-D points, ascending; only what lies in front of the camera
static void depth_frame_z(const Slam &S, std::vector<double> &z) {
    std::vector<double> pts;
    frame_map_points(S, &pts, nullptr);
    double R[9];
    quat_to_rot(S.cur->Twc.q, R);
    const double *t = S.cur->Twc.t;
    for (size_t i = 0; i + 2 < pts.size(); i += 3) {
        const double zc = (R[2] * (pts[i] - t[0]) + R[5] * (pts[i + 1] - t[1])) + R[8] * (pts[i + 2] - t[2]);   // R_wc^T (X - t), row 3
        if (zc > 0) z.push_back(zc);
    }
    std::sort(z.begin(), z.end());
}

static double depth_baseline(const SE3 &a, const SE3 &b) {
    const double d0 = a.t[0] - b.t[0], d1 = a.t[1] - b.t[1], d2 = a.t[2] - b.t[2];
    return std::sqrt(d0 * d0 + d1 * d1 + d2 * d2);
}

// after a tracked frame: its image and pose join the ring when the ring is empty or the camera has moved far enough from the newest
// entry.  A failure here (no memory for the ring) costs the entry, never the frame
static void depth_after_frame(alva_system *s) {
    if (s->last_status != 1 || !s->slam || !s->scene) return;
    try {
        s->depth.sync(s->slam->map_generation);
        int newest = -1, slot = 0;
        for (int i = 0; i < 4; i++) {
            if (s->depth.ring[i].seq > 0 && (newest < 0 || s->depth.ring[i].seq > s->depth.ring[newest].seq)) newest = i;
            if (s->depth.ring[i].seq < s->depth.ring[slot].seq) slot = i;   // a free entry, or the oldest
        }
        if (newest >= 0) {
            std::vector<double> z;
            depth_frame_z(*s->slam, z);
            if ((int) z.size() < DEPTH_MIN_POINTS) return;
            if (!(depth_baseline(s->slam->cur->Twc, s->depth.ring[newest].Twc) >= DEPTH_MIN_BASELINE * z[z.size() / 2])) return;
        }
        if (s->scene->depth_keep(slot) != ALVA_OK) return;
        s->depth.ring[slot].Twc = s->slam->cur->Twc;
        s->depth.ring[slot].seq = ++s->depth.seq;
    } catch (...) {
    }
}

// ---- light estimation (alva_light_bin / alva_light_fuse / alva_light_estimate in alvaar_hip.h define the stages; the environment is kept
// in the scene stages) ----
constexpr int LIGHT_STEP = ALVA_LIGHT_STEP, LIGHT_MIN_PIXELS = ALVA_LIGHT_MIN_PIXELS, LIGHT_W_NEW = ALVA_LIGHT_W_NEW, LIGHT_W_MAX = ALVA_LIGHT_W_MAX;

// after every frame that was processed: the colour frame is binned -- with the frame's rotation when it was tracked, for its own values
// only when not -- and fused.  Enqueued behind the frame's kernels; a failure here costs the frame's light, never the frame
// -> true when the frame was binned and fused (and so, where the frame is the caller's memory, waited for)
static bool light_after_frame(alva_system *s) {
    if (s->last_status < 0 || !s->slam || !s->scene) return false;
    s->light.sync(s->slam->map_generation, s->scene.get());
    const bool tracked = s->last_status == 1;
    double R[9];
    if (tracked) quat_to_rot(s->slam->cur->Twc.q, R);
    if (s->scene->light_frame(tracked ? R : nullptr, LIGHT_STEP, LIGHT_MIN_PIXELS, LIGHT_W_NEW, LIGHT_W_MAX) != ALVA_OK) return false;
    s->light.fed = true;
    s->light.has_R = tracked;
    s->light.frames++;
    for (int i = 0; i < 9; i++) s->light.R[i] = tracked ? R[i] : 0.;
    return true;
}

// ---- mesh colour (alva_color_thumb / alva_mesh_integrate_color / alva_mesh_color_at in alvaar_hip.h define the stages; the thumbnail and
// the colour volume are kept in the scene stages) ----
constexpr int MESH_COLOR_STEP = ALVA_MESH_COLOR_STEP;

// after a tracked frame: its colour is reduced to the kept thumbnail, inside the frame -- a device frame is the caller's memory, which it
// may overwrite once the call returns, and alva_system_mesh_update comes later.  Enqueued behind the frame's kernels.  Where the frame
// is the caller's memory the launch must have read it before the call returns: with light on, light's own wait on the same stream,
// which follows, covers it (-> true: that wait is owed); otherwise it waits here.  A failure costs the frame's colour, never the frame
static bool color_after_frame(alva_system *s, bool light_follows) {
    if (s->last_status != 1 || !s->slam || !s->scene) return false;
    bool pending = false;
    if (s->scene->color_frame(MESH_COLOR_STEP, !light_follows, &pending) != ALVA_OK) {
        s->mesh_color.clear();
        return false;
    }
    s->mesh_color.thumb_frame = s->slam->cur->id;
    return pending;
}

void scene_after_frame(alva_system *s) {
    const bool light = s->light_enabled && s->last_status >= 0;
    const bool owed = s->mesh_color_enabled && s->depth_enabled && color_after_frame(s, light);
    if (s->depth_enabled) depth_after_frame(s);
    const bool waited = s->light_enabled && light_after_frame(s);
    if (owed && !waited && s->scene) (void) s->scene->frame_wait();   // (light failed before its wait)
}

// a new configuration: a new map, new stages.  Everything that belongs to them is emptied and stamped with the new map's generation
void scene_configured(alva_system *s) {
    const long generation = s->slam->map_generation;
    s->plane_tracks.clear();
    s->plane_tracks.generation = generation;
    s->anchors.clear();
    s->anchors.generation = generation;
    s->depth.clear();   // (the images went with the old stages)
    s->depth.generation = generation;
    s->mesh.clear();    // (the volume too)
    s->mesh.generation = generation;
    s->mesh_color.clear();   // (the thumbnail and the colour volume went with the old stages)
    s->light.fed = false;   // (the environment went with the old stages too: nothing on the device to empty)
    s->light.clear(s->scene.get());
    s->light.generation = generation;
    s->frame_seen = false;
}

// alva_system_reset: what follows the frames starts again; planes and anchors go with the map, when their next call sees its generation
void scene_reset(alva_system *s) {
    s->depth.clear();
    s->mesh.clear();
    s->mesh_color.clear();
    s->light.clear(s->scene.get());
}

extern "C" int alva_system_hit_test(alva_system *s, int n_rays, const float *h_uv, float radius_px, int num_iterations, float *h_pose16,
                                    int *h_info8) {
    g_sys_err[0] = 0;
    if (!s || !s->slam || !h_uv || !h_pose16 || !h_info8 || n_rays < 1 || n_rays > 16 || num_iterations < 1 || num_iterations > 4096 ||
        !(radius_px > 0)) return bad_argument("alva_system_hit_test");
    memset(h_info8, 0, (size_t) n_rays * 8 * sizeof(int));
    if (s->last_status != 1) {   // initialising, reset, LOST or never called: there is no pose to cast a ray from
        for (int r = 0; r < n_rays; r++) {
            h_info8[8 * r] = 5;
            h_info8[8 * r + 2] = -1;
        }
        return 0;
    }
    return guarded(s, "alva_system_hit_test", [&]() -> int {
        std::vector<double> pts;
        frame_map_points(*s->slam, &pts, nullptr);
        double pose7[7];
        se3_to_pose7(s->slam->cur->Twc, pose7);
        const Camera &k = s->slam->cam;
        const int rc = s->scene->hit_test((int) (pts.size() / 3), pts.data(), pose7, camera_calib8(k).data(), n_rays, h_uv, radius_px, num_iterations,
                                          12345u, h_pose16, h_info8);
        if (rc) return sys_fail(rc, "alva_system_hit_test");
        int hits = 0;
        for (int r = 0; r < n_rays; r++) hits += h_info8[8 * r] == 0;
        return hits;
    });
}

extern "C" int alva_system_set_depth(alva_system *s, int enabled) {
    g_sys_err[0] = 0;
    if (!s) return bad_argument("alva_system_set_depth", "bad argument");
    s->depth_enabled = enabled != 0;
    if (!s->depth_enabled) {
        s->depth.clear();
        s->mesh.clear();
    }
    return ALVA_OK;
}

extern "C" int alva_system_set_mesh_color(alva_system *s, int enabled) {
    g_sys_err[0] = 0;
    if (!s) return bad_argument("alva_system_set_mesh_color", "bad argument");
    const bool on = enabled != 0;
    if (on == s->mesh_color_enabled) return ALVA_OK;
    s->mesh_color_enabled = on;
    s->mesh_color.clear();
    // a change empties the colours: what was fused while it was on last time is not what the volume has seen since
    if (s->scene && s->scene->mesh_color_drop() != ALVA_OK) return sys_fail(ALVA_ERR_HIP, "alva_system_set_mesh_color");
    return ALVA_OK;
}

extern "C" int alva_system_set_light(alva_system *s, int enabled) {
    g_sys_err[0] = 0;
    if (!s) return bad_argument("alva_system_set_light", "bad argument");
    s->light_enabled = enabled != 0;
    if (!s->light_enabled) s->light.clear(s->scene.get());
    return ALVA_OK;
}

extern "C" int alva_system_reset_light(alva_system *s) {
    g_sys_err[0] = 0;
    if (!s) return bad_argument("alva_system_reset_light", "bad argument");
    s->light.clear(s->scene.get());
    return ALVA_OK;
}

static int light_impl(alva_system *s, const char *what, float *h_sh27, float *h_primary_dir3, float *h_primary_rgb3, float *h_ambient4,
                      int *h_info8, uint64_t *dbg_acc, double *dbg_R9, int *dbg_flags4, uint8_t *dbg_state) {
    g_sys_err[0] = 0;
    if (!s || !s->slam || !s->scene || !h_sh27 || !h_primary_dir3 || !h_primary_rgb3 || !h_ambient4 || !h_info8) return bad_argument(what);
    if (!s->light_enabled) return switched_off(what, "light", "alva_system_set_light");
    s->light.sync(s->slam->map_generation, s->scene.get());   // (a new map empties the environment in here)
    if (dbg_R9) memcpy(dbg_R9, s->light.R, sizeof(s->light.R));
    if (dbg_flags4) {
        dbg_flags4[0] = s->light.fed ? 1 : 0;
        dbg_flags4[1] = s->light.has_R ? 1 : 0;
        dbg_flags4[2] = s->light.frames;
        dbg_flags4[3] = 0;
    }
    if (!s->light.fed) {   // no frame since light was turned on (or since the environment was emptied): nothing is launched
        memset(h_sh27, 0, 27 * sizeof(float));
        memset(h_primary_dir3, 0, 3 * sizeof(float));
        memset(h_primary_rgb3, 0, 3 * sizeof(float));
        h_ambient4[0] = 0.f;
        h_ambient4[1] = h_ambient4[2] = h_ambient4[3] = 1.f;
        memset(h_info8, 0, 8 * sizeof(int));
        h_info8[0] = 5;
        if (dbg_acc) memset(dbg_acc, 0, ALVA_LIGHT_ACC_WORDS * sizeof(uint64_t));
        if (dbg_state) memset(dbg_state, 0, ALVA_LIGHT_STATE_BYTES);
        return 5;
    }
    return guarded(s, what, [&]() -> int {
        const int rc = s->scene->light_estimate(h_sh27, h_primary_dir3, h_primary_rgb3, h_ambient4, h_info8, dbg_acc, dbg_state);
        if (rc) return sys_fail(rc, what);
        return h_info8[0];
    });
}

extern "C" int alva_system_light(alva_system *s, float *h_sh27, float *h_primary_dir3, float *h_primary_rgb3, float *h_ambient4, int *h_info8) {
    return light_impl(s, "alva_system_light", h_sh27, h_primary_dir3, h_primary_rgb3, h_ambient4, h_info8, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int alva_system_debug_light(alva_system *s, float *h_sh27, float *h_primary_dir3, float *h_primary_rgb3, float *h_ambient4,
                                       int *h_info8, uint64_t *h_acc, double *h_R_wc9, int *h_flags4, uint8_t *h_state) {
    return light_impl(s, "alva_system_debug_light", h_sh27, h_primary_dir3, h_primary_rgb3, h_ambient4, h_info8, h_acc, h_R_wc9, h_flags4,
                      h_state);
}

// ---- image detection (alva_image_match / alva_image_homography in alvaar_hip.h define the device stages, slam/image_place.hpp the host side)
extern "C" int alva_system_add_image(alva_system *s, const uint8_t *h_gray, int width, int height, size_t pitch, double width_m) {
    g_sys_err[0] = 0;
    if (!s || !s->slam || !s->scene) {
        snprintf(g_sys_err, sizeof(g_sys_err), "alva_system_add_image: not configured (the picture is described on the session's device)");
        return ALVA_ERR_STATE;
    }
    if (!h_gray || pitch < (size_t) (width > 0 ? width : 0) || !(width_m >= 0)) return bad_argument("alva_system_add_image", "bad argument");
    if (width < 96 || height < 96 || width > 1024 || height > 1024) {
        snprintf(g_sys_err, sizeof(g_sys_err), "alva_system_add_image: a picture of %d x %d pixels: both sides must be 96 .. 1024", width, height);
        return ALVA_ERR_ARG;
    }
    if ((int) s->images.list.size() >= ALVA_IMAGE_MAX) {
        snprintf(g_sys_err, sizeof(g_sys_err), "alva_system_add_image: the session already holds %d pictures, the most it can", ALVA_IMAGE_MAX);
        return ALVA_ERR_STATE;
    }
    int levels = 1;   // the largest L <= 8 with short side / 1.2^(L-1) >= 64
    for (double side = (double) std::min(width, height) / 1.2; levels < 8 && side >= 64.0; side /= 1.2) levels++;
    return guarded(s, "alva_system_add_image", [&]() -> int {
        alva_system::ImageTarget T;
        T.xy.resize((size_t) ALVA_IMAGE_QUERY_CAP * 2);
        T.desc.resize((size_t) ALVA_IMAGE_QUERY_CAP * 32);
        const int rc = s->scene->image_describe(h_gray, width, height, pitch, levels, T.xy.data(), T.desc.data(), &T.nq);
        if (rc) return sys_fail(rc, "alva_system_add_image");
        if (T.nq < ALVA_SYSTEM_IMAGE_MIN_KEYPOINTS) {
            snprintf(g_sys_err, sizeof(g_sys_err), "alva_system_add_image: the picture gives %d ORB keypoints, fewer than the %d a detection needs "
                     "(too little texture)", T.nq, ALVA_SYSTEM_IMAGE_MIN_KEYPOINTS);
            return ALVA_ERR_ARG;
        }
        T.id = s->images.next_id++;
        T.w = width;
        T.h = height;
        T.width_m = width_m;
        s->images.list.push_back(std::move(T));
        s->images.version++;
        return s->images.list.back().id;
    });
}

extern "C" int alva_system_remove_image(alva_system *s, int id) {
    g_sys_err[0] = 0;
    if (!s) return ALVA_ERR_ARG;
    for (size_t i = 0; i < s->images.list.size(); i++)
        if (s->images.list[i].id == id) {
            s->images.list.erase(s->images.list.begin() + (long) i);
            s->images.version++;
            return ALVA_OK;
        }
    snprintf(g_sys_err, sizeof(g_sys_err), "alva_system_remove_image: no picture with id %d", id);
    return ALVA_ERR_ARG;
}

extern "C" int alva_system_reset_images(alva_system *s) {
    g_sys_err[0] = 0;
    if (!s) return ALVA_ERR_ARG;
    s->images.clear();
    return ALVA_OK;
}

static int detect_images_impl(alva_system *s, const char *what, int num_iterations, float threshold_px, int min_inliers, int cap, int *h_ids,
                              float *h_poses16, float *h_extents2, float *h_scale1, float *h_quads8, int *h_info8, const alva_image_debug *dbg) {
    g_sys_err[0] = 0;
    if (!s || !s->slam || !s->scene || !h_ids || !h_poses16 || !h_extents2 || !h_scale1 || !h_quads8 || !h_info8 || cap < 0 ||
        num_iterations < 1 || num_iterations > 4096 || !(threshold_px >= 0) || min_inliers < 0) return bad_argument(what);
    const int n = std::min((int) s->images.list.size(), cap);
    if (n == 0) return 0;   // no picture: nothing is allocated or launched
    memset(h_poses16, 0, (size_t) n * 16 * sizeof(float));
    memset(h_extents2, 0, (size_t) n * 2 * sizeof(float));
    memset(h_scale1, 0, (size_t) n * sizeof(float));
    memset(h_quads8, 0, (size_t) n * 8 * sizeof(float));
    memset(h_info8, 0, (size_t) n * 8 * sizeof(int));
    for (int k = 0; k < n; k++) h_ids[k] = s->images.list[(size_t) k].id;
    if (dbg && dbg->tracked) *dbg->tracked = s->last_status == 1 ? 1 : 0;
    if (!s->frame_seen) {
        for (int k = 0; k < n; k++) {
            h_info8[8 * k] = 7;
            h_info8[8 * k + 2] = -1;
        }
        return 0;
    }
    return guarded(s, what, [&]() -> int {
        constexpr size_t QC = ALVA_IMAGE_QUERY_CAP;
        std::vector<uint8_t> qdesc((size_t) n * QC * 32), mask((size_t) n * QC);
        std::vector<float> qxy((size_t) n * QC * 2);
        std::vector<int> nq((size_t) n), wh((size_t) n * 2);
        std::vector<double> H((size_t) n * 9), R((size_t) n * 9), t((size_t) n * 3);
        for (int k = 0; k < n; k++) {
            const alva_system::ImageTarget &T = s->images.list[(size_t) k];
            nq[(size_t) k] = T.nq;
            wh[2 * (size_t) k] = T.w;
            wh[2 * (size_t) k + 1] = T.h;
            memcpy(qdesc.data() + (size_t) k * QC * 32, T.desc.data(), QC * 32);
            memcpy(qxy.data() + (size_t) k * QC * 2, T.xy.data(), QC * 8);
        }
        SceneStages::ImageDetectCall c;
        c.n_images = n;
        c.desc = qdesc.data();
        c.xy = qxy.data();
        c.nq = nq.data();
        c.wh = wh.data();
        c.version = s->images.version * 16 + n;   // (cap may cut the list)
        c.iterations = num_iterations;
        c.threshold_px = threshold_px;
        c.min_inliers = min_inliers;
        c.H9 = H.data();
        c.R9 = R.data();
        c.t3 = t.data();
        c.info8 = h_info8;
        c.mask = mask.data();
        if (dbg) {
            c.dbg_kp = dbg->kp; c.dbg_unpx = dbg->unpx; c.dbg_desc = dbg->desc; c.dbg_n_frame = dbg->n_frame; c.dbg_match = dbg->match;
            c.dbg_count = dbg->count; c.dbg_xy = dbg->xy; c.dbg_stage_info8 = dbg->stage_info; c.dbg_stage_R9 = dbg->stage_R;
            c.dbg_stage_t3 = dbg->stage_t;
        }
        const int rc = s->scene->image_detect(c);
        if (rc) return sys_fail(rc, what);
        if (dbg) {
            if (dbg->nq) memcpy(dbg->nq, nq.data(), (size_t) n * 4);
            if (dbg->wh) memcpy(dbg->wh, wh.data(), (size_t) n * 8);
            if (dbg->qxy) memcpy(dbg->qxy, qxy.data(), qxy.size() * 4);
            if (dbg->qdesc) memcpy(dbg->qdesc, qdesc.data(), qdesc.size());
            if (dbg->H) memcpy(dbg->H, H.data(), H.size() * 8);
            if (dbg->mask) memcpy(dbg->mask, mask.data(), mask.size());
            if (dbg->R) memcpy(dbg->R, R.data(), R.size() * 8);
            if (dbg->t) memcpy(dbg->t, t.data(), t.size() * 8);
        }
        const Camera &cam = s->slam->cam;
        const double calib4[4] = {cam.fx, cam.fy, cam.cx, cam.cy};
        const bool tracked = s->last_status == 1;
        // the map points the frame observes, in camera coordinates (the placement's rays and depths)
        std::vector<double> pts_cam;
        SE3 Twc;
        if (tracked) {
            Twc = s->slam->cur->Twc;
            if (dbg && dbg->pose7) se3_to_pose7(Twc, dbg->pose7);
            std::vector<double> pts;
            frame_map_points(*s->slam, &pts, nullptr);
            const SE3 Tcw = se3_inverse(Twc);
            pts_cam.resize(pts.size());
            for (size_t i = 0; i + 2 < pts.size(); i += 3) se3_apply(Tcw, pts.data() + i, pts_cam.data() + i);
        }
        int found = 0;
        std::vector<double> ratios;
        for (int k = 0; k < n; k++) {
            int *info = h_info8 + 8 * k;
            if (info[0] != 0) continue;
            const alva_system::ImageTarget &T = s->images.list[(size_t) k];
            const double aspect = (double) T.h / (double) T.w;
            const double *Rk = R.data() + 9 * (size_t) k, *tk = t.data() + 3 * (size_t) k;
            if (!image_quad(Rk, tk, aspect, calib4, h_quads8 + 8 * k)) {   // a corner behind the camera: not a view of the whole picture
                info[0] = 4;
                memset(h_quads8 + 8 * k, 0, 8 * sizeof(float));
                continue;
            }
            if (!tracked) {
                info[0] = 6;
                continue;
            }
            image_scale_ratios(Rk, tk, aspect, pts_cam.data(), (int) (pts_cam.size() / 3), ratios);
            info[5] = (int) ratios.size();
            double width = 0;
            if (!image_width_from_ratios(ratios, &width)) {
                info[0] = 5;
                continue;
            }
            image_world_pose(Rk, tk, width, Twc, h_poses16 + 16 * k);
            h_extents2[2 * k] = (float) width;
            h_extents2[2 * k + 1] = (float) (width * aspect);
            h_scale1[k] = T.width_m > 0 ? (float) (T.width_m / width) : 0.f;
            found++;
        }
        return found;
    });
}

extern "C" int alva_system_detect_images(alva_system *s, int num_iterations, float threshold_px, int min_inliers, int cap, int *h_ids,
                                         float *h_poses16, float *h_extents2, float *h_scale1, float *h_quads8, int *h_info8) {
    return detect_images_impl(s, "alva_system_detect_images", num_iterations, threshold_px, min_inliers, cap, h_ids, h_poses16, h_extents2, h_scale1,
                              h_quads8, h_info8, nullptr);
}

extern "C" int alva_system_debug_detect_images(alva_system *s, int num_iterations, float threshold_px, int min_inliers, int cap, int *h_ids,
                                               float *h_poses16, float *h_extents2, float *h_scale1, float *h_quads8, int *h_info8,
                                               const alva_image_debug *dbg) {
    return detect_images_impl(s, "alva_system_debug_detect_images", num_iterations, threshold_px, min_inliers, cap, h_ids, h_poses16, h_extents2,
                              h_scale1, h_quads8, h_info8, dbg);
}

// X_to = R_to^T (R_from X_from + t_from - t_to): R row-major then t
static void depth_relative(const SE3 &from, const SE3 &to, double *T) {
    double Rc[9], Rr[9];
    quat_to_rot(from.q, Rc);
    quat_to_rot(to.q, Rr);
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) T[3 * i + j] = (Rr[i] * Rc[j] + Rr[3 + i] * Rc[3 + j]) + Rr[6 + i] * Rc[6 + j];
        T[9 + i] = (Rr[i] * (from.t[0] - to.t[0]) + Rr[3 + i] * (from.t[1] - to.t[1])) + Rr[6 + i] * (from.t[2] - to.t[2]);
    }
}

// What a depth call sweeps against, for alva_system_depth and alva_system_depth_dense alike: code 6 (not tracking), 7 (no reference frame;
// the range is known all the same) or 0 with the ring slot and T_rc
struct DepthPick {
    int code = 6, ref = -1;
    double T[12] = {0}, rho_min = 0, rho_max = 0;
};
static void depth_pick(alva_system *s, DepthPick &pk) {
    std::vector<double> z;
    if (s->last_status == 1) depth_frame_z(*s->slam, z);
    if (s->last_status != 1 || (int) z.size() < DEPTH_MIN_POINTS) return;   // initialising, reset, LOST, never called, or next to no map in view
    s->depth.sync(s->slam->map_generation);
    // the range: half the near end to twice the far end of the frame's own points
    const size_t n = z.size();
    pk.rho_max = 1.0 / (0.5 * z[(n - 1) * 5 / 100]);
    pk.rho_min = 1.0 / (2.0 * z[(n - 1) * 95 / 100]);
    // the newest entry with enough baseline that looks the same way
    const SE3 &cur = s->slam->cur->Twc;
    double Rc[9], Rr[9];
    quat_to_rot(cur.q, Rc);
    const double median = z[z.size() / 2];
    for (int i = 0; i < 4; i++) {
        const alva_system::Depth::Ref &e = s->depth.ring[i];
        if (e.seq == 0 || (pk.ref >= 0 && e.seq < s->depth.ring[pk.ref].seq)) continue;
        quat_to_rot(e.Twc.q, Rr);
        const double cosang = (Rc[2] * Rr[2] + Rc[5] * Rr[5]) + Rc[8] * Rr[8];
        if (depth_baseline(cur, e.Twc) >= DEPTH_MIN_BASELINE * median && cosang >= DEPTH_MIN_COS) pk.ref = i;
    }
    pk.code = pk.ref < 0 ? 7 : 0;
    if (pk.ref >= 0) depth_relative(cur, s->depth.ring[pk.ref].Twc, pk.T);
}

// What alva_system_depth, alva_system_depth_dense and alva_system_mesh_update refuse alike, in this order: a bad argument (args_ok: the
// call's own pointers and ranges; the sweep's ranges are SweepParams::ok), depth off, and -- with cap -- arrays too small for the grid.
// -> 0: the call goes on
static int sweep_call_refused(const alva_system *s, const char *what, bool args_ok, const SweepParams &p, const int *cap) {
    g_sys_err[0] = 0;
    if (!s || !s->slam || !args_ok || !p.ok()) return bad_argument(what);
    if (!s->depth_enabled) return switched_off(what, "depth", "alva_system_set_depth");
    const int gw = s->slam->cam.width / p.step, gh = s->slam->cam.height / p.step;
    if (cap && *cap < gw * gh) {
        snprintf(g_sys_err, sizeof(g_sys_err), "%s: the arrays hold %d grid pixels, %d x %d are needed", what, *cap, gw, gh);
        return ALVA_ERR_ARG;
    }
    return 0;
}

static int depth_impl(alva_system *s, const char *what, const SweepParams &p, float *h_depth, uint8_t *h_conf, uint8_t *h_code, int cap,
                      int *h_info8, uint8_t *h_images2, double *h_T_rc12, double *h_rho2) {
    if (const int rc = sweep_call_refused(s, what, h_depth && h_conf && h_code && h_info8, p, &cap)) return rc;
    const Camera &k = s->slam->cam;
    const int gw = k.width / p.step, gh = k.height / p.step;
    const size_t G = (size_t) gw * (size_t) gh;
    memset(h_info8, 0, 8 * sizeof(int));
    h_info8[6] = gw;
    h_info8[7] = gh;
    memset(h_depth, 0, G * sizeof(float));
    memset(h_conf, 0, G);
    return guarded(s, what, [&]() -> int {
        DepthPick pk;
        depth_pick(s, pk);
        if (pk.code) {
            memset(h_code, pk.code, G);
            return 0;
        }
        const int rc = s->scene->depth_sweep(pk.ref, camera_calib8(k).data(), pk.T, p, pk.rho_min, pk.rho_max, h_depth, h_conf, h_code, h_info8,
                                             h_images2);
        if (rc) return sys_fail(rc, what);
        if (h_T_rc12) memcpy(h_T_rc12, pk.T, sizeof(pk.T));
        if (h_rho2) {
            h_rho2[0] = pk.rho_min;
            h_rho2[1] = pk.rho_max;
        }
        return h_info8[0];
    });
}

extern "C" int alva_system_depth(alva_system *s, int step, int num_hyp, int patch_radius, int min_texture, int min_conf, float *h_depth,
                                 uint8_t *h_conf, uint8_t *h_code, int cap, int *h_info8) {
    return depth_impl(s, "alva_system_depth", {step, num_hyp, patch_radius, min_texture, min_conf}, h_depth, h_conf, h_code, cap, h_info8, nullptr,
                      nullptr, nullptr);
}

extern "C" int alva_system_debug_depth(alva_system *s, int step, int num_hyp, int patch_radius, int min_texture, int min_conf, float *h_depth,
                                       uint8_t *h_conf, uint8_t *h_code, int cap, int *h_info8, uint8_t *h_images2, double *h_T_rc12,
                                       double *h_rho2) {
    return depth_impl(s, "alva_system_debug_depth", {step, num_hyp, patch_radius, min_texture, min_conf}, h_depth, h_conf, h_code, cap, h_info8,
                      h_images2, h_T_rc12, h_rho2);
}

// ---- dense depth (alva_depth_fuse / alva_depth_fill in alvaar_hip.h define the stages; the fused state is kept in the scene stages) ----
constexpr int DEPTH_DENSE_DECAY = ALVA_DEPTH_DENSE_DECAY, DEPTH_DENSE_W_MAX = ALVA_DEPTH_DENSE_W_MAX;
constexpr double DEPTH_DENSE_REL_TOL = ALVA_DEPTH_DENSE_REL_TOL;

struct DepthDenseDebug {
    float *rho_before, *rho_after, *raw_depth;
    uint8_t *w_before, *raw_conf, *raw_code, *gray;
    double *pose7x2, *T_cp12, *rho_ref;
    int *flags4;
};

static int depth_dense_impl(alva_system *s, const char *what, const SweepParams &p, int max_level, float *h_depth, uint8_t *h_weight,
                            uint8_t *h_src, uint8_t *h_level, int cap, int *h_info16, const DepthDenseDebug *dbg) {
    const bool args_ok = h_depth && h_weight && h_src && h_level && h_info16 && max_level >= 1 && max_level <= 8;
    if (const int rc = sweep_call_refused(s, what, args_ok, p, &cap)) return rc;
    const Camera &k = s->slam->cam;
    const int step = p.step, gw = k.width / step, gh = k.height / step;
    const size_t G = (size_t) gw * (size_t) gh;
    memset(h_info16, 0, 16 * sizeof(int));
    h_info16[8] = gw;
    h_info16[9] = gh;
    memset(h_depth, 0, G * sizeof(float));
    memset(h_weight, 0, G);
    memset(h_src, 0, G);
    memset(h_level, 255, G);
    if (dbg && dbg->flags4) dbg->flags4[0] = -1, dbg->flags4[1] = dbg->flags4[2] = dbg->flags4[3] = 0;
    return guarded(s, what, [&]() -> int {
        DepthPick pk;
        depth_pick(s, pk);   // (a new map empties the ring and the state in here)
        h_info16[10] = pk.code;
        if (pk.code == 6) return 0;   // not tracking: nothing runs, the state is kept
        alva_system::Depth::Dense &D = s->depth.dense;
        if (D.valid && (D.gw != gw || D.gh != gh || D.step != step)) D.valid = false;
        if (pk.code == 7 && !D.valid) return 0;
        const int mode = !D.valid ? 1 : D.frame == s->slam->cur->id ? 0 : 2;
        const SE3 &cur = s->slam->cur->Twc;
        double T_cp[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
        if (mode == 2) depth_relative(D.Twc, cur, T_cp);
        const std::array<double, 8> calib8 = camera_calib8(k);
        SceneStages::DepthDense c{};
        c.mode = mode;
        c.slot = pk.code == 0 ? pk.ref : -1;
        c.calib8 = calib8.data(); c.T_rc12 = pk.T; c.T_cp12 = T_cp;
        c.sweep = p;
        c.max_level = max_level; c.decay = DEPTH_DENSE_DECAY; c.w_max = DEPTH_DENSE_W_MAX;
        c.rho_min = pk.rho_min; c.rho_max = pk.rho_max; c.rel_tol = DEPTH_DENSE_REL_TOL; c.rho_ref = 2.0 * pk.rho_max;
        c.depth = h_depth; c.weight = h_weight; c.src = h_src; c.level = h_level; c.info16 = h_info16;
        if (dbg) {
            c.dbg_rho_before = dbg->rho_before; c.dbg_w_before = dbg->w_before; c.dbg_rho_after = dbg->rho_after;
            c.dbg_raw_depth = dbg->raw_depth; c.dbg_raw_conf = dbg->raw_conf; c.dbg_raw_code = dbg->raw_code; c.dbg_gray = dbg->gray;
            if (dbg->pose7x2) {
                se3_to_pose7(mode == 1 ? cur : D.Twc, dbg->pose7x2);
                se3_to_pose7(cur, dbg->pose7x2 + 7);
            }
            if (dbg->T_cp12) memcpy(dbg->T_cp12, T_cp, sizeof(T_cp));
            if (dbg->rho_ref) *dbg->rho_ref = c.rho_ref;
        }
        const int rc = s->scene->depth_dense(c);
        if (rc < 0) {
            D.valid = false;
            return sys_fail(rc, what);
        }
        if (mode >= 1) {
            D.valid = true;
            D.gw = gw; D.gh = gh; D.step = step;
            D.Twc = cur;
            D.frame = s->slam->cur->id;
            for (int i = 0; i < 6; i++) D.counts[i] = h_info16[i];
            D.swept0 = h_info16[11];
            D.warped = mode == 2;
        } else {   // the stored state, as the call that fused it reported it
            for (int i = 0; i < 6; i++) h_info16[i] = D.counts[i];
            h_info16[11] = D.swept0;
        }
        h_info16[12] = D.warped;
        if (dbg && dbg->flags4) dbg->flags4[0] = mode, dbg->flags4[1] = c.slot >= 0 && mode >= 1;
        return rc;
    });
}

extern "C" int alva_system_depth_dense(alva_system *s, int step, int num_hyp, int patch_radius, int min_texture, int min_conf, int max_level,
                                       float *h_depth, uint8_t *h_weight, uint8_t *h_src, uint8_t *h_level, int cap, int *h_info16) {
    return depth_dense_impl(s, "alva_system_depth_dense", {step, num_hyp, patch_radius, min_texture, min_conf}, max_level, h_depth, h_weight, h_src,
                            h_level, cap, h_info16, nullptr);
}

extern "C" int alva_system_debug_depth_dense(alva_system *s, int step, int num_hyp, int patch_radius, int min_texture, int min_conf, int max_level,
                                             float *h_depth, uint8_t *h_weight, uint8_t *h_src, uint8_t *h_level, int cap, int *h_info16,
                                             float *h_rho_before, uint8_t *h_w_before, float *h_rho_after, float *h_raw_depth,
                                             uint8_t *h_raw_conf, uint8_t *h_raw_code, uint8_t *h_gray, double *h_pose7x2, double *h_T_cp12,
                                             double *h_rho_ref, int *h_flags4) {
    const DepthDenseDebug dbg{h_rho_before, h_rho_after, h_raw_depth, h_w_before, h_raw_conf, h_raw_code, h_gray, h_pose7x2, h_T_cp12, h_rho_ref,
                              h_flags4};
    return depth_dense_impl(s, "alva_system_debug_depth_dense", {step, num_hyp, patch_radius, min_texture, min_conf}, max_level, h_depth,
                            h_weight, h_src, h_level, cap, h_info16, &dbg);
}

extern "C" int alva_system_reset_depth_dense(alva_system *s) {
    g_sys_err[0] = 0;
    if (!s) return bad_argument("alva_system_reset_depth_dense", "bad argument");
    s->depth.dense.valid = false;
    return ALVA_OK;
}

// ---- scene mesh (alva_mesh_integrate / alva_mesh_extract in alvaar_hip.h define the stages; the volume is kept in the scene stages) ----
constexpr int MESH_W_MAX = ALVA_MESH_W_MAX;
constexpr double MESH_TRUNC_VOXELS = ALVA_MESH_TRUNC_VOXELS;

struct MeshDebug {
    float *raw_depth;
    uint8_t *raw_conf, *raw_code;
    double *T_cw12;
    int16_t *q;
    uint8_t *w;
};

static void mesh_geometry(const alva_system::Mesh &M, double *g5) {
    g5[0] = M.origin[0]; g5[1] = M.origin[1]; g5[2] = M.origin[2];
    g5[3] = M.voxel; g5[4] = M.trunc;
}

static bool mesh_follow_block_ok(int block) { return block == 1 || block == 2 || block == 4 || block == 8 || block == 16 || block == 32; }

// V2 - V4 of alvaar_system.h: the valid volume M moved so that its centre lies within a block of `centre`.  -> 1 shifted, 0 nothing to
// do (nothing is launched), or a negative error (the caller empties M: what the volume holds is no longer known).  shift3 = V3's s,
// info8 = the stage's (zeros, and N, where nothing ran)
static int mesh_follow_shift(alva_system *s, alva_system::Mesh &M, const double *centre, int block, int *shift3, int *info8) {
    memset(info8, 0, 8 * sizeof(int));
    info8[7] = M.N;
    bool any = false;
    for (int i = 0; i < 3; i++) {
        const double d = (centre[i] - (M.origin[i] + M.side / 2)) / M.voxel;   // V2
        double b = std::isfinite(d) ? std::trunc(d / (double) block) : 0.0;   // V3
        const double lim = (double) (ALVA_MESH_FOLLOW_MAX_SHIFT / block);
        b = b > lim ? lim : b < -lim ? -lim : b;
        shift3[i] = block * (int) b;
        any = any || shift3[i] != 0;
    }
    if (!any) return 0;
    const int rc = s->scene->mesh_shift(shift3, info8);   // V4
    if (rc < 0) return rc;
    for (int i = 0; i < 3; i++) M.offset[i] += shift3[i];
    M.shifts++;
    M.lost += info8[2];
    M.place_origin();
    return 1;
}

static int mesh_update_impl(alva_system *s, const char *what, int resolution, double rel_extent, const SweepParams &p, int *h_info16,
                            double *h_geometry5, const MeshDebug *dbg) {
    const bool args_ok = h_info16 && h_geometry5 && (resolution == 32 || resolution == 64 || resolution == 128 || resolution == 256) &&
                         std::isfinite(rel_extent) && rel_extent > 0;
    if (const int rc = sweep_call_refused(s, what, args_ok, p, nullptr)) return rc;
    memset(h_info16, 0, 16 * sizeof(int));
    memset(h_geometry5, 0, 5 * sizeof(double));
    return guarded(s, what, [&]() -> int {
        DepthPick pk;
        depth_pick(s, pk);   // (a new map empties the ring in here)
        alva_system::Mesh &M = s->mesh;
        M.sync(s->slam->map_generation);
        h_info16[0] = pk.code;
        h_info16[6] = M.valid ? M.N : 0;
        h_info16[8] = M.frames;
        if (M.valid) mesh_geometry(M, h_geometry5);
        if (pk.code) return 0;   // not tracking, or no reference frame: nothing runs, the volume is kept
        const bool place = !M.valid || M.N != resolution || M.rel_extent != rel_extent;
        const int frame = s->slam->cur->id;
        if (!place && M.frame == frame) {
            h_info16[0] = 8;
            return 0;
        }
        const SE3 &cur = s->slam->cur->Twc;
        double R[9];   // R_wc, row-major
        quat_to_rot(cur.q, R);
        int shifted = 0, shift3[3] = {0, 0, 0};
        if (!place && s->mesh_follow) {   // V1 - V4, before the frame is integrated: it lands in the shifted volume
            double target[3];
            for (int i = 0; i < 3; i++) target[i] = cur.t[i] + M.m0 * R[3 * i + 2];   // V1: the placement's expression, the placement's m0
            int shift8[8];
            shifted = mesh_follow_shift(s, M, target, s->mesh_follow, shift3, shift8);
            if (shifted < 0) {
                M.clear();
                return sys_fail(shifted, what);
            }
        }
        alva_system::Mesh P = M;
        if (place) {
            std::vector<double> z;
            depth_frame_z(*s->slam, z);   // (depth_pick has seen at least DEPTH_MIN_POINTS of them)
            const double m = z[z.size() / 2], side = rel_extent * m;
            P.N = resolution;
            P.rel_extent = rel_extent;
            P.voxel = side / (double) resolution;
            P.trunc = MESH_TRUNC_VOXELS * P.voxel;
            P.m0 = m;
            P.side = side;
            for (int i = 0; i < 3; i++) P.origin0[i] = (cur.t[i] + m * R[3 * i + 2]) - side / 2;   // the centre: m along the optical axis
            P.offset[0] = P.offset[1] = P.offset[2] = 0;
            P.shifts = P.lost = 0;
            P.volume++;   // (another volume: alva_system_mesh_blocks starts over)
            P.place_origin();   // (offset 0: origin0's bits)
            P.frames = 0;
        }
        double T_cw[12];
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) T_cw[3 * i + j] = R[3 * j + i];
            T_cw[9 + i] = -((R[i] * cur.t[0] + R[3 + i] * cur.t[1]) + R[6 + i] * cur.t[2]);
        }
        const Camera &k = s->slam->cam;
        const std::array<double, 8> calib8 = camera_calib8(k);
        int info8[8] = {0, 0, 0, 0, 0, 0, 0, 0}, swept0 = 0;
        SceneStages::MeshUpdate c{};
        c.slot = pk.ref; c.N = P.N; c.zero = place;
        c.calib8 = calib8.data(); c.T_rc12 = pk.T; c.origin3 = P.origin; c.T_cw12 = T_cw;
        c.voxel = P.voxel; c.trunc = P.trunc; c.rho_min = pk.rho_min; c.rho_max = pk.rho_max;
        c.sweep = p;
        c.w_max = MESH_W_MAX;
        c.color_on = s->mesh_color_enabled;
        c.color_fuse = c.color_on && s->mesh_color.thumb_frame == frame;   // (a stale or missing thumbnail: geometry only)
        c.cstep = MESH_COLOR_STEP;
        c.info8 = info8; c.swept0 = &swept0;
        if (dbg) {
            c.dbg_raw_depth = dbg->raw_depth; c.dbg_raw_conf = dbg->raw_conf; c.dbg_raw_code = dbg->raw_code;
            c.dbg_q = dbg->q; c.dbg_w = dbg->w;
            if (dbg->T_cw12) memcpy(dbg->T_cw12, T_cw, sizeof(T_cw));
        }
        const int rc = s->scene->mesh_update(c);
        if (rc < 0) {
            M.clear();   // (what the volume holds is no longer known)
            return sys_fail(rc, what);
        }
        M = P;
        M.valid = true;
        M.frame = frame;
        M.frames++;
        for (int i = 0; i < 5; i++) h_info16[1 + i] = info8[i];
        h_info16[6] = M.N;
        h_info16[7] = swept0;
        h_info16[8] = M.frames;
        h_info16[9] = place ? 1 : 0;
        h_info16[10] = info8[6];
        h_info16[11] = c.color_fuse ? 1 : 0;
        h_info16[12] = shifted;
        for (int i = 0; i < 3; i++) h_info16[13 + i] = shift3[i];
        mesh_geometry(M, h_geometry5);
        return info8[0];
    });
}

extern "C" int alva_system_mesh_update(alva_system *s, int resolution, double rel_extent, int step, int num_hyp, int patch_radius,
                                       int min_texture, int min_conf, int *h_info16, double *h_geometry5) {
    return mesh_update_impl(s, "alva_system_mesh_update", resolution, rel_extent, {step, num_hyp, patch_radius, min_texture, min_conf}, h_info16,
                            h_geometry5, nullptr);
}

extern "C" int alva_system_debug_mesh_update(alva_system *s, int resolution, double rel_extent, int step, int num_hyp, int patch_radius,
                                             int min_texture, int min_conf, int *h_info16, double *h_geometry5, float *h_raw_depth,
                                             uint8_t *h_raw_conf, uint8_t *h_raw_code, double *h_T_cw12, int16_t *h_q, uint8_t *h_w) {
    const MeshDebug dbg{h_raw_depth, h_raw_conf, h_raw_code, h_T_cw12, h_q, h_w};
    return mesh_update_impl(s, "alva_system_debug_mesh_update", resolution, rel_extent, {step, num_hyp, patch_radius, min_texture, min_conf},
                            h_info16, h_geometry5, &dbg);
}

// alva_system_mesh (h_colors null) and alva_system_mesh_colored
static int mesh_impl(alva_system *s, const char *what, int min_weight, int max_vertices, int max_triangles, float *h_vertices, float *h_normals,
                     uint8_t *h_colors, bool colored, int *h_triangles, int *h_info8, double *h_geometry5) {
    g_sys_err[0] = 0;
    if (!s || !s->slam || !h_vertices || !h_normals || !h_triangles || !h_info8 || !h_geometry5 || min_weight < 1 || min_weight > 255 ||
        max_vertices < 1 || max_triangles < 1 || (colored && !h_colors)) return bad_argument(what);
    if (colored && !s->mesh_color_enabled) return switched_off(what, "mesh colour", "alva_system_set_mesh_color");
    memset(h_info8, 0, 8 * sizeof(int));
    memset(h_geometry5, 0, 5 * sizeof(double));
    return guarded(s, what, [&]() -> int {
        alva_system::Mesh &M = s->mesh;
        M.sync(s->slam->map_generation);
        if (!M.valid) {   // (the volume is in world coordinates: whether the tracker tracks right now does not matter)
            h_info8[0] = 5;
            return 0;
        }
        mesh_geometry(M, h_geometry5);
        int n_colored = 0;
        const int rc = s->scene->mesh_extract(M.origin, M.voxel, min_weight, max_vertices, max_triangles, h_vertices, h_normals, h_triangles,
                                              h_info8, h_colors, &n_colored);
        if (rc < 0) return sys_fail(rc, what);
        if (colored) h_info8[6] = n_colored;
        return h_info8[0] == 0 ? h_info8[2] : 0;
    });
}

extern "C" int alva_system_mesh(alva_system *s, int min_weight, int max_vertices, int max_triangles, float *h_vertices, float *h_normals,
                                int *h_triangles, int *h_info8, double *h_geometry5) {
    return mesh_impl(s, "alva_system_mesh", min_weight, max_vertices, max_triangles, h_vertices, h_normals, nullptr, false, h_triangles, h_info8,
                     h_geometry5);
}

extern "C" int alva_system_mesh_colored(alva_system *s, int min_weight, int max_vertices, int max_triangles, float *h_vertices, float *h_normals,
                                        uint8_t *h_colors, int *h_triangles, int *h_info8, double *h_geometry5) {
    return mesh_impl(s, "alva_system_mesh_colored", min_weight, max_vertices, max_triangles, h_vertices, h_normals, h_colors, true, h_triangles,
                     h_info8, h_geometry5);
}

extern "C" int alva_system_mesh_color_at(alva_system *s, int n, const float *h_points3, uint8_t *h_rgba, uint8_t *h_codes, int *h_info8) {
    const char *what = "alva_system_mesh_color_at";
    g_sys_err[0] = 0;
    if (!s || !s->slam || !h_points3 || !h_rgba || !h_codes || !h_info8 || n < 1 || n > (1 << 20)) return bad_argument(what);
    if (!s->mesh_color_enabled) return switched_off(what, "mesh colour", "alva_system_set_mesh_color");
    memset(h_info8, 0, 8 * sizeof(int));
    h_info8[0] = n;
    memset(h_rgba, 0, (size_t) n * 4);
    return guarded(s, what, [&]() -> int {
        alva_system::Mesh &M = s->mesh;
        M.sync(s->slam->map_generation);
        if (!M.valid || !s->scene->has_mesh_color()) {   // (world coordinates: it answers whether or not the tracker tracks, as alva_system_mesh)
            memset(h_codes, 5, (size_t) n);
            return 0;
        }
        const int rc = s->scene->mesh_color_at(M.origin, M.voxel, n, h_points3, h_rgba, h_codes, h_info8);
        if (rc < 0) return sys_fail(rc, what);
        return h_info8[1];
    });
}

extern "C" int alva_system_debug_mesh_color(alva_system *s, uint8_t *h_thumb, uint8_t *h_c) {
    const char *what = "alva_system_debug_mesh_color";
    g_sys_err[0] = 0;
    if (!s || !s->slam || !s->scene) return bad_argument(what);
    if (!s->mesh_color_enabled) return switched_off(what, "mesh colour", "alva_system_set_mesh_color");
    return guarded(s, what, [&]() -> int {
        alva_system::Mesh &M = s->mesh;
        M.sync(s->slam->map_generation);
        const Camera &k = s->slam->cam;
        if (h_thumb) memset(h_thumb, 0, (size_t) (k.width / MESH_COLOR_STEP) * (size_t) (k.height / MESH_COLOR_STEP) * 4);
        const bool volume = M.valid && s->scene->has_mesh_color();
        if (h_c && M.valid && !volume) memset(h_c, 0, 4 * (size_t) M.N * M.N * M.N);
        const bool thumb = s->mesh_color.thumb_frame >= 0;
        const int rc = s->scene->mesh_color_debug(thumb ? h_thumb : nullptr, volume ? h_c : nullptr);
        if (rc < 0) return sys_fail(rc, what);
        return (thumb && s->mesh_color.thumb_frame == s->slam->cur->id ? 1 : 0) | (volume ? 2 : 0);
    });
}

extern "C" int alva_system_reset_mesh(alva_system *s) {
    g_sys_err[0] = 0;
    if (!s) return bad_argument("alva_system_reset_mesh", "bad argument");
    s->mesh.clear();
    return ALVA_OK;
}

// ---- following the camera (alva_mesh_shift in alvaar_hip.h defines the stage, V1 - V4 in alvaar_system.h the rule) ----
extern "C" int alva_system_set_mesh_follow(alva_system *s, int block) {
    g_sys_err[0] = 0;
    if (!s || (block != 0 && !mesh_follow_block_ok(block))) {
        snprintf(g_sys_err, sizeof(g_sys_err), "alva_system_set_mesh_follow: bad argument (block 0, 1, 2, 4, 8, 16 or 32)");
        return ALVA_ERR_ARG;
    }
    s->mesh_follow = block;   // (the volume is not touched: where it lies now is where the next update finds it)
    return ALVA_OK;
}

extern "C" int alva_system_mesh_move(alva_system *s, const double *h_centre3, int block, int *h_info8, double *h_geometry5) {
    const char *what = "alva_system_mesh_move";
    g_sys_err[0] = 0;
    if (!s || !s->slam || !h_centre3 || !h_info8 || !h_geometry5 || !mesh_follow_block_ok(block)) return bad_argument(what);
    memset(h_info8, 0, 8 * sizeof(int));
    memset(h_geometry5, 0, 5 * sizeof(double));
    return guarded(s, what, [&]() -> int {
        alva_system::Mesh &M = s->mesh;
        M.sync(s->slam->map_generation);
        if (!M.valid) {   // (world coordinates: it answers whether or not the tracker tracks, as alva_system_mesh)
            h_info8[4] = 5;
            return 0;
        }
        int shift3[3];
        const int moved = mesh_follow_shift(s, M, h_centre3, block, shift3, h_info8);
        if (moved < 0) {
            M.clear();
            return sys_fail(moved, what);
        }
        mesh_geometry(M, h_geometry5);
        return moved;
    });
}

extern "C" int alva_system_mesh_follow_stats(alva_system *s, long *h_stats8) {
    g_sys_err[0] = 0;
    if (!s || !h_stats8) return bad_argument("alva_system_mesh_follow_stats", "bad argument");
    alva_system::Mesh &M = s->mesh;
    if (s->slam) M.sync(s->slam->map_generation);
    h_stats8[0] = s->mesh_follow;
    h_stats8[1] = (long) M.shifts;
    for (int i = 0; i < 3; i++) h_stats8[2 + i] = (long) M.offset[i];
    h_stats8[5] = (long) M.lost;
    h_stats8[6] = h_stats8[7] = 0;
    return ALVA_OK;
}

// ---- the mesh in blocks (alva_mesh_block_digest / alva_mesh_extract_blocks in alvaar_hip.h define the stages, G1 - G6 in alvaar_system.h
// the rule; the list is csrc/slam/mesh_blocks.hpp) ----
extern "C" int alva_system_mesh_blocks(alva_system *s, int min_weight, int block, int flags, int max_blocks, int max_vertices, int max_triangles,
                                       int *h_keys, int *h_block_info, float *h_vertices, float *h_normals, uint8_t *h_colors, int *h_triangles,
                                       int *h_lattice3, int *h_info8, double *h_geometry5) {
    const char *what = "alva_system_mesh_blocks";
    g_sys_err[0] = 0;
    if (!s || !s->slam || !h_keys || !h_block_info || !h_vertices || !h_normals || !h_triangles || !h_lattice3 || !h_info8 || !h_geometry5 ||
        min_weight < 1 || min_weight > 255 || (block != 8 && block != 16 && block != 32) || (flags & ~ALVA_MESH_BLOCKS_ALL) || max_blocks < 1 ||
        max_vertices < 1 || max_triangles < 1) return bad_argument(what);
    if (h_colors && !s->mesh_color_enabled) return switched_off(what, "mesh colour", "alva_system_set_mesh_color");
    memset(h_info8, 0, 8 * sizeof(int));
    memset(h_lattice3, 0, 3 * sizeof(int));
    memset(h_geometry5, 0, 5 * sizeof(double));
    return guarded(s, what, [&]() -> int {
        alva_system::Mesh &M = s->mesh;
        M.sync(s->slam->map_generation);
        if (!M.valid) {   // G1 (world coordinates: it answers whether or not the tracker tracks, as alva_system_mesh)
            h_info8[0] = 5;
            return 0;
        }
        mesh_geometry(M, h_geometry5);
        for (int i = 0; i < 3; i++) {
            if (M.offset[i] < -(1 << 30) || M.offset[i] > (1 << 30)) return sys_fail(ALVA_ERR_STATE, what);   // (L1's range)
            h_lattice3[i] = (int) M.offset[i];
        }
        alva_slam::MeshBlockList &L = s->mesh_blocks;
        L.begin(M.volume, min_weight, block);   // G2
        std::vector<uint64_t> digest;
        std::vector<int> counts;
        int nb3[3];
        int rc = s->scene->mesh_block_digest(h_lattice3, min_weight, block, digest, counts, nb3);   // G3
        if (rc < 0) return sys_fail(rc, what);
        alva_slam::MeshBlockList::Plan P;
        L.plan(h_lattice3, M.N, digest.data(), counts.data(), (flags & ALVA_MESH_BLOCKS_ALL) != 0, max_blocks, max_vertices, max_triangles, P);   // G4
        h_info8[0] = P.code;
        h_info8[1] = (int) P.reports.size();
        h_info8[2] = P.vertices;
        h_info8[3] = P.triangles;
        h_info8[4] = P.gone;
        h_info8[5] = L.epoch;
        h_info8[6] = P.present;
        h_info8[7] = block;
        if (P.code == 3) return 0;   // G5: nothing written, the table untouched
        std::vector<int> ranges(4 * P.reports.size() + 4, 0);
        if (P.n_extract > 0) {   // G6
            std::vector<int> keys(3 * (size_t) P.n_extract);
            for (int b = 0; b < P.n_extract; b++) memcpy(&keys[3 * (size_t) b], P.reports[(size_t) b].key, 3 * sizeof(int));
            int xinfo[8];
            rc = s->scene->mesh_extract_blocks(M.origin, M.voxel, h_lattice3, min_weight, block, P.n_extract, keys.data(), P.vertices, P.triangles,
                                               h_vertices, h_normals, h_colors, h_triangles, ranges.data(), xinfo);
            if (rc < 0) return sys_fail(rc, what);
            if (xinfo[0] != 0 || xinfo[1] != P.vertices || xinfo[2] != P.triangles) return sys_fail(ALVA_ERR_STATE, what);   // (the two stages count alike)
        }
        for (size_t b = 0; b < P.reports.size(); b++) {
            const alva_slam::MeshBlockList::Report &r = P.reports[b];
            memcpy(h_keys + 3 * b, r.key, 3 * sizeof(int));
            int *o = h_block_info + 8 * b;
            o[0] = r.state;
            memcpy(o + 1, &ranges[4 * b], 4 * sizeof(int));   // (zeros for the blocks that are gone)
            o[5] = (int) (uint32_t) r.digest;
            o[6] = (int) (uint32_t) (r.digest >> 32);
            o[7] = 0;
        }
        L.commit(h_lattice3, M.N, digest.data(), counts.data());
        return (int) P.reports.size();
    });
}

extern "C" int alva_system_reset_mesh_blocks(alva_system *s) {
    g_sys_err[0] = 0;
    if (!s) return bad_argument("alva_system_reset_mesh_blocks", "bad argument");
    s->mesh_blocks.reset();
    return ALVA_OK;
}

// ---- raycasting the scene volume (alva_mesh_raycast / alva_mesh_raycast_pixels in alvaar_hip.h define the stages): three ways to ask the
// kept volume, none of which changes anything in the session ----
struct MeshRayCall {
    int n;                     // rays, taps or the arrays' capacity
    const double *rays6;       // world rays, or
    const double *T_wc12;      // an explicit pose (null: the current frame's, and code 6 when there is none), with
    const float *uv;           // taps (null: the grid of `step`)
    int step, min_weight;
    bool pixels;
    double t_near, t_far;
    float *t, *points, *normals;
    uint8_t *codes;
    float *poses;
    uint8_t *pose_ok;
    int *info8;
};

// -> the count of code 0, or a negative error; the whole-call codes 5 (no volume) and 6 (no pose) go to every ray's code
static int mesh_ray_impl(alva_system *s, const char *what, const MeshRayCall &c) {
    const Camera &k = s->slam->cam;
    const bool grid = c.pixels && !c.uv;
    const size_t n = grid ? (size_t) (k.width / c.step) * (size_t) (k.height / c.step) : (size_t) c.n;
    if (grid && (size_t) c.n < n) {
        snprintf(g_sys_err, sizeof(g_sys_err), "%s: the arrays hold %d grid pixels, %d x %d are needed", what, c.n, k.width / c.step, k.height / c.step);
        return ALVA_ERR_ARG;
    }
    memset(c.info8, 0, 8 * sizeof(int));
    c.info8[0] = (int) n;
    if (c.t) memset(c.t, 0, n * sizeof(float));
    if (c.points) memset(c.points, 0, n * 3 * sizeof(float));
    if (c.normals) memset(c.normals, 0, n * 3 * sizeof(float));
    if (c.poses) memset(c.poses, 0, n * 16 * sizeof(float));
    if (c.pose_ok) memset(c.pose_ok, 0, n);
    return guarded(s, what, [&]() -> int {
        alva_system::Mesh &M = s->mesh;
        M.sync(s->slam->map_generation);
        const int whole = !M.valid ? 5 : c.pixels && !c.T_wc12 && s->last_status != 1 ? 6 : 0;
        if (whole) {   // (the volume is in world coordinates: only a call that needs the current pose needs the tracker to track)
            memset(c.codes, whole, n);
            return 0;
        }
        double T[12];
        if (c.pixels && !c.T_wc12) {
            const SE3 &cur = s->slam->cur->Twc;
            quat_to_rot(cur.q, T);   // R_wc, row-major
            memcpy(T + 9, cur.t, 3 * sizeof(double));
        }
        const std::array<double, 8> calib8 = camera_calib8(k);
        SceneStages::MeshRaycast r{};
        r.origin3 = M.origin; r.voxel = M.voxel; r.min_weight = c.min_weight; r.n = (int) n;
        r.rays6 = c.rays6;
        r.T_wc12 = !c.pixels ? nullptr : c.T_wc12 ? c.T_wc12 : T;
        r.calib8 = calib8.data(); r.width = k.width; r.height = k.height; r.step = c.step; r.uv = c.uv;
        r.t_near = c.t_near; r.t_far = c.t_far;
        r.t = c.t; r.points = c.points; r.normals = c.normals; r.codes = c.codes; r.poses = c.poses; r.pose_ok = c.pose_ok; r.info8 = c.info8;
        const int rc = s->scene->mesh_raycast(r);
        if (rc < 0) return sys_fail(rc, what);
        return c.info8[1];
    });
}

extern "C" int alva_system_mesh_raycast(alva_system *s, int n, const double *h_rays6, int min_weight, double t_near, double t_far, float *h_t,
                                        float *h_points, float *h_normals, uint8_t *h_codes, int *h_info8) {
    g_sys_err[0] = 0;
    if (!s || !s->slam || !h_rays6 || !h_t || !h_points || !h_normals || !h_codes || !h_info8 || n < 1 || n > (1 << 20) || min_weight < 1 ||
        min_weight > 255 || !std::isfinite(t_near) || std::isnan(t_far) || !(t_near <= t_far)) return bad_argument("alva_system_mesh_raycast");
    MeshRayCall c{};
    c.n = n; c.rays6 = h_rays6; c.step = 1; c.min_weight = min_weight; c.pixels = false; c.t_near = t_near; c.t_far = t_far;
    c.t = h_t; c.points = h_points; c.normals = h_normals; c.codes = h_codes; c.info8 = h_info8;
    return mesh_ray_impl(s, "alva_system_mesh_raycast", c);
}

extern "C" int alva_system_mesh_depth(alva_system *s, const double *h_T_wc12, int step, int min_weight, float *h_depth, float *h_normals,
                                      uint8_t *h_codes, int cap, int *h_info8) {
    g_sys_err[0] = 0;
    bool ok = s && s->slam && h_depth && h_normals && h_codes && h_info8 && step >= 1 && step <= 16 && min_weight >= 1 && min_weight <= 255 && cap >= 1;
    for (int i = 0; ok && h_T_wc12 && i < 12; i++) ok = std::isfinite(h_T_wc12[i]);
    if (!ok) return bad_argument("alva_system_mesh_depth");
    MeshRayCall c{};
    c.n = cap; c.T_wc12 = h_T_wc12; c.step = step; c.min_weight = min_weight; c.pixels = true; c.t_near = 0.0; c.t_far = INFINITY;
    c.t = h_depth; c.normals = h_normals; c.codes = h_codes; c.info8 = h_info8;
    return mesh_ray_impl(s, "alva_system_mesh_depth", c);
}

extern "C" int alva_system_mesh_hit_test(alva_system *s, int n_taps, const float *h_uv, int min_weight, float *h_poses16, int *h_info8) {
    g_sys_err[0] = 0;
    if (!s || !s->slam || !h_uv || !h_poses16 || !h_info8 || n_taps < 1 || n_taps > 16 || min_weight < 1 || min_weight > 255)
        return bad_argument("alva_system_mesh_hit_test");
    uint8_t codes[16], pose_ok[16];
    int info8[8];
    MeshRayCall c{};
    c.n = n_taps; c.uv = h_uv; c.step = 1; c.min_weight = min_weight; c.pixels = true; c.t_near = 0.0; c.t_far = INFINITY;
    c.codes = codes; c.poses = h_poses16; c.pose_ok = pose_ok; c.info8 = info8;
    const int rc = mesh_ray_impl(s, "alva_system_mesh_hit_test", c);
    if (rc < 0) return rc;
    int found = 0;
    memset(h_info8, 0, (size_t) n_taps * 8 * sizeof(int));
    for (int r = 0; r < n_taps; r++) {
        h_info8[8 * r] = codes[r];
        h_info8[8 * r + 1] = pose_ok[r];
        h_info8[8 * r + 2] = info8[6];
        h_info8[8 * r + 3] = info8[7];
        found += pose_ok[r];
    }
    return found;
}

extern "C" int alva_system_debug_depth_ring(alva_system *s, double *h_pose7x4) {
    if (!s || !s->slam) return 0;
    s->depth.sync(s->slam->map_generation);
    int order[4], n = 0;
    for (int i = 0; i < 4; i++)
        if (s->depth.ring[i].seq > 0) order[n++] = i;
    std::sort(order, order + n, [&](int a, int b) { return s->depth.ring[a].seq > s->depth.ring[b].seq; });
    for (int i = 0; i < n && h_pose7x4; i++) se3_to_pose7(s->depth.ring[order[i]].Twc, h_pose7x4 + 7 * i);
    return n;
}

constexpr int N_CAP = 16384;   // the stages' bound on the points of one call

// Every 3-D point of the map in ascending id; of a map past the stages' bound, the newest (the highest ids).  The candidates of plane
// detection, plane tracking and the anchors' supports
static void map_points_by_id(const Slam &S, std::vector<int> &ids, std::vector<double> &pts) {
    for (const auto &e: S.map_points)
        if (e.second->r->is3d) ids.push_back(e.first);
    std::sort(ids.begin(), ids.end());
    if (ids.size() > (size_t) N_CAP) ids.erase(ids.begin(), ids.end() - N_CAP);
    const int n = (int) ids.size();
    pts.resize((size_t) n * 3);
    for (int i = 0; i < n; i++) memcpy(&pts[3 * (size_t) i], S.map_points.at(ids[i])->r->X, 24);
}

// What alva_system_detect_planes and alva_system_detect_plane_outlines hand to the stage: the pose, the slab's half thickness and every
// 3-D point of the map.  false: a frame that tracks but gives no scale (the caller answers as the stage does for n = 0)
static bool plane_detection_input(alva_system *s, double rel_thickness, double (&pose7)[7], double &thickness, std::vector<int> &ids,
                                  std::vector<double> &pts) {
    double R[9];
    se3_to_pose7(s->slam->cur->Twc, pose7);
    quat_to_rot(pose7 + 3, R);
    // D: the camera-frame depth of rank n / 2 among the frame's observed 3-D points -- the scale of a monocular map is arbitrary
    std::vector<double> seen, depth;
    frame_map_points(*s->slam, &seen, nullptr);
    for (size_t i = 0; i < seen.size(); i += 3) {
        const double d0 = seen[i] - pose7[0], d1 = seen[i + 1] - pose7[1], d2 = seen[i + 2] - pose7[2];
        depth.push_back((R[2] * d0 + R[5] * d1) + R[8] * d2);   // the z of R_wc^T (P - t)
    }
    if (depth.empty()) return false;   // tracking, but nothing triangulated is in view yet: no scale to size the slab by
    std::nth_element(depth.begin(), depth.begin() + depth.size() / 2, depth.end());
    thickness = rel_thickness * depth[depth.size() / 2];
    if (!(thickness > 0)) return false;
    map_points_by_id(*s->slam, ids, pts);
    return true;
}

// What the three plane entry points have in common: the arguments (max_vertices = 0: no outlines), their check, the outputs of a call
// that has not run yet, the stage call and the count of planes
struct PlaneRequest {
    double rel_thickness;
    int min_inliers, max_planes, num_iterations;
    float *planes24;
    int *info8, *point_ids, *labels;
    int cap, max_vertices;
    float *outline;
    int *outline_info8;
    double *area;

    bool ok(const alva_system *s) const {
        return s && s->slam && planes24 && info8 && rel_thickness > 0 && std::isfinite(rel_thickness) && min_inliers >= 8 && min_inliers <= N_CAP &&
               max_planes >= 1 && max_planes <= 8 && num_iterations >= 1 && num_iterations <= 4096 && cap >= 0 &&
               !((point_ids || labels) && cap < N_CAP) &&
               !(max_vertices && (max_vertices < 8 || max_vertices > 1024 || !outline || !outline_info8 || !area));
    }
    void clear() const {
        memset(planes24, 0, (size_t) max_planes * 24 * sizeof(float));
        memset(info8, 0, (size_t) max_planes * 8 * sizeof(int));
        if (max_vertices) {
            memset(outline, 0, (size_t) max_planes * max_vertices * 2 * sizeof(float));
            memset(outline_info8, 0, (size_t) max_planes * 8 * sizeof(int));
            memset(area, 0, (size_t) max_planes * sizeof(double));
        }
        if (point_ids) std::fill_n(point_ids, cap, -1);   // the lists end with -1s
        if (labels) std::fill_n(labels, cap, -1);
    }
    void all_rounds(int code, int outline_code) const {
        for (int r = 0; r < max_planes; r++) {
            info8[8 * r] = code;
            info8[8 * r + 2] = -1;
            if (max_vertices) outline_info8[8 * r] = outline_code;
        }
    }
    // the stage on the candidates ids / pts, the n_prior records prior24 in front; the planes found, or the session's error code
    int run(alva_system *s, const char *what, const double *pose7, double thickness, const std::vector<int> &ids, const std::vector<double> &pts,
            int n_prior, const float *prior24) const {
        const int n = (int) ids.size();
        const SceneStages::PlaneCall c{n, pts.data(), pose7, thickness, min_inliers, max_planes, num_iterations, 12345u, n_prior, prior24, planes24, info8,
                                  labels, max_vertices, outline, outline_info8, area};
        const int rc = s->scene->planes(c);
        if (rc) return sys_fail(rc, what);
        if (point_ids) memcpy(point_ids, ids.data(), (size_t) n * sizeof(int));
        int found = 0;
        for (int r = 0; r < max_planes; r++) found += info8[8 * r] == 0;
        return found;
    }
};

// alva_system_detect_planes and alva_system_detect_plane_outlines
static int system_detect_planes(alva_system *s, const char *what, const PlaneRequest &q) {
    g_sys_err[0] = 0;
    if (!q.ok(s)) return bad_argument(what);
    q.clear();
    if (s->last_status != 1) {   // initialising, reset, LOST or never called: no pose to orient the planes by, no depth to scale the slab by
        q.all_rounds(6, 6);
        return 0;
    }
    return guarded(s, what, [&]() -> int {
        double pose7[7], thickness = 0;
        std::vector<int> ids;
        std::vector<double> pts;
        if (!plane_detection_input(s, q.rel_thickness, pose7, thickness, ids, pts)) {
            q.all_rounds(5, 5);   // what the stages say of n = 0: round 0 has too few points, the others do not run; no plane has a record
            q.info8[0] = 1;
            return 0;
        }
        return q.run(s, what, pose7, thickness, ids, pts, 0, nullptr);
    });
}

extern "C" int alva_system_detect_planes(alva_system *s, double rel_thickness, int min_inliers, int max_planes, int num_iterations,
                                         float *h_planes24, int *h_info8, int *h_point_ids, int *h_labels, int cap) {
    return system_detect_planes(s, "alva_system_detect_planes", {rel_thickness, min_inliers, max_planes, num_iterations, h_planes24, h_info8,
                                                                 h_point_ids, h_labels, cap, 0, nullptr, nullptr, nullptr});
}

extern "C" int alva_system_detect_plane_outlines(alva_system *s, double rel_thickness, int min_inliers, int max_planes, int num_iterations,
                                                 float *h_planes24, int *h_info8, int *h_point_ids, int *h_labels, int cap, int max_vertices,
                                                 float *h_outline, int *h_outline_info8, double *h_area) {
    if (max_vertices == 0) max_vertices = -1;   // 0 means "no outlines" to the common body only: here it is a bad argument
    return system_detect_planes(s, "alva_system_detect_plane_outlines", {rel_thickness, min_inliers, max_planes, num_iterations, h_planes24, h_info8,
                                                                         h_point_ids, h_labels, cap, max_vertices, h_outline, h_outline_info8, h_area});
}

extern "C" int alva_system_track_planes(alva_system *s, double rel_thickness, int min_inliers, int max_planes, int num_iterations,
                                        float *h_planes24, int *h_info8, int *h_plane_ids, int *h_merged_into, int *h_point_ids,
                                        int *h_labels, int cap, int max_vertices, float *h_outline, int *h_outline_info8, double *h_area) {
    const char *what = "alva_system_track_planes";
    const PlaneRequest q{rel_thickness, min_inliers, max_planes, num_iterations, h_planes24, h_info8, h_point_ids, h_labels, cap, max_vertices,
                         h_outline, h_outline_info8, h_area};
    g_sys_err[0] = 0;
    if (!q.ok(s) || !h_plane_ids || !h_merged_into) return bad_argument(what);
    s->plane_tracks.sync(s->slam->map_generation);   // the planes of a map that was thrown away are gone with it
    if (max_planes < s->plane_tracks.n) {
        snprintf(g_sys_err, sizeof(g_sys_err), "%s: max_planes %d is below the %d planes tracked", what, max_planes, s->plane_tracks.n);
        return ALVA_ERR_ARG;
    }
    q.clear();
    auto nothing_runs = [&]() {   // code 6 in every slot, no ids; the list stays as it is
        q.all_rounds(6, 6);
        for (int r = 0; r < max_planes; r++) h_plane_ids[r] = h_merged_into[r] = -1;
        return 0;
    };
    if (s->last_status != 1) return nothing_runs();   // initialising, reset, LOST or never called: the planes wait for the pose to come back
    return guarded(s, what, [&]() -> int {
        double pose7[7], thickness = 0;
        std::vector<int> ids;
        std::vector<double> pts;
        if (!plane_detection_input(s, rel_thickness, pose7, thickness, ids, pts)) return nothing_runs();   // no scale: as if not tracking
        float prior24[PlaneTracks::MAX_TRACKS * 24];
        const int n_prior = s->plane_tracks.priors(prior24);
        const int found = q.run(s, what, pose7, thickness, ids, pts, n_prior, prior24);
        if (found >= 0) s->plane_tracks.apply(h_planes24, h_info8, n_prior, max_planes, thickness, h_plane_ids, h_merged_into);
        return found;
    });
}

extern "C" void alva_system_reset_planes(alva_system *s) {
    if (s) s->plane_tracks.clear();
}

// ---- anchors (slam/anchors.hpp keeps the list; alva_anchor_attach and alva_anchor_update in alvaar_hip.h define the stages)
// the supports of the anchors `which` (places in the list, at most 16) among the candidates ids / pts, at the poses pose16[k]
static int attach_anchors(alva_system *s, const std::vector<int> &which, const float *pose16, const std::vector<int> &ids,
                          const std::vector<double> &pts) {
    const int n = (int) ids.size(), na = (int) which.size();
    double pos3[16 * 3];
    for (int k = 0; k < na; k++)
        for (int c = 0; c < 3; c++) pos3[3 * k + c] = (double) pose16[16 * k + 12 + c];
    const int K = Anchor::MAX_SUPPORT;
    std::vector<int> index((size_t) na * K), count((size_t) na);
    std::vector<double> dist2((size_t) na * K);
    // one call for all of them: the stage's rows have the stride of ITS max_support, and anchors may differ in theirs -- the K nearest
    // under a total order are the first K of the 64 nearest, so every anchor takes the front of a 64-row
    const int rc = s->scene->anchor_attach(n, pts.data(), na, pos3, K, index.data(), dist2.data(), count.data());
    if (rc) return rc;
    for (int k = 0; k < na; k++) {
        const int want = s->anchors.list[which[k]].max_support, m = count[k] < want ? count[k] : want;
        int sup_id[Anchor::MAX_SUPPORT];
        double sup_xyz[Anchor::MAX_SUPPORT][3];
        for (int j = 0; j < m; j++) {
            const int i = index[(size_t) k * K + j];
            sup_id[j] = ids[(size_t) i];
            memcpy(sup_xyz[j], &pts[3 * (size_t) i], 24);
        }
        s->anchors.attach(which[k], pose16 + 16 * k, m, sup_id, &sup_xyz[0][0]);
    }
    return ALVA_OK;
}

extern "C" int alva_system_create_anchors(alva_system *s, int n, const float *h_pose16, int max_support, int *h_anchor_ids, int *h_info8) {
    const char *what = "alva_system_create_anchors";
    g_sys_err[0] = 0;
    if (!s || !s->slam || !h_pose16 || !h_anchor_ids || !h_info8 || n < 1 || n > 16 || max_support < 8 || max_support > Anchor::MAX_SUPPORT)
        return bad_argument(what);
    s->anchors.sync(s->slam->map_generation);   // the anchors of a map that was thrown away are gone with it
    memset(h_info8, 0, (size_t) n * 8 * sizeof(int));
    for (int k = 0; k < n; k++) h_anchor_ids[k] = -1;
    if (s->last_status != 1) {   // initialising, reset, LOST or never called: the map is not one to tie a pose to
        for (int k = 0; k < n; k++) h_info8[8 * k] = 6;
        return 0;
    }
    return guarded(s, what, [&]() -> int {
        std::vector<int> ids, which;
        std::vector<double> pts;
        map_points_by_id(*s->slam, ids, pts);
        float poses[16 * 16];
        for (int k = 0; k < n; k++) {
            int *info = h_info8 + 8 * k;
            info[2] = (int) ids.size();
            bool finite = true;
            for (int c = 0; c < 16; c++) finite = finite && std::isfinite(h_pose16[16 * k + c]);
            if (!finite) info[0] = 4;
            else if (ids.size() < 4) info[0] = 1;
            else if (s->anchors.full()) info[0] = 3;
            if (info[0]) continue;
            memcpy(poses + 16 * which.size(), h_pose16 + 16 * k, 16 * sizeof(float));
            which.push_back(s->anchors.add(h_pose16 + 16 * k, max_support));
            h_anchor_ids[k] = s->anchors.list[which.back()].id;
        }
        if (which.empty()) return 0;
        const int rc = attach_anchors(s, which, poses, ids, pts);
        if (rc) {   // none of them exists without its supports
            s->anchors.n -= (int) which.size();
            for (int k = 0; k < n; k++) h_anchor_ids[k] = -1;
            return sys_fail(rc, what);
        }
        for (int k = 0, w = 0; k < n; k++)
            if (h_anchor_ids[k] >= 0) h_info8[8 * k + 1] = s->anchors.list[which[w++]].alive;
        return (int) which.size();
    });
}

extern "C" int alva_system_update_anchors(alva_system *s, int cap, int *h_anchor_ids, float *h_pose16, int *h_info8) {
    const char *what = "alva_system_update_anchors";
    g_sys_err[0] = 0;
    if (!s || !s->slam || cap < 0 || (cap > 0 && (!h_anchor_ids || !h_pose16 || !h_info8))) return bad_argument(what);
    Anchors &L = s->anchors;
    L.sync(s->slam->map_generation);
    if (cap < L.n) {
        snprintf(g_sys_err, sizeof(g_sys_err), "%s: cap %d is below the %d anchors kept", what, cap, L.n);
        return ALVA_ERR_ARG;
    }
    const int na = L.n;
    if (na == 0) return 0;
    memset(h_info8, 0, (size_t) na * 8 * sizeof(int));
    for (int k = 0; k < na; k++) {
        h_anchor_ids[k] = L.list[k].id;
        h_info8[8 * k + 4] = L.list[k].age;
        h_info8[8 * k + 5] = L.list[k].count_at_attach;
    }
    if (s->last_status != 1) {   // nothing runs: every anchor answers with its last pose, and the list waits for the pose to come back
        for (int k = 0; k < na; k++) {
            memcpy(h_pose16 + 16 * k, L.list[k].last_pose, 16 * sizeof(float));
            h_info8[8 * k] = 6;
            h_info8[8 * k + 1] = L.list[k].alive;
        }
        return na;
    }
    return guarded(s, what, [&]() -> int {
        const Slam &S = *s->slam;
        auto find = [&](int id, double *xyz) {   // existence is looked up now: the map layer knows nothing of anchors
            if (!S.map_points.count(id)) return false;
            const MpRec *r = S.map_points.at(id)->r;
            if (!r->is3d) return false;
            memcpy(xyz, r->X, 24);
            return true;
        };
        std::vector<int> count((size_t) na);
        std::vector<double> ref((size_t) na * 64 * 3), cur((size_t) na * 64 * 3);
        std::vector<float> pose_ref((size_t) na * 16);
        for (int k = 0; k < na; k++) {
            count[k] = L.gather(k, find, &ref[(size_t) k * 192], &cur[(size_t) k * 192]);
            memcpy(&pose_ref[16 * (size_t) k], L.list[k].ref_pose, 16 * sizeof(float));
        }
        std::vector<int> info((size_t) na * 8);
        int rc = s->scene->anchor_update(na, count.data(), ref.data(), cur.data(), pose_ref.data(), h_pose16, info.data());
        if (rc) return sys_fail(rc, what);
        std::vector<int> again;
        for (int k = 0; k < na; k++) {
            L.deliver(k, h_pose16 + 16 * k);
            h_info8[8 * k] = info[8 * (size_t) k];
            h_info8[8 * k + 1] = count[k];
            h_info8[8 * k + 2] = info[8 * (size_t) k + 2];
            h_info8[8 * k + 4] = L.list[k].age;
            if (L.wants_attach(k)) again.push_back(k);
        }
        if (again.empty()) return na;
        // re-attach at the new pose: it becomes the reference, the supports the K nearest of the points as they are now
        std::vector<int> ids;
        std::vector<double> pts;
        map_points_by_id(S, ids, pts);
        if (ids.size() < 4) return na;   // nothing to hold on to: the anchors keep what they have
        for (size_t b = 0; b < again.size(); b += 16) {
            const std::vector<int> which(again.begin() + b, again.begin() + std::min(again.size(), b + 16));
            float poses[16 * 16];
            for (size_t k = 0; k < which.size(); k++) memcpy(poses + 16 * k, h_pose16 + 16 * which[k], 16 * sizeof(float));
            rc = attach_anchors(s, which, poses, ids, pts);
            if (rc) return sys_fail(rc, what);
            for (int k: which) {
                h_info8[8 * k + 3] = 1;
                h_info8[8 * k + 5] = L.list[k].count_at_attach;
            }
        }
        return na;
    });
}

extern "C" int alva_system_remove_anchor(alva_system *s, int anchor_id) {
    if (!s) return 0;
    if (s->slam) s->anchors.sync(s->slam->map_generation);
    return s->anchors.remove(anchor_id);
}

extern "C" void alva_system_reset_anchors(alva_system *s) {
    if (s) s->anchors.clear();
}
