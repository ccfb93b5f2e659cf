// The scene features' device side (scene_stages.hpp): every method is one or more calls through include/alvaar_hip.h on the stream of the
// session's HipStages, on the frame it holds.  Host arrays cross through the stages' staging arenas (stage_arena.hpp).
#include "common.hpp"
#include "stage_arena.hpp"
#include "pose_internal.hpp"
#include "scene_stages.hpp"
#include "slam/image_place.hpp"

namespace alva_slam {

SceneStages::~SceneStages() {
    const HipStages::Frame f = hs.frame();
    (void) hipSetDevice(f.ctx->device);
    (void) alva_ctx_sync(f.ctx);
    if (depth_ring) (void) hipFree(depth_ring);
    if (dense_block) (void) hipFree(dense_block);
    if (mesh_block) (void) hipFree(mesh_block);
    if (mesh_out) (void) hipFree(mesh_out);
    if (ray_block) (void) hipFree(ray_block);
    if (mesh_color_block) (void) hipFree(mesh_color_block);
    if (mesh_alt) (void) hipFree(mesh_alt);
    if (mesh_color_alt) (void) hipFree(mesh_color_alt);
    if (color_thumb) (void) hipFree(color_thumb);
    if (color_done) (void) hipHostFree(color_done);
    if (img_orb) alva_orb_destroy(img_orb);
    if (img_block) (void) hipFree(img_block);
    if (light_block) (void) hipFree(light_block);
    if (light_started) (void) hipHostFree(light_started);
}

int SceneStages::hit_test(int n, const double *pts, const double *pose7_twc, const double *calib8, int n_rays, const float *uv, float radius_px,
                          int iterations, uint32_t seed, float *pose16, int *info8) {
    const HipStages::Frame f = hs.frame();
    StagePlan p;
    const size_t a = p.add((size_t) (n > 0 ? n : 0) * 24);
    std::vector<uint8_t *> d, h;
    int rc = hs.carve(p, d, h);
    if (rc) return rc;
    UP(f.st, a, pts, (size_t) (n > 0 ? n : 0) * 24);
    return alva_hit_test(f.ctx, n > 0 ? (const double *) d[a] : nullptr, n, pose7_twc, calib8, n_rays, uv, radius_px, iterations, seed, nullptr,
                         pose16, info8, nullptr);
}

int SceneStages::depth_keep(int slot) {
    const HipStages::Frame f = hs.frame();
    if (slot < 0 || slot >= DEPTH_SLOTS) return ALVA_ERR_ARG;
    const alva_level &L = *f.level0;
    if (!depth_ring) {
        depth_slot_bytes = (L.gray_pitch * (size_t) L.h + 255) / 256 * 256;
        ALVA_HIP(hipMalloc((void **) &depth_ring, depth_slot_bytes * DEPTH_SLOTS));
    }
    // rows in the pyramid's own pitch, so that one pitch serves both images of a sweep; behind the frame's kernels on the same stream
    alva_lane_flush();
    ALVA_HIP(hipMemcpy2DAsync(depth_ring + depth_slot_bytes * (size_t) slot, L.gray_pitch, L.gray, L.gray_pitch, (size_t) L.w, (size_t) L.h,
                              hipMemcpyDeviceToDevice, f.st));
    return ALVA_OK;
}

int SceneStages::depth_sweep(int slot, const double *calib8, const double *T_rc12, int step, int num_hyp, double rho_min, double rho_max,
                             int patch_radius, int min_texture, int min_conf, float *depth, uint8_t *conf, uint8_t *code, int *info8,
                             uint8_t *images2) {
    const HipStages::Frame f = hs.frame();
    if (slot < 0 || slot >= DEPTH_SLOTS || !depth_ring || step < 1) return ALVA_ERR_ARG;
    const alva_level &L = *f.level0;
    const uint8_t *ref = depth_ring + depth_slot_bytes * (size_t) slot;
    const size_t G = (size_t) (L.w / step) * (size_t) (L.h / step), P = (size_t) L.w * (size_t) L.h;
    StagePlan p;
    const size_t a = p.add(G * 4), b = p.add(G), c = p.add(G), e = p.add(images2 ? 2 * P : 0);
    std::vector<uint8_t *> d, h;
    int rc = hs.carve(p, d, h);
    if (rc) return rc;
    rc = alva_depth_sweep(f.ctx, L.gray, ref, L.gray_pitch, L.w, L.h, calib8, T_rc12, step, num_hyp, rho_min, rho_max, patch_radius,
                          min_texture, min_conf, (float *) d[a], d[b], d[c], info8, nullptr);
    if (rc) return rc;
    ALVA_HIP(hipMemcpyAsync(h[a], d[a], (size_t) (d[c] - d[a]) + G, hipMemcpyDeviceToHost, f.st));   // depth, conf and code are consecutive
    if (images2) {
        alva_lane_flush();
        ALVA_HIP(hipMemcpy2DAsync(h[e], (size_t) L.w, L.gray, L.gray_pitch, (size_t) L.w, (size_t) L.h, hipMemcpyDeviceToHost, f.st));
        ALVA_HIP(hipMemcpy2DAsync(h[e] + P, (size_t) L.w, ref, L.gray_pitch, (size_t) L.w, (size_t) L.h, hipMemcpyDeviceToHost, f.st));
    }
    ALVA_HIP(alva_stream_sync(f.st));
    memcpy(depth, h[a], G * 4);
    memcpy(conf, h[b], G);
    memcpy(code, h[c], G);
    if (images2) memcpy(images2, h[e], 2 * P);
    return ALVA_OK;
}

int SceneStages::depth_dense(const DepthDense &c) {
    const HipStages::Frame f = hs.frame();
    if (c.step < 1 || c.mode < 0 || c.mode > 2 || !c.depth || !c.weight || !c.src || !c.level || !c.info16) return ALVA_ERR_ARG;
    const alva_level &L = *f.level0;
    const int gw = L.w / c.step, gh = L.h / c.step;
    const size_t G = (size_t) gw * (size_t) gh, P = (size_t) L.w * (size_t) L.h;
    if (G == 0) return ALVA_ERR_ARG;
    const bool same_grid = dense_block && dense_gw == gw && dense_gh == gh;
    if (c.mode != 1 && !same_grid) return ALVA_ERR_STATE;   // (the caller keeps track of the state it asks to warp or fill)
    const bool sweep = c.mode >= 1 && c.slot >= 0;
    if (sweep && (c.slot >= DEPTH_SLOTS || !depth_ring)) return ALVA_ERR_ARG;
    if (dense_cap < G) {
        ALVA_HIP(alva_stream_sync(f.st));
        if (dense_block) ALVA_HIP(hipFree(dense_block));
        dense_block = nullptr;
        dense_cap = 0;
        dense_gw = dense_gh = 0;
        const size_t cap = (G + 255) / 256 * 256;
        ALVA_HIP(hipMalloc((void **) &dense_block, 11 * cap));
        dense_cap = cap;   // (only now: after a failed allocation the next call allocates again)
    }
    const bool dbg = c.dbg_rho_before || c.dbg_w_before || c.dbg_rho_after || c.dbg_raw_depth || c.dbg_raw_conf || c.dbg_raw_code || c.dbg_gray;
    StagePlan p;
    // device: the raw sweep images; both: depth, level (the fill's outputs), and for tests the state before and the gray image
    const size_t r_d = p.add(G * 4), r_cf = p.add(G), r_cd = p.add(G), o_d = p.add(G * 4), o_l = p.add(G), o_w = p.add(G), o_s = p.add(G),
                 b_r = p.add(dbg ? G * 4 : 0), b_w = p.add(dbg ? G : 0), a_r = p.add(dbg ? G * 4 : 0), e_g = p.add(dbg ? P : 0);
    std::vector<uint8_t *> d, h;
    int rc = hs.carve(p, d, h);
    if (rc) return rc;
    int info8[8] = {0, 0, 0, 0, 0, 0, 0, 0}, info4[4] = {0, 0, 0, 0};
    if (c.mode >= 1) {
        const int in = dense_cur, out = in ^ 1;
        const bool prev = c.mode == 2;
        if (dbg) {
            if (prev) {
                ALVA_HIP(hipMemcpyAsync(h[b_r], dense_rho(in), G * 4, hipMemcpyDeviceToHost, f.st));
                ALVA_HIP(hipMemcpyAsync(h[b_w], dense_w(in), G, hipMemcpyDeviceToHost, f.st));
            } else {
                memset(h[b_r], 0, G * 4);
                memset(h[b_w], 0, G);
            }
        }
        if (sweep) {
            rc = alva_depth_sweep(f.ctx, L.gray, depth_ring + depth_slot_bytes * (size_t) c.slot, L.gray_pitch, L.w, L.h, c.calib8, c.T_rc12,
                                  c.step, c.num_hyp, c.rho_min, c.rho_max, c.patch_radius, c.min_texture, c.min_conf, (float *) d[r_d], d[r_cf],
                                  d[r_cd], info8, nullptr);
            if (rc) return rc;
            c.info16[11] = info8[0];
        }
        static const double ident[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
        rc = alva_depth_fuse(f.ctx, prev ? dense_rho(in) : nullptr, prev ? dense_w(in) : nullptr, prev ? c.T_cp12 : ident, c.calib8, L.w, L.h,
                             c.step, sweep ? (const float *) d[r_d] : nullptr, sweep ? d[r_cf] : nullptr, sweep ? d[r_cd] : nullptr, c.decay, c.w_max,
                             c.rel_tol, dense_rho(out), dense_w(out), dense_src(), info8);
        if (rc) {
            dense_gw = dense_gh = 0;
            return rc;
        }
        for (int i = 0; i < 6; i++) c.info16[i] = info8[i];
        dense_cur = out;
        dense_gw = gw;
        dense_gh = gh;
    }
    const int k = dense_cur;
    if (dbg && c.mode == 0) {   // nothing is fused: before = after
        ALVA_HIP(hipMemcpyAsync(h[b_r], dense_rho(k), G * 4, hipMemcpyDeviceToHost, f.st));
        ALVA_HIP(hipMemcpyAsync(h[b_w], dense_w(k), G, hipMemcpyDeviceToHost, f.st));
    }
    rc = alva_depth_fill(f.ctx, dense_rho(k), dense_w(k), L.gray, L.gray_pitch, L.w, L.h, c.step, c.rho_ref, c.max_level, (float *) d[o_d],
                         d[o_l], info4);
    if (rc) return rc;
    c.info16[6] = info4[1];
    c.info16[7] = info4[2];
    c.info16[8] = gw;
    c.info16[9] = gh;
    // one set of downloads
    ALVA_HIP(hipMemcpyAsync(h[o_d], d[o_d], (size_t) (d[o_l] - d[o_d]) + G, hipMemcpyDeviceToHost, f.st));   // depth and level are consecutive
    ALVA_HIP(hipMemcpyAsync(h[o_w], dense_w(k), G, hipMemcpyDeviceToHost, f.st));
    ALVA_HIP(hipMemcpyAsync(h[o_s], dense_src(), G, hipMemcpyDeviceToHost, f.st));
    if (dbg) {
        ALVA_HIP(hipMemcpyAsync(h[a_r], dense_rho(k), G * 4, hipMemcpyDeviceToHost, f.st));
        if (c.mode >= 1 && sweep) ALVA_HIP(hipMemcpyAsync(h[r_d], d[r_d], (size_t) (d[r_cd] - d[r_d]) + G, hipMemcpyDeviceToHost, f.st));
        ALVA_HIP(hipMemcpy2DAsync(h[e_g], (size_t) L.w, L.gray, L.gray_pitch, (size_t) L.w, (size_t) L.h, hipMemcpyDeviceToHost, f.st));
    }
    ALVA_HIP(alva_stream_sync(f.st));
    memcpy(c.depth, h[o_d], G * 4);
    memcpy(c.level, h[o_l], G);
    memcpy(c.weight, h[o_w], G);
    memcpy(c.src, h[o_s], G);
    const bool swept = c.mode >= 1 && sweep;
    if (c.dbg_rho_before) memcpy(c.dbg_rho_before, h[b_r], G * 4);
    if (c.dbg_w_before) memcpy(c.dbg_w_before, h[b_w], G);
    if (c.dbg_rho_after) memcpy(c.dbg_rho_after, h[a_r], G * 4);
    if (dbg && !swept) {   // nothing was swept: no depth, no confidence, no code
        memset(h[r_d], 0, G * 4);
        memset(h[r_cf], 0, G);
        memset(h[r_cd], 255, G);
    }
    if (c.dbg_raw_depth) memcpy(c.dbg_raw_depth, h[r_d], G * 4);
    if (c.dbg_raw_conf) memcpy(c.dbg_raw_conf, h[r_cf], G);
    if (c.dbg_raw_code) memcpy(c.dbg_raw_code, h[r_cd], G);
    if (c.dbg_gray) memcpy(c.dbg_gray, h[e_g], P);
    return info4[0] + info4[1];
}

int SceneStages::mesh_update(const MeshUpdate &c) {
    const HipStages::Frame f = hs.frame();
    if (c.step < 1 || c.N < 4 || c.N > 256 || c.slot < 0 || c.slot >= DEPTH_SLOTS || !depth_ring || !c.info8 || !c.swept0) return ALVA_ERR_ARG;
    const alva_level &L = *f.level0;
    const size_t G = (size_t) (L.w / c.step) * (size_t) (L.h / c.step), V = (size_t) c.N * c.N * c.N;
    if (G == 0) return ALVA_ERR_ARG;
    bool zero = c.zero;
    if (!mesh_block || mesh_N != c.N) {
        ALVA_HIP(alva_stream_sync(f.st));
        if (mesh_block) ALVA_HIP(hipFree(mesh_block));
        mesh_block = nullptr;
        mesh_N = 0;
        ALVA_HIP(hipMalloc((void **) &mesh_block, (3 * V + 255) / 256 * 256));
        mesh_N = c.N;   // (only now: after a failed allocation the next call allocates again)
        zero = true;
    }
    if (zero) ALVA_HIP(hipMemsetAsync(mesh_block, 0, 3 * V, f.st));
    if (c.color_on) {   // the colour volume: allocated, replaced and zeroed where the distance volume is
        if (c.color_fuse && !color_thumb) return ALVA_ERR_STATE;
        bool czero = zero;
        if (!mesh_color_block || mesh_color_N != c.N) {
            ALVA_HIP(alva_stream_sync(f.st));
            if (mesh_color_block) ALVA_HIP(hipFree(mesh_color_block));
            mesh_color_block = nullptr;
            mesh_color_N = 0;
            ALVA_HIP(hipMalloc((void **) &mesh_color_block, (4 * V + 255) / 256 * 256));
            mesh_color_N = c.N;
            czero = true;
        }
        if (czero) ALVA_HIP(hipMemsetAsync(mesh_color_block, 0, 4 * V, f.st));
    }
    const bool dbg = c.dbg_raw_depth || c.dbg_raw_conf || c.dbg_raw_code;
    StagePlan p;
    const size_t r_d = p.add(G * 4), r_cf = p.add(G), r_cd = p.add(G);   // the raw sweep images: on the device, and for tests on the host
    std::vector<uint8_t *> d, h;
    int rc = hs.carve(p, d, h);
    if (rc) return rc;
    int sweep8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    rc = alva_depth_sweep(f.ctx, L.gray, depth_ring + depth_slot_bytes * (size_t) c.slot, L.gray_pitch, L.w, L.h, c.calib8, c.T_rc12, c.step,
                          c.num_hyp, c.rho_min, c.rho_max, c.patch_radius, c.min_texture, c.min_conf, (float *) d[r_d], d[r_cf], d[r_cd], sweep8,
                          nullptr);
    if (rc) return rc;
    *c.swept0 = sweep8[0];
    rc = c.color_on && c.color_fuse
             ? alva_mesh_integrate_color(f.ctx, mesh_q(), mesh_w(), mesh_color_block, c.N, c.origin3, c.voxel, c.trunc, c.T_cw12, c.calib8, L.w, L.h,
                                         c.step, (const float *) d[r_d], d[r_cf], d[r_cd], color_thumb, c.cstep, c.w_max, c.info8)
             : alva_mesh_integrate(f.ctx, mesh_q(), mesh_w(), c.N, c.origin3, c.voxel, c.trunc, c.T_cw12, c.calib8, L.w, L.h, c.step,
                                   (const float *) d[r_d], d[r_cf], d[r_cd], c.w_max, c.info8);
    if (rc) return rc;
    if (dbg || c.dbg_q || c.dbg_w) {
        if (dbg) ALVA_HIP(hipMemcpyAsync(h[r_d], d[r_d], (size_t) (d[r_cd] - d[r_d]) + G, hipMemcpyDeviceToHost, f.st));   // consecutive
        if (c.dbg_q) ALVA_HIP(hipMemcpyAsync(c.dbg_q, mesh_q(), 2 * V, hipMemcpyDeviceToHost, f.st));
        if (c.dbg_w) ALVA_HIP(hipMemcpyAsync(c.dbg_w, mesh_w(), V, hipMemcpyDeviceToHost, f.st));
        ALVA_HIP(alva_stream_sync(f.st));
        if (c.dbg_raw_depth) memcpy(c.dbg_raw_depth, h[r_d], G * 4);
        if (c.dbg_raw_conf) memcpy(c.dbg_raw_conf, h[r_cf], G);
        if (c.dbg_raw_code) memcpy(c.dbg_raw_code, h[r_cd], G);
    }
    return ALVA_OK;
}

int SceneStages::mesh_extract(const double *origin3, double voxel, int min_weight, int max_vertices, int max_triangles, float *vertices,
                              float *normals, int *triangles, int *info8, uint8_t *colors, int *n_colored) {
    const HipStages::Frame f = hs.frame();
    if (!mesh_block) return ALVA_ERR_STATE;
    if (max_vertices < 1 || max_triangles < 1 || !vertices || !normals || !triangles || !info8) return ALVA_ERR_ARG;
    const size_t vb = ((size_t) max_vertices * 12 + 255) / 256 * 256, tb = ((size_t) max_triangles * 12 + 255) / 256 * 256;
    const size_t cb = colors ? ((size_t) max_vertices * 5 + 255) / 256 * 256 : 0;   // rgba [max_vertices][4], then the codes
    if (mesh_out_bytes < 2 * vb + tb + cb) {
        ALVA_HIP(alva_stream_sync(f.st));
        if (mesh_out) ALVA_HIP(hipFree(mesh_out));
        mesh_out = nullptr;
        mesh_out_bytes = 0;
        ALVA_HIP(hipMalloc((void **) &mesh_out, 2 * vb + tb + cb));
        mesh_out_bytes = 2 * vb + tb + cb;
    }
    float *d_v = (float *) mesh_out, *d_n = (float *) (mesh_out + vb);
    int *d_t = (int *) (mesh_out + 2 * vb);
    const int rc = alva_mesh_extract(f.ctx, mesh_q(), mesh_w(), mesh_N, origin3, voxel, min_weight, max_vertices, max_triangles, d_v, d_n, d_t,
                                     info8);
    if (rc) return rc;
    if (n_colored) *n_colored = 0;
    if (info8[0] == 0) {   // the counts are known only now: a second, exact download
        const size_t nv = (size_t) info8[1];
        if (colors && has_mesh_color()) {   // the colour volume at the vertices, where they are: on the device
            uint8_t *d_rgba = mesh_out + 2 * vb + tb, *d_code = d_rgba + (size_t) max_vertices * 4;
            for (size_t at = 0; at < nv; at += (size_t) 1 << 20) {
                const int n = (int) (nv - at < ((size_t) 1 << 20) ? nv - at : (size_t) 1 << 20);
                int cinfo[8];
                const int crc = alva_mesh_color_at(f.ctx, mesh_color_block, mesh_N, origin3, voxel, n, d_v + 3 * at, d_rgba + 4 * at, d_code + at, cinfo);
                if (crc) return crc;
                if (n_colored) *n_colored += cinfo[1];
            }
            ALVA_HIP(hipMemcpyAsync(colors, d_rgba, nv * 4, hipMemcpyDeviceToHost, f.st));
        } else if (colors) memset(colors, 0, nv * 4);
        ALVA_HIP(hipMemcpyAsync(vertices, d_v, nv * 12, hipMemcpyDeviceToHost, f.st));
        ALVA_HIP(hipMemcpyAsync(normals, d_n, nv * 12, hipMemcpyDeviceToHost, f.st));
        if (info8[2] > 0) ALVA_HIP(hipMemcpyAsync(triangles, d_t, (size_t) info8[2] * 12, hipMemcpyDeviceToHost, f.st));
        ALVA_HIP(alva_stream_sync(f.st));
    }
    return ALVA_OK;
}

int SceneStages::mesh_clear() {
    const HipStages::Frame f = hs.frame();
    if (mesh_block) ALVA_HIP(hipMemsetAsync(mesh_block, 0, 3 * (size_t) mesh_N * mesh_N * mesh_N, f.st));
    if (mesh_color_block) ALVA_HIP(hipMemsetAsync(mesh_color_block, 0, 4 * (size_t) mesh_color_N * mesh_color_N * mesh_color_N, f.st));
    return ALVA_OK;
}

int SceneStages::mesh_shift(const int *shift3, int *info8) {
    const HipStages::Frame f = hs.frame();
    if (!mesh_block) return ALVA_ERR_STATE;
    if (!shift3 || !info8) return ALVA_ERR_ARG;
    const size_t V = (size_t) mesh_N * mesh_N * mesh_N;
    const bool color = has_mesh_color();
    if (!mesh_alt || mesh_alt_N != mesh_N) {
        ALVA_HIP(alva_stream_sync(f.st));
        if (mesh_alt) ALVA_HIP(hipFree(mesh_alt));
        mesh_alt = nullptr;
        mesh_alt_N = 0;
        ALVA_HIP(hipMalloc((void **) &mesh_alt, (3 * V + 255) / 256 * 256));
        mesh_alt_N = mesh_N;
    }
    if (color && (!mesh_color_alt || mesh_color_alt_N != mesh_N)) {
        ALVA_HIP(alva_stream_sync(f.st));
        if (mesh_color_alt) ALVA_HIP(hipFree(mesh_color_alt));
        mesh_color_alt = nullptr;
        mesh_color_alt_N = 0;
        ALVA_HIP(hipMalloc((void **) &mesh_color_alt, (4 * V + 255) / 256 * 256));
        mesh_color_alt_N = mesh_N;
    }
    const int rc = alva_mesh_shift(f.ctx, mesh_q(), mesh_w(), color ? mesh_color_block : nullptr, mesh_N, shift3, (int16_t *) mesh_alt,
                                   mesh_alt + 2 * V, color ? mesh_color_alt : nullptr, info8);
    if (rc) return rc;
    // the stage has waited: the old blocks are no longer read.  Both blocks of a pair are of mesh_N
    std::swap(mesh_block, mesh_alt);
    if (color) std::swap(mesh_color_block, mesh_color_alt);
    return ALVA_OK;
}

int SceneStages::ray_reserve(size_t n) {
    if (ray_cap >= n) return ALVA_OK;
    const HipStages::Frame f = hs.frame();
    ALVA_HIP(alva_stream_sync(f.st));
    if (ray_block) ALVA_HIP(hipFree(ray_block));
    ray_block = nullptr;
    ray_cap = 0;
    const size_t cap = (n + 255) / 256 * 256;
    ALVA_HIP(hipMalloc((void **) &ray_block, RAY_BYTES * cap));
    ray_cap = cap;   // (only now: after a failed allocation the next call allocates again)
    return ALVA_OK;
}

int SceneStages::color_frame(int cstep, bool wait, bool *pending) {
    const HipStages::Frame f = hs.frame();
    *pending = false;
    if (!f.src) return ALVA_ERR_STATE;
    const Camera &k = *f.cam;
    if (cstep < 1 || k.width / cstep < 1 || k.height / cstep < 1) return ALVA_ERR_ARG;
    const size_t bytes = ((size_t) (k.width / cstep) * (size_t) (k.height / cstep) * 4 + 255) / 256 * 256;
    if (!color_done) {
        ALVA_HIP(hipHostMalloc((void **) &color_done, 64, hipHostMallocDefault));
        *color_done = 0;
    }
    if (!color_thumb || color_thumb_bytes != bytes) {
        ALVA_HIP(alva_stream_sync(f.st));
        if (color_thumb) ALVA_HIP(hipFree(color_thumb));
        color_thumb = nullptr;
        ALVA_HIP(hipMalloc((void **) &color_thumb, bytes + 256));
        color_thumb_bytes = bytes;
        color_thumb_exact = (size_t) (k.width / cstep) * (size_t) (k.height / cstep) * 4;
        ALVA_HIP(hipMemsetAsync(color_thumb, 0, bytes + 256, f.st));   // (the arrival counter behind the thumbnail starts at zero)
    }
    // as light_frame: the staging copy is the session's own; any other source is the caller's memory and must have been read when the
    // call returns.  The launch's last workgroup says so in a word in pinned memory, polled like the tracking step's
    const bool callers_memory = !f.src_is_staging, word = callers_memory && wait && f.poll;
    const uint32_t seq = ++color_seq ? color_seq : ++color_seq;   // (never 0, the word's first value)
    const int rc = alva_color_thumb_done(f.ctx, f.src, (size_t) k.width * 4, k.width, k.height, cstep, color_thumb,
                                         word ? (uint32_t *) (color_thumb + color_thumb_bytes) : nullptr, word ? color_done : nullptr, seq);
    if (rc) return rc;
    if (callers_memory && !wait) *pending = true;
    else if (callers_memory) {
        if (!f.poll) ALVA_HIP(alva_stream_sync(f.st));
        else if (!alva_wait_until([&] { return *(volatile uint32_t *) color_done == seq; }, f.st)) {
            alva_set_error("color_frame: the thumbnail never finished");
            return ALVA_ERR_HIP;
        }
    }
    return ALVA_OK;
}

int SceneStages::frame_wait() {
    const HipStages::Frame f = hs.frame();
    ALVA_HIP(alva_stream_sync(f.st));
    return ALVA_OK;
}

int SceneStages::mesh_color_at(const double *origin3, double voxel, int n, const float *points3, uint8_t *rgba, uint8_t *codes, int *info8) {
    const HipStages::Frame f = hs.frame();
    if (!has_mesh_color()) return ALVA_ERR_STATE;
    if (n < 1 || n > (1 << 20) || !points3 || !rgba || !codes || !info8) return ALVA_ERR_ARG;
    const int rc0 = ray_reserve((size_t) n);
    if (rc0) return rc0;
    uint8_t *B = ray_block;   // the points, the colours, the codes: 17 of the block's bytes per ray
    float *d_p = (float *) B;
    uint8_t *d_rgba = B + 12 * ray_cap, *d_code = B + 16 * ray_cap;
    ALVA_HIP(hipMemcpyAsync(d_p, points3, (size_t) n * 12, hipMemcpyHostToDevice, f.st));   // (pageable: returns when the source has been read)
    const int rc = alva_mesh_color_at(f.ctx, mesh_color_block, mesh_N, origin3, voxel, n, d_p, d_rgba, d_code, info8);
    if (rc) return rc;
    ALVA_HIP(hipMemcpyAsync(rgba, d_rgba, (size_t) n * 4, hipMemcpyDeviceToHost, f.st));
    ALVA_HIP(hipMemcpyAsync(codes, d_code, (size_t) n, hipMemcpyDeviceToHost, f.st));
    ALVA_HIP(alva_stream_sync(f.st));
    return ALVA_OK;
}

int SceneStages::mesh_color_debug(uint8_t *thumb, uint8_t *c) {
    const HipStages::Frame f = hs.frame();
    if (thumb && color_thumb) ALVA_HIP(hipMemcpyAsync(thumb, color_thumb, color_thumb_exact, hipMemcpyDeviceToHost, f.st));
    if (c && has_mesh_color()) ALVA_HIP(hipMemcpyAsync(c, mesh_color_block, 4 * (size_t) mesh_N * mesh_N * mesh_N, hipMemcpyDeviceToHost, f.st));
    ALVA_HIP(alva_stream_sync(f.st));
    return ALVA_OK;
}

int SceneStages::mesh_color_drop() {
    const HipStages::Frame f = hs.frame();
    if (!mesh_color_block && !color_thumb && !mesh_color_alt) return ALVA_OK;
    ALVA_HIP(alva_stream_sync(f.st));
    if (mesh_color_block) ALVA_HIP(hipFree(mesh_color_block));
    mesh_color_block = nullptr;
    mesh_color_N = 0;
    if (mesh_color_alt) ALVA_HIP(hipFree(mesh_color_alt));
    mesh_color_alt = nullptr;
    mesh_color_alt_N = 0;
    if (color_thumb) ALVA_HIP(hipFree(color_thumb));
    color_thumb = nullptr;
    color_thumb_bytes = 0;
    return ALVA_OK;
}

int SceneStages::mesh_raycast(const MeshRaycast &c) {
    const HipStages::Frame f = hs.frame();
    if (!mesh_block) return ALVA_ERR_STATE;
    const bool pixels = c.T_wc12 != nullptr, grid = pixels && !c.uv;
    if (!c.info8 || !c.origin3 || (pixels ? !c.calib8 || c.step < 1 || c.width < 1 || c.height < 1 : !c.rays6 || c.poses || c.pose_ok)) return ALVA_ERR_ARG;
    const size_t n = grid ? (size_t) (c.width / c.step) * (size_t) (c.height / c.step) : (size_t) (c.n > 0 ? c.n : 0);
    if (n < 1 || n > ((size_t) 1 << 22) || (c.pose_ok && !c.poses)) return ALVA_ERR_ARG;
    const int rrc = ray_reserve(n);
    if (rrc) return rrc;
    uint8_t *B = ray_block;
    float *d_t = (float *) (B + 48 * ray_cap), *d_p = (float *) (B + 52 * ray_cap), *d_n = (float *) (B + 64 * ray_cap);
    float *d_pose = (float *) (B + 76 * ray_cap);
    uint8_t *d_code = B + 140 * ray_cap, *d_ok = B + 141 * ray_cap;
    // (pageable host memory: the copies return when the source has been read)
    if (!pixels) ALVA_HIP(hipMemcpyAsync(B, c.rays6, n * 48, hipMemcpyHostToDevice, f.st));
    else if (c.uv) ALVA_HIP(hipMemcpyAsync(B, c.uv, n * 8, hipMemcpyHostToDevice, f.st));
    const int rc = pixels ? alva_mesh_raycast_pixels(f.ctx, mesh_q(), mesh_w(), mesh_N, c.origin3, c.voxel, c.min_weight, c.T_wc12, c.calib8, c.width,
                                                     c.height, c.step, (int) n, c.uv ? (const float *) B : nullptr, c.t_near, c.t_far, d_t, d_p, d_n,
                                                     d_code, c.poses ? d_pose : nullptr, c.pose_ok ? d_ok : nullptr, c.info8)
                          : alva_mesh_raycast(f.ctx, mesh_q(), mesh_w(), mesh_N, c.origin3, c.voxel, c.min_weight, (int) n, (const double *) B,
                                              c.t_near, c.t_far, d_t, d_p, d_n, d_code, c.info8);
    if (rc) return rc;
    if (c.t) ALVA_HIP(hipMemcpyAsync(c.t, d_t, n * 4, hipMemcpyDeviceToHost, f.st));
    if (c.points) ALVA_HIP(hipMemcpyAsync(c.points, d_p, n * 12, hipMemcpyDeviceToHost, f.st));
    if (c.normals) ALVA_HIP(hipMemcpyAsync(c.normals, d_n, n * 12, hipMemcpyDeviceToHost, f.st));
    if (c.codes) ALVA_HIP(hipMemcpyAsync(c.codes, d_code, n, hipMemcpyDeviceToHost, f.st));
    if (c.poses) ALVA_HIP(hipMemcpyAsync(c.poses, d_pose, n * 64, hipMemcpyDeviceToHost, f.st));
    if (c.pose_ok) ALVA_HIP(hipMemcpyAsync(c.pose_ok, d_ok, n, hipMemcpyDeviceToHost, f.st));
    ALVA_HIP(alva_stream_sync(f.st));
    return ALVA_OK;
}

int SceneStages::light_frame(const double *R_wc9, int step, int min_pixels, int w_new, int w_max) {
    const HipStages::Frame f = hs.frame();
    if (!f.src) return ALVA_ERR_STATE;
    if (!light_started) {
        ALVA_HIP(hipHostMalloc((void **) &light_started, 64, hipHostMallocDefault));
        *light_started = 0;
    }
    if (!light_block) {
        ALVA_HIP(hipMalloc((void **) &light_block, LIGHT_BLOCK_BYTES));
        ALVA_HIP(hipMemsetAsync(light_block, 0, LIGHT_BLOCK_BYTES, f.st));
    }
    const Camera &k = *f.cam;
    const double calib8[8] = {k.fx, k.fy, k.cx, k.cy, k.k1, k.k2, k.p1, k.p2};
    int rc = alva_light_bin(f.ctx, f.src, (size_t) k.width * 4, k.width, k.height, calib8, R_wc9, step, light_acc());
    if (rc) return rc;
    // the staging copy is the session's own and the next upload is ordered behind these launches; any other source is the caller's
    // memory, which it may overwrite as soon as the call returns: the bin has to have read it by then.  The fuse says so when it starts
    // (it need not have finished): a word in pinned memory, polled like the tracking step's
    const bool callers_memory = !f.src_is_staging;
    const uint32_t seq = ++light_seq ? light_seq : ++light_seq;   // (never 0, the word's first value)
    rc = alva_light_fuse_started(f.ctx, light_acc(), light_state(), min_pixels, w_new, w_max, light_acc_last(),
                                 callers_memory && f.poll ? light_started : nullptr, seq);
    if (rc) return rc;
    if (callers_memory) {
        if (!f.poll) ALVA_HIP(alva_stream_sync(f.st));
        else if (!alva_wait_until([&] { return *(volatile uint32_t *) light_started == seq; }, f.st)) {
            alva_set_error("light_frame: the fuse never started");
            return ALVA_ERR_HIP;
        }
    }
    return ALVA_OK;
}

int SceneStages::light_estimate(float *sh27, float *primary_dir3, float *primary_rgb3, float *ambient4, int *info8, uint64_t *dbg_acc,
                                uint8_t *dbg_state) {
    const HipStages::Frame f = hs.frame();
    if (!light_block) return ALVA_ERR_STATE;
    if (dbg_acc) ALVA_HIP(hipMemcpyAsync(dbg_acc, light_acc_last(), ALVA_LIGHT_ACC_WORDS * 8, hipMemcpyDeviceToHost, f.st));
    if (dbg_state) ALVA_HIP(hipMemcpyAsync(dbg_state, light_state(), ALVA_LIGHT_STATE_BYTES, hipMemcpyDeviceToHost, f.st));
    return alva_light_estimate(f.ctx, light_state(), sh27, primary_dir3, primary_rgb3, ambient4, info8);   // (its wait covers the copies)
}

int SceneStages::light_clear() {
    const HipStages::Frame f = hs.frame();
    if (light_block) ALVA_HIP(hipMemsetAsync(light_block, 0, LIGHT_BLOCK_BYTES, f.st));
    return ALVA_OK;
}

int SceneStages::image_describe(const uint8_t *gray, int width, int height, size_t pitch, int nlevels, float *xy, uint8_t *desc, int *count) {
    const HipStages::Frame f = hs.frame();
    *count = 0;
    constexpr int CAP = ALVA_IMAGE_QUERY_CAP;
    alva_orb *orb = nullptr;
    uint8_t *blk = nullptr;
    const size_t img_bytes = ((size_t) width * height + 255) / 256 * 256;
    int rc = alva_orb_create(f.ctx, width, height, 500, 1.2f, nlevels, 20, &orb);
    if (rc) return rc;
    int n = 0;
    std::vector<float> kp((size_t) CAP * 6);
    do {
        if (hipMalloc((void **) &blk, img_bytes + (size_t) CAP * (24 + 32)) != hipSuccess) {
            rc = ALVA_ERR_NOMEM;
            break;
        }
        alva_lane_flush();
        if (hipMemcpy2DAsync(blk, (size_t) width, gray, pitch, (size_t) width, (size_t) height, hipMemcpyHostToDevice, f.st) != hipSuccess) {
            rc = ALVA_ERR_HIP;
            break;
        }
        float *d_kp = (float *) (blk + img_bytes);
        uint8_t *d_desc = blk + img_bytes + (size_t) CAP * 24;
        rc = alva_orb_detect_and_compute(f.ctx, orb, blk, (size_t) width, d_kp, d_desc, CAP, &n);
        if (rc) break;
        n = n < CAP ? n : CAP;
        if (n > 0 && (hipMemcpy(kp.data(), d_kp, (size_t) n * 24, hipMemcpyDeviceToHost) != hipSuccess ||
                      hipMemcpy(desc, d_desc, (size_t) n * 32, hipMemcpyDeviceToHost) != hipSuccess))
            rc = ALVA_ERR_HIP;
    } while (false);
    (void) alva_stream_sync(f.st);
    if (blk) (void) hipFree(blk);
    alva_orb_destroy(orb);
    if (rc) return rc;
    for (int i = 0; i < n; i++) {
        xy[2 * i] = kp[6 * (size_t) i];
        xy[2 * i + 1] = kp[6 * (size_t) i + 1];
    }
    *count = n;
    return ALVA_OK;
}

int SceneStages::image_detect(const ImageDetectCall &c) {
    const HipStages::Frame f = hs.frame();
    constexpr int QC = ALVA_IMAGE_QUERY_CAP, TC = ALVA_IMAGE_TRAIN_CAP;
    if (!f.src || c.n_images < 1 || c.n_images > ALVA_IMAGE_MAX) return ALVA_ERR_STATE;
    const alva_level &L = *f.level0;
    const Camera &k = *f.cam;
    if (!img_orb) {
        const int rc = alva_orb_create(f.ctx, L.w, L.h, 1500, 1.2f, 8, 20, &img_orb);
        if (rc) return rc;
    }
    if (!img_block) {
        ALVA_HIP(hipMalloc((void **) &img_block, IMG_BLOCK_BYTES));
        img_version = -1;
    }
    uint8_t *B = img_block;
    float *d_kp = (float *) (B + IMG_KP), *d_xy = (float *) (B + IMG_XY), *d_unpx = (float *) (B + IMG_UNPX);
    uint8_t *d_desc = B + IMG_DESC, *d_qdesc = B + IMG_QDESC;
    float *d_qxy = (float *) (B + IMG_QXY);
    int *d_match = (int *) (B + IMG_MATCH), *d_count = (int *) (B + IMG_COUNT);
    double *d_pairs = (double *) (B + IMG_PAIRS), *d_uv = (double *) (B + IMG_UV), *d_wpt = (double *) (B + IMG_WPT);
    const size_t n_img = (size_t) c.n_images;
    if (img_version != c.version) {   // (pageable host memory: the copies return when the source has been read)
        ALVA_HIP(hipMemcpyAsync(d_qdesc, c.desc, n_img * QC * 32, hipMemcpyHostToDevice, f.st));
        ALVA_HIP(hipMemcpyAsync(d_qxy, c.xy, n_img * QC * 8, hipMemcpyHostToDevice, f.st));
        img_version = c.version;
    }
    // the frame: ORB on level 0 of the pyramid the session holds, the keypoints' positions undistorted
    int n = 0;
    int rc = alva_orb_detect_and_compute(f.ctx, img_orb, L.gray, L.gray_pitch, d_kp, d_desc, TC, &n);   // (waits: the count)
    if (rc) return rc;
    n = n < TC ? n : TC;
    if (n > 0) {
        alva_lane_flush();
        ALVA_HIP(hipMemcpy2DAsync(d_xy, 8, d_kp, 24, 8, (size_t) n, hipMemcpyDeviceToDevice, f.st));
        rc = alva_undistort_points(f.ctx, d_xy, n, k.fx, k.fy, k.cx, k.cy, k.k1, k.k2, k.p1, k.p2, d_unpx);
        if (rc) return rc;
    }
    rc = alva_image_match(f.ctx, c.n_images, d_qdesc, d_qxy, c.nq, d_desc, d_unpx, alva_orb_device_count(img_orb), TC, 64, 0.8f, d_match, d_pairs,
                          d_count);
    if (rc) return rc;
    std::vector<double> pairs(n_img * QC * 4);
    std::vector<int> count(n_img);
    ALVA_HIP(hipMemcpyAsync(pairs.data(), d_pairs, pairs.size() * 8, hipMemcpyDeviceToHost, f.st));
    ALVA_HIP(hipMemcpyAsync(count.data(), d_count, n_img * 4, hipMemcpyDeviceToHost, f.st));
    if (c.dbg_kp && n > 0) ALVA_HIP(hipMemcpyAsync(c.dbg_kp, d_xy, (size_t) n * 8, hipMemcpyDeviceToHost, f.st));
    if (c.dbg_unpx && n > 0) ALVA_HIP(hipMemcpyAsync(c.dbg_unpx, d_unpx, (size_t) n * 8, hipMemcpyDeviceToHost, f.st));
    if (c.dbg_desc && n > 0) ALVA_HIP(hipMemcpyAsync(c.dbg_desc, d_desc, (size_t) n * 32, hipMemcpyDeviceToHost, f.st));
    if (c.dbg_match) ALVA_HIP(hipMemcpyAsync(c.dbg_match, d_match, n_img * QC * 12, hipMemcpyDeviceToHost, f.st));
    if (c.dbg_n_frame) *c.dbg_n_frame = n;
    const double calib4[4] = {k.fx, k.fy, k.cx, k.cy};
    rc = alva_image_homography(f.ctx, c.n_images, d_pairs, d_count, c.wh, L.w, L.h, calib4, c.iterations, c.threshold_px, c.min_inliers, 12345u,
                               nullptr, c.H9, c.info8, c.mask, c.R9, c.t3);   // (its wait covers the copies)
    if (rc) return rc;
    if (c.dbg_xy) memcpy(c.dbg_xy, pairs.data(), pairs.size() * 8);
    if (c.dbg_count) memcpy(c.dbg_count, count.data(), n_img * 4);
    if (c.dbg_stage_info8) memcpy(c.dbg_stage_info8, c.info8, n_img * 32);
    if (c.dbg_stage_R9) memcpy(c.dbg_stage_R9, c.R9, n_img * 72);
    if (c.dbg_stage_t3) memcpy(c.dbg_stage_t3, c.t3, n_img * 24);
    // the refinement: the winner's inliers as points (p.x, p.y, 0) of the picture's frame against their undistorted pixels, through the
    // tracker's own minimiser with the tracker's parameters (pnp above), from stage 2's pose; one wait per refined picture
    for (int j = 0; j < c.n_images; j++) {
        int *info = c.info8 + 8 * j;
        info[6] = n;
        if (info[0] != 0) continue;
        const int mj = info[1], w = c.wh[2 * j], h = c.wh[2 * j + 1];
        const double *xy4 = pairs.data() + (size_t) j * QC * 4;
        std::vector<double> uv, wpt;
        for (int i = 0; i < mj; i++)
            if (c.mask[(size_t) j * QC + i]) {
                uv.push_back(xy4[4 * i + 2]);
                uv.push_back(xy4[4 * i + 3]);
                wpt.push_back((xy4[4 * i] - (double) w / 2) / (double) w);
                wpt.push_back((xy4[4 * i + 1] - (double) h / 2) / (double) w);
                wpt.push_back(0.0);
            }
        const int ni = (int) (uv.size() / 2);
        ALVA_HIP(hipMemcpyAsync(d_uv, uv.data(), uv.size() * 8, hipMemcpyHostToDevice, f.st));
        ALVA_HIP(hipMemcpyAsync(d_wpt, wpt.data(), wpt.size() * 8, hipMemcpyHostToDevice, f.st));
        double pose7[7], pinfo[8];
        image_pose_to_twc7(c.R9 + 9 * j, c.t3 + 3 * j, pose7);
        std::vector<int> outliers((size_t) ni);
        int n_out = 0, ok = 0;
        rc = SessionPose(k.fx, k.fy, k.cx, k.cy).refine(f.ctx, d_uv, d_wpt, ni, pose7, outliers.data(), &n_out, pinfo, &ok);
        if (rc) return rc;
        double R[9], t[3];
        if (ok) image_pose_from_twc7(pose7, R, t);
        const int kept = ok ? image_count_inliers(R, t, w, h, calib4, xy4, mj, (double) c.threshold_px, nullptr) : 0;
        info[4] = kept;
        if (!ok || kept < c.min_inliers) {
            info[0] = 4;
            memset(c.R9 + 9 * j, 0, 72);
            memset(c.t3 + 3 * j, 0, 24);
            continue;
        }
        memcpy(c.R9 + 9 * j, R, 72);
        memcpy(c.t3 + 3 * j, t, 24);
    }
    return ALVA_OK;
}

int SceneStages::planes(const PlaneCall &c) {
    const HipStages::Frame f = hs.frame();
    StagePlan p;
    const int n = c.n;
    const size_t np = (size_t) (n > 0 ? n : 0);
    const size_t a = p.add(np * 24), b = p.add(np * 4);
    std::vector<uint8_t *> d, h;
    int rc = hs.carve(p, d, h);
    if (rc) return rc;
    UP(f.st, a, c.pts, np * 24);
    const double *d_pts = n > 0 ? (const double *) d[a] : nullptr;
    int *d_labels = n > 0 && (c.labels || c.max_vertices) ? (int *) d[b] : nullptr;   // the outlines need them whether or not the caller does
    rc = c.n_prior == 0 ? alva_detect_planes(f.ctx, d_pts, n, c.pose7_twc, c.thickness, c.min_inliers, c.max_planes, c.iterations, c.seed, nullptr,
                                             c.planes24, c.info8, d_labels, nullptr)
                        : alva_track_planes(f.ctx, d_pts, n, c.pose7_twc, c.thickness, c.min_inliers, c.max_planes, c.iterations, c.seed, nullptr,
                                            c.n_prior, c.prior24, c.planes24, c.info8, d_labels, nullptr);
    if (rc < 0) return rc;
    if (c.labels && n > 0) DOWN(f.st, b, np * 4);   // queued ahead of the outline launch: alva_plane_outlines' wait covers it
    if (c.max_vertices) {
        rc = alva_plane_outlines(f.ctx, d_pts, n, d_labels, c.max_planes, c.planes24, c.max_vertices, c.outline, nullptr, c.outline_info8, c.area);
        if (rc < 0) return rc;
    }
    if (c.labels && n > 0) {
        ALVA_HIP(alva_stream_sync(f.st));   // (alva_plane_outlines returns without a wait when no plane has a frame)
        memcpy(c.labels, h[b], np * 4);
    }
    return ALVA_OK;
}

int SceneStages::anchor_attach(int n, const double *pts, int n_anchors, const double *pos3, int max_support, int *index, double *dist2,
                               int *count) {
    const HipStages::Frame f = hs.frame();
    StagePlan p;
    const size_t np = (size_t) (n > 0 ? n : 0);
    const size_t a = p.add(np * 24);
    std::vector<uint8_t *> d, h;
    int rc = hs.carve(p, d, h);
    if (rc) return rc;
    UP(f.st, a, pts, np * 24);
    return alva_anchor_attach(f.ctx, n > 0 ? (const double *) d[a] : nullptr, n, n_anchors, pos3, max_support, index, dist2, count);
}

int SceneStages::anchor_update(int n_anchors, const int *count, const double *ref, const double *cur, const float *pose16_ref, float *pose16,
                               int *info8) {
    const HipStages::Frame f = hs.frame();
    return alva_anchor_update(f.ctx, n_anchors, count, ref, cur, pose16_ref, pose16, nullptr, info8);   // (its inputs travel in pinned memory)
}

}  // namespace alva_slam
