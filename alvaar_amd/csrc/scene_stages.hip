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
    if (img_orb) alva_orb_destroy(img_orb);
}   // (the blocks and the pinned words free themselves, after the wait above)

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
        const int rc = depth_ring.allocate(depth_slot_bytes * DEPTH_SLOTS);
        if (rc) return rc;
    }
    // rows in the pyramid's own pitch, so that one pitch serves both images of a sweep; behind the frame's kernels on the same stream
    alva_lane_flush();
    ALVA_HIP(hipMemcpy2DAsync(depth_ring.ptr + depth_slot_bytes * (size_t) slot, L.gray_pitch, L.gray, L.gray_pitch, (size_t) L.w, (size_t) L.h,
                              hipMemcpyDeviceToDevice, f.st));
    return ALVA_OK;
}

int SceneStages::sweep(int slot, const double *calib8, const double *T_rc12, const SweepParams &p, double rho_min, double rho_max,
                       float *d_depth, uint8_t *d_conf, uint8_t *d_code, int *info8) {
    const HipStages::Frame f = hs.frame();
    if (slot < 0 || slot >= DEPTH_SLOTS || !depth_ring) return ALVA_ERR_ARG;
    const alva_level &L = *f.level0;
    return alva_depth_sweep(f.ctx, L.gray, depth_ring.ptr + depth_slot_bytes * (size_t) slot, L.gray_pitch, L.w, L.h, calib8, T_rc12, p.step,
                            p.num_hyp, rho_min, rho_max, p.patch_radius, p.min_texture, p.min_conf, d_depth, d_conf, d_code, info8, nullptr);
}

int SceneStages::depth_sweep(int slot, const double *calib8, const double *T_rc12, const SweepParams &sp, double rho_min, double rho_max,
                             float *depth, uint8_t *conf, uint8_t *code, int *info8, uint8_t *images2) {
    const HipStages::Frame f = hs.frame();
    if (sp.step < 1) return ALVA_ERR_ARG;
    const alva_level &L = *f.level0;
    const size_t G = (size_t) (L.w / sp.step) * (size_t) (L.h / sp.step), P = (size_t) L.w * (size_t) L.h;
    StagePlan p;
    const size_t a = p.add(G * 4), b = p.add(G), c = p.add(G), e = p.add(images2 ? 2 * P : 0);
    std::vector<uint8_t *> d, h;
    int rc = hs.carve(p, d, h);
    if (rc) return rc;
    rc = sweep(slot, calib8, T_rc12, sp, rho_min, rho_max, (float *) d[a], d[b], d[c], info8);
    if (rc) return rc;
    ALVA_HIP(hipMemcpyAsync(h[a], d[a], (size_t) (d[c] - d[a]) + G, hipMemcpyDeviceToHost, f.st));   // depth, conf and code are consecutive
    if (images2) {
        const uint8_t *ref = depth_ring.ptr + depth_slot_bytes * (size_t) slot;   // (sweep has checked the slot)
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
    const int step = c.sweep.step;
    if (step < 1 || c.mode < 0 || c.mode > 2 || !c.depth || !c.weight || !c.src || !c.level || !c.info16) return ALVA_ERR_ARG;
    const alva_level &L = *f.level0;
    const int gw = L.w / step, gh = L.h / step;
    const size_t G = (size_t) gw * (size_t) gh, P = (size_t) L.w * (size_t) L.h;
    if (G == 0) return ALVA_ERR_ARG;
    const bool same_grid = dense_block && dense_gw == gw && dense_gh == gh;
    if (c.mode != 1 && !same_grid) return ALVA_ERR_STATE;   // (the caller keeps track of the state it asks to warp or fill)
    const bool swept = c.mode >= 1 && c.slot >= 0;
    if (dense_cap() < G) {   // grow-only
        dense_gw = dense_gh = 0;
        const int rc = dense_block.replace(11 * ((G + 255) / 256 * 256), f.st);
        if (rc) return rc;
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
        if (swept) {
            rc = sweep(c.slot, c.calib8, c.T_rc12, c.sweep, c.rho_min, c.rho_max, (float *) d[r_d], d[r_cf], d[r_cd], info8);
            if (rc) return rc;
            c.info16[11] = info8[0];
        }
        static const double ident[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
        rc = alva_depth_fuse(f.ctx, prev ? dense_rho(in) : nullptr, prev ? dense_w(in) : nullptr, prev ? c.T_cp12 : ident, c.calib8, L.w, L.h,
                             step, swept ? (const float *) d[r_d] : nullptr, swept ? d[r_cf] : nullptr, swept ? d[r_cd] : nullptr, c.decay, c.w_max,
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
    rc = alva_depth_fill(f.ctx, dense_rho(k), dense_w(k), L.gray, L.gray_pitch, L.w, L.h, step, c.rho_ref, c.max_level, (float *) d[o_d],
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
        if (swept) ALVA_HIP(hipMemcpyAsync(h[r_d], d[r_d], (size_t) (d[r_cd] - d[r_d]) + G, hipMemcpyDeviceToHost, f.st));
        ALVA_HIP(hipMemcpy2DAsync(h[e_g], (size_t) L.w, L.gray, L.gray_pitch, (size_t) L.w, (size_t) L.h, hipMemcpyDeviceToHost, f.st));
    }
    ALVA_HIP(alva_stream_sync(f.st));
    memcpy(c.depth, h[o_d], G * 4);
    memcpy(c.level, h[o_l], G);
    memcpy(c.weight, h[o_w], G);
    memcpy(c.src, h[o_s], G);
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
    const int step = c.sweep.step;
    if (step < 1 || c.N < 4 || c.N > 256 || !c.info8 || !c.swept0) return ALVA_ERR_ARG;
    const alva_level &L = *f.level0;
    const size_t G = (size_t) (L.w / step) * (size_t) (L.h / step), V = (size_t) c.N * c.N * c.N;
    if (G == 0) return ALVA_ERR_ARG;
    int rc;
    bool zero = c.zero;
    if (!mesh.is(c.N)) {   // the exact key: N
        if ((rc = mesh.replace(c.N, 3, f.st))) return rc;
        zero = true;
    }
    if (zero) ALVA_HIP(hipMemsetAsync(mesh.block.ptr, 0, 3 * V, f.st));
    if (c.color_on) {   // the colour volume: allocated, replaced and zeroed where the distance volume is
        if (c.color_fuse && !color_thumb) return ALVA_ERR_STATE;
        bool czero = zero;
        if (!mesh_color.is(c.N)) {
            if ((rc = mesh_color.replace(c.N, 4, f.st))) return rc;
            czero = true;
        }
        if (czero) ALVA_HIP(hipMemsetAsync(mesh_color.block.ptr, 0, 4 * V, f.st));
    }
    const bool dbg = c.dbg_raw_depth || c.dbg_raw_conf || c.dbg_raw_code;
    StagePlan p;
    const size_t r_d = p.add(G * 4), r_cf = p.add(G), r_cd = p.add(G);   // the raw sweep images: on the device, and for tests on the host
    std::vector<uint8_t *> d, h;
    if ((rc = hs.carve(p, d, h))) return rc;
    int sweep8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    rc = sweep(c.slot, c.calib8, c.T_rc12, c.sweep, c.rho_min, c.rho_max, (float *) d[r_d], d[r_cf], d[r_cd], sweep8);
    if (rc) return rc;
    *c.swept0 = sweep8[0];
    rc = c.color_on && c.color_fuse
             ? alva_mesh_integrate_color(f.ctx, mesh_q(), mesh_w(), mesh_color.block.ptr, c.N, c.origin3, c.voxel, c.trunc, c.T_cw12, c.calib8, L.w,
                                         L.h, step, (const float *) d[r_d], d[r_cf], d[r_cd], color_thumb.ptr, c.cstep, c.w_max, c.info8)
             : alva_mesh_integrate(f.ctx, mesh_q(), mesh_w(), c.N, c.origin3, c.voxel, c.trunc, c.T_cw12, c.calib8, L.w, L.h, step,
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
    if (!mesh.block) return ALVA_ERR_STATE;
    if (max_vertices < 1 || max_triangles < 1 || !vertices || !normals || !triangles || !info8) return ALVA_ERR_ARG;
    const size_t vb = ((size_t) max_vertices * 12 + 255) / 256 * 256, tb = ((size_t) max_triangles * 12 + 255) / 256 * 256;
    const size_t cb = colors ? ((size_t) max_vertices * 5 + 255) / 256 * 256 : 0;   // rgba [max_vertices][4], then the codes
    int rc;
    if (mesh_out.bytes < 2 * vb + tb + cb && (rc = mesh_out.replace(2 * vb + tb + cb, f.st))) return rc;   // grow-only
    uint8_t *const out = mesh_out.ptr;
    float *d_v = (float *) out, *d_n = (float *) (out + vb);
    int *d_t = (int *) (out + 2 * vb);
    rc = alva_mesh_extract(f.ctx, mesh_q(), mesh_w(), mesh.N, origin3, voxel, min_weight, max_vertices, max_triangles, d_v, d_n, d_t, info8);
    if (rc) return rc;
    if (n_colored) *n_colored = 0;
    if (info8[0] == 0) {   // the counts are known only now: a second, exact download
        const size_t nv = (size_t) info8[1];
        if (colors && has_mesh_color()) {   // the colour volume at the vertices, where they are: on the device
            uint8_t *d_rgba = out + 2 * vb + tb, *d_code = d_rgba + (size_t) max_vertices * 4;
            for (size_t at = 0; at < nv; at += (size_t) 1 << 20) {
                const int n = (int) (nv - at < ((size_t) 1 << 20) ? nv - at : (size_t) 1 << 20);
                int cinfo[8];
                rc = alva_mesh_color_at(f.ctx, mesh_color.block.ptr, mesh.N, origin3, voxel, n, d_v + 3 * at, d_rgba + 4 * at, d_code + at, cinfo);
                if (rc) return rc;
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
    if (mesh.block) ALVA_HIP(hipMemsetAsync(mesh.block.ptr, 0, 3 * mesh.voxels(), f.st));
    if (mesh_color.block) ALVA_HIP(hipMemsetAsync(mesh_color.block.ptr, 0, 4 * mesh_color.voxels(), f.st));
    return ALVA_OK;
}

int SceneStages::mesh_shift(const int *shift3, int *info8) {
    const HipStages::Frame f = hs.frame();
    if (!mesh.block) return ALVA_ERR_STATE;
    if (!shift3 || !info8) return ALVA_ERR_ARG;
    const bool color = has_mesh_color();
    int rc;
    if (!mesh_alt.is(mesh.N) && (rc = mesh_alt.replace(mesh.N, 3, f.st))) return rc;   // the exact key: the volume's N
    if (color && !mesh_color_alt.is(mesh.N) && (rc = mesh_color_alt.replace(mesh.N, 4, f.st))) return rc;
    rc = alva_mesh_shift(f.ctx, mesh_q(), mesh_w(), color ? mesh_color.block.ptr : nullptr, mesh.N, shift3, (int16_t *) mesh_alt.block.ptr,
                         mesh_alt.block.ptr + 2 * mesh.voxels(), color ? mesh_color_alt.block.ptr : nullptr, info8);
    if (rc) return rc;
    // the stage has waited: the old blocks are no longer read.  Each pair swaps block and N together
    std::swap(mesh, mesh_alt);
    if (color) std::swap(mesh_color, mesh_color_alt);
    return ALVA_OK;
}

int SceneStages::mesh_block_digest(const int *lattice3, int min_weight, int B, std::vector<uint64_t> &digest, std::vector<int> &counts, int *nb3) {
    const HipStages::Frame f = hs.frame();
    if (!mesh.block) return ALVA_ERR_STATE;
    if (!lattice3 || !nb3) return ALVA_ERR_ARG;
    const size_t side = (size_t) mesh.N / 8 + 2, cap = side * side * side;   // the largest grid any lattice and block give
    int rc;
    if (mesh_digest_out.bytes < cap * 16 && (rc = mesh_digest_out.replace(cap * 16, f.st))) return rc;   // grow-only
    unsigned long long *d_digest = (unsigned long long *) mesh_digest_out.ptr;
    int *d_counts = (int *) (mesh_digest_out.ptr + cap * 8);
    if ((rc = alva_mesh_block_digest(f.ctx, mesh_q(), mesh_w(), mesh.N, lattice3, min_weight, B, nb3, d_digest, d_counts))) return rc;
    const size_t nb = (size_t) nb3[0] * nb3[1] * nb3[2];
    digest.resize(nb);
    counts.resize(2 * nb);
    ALVA_HIP(hipMemcpyAsync(digest.data(), d_digest, nb * 8, hipMemcpyDeviceToHost, f.st));
    ALVA_HIP(hipMemcpyAsync(counts.data(), d_counts, nb * 8, hipMemcpyDeviceToHost, f.st));
    ALVA_HIP(alva_stream_sync(f.st));
    return ALVA_OK;
}

int SceneStages::mesh_extract_blocks(const double *origin3, double voxel, const int *lattice3, int min_weight, int B, int n_sel,
                                     const int *sel_keys, int n_vertices, int n_triangles, float *vertices, float *normals, uint8_t *colors,
                                     int *triangles, int *ranges, int *info8) {
    const HipStages::Frame f = hs.frame();
    if (!mesh.block) return ALVA_ERR_STATE;
    if (n_sel < 1 || n_vertices < 1 || n_triangles < 1 || !vertices || !normals || !triangles || !ranges || !info8) return ALVA_ERR_ARG;
    const size_t vb = ((size_t) n_vertices * 12 + 255) / 256 * 256, tb = ((size_t) n_triangles * 12 + 255) / 256 * 256;
    const size_t cb = colors ? ((size_t) n_vertices * 5 + 255) / 256 * 256 : 0;   // rgba [n_vertices][4], then the codes
    int rc;
    if (mesh_out.bytes < 2 * vb + tb + cb && (rc = mesh_out.replace(2 * vb + tb + cb, f.st))) return rc;   // grow-only, mesh_extract's block
    uint8_t *const out = mesh_out.ptr;
    float *d_v = (float *) out, *d_n = (float *) (out + vb);
    int *d_t = (int *) (out + 2 * vb);
    rc = alva_mesh_extract_blocks(f.ctx, mesh_q(), mesh_w(), mesh.N, origin3, voxel, lattice3, min_weight, B, n_sel, sel_keys, n_vertices,
                                  n_triangles, d_v, d_n, d_t, ranges, info8);
    if (rc) return rc;
    if (info8[0] != 0) return ALVA_OK;
    const size_t nv = (size_t) info8[1];
    if (colors && has_mesh_color()) {   // the colour volume at the packed vertices, where they are: on the device
        uint8_t *d_rgba = out + 2 * vb + tb, *d_code = d_rgba + (size_t) n_vertices * 4;
        for (size_t at = 0; at < nv; at += (size_t) 1 << 20) {
            const int n = (int) (nv - at < ((size_t) 1 << 20) ? nv - at : (size_t) 1 << 20);
            int cinfo[8];
            rc = alva_mesh_color_at(f.ctx, mesh_color.block.ptr, mesh.N, origin3, voxel, n, d_v + 3 * at, d_rgba + 4 * at, d_code + at, cinfo);
            if (rc) return rc;
        }
        ALVA_HIP(hipMemcpyAsync(colors, d_rgba, nv * 4, hipMemcpyDeviceToHost, f.st));
    } else if (colors) memset(colors, 0, nv * 4);
    ALVA_HIP(hipMemcpyAsync(vertices, d_v, nv * 12, hipMemcpyDeviceToHost, f.st));
    ALVA_HIP(hipMemcpyAsync(normals, d_n, nv * 12, hipMemcpyDeviceToHost, f.st));
    if (info8[2] > 0) ALVA_HIP(hipMemcpyAsync(triangles, d_t, (size_t) info8[2] * 12, hipMemcpyDeviceToHost, f.st));
    ALVA_HIP(alva_stream_sync(f.st));
    return ALVA_OK;
}

int SceneStages::ray_reserve(size_t n) {   // grow-only
    if (ray_cap() >= n) return ALVA_OK;
    return ray_block.replace(RAY_BYTES * ((n + 255) / 256 * 256), hs.frame().st);
}

int SceneStages::color_frame(int cstep, bool wait, bool *pending) {
    const HipStages::Frame f = hs.frame();
    *pending = false;
    if (!f.src) return ALVA_ERR_STATE;
    const Camera &k = *f.cam;
    if (cstep < 1 || k.width / cstep < 1 || k.height / cstep < 1) return ALVA_ERR_ARG;
    const size_t exact = (size_t) (k.width / cstep) * (size_t) (k.height / cstep) * 4, bytes = (exact + 255) / 256 * 256;
    int rc;
    if (color_thumb.bytes != bytes + 256) {   // the exact key: the thumbnail's size.  Behind it, 256 bytes for the arrival counter
        if ((rc = color_thumb.replace(bytes + 256, f.st))) return rc;
        color_thumb_exact = exact;
        ALVA_HIP(hipMemsetAsync(color_thumb.ptr, 0, bytes + 256, f.st));   // (the arrival counter starts at zero)
    }
    // the launch's last workgroup publishes the word.  wait = false: the caller has a wait of its own coming on the same stream
    uint32_t *word;
    if ((rc = color_read.arm(f, wait, &word))) return rc;
    rc = alva_color_thumb_done(f.ctx, f.src, (size_t) k.width * 4, k.width, k.height, cstep, color_thumb.ptr,
                               word ? (uint32_t *) (color_thumb.ptr + bytes) : nullptr, word, color_read.seq);
    if (rc || !FrameRead::owed(f)) return rc;
    if (!wait) *pending = true;
    else if ((rc = color_read.wait(f)) == 1) {
        alva_set_error("color_frame: the thumbnail never finished");
        return ALVA_ERR_HIP;
    }
    return rc;
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
    uint8_t *B = ray_block.ptr;   // the points, the colours, the codes: 17 of the block's bytes per ray
    float *d_p = (float *) B;
    uint8_t *d_rgba = B + 12 * ray_cap(), *d_code = B + 16 * ray_cap();
    ALVA_HIP(hipMemcpyAsync(d_p, points3, (size_t) n * 12, hipMemcpyHostToDevice, f.st));   // (pageable: returns when the source has been read)
    const int rc = alva_mesh_color_at(f.ctx, mesh_color.block.ptr, mesh.N, origin3, voxel, n, d_p, d_rgba, d_code, info8);
    if (rc) return rc;
    ALVA_HIP(hipMemcpyAsync(rgba, d_rgba, (size_t) n * 4, hipMemcpyDeviceToHost, f.st));
    ALVA_HIP(hipMemcpyAsync(codes, d_code, (size_t) n, hipMemcpyDeviceToHost, f.st));
    ALVA_HIP(alva_stream_sync(f.st));
    return ALVA_OK;
}

int SceneStages::mesh_color_debug(uint8_t *thumb, uint8_t *c) {
    const HipStages::Frame f = hs.frame();
    if (thumb && color_thumb) ALVA_HIP(hipMemcpyAsync(thumb, color_thumb.ptr, color_thumb_exact, hipMemcpyDeviceToHost, f.st));
    if (c && has_mesh_color()) ALVA_HIP(hipMemcpyAsync(c, mesh_color.block.ptr, 4 * mesh.voxels(), hipMemcpyDeviceToHost, f.st));
    ALVA_HIP(alva_stream_sync(f.st));
    return ALVA_OK;
}

int SceneStages::mesh_color_drop() {
    const hipStream_t st = hs.frame().st;
    int rc;
    if ((rc = mesh_color.release(st)) || (rc = mesh_color_alt.release(st))) return rc;
    return color_thumb.release(st);
}

int SceneStages::mesh_raycast(const MeshRaycast &c) {
    const HipStages::Frame f = hs.frame();
    if (!mesh.block) return ALVA_ERR_STATE;
    const bool pixels = c.T_wc12 != nullptr, grid = pixels && !c.uv;
    if (!c.info8 || !c.origin3 || (pixels ? !c.calib8 || c.step < 1 || c.width < 1 || c.height < 1 : !c.rays6 || c.poses || c.pose_ok)) return ALVA_ERR_ARG;
    const size_t n = grid ? (size_t) (c.width / c.step) * (size_t) (c.height / c.step) : (size_t) (c.n > 0 ? c.n : 0);
    if (n < 1 || n > ((size_t) 1 << 22) || (c.pose_ok && !c.poses)) return ALVA_ERR_ARG;
    const int rrc = ray_reserve(n);
    if (rrc) return rrc;
    uint8_t *B = ray_block.ptr;
    const size_t cap = ray_cap();
    float *d_t = (float *) (B + 48 * cap), *d_p = (float *) (B + 52 * cap), *d_n = (float *) (B + 64 * cap);
    float *d_pose = (float *) (B + 76 * cap);
    uint8_t *d_code = B + 140 * cap, *d_ok = B + 141 * cap;
    // (pageable host memory: the copies return when the source has been read)
    if (!pixels) ALVA_HIP(hipMemcpyAsync(B, c.rays6, n * 48, hipMemcpyHostToDevice, f.st));
    else if (c.uv) ALVA_HIP(hipMemcpyAsync(B, c.uv, n * 8, hipMemcpyHostToDevice, f.st));
    const int rc = pixels ? alva_mesh_raycast_pixels(f.ctx, mesh_q(), mesh_w(), mesh.N, c.origin3, c.voxel, c.min_weight, c.T_wc12, c.calib8, c.width,
                                                     c.height, c.step, (int) n, c.uv ? (const float *) B : nullptr, c.t_near, c.t_far, d_t, d_p, d_n,
                                                     d_code, c.poses ? d_pose : nullptr, c.pose_ok ? d_ok : nullptr, c.info8)
                          : alva_mesh_raycast(f.ctx, mesh_q(), mesh_w(), mesh.N, c.origin3, c.voxel, c.min_weight, (int) n, (const double *) B,
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
    int rc;
    if (!light_block) {   // once
        if ((rc = light_block.allocate(LIGHT_BLOCK_BYTES))) return rc;
        ALVA_HIP(hipMemsetAsync(light_block.ptr, 0, LIGHT_BLOCK_BYTES, f.st));
    }
    const Camera &k = *f.cam;
    rc = alva_light_bin(f.ctx, f.src, (size_t) k.width * 4, k.width, k.height, camera_calib8(k).data(), R_wc9, step, light_acc());
    if (rc) return rc;
    // the bin has to have read the frame; the fuse, behind it, publishes the word when it starts (it need not have finished)
    uint32_t *word;
    if ((rc = light_read.arm(f, true, &word))) return rc;
    rc = alva_light_fuse_started(f.ctx, light_acc(), light_state(), min_pixels, w_new, w_max, light_acc_last(), word, light_read.seq);
    if (rc || !FrameRead::owed(f)) return rc;
    if ((rc = light_read.wait(f)) == 1) {
        alva_set_error("light_frame: the fuse never started");
        return ALVA_ERR_HIP;
    }
    return rc;
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
    if (light_block) ALVA_HIP(hipMemsetAsync(light_block.ptr, 0, LIGHT_BLOCK_BYTES, f.st));
    return ALVA_OK;
}

int SceneStages::image_describe(const uint8_t *gray, int width, int height, size_t pitch, int nlevels, float *xy, uint8_t *desc, int *count) {
    const HipStages::Frame f = hs.frame();
    *count = 0;
    constexpr int CAP = ALVA_IMAGE_QUERY_CAP;
    alva_orb *orb = nullptr;
    const size_t img_bytes = ((size_t) width * height + 255) / 256 * 256;
    int rc = alva_orb_create(f.ctx, width, height, 500, 1.2f, nlevels, 20, &orb);
    if (rc) return rc;
    int n = 0;
    std::vector<float> kp((size_t) CAP * 6);
    DeviceBlock blk;   // the picture, its keypoints, its descriptors: for this call only
    rc = [&]() -> int {
        if (blk.allocate(img_bytes + (size_t) CAP * (24 + 32))) return ALVA_ERR_NOMEM;
        alva_lane_flush();
        ALVA_HIP(hipMemcpy2DAsync(blk.ptr, (size_t) width, gray, pitch, (size_t) width, (size_t) height, hipMemcpyHostToDevice, f.st));
        float *d_kp = (float *) (blk.ptr + img_bytes);
        uint8_t *d_desc = blk.ptr + img_bytes + (size_t) CAP * 24;
        const int drc = alva_orb_detect_and_compute(f.ctx, orb, blk.ptr, (size_t) width, d_kp, d_desc, CAP, &n);
        if (drc) return drc;
        n = n < CAP ? n : CAP;
        if (n > 0) {
            ALVA_HIP(hipMemcpy(kp.data(), d_kp, (size_t) n * 24, hipMemcpyDeviceToHost));
            ALVA_HIP(hipMemcpy(desc, d_desc, (size_t) n * 32, hipMemcpyDeviceToHost));
        }
        return ALVA_OK;
    }();
    (void) alva_stream_sync(f.st);   // whatever happened: before the detector goes here, and the block when the call returns
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
    if (!img_block) {   // once
        const int rc = img_block.allocate(IMG_BLOCK_BYTES);
        if (rc) return rc;
        img_version = -1;
    }
    uint8_t *B = img_block.ptr;
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
