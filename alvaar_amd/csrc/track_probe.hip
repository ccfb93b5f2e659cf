// TEST-ONLY (include/alvaar_system_testing.h): single tracking steps through a set of stages of its own, without a map layer.  The probe
// builds its HipStages as alva_system_configure builds a session's (system.hip configure_impl), feeds frames as the frame loop does and
// calls track_begin / track_pose_collect with the caller's slot table; it reads what the step left through HipStages' read-only views
// and changes nothing in the step.
#include "common.hpp"
#include "pose_internal.hpp"
#include "stages_hip.hpp"
#include "../../include/alvaar_system_testing.h"
#include <memory>

using namespace alva_slam;

struct alva_track_probe {
    int device = 0;
    std::unique_ptr<HipStages> stages;
    Camera cam;
    int frames = 0;
    int n_prev = -1;   // slots of the last step that went through (what a carried table is carried from), -1: none
};

extern "C" int alva_track_probe_create(int device, int width, int height, const double *calib8, alva_track_probe **out) {
    ALVA_ARG(out && calib8 && width >= 64 && height >= 64 && width % 4 == 0 && calib8[0] > 0 && calib8[1] > 0);
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) {
        alva_set_error("alva_track_probe_create: no HIP device %d (this library has no CPU path)", device);
        return ALVA_ERR_HIP;
    }
    std::unique_ptr<alva_track_probe> p(new alva_track_probe());
    p->device = device;
    Camera &cam = p->cam;
    cam.width = width; cam.height = height; cam.border = 20;
    cam.fx = calib8[0]; cam.fy = calib8[1]; cam.cx = calib8[2]; cam.cy = calib8[3];
    cam.k1 = calib8[4]; cam.k2 = calib8[5]; cam.p1 = calib8[6]; cam.p2 = calib8[7];
    double invK[9];
    camera_inverse_K(cam, invK);
    std::unique_ptr<HipStages> st(new HipStages());
    st->image_width_ = width;
    st->image_height_ = height;
    int rc = st->init(device, cam, false, invK, nullptr);
    if (rc) return rc;
    if (!getenv("ALVA_NO_WARMUP")) {
        rc = st->warm_up(40);
        if (rc) return rc;
    }
    p->stages = std::move(st);
    *out = p.release();
    return ALVA_OK;
}

extern "C" void alva_track_probe_destroy(alva_track_probe *probe) { delete probe; }

extern "C" int alva_track_probe_frame(alva_track_probe *probe, const uint8_t *h_rgba) {
    ALVA_ARG(probe && h_rgba);
    int rc = probe->stages->new_frame(h_rgba);
    if (rc) return rc;
    rc = probe->stages->frame_done();
    if (rc) return rc;
    // new_frame uploads from ONE pinned staging copy, asynchronously.  In the frame loop a stage that waits (the tracker, the detector)
    // always stands between two frames; the probe has none there, so it waits itself before the next frame may overwrite the staging
    rc = alva_ctx_sync(probe->stages->frame().ctx);
    if (rc) return rc;
    probe->frames++;
    return ALVA_OK;
}

extern "C" int alva_track_probe_step(alva_track_probe *probe, const alva_track_probe_job *job, alva_track_probe_out *out) {
    ALVA_ARG(probe && job && out && job->n >= 0 && job->table_route >= 0 && job->table_route <= 2);
    const int n = job->n;
    const size_t N = (size_t) n;
    ALVA_ARG(n == 0 || (out->code && out->px && out->unpx && out->bv && out->p3p_outlier && out->pnp_outlier && out->Pbv && out->Puv && out->Pwpt));
    ALVA_ARG(n == 0 || (job->table_route == 2 ? job->carry != nullptr : job->px && job->is3d && job->wpt));
    if (probe->frames < 2) {
        alva_set_error("alva_track_probe_step: %d frames so far, a step needs a previous and a current one", probe->frames);
        return ALVA_ERR_STATE;
    }
    HipStages &st = *probe->stages;
    ALVA_HIP(hipSetDevice(probe->device));
    TrackJob J;
    J.n = n;
    memcpy(J.Tcw_q, job->Tcw_q, sizeof(J.Tcw_q));
    memcpy(J.Tcw_t, job->Tcw_t, sizeof(J.Tcw_t));
    SE3 Tcw;
    memcpy(Tcw.q, job->Tcw_q, sizeof(Tcw.q));
    memcpy(Tcw.t, job->Tcw_t, sizeof(Tcw.t));
    se3_to_pose7(se3_inverse(Tcw), J.pose7_pred);
    J.use_prior = job->use_prior;
    J.klt_levels = job->klt_levels;
    J.want_pose = job->want_pose;
    J.do_p3p = job->do_p3p;
    J.do_random = job->do_random;
    if (n > 0 && job->table_route == 0) {
        J.px = job->px;
        J.is3d = job->is3d;
        J.wpt = job->wpt;
    } else if (n > 0 && job->table_route == 1) {
        float *px = nullptr;
        uint8_t *is3d = nullptr;
        double *wpt = nullptr;
        if (!st.track_slot_buffers(n, &px, &is3d, &wpt) || !st.track_table_on_device()) {
            alva_set_error("alva_track_probe_step: no host-written device table here (track_slot_buffers)");
            return ALVA_ERR_STATE;
        }
        memcpy(px, job->px, N * 8);   // (device memory behind the bus: written, never read)
        memcpy(is3d, job->is3d, N);
        memcpy(wpt, job->wpt, N * 24);
        J.px = px;
        J.is3d = is3d;
        J.wpt = wpt;
    } else if (n > 0) {
        uint16_t *carry = probe->n_prev >= 0 ? st.track_carry_buffer(probe->n_prev, n) : nullptr;
        if (!carry) {
            alva_set_error("alva_track_probe_step: no table to carry %d slots from (the previous step left %d; track_carry_buffer)", n, probe->n_prev);
            return ALVA_ERR_STATE;
        }
        memcpy(carry, job->carry, N * 2);
        J.carry = carry;
    }
    probe->n_prev = -1;
    TrackKlt K;
    TrackPose P;
    int rc = st.track_begin(J, K);
    if (rc) return rc;
    rc = st.track_pose_collect(P);
    if (rc) return rc;
    probe->n_prev = n > 0 ? n : -1;
    if (n > 0) {
        memcpy(out->code, K.code_v, N);
        memcpy(out->px, K.px_v, N * 8);
        memcpy(out->unpx, K.unpx_v, N * 8);
        memcpy(out->bv, K.bv_v, N * 24);
    }
    out->p3p_req = K.p3p_req;
    out->n_pose = K.n_pose;
    out->status = P.status;
    memcpy(out->pose7_p3p, P.pose7_p3p, sizeof(P.pose7_p3p));
    memcpy(out->pose7, P.pose7, sizeof(P.pose7));
    const size_t np = (size_t) K.n_pose;
    if (np > N || P.p3p_outlier.size() > N || P.pnp_outlier.size() > N) {
        alva_set_error("alva_track_probe_step: %zu correspondences of %d slots", np, n);
        return ALVA_ERR_STATE;
    }
    if (!P.p3p_outlier.empty()) memcpy(out->p3p_outlier, P.p3p_outlier.data(), P.p3p_outlier.size());
    if (!P.pnp_outlier.empty()) memcpy(out->pnp_outlier, P.pnp_outlier.data(), P.pnp_outlier.size());
    const HipStages::TrackStepInfo info = st.track_step_info();
    const int info8[8] = {info.route, info.stage_in, info.pose_all_queued, info.pose_all_answer, info.retry, info.seq, info.compact_launches, 0};
    memcpy(out->info8, info8, sizeof(info8));
    if (np > 0 && info.route >= 0) {
        const double *Pbv, *Puv, *Pwpt;
        st.track_pose_rows(&Pbv, &Puv, &Pwpt);
        if (!Pbv) {
            alva_set_error("alva_track_probe_step: the step left no correspondence rows");
            return ALVA_ERR_STATE;
        }
        rc = alva_ctx_sync(st.frame().ctx);
        if (rc) return rc;
        ALVA_HIP(hipMemcpy(out->Pbv, Pbv, np * 24, hipMemcpyDeviceToHost));
        ALVA_HIP(hipMemcpy(out->Puv, Puv, np * 16, hipMemcpyDeviceToHost));
        ALVA_HIP(hipMemcpy(out->Pwpt, Pwpt, np * 24, hipMemcpyDeviceToHost));
    }
    return ALVA_OK;
}

extern "C" int alva_track_probe_solve_pose(alva_track_probe *probe, int n, const double *bv, const double *uv, const double *wpt, int do_random,
                                           int *status, double *pose7_p3p, double *pose7, uint8_t *p3p_outlier, uint8_t *pnp_outlier) {
    ALVA_ARG(probe && n >= 4 && bv && uv && wpt && status && pose7_p3p && pose7 && p3p_outlier && pnp_outlier);
    ALVA_HIP(hipSetDevice(probe->device));
    alva_ctx *ctx = probe->stages->frame().ctx;
    const Camera &k = probe->cam;
    const size_t N = (size_t) n;
    double *d = nullptr;
    ALVA_HIP(hipMalloc((void **) &d, N * 64));
    int rc = ALVA_OK;
    hipError_t e = hipMemcpy(d, bv, N * 24, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + 3 * N, uv, N * 16, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + 5 * N, wpt, N * 24, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        alva_set_error("alva_track_probe_solve_pose: %s", hipGetErrorString(e));
        rc = ALVA_ERR_HIP;
    }
    if (!rc) rc = SessionPose(k.fx, k.fy, k.cx, k.cy).enqueue(ctx, d, d + 3 * N, d + 5 * N, n, do_random);   // the solve track_begin enqueues
    for (int i = 0; i < 7; i++) pose7_p3p[i] = pose7[i] = i == 6 ? 1. : 0.;
    if (!rc) rc = alva_compute_pose_collect_p3p(ctx, pose7, pose7_p3p, p3p_outlier, pnp_outlier, status);
    (void) alva_ctx_sync(ctx);
    (void) hipFree(d);
    return rc;
}
