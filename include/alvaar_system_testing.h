/* TEST-ONLY entry points of libalvaar_hip.so -- not part of the drop-in surface (include/alvaar_system.h); a caller that replaces the
 * reference's `System` never needs this header.  Used by tests/ (through alvaar_amd/system.py: AlvaAR.set_init_pose, and
 * alvaar_amd/capi.py: TrackProbe) and by __graft_entry__.smoke(). */
#ifndef ALVAAR_SYSTEM_TESTING_H
#define ALVAAR_SYSTEM_TESTING_H
#include "alvaar_system.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The two-view initialisation (VisualFrontend::initialise, src/slam/src/visual_frontend.cpp:517-549 -> MultiViewGeometry::
 * compute5ptEssentialMatrix, multi_view_geometry.cpp:225-320) adopts this pose (Twc of the initialisation frame, unit baseline) ONCE
 * instead of its own five-point result.  Why a differential test wants that: OpenGV's forward-difference refinement of the two-view pose
 * sits at its rounding-noise floor -- ONE ulp on ONE input bearing moves the reference's own result by up to 1e-4
 * (tests/test_relpose.py::test_reference_refinement_noise_floor) -- so no second build of the algorithm reproduces that pose to 1e-5, and
 * everything downstream inherits the difference as a gauge (scale / world frame) of the map.  With both maps started from the reference's
 * pose every later frame is compared at 1e-5; WITHOUT the hook the discrete state is still identical and the poses agree to 1e-3 raw /
 * 1e-4 after Sim(3) alignment (tests/test_gpu_system.py::test_system_equals_reference_without_the_hook).  NULL disarms. */
int alva_system_debug_set_init_pose(alva_system *sys, const double *pose7);

/* The slot-wise tracking step on its own (tests/test_gpu_trackstep.py): a probe owns ONE set of stages, built as a session's are, and no
 * map layer.  alva_track_probe_frame feeds an RGBA frame (the second one makes "previous" and "current"); alva_track_probe_step runs
 * one track_begin on the caller's slot table and then track_pose_collect, and returns everything the step decided.  The probe adds
 * nothing to the step: no timeouts, no withheld answers. */
typedef struct alva_track_probe alva_track_probe;

typedef struct alva_track_probe_job {
    int n;
    const float *px;          /* [n][2]   (routes 0 and 1) */
    const uint8_t *is3d;      /* [n] */
    const double *wpt;        /* [n][3] */
    const uint16_t *carry;    /* [n]      (route 2): slot i was slot carry[i] of the previous step on this probe */
    double Tcw_q[4], Tcw_t[3];
    int use_prior, klt_levels, want_pose, do_p3p, do_random;
    int table_route;          /* 0 the caller's arrays (pinned copy + copy kernel), 1 written into the stages' own slot buffers,
                                 2 carried from the previous step's table */
} alva_track_probe_job;

typedef struct alva_track_probe_out {   /* every array is the caller's, sized for n slots */
    uint8_t *code;            /* [n] */
    float *px, *unpx;         /* [n][2] */
    double *bv;               /* [n][3] */
    int p3p_req, n_pose;
    int status;               /* -1 no solve, 0 P3P rejected, 1 refinement rejected, 2 accepted */
    double pose7_p3p[7], pose7[7];
    uint8_t *p3p_outlier, *pnp_outlier;   /* [n], the first n_pose are written */
    double *Pbv, *Puv, *Pwpt; /* [n][3] [n][2] [n][3]: the gathered correspondences, n_pose rows, read back after the pose was collected */
    int info8[8];             /* what ran: [0] table route taken  [1] copy kernel launched  [2] fused pose launch queued
                                 [3] its answer: 0 none, 1 go, 2 abort  [4] retry launch ran  [5] sequence number of the step
                                 [6] launches of the compaction kernel  [7] 0 */
} alva_track_probe_out;

/* calib8 = fx fy cx cy k1 k2 p1 p2 */
int alva_track_probe_create(int device, int width, int height, const double *calib8, alva_track_probe **out);
void alva_track_probe_destroy(alva_track_probe *probe);
int alva_track_probe_frame(alva_track_probe *probe, const uint8_t *h_rgba);
/* ALVA_ERR_STATE (with a message) when the requested table route is not available: no host-writable device memory for routes 1 and 2,
 * no previous table (or a smaller one) for route 2 */
int alva_track_probe_step(alva_track_probe *probe, const alva_track_probe_job *job, alva_track_probe_out *out);
/* The stand-alone pose solve (alva_compute_pose with the tracking step's constants) on host rows, on the probe's own context, with the
 * accepted P3P pose as well: what a step's pose is compared with.  status 0 / 1 / 2 as alva_compute_pose; masks [n] */
int alva_track_probe_solve_pose(alva_track_probe *probe, int n, const double *bv, const double *uv, const double *wpt, int do_random,
                                int *status, double *pose7_p3p, double *pose7, uint8_t *p3p_outlier, uint8_t *pnp_outlier);

#ifdef __cplusplus
}
#endif
#endif
