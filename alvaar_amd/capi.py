"""ctypes binding of include/alvaar_hip.h.  Device buffers are torch CUDA tensors."""
from __future__ import annotations

import ctypes as C
from pathlib import Path

# torch first: it ships its own ROCm runtime (torch/lib/libamdhip64.so).  Loading our library before
# torch would bind it to /opt/rocm's copy and leave two HIP runtimes in one process.
import torch  # noqa: F401  (plumbing: device memory + streams)

import os
# ALVA_LIB: another build of the same library (A/B measurements on one GPU box); the default is the in-tree build
_LIB_PATH = Path(os.environ["ALVA_LIB"]) if os.environ.get("ALVA_LIB") else Path(__file__).resolve().parent / "libalvaar_hip.so"


class AlvaError(RuntimeError):
    pass


class StageError(AlvaError):
    """a refused stage call, with the library's return code (ERR_ARG / ERR_STATE of include/alvaar_hip.h)"""
    ERR_ARG, ERR_STATE = -1, -4

    def __init__(self, rc, text):
        super().__init__(f"alvaar_hip error {rc}: {text}")
        self.rc = rc


def _load() -> C.CDLL:
    if not _LIB_PATH.exists():
        raise AlvaError(
            f"{_LIB_PATH} is missing: build it with `python -m alvaar_amd.build` "
            "(there is deliberately no CPU fallback)")
    return C.CDLL(str(_LIB_PATH))


lib = _load()

_vp, _i, _f, _d, _sz = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_size_t


class PyrLevel(C.Structure):
    _fields_ = [("width", _i), ("height", _i), ("d_gray", _vp), ("gray_pitch", _sz),
                ("d_deriv", _vp), ("deriv_pitch", _sz)]


def _sig(name, argtypes, restype=_i):
    if os.environ.get("ALVA_LIB") and not hasattr(lib, name):
        return None   # an OLDER build loaded for an A/B measurement may lack the newest entry points (the in-tree build never does)
    fn = getattr(lib, name)
    fn.argtypes = argtypes
    fn.restype = restype
    return fn


_sig("alva_last_error", [], C.c_char_p)
_sig("alva_version", [], C.c_char_p)
_sig("alva_ctx_create", [_i, _vp, _i, C.POINTER(_vp)])
_sig("alva_ctx_create_with_priority", [_i, _i, C.POINTER(_vp)])
_sig("alva_ctx_destroy", [_vp], None)
_sig("alva_ctx_sync", [_vp])
_sig("alva_rgba2gray", [_vp, _vp, _sz, _i, _i, _vp, _sz])
_sig("alva_pyramid_create", [_vp, _i, _i, _i, _i, C.POINTER(_vp)])
_sig("alva_pyramid_destroy", [_vp], None)
_sig("alva_pyramid_num_levels", [_vp])
_sig("alva_pyramid_level", [_vp, _i, C.POINTER(PyrLevel)])
_sig("alva_pyramid_build_from_gray", [_vp, _vp, _vp, _sz])
_sig("alva_pyramid_download_level", [_vp, _vp, _i, _vp, _vp])
_sig("alva_pyramid_build_from_rgba", [_vp, _vp, _vp, _sz, _vp, _sz])
_sig("alva_pyramid_build_from_rgba_batch", [_vp, _vp, _vp, _sz, _vp, _sz, _i])
_sig("alva_lk_track", [_vp, _vp, _vp, _i, _i, _f, _vp, _vp, _vp, _vp, _i])
_sig("alva_fbklt_track", [_vp, _vp, _vp, _i, _f, _f, _i, _f, _vp, _vp, _vp, _i])
_sig("alva_p3p_draw_samples", [_i, _i, _i, C.c_uint32, _vp])
_sig("alva_p3p_lmeds", [_vp, _vp, _vp, _i, _i, _f, _i, C.c_uint32, _f, _f, _vp, _vp, _vp, _vp, _vp])


class P3pHypProblem(C.Structure):
    """alva_p3p_hyp_problem (include/alvaar_hip.h)"""
    _fields_ = [("d_bearings", _vp), ("d_wpts", _vp), ("h_samples", _vp), ("n", _i), ("H", _i), ("max_iters", _i),
                ("h_models", _vp), ("h_valid", _vp), ("h_penalty", _vp), ("h_masks", _vp), ("h_inlier", _vp),
                ("best", _i), ("n_valid_used", _i), ("n_inliers", _i), ("have_model", _i), ("counter_after", _i), ("model", C.c_double * 12)]


_sig("alva_p3p_hypotheses", [_vp, _vp, _i, _f, _f, _f, _i])
_sig("alva_pnp_refine", [_vp, _vp, _vp, _i, _vp, _i, _f, _i, _i, _f, _f, _f, _f, _vp, _vp, _vp, _vp])
_sig("alva_local_ba", [_vp, _i, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _d, _d, _vp, _vp, _vp, _vp])
_sig("alva_detect_grid", [_vp, _vp, _sz, _i, _i, _i, _vp, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp])


class DetectPending(C.Structure):
    _fields_ = [("h_cnt", _vp), ("n_cells", _i), ("reserved", _i)]


_sig("alva_detect_grid_enqueue", [_vp, _vp, _sz, _i, _i, _i, _vp, _i, _i, _i, _i, _i, _d, _vp, _i, C.POINTER(DetectPending)])
_sig("alva_detect_grid_collect", [_vp, C.POINTER(DetectPending), C.POINTER(_d), C.POINTER(_i)])
_sig("alva_detect_grid_debug_eig", [_vp, _i, _i, _vp])
_sig("alva_fast", [_vp, _vp, _sz, _i, _i, _i, _vp, _vp, _i, _vp])
_sig("alva_orb_create", [_vp, _i, _i, _i, _f, _i, _i, C.POINTER(_vp)])
_sig("alva_orb_destroy", [_vp], None)
_sig("alva_orb_detect_and_compute", [_vp, _vp, _vp, _sz, _vp, _vp, _i, _vp])
_sig("alva_ctx_wait", [_vp, _vp])
_sig("alva_prof_enable", [_i])
_sig("alva_prof_report", [C.c_char_p, _sz])
_sig("alva_orb_collect", [_vp, _vp, _vp])
_sig("alva_orb_debug_level", [_vp, _vp, _i, _i, _vp, _sz, _vp, _vp])
_sig("alva_match_to_map_records", [_vp, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _f, _f, _vp])
_sig("alva_match_to_map", [_vp, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _f, _f, _vp])
_sig("alva_match_to_map_flags", [_vp, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _f, _f, _vp])
_sig("alva_undistort_points", [_vp, _vp, _i] + [C.c_double] * 8 + [_vp])
_sig("alva_project_dist", [_vp, _vp, _i] + [C.c_double] * 8 + [_vp])
_sig("alva_clahe", [_vp, _vp, _sz, _i, _i, C.c_double, _i, _i, _vp, _sz])
_sig("alva_triangulate", [_vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, C.c_double, C.c_double, C.c_double, C.c_double, _f, _vp, _vp, _vp, _vp, _vp])
_sig("alva_frontend_create", [_i, _i, _i, _i, _i, C.POINTER(_vp)])
_sig("alva_frontend_destroy", [_vp], None)
_sig("alva_frontend_track", [_vp, _vp, _sz, _vp, _i, _vp, _vp, _vp, _i, _f, _f, _f, _f, _vp, _vp, _vp])
_sig("alva_frontend_track_ahead", [_vp, _vp, _sz, _vp, _vp, _i, _vp, _vp, _vp, _i, _f, _f, _f, _f, _vp, _vp, _vp])
_sig("alva_frontend_results", [_vp] + [C.POINTER(_vp)] * 6)
_sig("alva_frontend_sync", [_vp])
_sig("alva_frontend_run_many", [_vp, _i, _i, _i, _vp, _i, _sz, _vp, _i, _vp, _vp, _vp, _i, _f, _f, _f, _f, _vp, _vp])
_sig("alva_fbklt_track_batch", [_vp, _vp, _vp, _i, _i, _f, _f, _i, _f, _vp, _vp, _vp, _vp, _i])
_sig("alva_track_batch_create", [_i, _i, _i, _i, _i, _i, C.POINTER(_vp)])
_sig("alva_track_batch_destroy", [_vp], None)
_sig("alva_track_batch_step", [_vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _vp, _vp])
_sig("alva_track_batch_results", [_vp, _i, C.POINTER(_vp), C.POINTER(_vp)])
_sig("alva_track_batch_ctx", [_vp], _vp)
_sig("alva_track_batch_stats", [_vp, _vp, _vp])
_sig("alva_track_batch_enable_detector", [_vp, _i])
_sig("alva_track_batch_step_detect", [_vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _vp, _vp, _vp])
_sig("alva_track_batch_detections", [_vp, _i] + [C.POINTER(_vp)] * 4)
_sig("alva_orb_detect_and_compute_batch", [_vp, _vp, _i, _vp, _sz, _vp, _vp, _i])
_sig("alva_orb_collect_batch", [_vp, _vp, _i, _vp])
_sig("alva_orb_device_count", [_vp], _vp)
_sig("alva_orb_ambiguous_rotations", [_vp, _i])
_sig("alva_bf_match_hamming_batch", [_vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i])
_sig("alva_track_batch_set_klt_lanes", [_vp, _i])
_sig("alva_compute_pose_enqueue", [_vp, _vp, _vp, _vp, _i, _i, _f, _i, C.c_uint32, _i, _f, _f, _f, _f, _f])
_sig("alva_compute_pose_collect", [_vp, _vp, _vp, _vp, _vp])
_sig("alva_compute_pose", [_vp, _vp, _vp, _vp, _i, _i, _f, _i, C.c_uint32, _i, _f, _f, _f, _f, _f, _vp, _vp, _vp, _vp])
_sig("alva_describe", [_vp, _vp, _sz, _i, _i, _vp, _i, _vp, _vp])
_sig("alva_orb_blur", [_vp, _vp, _sz, _i, _i, _vp, _sz])
_sig("alva_bf_match_hamming", [_vp, _vp, _i, _vp, _i, _vp, _vp])
_sig("alva_find_plane", [_vp, _vp, _i, _vp, _i, _i, C.c_uint32, _vp, _vp, _vp])
_sig("alva_find_plane_trace", [_vp, _vp, _i, _vp, _i, _i, C.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp])
_sig("alva_hit_test", [_vp, _vp, _i, _vp, _vp, _i, _vp, _f, _i, C.c_uint32, _vp, _vp, _vp, _vp])
_sig("alva_detect_planes", [_vp, _vp, _i, _vp, C.c_double, _i, _i, _i, C.c_uint32, _vp, _vp, _vp, _vp, _vp])
_sig("alva_track_planes", [_vp, _vp, _i, _vp, C.c_double, _i, _i, _i, C.c_uint32, _vp, _i, _vp, _vp, _vp, _vp, _vp])
_sig("alva_plane_outlines", [_vp, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp])
_sig("alva_anchor_attach", [_vp, _vp, _i, _i, _vp, _i, _vp, _vp, _vp])
_sig("alva_anchor_update", [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp])
_sig("alva_depth_sweep", [_vp, _vp, _vp, _sz, _i, _i, _vp, _vp, _i, _i, _d, _d, _i, _i, _i, _vp, _vp, _vp, _vp, _vp])
_sig("alva_depth_fuse", [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _i, _i, _d, _vp, _vp, _vp, _vp])
_sig("alva_depth_fill", [_vp, _vp, _vp, _vp, _sz, _i, _i, _i, _d, _i, _vp, _vp, _vp])
_sig("alva_mesh_integrate", [_vp, _vp, _vp, _i, _vp, _d, _d, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _i, _vp])
_sig("alva_mesh_extract", [_vp, _vp, _vp, _i, _vp, _d, _i, _i, _i, _vp, _vp, _vp, _vp])
_sig("alva_mesh_raycast", [_vp, _vp, _vp, _i, _vp, _d, _i, _i, _vp, _d, _d, _vp, _vp, _vp, _vp, _vp])
_sig("alva_mesh_raycast_pixels", [_vp, _vp, _vp, _i, _vp, _d, _i, _vp, _vp, _i, _i, _i, _i, _vp, _d, _d, _vp, _vp, _vp, _vp, _vp, _vp, _vp])
_sig("alva_color_thumb", [_vp, _vp, _sz, _i, _i, _i, _vp])
_sig("alva_mesh_integrate_color", [_vp, _vp, _vp, _vp, _i, _vp, _d, _d, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _vp])
_sig("alva_mesh_color_at", [_vp, _vp, _i, _vp, _d, _i, _vp, _vp, _vp, _vp])
_sig("alva_mesh_shift", [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp])
_sig("alva_mesh_block_digest", [_vp, _vp, _vp, _i, _vp, _i, _i, _vp, _vp, _vp])
_sig("alva_mesh_extract_blocks", [_vp, _vp, _vp, _i, _vp, _d, _vp, _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp])
_sig("alva_light_bin", [_vp, _vp, _sz, _i, _i, _vp, _vp, _i, _vp])
_sig("alva_light_fuse", [_vp, _vp, _vp, _i, _i, _i, _vp])
_sig("alva_light_estimate", [_vp, _vp, _vp, _vp, _vp, _vp, _vp])
LIGHT_CELLS, LIGHT_ACC_WORDS, LIGHT_STATE_BYTES = 384, 1544, 5024   # ALVA_LIGHT_* of include/alvaar_hip.h
_sig("alva_image_match", [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _vp, _vp, _vp])
_sig("alva_image_homography", [_vp, _i, _vp, _vp, _vp, _i, _i, _vp, _i, _f, _i, C.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp])
IMAGE_MAX, IMAGE_QUERY_CAP, IMAGE_TRAIN_CAP = 8, 512, 2048   # ALVA_IMAGE_* of include/alvaar_hip.h
_sig("alva_relpose_draw_samples", [_i, _i, _i, C.c_uint32, _vp])
_sig("alva_relpose_hypotheses", [_vp, _vp, _vp, _i, _vp, _i, _f, _f, _f, _vp, _vp])
_sig("alva_reloc_match", [_vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _f, _vp, _vp, _vp, _vp, _vp])
_sig("alva_compute_5pt_essential", [_vp, _vp, _vp, _i, _i, _f, _i, _i, C.c_uint32, _f, _f, _vp, _vp, _vp, _vp, _vp])


class RelposeInfo(C.Structure):
    _fields_ = [("iterations", _i), ("n_inliers", _i), ("draws", _i), ("lm_iterations", _i), ("lm_status", _i), ("lm_nfev", _i),
                ("ransac_model", C.c_double * 12)]


def check(rc: int) -> None:
    if rc != 0:
        raise AlvaError(f"alvaar_hip error {rc}: {lib.alva_last_error().decode()}")


def _ptr(t) -> int:
    return 0 if t is None else t.data_ptr()


def _rgba_pitch(*frames) -> int:
    """the row pitch of [h,w,4] uint8 frames (any may be None) that one call passes under ONE pitch argument: views with padded rows or
    inside a larger buffer are fine, a pixel is 4 adjacent bytes, and all frames share the row stride"""
    frames = [f for f in frames if f is not None]
    for f in frames:
        assert f.dtype == torch.uint8 and f.dim() == 3 and f.shape[2] == 4 and f.stride(1) == 4 and f.stride(2) == 1
        assert f.shape == frames[0].shape and f.stride(0) == frames[0].stride(0), "frames of one call share one geometry and row pitch"
    return frames[0].stride(0)


def _gray_pitch(*grays) -> int:
    """the same for [h,w] uint8 images (0 when there is none)"""
    grays = [g for g in grays if g is not None]
    for g in grays:
        assert g.dtype == torch.uint8 and g.dim() == 2 and g.stride(1) == 1
        assert g.shape == grays[0].shape and g.stride(0) == grays[0].stride(0), "images of one call share one geometry and row pitch"
    return grays[0].stride(0) if grays else 0


class Context:
    """One HIP stream on one device (alva_ctx).  By default enqueues on torch's current stream so
    torch.cuda.synchronize()/Events see the work."""

    def __init__(self, device: int = 0, stream: int | None = None, own_stream: bool = False):
        if not torch.cuda.is_available():
            raise AlvaError("no HIP device visible: the alvaar_amd hot path has no CPU fallback")
        self.device = device
        if stream is None and not own_stream:
            stream = torch.cuda.current_stream(device).cuda_stream
        h = _vp()
        check(lib.alva_ctx_create(device, _vp(stream or 0), 1 if own_stream else 0, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None) and lib is not None:   # `lib` is already gone at interpreter shutdown
            lib.alva_ctx_destroy(self.h)
            self.h = None

    __del__ = close

    def sync(self):
        check(lib.alva_ctx_sync(self.h))

    # a2
    def rgba2gray(self, rgba, out=None):
        """rgba [h,w,4] uint8 and out [h,w] uint8 may be views with padded rows (alvaar_hip.h states the pitch and alignment rules)"""
        h, w, c = rgba.shape
        pitch = _rgba_pitch(rgba)
        if out is None:
            out = torch.empty((h, w), dtype=torch.uint8, device=rgba.device)
        assert tuple(out.shape) == (h, w)
        check(lib.alva_rgba2gray(self.h, _ptr(rgba), pitch, w, h, _ptr(out), _gray_pitch(out)))
        return out


    # a4
    def lk_track(self, prev: "Pyramid", nxt: "Pyramid", pts, init, num_levels=3, max_iters=30, eps=0.01):
        n = pts.shape[0]
        out = init.clone().contiguous()
        status = torch.empty(n, dtype=torch.uint8, device=pts.device)
        err = torch.empty(n, dtype=torch.float32, device=pts.device)
        check(lib.alva_lk_track(self.h, prev.h, nxt.h, num_levels, max_iters, eps, _ptr(pts), _ptr(out), _ptr(status), _ptr(err), n))
        return out, status, err

    def fbklt_track(self, prev: "Pyramid", curr: "Pyramid", pts, prior, num_levels=3, err_thresh=30.0, fb_dist=0.5,
                    max_iters=30, eps=0.01):
        """FeatureTracker::fbKltTracking: returns (updated prior [n,2], status [n] u8)."""
        n = pts.shape[0]
        out = prior.clone().contiguous()
        status = torch.empty(n, dtype=torch.uint8, device=pts.device)
        check(lib.alva_fbklt_track(self.h, prev.h, curr.h, num_levels, err_thresh, fb_dist, max_iters, eps, _ptr(pts), _ptr(out),
                                   _ptr(status), n))
        return out, status

    # a8
    def p3p_lmeds(self, bearings, wpts, max_iters=100, err=3.0, fx=579.4, fy=579.4, do_random=False, seed=12345):
        """MultiViewGeometry::p3pRansac: returns (ok, R [3,3] numpy, t [3] numpy, outlier indices numpy)."""
        import numpy as np
        n = bearings.shape[0]
        assert bearings.dtype == torch.float64 and wpts.dtype == torch.float64
        R = np.zeros((3, 3))
        t = np.zeros(3)
        out = np.zeros(max(n, 1), np.int32)
        nout = C.c_int(0)
        ok = C.c_int(0)
        check(lib.alva_p3p_lmeds(self.h, _ptr(bearings), _ptr(wpts), n, max_iters, err, int(do_random), seed, fx, fy,
                                 R.ctypes.data, t.ctypes.data, out.ctypes.data, C.byref(nout), C.byref(ok)))
        return bool(ok.value), R, t, out[:nout.value].copy()

    def p3p_hypotheses(self, problems, err=3.0, fx=579.4, fy=579.4, route=0):
        """The P3P-LMedS hypothesis stage on caller-supplied samples (alva_p3p_hypotheses).  `problems`: dicts with bv / wpt (device
        float64 [n,3]), samples (int32 [H,4]), max_iters and optionally n (default: bv's rows).  route 0: the single-problem launch,
        one problem after the other; route 1: all problems in one batch.  Returns one dict per problem: models [H,12], valid [H],
        penalty [H] (+inf where there is no model), masks [H, ceil(n/64)] uint64 (route 0; None on route 1), inlier [n] and the
        selection's best, n_valid_used, have_model, n_inliers, model [12], counter_after."""
        import numpy as np
        arr = (P3pHypProblem * max(len(problems), 1))()
        keep = []
        for q, pb in zip(arr, problems):
            s = np.ascontiguousarray(pb["samples"], np.int32).reshape(-1, 4)
            n = int(pb["n"]) if "n" in pb else int(pb["bv"].shape[0])
            H, words = s.shape[0], (max(n, 0) + 63) // 64
            out = dict(models=np.zeros((H, 12)), valid=np.zeros(H, np.int32), penalty=np.zeros(H),
                       masks=np.zeros((H, words), np.uint64) if route == 0 else None, inlier=np.zeros(max(n, 1), np.uint8))
            for t in (pb["bv"], pb["wpt"]):
                assert t is None or (t.dtype == torch.float64 and t.is_contiguous())
            q.d_bearings, q.d_wpts, q.h_samples = _ptr(pb["bv"]), _ptr(pb["wpt"]), s.ctypes.data if H else None
            q.n, q.H, q.max_iters = n, H, int(pb["max_iters"])
            q.h_models, q.h_valid, q.h_penalty = out["models"].ctypes.data, out["valid"].ctypes.data, out["penalty"].ctypes.data
            q.h_masks = None if out["masks"] is None else out["masks"].ctypes.data
            q.h_inlier = out["inlier"].ctypes.data
            keep.append((s, out, n))
        check(lib.alva_p3p_hypotheses(self.h, C.addressof(arr), len(problems), float(err), float(fx), float(fy), int(route)))
        res = []
        for q, (s, out, n) in zip(arr, keep):
            out["inlier"] = out["inlier"][:n]
            out.update(best=q.best, n_valid_used=q.n_valid_used, have_model=q.have_model, n_inliers=q.n_inliers,
                       model=np.array(q.model), counter_after=q.counter_after)
            res.append(out)
        return res

    # f2b
    def compute_5pt_essential(self, bv1, bv2, max_iters=100, err=3.0, optimize=True, fx=579.4, fy=579.4, do_random=False, seed=12345):
        """MultiViewGeometry::compute5ptEssentialMatrix: returns (ok, Rwc [3,3], twc [3], inlier mask [n] bool, RelposeInfo)."""
        import numpy as np
        n = bv1.shape[0]
        assert bv1.dtype == torch.float64 and bv2.dtype == torch.float64 and bv2.shape[0] == n
        R = np.zeros((3, 3))
        t = np.zeros(3)
        mask = np.zeros(max(n, 1), np.uint8)
        info = RelposeInfo()
        ok = C.c_int(0)
        check(lib.alva_compute_5pt_essential(self.h, _ptr(bv1), _ptr(bv2), n, int(max_iters), float(err), int(optimize), int(do_random),
                                             int(seed), float(fx), float(fy), R.ctypes.data, t.ctypes.data, mask.ctypes.data,
                                             C.addressof(info), C.addressof(ok)))
        return bool(ok.value), R, t, mask[:n].astype(bool), info

    # f3
    def find_plane(self, points, pose7, num_iterations=250, samples3=None, do_random=False, seed=12345, want_trace=False):
        """The intended System::processPlane: returns the plane pose [16] float32 or None.  With want_trace (alva_find_plane_trace; for
        tests): (pose or None, dict(scores [iters] float32, planes [iters,4] float32, inlier [n] uint8, best, n_inliers, kth,
        best_score float32, moments [13] float64))."""
        import numpy as np
        assert points.dtype == torch.float64
        pose = np.ascontiguousarray(pose7, np.float64)
        out = np.zeros(16, np.float32)
        found = C.c_int(0)
        s = None if samples3 is None else np.ascontiguousarray(samples3, np.int32)
        n, iters = points.shape[0], int(num_iterations if s is None else len(s))
        args = (self.h, _ptr(points) if n else None, n, pose.ctypes.data, iters, int(do_random), int(seed), None if s is None else s.ctypes.data,
                out.ctypes.data, C.addressof(found))
        if not want_trace:
            check(lib.alva_find_plane(*args))
            return out if found.value else None
        scores, planes = np.zeros(max(iters, 1), np.float32), np.zeros((max(iters, 1), 4), np.float32)
        inlier, info, best_score, mom = np.zeros(max(n, 1), np.uint8), np.zeros(4, np.int32), np.zeros(1, np.float32), np.zeros(13, np.float64)
        check(lib.alva_find_plane_trace(*args, scores.ctypes.data, planes.ctypes.data, inlier.ctypes.data, info.ctypes.data,
                                        best_score.ctypes.data, mom.ctypes.data))
        trace = dict(scores=scores[:iters], planes=planes[:iters], inlier=inlier[:n], best=int(info[0]), n_inliers=int(info[1]),
                     kth=int(info[2]), best_score=best_score[0], moments=mom)
        return (out if found.value else None), trace

    def hit_test(self, points, pose7, calib8, uv, radius_px=40, num_iterations=64, seed=12345, rand3=None, want_moments=False):
        """alva_hit_test: points [n,3] float64 on the device, pose7 = Twc (t, q = x y z w), calib8 = fx fy cx cy k1 k2 p1 p2, uv [r,2]
        taps in raw pixels; rand3 [iterations,3] uint32 replaces the hashed sample words.  Returns (poses [r,16] float32 -- rows of
        rays whose code is not 0 stay zero --, info [r,8] int32) and, with want_moments, the inlier moments [r,10] float64."""
        import numpy as np
        if not hasattr(lib, "alva_hit_test"):   # (an older build loaded through ALVA_LIB for an A/B measurement)
            raise AlvaError("this build of the library has no alva_hit_test")
        assert points.dtype == torch.float64 and points.is_contiguous()
        pose = np.ascontiguousarray(pose7, np.float64)
        calib = np.ascontiguousarray(calib8, np.float64)
        taps = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
        assert pose.size == 7 and calib.size == 8
        r = taps.shape[0]
        words = None if rand3 is None else np.ascontiguousarray(rand3, np.uint32).reshape(-1, 3)
        poses = np.zeros((max(r, 1), 16), np.float32)
        info = np.zeros((max(r, 1), 8), np.int32)
        mom = np.zeros((max(r, 1), 10), np.float64) if want_moments else None
        check(lib.alva_hit_test(self.h, _ptr(points) if points.shape[0] else None, points.shape[0], pose.ctypes.data, calib.ctypes.data, r,
                                taps.ctypes.data, float(radius_px), int(num_iterations if words is None else len(words)), int(seed),
                                None if words is None else words.ctypes.data, poses.ctypes.data, info.ctypes.data,
                                None if mom is None else mom.ctypes.data))
        return (poses[:r], info[:r], mom[:r]) if want_moments else (poses[:r], info[:r])

    def depth_sweep(self, cur, ref, calib8, T_rc12, rho_min, rho_max, step=4, num_hyp=64, patch_radius=2, min_texture=4, min_conf=96,
                    width=None, want_best=False):
        """alva_depth_sweep: cur and ref [h,w] uint8 on the device (any row stride, the same for both; `width` narrows the image to the
        first `width` columns), calib8 = fx fy cx cy k1 k2 p1 p2, T_rc12 = R_rc row-major then t_rc (X_ref = R_rc X_cur + t_rc).  Returns
        (depth [gh,gw] float32, conf [gh,gw] uint8, code [gh,gw] uint8, info [8] int32) as numpy arrays and, with want_best, {kb, best,
        second, T} [gh,gw,4] int32."""
        import numpy as np
        assert cur.dtype == torch.uint8 and ref.dtype == torch.uint8 and cur.dim() == 2 and cur.shape == ref.shape
        assert cur.stride(1) == 1 and ref.stride(1) == 1 and cur.stride(0) == ref.stride(0)
        h, w = int(cur.shape[0]), int(cur.shape[1] if width is None else width)
        calib = np.ascontiguousarray(calib8, np.float64)
        T = np.ascontiguousarray(T_rc12, np.float64).reshape(-1)
        assert calib.size == 8 and T.size == 12 and w <= cur.shape[1]
        step = int(step)
        gw, gh = (w // step, h // step) if 1 <= step <= 16 else (1, 1)
        n = max(gw * gh, 1)
        depth = torch.empty(n, dtype=torch.float32, device=cur.device)
        conf = torch.empty(n, dtype=torch.uint8, device=cur.device)
        code = torch.empty(n, dtype=torch.uint8, device=cur.device)
        best = torch.empty(4 * n, dtype=torch.int32, device=cur.device) if want_best else None
        info = np.zeros(8, np.int32)
        check(lib.alva_depth_sweep(self.h, _ptr(cur), _ptr(ref), cur.stride(0), w, h, calib.ctypes.data, T.ctypes.data, step, int(num_hyp),
                                   float(rho_min), float(rho_max), int(patch_radius), int(min_texture), int(min_conf), _ptr(depth), _ptr(conf),
                                   _ptr(code), info.ctypes.data, _ptr(best)))
        out = (depth.cpu().numpy().reshape(gh, gw), conf.cpu().numpy().reshape(gh, gw), code.cpu().numpy().reshape(gh, gw), info)
        return out + (best.cpu().numpy().reshape(gh, gw, 4),) if want_best else out

    def depth_fuse(self, prev, T_cp12, calib8, width, height, step, meas, decay=230, w_max=128, rel_tol=0.05):
        """alva_depth_fuse: prev = (rho [gh,gw] float32, w [gh,gw] uint8) on the device or None, meas = (depth float32, conf uint8, code
        uint8), each [gh,gw] on the device, or None; T_cp12 = R_cp row-major then t_cp (X_cur = R_cp X_prev + t_cp).  Returns (rho
        float32, w uint8, src uint8, each [gh,gw], info [8] int32) as numpy arrays."""
        import numpy as np
        step = int(step)
        gw, gh = (int(width) // step, int(height) // step) if 1 <= step <= 16 else (1, 1)
        n = max(gw * gh, 1)
        calib = np.ascontiguousarray(calib8, np.float64)
        T = np.ascontiguousarray(T_cp12, np.float64).reshape(-1)
        assert calib.size == 8 and T.size == 12
        for group, types in ((prev, (torch.float32, torch.uint8)), (meas, (torch.float32, torch.uint8, torch.uint8))):
            if group is not None:
                assert len(group) == len(types)
                for a, ty in zip(group, types):
                    assert a.dtype == ty and a.is_contiguous() and a.numel() >= n
        dev = (prev or meas or (None,))[0]
        dev = "cuda" if dev is None else dev.device
        rho = torch.empty(n, dtype=torch.float32, device=dev)
        w = torch.empty(n, dtype=torch.uint8, device=dev)
        src = torch.empty(n, dtype=torch.uint8, device=dev)
        info = np.zeros(8, np.int32)
        pr, pw = (None, None) if prev is None else prev
        md, mc, mk = (None, None, None) if meas is None else meas
        check(lib.alva_depth_fuse(self.h, _ptr(pr), _ptr(pw), T.ctypes.data, calib.ctypes.data, int(width), int(height), step, _ptr(md), _ptr(mc),
                                  _ptr(mk), int(decay), int(w_max), float(rel_tol), _ptr(rho), _ptr(w), _ptr(src), info.ctypes.data))
        return rho.cpu().numpy().reshape(gh, gw), w.cpu().numpy().reshape(gh, gw), src.cpu().numpy().reshape(gh, gw), info

    def depth_fill(self, rho, w, cur, step, rho_ref, max_level=5, width=None):
        """alva_depth_fill: the state rho [gh,gw] float32 and w [gh,gw] uint8 and the gray image cur [h,w] uint8 on the device (any row
        stride; `width` narrows the image to its first `width` columns).  Returns (depth [gh,gw] float32, level [gh,gw] uint8, info [4]
        int32) as numpy arrays."""
        import numpy as np
        assert cur.dtype == torch.uint8 and cur.dim() == 2 and cur.stride(1) == 1
        assert rho.dtype == torch.float32 and w.dtype == torch.uint8 and rho.is_contiguous() and w.is_contiguous()
        h, wd = int(cur.shape[0]), int(cur.shape[1] if width is None else width)
        assert wd <= cur.shape[1]
        step = int(step)
        gw, gh = (wd // step, h // step) if 1 <= step <= 16 else (1, 1)
        n = max(gw * gh, 1)
        assert rho.numel() >= n and w.numel() >= n
        depth = torch.empty(n, dtype=torch.float32, device=cur.device)
        level = torch.empty(n, dtype=torch.uint8, device=cur.device)
        info = np.zeros(4, np.int32)
        check(lib.alva_depth_fill(self.h, _ptr(rho), _ptr(w), _ptr(cur), cur.stride(0), wd, h, step, float(rho_ref), int(max_level), _ptr(depth),
                                  _ptr(level), info.ctypes.data))
        return depth.cpu().numpy().reshape(gh, gw), level.cpu().numpy().reshape(gh, gw), info

    @staticmethod
    def _mesh_volume(q, w):
        assert q.dtype == torch.int16 and w.dtype == torch.uint8 and q.is_contiguous() and w.is_contiguous()
        n = int(q.shape[0]) if q.dim() == 3 else 0
        assert q.dim() == 3 and tuple(q.shape) == (n, n, n) and tuple(w.shape) == (n, n, n) and q.device == w.device
        return n

    def mesh_integrate(self, q, w, origin3, voxel, trunc, T_cw12, calib8, width, height, step, meas, w_max=128):
        """alva_mesh_integrate: the volume q [N,N,N] int16 and w [N,N,N] uint8 on the device, updated IN PLACE; origin3 the world
        position of its minimum corner, T_cw12 = R_cw row-major then t_cw (X_cam = R_cw X_world + t_cw), meas = (depth float32, conf
        uint8, code uint8), each [gh,gw] on the device.  Returns info [8] int32."""
        import numpy as np
        n = self._mesh_volume(q, w)
        step = int(step)
        gw, gh = (int(width) // step, int(height) // step) if 1 <= step <= 16 else (1, 1)
        o = np.ascontiguousarray(origin3, np.float64).reshape(-1)
        T = np.ascontiguousarray(T_cw12, np.float64).reshape(-1)
        calib = np.ascontiguousarray(calib8, np.float64)
        assert o.size == 3 and T.size == 12 and calib.size == 8 and len(meas) == 3
        for a, ty in zip(meas, (torch.float32, torch.uint8, torch.uint8)):
            assert a.dtype == ty and a.is_contiguous() and a.numel() >= max(gw * gh, 1) and a.device == q.device
        info = np.zeros(8, np.int32)
        check(lib.alva_mesh_integrate(self.h, _ptr(q), _ptr(w), n, o.ctypes.data, float(voxel), float(trunc), T.ctypes.data, calib.ctypes.data,
                                      int(width), int(height), step, _ptr(meas[0]), _ptr(meas[1]), _ptr(meas[2]), int(w_max), info.ctypes.data))
        return info

    def mesh_extract(self, q, w, origin3, voxel, min_weight, max_vertices, max_triangles):
        """alva_mesh_extract: the volume q [N,N,N] int16 and w [N,N,N] uint8 on the device.  Returns (vertices [nv,3] float32, normals
        [nv,3] float32, triangles [nt,3] int32, info [8] int32) as numpy arrays; nv = nt = 0 unless info[0] == 0."""
        import numpy as np
        n = self._mesh_volume(q, w)
        o = np.ascontiguousarray(origin3, np.float64).reshape(-1)
        assert o.size == 3
        mv, mt = max(int(max_vertices), 1), max(int(max_triangles), 1)
        vertices = torch.empty((mv, 3), dtype=torch.float32, device=q.device)
        normals = torch.empty((mv, 3), dtype=torch.float32, device=q.device)
        triangles = torch.empty((mt, 3), dtype=torch.int32, device=q.device)
        info = np.zeros(8, np.int32)
        check(lib.alva_mesh_extract(self.h, _ptr(q), _ptr(w), n, o.ctypes.data, float(voxel), int(min_weight), int(max_vertices),
                                    int(max_triangles), _ptr(vertices), _ptr(normals), _ptr(triangles), info.ctypes.data))
        nv, nt = (int(info[1]), int(info[2])) if info[0] == 0 else (0, 0)
        return vertices[:nv].cpu().numpy(), normals[:nv].cpu().numpy(), triangles[:nt].cpu().numpy(), info

    @staticmethod
    def _raycast_outputs(n, device, pose):
        out = dict(t=torch.empty(n, dtype=torch.float32, device=device), point=torch.empty((n, 3), dtype=torch.float32, device=device),
                   normal=torch.empty((n, 3), dtype=torch.float32, device=device), code=torch.empty(n, dtype=torch.uint8, device=device))
        if pose:
            out.update(pose=torch.empty((n, 16), dtype=torch.float32, device=device), pose_ok=torch.empty(n, dtype=torch.uint8, device=device))
        return out

    def mesh_raycast(self, q, w, origin3, voxel, min_weight, rays6, t_near=0.0, t_far=float("inf")):
        """alva_mesh_raycast: the volume as for mesh_extract, rays6 [n,6] float64 on the device (origin, then direction, in world
        coordinates).  Returns a dict of numpy arrays: t [n] float32, point and normal [n,3] float32, code [n] uint8, info [8] int32."""
        import numpy as np
        n_vol = self._mesh_volume(q, w)
        o = np.ascontiguousarray(origin3, np.float64).reshape(-1)
        assert o.size == 3 and rays6.dtype == torch.float64 and rays6.is_contiguous() and rays6.dim() == 2 and rays6.shape[1] == 6
        n = int(rays6.shape[0])
        out = self._raycast_outputs(max(n, 1), q.device, False)
        info = np.zeros(8, np.int32)
        check(lib.alva_mesh_raycast(self.h, _ptr(q), _ptr(w), n_vol, o.ctypes.data, float(voxel), int(min_weight), n, _ptr(rays6), float(t_near),
                                    float(t_far), _ptr(out["t"]), _ptr(out["point"]), _ptr(out["normal"]), _ptr(out["code"]), info.ctypes.data))
        return dict({k: v[:n].cpu().numpy() for k, v in out.items()}, info=info)

    def mesh_raycast_pixels(self, q, w, origin3, voxel, min_weight, T_wc12, calib8, width, height, step, uv=None, t_near=0.0, t_far=float("inf"),
                            pose=True):
        """alva_mesh_raycast_pixels: the rays of image pixels from the pose T_wc12 = R_wc row-major then t_wc.  uv None: the grid (width //
        step) x (height // step), row-major; otherwise uv [n,2] float32 raw pixels on the device.  Returns a dict of numpy arrays: t [n]
        float32 (the camera-space z), point and normal [n,3] float32, code [n] uint8, with pose also pose [n,16] float32 and pose_ok [n]
        uint8, and info [8] int32."""
        import numpy as np
        n_vol = self._mesh_volume(q, w)
        step = int(step)
        o = np.ascontiguousarray(origin3, np.float64).reshape(-1)
        T = np.ascontiguousarray(T_wc12, np.float64).reshape(-1)
        calib = np.ascontiguousarray(calib8, np.float64)
        assert o.size == 3 and T.size == 12 and calib.size == 8
        if uv is None:
            n = (int(width) // step) * (int(height) // step) if 1 <= step <= 16 else 1
        else:
            assert uv.dtype == torch.float32 and uv.is_contiguous() and uv.dim() == 2 and uv.shape[1] == 2 and uv.device == q.device
            n = int(uv.shape[0])
        out = self._raycast_outputs(max(n, 1), q.device, pose)
        info = np.zeros(8, np.int32)
        check(lib.alva_mesh_raycast_pixels(self.h, _ptr(q), _ptr(w), n_vol, o.ctypes.data, float(voxel), int(min_weight), T.ctypes.data,
                                           calib.ctypes.data, int(width), int(height), step, n, _ptr(uv), float(t_near), float(t_far),
                                           _ptr(out["t"]), _ptr(out["point"]), _ptr(out["normal"]), _ptr(out["code"]), _ptr(out.get("pose")),
                                           _ptr(out.get("pose_ok")), info.ctypes.data))
        return dict({k: v[:n].cpu().numpy() for k, v in out.items()}, info=info)

    def color_thumb(self, rgba, cstep=4, width=None):
        """alva_color_thumb: rgba [h,w,4] uint8 on the device (any row stride that is a multiple of 4; `width` narrows the image to its
        first `width` columns) reduced to a thumbnail [h // cstep, w // cstep, 4] uint8 on the device: the mean of every cstep x cstep
        block in the pixel-value domain, alpha 255.  Enqueues; returns the thumbnail."""
        if not hasattr(lib, "alva_color_thumb"):   # (an older build loaded through ALVA_LIB for an A/B measurement)
            raise AlvaError("alva_color_thumb is not in the loaded library")
        assert rgba.dtype == torch.uint8 and rgba.dim() == 3 and rgba.shape[2] == 4 and rgba.stride(2) == 1 and rgba.stride(1) == 4
        h, w = int(rgba.shape[0]), int(rgba.shape[1] if width is None else width)
        assert w <= rgba.shape[1]
        cstep = int(cstep)
        tw, th = (w // cstep, h // cstep) if 1 <= cstep <= 16 else (1, 1)
        out = torch.empty((max(th, 1), max(tw, 1), 4), dtype=torch.uint8, device=rgba.device)
        check(lib.alva_color_thumb(self.h, _ptr(rgba), rgba.stride(0), w, h, cstep, _ptr(out)))
        return out

    def mesh_integrate_color(self, q, w, c, origin3, voxel, trunc, T_cw12, calib8, width, height, step, meas, thumb, cstep=4, w_max=128):
        """alva_mesh_integrate_color: mesh_integrate with the colour volume c [N,N,N,4] uint8 (r, g, b, colour weight) on the device,
        updated IN PLACE like q and w, and thumb = color_thumb's output for the frame ([height // cstep, width // cstep, 4] uint8 on the
        device).  Returns info [8] int32; info[6] = voxels coloured."""
        import numpy as np
        if not hasattr(lib, "alva_mesh_integrate_color"):
            raise AlvaError("alva_mesh_integrate_color is not in the loaded library")
        n = self._mesh_volume(q, w)
        assert c.dtype == torch.uint8 and c.is_contiguous() and tuple(c.shape) == (n, n, n, 4) and c.device == q.device
        step, cstep = int(step), int(cstep)
        gw, gh = (int(width) // step, int(height) // step) if 1 <= step <= 16 else (1, 1)
        tw, th = (int(width) // cstep, int(height) // cstep) if 1 <= cstep <= 16 else (1, 1)
        o = np.ascontiguousarray(origin3, np.float64).reshape(-1)
        T = np.ascontiguousarray(T_cw12, np.float64).reshape(-1)
        calib = np.ascontiguousarray(calib8, np.float64)
        assert o.size == 3 and T.size == 12 and calib.size == 8 and len(meas) == 3
        for a, ty in zip(meas, (torch.float32, torch.uint8, torch.uint8)):
            assert a.dtype == ty and a.is_contiguous() and a.numel() >= max(gw * gh, 1) and a.device == q.device
        assert thumb.dtype == torch.uint8 and thumb.is_contiguous() and thumb.numel() >= 4 * max(tw * th, 1) and thumb.device == q.device
        info = np.zeros(8, np.int32)
        check(lib.alva_mesh_integrate_color(self.h, _ptr(q), _ptr(w), _ptr(c), n, o.ctypes.data, float(voxel), float(trunc), T.ctypes.data,
                                            calib.ctypes.data, int(width), int(height), step, _ptr(meas[0]), _ptr(meas[1]), _ptr(meas[2]),
                                            _ptr(thumb), cstep, int(w_max), info.ctypes.data))
        return info

    def mesh_color_at(self, c, origin3, voxel, points):
        """alva_mesh_color_at: the colour volume c [N,N,N,4] uint8 on the device sampled at points [n,3] float32 on the device (world
        coordinates).  Returns (rgba [n,4] uint8, codes [n] uint8, info [8] int32) as numpy arrays; code 0 a colour, 1 outside the
        volume, 2 no colour was fused there, 4 a point that is not finite."""
        import numpy as np
        if not hasattr(lib, "alva_mesh_color_at"):
            raise AlvaError("alva_mesh_color_at is not in the loaded library")
        assert c.dtype == torch.uint8 and c.is_contiguous() and c.dim() == 4 and c.shape[3] == 4 and c.shape[0] == c.shape[1] == c.shape[2]
        assert points.dtype == torch.float32 and points.is_contiguous() and points.dim() == 2 and points.shape[1] == 3 and points.device == c.device
        o = np.ascontiguousarray(origin3, np.float64).reshape(-1)
        assert o.size == 3
        n = int(points.shape[0])
        rgba = torch.empty((max(n, 1), 4), dtype=torch.uint8, device=c.device)
        codes = torch.empty(max(n, 1), dtype=torch.uint8, device=c.device)
        info = np.zeros(8, np.int32)
        check(lib.alva_mesh_color_at(self.h, _ptr(c), int(c.shape[0]), o.ctypes.data, float(voxel), n, _ptr(points), _ptr(rgba), _ptr(codes),
                                     info.ctypes.data))
        return rgba[:n].cpu().numpy(), codes[:n].cpu().numpy(), info

    def mesh_shift(self, q, w, shift3, c=None, out=None):
        """alva_mesh_shift: the volume q [N,N,N] int16 and w [N,N,N] uint8 (and c [N,N,N,4] uint8, the colour volume) on the device,
        translated by shift3 = (s_x, s_y, s_z) voxels -- any ints -- into NEW tensors: the destination voxel (i, j, k) = [k, j, i] has
        the source (i + s_x, j + s_y, k + s_z), zeros where that lies outside.  The inputs are not changed.  Returns (q2, w2, info [8]
        int32) or, with c, (q2, w2, c2, info): info = (copied, copied with w > 0, weighted voxels lost, copied with a colour weight > 0,
        0, 0, 0, N).  out: the output tensors (q2, w2[, c2]) to write into instead (the stage refuses any that overlaps an input)."""
        import numpy as np
        if not hasattr(lib, "alva_mesh_shift"):
            raise AlvaError("alva_mesh_shift is not in the loaded library")
        n = self._mesh_volume(q, w)
        if c is not None:
            assert c.dtype == torch.uint8 and c.is_contiguous() and tuple(c.shape) == (n, n, n, 4) and c.device == q.device
        s = np.ascontiguousarray(shift3, np.int32).reshape(-1)
        assert s.size == 3
        if out is None:
            out = (torch.empty_like(q), torch.empty_like(w)) + (() if c is None else (torch.empty_like(c),))
        assert len(out) == (2 if c is None else 3)
        for a, b in zip(out, (q, w, c)):
            assert a.dtype == b.dtype and a.device == b.device and a.numel() == b.numel() and a.is_contiguous()
        info = np.zeros(8, np.int32)
        check(lib.alva_mesh_shift(self.h, _ptr(q), _ptr(w), _ptr(c), n, s.ctypes.data, _ptr(out[0]), _ptr(out[1]),
                                  _ptr(out[2]) if c is not None else 0, info.ctypes.data))
        return tuple(out) + (info,)

    @staticmethod
    def mesh_block_grid(n, lattice3, block):
        """L1's block grid of a volume of n^3 voxels: (lowest key [3], blocks per axis [3]) as int64 arrays"""
        import numpy as np
        lat = np.asarray(lattice3, np.int64).reshape(-1)
        assert lat.size == 3
        bmin = lat // int(block)   # numpy's // is a floor
        return bmin, (lat + n - 1) // int(block) - bmin + 1

    def mesh_block_digest(self, q, w, lattice3, min_weight, block):
        """alva_mesh_block_digest: the volume q [N,N,N] int16 and w [N,N,N] uint8 on the device, lattice3 the global index of voxel
        (0, 0, 0), block 8, 16 or 32.  Returns (digest [nb] uint64, counts [nb,2] int32 = (nv, nq), nb3 [3] int32) as numpy arrays; the
        blocks are in ascending (b_z, b_y, b_x) from the key floor(lattice / block)."""
        import numpy as np
        if not hasattr(lib, "alva_mesh_block_digest"):
            raise AlvaError("alva_mesh_block_digest is not in the loaded library")
        n = self._mesh_volume(q, w)
        lat = np.ascontiguousarray(lattice3, np.int32).reshape(-1)
        assert lat.size == 3
        # the outputs' size: the largest grid any lattice gives (the call itself checks block and the lattice)
        cap = (n // 8 + 2) ** 3
        digest = torch.empty(cap, dtype=torch.int64, device=q.device)
        counts = torch.empty((cap, 2), dtype=torch.int32, device=q.device)
        nb3 = np.zeros(3, np.int32)
        rc = lib.alva_mesh_block_digest(self.h, _ptr(q), _ptr(w), n, lat.ctypes.data, int(min_weight), int(block), nb3.ctypes.data, _ptr(digest),
                                        _ptr(counts))
        if rc != 0:
            raise StageError(rc, lib.alva_last_error().decode())
        nb = int(nb3.prod())
        return digest[:nb].cpu().numpy().view(np.uint64), counts[:nb].cpu().numpy(), nb3

    def mesh_extract_blocks(self, q, w, origin3, voxel, lattice3, min_weight, block, sel_keys, max_vertices, max_triangles):
        """alva_mesh_extract_blocks: the volume as for mesh_block_digest, sel_keys [n_sel,3] = (b_x, b_y, b_z) strictly ascending in (z, y,
        x).  Returns a dict of numpy arrays: vertices, normals [nv,3] float32, triangles [nt,3] int32 (indices local to each block), ranges
        [n_sel,4] int32 = (v0, nv, t0, nt), info [8] int32; everything is empty or zero unless info[0] == 0.  A refused selection raises
        StageError with rc == StageError.ERR_ARG."""
        import numpy as np
        if not hasattr(lib, "alva_mesh_extract_blocks"):
            raise AlvaError("alva_mesh_extract_blocks is not in the loaded library")
        n = self._mesh_volume(q, w)
        o = np.ascontiguousarray(origin3, np.float64).reshape(-1)
        lat = np.ascontiguousarray(lattice3, np.int32).reshape(-1)
        keys = np.ascontiguousarray(sel_keys, np.int32).reshape(-1, 3)
        assert o.size == 3 and lat.size == 3
        mv, mt = max(int(max_vertices), 1), max(int(max_triangles), 1)
        vertices = torch.empty((mv, 3), dtype=torch.float32, device=q.device)
        normals = torch.empty((mv, 3), dtype=torch.float32, device=q.device)
        triangles = torch.empty((mt, 3), dtype=torch.int32, device=q.device)
        ranges = np.zeros((len(keys), 4), np.int32)
        info = np.zeros(8, np.int32)
        rc = lib.alva_mesh_extract_blocks(self.h, _ptr(q), _ptr(w), n, o.ctypes.data, float(voxel), lat.ctypes.data, int(min_weight), int(block),
                                          len(keys), keys.ctypes.data, int(max_vertices), int(max_triangles), _ptr(vertices), _ptr(normals),
                                          _ptr(triangles), ranges.ctypes.data, info.ctypes.data)
        if rc != 0:
            raise StageError(rc, lib.alva_last_error().decode())
        nv, nt = (int(info[1]), int(info[2])) if info[0] == 0 else (0, 0)
        return dict(vertices=vertices[:nv].cpu().numpy(), normals=normals[:nv].cpu().numpy(), triangles=triangles[:nt].cpu().numpy(),
                    ranges=ranges, info=info)

    def light_bin(self, rgba, calib8, R_wc9, step=4, acc=None, width=None):
        """alva_light_bin: rgba [h,w,4] uint8 on the device (any row stride; `width` narrows the image to its first `width` columns),
        calib8 = fx fy cx cy k1 k2 p1 p2, R_wc9 the camera-to-world rotation (row-major) or None (not tracking).  acc: the frame
        accumulators, int64 [LIGHT_ACC_WORDS] on the device, added to (None: fresh zeros).  Enqueues; returns acc."""
        import numpy as np
        assert rgba.dtype == torch.uint8 and rgba.dim() == 3 and rgba.shape[2] == 4 and rgba.stride(2) == 1 and rgba.stride(1) == 4
        h, w = int(rgba.shape[0]), int(rgba.shape[1] if width is None else width)
        assert w <= rgba.shape[1]
        calib = np.ascontiguousarray(calib8, np.float64)
        R = None if R_wc9 is None else np.ascontiguousarray(R_wc9, np.float64).reshape(-1)
        assert calib.size == 8 and (R is None or R.size == 9)
        if acc is None:
            acc = torch.zeros(LIGHT_ACC_WORDS, dtype=torch.int64, device=rgba.device)
        assert acc.dtype == torch.int64 and acc.is_contiguous() and acc.numel() >= LIGHT_ACC_WORDS
        check(lib.alva_light_bin(self.h, _ptr(rgba), rgba.stride(0), w, h, calib.ctypes.data, None if R is None else R.ctypes.data, int(step),
                                 _ptr(acc)))
        return acc

    def light_fuse(self, acc, state=None, min_pixels=64, w_new=32, w_max=224, want_acc=False):
        """alva_light_fuse: the accumulators (int64 [LIGHT_ACC_WORDS], zeroed by the call) folded into the environment state (uint8
        [LIGHT_STATE_BYTES] on the device, updated in place; None: a fresh empty one).  Enqueues; returns state, or (state, the
        accumulators as they were) with want_acc."""
        assert acc.dtype == torch.int64 and acc.is_contiguous() and acc.numel() >= LIGHT_ACC_WORDS
        if state is None:
            state = torch.zeros(LIGHT_STATE_BYTES, dtype=torch.uint8, device=acc.device)
        assert state.dtype == torch.uint8 and state.is_contiguous() and state.numel() >= LIGHT_STATE_BYTES
        was = torch.empty(LIGHT_ACC_WORDS, dtype=torch.int64, device=acc.device) if want_acc else None
        check(lib.alva_light_fuse(self.h, _ptr(acc), _ptr(state), int(min_pixels), int(w_new), int(w_max), _ptr(was)))
        return (state, was) if want_acc else state

    def light_estimate(self, state):
        """alva_light_estimate: the state (uint8 [LIGHT_STATE_BYTES] on the device) projected -> (sh [9,3], primary_dir [3], primary_rgb
        [3], ambient [4], each float32, info [8] int32) as numpy arrays."""
        import numpy as np
        assert state.dtype == torch.uint8 and state.is_contiguous() and state.numel() >= LIGHT_STATE_BYTES
        sh, pd, pc, amb, info = np.zeros(27, np.float32), np.zeros(3, np.float32), np.zeros(3, np.float32), np.zeros(4, np.float32), np.zeros(8, np.int32)
        check(lib.alva_light_estimate(self.h, _ptr(state), *(a.ctypes.data for a in (sh, pd, pc, amb, info))))
        return sh.reshape(9, 3), pd, pc, amb, info

    def image_match(self, qdesc, qxy, nq, tdesc, txy, n_train, max_dist=64, ratio=0.8):
        """alva_image_match: qdesc [n_images, IMAGE_QUERY_CAP, 32] uint8 and qxy [n_images, IMAGE_QUERY_CAP, 2] float32 (the images'
        descriptors and keypoints, nq[j] rows of image j in use), tdesc [cap, 32] uint8 and txy [cap, 2] float32 (the frame's, cap <=
        IMAGE_TRAIN_CAP), n_train an int32 tensor holding the frame's count -- all on the device.  Enqueues; returns (match [n_images,
        IMAGE_QUERY_CAP, 3] int32, xy [n_images, IMAGE_QUERY_CAP, 4] float64, count [n_images] int32) on the device: the first count[j]
        rows of image j are its pairs, the rest is not written."""
        import numpy as np
        n = int(qdesc.shape[0])
        assert qdesc.dtype == torch.uint8 and tuple(qdesc.shape) == (n, IMAGE_QUERY_CAP, 32) and qdesc.is_contiguous()
        assert qxy.dtype == torch.float32 and tuple(qxy.shape) == (n, IMAGE_QUERY_CAP, 2) and qxy.is_contiguous()
        cap = int(tdesc.shape[0])
        assert tdesc.dtype == torch.uint8 and tuple(tdesc.shape) == (cap, 32) and tdesc.is_contiguous()
        assert txy.dtype == torch.float32 and tuple(txy.shape) == (cap, 2) and txy.is_contiguous()
        assert n_train.dtype == torch.int32 and n_train.numel() >= 1
        counts = np.ascontiguousarray(nq, np.int32)
        assert counts.size == n
        dev = qdesc.device
        match = torch.zeros((n, IMAGE_QUERY_CAP, 3), dtype=torch.int32, device=dev)
        xy = torch.zeros((n, IMAGE_QUERY_CAP, 4), dtype=torch.float64, device=dev)
        count = torch.zeros(n, dtype=torch.int32, device=dev)
        check(lib.alva_image_match(self.h, n, _ptr(qdesc), _ptr(qxy), counts.ctypes.data, _ptr(tdesc) if cap else None,
                                   _ptr(txy) if cap else None, _ptr(n_train), cap, int(max_dist), float(ratio), _ptr(match), _ptr(xy),
                                   _ptr(count)))
        return match, xy, count

    def image_homography(self, xy, count, wh, frame_wh, calib4, num_iterations=256, threshold_px=3.0, min_inliers=20, seed=12345,
                         rand4=None):
        """alva_image_homography: xy [n_images, IMAGE_QUERY_CAP, 4] float64 and count [n_images] int32 on the device (alva_image_match's
        outputs), wh [n_images, 2] the pictures' sizes, frame_wh, calib4 = fx fy cx cy; rand4 [iterations, 4] uint32 replaces the hashed
        sample words.  Returns numpy arrays (H [n, 9], info [n, 8] int32, mask [n, IMAGE_QUERY_CAP] uint8, R [n, 9], t [n, 3])."""
        import numpy as np
        n = int(xy.shape[0])
        assert xy.dtype == torch.float64 and tuple(xy.shape) == (n, IMAGE_QUERY_CAP, 4) and xy.is_contiguous()
        assert count.dtype == torch.int32 and count.numel() == n and count.is_contiguous()
        sizes = np.ascontiguousarray(wh, np.int32).reshape(-1, 2)
        calib = np.ascontiguousarray(calib4, np.float64)
        assert len(sizes) == n and calib.size >= 4
        words = None if rand4 is None else np.ascontiguousarray(rand4, np.uint32).reshape(-1, 4)
        H, info, mask = np.zeros((n, 9)), np.zeros((n, 8), np.int32), np.zeros((n, IMAGE_QUERY_CAP), np.uint8)
        R, t = np.zeros((n, 9)), np.zeros((n, 3))
        check(lib.alva_image_homography(self.h, n, _ptr(xy), _ptr(count), sizes.ctypes.data, int(frame_wh[0]), int(frame_wh[1]),
                                        calib.ctypes.data, int(num_iterations if words is None else len(words)), float(threshold_px),
                                        int(min_inliers), int(seed), None if words is None else words.ctypes.data, H.ctypes.data,
                                        info.ctypes.data, mask.ctypes.data, R.ctypes.data, t.ctypes.data))
        return H, info, mask, R, t

    def _planes(self, prior, points, pose7, thickness, min_inliers, max_planes, num_iterations, seed, rand3, want_labels, want_moments,
                labels_out=None):
        """what detect_planes (prior None: lib.alva_detect_planes) and track_planes (prior [n_prior,24]: lib.alva_track_planes) share"""
        import numpy as np
        assert points.dtype == torch.float64 and points.is_contiguous()
        pose = np.ascontiguousarray(pose7, np.float64)
        assert pose.size == 7
        n_prior = 0 if prior is None else len(prior)
        n, k = points.shape[0], max(int(max_planes), n_prior, 1)
        words = None if rand3 is None else np.ascontiguousarray(rand3, np.uint32).reshape(-1, 3)
        want_words = int(max_planes) * int(num_iterations) if prior is None else max(int(max_planes) - n_prior, 0) * int(num_iterations)
        if words is not None and len(words) != want_words:
            raise AlvaError("rand3 must hold %s * num_iterations triples" % ("max_planes" if prior is None else "(max_planes - n_prior)"))
        planes, info = np.zeros((k, 24), np.float32), np.zeros((k, 8), np.int32)
        mom = np.zeros((k, 10), np.float64) if want_moments else None
        labels = labels_out
        if labels is None and want_labels:
            labels = torch.empty(max(n, 1), dtype=torch.int32, device=points.device)
        if labels is not None:
            assert labels.dtype == torch.int32 and labels.is_contiguous() and labels.shape[0] >= n
        head = (self.h, _ptr(points) if n else None, n, pose.ctypes.data, float(thickness), int(min_inliers), int(max_planes), int(num_iterations),
                int(seed), None if words is None else words.ctypes.data)
        tail = (planes.ctypes.data, info.ctypes.data, None if labels is None else _ptr(labels), None if mom is None else mom.ctypes.data)
        rc = (lib.alva_detect_planes(*head, *tail) if prior is None else
              lib.alva_track_planes(*head, n_prior, prior.ctypes.data if n_prior else None, *tail))
        if rc < 0:
            check(rc)
        out = (planes[:max_planes], info[:max_planes])
        if want_labels:
            out += (labels[:n].cpu().numpy(),)
        if want_moments:
            out += (mom[:max_planes],)
        return out

    def detect_planes(self, points, pose7, thickness, min_inliers=48, max_planes=4, num_iterations=128, seed=12345, rand3=None,
                      want_labels=False, want_moments=False):
        """alva_detect_planes: points [n,3] float64 on the device, pose7 = Twc (t, q = x y z w); rand3 [max_planes * iterations, 3] uint32
        replaces the hashed sample words.  Returns (planes [max_planes,24] float32 -- rows of rounds whose code is not 0 stay zero --,
        info [max_planes,8] int32), then with want_labels the labels [n] int32 (numpy) and with want_moments the refits' sums
        [max_planes,10] float64."""
        return self._planes(None, points, pose7, thickness, min_inliers, max_planes, num_iterations, seed, rand3, want_labels, want_moments)

    def track_planes(self, points, pose7, thickness, prior24=None, min_inliers=48, max_planes=4, num_iterations=128, seed=12345, rand3=None,
                     want_labels=False, want_moments=False, labels_out=None):
        """alva_track_planes: detect_planes' arguments and results, with prior24 [n_prior,24] float32 -- the records of an earlier call,
        which keep their slots (None: no priors, and the call is detect_planes).  rand3 [(max_planes - n_prior) * iterations, 3] uint32.
        info [max_planes,8] = code (0 a plane, 1 .. 5 detect_planes', 7 / 8 a prior lost before / after its refit, 9 unusable prior),
        points or live points, -1 or winning iteration, claimed or best count, inliers, origin (1 tracked, 0 new).  labels_out: a device
        int32 tensor [n] to receive the labels (they stay on the device)."""
        import numpy as np
        prior = np.zeros((0, 24), np.float32) if prior24 is None else np.ascontiguousarray(prior24, np.float32).reshape(-1, 24)
        return self._planes(prior, points, pose7, thickness, min_inliers, max_planes, num_iterations, seed, rand3, want_labels, want_moments,
                            labels_out)

    def anchor_attach(self, points, pos3, max_support=32):
        """alva_anchor_attach: points [n,3] float64 on the device, pos3 [a,3] float64 -- the anchors' world positions.  Returns (index
        [a,max_support] int32 -- the max_support nearest points of each position in ascending (distance, index), -1 past count --, dist2
        [a,max_support] float64 -- their squared distances, 0 past count --, count [a] int32)."""
        import numpy as np
        assert points.dtype == torch.float64 and points.is_contiguous()
        pos = np.ascontiguousarray(pos3, np.float64).reshape(-1, 3)
        n, a, k = points.shape[0], len(pos), max(int(max_support), 1)
        index, dist2 = np.zeros((max(a, 1), k), np.int32), np.zeros((max(a, 1), k), np.float64)
        count = np.zeros(max(a, 1), np.int32)
        check(lib.alva_anchor_attach(self.h, _ptr(points) if n else None, n, a, pos.ctypes.data, int(max_support), index.ctypes.data,
                                     dist2.ctypes.data, count.ctypes.data))
        return index[:a], dist2[:a], count[:a]

    def anchor_update(self, count, ref, cur, pose16_ref):
        """alva_anchor_update: count [a] int32 supports per anchor, ref / cur [a,64,3] float64 -- where each support was at attach time
        and is now, rows past count are not read --, pose16_ref [a,16] float32.  Returns (pose16 [a,16] float32, rt12 [a,12] float64 = R
        row-major then t, info [a,8] int32 = code (0 rigid, 1 translation only, 2 no support), supports, kept by the trim)."""
        import numpy as np
        cnt = np.ascontiguousarray(count, np.int32).reshape(-1)
        a = len(cnt)
        r, c = np.ascontiguousarray(ref, np.float64).reshape(-1, 64, 3), np.ascontiguousarray(cur, np.float64).reshape(-1, 64, 3)
        pr = np.ascontiguousarray(pose16_ref, np.float32).reshape(-1, 16)
        if not (len(r) == a and len(c) == a and len(pr) == a):
            raise AlvaError("count, ref, cur and pose16_ref must describe the same number of anchors")
        pose, rt, info = np.zeros((max(a, 1), 16), np.float32), np.zeros((max(a, 1), 12), np.float64), np.zeros((max(a, 1), 8), np.int32)
        check(lib.alva_anchor_update(self.h, a, cnt.ctypes.data, r.ctypes.data, c.ctypes.data, pr.ctypes.data, pose.ctypes.data, rt.ctypes.data,
                                     info.ctypes.data))
        return pose[:a], rt[:a], info[:a]

    def plane_outlines(self, points, labels, planes24, max_vertices=64, want_q=False):
        """alva_plane_outlines: points [n,3] float64 and labels [n] int32 on the device (detect_planes' labels), planes24 [k,24] float32
        (detect_planes' records, numpy).  Returns (outline [k,max_vertices,2] float32 -- the convex polygon of each plane's points in the
        plane's own frame, counter-clockwise, zero past the last vertex --, info [k,8] int32 = code, vertices, points, area [k] float64)
        and, with want_q, the vertices' integer grid coordinates [k,max_vertices,2] int32."""
        import numpy as np
        n = points.shape[0]
        assert points.dtype == torch.float64 and points.is_contiguous() and labels.dtype == torch.int32 and labels.is_contiguous()
        assert labels.shape[0] == n
        rec = np.ascontiguousarray(planes24, np.float32).reshape(-1, 24)
        k, mv = len(rec), int(max_vertices)
        shape = (max(k, 1), max(mv, 1), 2)
        outline, info, area = np.zeros(shape, np.float32), np.zeros((max(k, 1), 8), np.int32), np.zeros(max(k, 1), np.float64)
        q = np.zeros(shape, np.int32) if want_q else None
        rc = lib.alva_plane_outlines(self.h, _ptr(points) if n else None, n, _ptr(labels) if n else None, k, rec.ctypes.data, mv,
                                     outline.ctypes.data, None if q is None else q.ctypes.data, info.ctypes.data, area.ctypes.data)
        if rc < 0:
            check(rc)
        out = (outline[:k], info[:k], area[:k])
        return out + (q[:k],) if want_q else out

    def relpose_hypotheses(self, bv1, bv2, samples8, err=3.0, fx=579.4, fy=579.4):
        """One RANSAC hypothesis per 8-index sample: returns (models [H,12] = R row-major | t, inlier counts [H], -1 = no model)."""
        import numpy as np
        s = np.ascontiguousarray(samples8, np.int32)
        H = s.shape[0]
        models = np.zeros((H, 12))
        counts = np.zeros(H, np.int32)
        check(lib.alva_relpose_hypotheses(self.h, _ptr(bv1), _ptr(bv2), bv1.shape[0], s.ctypes.data, H, float(err), float(fx), float(fy),
                                          models.ctypes.data, counts.ctypes.data))
        return models, counts

    # a9
    def pnp_refine(self, uv, wpts, pose7, K, max_iters=5, chi2th=5.9915, robust=True, l2=True):
        """MultiViewGeometry::ceresPnP: returns (ok, pose7 numpy, outlier indices numpy, info[8])."""
        import numpy as np
        n = uv.shape[0]
        assert uv.dtype == torch.float64 and wpts.dtype == torch.float64
        pose = np.ascontiguousarray(pose7, np.float64).copy()
        out = np.zeros(max(n, 1), np.int32)
        nout = C.c_int(0)
        ok = C.c_int(0)
        info = np.zeros(8)
        check(lib.alva_pnp_refine(self.h, _ptr(uv), _ptr(wpts), n, pose.ctypes.data, max_iters, chi2th, int(robust), int(l2),
                                  K[0], K[1], K[2], K[3], out.ctypes.data, C.byref(nout), info.ctypes.data, C.byref(ok)))
        return bool(ok.value), pose, out[:nout.value].copy(), info

    # a10-a13
    def local_ba(self, pb, max_iters=5, ftol=0.0, huber_chi2=5.9915, inv_depth=True):
        """The solve of Optimizer::localBA on a flat problem dict (see synth.make_ba_problem)."""
        import numpy as np
        poses = np.ascontiguousarray(pb["poses"], np.float64).copy()
        kfc = np.ascontiguousarray(pb["kf_const"], np.uint8)
        calib = np.ascontiguousarray(pb["calib"], np.float64)
        akf = np.ascontiguousarray(pb["anchor_kf"], np.int32)
        auv = np.ascontiguousarray(pb["anchor_uv"], np.float64)
        pts = np.ascontiguousarray(pb["inv_depth"] if inv_depth else pb["pts_xyz"], np.float64).copy()
        okf = np.ascontiguousarray(pb["obs_kf"], np.int32)
        opt = np.ascontiguousarray(pb["obs_pt"], np.int32)
        ouv = np.ascontiguousarray(pb["obs_uv"], np.float64)
        nobs = len(okf)
        chi2 = np.zeros(max(nobs, 1))
        depth = np.zeros(max(nobs, 1), np.uint8)
        info = np.zeros(9)
        ok = C.c_int(0)
        check(lib.alva_local_ba(self.h, len(poses), poses.ctypes.data, kfc.ctypes.data, calib.ctypes.data, int(inv_depth), len(akf),
                                akf.ctypes.data, auv.ctypes.data, pts.ctypes.data, nobs, okf.ctypes.data, opt.ctypes.data,
                                ouv.ctypes.data, max_iters, ftol, huber_chi2, chi2.ctypes.data, depth.ctypes.data, info.ctypes.data,
                                C.byref(ok)))
        return dict(ok=bool(ok.value), poses=poses, pts=pts, chi2=chi2[:nobs], depth=depth[:nobs], info=info)

    def local_ba_csr(self, pb, max_iters=5, ftol=0.0, huber_chi2=5.9915, chi2_threshold=5.9915):
        """alva_local_ba_csr: the same solve for observations grouped by point (the problem dict's observations are stably sorted by
        point here); the sweep's test per residual block comes back as booleans in the SORTED order, `order` maps back."""
        import numpy as np
        poses = np.ascontiguousarray(pb["poses"], np.float64).copy()
        kfc = np.ascontiguousarray(pb["kf_const"], np.uint8)
        calib = np.ascontiguousarray(pb["calib"], np.float64)
        akf = np.ascontiguousarray(pb["anchor_kf"], np.int32)
        auv = np.ascontiguousarray(pb["anchor_uv"], np.float64)
        pts = np.ascontiguousarray(pb["inv_depth"], np.float64).copy()
        opt0 = np.asarray(pb["obs_pt"], np.int64)
        order = np.argsort(opt0, kind="stable")
        okf = np.ascontiguousarray(np.asarray(pb["obs_kf"], np.int32)[order])
        ouv = np.ascontiguousarray(np.asarray(pb["obs_uv"], np.float64)[order])
        nobs, npt = len(okf), len(akf)
        ptr = np.zeros(npt + 1, np.int32)
        np.cumsum(np.bincount(opt0, minlength=npt), out=ptr[1:])
        bits = np.zeros((nobs + 63) // 64 + 1, np.uint64)
        nbad, ok, info = C.c_int(0), C.c_int(0), np.zeros(9)
        lib.alva_local_ba_csr.argtypes = [_vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _d, _d, _d, _vp, _vp, _vp, _vp]
        check(lib.alva_local_ba_csr(self.h, len(poses), poses.ctypes.data, kfc.ctypes.data, calib.ctypes.data, npt, ptr.ctypes.data, akf.ctypes.data,
                                    auv.ctypes.data, pts.ctypes.data, nobs, okf.ctypes.data, ouv.ctypes.data, max_iters, ftol, huber_chi2,
                                    chi2_threshold, bits.ctypes.data, C.byref(nbad), info.ctypes.data, C.byref(ok)))
        bad = np.unpackbits(bits.view(np.uint8), bitorder="little")[:nobs].astype(bool)
        return dict(ok=bool(ok.value), poses=poses, pts=pts, bad=bad, n_bad=nbad.value, order=order, info=info)

    def local_ba_batch(self, pbs, max_iters=5, ftol=0.0, huber_chi2=5.9915):
        """alva_local_ba_batch on a list of flat problem dicts (anchored inverse depth); returns one result dict per problem"""
        import numpy as np
        n = len(pbs)
        keep = []

        def arr(x, dt, copy=False):
            a = np.ascontiguousarray(x, dt)
            a = a.copy() if copy else a
            keep.append(a)
            return a
        poses = [arr(pb["poses"], np.float64, True) for pb in pbs]
        kfc = [arr(pb["kf_const"], np.uint8) for pb in pbs]
        akf = [arr(pb["anchor_kf"], np.int32) for pb in pbs]
        auv = [arr(pb["anchor_uv"], np.float64) for pb in pbs]
        pts = [arr(pb["inv_depth"], np.float64, True) for pb in pbs]
        okf = [arr(pb["obs_kf"], np.int32) for pb in pbs]
        opt = [arr(pb["obs_pt"], np.int32) for pb in pbs]
        ouv = [arr(pb["obs_uv"], np.float64) for pb in pbs]
        chi2 = [np.zeros(len(o)) for o in okf]
        depth = [np.zeros(len(o), np.uint8) for o in okf]
        calib = arr(pbs[0]["calib"], np.float64)
        info = np.zeros((n, 4))
        ok = np.zeros(n, np.int32)
        ptrs = lambda lst: (C.c_void_p * n)(*[a.ctypes.data for a in lst])
        ints = lambda vals: (C.c_int * n)(*vals)
        lib.alva_local_ba_batch.argtypes = [_vp, _i] + [_vp] * 3 + [_vp] + [_vp] * 4 + [_vp] * 4 + [_i, _d, _d] + [_vp] * 4
        check(lib.alva_local_ba_batch(self.h, n, ints([len(p) for p in poses]), ptrs(poses), ptrs(kfc), calib.ctypes.data, ints([len(a) for a in akf]),
                                      ptrs(akf), ptrs(auv), ptrs(pts), ints([len(o) for o in okf]), ptrs(okf), ptrs(opt), ptrs(ouv), max_iters, ftol,
                                      huber_chi2, ptrs(chi2), ptrs(depth), info.ctypes.data, ok.ctypes.data))
        return [dict(ok=bool(ok[b]), poses=poses[b], pts=pts[b], chi2=chi2[b], depth=depth[b], info=info[b]) for b in range(n)]

    # a5
    def detect_grid(self, gray, cell, occupied=None, roi=None, max_quality=0.001, cap=None):
        """FeatureExtractor::detectFeaturePoints: returns (pts [n,2] float32 cuda tensor, new max_quality)."""
        h, w = gray.shape
        if roi is None:
            roi = (20, 20, w - 40, h - 40)
        if cap is None:
            cap = 2 * (w // cell) * (h // cell) + 1
        nocc = 0 if occupied is None else occupied.shape[0]
        out = torch.zeros((max(cap, 1), 2), dtype=torch.float32, device=gray.device)   # (cap 0: the C ABI still wants a buffer)
        mq = C.c_double(max_quality)
        cnt = C.c_int(0)
        check(lib.alva_detect_grid(self.h, _ptr(gray), gray.stride(0), w, h, cell, _ptr(occupied) if nocc else None, nocc,
                                   roi[0], roi[1], roi[2], roi[3], C.byref(mq), _ptr(out), cap, C.byref(cnt)))
        return out[:min(cnt.value, cap)], mq.value

    def detect_grid_debug_eig(self, n_cells, cell):
        """the lambda_min plane of the last detect_grid call on this context: [n_cells, cell, cell] float32 cuda tensor"""
        out = torch.zeros((n_cells, cell, cell), dtype=torch.float32, device="cuda")
        check(lib.alva_detect_grid_debug_eig(self.h, n_cells, cell, _ptr(out)))
        return out

    def detect_grid_enqueue(self, gray, cell, occupied=None, roi=None, max_quality=0.001, cap=None, out=None):
        """alva_detect_grid_enqueue: launches the detection with the threshold `max_quality` and returns at once.  `out` may be a caller's
        [>= cap, 2] float32 cuda tensor (only its first `cap` rows may be written).  Returns the handle for detect_grid_collect; no other
        call on the context in between."""
        h, w = gray.shape
        if roi is None:
            roi = (20, 20, w - 40, h - 40)
        if cap is None:
            cap = 2 * (w // cell) * (h // cell) + 1
        if out is None:
            out = torch.zeros((max(cap, 1), 2), dtype=torch.float32, device=gray.device)
        assert out.dtype == torch.float32 and out.is_contiguous() and out.shape[0] >= cap and out.shape[1] == 2
        nocc = 0 if occupied is None else occupied.shape[0]
        pending = DetectPending()
        check(lib.alva_detect_grid_enqueue(self.h, _ptr(gray), gray.stride(0), w, h, cell, _ptr(occupied) if nocc else None, nocc,
                                           roi[0], roi[1], roi[2], roi[3], max_quality, _ptr(out), cap, C.byref(pending)))
        return dict(pending=pending, out=out, cap=cap, max_quality=max_quality, keep=(gray, occupied))

    def detect_grid_collect(self, handle):
        """alva_detect_grid_collect: waits for the enqueued detection.  Returns (pts [min(count, cap), 2] float32 cuda tensor, the new
        max_quality, count = the number of points found, which the capacity does not limit)."""
        mq = C.c_double(handle["max_quality"])
        cnt = C.c_int(-1)
        check(lib.alva_detect_grid_collect(self.h, C.byref(handle["pending"]), C.byref(mq), C.byref(cnt)))
        return handle["out"][:min(cnt.value, handle["cap"])], mq.value, cnt.value

    # a5'
    def fast(self, gray, threshold=20, cap=200000):
        """cv::FAST(TYPE_9_16, NMS): returns (xy [n,2] int32, score [n] int32) cuda tensors, row-major order."""
        h, w = gray.shape
        xy = torch.zeros((cap, 2), dtype=torch.int32, device=gray.device)
        sc = torch.zeros(cap, dtype=torch.int32, device=gray.device)
        cnt = C.c_int(0)
        check(lib.alva_fast(self.h, _ptr(gray), gray.stride(0), w, h, threshold, _ptr(xy), _ptr(sc), cap, C.byref(cnt)))
        n = min(cnt.value, cap)
        return xy[:n], sc[:n]

    # f1
    def match_to_map(self, calib10, cell_size, num_cells_w, grid_cells, cell_ptr, cell_mp, kf_q, kf_t, mp_wpt, mp_is3d, obs_ptr, obs_kf,
                     obs_px, obs_desc, frame_kf, num_kp3d, local, max_proj_err=2.0, dist_ratio=0.2):
        """Mapper::matchToMap on a flattened map (see include/alvaar_hip.h); all arrays cuda tensors, calib10 a host sequence.
        Returns match_of_mp [n_mp] int32 (cuda)."""
        import numpy as np
        n_mp = mp_wpt.shape[0]
        out = torch.empty(n_mp, dtype=torch.int32, device=mp_wpt.device)
        cal = np.ascontiguousarray(calib10, np.float64)
        check(lib.alva_match_to_map(self.h, cal.ctypes.data, int(cell_size), int(num_cells_w), int(grid_cells), _ptr(cell_ptr), _ptr(cell_mp),
                                    kf_q.shape[0], _ptr(kf_q), _ptr(kf_t), n_mp, _ptr(mp_wpt), _ptr(mp_is3d), _ptr(obs_ptr), _ptr(obs_kf),
                                    _ptr(obs_px), _ptr(obs_desc), int(frame_kf), int(num_kp3d), local.shape[0], _ptr(local),
                                    float(max_proj_err), float(dist_ratio), _ptr(out)))
        return out

    def match_to_map_flags(self, calib10, cell_size, num_cells_w, grid_cells, cell_ptr, cell_mp, kf_q, kf_t, mp_wpt, mp_is3d, obs_ptr, obs_kf,
                           obs_px, obs_desc, frame_kf, num_kp3d, local, mp_has_desc=None, obs_has_desc=None, max_proj_err=2.0, dist_ratio=0.2):
        """alva_match_to_map_flags -- the entry the System's flat path calls: match_to_map plus mp_has_desc [n_mp] / obs_has_desc [n_obs]
        uint8 cuda tensors (a map point / an observation without a descriptor); None passes NULL = every observation carries one.
        Returns match_of_mp [n_mp] int32 (cuda)."""
        import numpy as np
        n_mp = mp_wpt.shape[0]
        for t, n in ((mp_has_desc, n_mp), (obs_has_desc, obs_kf.shape[0])):
            if t is not None and (t.dtype != torch.uint8 or t.shape[0] != n or not t.is_contiguous()):
                raise ValueError("has-descriptor flags: contiguous uint8, one per map point / per observation")
        out = torch.empty(n_mp, dtype=torch.int32, device=mp_wpt.device)
        cal = np.ascontiguousarray(calib10, np.float64)
        check(lib.alva_match_to_map_flags(self.h, cal.ctypes.data, int(cell_size), int(num_cells_w), int(grid_cells), _ptr(cell_ptr),
                                          _ptr(cell_mp), kf_q.shape[0], _ptr(kf_q), _ptr(kf_t), n_mp, _ptr(mp_wpt), _ptr(mp_is3d),
                                          _ptr(mp_has_desc), _ptr(obs_ptr), _ptr(obs_kf), _ptr(obs_px), _ptr(obs_desc), _ptr(obs_has_desc),
                                          int(frame_kf), int(num_kp3d), local.shape[0], _ptr(local), float(max_proj_err), float(dist_ratio),
                                          _ptr(out)))
        return out

    MP_ENT_CAP = 40   # csrc/slam/mp_rec.hpp

    @staticmethod
    def mp_record_dtype():
        """numpy layout of one map-point record (csrc/slam/mp_rec.hpp, 1024 bytes)"""
        import numpy as np
        ent = np.dtype([("kf", "<i4"), ("flags", "u1"), ("pad", "u1", 3), ("px", "<f4", 2), ("unpx", "<f4", 2)])
        rec = np.dtype([("X", "<f8", 3), ("inv_depth", "<f8"), ("id", "<i4"), ("anchor_kf", "<i4"), ("is3d", "u1"), ("has_desc", "u1"),
                        ("observed", "u1"), ("n_ent", "u1"), ("n_obs", "u1"), ("overflow", "u1"), ("pad8", "u1", 2), ("dev_slot", "<i4"),
                        ("pad32", "<i4", 3), ("ent", ent, Context.MP_ENT_CAP)])
        assert ent.itemsize == 24 and rec.itemsize == 1024
        return rec

    def match_to_map_records(self, calib10, cell_size, num_cells_w, grid_cells, cell_ptr, cell_mp, kf_ids, kf_q, kf_t, frame_kf_index, mp_slot,
                             chunk_table, medoid_store, num_kp3d, local, max_proj_err=2.0, dist_ratio=0.2):
        """Mapper::matchToMap on map-point RECORDS (alva_match_to_map_records): mp_slot [n_mp] names each row's record; chunk_table is a cuda
        int64 tensor of the record chunks' addresses (pinned host memory, 4096 records per chunk); descriptors come from medoid_store's
        tables.  Returns match_of_mp [n_mp] int32 (cuda)."""
        import numpy as np
        lib.alva_medoid_tables.restype = C.c_void_p
        lib.alva_medoid_tables.argtypes = [C.c_void_p]
        n_mp = mp_slot.shape[0]
        out = torch.empty(n_mp, dtype=torch.int32, device=mp_slot.device)
        cal = np.ascontiguousarray(calib10, np.float64)
        frame_kf_id = int(kf_ids[int(frame_kf_index)].item())
        check(lib.alva_match_to_map_records(self.h, cal.ctypes.data, int(cell_size), int(num_cells_w), int(grid_cells), _ptr(cell_ptr), _ptr(cell_mp),
                                            kf_ids.shape[0], _ptr(kf_ids), _ptr(kf_q), _ptr(kf_t), int(frame_kf_index), frame_kf_id, n_mp, _ptr(mp_slot),
                                            _ptr(chunk_table), lib.alva_medoid_tables(medoid_store.h), int(num_kp3d), local.shape[0],
                                            _ptr(local), float(max_proj_err), float(dist_ratio), _ptr(out)))
        return out

    # f4b
    def undistort_points(self, px, K, dist):
        """CameraCalibration::undistortImagePoint for n pixels [n,2] f32; K = (fx,fy,cx,cy), dist = (k1,k2,p1,p2)"""
        out = torch.empty_like(px)
        check(lib.alva_undistort_points(self.h, _ptr(px), px.shape[0], *[float(v) for v in K], *[float(v) for v in dist], _ptr(out)))
        return out

    def project_dist(self, cam_pts, K, dist):
        """CameraCalibration::projectCamToImageDist for n camera-frame points [n,3] f64 -> [n,2] f32 pixels"""
        out = torch.empty((cam_pts.shape[0], 2), dtype=torch.float32, device=cam_pts.device)
        check(lib.alva_project_dist(self.h, _ptr(cam_pts), cam_pts.shape[0], *[float(v) for v in K], *[float(v) for v in dist], _ptr(out)))
        return out

    # f4a
    def clahe(self, gray, clip_limit=3.0, tiles=None, tile_size=50):
        """cv::createCLAHE(clip, tiles)->apply; default grid = size / 50 as VisualFrontend builds it"""
        h, w = gray.shape
        tx, ty = tiles if tiles is not None else (w // tile_size, h // tile_size)
        out = torch.empty_like(gray)
        check(lib.alva_clahe(self.h, _ptr(gray), gray.stride(0), w, h, float(clip_limit), int(tx), int(ty), _ptr(out), out.stride(0)))
        return out

    # f2a
    def triangulate(self, T, group, bvl, bvr, unpxl, unpxr, K, max_reproj_err=3.0):
        """Mapper::triangulateTemporal per keypoint: returns dict(lpt, wpt, inv_depth, status, parallax) of cuda tensors."""
        n = bvl.shape[0]
        dev = bvl.device
        out = dict(lpt=torch.empty((n, 3), dtype=torch.float64, device=dev), wpt=torch.empty((n, 3), dtype=torch.float64, device=dev),
                   inv_depth=torch.empty(n, dtype=torch.float64, device=dev), status=torch.empty(n, dtype=torch.uint8, device=dev),
                   parallax=torch.empty(n, dtype=torch.float64, device=dev))
        check(lib.alva_triangulate(self.h, n, _ptr(T), T.shape[0], _ptr(group), _ptr(bvl), _ptr(bvr), _ptr(unpxl), _ptr(unpxr),
                                   K[0], K[1], K[2], K[3], max_reproj_err, _ptr(out["lpt"]), _ptr(out["wpt"]), _ptr(out["inv_depth"]),
                                   _ptr(out["status"]), _ptr(out["parallax"])))
        return out

    def wait_for(self, producer: "Context"):
        """stream-order dependency on another context's enqueued work (no host wait)"""
        check(lib.alva_ctx_wait(self.h, producer.h))

    # a8 + a9 chained
    def compute_pose(self, bearings, uv, wpts, K, p3p_iters=100, p3p_err=3.0, pnp_iters=5, chi2th=5.9915, do_random=False, seed=12345):
        """VisualFrontend::computePose: returns (status 0/1/2, pose7, p3p_outlier mask, pnp_outlier mask)."""
        import numpy as np
        n = bearings.shape[0]
        pose = np.zeros(7)
        m1 = np.zeros(max(n, 1), np.uint8)
        m2 = np.zeros(max(n, 1), np.uint8)
        st = C.c_int(0)
        check(lib.alva_compute_pose(self.h, _ptr(bearings), _ptr(uv), _ptr(wpts), n, p3p_iters, p3p_err, int(do_random), seed, pnp_iters,
                                    chi2th, K[0], K[1], K[2], K[3], pose.ctypes.data, m1.ctypes.data, m2.ctypes.data, C.byref(st)))
        return st.value, pose, m1[:n].astype(bool), m2[:n].astype(bool)

    def compute_pose_enqueue(self, bearings, uv, wpts, K, p3p_iters=100, p3p_err=3.0, pnp_iters=5, chi2th=5.9915, do_random=False,
                             seed=12345):
        self._pose_n = bearings.shape[0]
        self._pose_keep = (bearings, uv, wpts)
        check(lib.alva_compute_pose_enqueue(self.h, _ptr(bearings), _ptr(uv), _ptr(wpts), self._pose_n, p3p_iters, p3p_err, int(do_random),
                                            seed, pnp_iters, chi2th, K[0], K[1], K[2], K[3]))

    def compute_pose_collect(self):
        import numpy as np
        n = self._pose_n
        pose = np.zeros(7)
        m1 = np.zeros(max(n, 1), np.uint8)
        m2 = np.zeros(max(n, 1), np.uint8)
        st = C.c_int(0)
        check(lib.alva_compute_pose_collect(self.h, pose.ctypes.data, m1.ctypes.data, m2.ctypes.data, C.byref(st)))
        self._pose_keep = None
        return st.value, pose, m1[:n].astype(bool), m2[:n].astype(bool)

    # a6
    def orb_blur(self, gray, out=None):
        """gray [h,w] uint8 and out [h,w] uint8 (default: a new tensor) may be views with any row pitch and start"""
        h, w = gray.shape
        if out is None:
            out = torch.empty((h, w), dtype=torch.uint8, device=gray.device)
        assert tuple(out.shape) == (h, w)
        check(lib.alva_orb_blur(self.h, _ptr(gray), _gray_pitch(gray), w, h, _ptr(out), _gray_pitch(out)))
        return out

    def describe(self, gray, pts):
        """FeatureExtractor::describeFeaturePoints: returns (desc [n,32] u8, valid [n] u8)."""
        h, w = gray.shape
        n = pts.shape[0]
        assert pts.dtype == torch.float32 and pts.is_contiguous()
        desc = torch.empty((n, 32), dtype=torch.uint8, device=gray.device)
        valid = torch.empty(n, dtype=torch.uint8, device=gray.device)
        check(lib.alva_describe(self.h, _ptr(gray), gray.stride(0), w, h, _ptr(pts), n, _ptr(desc), _ptr(valid)))
        return desc, valid

    # a7
    def bf_match_hamming(self, query, train):
        nq, nt = query.shape[0], train.shape[0]
        assert query.dtype == torch.uint8 and query.shape[1] == 32 and query.is_contiguous()
        assert train.dtype == torch.uint8 and train.shape[1] == 32 and train.is_contiguous()
        idx = torch.empty(nq, dtype=torch.int32, device=query.device)
        dist = torch.empty(nq, dtype=torch.int32, device=query.device)
        check(lib.alva_bf_match_hamming(self.h, _ptr(query), nq, _ptr(train), nt, _ptr(idx), _ptr(dist)))
        return idx, dist

    # relocalization: global k = 2 match against a map record block (alva_reloc_match)
    def reloc_match(self, query, rows, valid=None, max_dist=51, ratio=0.8, bv=None, unpx=None, wpt=True):
        """query [n][32] uint8, rows [m][64] uint8 (alva_pack_map_records layout), valid [n] uint8 or None, bv [n][3] float64 /
        unpx [n][2] float32 or None (all on the device).  Returns (match [k][4] int32 = query, row, id, distance in ascending query
        index, gathered bv [k][3], uv [k][2], wpt [k][3] as float64 -- the first two None without their inputs, the third None with
        wpt=False); synchronises."""
        nq, nr = query.shape[0], rows.shape[0]
        assert query.dtype == torch.uint8 and query.shape[1] == 32 and query.is_contiguous()
        assert rows.dtype == torch.uint8 and rows.shape[1] == 64 and rows.is_contiguous()
        dev = query.device
        match = torch.empty((max(nq, 1), 4), dtype=torch.int32, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        obv = torch.empty((max(nq, 1), 3), dtype=torch.float64, device=dev) if bv is not None else None
        ouv = torch.empty((max(nq, 1), 2), dtype=torch.float64, device=dev) if unpx is not None else None
        owpt = torch.empty((max(nq, 1), 3), dtype=torch.float64, device=dev) if wpt else None
        check(lib.alva_reloc_match(self.h, _ptr(query), _ptr(valid), nq, _ptr(bv), _ptr(unpx), _ptr(rows) if nr else None, nr, int(max_dist),
                                   float(ratio), _ptr(match), _ptr(count), _ptr(obv), _ptr(ouv), _ptr(owpt)))
        self.sync()
        k = int(count.item())
        return match[:k], (obv[:k] if obv is not None else None), (ouv[:k] if ouv is not None else None), (owpt[:k] if owpt is not None else None)


class Pyramid:
    """alva_pyramid: padded gray + Scharr-derivative levels resident in HBM."""

    def __init__(self, ctx: Context, width: int, height: int, win: int = 9, max_level: int = 3):
        self.ctx = ctx
        self.win = win
        self.width, self.height = width, height
        h = _vp()
        check(lib.alva_pyramid_create(ctx.h, width, height, win, max_level, C.byref(h)))
        self.h = h
        self.num_levels = lib.alva_pyramid_num_levels(self.h)

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            lib.alva_pyramid_destroy(self.h)
            self.h = None

    __del__ = close

    def build_from_gray(self, gray):
        assert tuple(gray.shape) == (self.height, self.width)
        check(lib.alva_pyramid_build_from_gray(self.ctx.h, self.h, _ptr(gray), _gray_pitch(gray)))

    def build_from_rgba(self, rgba, gray_out=None):
        """rgba [h,w,4] uint8 and gray_out [h,w] uint8 may be views with padded rows, each with its own pitch"""
        assert tuple(rgba.shape) == (self.height, self.width, 4) and (gray_out is None or tuple(gray_out.shape) == (self.height, self.width))
        check(lib.alva_pyramid_build_from_rgba(self.ctx.h, self.h, _ptr(rgba), _rgba_pitch(rgba), _ptr(gray_out), _gray_pitch(gray_out)))

    def level(self, l: int) -> PyrLevel:
        info = PyrLevel()
        check(lib.alva_pyramid_level(self.h, l, C.byref(info)))
        return info

    def download_level(self, l: int):
        """Returns (gray_padded u8 [H+2w, W+2w], deriv_padded i16 [H+2w, W+2w, 2]) as numpy (tests)."""
        import numpy as np
        info = self.level(l)
        W, H = info.width + 2 * self.win, info.height + 2 * self.win
        g = np.empty((H, W), np.uint8)
        d = np.empty((H, W, 2), np.int16)
        check(lib.alva_pyramid_download_level(self.ctx.h, self.h, l, g.ctypes.data, d.ctypes.data))
        return g, d


class Orb:
    """alva_orb: cv::ORB::create(nfeatures, scale, nlevels, 31, 0, 2, HARRIS_SCORE, 31, fast_threshold)."""

    def __init__(self, ctx: Context, width: int, height: int, nfeatures: int = 2000, scale: float = 1.2, nlevels: int = 8,
                 fast_threshold: int = 20):
        self.ctx = ctx
        self.nfeatures = nfeatures
        h = _vp()
        check(lib.alva_orb_create(ctx.h, width, height, nfeatures, scale, nlevels, fast_threshold, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            lib.alva_orb_destroy(self.h)
            self.h = None

    __del__ = close

    def enqueue(self, gray, kp_buf, desc_buf, ctx=None):
        """detectAndCompute without the host wait, into caller-owned buffers (kp_buf [cap,6] f32, desc_buf [cap,32] u8)."""
        self._pending = (ctx or self.ctx, kp_buf, desc_buf)
        check(lib.alva_orb_detect_and_compute(self._pending[0].h, self.h, _ptr(gray), gray.stride(0), _ptr(kp_buf), _ptr(desc_buf),
                                              kp_buf.shape[0], None))

    def collect(self):
        """wait for enqueue(): returns (kp[:n], desc[:n]) views of the caller's buffers"""
        ctx, kp, desc = self._pending
        cnt = C.c_int(0)
        check(lib.alva_orb_collect(ctx.h, self.h, C.byref(cnt)))
        n = min(cnt.value, kp.shape[0])
        return kp[:n], (desc[:n] if desc is not None else None)

    def level(self, l: int, blurred: bool = False):
        """level l of the pyramid the last run built (blurred: its 7x7 blur) as a cuda uint8 tensor [h, w] (alva_orb_debug_level)"""
        w, h = C.c_int(0), C.c_int(0)
        check(lib.alva_orb_debug_level(self.ctx.h, self.h, l, int(blurred), None, 0, C.byref(w), C.byref(h)))
        out = torch.empty((h.value, w.value), dtype=torch.uint8, device=f"cuda:{self.ctx.device}")
        check(lib.alva_orb_debug_level(self.ctx.h, self.h, l, int(blurred), _ptr(out), out.stride(0), None, None))
        return out

    def detect_and_compute(self, gray, describe=True, cap=None):
        """returns (kp [n,6] float32 {x,y,size,angle,response,octave}, desc [n,32] u8) cuda tensors"""
        if cap is None:
            cap = 4 * self.nfeatures + 1024
        kp = torch.zeros((cap, 6), dtype=torch.float32, device=gray.device)
        desc = torch.zeros((cap, 32), dtype=torch.uint8, device=gray.device) if describe else None
        cnt = C.c_int(0)
        check(lib.alva_orb_detect_and_compute(self.ctx.h, self.h, _ptr(gray), gray.stride(0), _ptr(kp), _ptr(desc), cap, C.byref(cnt)))
        n = min(cnt.value, cap)
        return kp[:n], (desc[:n] if describe else None)


class Frontend:
    """alva_frontend: native per-frame driver (VisualFrontend::trackMono order) over two HIP streams."""

    def __init__(self, device: int, width: int, height: int, max_tracked: int, orb_features: int = 2000):
        import numpy as np
        h = _vp()
        check(lib.alva_frontend_create(device, width, height, max_tracked, orb_features, C.byref(h)))
        self.h = h
        self.device = device
        self.cap = 4 * orb_features + 1024
        self.max_tracked = max_tracked
        self._pose = np.zeros(7)
        self._st = C.c_int(0)
        self._nkp = C.c_int(0)

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            lib.alva_frontend_destroy(self.h)
            self.h = None

    __del__ = close

    def track(self, rgba, pts, bearings, uv, wpts, K, rgba_next=None, look_ahead=True):
        """returns (pose status 0/1/2, pose7 numpy (a view, overwritten by the next call), number of ORB keypoints).
        rgba_next: the frame the next call will pass as rgba (its gray + pyramid are built on a third stream meanwhile); it shares
        rgba's row pitch.  look_ahead=False with no rgba_next goes through alva_frontend_track itself."""
        pitch = _rgba_pitch(rgba, rgba_next)
        if rgba_next is None and not look_ahead:
            check(lib.alva_frontend_track(self.h, _ptr(rgba), pitch, _ptr(pts), pts.shape[0], _ptr(bearings), _ptr(uv), _ptr(wpts),
                                          bearings.shape[0], K[0], K[1], K[2], K[3], self._pose.ctypes.data, C.byref(self._st),
                                          C.byref(self._nkp)))
            self._npts = pts.shape[0]
            return self._st.value, self._pose, self._nkp.value
        check(lib.alva_frontend_track_ahead(self.h, _ptr(rgba), pitch, None if rgba_next is None else _ptr(rgba_next), _ptr(pts),
                                            pts.shape[0], _ptr(bearings), _ptr(uv), _ptr(wpts), bearings.shape[0], K[0], K[1], K[2], K[3],
                                            self._pose.ctypes.data, C.byref(self._st), C.byref(self._nkp)))
        self._npts = pts.shape[0]
        return self._st.value, self._pose, self._nkp.value

    def sync(self):
        check(lib.alva_frontend_sync(self.h))

    def results(self):
        """dict of torch views (no copy) of the device-resident results of the last track(); call sync() before reading"""
        ptrs = [_vp() for _ in range(6)]
        check(lib.alva_frontend_results(self.h, *[C.byref(p) for p in ptrs]))
        n, m = self._npts, self._nkp.value

        def view(ptr, shape, dtype):
            import numpy as np
            nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
            if nbytes == 0:
                return torch.empty(shape, dtype=dtype, device=f"cuda:{self.device}")
            class _W:
                pass
            w = _W()
            typestr = {torch.float32: "<f4", torch.uint8: "|u1", torch.int32: "<i4"}[dtype]
            w.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (ptr.value, False), "version": 2}
            return torch.as_tensor(w, device=f"cuda:{self.device}")
        return {"tracked": view(ptrs[0], (n, 2), torch.float32), "status": view(ptrs[1], (n,), torch.uint8),
                "keypoints": view(ptrs[2], (m, 6), torch.float32), "descriptors": view(ptrs[3], (m, 32), torch.uint8),
                "match_idx": view(ptrs[4], (m,), torch.int32), "match_dist": view(ptrs[5], (m,), torch.int32)}


def fbklt_track_batch(ctx: "Context", prevs, currs, pts, priors, num_levels=3, lanes=5, err_thresh=30.0, fb_dist=0.5, max_iters=30, eps=0.01):
    """alva_fbklt_track_batch: returns (list of tracked [n,2] f32 tensors, list of status [n] u8 tensors); priors are not modified."""
    n = len(prevs)
    outs = [p.clone() for p in priors]
    sts = [torch.empty((p.shape[0],), dtype=torch.uint8, device=p.device) for p in pts]
    arr = lambda v: (_vp * n)(*v)
    check(lib.alva_fbklt_track_batch(ctx.h, arr([p.h for p in prevs]), arr([p.h for p in currs]), n, num_levels, err_thresh, fb_dist, max_iters, eps,
                                     arr([_ptr(p) for p in pts]), arr([_ptr(o) for o in outs]), arr([_ptr(s_) for s_ in sts]),
                                     (_i * n)(*[p.shape[0] for p in pts]), lanes))
    return outs, sts


def orb_enqueue_batch(ctx: "Context", orbs, grays, kp_bufs, desc_bufs, cap, gray_pitch=None):
    """alva_orb_detect_and_compute_batch into caller-owned buffers (per camera kp [>= cap,6] f32, desc [>= cap,32] u8); no host wait.
    gray_pitch defaults to the row stride of the images, which must then all share it (views with padded rows are fine)."""
    n = len(orbs)
    if gray_pitch is None:
        gray_pitch = _gray_pitch(*grays)
    arr = lambda v: (_vp * n)(*v)
    check(lib.alva_orb_detect_and_compute_batch(ctx.h, arr([None if o is None else o.h for o in orbs]), n, arr([_ptr(g) for g in grays]),
                                                int(gray_pitch), arr([_ptr(k) for k in kp_bufs]), arr([_ptr(d) for d in desc_bufs]), int(cap)))


def orb_collect_batch(ctx: "Context", orbs):
    """alva_orb_collect_batch: waits for orb_enqueue_batch, returns every camera's keypoint count (what it FOUND, which may exceed cap)"""
    n = len(orbs)
    counts = (_i * max(n, 1))()
    check(lib.alva_orb_collect_batch(ctx.h, (_vp * n)(*[o.h for o in orbs]), n, counts))
    return list(counts)[:n]


def orb_detect_and_compute_batch(ctx: "Context", orbs, grays, cap):
    """cv::ORB::detectAndCompute of len(orbs) cameras in one set of launches: returns per camera (kp[:n] [n,6] f32, desc[:n] [n,32] u8)"""
    dev = f"cuda:{ctx.device}"
    kps = [torch.zeros((cap, 6), dtype=torch.float32, device=dev) for _ in orbs]
    descs = [torch.zeros((cap, 32), dtype=torch.uint8, device=dev) for _ in orbs]
    orb_enqueue_batch(ctx, orbs, grays, kps, descs, cap)
    counts = orb_collect_batch(ctx, orbs)
    return [(k[:min(c, cap)], d[:min(c, cap)]) for k, d, c in zip(kps, descs, counts)]


def bf_match_hamming_batch(ctx: "Context", queries, n_query_dev, cap_query, trains, n_train, idx_out, dist_out, expected_queries):
    """alva_bf_match_hamming_batch: len(queries) matches in one pair of launches, enqueue-only (the caller syncs).  Per match: queries
    [.,32] u8, n_query_dev a device int32 holding their number, train set [.,32] u8 with n_train rows known to the host, caller-allocated
    idx_out / dist_out [cap_query] int32.  Every tensor of a match whose n_train is 0 may be None."""
    n = len(queries)
    arr = lambda v: (_vp * n)(*[_ptr(t) for t in v])
    check(lib.alva_bf_match_hamming_batch(ctx.h, n, arr(queries), arr(n_query_dev), int(cap_query), arr(trains), (_i * n)(*[int(v) for v in n_train]),
                                          arr(idx_out), arr(dist_out), int(expected_queries)))


class TrackBatch:
    """alva_track_batch: trackMono (preprocessImage -> kltTracking -> computePose) of B lock-step cameras, one launch per stage."""

    def __init__(self, device: int, width: int, height: int, cameras: int, max_tracked: int, max_corr: int):
        import numpy as np
        h = _vp()
        check(lib.alva_track_batch_create(device, width, height, cameras, max_tracked, max_corr, C.byref(h)))
        self.h, self.device, self.B = h, device, cameras
        self.poses = np.zeros((cameras, 7))
        self.status = np.zeros(cameras, np.int32)
        self._n_pts = [0] * cameras
        self._args = None

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            lib.alva_track_batch_destroy(self.h)
            self.h = None

    __del__ = close

    def bind(self, pts, bearings, uv, wpts):
        """pointer tables of the per-camera inputs that stay put between frames (lists of cuda tensors, one per camera)"""
        B = self.B
        arr = lambda ts: (_vp * B)(*[_ptr(t) if t is not None and t.numel() else None for t in ts])
        self._args = (arr(pts), (_i * B)(*[0 if t is None else t.shape[0] for t in pts]), arr(bearings), arr(uv), arr(wpts),
                      (_i * B)(*[0 if t is None else t.shape[0] for t in bearings]))
        self._n_pts = [0 if t is None else t.shape[0] for t in pts]
        self._keep = (pts, bearings, uv, wpts)

    def step(self, rgbas, K, plain=False):
        """rgbas: list of B [H,W,4] u8 cuda tensors that share one row pitch (views with padded rows are fine).  Returns (status[B],
        poses[B,7]) -- views, overwritten by the next step.  plain: through alva_track_batch_step, which returns no keypoint counts."""
        a_pts, a_np, a_bv, a_uv, a_wp, a_nc = self._args
        assert len(rgbas) == self.B
        pitch = _rgba_pitch(*rgbas)
        fr = (_vp * self.B)(*[_ptr(r) for r in rgbas])
        if plain:
            check(lib.alva_track_batch_step(self.h, fr, pitch, a_pts, a_np, a_bv, a_uv, a_wp, a_nc, K[0], K[1], K[2], K[3],
                                            self.poses.ctypes.data, self.status.ctypes.data))
            return self.status, self.poses
        check(lib.alva_track_batch_step_detect(self.h, fr, pitch, a_pts, a_np, a_bv, a_uv, a_wp, a_nc, K[0], K[1], K[2], K[3],
                                               self.poses.ctypes.data, self.status.ctypes.data,
                                               self.nkp.ctypes.data if getattr(self, "nkp", None) is not None else None))
        return self.status, self.poses

    def enable_detector(self, orb_features: int = 2000):
        import numpy as np
        check(lib.alva_track_batch_enable_detector(self.h, orb_features))
        self.nkp = np.zeros(self.B, np.int32)
        self.cap = 4 * orb_features + 1024

    def detections(self, cam: int):
        """dict of torch views of one camera's detector results of the last step (keypoints [n,6], descriptors [n,32], match idx/dist [n])"""
        ptrs = [_vp() for _ in range(4)]
        check(lib.alva_track_batch_detections(self.h, cam, *[C.byref(p) for p in ptrs]))
        n = int(self.nkp[cam])
        return {"keypoints": _dev_view(ptrs[0], (n, 6), torch.float32, self.device), "descriptors": _dev_view(ptrs[1], (n, 32), torch.uint8, self.device),
                "match_idx": _dev_view(ptrs[2], (n,), torch.int32, self.device), "match_dist": _dev_view(ptrs[3], (n,), torch.int32, self.device)}

    def frame_table(self, rgbas):
        """pointer table of one set of B frames for step_table() (build once per resident frame set: a Python list comprehension
        over 64 tensors costs more than the whole GPU step)"""
        assert len(rgbas) == self.B
        return (_vp * self.B)(*[_ptr(r) for r in rgbas]), _rgba_pitch(*rgbas), rgbas

    def step_table(self, table, K):
        a_pts, a_np, a_bv, a_uv, a_wp, a_nc = self._args
        check(lib.alva_track_batch_step_detect(self.h, table[0], table[1], a_pts, a_np, a_bv, a_uv, a_wp, a_nc, K[0], K[1], K[2], K[3],
                                               self.poses.ctypes.data, self.status.ctypes.data,
                                               self.nkp.ctypes.data if getattr(self, "nkp", None) is not None else None))
        return self.status, self.poses

    def results(self, cam: int):
        """(tracked [n,2] f32, status [n] u8) of one camera: torch views of device memory, valid until the next step"""
        p, q = _vp(), _vp()
        check(lib.alva_track_batch_results(self.h, cam, C.byref(p), C.byref(q)))
        n = self._n_pts[cam]
        return _dev_view(p, (n, 2), torch.float32, self.device), _dev_view(q, (n,), torch.uint8, self.device)

    def ctx_handle(self):
        return lib.alva_track_batch_ctx(self.h)

    def set_klt_lanes(self, lanes: int):
        check(lib.alva_track_batch_set_klt_lanes(self.h, lanes))

    def stats(self):
        """(steps done, cameras re-solved through the single-camera call)"""
        a, b = C.c_long(0), C.c_long(0)
        check(lib.alva_track_batch_stats(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value


def _dev_view(ptr, shape, dtype, device):
    import numpy as np
    if int(np.prod(shape)) == 0:
        return torch.empty(shape, dtype=dtype, device=f"cuda:{device}")

    class _W:
        pass
    w = _W()
    typestr = {torch.float32: "<f4", torch.uint8: "|u1", torch.int32: "<i4"}[dtype]
    w.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (ptr.value, False), "version": 2}
    return torch.as_tensor(w, device=f"cuda:{device}")


def build_pyramids_batch(ctx: "Context", pyrs, rgbas, grays=None):
    """alva_pyramid_build_from_rgba_batch: all cameras' gray + LK pyramid in five launches.  The frames share one row pitch and the gray
    outputs another (views with padded rows are fine)."""
    n = len(pyrs)
    assert len(rgbas) == n and (grays is None or len(grays) == n)
    ph = (_vp * n)(*[p.h for p in pyrs])
    pr = (_vp * n)(*[_ptr(r) for r in rgbas])
    pg = None if grays is None else (_vp * n)(*[_ptr(g) for g in grays])
    check(lib.alva_pyramid_build_from_rgba_batch(ctx.h, ph, pr, _rgba_pitch(*rgbas), pg, 0 if grays is None else _gray_pitch(*grays), n))


def relpose_draw_samples(n_points: int, count: int, do_random: bool = False, seed: int = 12345):
    import numpy as np
    s = np.zeros((count, 8), np.int32)
    check(lib.alva_relpose_draw_samples(n_points, count, int(do_random), seed, s.ctypes.data))
    return s


def kernel_times(fn, reps: int):
    """Run fn() reps times with per-kernel HIP-event timing on; returns {kernel: (launches, average microseconds)}."""
    check(lib.alva_prof_enable(1))
    try:
        for _ in range(reps):
            fn()
    finally:
        check(lib.alva_prof_enable(0))
    buf = C.create_string_buffer(1 << 16)
    check(lib.alva_prof_report(buf, len(buf)))
    out = {}
    for line in buf.value.decode().splitlines():
        name, calls, us = line.split("\t")
        out[name] = (int(calls), float(us))
    return out


def frontend_run_many(fes, steps, warmup, frames, pts, bearings, uv, wpts, K):
    """fes: list of Frontend; frames: list (per stream) of [ring,H,W,4] u8 cuda tensors; pts/bearings/uv/wpts: per-stream tensors.
    Returns (seconds, accepted poses)."""
    n = len(fes)
    ring = frames[0].shape[0]
    arr = lambda ptrs: (_vp * len(ptrs))(*ptrs)
    a_fe = arr([f.h.value for f in fes])
    a_fr = arr([frames[s][k].data_ptr() for s in range(n) for k in range(ring)])
    a_pts, a_bv, a_uv, a_wp = (arr([t[s].data_ptr() for s in range(n)]) for t in (pts, bearings, uv, wpts))
    secs, acc = C.c_double(0), C.c_int(0)
    check(lib.alva_frontend_run_many(a_fe, n, steps, warmup, a_fr, ring, frames[0].stride(1), a_pts, pts[0].shape[0], a_bv, a_uv, a_wp,
                                     bearings[0].shape[0], K[0], K[1], K[2], K[3], C.byref(secs), C.byref(acc)))
    return secs.value, acc.value


import numpy as np  # noqa: E402  (MedoidStore builds its operation records with numpy)


class MedoidStore:
    """alva_medoid_store (include/alvaar_hip.h, f1): the map points' descriptor tables on the device, edited by replaying operation logs.
    ops: list of (mp_slot, op, kf, desc32 | None, rehash_to) in program order (op 0 add, 1 remove, 2 clear, 3 reset)."""
    OP = np.dtype([("op", "<i4"), ("kf", "<i4"), ("rehash_to", "<i4"), ("next", "<i4"), ("desc", "u1", 32), ("pad", "<i4", 4)])
    TABLE_SLOT = np.dtype([("key", "<i4"), ("next", "<i4"), ("dist", "<f4"), ("pad", "<i4"), ("desc", "u1", 32)])

    def __init__(self, ctx: "Context"):
        lib.alva_medoid_store_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        lib.alva_medoid_store_destroy.argtypes = [C.c_void_p]
        lib.alva_medoid_store_destroy.restype = None
        lib.alva_medoid_replay.argtypes = [C.c_void_p, _i, C.c_void_p, _i, C.c_void_p, C.c_void_p, _i]
        lib.alva_medoid_export.argtypes = [C.c_void_p, _i, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.alva_medoid_dump.argtypes = [C.c_void_p, _i, C.c_void_p, C.c_size_t]
        lib.alva_medoid_table_bytes.restype = C.c_size_t
        lib.alva_medoid_op_bytes.restype = C.c_size_t
        assert lib.alva_medoid_op_bytes() == self.OP.itemsize
        self.ctx = ctx
        self.h = C.c_void_p()
        check(lib.alva_medoid_store_create(ctx.h, C.byref(self.h)))

    def replay(self, ops, slots: int):
        rec = np.zeros(len(ops), self.OP)
        first, last, touched = {}, {}, []
        for i, (slot, op, kf, desc, rehash_to) in enumerate(ops):
            rec[i]["op"], rec[i]["kf"], rec[i]["rehash_to"], rec[i]["next"] = op, kf, rehash_to, -1
            if desc is not None:
                rec[i]["desc"] = desc
            if slot in last:
                rec[last[slot]]["next"] = i
            else:
                first[slot] = i
                touched.append(slot)
            last[slot] = i
        mp = np.array(touched, np.int32)
        fo = np.array([first[s] for s in touched], np.int32)
        check(lib.alva_medoid_replay(self.h, len(ops), rec.ctypes.data, len(mp), mp.ctypes.data, fo.ctypes.data, int(slots)))

    def export(self, slots):
        s = np.ascontiguousarray(slots, np.int32)
        desc, valid, info = np.zeros((len(s), 32), np.uint8), np.zeros(len(s), np.uint8), np.zeros((len(s), 3), np.int32)
        check(lib.alva_medoid_export(self.h, len(s), s.ctypes.data, desc.ctypes.data, valid.ctypes.data, info.ctypes.data))
        return desc, valid, info

    def dump_raw(self, slot: int):
        """the bytes of one map point's table (layout: csrc/slam/medoid_table.hpp)"""
        n = lib.alva_medoid_table_bytes()
        raw = np.zeros(n, np.uint8)
        check(lib.alva_medoid_dump(self.h, int(slot), raw.ctypes.data, n))
        return raw

    def dump(self, slot: int):
        """the raw table of one map point -> (medoid bytes, has medoid, [(key, dist)] in the container's iteration order, bucket count)"""
        raw = self.dump_raw(slot)
        n = raw.size
        hdr = raw[:32].view(np.int32)   # head, free, count, nbkt, used, medoid_valid, overflow, medoid_kf
        cap = 48                        # alva_medoid::CAP (csrc/slam/medoid_table.hpp): 64-byte header | CAP slots | 59 bucket heads + pad
        assert n == 64 + cap * self.TABLE_SLOT.itemsize + 60 * 4, "medoid table layout changed"
        slots = raw[64:64 + cap * self.TABLE_SLOT.itemsize].view(self.TABLE_SLOT)
        out, s = [], int(hdr[0])
        while s != -1 and len(out) <= cap:
            out.append((int(slots[s]["key"]), float(slots[s]["dist"])))
            s = int(slots[s]["next"])
        return raw[32:64].copy(), bool(hdr[5]), out, int(hdr[3]), bool(hdr[6])

    def pack_records(self, chunk_table, n_slots: int, stream_id: int, capacity: int, out) -> int:
        """alva_pack_map_records: the 3-D map points with a descriptor among record slots 0 .. n_slots - 1 as 64-byte exchange rows
        {int32 stream, int32 id, f64 xyz[3], u8 medoid[32]} in `out` [capacity][64] uint8 (cuda), unused rows with id -1.  chunk_table is a
        cuda int64 tensor of the record chunks' addresses (4096 records of Context.mp_record_dtype() per chunk, as match_to_map_records
        takes it).  Returns the number of points found; beyond `capacity` only `capacity` of them were written."""
        lib.alva_pack_map_records.argtypes = [C.c_void_p, C.c_void_p, _i, _i, _i, C.c_void_p, C.POINTER(_i)]
        assert chunk_table.dtype == torch.int64 and chunk_table.is_cuda and chunk_table.shape[0] * 4096 >= n_slots
        assert out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous() and out.numel() >= 64 * capacity
        n = _i(0)
        check(lib.alva_pack_map_records(self.h, _ptr(chunk_table), int(n_slots), int(stream_id), int(capacity), _ptr(out), C.byref(n)))
        return n.value

    def close(self):
        if self.h:
            lib.alva_medoid_store_destroy(self.h)
            self.h = C.c_void_p()

    __del__ = close


# ---- test-only: single tracking steps (include/alvaar_system_testing.h, csrc/track_probe.hip) ----------------------------------
class TrackProbeJob(C.Structure):
    _fields_ = [("n", _i), ("px", _vp), ("is3d", _vp), ("wpt", _vp), ("carry", _vp), ("Tcw_q", _d * 4), ("Tcw_t", _d * 3),
                ("use_prior", _i), ("klt_levels", _i), ("want_pose", _i), ("do_p3p", _i), ("do_random", _i), ("table_route", _i)]


class TrackProbeOut(C.Structure):
    _fields_ = [("code", _vp), ("px", _vp), ("unpx", _vp), ("bv", _vp), ("p3p_req", _i), ("n_pose", _i), ("status", _i),
                ("pose7_p3p", _d * 7), ("pose7", _d * 7), ("p3p_outlier", _vp), ("pnp_outlier", _vp), ("Pbv", _vp), ("Puv", _vp),
                ("Pwpt", _vp), ("info8", _i * 8)]


_sig("alva_track_probe_create", [_i, _i, _i, _vp, C.POINTER(_vp)])
_sig("alva_track_probe_destroy", [_vp], None)
_sig("alva_track_probe_frame", [_vp, _vp])
_sig("alva_track_probe_step", [_vp, C.POINTER(TrackProbeJob), C.POINTER(TrackProbeOut)])
_sig("alva_track_probe_solve_pose", [_vp, _i, _vp, _vp, _vp, _i, C.POINTER(_i), _vp, _vp, _vp, _vp])


class TrackProbeError(AlvaError):
    """a refused step, with the library's return code (ERR_ARG / ERR_STATE of include/alvaar_hip.h)"""
    ERR_ARG, ERR_STATE = -1, -4

    def __init__(self, rc, text):
        super().__init__(f"alvaar_hip error {rc}: {text}")
        self.rc = rc


class TrackProbe:
    """One set of stages without a map layer: frames in, single tracking steps (HipStages::track_begin + track_pose_collect) out."""
    INFO = ("route", "stage_in", "pose_all_queued", "pose_all_answer", "retry", "seq", "compact_launches", "reserved")

    def __init__(self, device, width, height, calib8):
        import numpy as np
        if not torch.cuda.is_available():
            raise AlvaError("no HIP device visible: the alvaar_amd hot path has no CPU fallback")
        k = np.ascontiguousarray(calib8, np.float64)
        assert k.shape == (8,)
        h = _vp()
        check(lib.alva_track_probe_create(device, width, height, k.ctypes.data, C.byref(h)))
        self.h, self.width, self.height = h, width, height

    def close(self):
        if getattr(self, "h", None) and lib is not None:
            lib.alva_track_probe_destroy(self.h)
            self.h = None

    __del__ = close

    def frame(self, rgba):
        import numpy as np
        rgba = np.ascontiguousarray(rgba, np.uint8)
        assert rgba.shape == (self.height, self.width, 4)
        check(lib.alva_track_probe_frame(self.h, rgba.ctypes.data))

    def step(self, n, Tcw_q, Tcw_t, px=None, is3d=None, wpt=None, carry=None, use_prior=1, klt_levels=3, want_pose=0, do_p3p=1,
             do_random=0, table_route=0):
        """-> dict(code, px, unpx, bv, p3p_req, n_pose, status, pose7_p3p, pose7, p3p_outlier, pnp_outlier, Pbv, Puv, Pwpt, info)"""
        import numpy as np
        job = TrackProbeJob()
        job.n = n
        keep = []
        for name, arr, dt, shape in (("px", px, np.float32, (n, 2)), ("is3d", is3d, np.uint8, (n,)), ("wpt", wpt, np.float64, (n, 3)),
                                     ("carry", carry, np.uint16, (n,))):
            if arr is None:
                continue
            a = np.ascontiguousarray(arr, dt)
            assert a.shape == shape, (name, a.shape, shape)
            keep.append(a)
            setattr(job, name, a.ctypes.data)
        job.Tcw_q[:] = [float(v) for v in Tcw_q]
        job.Tcw_t[:] = [float(v) for v in Tcw_t]
        job.use_prior, job.klt_levels, job.want_pose, job.do_p3p, job.do_random = use_prior, klt_levels, want_pose, do_p3p, do_random
        job.table_route = table_route
        m = max(n, 1)
        r = dict(code=np.zeros(m, np.uint8), px=np.zeros((m, 2), np.float32), unpx=np.zeros((m, 2), np.float32), bv=np.zeros((m, 3)),
                 p3p_outlier=np.zeros(m, np.uint8), pnp_outlier=np.zeros(m, np.uint8), Pbv=np.zeros((m, 3)), Puv=np.zeros((m, 2)),
                 Pwpt=np.zeros((m, 3)))
        out = TrackProbeOut()
        for name, a in r.items():
            setattr(out, name, a.ctypes.data)
        rc = lib.alva_track_probe_step(self.h, C.byref(job), C.byref(out))
        if rc != 0:
            raise TrackProbeError(rc, lib.alva_last_error().decode())
        n_pose = out.n_pose
        r = {k: (v[:n_pose] if k in ("p3p_outlier", "pnp_outlier", "Pbv", "Puv", "Pwpt") else v[:n]) for k, v in r.items()}
        r.update(p3p_req=out.p3p_req, n_pose=n_pose, status=out.status, pose7_p3p=np.array(out.pose7_p3p), pose7=np.array(out.pose7),
                 info=dict(zip(self.INFO, out.info8)))
        return r

    def solve_pose(self, bv, uv, wpt, do_random=0):
        """the stand-alone pose solve with the step's constants -> (status, pose7_p3p, pose7, p3p_outlier, pnp_outlier)"""
        import numpy as np
        bv, uv, wpt = (np.ascontiguousarray(a, np.float64) for a in (bv, uv, wpt))
        n = len(bv)
        assert bv.shape == (n, 3) and uv.shape == (n, 2) and wpt.shape == (n, 3)
        st = _i(0)
        p3p, pose = np.zeros(7), np.zeros(7)
        m1, m2 = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        check(lib.alva_track_probe_solve_pose(self.h, n, bv.ctypes.data, uv.ctypes.data, wpt.ctypes.data, do_random, C.byref(st),
                                              p3p.ctypes.data, pose.ctypes.data, m1.ctypes.data, m2.ctypes.data))
        return st.value, p3p, pose, m1, m2
