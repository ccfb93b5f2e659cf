"""Python mirror of the reference's JS wrapper class `AlvaAR` (src/system.js:45-238) over the alva_system_* C ABI
(include/alvaar_system.h): same method names, same intrinsics-from-FOV rule, same return conventions
(pose array or None).  It is the host-side caller of the drop-in boundary, used by tests."""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np

from .capi import lib, AlvaError

_vp, _i, _d = C.c_void_p, C.c_int, C.c_double
lib.alva_system_create.argtypes = [_i, C.POINTER(_vp)]
lib.alva_system_destroy.argtypes = [_vp]
lib.alva_system_destroy.restype = None
lib.alva_system_configure.argtypes = [_vp, _i, _i] + [_d] * 8
lib.alva_system_reset.argtypes = [_vp]
lib.alva_system_reset.restype = None
lib.alva_system_find_camera_pose.argtypes = [_vp, _vp, _vp]
lib.alva_system_find_camera_pose_with_imu.argtypes = [_vp, _vp, _vp, _vp]
lib.alva_system_find_camera_pose_with_imu_ts.argtypes = [_vp, _vp, _vp, C.c_double, _vp]
lib.alva_system_find_plane.argtypes = [_vp, _vp, _i]
lib.alva_system_get_frame_points.argtypes = [_vp, _vp]
lib.alva_system_get_keypoints.argtypes = [_vp, _vp, _vp, _vp, _i]
lib.alva_system_configure_ex.argtypes = [_vp, _i, _i] + [_d] * 8 + [_i] * 3
lib.alva_system_find_camera_pose_ts.argtypes = [_vp, _vp, _d, _vp]
lib.alva_system_register_frame_buffer.argtypes = [_vp, _vp, C.c_size_t]
lib.alva_system_unregister_frame_buffer.argtypes = [_vp]
if hasattr(lib, "alva_system_alloc_frame_buffer"):
    lib.alva_system_alloc_frame_buffer.argtypes = [_vp, C.c_size_t, C.POINTER(_vp)]
lib.alva_system_find_camera_pose_device.argtypes = [_vp, _vp, _d, _vp]
lib.alva_system_hint_next_frame_device.argtypes = [_vp, _vp]
lib.alva_system_debug_state.argtypes = [_vp, _vp]
lib.alva_system_debug_pose7.argtypes = [_vp, _vp, _vp]
lib.alva_system_debug_frame_keypoints.argtypes = [_vp, _i] + [_vp] * 5
lib.alva_system_debug_keyframe_ids.argtypes = [_vp, _i, _vp]
lib.alva_system_debug_keyframe.argtypes = [_vp, _i, _vp, _vp, _i, _vp, _vp, _vp]
lib.alva_system_debug_covisibility.argtypes = [_vp, _i, _i, _vp]
lib.alva_system_debug_map_points.argtypes = [_vp, _i] + [_vp] * 5
lib.alva_system_debug_counters.argtypes = [_vp, _vp]
lib.alva_system_merge_map_points.argtypes = [_vp, _i, _i]
lib.alva_system_set_shared_ids.argtypes = [_vp, _i, _vp, _vp, _vp]
lib.alva_system_get_shared_ids.argtypes = [_vp, _i, _vp, _vp, _vp]
lib.alva_system_debug_klt_work.argtypes = [_vp, _vp, _i]
lib.alva_system_debug_set_init_pose.argtypes = [_vp, _vp]
lib.alva_system_debug_timing.argtypes = [_vp, _vp, _i]
lib.alva_system_debug_timing_keyframe.argtypes = [_vp, _vp, _i]
lib.alva_system_debug_timing_fine.argtypes = [_vp, _vp, _i]
lib.alva_system_last_error.restype = C.c_char_p
lib.alva_system_group_create.argtypes = [_i, C.POINTER(_vp)]
lib.alva_system_group_destroy.argtypes = [_vp]
lib.alva_system_group_destroy.restype = None
lib.alva_system_group_find_camera_pose_device.argtypes = [_vp, _i, _vp, _vp, _d, _vp, _vp]
lib.alva_system_group_stream.argtypes = [_vp, _i, _i, C.POINTER(_vp)]
lib.alva_system_set_stream.argtypes = [_vp, _vp]
lib.alva_system_group_set_lockstep.argtypes = [_vp, _i]
lib.alva_system_group_launch_stats.argtypes = [_vp, _vp]
lib.alva_system_group_set_lanes.argtypes = [_vp, _i]
lib.alva_system_group_time_stats.argtypes = [_vp, _vp, _i]
if hasattr(lib, "alva_system_set_relocalization"):   # (an older build loaded through ALVA_LIB for an A/B measurement lacks them)
    lib.alva_system_set_relocalization.argtypes = [_vp, _i, _i]
    lib.alva_system_relocalization_stats.argtypes = [_vp, _vp]
if hasattr(lib, "alva_system_hit_test"):
    lib.alva_system_hit_test.argtypes = [_vp, _i, _vp, C.c_float, _i, _vp, _vp]
    lib.alva_system_debug_frame_map_point_ids.argtypes = [_vp, _i, _vp]
if hasattr(lib, "alva_system_depth"):
    lib.alva_system_set_depth.argtypes = [_vp, _i]
    lib.alva_system_depth.argtypes = [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp]
    lib.alva_system_debug_depth.argtypes = [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp]
    lib.alva_system_debug_depth_ring.argtypes = [_vp, _vp]
if hasattr(lib, "alva_system_depth_dense"):
    lib.alva_system_depth_dense.argtypes = [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp]
    lib.alva_system_debug_depth_dense.argtypes = [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp] + [_vp] * 11
    lib.alva_system_reset_depth_dense.argtypes = [_vp]
if hasattr(lib, "alva_system_mesh"):
    lib.alva_system_mesh_update.argtypes = [_vp, _i, _d, _i, _i, _i, _i, _i, _vp, _vp]
    lib.alva_system_debug_mesh_update.argtypes = [_vp, _i, _d, _i, _i, _i, _i, _i, _vp, _vp] + [_vp] * 6
    lib.alva_system_mesh.argtypes = [_vp, _i, _i, _i] + [_vp] * 5
    lib.alva_system_reset_mesh.argtypes = [_vp]
if hasattr(lib, "alva_system_mesh_raycast"):
    lib.alva_system_mesh_raycast.argtypes = [_vp, _i, _vp, _i, _d, _d] + [_vp] * 5
    lib.alva_system_mesh_depth.argtypes = [_vp, _vp, _i, _i, _vp, _vp, _vp, _i, _vp]
    lib.alva_system_mesh_hit_test.argtypes = [_vp, _i, _vp, _i, _vp, _vp]
if hasattr(lib, "alva_system_mesh_colored"):
    lib.alva_system_set_mesh_color.argtypes = [_vp, _i]
    lib.alva_system_mesh_colored.argtypes = [_vp, _i, _i, _i] + [_vp] * 6
    lib.alva_system_mesh_color_at.argtypes = [_vp, _i, _vp, _vp, _vp, _vp]
    lib.alva_system_debug_mesh_color.argtypes = [_vp, _vp, _vp]
if hasattr(lib, "alva_system_mesh_move"):
    lib.alva_system_set_mesh_follow.argtypes = [_vp, _i]
    lib.alva_system_mesh_move.argtypes = [_vp, _vp, _i, _vp, _vp]
    lib.alva_system_mesh_follow_stats.argtypes = [_vp, _vp]
if hasattr(lib, "alva_system_mesh_blocks"):
    lib.alva_system_mesh_blocks.argtypes = [_vp, _i, _i, _i, _i, _i, _i] + [_vp] * 9
    lib.alva_system_reset_mesh_blocks.argtypes = [_vp]
if hasattr(lib, "alva_system_light"):
    lib.alva_system_set_light.argtypes = [_vp, _i]
    lib.alva_system_light.argtypes = [_vp] * 6
    lib.alva_system_debug_light.argtypes = [_vp] * 10
    lib.alva_system_reset_light.argtypes = [_vp]
if hasattr(lib, "alva_system_detect_images"):
    lib.alva_system_add_image.argtypes = [_vp, _vp, _i, _i, C.c_size_t, _d]
    lib.alva_system_remove_image.argtypes = [_vp, _i]
    lib.alva_system_reset_images.argtypes = [_vp]
    lib.alva_system_detect_images.argtypes = [_vp, _i, C.c_float, _i, _i] + [_vp] * 6
    lib.alva_system_debug_detect_images.argtypes = [_vp, _i, C.c_float, _i, _i] + [_vp] * 7


class _ImageDebug(C.Structure):   # alva_image_debug of include/alvaar_system.h
    _fields_ = [(name, _vp) for name in ("n_frame", "kp", "unpx", "desc", "nq", "wh", "qxy", "qdesc", "match", "xy", "count", "H", "mask",
                                         "stage_info", "stage_R", "stage_t", "R", "t", "pose7", "tracked")]


if hasattr(lib, "alva_system_detect_planes"):
    lib.alva_system_detect_planes.argtypes = [_vp, C.c_double, _i, _i, _i, _vp, _vp, _vp, _vp, _i]
if hasattr(lib, "alva_system_track_planes"):
    lib.alva_system_track_planes.argtypes = [_vp, C.c_double, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp]
    lib.alva_system_reset_planes.argtypes = [_vp]
    lib.alva_system_reset_planes.restype = None
if hasattr(lib, "alva_system_create_anchors"):
    lib.alva_system_create_anchors.argtypes = [_vp, _i, _vp, _i, _vp, _vp]
    lib.alva_system_update_anchors.argtypes = [_vp, _i, _vp, _vp, _vp]
    lib.alva_system_remove_anchor.argtypes = [_vp, _i]
    lib.alva_system_reset_anchors.argtypes = [_vp]
    lib.alva_system_reset_anchors.restype = None
if hasattr(lib, "alva_system_detect_plane_outlines"):
    lib.alva_system_detect_plane_outlines.argtypes = [_vp, C.c_double, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp]


def camera_intrinsics(width: int, height: int, fov: float = 45.0):
    """AlvaAR.getCameraIntrinsics (src/system.js:84-141)"""
    aspect = width / height
    fov_h, fov_v = (fov * aspect, fov) if width > height else (fov, fov * aspect)
    deg2rad = 0.01745329251994329576
    fx = (width * 0.5) / math.tan(fov_h * 0.5 * deg2rad)
    fy = (height * 0.5) / math.tan(fov_v * 0.5 * deg2rad)
    f = min(fx, fy)
    return dict(width=width, height=height, fx=f, fy=f, cx=width * 0.5, cy=height * 0.5, k1=0.0, k2=0.0, p1=0.0, p2=0.0)


class AlvaAR:
    def __init__(self, width: int, height: int, fov: float = 45.0, device: int = 0, cell_size: int | None = None, clahe: bool = False,
                 random_sampling: bool = True, distortion=(0.0, 0.0, 0.0, 0.0), hip_stream=None, relocalization: bool = False,
                 max_lost_frames: int = 0, depth: bool = False, light: bool = False, mesh_color: bool = False, mesh_follow: int = 0):
        """cell_size / clahe / random_sampling: the settings System::configure hard-codes (system.cpp:15-19, state.hpp:67);
        None = the shipped configuration through alva_system_configure.  relocalization / max_lost_frames:
        alva_system_set_relocalization (off by default: tracking loss resets the map like the reference; on: status 4 while the
        frozen map is searched, status 2 after max_lost_frames (> 0) frames of 4).  depth: alva_system_set_depth (off by default; on:
        reference frames are kept for depthImage).  light: alva_system_set_light (off by default; on: every frame is binned into the
        session's environment map for lightEstimate).  mesh_color: alva_system_set_mesh_color (off by default; on, together with
        depth: every tracked frame's colour is kept as a thumbnail and meshUpdate fuses it into the volume, for mesh(colors=True) and
        meshColorAt).  mesh_follow: alva_system_set_mesh_follow (0 = off, the default; 1, 2, 4, 8, 16 or 32: meshUpdate shifts the
        volume in blocks of that many voxels so that it stays in front of the camera -- what leaves the cube is gone)."""
        self.intrinsics = camera_intrinsics(width, height, fov)
        self.intrinsics.update(dict(zip(("k1", "k2", "p1", "p2"), map(float, distortion))))
        h = _vp()
        rc = lib.alva_system_create(device, C.byref(h))
        if rc:
            raise AlvaError(lib.alva_system_last_error().decode())
        self.h = h
        if hip_stream is not None:   # a stream shared with other sessions (SystemGroup.stream)
            lib.alva_system_set_stream(h, hip_stream)
        if relocalization or max_lost_frames:
            rc = lib.alva_system_set_relocalization(h, int(bool(relocalization)), int(max_lost_frames))
            if rc:
                msg = lib.alva_system_last_error().decode()
                lib.alva_system_destroy(h)
                self.h = None
                raise AlvaError(msg)
        if depth:
            lib.alva_system_set_depth(h, 1)
        if light:
            lib.alva_system_set_light(h, 1)
        if mesh_color:
            if not hasattr(lib, "alva_system_set_mesh_color"):   # (an older build loaded through ALVA_LIB for an A/B measurement)
                lib.alva_system_destroy(h)
                self.h = None
                raise AlvaError("alva_system_set_mesh_color is not in the loaded library")
            lib.alva_system_set_mesh_color(h, 1)
        if mesh_follow:
            if not hasattr(lib, "alva_system_set_mesh_follow"):
                lib.alva_system_destroy(h)
                self.h = None
                raise AlvaError("alva_system_set_mesh_follow is not in the loaded library")
            if lib.alva_system_set_mesh_follow(h, int(mesh_follow)):
                msg = lib.alva_system_last_error().decode()
                lib.alva_system_destroy(h)
                self.h = None
                raise AlvaError(msg)
        k = self.intrinsics
        if cell_size is None and not clahe and random_sampling:
            rc = lib.alva_system_configure(h, width, height, k["fx"], k["fy"], k["cx"], k["cy"], k["k1"], k["k2"], k["p1"], k["p2"])
        else:
            rc = lib.alva_system_configure_ex(h, width, height, k["fx"], k["fy"], k["cx"], k["cy"], k["k1"], k["k2"], k["p1"], k["p2"],
                                              cell_size or 40, int(clahe), int(random_sampling))
        if rc:
            msg = lib.alva_system_last_error().decode()
            lib.alva_system_destroy(h)
            self.h = None
            raise AlvaError(msg)
        self._pose = np.zeros(16, np.float32)
        self._pose_ptr = self._pose.ctypes.data   # (ndarray.ctypes builds a helper object per access: ~1 us of every per-frame call)
        self._fcp_device = lib.alva_system_find_camera_pose_device
        # src/system.js:63-67: ONE frame buffer (memImg) allocated at construction and reused for every frame; here it is page-locked and
        # mapped once (alva_system_register_frame_buffer) so that the gray / pyramid kernel reads it in place.  4096-byte aligned.
        # Round 5: the buffer lives in DEVICE memory that the host writes over the PCIe BAR (alva_system_alloc_frame_buffer): memImg.write IS
        # the upload and the kernels read the frame out of HBM.  Never read mem_img back (a load crosses the bus).  ALVA_NO_BAR_FRAME=1 or a
        # system without such memory: the page-locked host buffer of rounds 3 - 4.
        nbytes = width * height * 4
        self.mem_img = None
        self._bar_frame = False
        if not os.environ.get("ALVA_NO_BAR_FRAME") and hasattr(lib, "alva_system_alloc_frame_buffer"):
            p = _vp()
            if lib.alva_system_alloc_frame_buffer(h, nbytes, C.byref(p)) == 0 and p.value:
                self.mem_img = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(nbytes,)).reshape(height, width, 4)
                self._bar_frame = True
        if self.mem_img is None:
            self._mem_raw = np.empty(nbytes + 4096, np.uint8)
            off = (-self._mem_raw.ctypes.data) % 4096
            self.mem_img = self._mem_raw[off:off + nbytes].reshape(height, width, 4)
        self._registered = self._bar_frame or lib.alva_system_register_frame_buffer(h, self.mem_img.ctypes.data, nbytes) == 0
        self._mem_ptr = self.mem_img.ctypes.data

    @staticmethod
    def Initialize(width: int, height: int, fov: float = 45.0) -> "AlvaAR":  # noqa: N802 (reference name)
        return AlvaAR(width, height, fov)

    def close(self):
        if getattr(self, "h", None):
            lib.alva_system_destroy(self.h)   # releases the frame-buffer registration before mem_img goes away
            self.h = None

    __del__ = close

    def findCameraPose(self, frame_rgba: np.ndarray, timestamp_ms: float | None = None):  # noqa: N802
        """returns (pose[16] or None, status) -- the JS wrapper returns the pose only on status 1.  timestamp_ms = None reads the
        system clock like the reference (system.cpp:114)."""
        self._stage(frame_rgba)
        if timestamp_ms is None:
            status = lib.alva_system_find_camera_pose(self.h, self._mem_ptr, self._pose_ptr)
        else:
            status = lib.alva_system_find_camera_pose_ts(self.h, self._mem_ptr, timestamp_ms, self._pose_ptr)
        if status < 0:
            raise AlvaError(lib.alva_system_last_error().decode())
        return (self._pose.copy() if status == 1 else None), status

    def _stage(self, frame_rgba) -> np.ndarray:
        """memImg.write(frame.data) (src/system.js:175): the frame goes into the wrapper's own registered buffer -- unless the caller
        already wrote it there (passes self.mem_img itself)."""
        if frame_rgba is self.mem_img:
            return self.mem_img
        np.copyto(self.mem_img, np.asarray(frame_rgba, np.uint8).reshape(self.mem_img.shape))
        return self.mem_img

    def find_camera_pose_device(self, d_rgba_ptr: int, timestamp_ms: float, next_d_rgba_ptr: int | None = None):
        """frame already in device memory (torch tensor .data_ptr()); returns the status, the pose is in self._pose.
        next_d_rgba_ptr: the frame the NEXT call will pass (alva_system_hint_next_frame_device: its pyramid is built ahead)"""
        if next_d_rgba_ptr:
            lib.alva_system_hint_next_frame_device(self.h, next_d_rgba_ptr)
        status = self._fcp_device(self.h, d_rgba_ptr, timestamp_ms, self._pose_ptr)
        if status < 0:
            raise AlvaError(lib.alva_system_last_error().decode())
        return status

    def findCameraPoseWithIMU(self, frame_rgba, orientation_wxyz, motion=(), timestamp_ms: float | None = None):  # noqa: N802
        frame = self._stage(frame_rgba)
        imu = np.zeros(256, np.float64)
        imu[:4] = orientation_wxyz
        imu[4] = len(motion)
        for k, smp in enumerate(motion):
            imu[5 + 7 * k:12 + 7 * k] = smp
        if timestamp_ms is None:
            status = lib.alva_system_find_camera_pose_with_imu(self.h, frame.ctypes.data, imu.ctypes.data, self._pose.ctypes.data)
        else:
            status = lib.alva_system_find_camera_pose_with_imu_ts(self.h, frame.ctypes.data, imu.ctypes.data, float(timestamp_ms), self._pose.ctypes.data)
        return self._pose.copy() if status == 1 else None

    def findPlane(self, num_iterations: int = 250):  # noqa: N802
        out = np.zeros(16, np.float32)
        return out if lib.alva_system_find_plane(self.h, out.ctypes.data, num_iterations) == 1 else None

    def hitTest(self, uv, radius_px: float = 40.0, num_iterations: int = 64):  # noqa: N802
        """alva_system_hit_test: taps uv [n,2] in raw image pixels -> (poses [n,16] float32, info [n,8] int32); info[:,0] is the code
        (0 found, 1 too few points under the tap, 2 no hypothesis, 3 too few inliers, 4 grazing / behind, 5 not tracking) and a pose
        row is meaningful only where it is 0"""
        taps = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
        n = taps.shape[0]
        poses, info = np.zeros((max(n, 1), 16), np.float32), np.zeros((max(n, 1), 8), np.int32)
        rc = lib.alva_system_hit_test(self.h, n, taps.ctypes.data, float(radius_px), int(num_iterations), poses.ctypes.data, info.ctypes.data)
        if rc < 0:
            raise AlvaError(lib.alva_system_last_error().decode())
        return poses[:n], info[:n]

    def depthImage(self, step: int = 4, num_hyp: int = 64, patch_radius: int = 2, min_texture: int = 4, min_conf: int = 96,  # noqa: N802
                   debug: bool = False):
        """alva_system_depth: the current frame's depth from motion on the grid (width // step) x (height // step) -> (depth [gh,gw]
        float32: camera-space z in map units, 0 where there is none; conf [gh,gw] uint8; code [gh,gw] uint8: 0 a depth, 1 border, 2 no
        texture, 3 not seen by the reference frame, 4 low confidence, 5 outside the swept range, 6 not tracking, 7 no reference frame
        yet; info = dict(counts of the codes 0..5, gw, gh, status: 0 answered, 6 or 7 for the whole image)).  Needs AlvaAR(...,
        depth=True).  debug: info also holds what the sweep was handed (cur, ref [h,w] uint8, T_rc [12], rho (min, max)) when it ran."""
        step = int(step)
        w, h = self.intrinsics["width"], self.intrinsics["height"]
        gw, gh = (w // step, h // step) if 1 <= step <= 16 else (1, 1)
        n = max(gw * gh, 1)
        depth, conf, code, info = np.zeros(n, np.float32), np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(8, np.int32)
        args = (self.h, step, int(num_hyp), int(patch_radius), int(min_texture), int(min_conf), depth.ctypes.data, conf.ctypes.data,
                code.ctypes.data, n, info.ctypes.data)
        if debug:
            images, T, rho = np.zeros((2, h, w), np.uint8), np.zeros(12), np.zeros(2)
            rc = lib.alva_system_debug_depth(*args, images.ctypes.data, T.ctypes.data, rho.ctypes.data)
        else:
            rc = lib.alva_system_depth(*args)
        if rc < 0:
            raise AlvaError(lib.alva_system_last_error().decode())
        status = 0 if info[:6].sum() else int(code[0])
        out = dict(counts=info[:6].copy(), gw=int(info[6]), gh=int(info[7]), status=status)
        if debug and status == 0:
            out.update(cur=images[0], ref=images[1], T_rc=T, rho=(float(rho[0]), float(rho[1])))
        return depth.reshape(gh, gw), conf.reshape(gh, gw), code.reshape(gh, gw), out

    def depthDense(self, step: int = 4, num_hyp: int = 64, patch_radius: int = 2, min_texture: int = 4, min_conf: int = 96,  # noqa: N802
                   max_level: int = 5, debug: bool = False):
        """alva_system_depth_dense: the depth image fused over the session's frames and completed, on the grid (width // step) x (height
        // step) -> (depth [gh,gw] float32: camera-space z in map units, 0 where there is none; weight [gh,gw] uint8: the fused state's
        weight, 0 for a filled or empty cell; src [gh,gw] uint8: how the cell was fused, 0..5; level [gh,gw] uint8: 0 a fused value, 1 ..
        max_level a filled one whose nearest evidence is about 2^level cells away, 255 none; info = dict(fuse = counts of src 0..5,
        filled, empty, gw, gh, status: 0 answered, 6 not tracking, 7 no reference frame, swept = the sweep's count of code 0, warped)).
        Needs AlvaAR(..., depth=True).  debug: info also holds what the two stages were handed (rho_before, w_before, rho_after, raw =
        (depth, conf, code), gray [h,w], poses [2,7], T_cp [12], rho_ref, ran = -1 nothing / 0 fill only / 1 fuse / 2 warp and fuse,
        did_sweep)."""
        step = int(step)
        w, h = self.intrinsics["width"], self.intrinsics["height"]
        gw, gh = (w // step, h // step) if 1 <= step <= 16 else (1, 1)
        n = max(gw * gh, 1)
        depth, weight, src, level = np.zeros(n, np.float32), np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        info = np.zeros(16, np.int32)
        args = (self.h, step, int(num_hyp), int(patch_radius), int(min_texture), int(min_conf), int(max_level), depth.ctypes.data,
                weight.ctypes.data, src.ctypes.data, level.ctypes.data, n, info.ctypes.data)
        if debug:
            rb, wb, ra = np.zeros(n, np.float32), np.zeros(n, np.uint8), np.zeros(n, np.float32)
            rd, rc_, rk = np.zeros(n, np.float32), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
            gray, poses, T, rho_ref, flags = np.zeros((h, w), np.uint8), np.zeros((2, 7)), np.zeros(12), np.zeros(1), np.zeros(4, np.int32)
            rc = lib.alva_system_debug_depth_dense(*args, *(a.ctypes.data for a in (rb, wb, ra, rd, rc_, rk, gray, poses, T, rho_ref, flags)))
        else:
            rc = lib.alva_system_depth_dense(*args)
        if rc < 0:
            raise AlvaError(lib.alva_system_last_error().decode())
        out = dict(fuse=info[:6].copy(), filled=int(info[6]), empty=int(info[7]), gw=int(info[8]), gh=int(info[9]), status=int(info[10]),
                   swept=int(info[11]), warped=int(info[12]), count=int(rc))
        shape = (gh, gw)
        if debug:
            out.update(rho_before=rb.reshape(shape), w_before=wb.reshape(shape), rho_after=ra.reshape(shape),
                       raw=(rd.reshape(shape), rc_.reshape(shape), rk.reshape(shape)), gray=gray, poses=poses, T_cp=T, rho_ref=float(rho_ref[0]),
                       ran=int(flags[0]), did_sweep=int(flags[1]))
        return depth.reshape(shape), weight.reshape(shape), src.reshape(shape), level.reshape(shape), out

    def resetDepthDense(self):  # noqa: N802
        if lib.alva_system_reset_depth_dense(self.h):
            raise AlvaError(lib.alva_system_last_error().decode())

    def meshUpdate(self, resolution: int = 64, rel_extent: float = 4.0, step: int = 4, num_hyp: int = 64, patch_radius: int = 2,  # noqa: N802
                   min_texture: int = 4, min_conf: int = 96, debug: bool = False):
        """alva_system_mesh_update: the current frame's depth from motion integrated into the session's signed distance volume
        (resolution^3 voxels on the device, in world coordinates; placed by the first call from the frame's median depth x rel_extent and
        then fixed) -> dict(status: 0 integrated, 6 not tracking, 7 no reference frame yet, 8 this frame is integrated already; updated,
        hidden, free, outside, no_depth: the voxels' counts; resolution, swept = the sweep's count of code 0, frames integrated so far,
        placed: by this call; colored = voxels whose colour was updated, color_fused: 1 when this call fused colour (mesh_color on and
        the frame's thumbnail kept); origin [3], voxel, trunc: where the volume lies; count = voxels updated; shifted: 1 when this call
        moved the volume before it integrated (mesh_follow on), shift [3] int32: by how many voxels).  Needs AlvaAR(..., depth=True).
        debug: also what the call saw, when it integrated: raw = (depth, conf, code) [gh,gw], T_cw [12], and the volume after, q
        [N,N,N] int16 and w [N,N,N] uint8."""
        step, n_res = int(step), int(resolution)
        info, geo = np.zeros(16, np.int32), np.zeros(5)
        args = (self.h, n_res, float(rel_extent), step, int(num_hyp), int(patch_radius), int(min_texture), int(min_conf), info.ctypes.data,
                geo.ctypes.data)
        if debug:
            w, h = self.intrinsics["width"], self.intrinsics["height"]
            gw, gh = (w // step, h // step) if 1 <= step <= 16 else (1, 1)
            n, vol = max(gw * gh, 1), n_res ** 3 if n_res in (32, 64, 128, 256) else 1
            rd, rc_, rk, T = np.zeros(n, np.float32), np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(12)
            q, wt = np.zeros(vol, np.int16), np.zeros(vol, np.uint8)
            rc = lib.alva_system_debug_mesh_update(*args, *(a.ctypes.data for a in (rd, rc_, rk, T, q, wt)))
        else:
            rc = lib.alva_system_mesh_update(*args)
        if rc < 0:
            raise AlvaError(lib.alva_system_last_error().decode())
        out = dict(status=int(info[0]), updated=int(info[1]), hidden=int(info[2]), free=int(info[3]), outside=int(info[4]), no_depth=int(info[5]),
                   resolution=int(info[6]), swept=int(info[7]), frames=int(info[8]), placed=int(info[9]), colored=int(info[10]),
                   color_fused=int(info[11]), origin=geo[:3].copy(), voxel=float(geo[3]), trunc=float(geo[4]), count=int(rc),
                   shifted=int(info[12]), shift=info[13:16].copy())
        if debug and out["status"] == 0:
            out.update(raw=(rd.reshape(gh, gw), rc_.reshape(gh, gw), rk.reshape(gh, gw)), T_cw=T, q=q.reshape(n_res, n_res, n_res),
                       w=wt.reshape(n_res, n_res, n_res))
        return out

    def mesh(self, min_weight: int = 2, max_vertices: int = 1 << 18, max_triangles: int = 1 << 19, colors: bool = False):
        """alva_system_mesh: the surface of the session's volume -> (vertices [nv,3] float32 in world coordinates, normals [nv,3] float32
        pointing to the free side, triangles [nt,3] int32, info = dict(status: 0 a mesh, 1 no surface yet, 3 over max_vertices or
        max_triangles (the counts are the true ones), 5 no volume yet; vertices, triangles, valid, inside: counts; resolution; origin
        [3], voxel, trunc)).  The whole volume is extracted at every call, whether or not the tracker tracks right now.
        colors=True: alva_system_mesh_colored -> (vertices, normals, colors [nv,4] uint8, triangles, info): r, g, b of every vertex from
        the colour volume, alpha 255 where it has a colour and four zeros where it has none; info["colored"] counts the former.  Needs
        AlvaAR(..., mesh_color=True)."""
        mv, mt = max(int(max_vertices), 1), max(int(max_triangles), 1)
        v, nrm, t = np.zeros((mv, 3), np.float32), np.zeros((mv, 3), np.float32), np.zeros((mt, 3), np.int32)
        info, geo = np.zeros(8, np.int32), np.zeros(5)
        if colors:
            if not hasattr(lib, "alva_system_mesh_colored"):
                raise AlvaError("alva_system_mesh_colored is not in the loaded library")
            col = np.zeros((mv, 4), np.uint8)
            rc = lib.alva_system_mesh_colored(self.h, int(min_weight), int(max_vertices), int(max_triangles), v.ctypes.data, nrm.ctypes.data,
                                              col.ctypes.data, t.ctypes.data, info.ctypes.data, geo.ctypes.data)
        else:
            rc = lib.alva_system_mesh(self.h, int(min_weight), int(max_vertices), int(max_triangles), v.ctypes.data, nrm.ctypes.data, t.ctypes.data,
                                      info.ctypes.data, geo.ctypes.data)
        if rc < 0:
            raise AlvaError(lib.alva_system_last_error().decode())
        nv, nt = (int(info[1]), int(info[2])) if info[0] == 0 else (0, 0)
        out = dict(status=int(info[0]), vertices=int(info[1]), triangles=int(info[2]), valid=int(info[3]), inside=int(info[4]),
                   resolution=int(info[5]), origin=geo[:3].copy(), voxel=float(geo[3]), trunc=float(geo[4]))
        if colors:
            out["colored"] = int(info[6])
            return v[:nv].copy(), nrm[:nv].copy(), col[:nv].copy(), t[:nt].copy(), out
        return v[:nv].copy(), nrm[:nv].copy(), t[:nt].copy(), out

    def meshColorAt(self, points):  # noqa: N802
        """alva_system_mesh_color_at: the colour volume at world points [n,3] (for example meshRaycast's points) -> (rgba [n,4] uint8: alpha
        255 with a colour, else four zeros; codes [n] uint8: 0 a colour, 1 outside the volume, 2 no colour was fused there, 4 not finite, 5
        no volume or no colour volume yet; info [8] int32 = (n, the counts of the codes 0, 1, 2, 4, 0, 0, resolution)).  It answers whether
        or not the tracker tracks right now.  Needs AlvaAR(..., mesh_color=True)."""
        if not hasattr(lib, "alva_system_mesh_color_at"):
            raise AlvaError("alva_system_mesh_color_at is not in the loaded library")
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        n = pts.shape[0]
        m = max(n, 1)
        rgba, codes, info = np.zeros((m, 4), np.uint8), np.zeros(m, np.uint8), np.zeros(8, np.int32)
        rc = lib.alva_system_mesh_color_at(self.h, n, pts.ctypes.data, rgba.ctypes.data, codes.ctypes.data, info.ctypes.data)
        if rc < 0:
            raise AlvaError(lib.alva_system_last_error().decode())
        return rgba[:n], codes[:n], info

    def setMeshColor(self, enabled: bool):  # noqa: N802
        """alva_system_set_mesh_color; a change empties the colours"""
        if not hasattr(lib, "alva_system_set_mesh_color"):
            raise AlvaError("alva_system_set_mesh_color is not in the loaded library")
        if lib.alva_system_set_mesh_color(self.h, int(bool(enabled))):
            raise AlvaError(lib.alva_system_last_error().decode())

    def mesh_color_state(self, resolution: int):
        """alva_system_debug_mesh_color (for the replay tests): (thumb [h // 4, w // 4, 4] uint8 -- the kept thumbnail --, c [N,N,N,4]
        uint8 -- the colour volume, N = resolution --, flags: bit 0 the thumbnail is the current frame's, bit 1 there is a colour volume)"""
        w, h, n = self.intrinsics["width"], self.intrinsics["height"], int(resolution)
        thumb, c = np.zeros((h // 4, w // 4, 4), np.uint8), np.zeros((n, n, n, 4), np.uint8)
        rc = lib.alva_system_debug_mesh_color(self.h, thumb.ctypes.data, c.ctypes.data)
        if rc < 0:
            raise AlvaError(lib.alva_system_last_error().decode())
        return thumb, c, int(rc)

    def resetMesh(self):  # noqa: N802
        if lib.alva_system_reset_mesh(self.h):
            raise AlvaError(lib.alva_system_last_error().decode())

    def meshBlocks(self, min_weight: int = 2, block: int = 16, all: bool = False, colors: bool = False, max_blocks: int = 1 << 12,  # noqa: N802, A002
                   max_vertices: int = 1 << 18, max_triangles: int = 1 << 19):
        """alva_system_mesh_blocks: the mesh in blocks of `block` (8, 16 or 32) voxels of a world-fixed lattice, and of those only the
        ones that changed since the last successful call (all=True: every present block) -> a dict: keys [n,3] int32 = (b_x, b_y, b_z),
        state [n] int32 (0 unchanged -- only with all --, 1 new, 2 changed, 3 no surface any more, 4 left the cube: keep your copy if
        you like), ranges [n,4] int32 = (v0, nv, t0, nt) into vertices / normals [nv,3] float32, colors [nv,4] uint8 (None unless
        colors=True, which needs AlvaAR(..., mesh_color=True)) and triangles [nt,3] int32, whose indices are LOCAL to their block (0 ..
        nv - 1), digest [n] uint64, lattice [3] int32 (the volume's offset in voxels), info = dict(status: 0, 3 over max_blocks /
        max_vertices / max_triangles (the counts are the true ones, nothing is handed out and the list is untouched: call again with
        room), 5 no volume yet; blocks, vertices, triangles, gone, epoch -- drop every chunk when it changes --, present, block), geometry
        = dict(origin [3], voxel, trunc).  Change detection is on geometry alone: for refreshed colours ask with all=True."""
        if not hasattr(lib, "alva_system_mesh_blocks"):
            raise AlvaError("alva_system_mesh_blocks is not in the loaded library")
        mb, mv, mt = max(int(max_blocks), 1), max(int(max_vertices), 1), max(int(max_triangles), 1)
        keys, binfo = np.zeros((mb, 3), np.int32), np.zeros((mb, 8), np.int32)
        v, nrm, t = np.zeros((mv, 3), np.float32), np.zeros((mv, 3), np.float32), np.zeros((mt, 3), np.int32)
        col = np.zeros((mv, 4), np.uint8) if colors else None
        lattice, info, geo = np.zeros(3, np.int32), np.zeros(8, np.int32), np.zeros(5)
        rc = lib.alva_system_mesh_blocks(self.h, int(min_weight), int(block), 1 if all else 0, int(max_blocks), int(max_vertices), int(max_triangles),
                                         keys.ctypes.data, binfo.ctypes.data, v.ctypes.data, nrm.ctypes.data, col.ctypes.data if colors else 0,
                                         t.ctypes.data, lattice.ctypes.data, info.ctypes.data, geo.ctypes.data)
        if rc < 0:
            raise AlvaError(lib.alva_system_last_error().decode())
        n, nv, nt = (int(info[1]), int(info[2]), int(info[3])) if info[0] == 0 else (0, 0, 0)
        digest = (binfo[:n, 5].astype(np.uint32).astype(np.uint64) | (binfo[:n, 6].astype(np.uint32).astype(np.uint64) << np.uint64(32)))
        return dict(keys=keys[:n].copy(), state=binfo[:n, 0].copy(), ranges=binfo[:n, 1:5].copy(), digest=digest, vertices=v[:nv].copy(),
                    normals=nrm[:nv].copy(), colors=col[:nv].copy() if colors else None, triangles=t[:nt].copy(), lattice=lattice,
                    info=dict(status=int(info[0]), blocks=int(info[1]), vertices=int(info[2]), triangles=int(info[3]), gone=int(info[4]),
                              epoch=int(info[5]), present=int(info[6]), block=int(info[7])),
                    geometry=dict(origin=geo[:3].copy(), voxel=float(geo[3]), trunc=float(geo[4])))

    def resetMeshBlocks(self):  # noqa: N802
        """alva_system_reset_mesh_blocks: forget the list -- epoch + 1, the next call reports every present block as new"""
        if not hasattr(lib, "alva_system_reset_mesh_blocks"):
            raise AlvaError("alva_system_reset_mesh_blocks is not in the loaded library")
        if lib.alva_system_reset_mesh_blocks(self.h):
            raise AlvaError(lib.alva_system_last_error().decode())

    def setMeshFollow(self, block: int):  # noqa: N802
        """alva_system_set_mesh_follow: block 0 (off), 1, 2, 4, 8, 16 or 32 voxels; the switch itself does not touch the volume"""
        if not hasattr(lib, "alva_system_set_mesh_follow"):
            raise AlvaError("alva_system_set_mesh_follow is not in the loaded library")
        if lib.alva_system_set_mesh_follow(self.h, int(block)):
            raise AlvaError(lib.alva_system_last_error().decode())

    def meshFollowStats(self):  # noqa: N802
        """alva_system_mesh_follow_stats -> dict(block, shifts: of this volume so far, offset [3] int64: its offset in voxels since it
        was placed, lost: weighted voxels that left the cube so far)"""
        if not hasattr(lib, "alva_system_mesh_follow_stats"):
            raise AlvaError("alva_system_mesh_follow_stats is not in the loaded library")
        st = (C.c_long * 8)()
        if lib.alva_system_mesh_follow_stats(self.h, st):
            raise AlvaError(lib.alva_system_last_error().decode())
        return dict(block=int(st[0]), shifts=int(st[1]), offset=np.array([st[2], st[3], st[4]], np.int64), lost=int(st[5]))

    def meshMove(self, center, block: int = 8):  # noqa: N802
        """alva_system_mesh_move: the volume shifted, in whole blocks of `block` voxels, so that its centre lies within a block of the
        world point center [3] -> dict(shifted: 1 when it moved, status: 0 or 5 no volume yet, shift [3] int64 in voxels, copied, kept,
        lost, colored: alva_mesh_shift's counts (voxels copied, copied with a weight, weighted voxels lost, copied with a colour),
        resolution, origin [3], voxel, trunc: where the volume lies now).  What leaves the cube is gone.  It answers whether or not the
        tracker tracks right now."""
        if not hasattr(lib, "alva_system_mesh_move"):
            raise AlvaError("alva_system_mesh_move is not in the loaded library")
        c = np.ascontiguousarray(center, np.float64).reshape(-1)
        assert c.size == 3
        info, geo = np.zeros(8, np.int32), np.zeros(5)
        before = self.meshFollowStats()["offset"]
        rc = lib.alva_system_mesh_move(self.h, c.ctypes.data, int(block), info.ctypes.data, geo.ctypes.data)
        if rc < 0:
            raise AlvaError(lib.alva_system_last_error().decode())
        return dict(shifted=int(rc), status=int(info[4]), shift=self.meshFollowStats()["offset"] - before, copied=int(info[0]), kept=int(info[1]),
                    lost=int(info[2]), colored=int(info[3]), resolution=int(info[7]), origin=geo[:3].copy(), voxel=float(geo[3]),
                    trunc=float(geo[4]))

    @staticmethod
    def _ray_info(info, codes):
        """h_info8 of the raycast calls as a dict; status: 0 answered, 5 no volume, 6 not tracking (then every ray's code)"""
        return dict(status=0 if info[1:6].sum() or codes.size == 0 else int(codes.reshape(-1)[0]), rays=int(info[0]), counts=info[1:6].copy(),
                    max_samples=int(info[6]), resolution=int(info[7]))

    def meshRaycast(self, rays6, min_weight: int = 2, t_near: float = 0.0, t_far: float = float("inf")):  # noqa: N802
        """alva_system_mesh_raycast: world rays rays6 [n,6] float64 (origin, then direction of any length; t is in its units) against the
        session's volume -> (t [n] float32, points [n,3] float32, normals [n,3] float32 pointing to the free side, codes [n] uint8: 0 a
        hit, 1 misses the volume, 2 no surface on the ray, 3 the surface from behind, 4 rejected, 5 no volume yet; info = dict(status,
        rays, counts of the codes 0..4, max_samples, resolution)).  It answers whether or not the tracker tracks right now."""
        rays = np.ascontiguousarray(rays6, np.float64).reshape(-1, 6)
        n = rays.shape[0]
        m = max(n, 1)
        t, p, nr, codes, info = np.zeros(m, np.float32), np.zeros((m, 3), np.float32), np.zeros((m, 3), np.float32), np.zeros(m, np.uint8), np.zeros(8, np.int32)
        rc = lib.alva_system_mesh_raycast(self.h, n, rays.ctypes.data, int(min_weight), float(t_near), float(t_far), t.ctypes.data, p.ctypes.data,
                                          nr.ctypes.data, codes.ctypes.data, info.ctypes.data)
        if rc < 0:
            raise AlvaError(lib.alva_system_last_error().decode())
        return t[:n], p[:n], nr[:n], codes[:n], self._ray_info(info, codes[:n])

    def meshDepth(self, T_wc=None, step: int = 4, min_weight: int = 2):  # noqa: N802
        """alva_system_mesh_depth: the depth image of the session's volume on the grid (width // step) x (height // step), from the pose
        T_wc [12] (R_wc row-major, then t_wc; any pose, tracking or not) or, with None, from the current frame's -> (depth [gh,gw] float32:
        camera-space z in map units, 0 where there is none; normals [gh,gw,3] float32 in world coordinates; codes [gh,gw] uint8: 0 a
        depth, 1 misses the volume, 2 no surface on the ray, 3 the surface from behind, 5 no volume yet, 6 not tracking; info as
        meshRaycast's).  It is the volume's depth, not the current frame's: what was never seen is transparent."""
        step = int(step)
        w, h = self.intrinsics["width"], self.intrinsics["height"]
        gw, gh = (w // step, h // step) if 1 <= step <= 16 else (1, 1)
        n = max(gw * gh, 1)
        depth, nr, codes, info = np.zeros(n, np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.uint8), np.zeros(8, np.int32)
        T = None if T_wc is None else np.ascontiguousarray(T_wc, np.float64).reshape(-1)
        assert T is None or T.size == 12
        rc = lib.alva_system_mesh_depth(self.h, None if T is None else T.ctypes.data, step, int(min_weight), depth.ctypes.data, nr.ctypes.data,
                                        codes.ctypes.data, n, info.ctypes.data)
        if rc < 0:
            raise AlvaError(lib.alva_system_last_error().decode())
        return depth.reshape(gh, gw), nr.reshape(gh, gw, 3), codes.reshape(gh, gw), self._ray_info(info, codes)

    def meshHitTest(self, uv, min_weight: int = 2):  # noqa: N802
        """alva_system_mesh_hit_test: taps uv [n,2] in raw image pixels, from the current frame's pose, against the session's volume ->
        (poses [n,16] float32 in hitTest's layout, info [n,8] int32); info[:,0] is the code (0 a hit, 1 misses the volume, 2 no surface on
        the ray, 3 the surface from behind, 4 rejected, 5 no volume yet, 6 not tracking), info[:,1] is 1 where the pose row is
        meaningful (a hit that is not too grazing), info[:,2] the call's largest sample count, info[:,3] the volume's resolution"""
        taps = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
        n = taps.shape[0]
        poses, info = np.zeros((max(n, 1), 16), np.float32), np.zeros((max(n, 1), 8), np.int32)
        rc = lib.alva_system_mesh_hit_test(self.h, n, taps.ctypes.data, int(min_weight), poses.ctypes.data, info.ctypes.data)
        if rc < 0:
            raise AlvaError(lib.alva_system_last_error().decode())
        return poses[:n], info[:n]

    def set_depth(self, enabled: bool):
        if lib.alva_system_set_depth(self.h, int(bool(enabled))):
            raise AlvaError(lib.alva_system_last_error().decode())

    def depth_ring(self):
        """the poses (t, q = x y z w) of the kept reference frames, newest first: [n,7] float64"""
        out = np.zeros((4, 7))
        return out[:lib.alva_system_debug_depth_ring(self.h, out.ctypes.data)].copy()

    def lightEstimate(self, debug: bool = False):  # noqa: N802
        """alva_system_light -> (sh [9,3], primary_dir [3], primary_rgb [3], ambient [4], each float32, info [8] int32): the spherical
        harmonics of the environment in the world frame (rows Y00, y, z, x, xy, yz, Y20, xz, Y22; columns R, G, B), the unit vector
        towards the primary light and its intensity (zeros without one), ambient = (mean luminance of the last frame, colour correction
        r, g, b), info = (code: 0 an estimate / 1 no environment yet / 5 no frame yet, cells with a value, cells the last frame touched,
        its blocks, its saturated pixels, frames fused, primary valid, 0).  Pixel-intensity domain, not photometric.  Needs AlvaAR(...,
        light=True).  debug: a sixth value, dict(acc int64 [LIGHT_ACC_WORDS], R_wc [3,3] or None, fed, frames, state uint8
        [LIGHT_STATE_BYTES]): what the last frame handed to the stages."""
        from .capi import LIGHT_ACC_WORDS, LIGHT_STATE_BYTES
        sh, pd, pc, amb, info = np.zeros(27, np.float32), np.zeros(3, np.float32), np.zeros(3, np.float32), np.zeros(4, np.float32), np.zeros(8, np.int32)
        args = (self.h, *(a.ctypes.data for a in (sh, pd, pc, amb, info)))
        if debug:
            acc, R, flags, state = np.zeros(LIGHT_ACC_WORDS, np.int64), np.zeros(9), np.zeros(4, np.int32), np.zeros(LIGHT_STATE_BYTES, np.uint8)
            rc = lib.alva_system_debug_light(*args, acc.ctypes.data, R.ctypes.data, flags.ctypes.data, state.ctypes.data)
        else:
            rc = lib.alva_system_light(*args)
        if rc < 0:
            raise AlvaError(lib.alva_system_last_error().decode())
        out = (sh.reshape(9, 3), pd, pc, amb, info)
        if debug:
            out += (dict(acc=acc, R_wc=R.reshape(3, 3) if flags[1] else None, fed=bool(flags[0]), frames=int(flags[2]), state=state),)
        return out

    def resetLight(self):  # noqa: N802
        if lib.alva_system_reset_light(self.h):
            raise AlvaError(lib.alva_system_last_error().decode())

    def set_light(self, enabled: bool):
        if lib.alva_system_set_light(self.h, int(bool(enabled))):
            raise AlvaError(lib.alva_system_last_error().decode())

    def addImage(self, gray, width_m: float = 0.0) -> int:  # noqa: N802
        """alva_system_add_image: gray [h, w] uint8 (sides 96 .. 1024), width_m its printed width in metres (0 = unknown) -> its id.
        Described once, here (ORB, 500 features); at most 8 pictures; they outlive configure and reset.  Raises AlvaError with the reason
        when the picture is refused (size, a ninth picture, fewer than 32 keypoints)."""
        g = np.asarray(gray)
        if g.ndim != 2 or g.dtype != np.uint8:
            raise AlvaError("addImage: the picture must be a 2-D uint8 array")
        if g.strides[1] != 1 or g.strides[0] < g.shape[1]:
            g = np.ascontiguousarray(g)
        rc = lib.alva_system_add_image(self.h, g.ctypes.data, g.shape[1], g.shape[0], g.strides[0], float(width_m))
        if rc < 0:
            raise AlvaError(lib.alva_system_last_error().decode())
        self._image_ids = getattr(self, "_image_ids", []) + [rc]   # (the session's pictures, for the row count of detectImages)
        return rc

    def removeImage(self, image_id: int):  # noqa: N802
        if lib.alva_system_remove_image(self.h, int(image_id)):
            raise AlvaError(lib.alva_system_last_error().decode())
        self._image_ids = [i for i in getattr(self, "_image_ids", []) if i != int(image_id)]

    def resetImages(self):  # noqa: N802
        if lib.alva_system_reset_images(self.h):
            raise AlvaError(lib.alva_system_last_error().decode())
        self._image_ids = []

    def detectImages(self, iterations: int = 256, threshold_px: float = 3.0, min_inliers: int = 20, debug: bool = False):  # noqa: N802
        """alva_system_detect_images -> (ids [n] int32, poses [n,16], extents [n,2], scale [n], quads [n,4,2] float32, info [n,8] int32),
        one row per added picture in ascending id, from the current frame.  info[:,0] is the code: 0 found (pose in world coordinates at
        the picture's centre, x right, y the normal towards the viewer, z down the picture; extents in map units; scale = metres per map
        unit or 0), 1 too few pairs, 2 no hypothesis, 3 too few on the best, 4 not a rigid view of a plane, 5 seen but not placed (fewer
        than 8 map points on it), 6 seen, not tracking, 7 no frame yet; quads (undistorted pixels: top-left, top-right, bottom-right,
        bottom-left) are valid for 0, 5, 6.  Nothing is remembered between calls: hand a pose to createAnchors to make it stick.  A
        few-Hz call (several host waits).  debug: a seventh value, what the call saw (alva_image_debug) as a dict."""
        from .capi import IMAGE_MAX as M, IMAGE_QUERY_CAP as Q, IMAGE_TRAIN_CAP as T
        ids, poses, extents, scale = np.zeros(M, np.int32), np.zeros((M, 16), np.float32), np.zeros((M, 2), np.float32), np.zeros(M, np.float32)
        quads, info = np.zeros((M, 4, 2), np.float32), np.zeros((M, 8), np.int32)
        args = (self.h, int(iterations), float(threshold_px), int(min_inliers), M, *(a.ctypes.data for a in (ids, poses, extents, scale, quads, info)))
        if debug:
            d = dict(n_frame=np.zeros(1, np.int32), kp=np.zeros((T, 2), np.float32), unpx=np.zeros((T, 2), np.float32), desc=np.zeros((T, 32), np.uint8),
                     nq=np.zeros(M, np.int32), wh=np.zeros((M, 2), np.int32), qxy=np.zeros((M, Q, 2), np.float32), qdesc=np.zeros((M, Q, 32), np.uint8),
                     match=np.zeros((M, Q, 3), np.int32), xy=np.zeros((M, Q, 4)), count=np.zeros(M, np.int32), H=np.zeros((M, 9)),
                     mask=np.zeros((M, Q), np.uint8), stage_info=np.zeros((M, 8), np.int32), stage_R=np.zeros((M, 9)), stage_t=np.zeros((M, 3)),
                     R=np.zeros((M, 9)), t=np.zeros((M, 3)), pose7=np.zeros(7), tracked=np.zeros(1, np.int32))
            rec = _ImageDebug(**{k: v.ctypes.data for k, v in d.items()})
            rc = lib.alva_system_debug_detect_images(*args, C.addressof(rec))
        else:
            rc = lib.alva_system_detect_images(*args)
        if rc < 0:
            raise AlvaError(lib.alva_system_last_error().decode())
        n = len(getattr(self, "_image_ids", ()))
        out = (ids[:n], poses[:n], extents[:n], scale[:n], quads[:n], info[:n])
        return out + (d,) if debug else out

    def _planes(self, fn, params, max_vertices, tracked):
        """the buffers, the call, the error check and the slicing of detectPlanes, detectPlaneOutlines (max_vertices not None) and
        trackPlanes (tracked) -> (planes, info), (plane_ids, merged_into) or (), (ids, labels), (outlines, outline_info, areas) or ()"""
        cap, mp = 16384, params[2]
        k = max(mp, 1)
        planes, info = np.zeros((k, 24), np.float32), np.zeros((k, 8), np.int32)
        ids, labels = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        args, tracks, out = [planes.ctypes.data, info.ctypes.data, ids.ctypes.data, labels.ctypes.data, cap], (), ()
        if tracked:
            pids, merged = np.full(k, -1, np.int32), np.full(k, -1, np.int32)
            args[2:2], tracks = (pids.ctypes.data, merged.ctypes.data), (pids[:mp], merged[:mp])
        if max_vertices is not None:
            outlines, oinfo, areas = np.zeros((k, max(max_vertices, 1), 2), np.float32), np.zeros((k, 8), np.int32), np.zeros(k, np.float64)
            args += (int(max_vertices), outlines.ctypes.data, oinfo.ctypes.data, areas.ctypes.data)
            out = (outlines[:mp], oinfo[:mp], areas[:mp])
        rc = fn(self.h, float(params[0]), int(params[1]), int(mp), int(params[3]), *args)
        if rc < 0:
            raise AlvaError(lib.alva_system_last_error().decode())
        n = int((ids >= 0).sum())   # the call ends the id list with -1s
        return (planes[:mp], info[:mp]), tracks, (ids[:n], labels[:n]), out

    def detectPlanes(self, rel_thickness: float, min_inliers: int = 48, max_planes: int = 4, num_iterations: int = 128):  # noqa: N802
        """alva_system_detect_planes: the planes of the map -> (planes [max_planes,24] float32, info [max_planes,8] int32, ids [n] int32,
        labels [n] int32).  planes[k] = pose16 (columns long axis, normal, short axis; translation = the rectangle's centre), extent
        along the long and the short axis, the plane's offset normal . centre, five zeros -- meaningful only where info[k,0] is 0
        (1 too few live points, 2 no hypothesis, 3 / 4 too few inliers, 5 not run, 6 not tracking).  ids are the map points the call
        looked at (ascending, at most 16384) and labels[i] the plane of point ids[i], or -1.  rel_thickness is the slab's half
        thickness as a fraction of the current frame's median point depth"""
        base, _, pts, _ = self._planes(lib.alva_system_detect_planes, (rel_thickness, min_inliers, max_planes, num_iterations), None, False)
        return base + pts

    def detectPlaneOutlines(self, rel_thickness: float, min_inliers: int = 48, max_planes: int = 4, num_iterations: int = 128,  # noqa: N802
                            max_vertices: int = 64):
        """alva_system_detect_plane_outlines: detectPlanes' four results (the same bytes), then outlines [max_planes,max_vertices,2]
        float32 -- each plane's convex boundary polygon in the plane's own frame (u along the long axis, v along the short one, from the
        rectangle's centre; world point = centre + u * long axis + v * short axis), counter-clockwise, zero past the last vertex --,
        outline_info [max_planes,8] int32 = code (0 an outline, 1 fewer than 3 points, 2 no area, 3 more than max_vertices vertices,
        4 unusable record, 5 no such plane, 6 not tracking), vertices, points; areas [max_planes] float64"""
        base, _, pts, out = self._planes(lib.alva_system_detect_plane_outlines, (rel_thickness, min_inliers, max_planes, num_iterations),
                                         max_vertices, False)
        return base + pts + out

    def trackPlanes(self, rel_thickness: float, min_inliers: int = 48, max_planes: int = 4, num_iterations: int = 128,  # noqa: N802
                    max_vertices: int = 0):
        """alva_system_track_planes: detectPlanes' planes, kept between calls -> (planes [max_planes,24] float32, info [max_planes,8]
        int32, plane_ids [max_planes] int32, merged_into [max_planes] int32, ids [n] int32, labels [n] int32) and, with max_vertices > 0,
        detectPlaneOutlines' (outlines, outline_info, areas).  A plane returned by an earlier call comes first, in its id's order, refitted
        to the map as it is now; info[k] = code, points or live points, -1 or winning iteration, claimed or best count, inliers, origin
        (1 tracked, 0 new); codes 0 a plane, 1 .. 5 detectPlanes', 6 not tracking (the planes are kept), 7 / 8 a tracked plane lost
        before / after its refit, 9 its record unusable.  plane_ids[k] is the plane's id (never reused) or -1, merged_into[k] the id of the
        plane that plane k turned out to be part of (it is returned once more, then gone) or -1"""
        base, tracks, pts, out = self._planes(lib.alva_system_track_planes, (rel_thickness, min_inliers, max_planes, num_iterations),
                                              max_vertices, True)
        return base + tracks + pts + (out if max_vertices > 0 else ())

    def resetPlanes(self):  # noqa: N802
        """alva_system_reset_planes: forget the tracked planes; the next trackPlanes finds them anew, under fresh ids"""
        lib.alva_system_reset_planes(self.h)

    def createAnchors(self, poses16, max_support: int = 32):  # noqa: N802
        """alva_system_create_anchors: poses16 [n,16] float32 (1..16 poses as hitTest, findPlane and detectPlanes return them) ->
        (ids [n] int32 -- -1 where none was created --, info [n,8] int32 = code, supports, points looked at).  Codes: 0 created, 1 fewer
        than four 3-D points in the map, 3 the list of 64 is full, 4 a non-finite pose, 6 not tracking.  An anchor is tied to the
        max_support map points nearest to it; updateAnchors moves its pose with them"""
        poses = np.ascontiguousarray(poses16, np.float32).reshape(-1, 16)
        n = len(poses)
        ids, info = np.full(max(n, 1), -1, np.int32), np.zeros((max(n, 1), 8), np.int32)
        rc = lib.alva_system_create_anchors(self.h, n, poses.ctypes.data, int(max_support), ids.ctypes.data, info.ctypes.data)
        if rc < 0:
            raise AlvaError(lib.alva_system_last_error().decode())
        return ids[:n], info[:n]

    def updateAnchors(self):  # noqa: N802
        """alva_system_update_anchors: every anchor's pose on the map as it is now -> (ids [n] int32 ascending, poses [n,16] float32, info
        [n,8] int32 = code, supports alive, kept by the trim, re-attached, age, supports at attach).  Codes: 0 a rigid update, 1
        translation only, 2 no support alive, 6 not tracking (the pose delivered last; the anchors are kept)"""
        cap = 64
        ids, poses, info = np.full(cap, -1, np.int32), np.zeros((cap, 16), np.float32), np.zeros((cap, 8), np.int32)
        n = lib.alva_system_update_anchors(self.h, cap, ids.ctypes.data, poses.ctypes.data, info.ctypes.data)
        if n < 0:
            raise AlvaError(lib.alva_system_last_error().decode())
        return ids[:n], poses[:n], info[:n]

    def removeAnchor(self, anchor_id: int) -> bool:  # noqa: N802
        """alva_system_remove_anchor: True when the anchor existed"""
        return lib.alva_system_remove_anchor(self.h, int(anchor_id)) == 1

    def resetAnchors(self):  # noqa: N802
        """alva_system_reset_anchors: forget every anchor; ids go on from where they were"""
        lib.alva_system_reset_anchors(self.h)

    def getFramePoints(self):  # noqa: N802
        buf = np.zeros(4096, np.int32)
        n = lib.alva_system_get_frame_points(self.h, buf.ctypes.data)
        m = min(n, 2048)
        return [dict(x=int(buf[2 * i]), y=int(buf[2 * i + 1])) for i in range(m)]

    def reset(self):
        lib.alva_system_reset(self.h)

    def set_relocalization(self, enabled: bool, max_lost_frames: int = 0):
        if lib.alva_system_set_relocalization(self.h, int(bool(enabled)), int(max_lost_frames)):
            raise AlvaError(lib.alva_system_last_error().decode())

    def relocalization_stats(self):
        """alva_system_relocalization_stats: dict(lost_frames=frames in the current LOST episode, attempts, successes,
        last_inliers=inliers of the last attempt)"""
        out = np.zeros(4, np.int64)
        lib.alva_system_relocalization_stats(self.h, out.ctypes.data)
        return dict(zip(("lost_frames", "attempts", "successes", "last_inliers"), (int(v) for v in out)))

    def keypoints(self, cap: int = 16384):
        ids = np.zeros(cap, np.int32)
        px = np.zeros((cap, 2), np.float32)
        is3d = np.zeros(cap, np.uint8)
        n = min(lib.alva_system_get_keypoints(self.h, ids.ctypes.data, px.ctypes.data, is3d.ctypes.data, cap), cap)
        return ids[:n], px[:n], is3d[:n].astype(bool)

    # ---- inspection (alva_system_debug_*), same layouts as the reference-side shim of the tests
    def pose7(self):
        p, q = np.zeros(7), np.zeros(7)
        lib.alva_system_debug_pose7(self.h, p.ctypes.data, q.ctypes.data)
        return p, q

    def state(self):
        out = np.zeros(16, np.int32)
        lib.alva_system_debug_state(self.h, out.ctypes.data)
        return out

    def frame_keypoints(self, cap: int = 16384):
        ids, px, un = np.zeros(cap, np.int32), np.zeros((cap, 2), np.float32), np.zeros((cap, 2), np.float32)
        i3, hd = np.zeros(cap, np.uint8), np.zeros(cap, np.uint8)
        n = lib.alva_system_debug_frame_keypoints(self.h, cap, ids.ctypes.data, px.ctypes.data, un.ctypes.data, i3.ctypes.data, hd.ctypes.data)
        return ids[:n], px[:n], un[:n], i3[:n], hd[:n]

    def keyframe_ids(self, cap: int = 256):
        ids = np.zeros(cap, np.int32)
        n = lib.alva_system_debug_keyframe_ids(self.h, cap, ids.ctypes.data)
        return ids[:n]

    def keyframe(self, kfid: int, cap: int = 16384):
        pose, info = np.zeros(7), np.zeros(6, np.int32)
        ids, px, i3 = np.zeros(cap, np.int32), np.zeros((cap, 2), np.float32), np.zeros(cap, np.uint8)
        n = lib.alva_system_debug_keyframe(self.h, kfid, pose.ctypes.data, info.ctypes.data, cap, ids.ctypes.data, px.ctypes.data, i3.ctypes.data)
        return pose, info, ids[:n], px[:n], i3[:n]

    def covisibility(self, kfid: int = -1, cap: int = 256):
        pairs = np.zeros((cap, 2), np.int32)
        n = lib.alva_system_debug_covisibility(self.h, kfid, cap, pairs.ctypes.data)
        return pairs[:max(n, 0)]

    def map_points(self, cap: int = 65536):
        ids, xyz, fl = np.zeros(cap, np.int32), np.zeros((cap, 3)), np.zeros((cap, 5), np.int32)
        inv, desc = np.zeros(cap), np.zeros((cap, 32), np.uint8)
        n = lib.alva_system_debug_map_points(self.h, cap, ids.ctypes.data, xyz.ctypes.data, fl.ctypes.data, inv.ctypes.data, desc.ctypes.data)
        return ids[:n], xyz[:n], fl[:n], inv[:n], desc[:n]

    def frame_map_point_ids(self, cap: int = 65536):
        """ids of the current frame's observed 3-D map points in the order findPlane / hitTest hand them to their kernels"""
        ids = np.zeros(cap, np.int32)
        n = lib.alva_system_debug_frame_map_point_ids(self.h, cap, ids.ctypes.data)
        return ids[:min(max(n, 0), cap)]

    def pack_map_records(self, stream_id: int, capacity: int, out):
        """alva_system_pack_map_records: this session's 3-D map points as 64-byte exchange records written on the device into `out`
        (cuda uint8 tensor [capacity, 64]); returns the number of points found (may exceed capacity: then `out` holds a subset)"""
        n = C.c_int(0)
        lib.alva_system_pack_map_records.argtypes = [_vp, C.c_int, C.c_int, _vp, C.POINTER(C.c_int)]
        rc = lib.alva_system_pack_map_records(self.h, int(stream_id), int(capacity), out.data_ptr(), C.byref(n))
        if rc < 0:
            raise AlvaError(lib.alva_system_last_error().decode())
        return n.value

    def merge_map_points(self, prev_id: int, new_id: int) -> bool:
        """MapManager::mergeMapPoints(prev_id, new_id) on this session's map (include/alvaar_system.h); False = the reference's early return"""
        rc = lib.alva_system_merge_map_points(self.h, int(prev_id), int(new_id))
        if rc < 0:
            raise AlvaError(lib.alva_system_last_error().decode())
        return rc == 1

    def set_shared_ids(self, local_ids, shared_stream, shared_id) -> int:
        a, b, c = (np.ascontiguousarray(v, np.int32) for v in (local_ids, shared_stream, shared_id))
        rc = lib.alva_system_set_shared_ids(self.h, len(a), a.ctypes.data, b.ctypes.data, c.ctypes.data)
        if rc < 0:
            raise AlvaError(lib.alva_system_last_error().decode())
        return rc

    def shared_ids(self, cap: int = 65536):
        a, b, c = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        n = lib.alva_system_get_shared_ids(self.h, cap, a.ctypes.data, b.ctypes.data, c.ctypes.data)
        if n < 0:
            raise AlvaError(lib.alva_system_last_error().decode())
        n = min(n, cap)
        return a[:n], b[:n], c[:n]

    def counters(self):
        out = (C.c_long * 3)()
        lib.alva_system_debug_counters(self.h, out)
        return dict(ba_solves=out[0], merges=out[1], culled_keyframes=out[2])

    def klt_work(self, reset: bool = True):
        """(keypoint-levels, slots) of the tracking steps since the last reset"""
        out = (C.c_long * 2)()
        lib.alva_system_debug_klt_work(self.h, out, int(reset))
        return int(out[0]), int(out[1])

    def timing(self, reset: bool = True):
        """seconds per section of the frame loop since the last reset (see alva_system_debug_timing)"""
        out = np.zeros(8)
        lib.alva_system_debug_timing(self.h, out.ctypes.data, int(reset))
        names = ("upload+pyramid", "gather", "track_step", "track_apply", "pose_wait", "pose_apply+kf_check", "keyframe_create", "mapping")
        return dict(zip(names, out))

    def timing_keyframe(self, reset: bool = True):
        out = np.zeros(16)
        lib.alva_system_debug_timing_keyframe(self.h, out.ctypes.data, int(reset))
        names = ("prepare", "describe_tracked", "detect", "describe_new", "insert+copy", "triangulate", "covisibility", "local_map_matching",
                 "optimize", "(match stage)", "(BA stage)", "(BA build)", "(BA solves+sweep)", "(BA write-back)", "(BA culling)", "(descriptor medoids)")
        return dict(zip(names, out[:16]))

    FINE_NAMES = ("match: local-map union", "match: flatten+stage", "match: merges", "flatten: kf table + cells", "flatten: local list",
                  "flatten: per map point", "BA build: keyframes + point set", "BA build: observations", "filter: keyframe removals",
                  "window: remove kf-30", "copy: frame", "copy: order mirror", "copy: observation mirror", "new keypoints + map points",
                  "covis: counts", "covis: local ids", "covis: into local map", "parallax pairs (all frames)", "parallax (all frames)", "parallax sort (all frames)",
                  "#flattened map points", "#flattened observations", "#local candidates", "#BA points", "#BA residual blocks", "#BA keyframes",
                  "#new keypoints", "#local ids", "#covisible keyframes", "#frames: slot table carried", "#frames: slot table assembled", "probe 31")   # (31: scratch for measurements)

    def timing_fine(self, reset: bool = True):
        out = np.zeros(32)
        lib.alva_system_debug_timing_fine(self.h, out.ctypes.data, int(reset))
        return {n: v for n, v in zip(self.FINE_NAMES, out) if n}

    def set_init_pose(self, pose7):
        if pose7 is None:
            lib.alva_system_debug_set_init_pose(self.h, None)
        else:
            p = np.ascontiguousarray(pose7, np.float64)
            lib.alva_system_debug_set_init_pose(self.h, p.ctypes.data)


class SystemGroup:
    """alva_system_group: S AlvaAR sessions advanced one frame per call on `n_threads` host threads (sessions are fibers: a session's
    waits for the GPU run the thread's other sessions).  No reference counterpart (the reference is one System per worker)."""

    def __init__(self, sessions, n_threads: int):
        h = _vp()
        rc = lib.alva_system_group_create(int(n_threads), C.byref(h))
        if rc:
            raise AlvaError("alva_system_group_create failed")
        self.h = h
        self.set_sessions(sessions)

    def stream(self, index: int, device: int = 0):
        """the group's shared HIP stream number `index` (created on first use): pass it to AlvaAR(..., hip_stream=...)"""
        st = _vp()
        if lib.alva_system_group_stream(self.h, device, index, C.byref(st)):
            raise AlvaError("alva_system_group_stream failed")
        return st

    def set_lockstep(self, on: bool):
        """lock-step launches (include/alvaar_system.h): one launch per kernel kind for the sessions of a worker that share a stream"""
        if lib.alva_system_group_set_lockstep(self.h, 1 if on else 0):
            raise AlvaError("alva_system_group_set_lockstep failed")

    def set_lanes(self, lanes: int):
        """number of lanes (group-owned streams that carry the shared tracking-chain launches); session i -> lane (i + i // n_threads) % lanes"""
        if lib.alva_system_group_set_lanes(self.h, int(lanes)):
            raise AlvaError("alva_system_group_set_lanes failed")

    def time_stats(self, reset: bool = True):
        """workers' seconds inside group steps, seconds of them inside session slices that did work (not polls), slices, working slices"""
        out = (C.c_double * 4)()
        if lib.alva_system_group_time_stats(self.h, out, 1 if reset else 0):
            raise AlvaError("alva_system_group_time_stats failed")
        return float(out[0]), float(out[1]), int(out[2]), int(out[3])

    def launch_stats(self):
        """(combined launches issued, session launches they carried) since the group was created"""
        out = (C.c_long * 2)()
        if lib.alva_system_group_launch_stats(self.h, out):
            raise AlvaError("alva_system_group_launch_stats failed")
        return int(out[0]), int(out[1])

    def set_sessions(self, sessions):
        self.sessions = list(sessions)
        n = len(self.sessions)
        self._sys = (_vp * n)(*[s.h for s in self.sessions])
        self._ptr = (_vp * n)()
        self.poses = np.zeros((n, 16), np.float32)
        self.status = np.zeros(n, np.int32)

    def step_device(self, d_rgba_ptrs, timestamp_ms: float):
        """one frame per session (device pointers, one per session); returns the status array (view)"""
        for i, p in enumerate(d_rgba_ptrs):
            self._ptr[i] = p
        rc = lib.alva_system_group_find_camera_pose_device(self.h, len(self.sessions), self._sys, self._ptr, float(timestamp_ms),
                                                           self.poses.ctypes.data, self.status.ctypes.data)
        if rc:
            raise AlvaError("alva_system_group_find_camera_pose_device failed")
        if (self.status < 0).any():
            raise AlvaError(lib.alva_system_last_error().decode() or "a session of the group failed")
        return self.status

    def close(self):
        if getattr(self, "h", None):
            lib.alva_system_group_destroy(self.h)
            self.h = None

    __del__ = close
