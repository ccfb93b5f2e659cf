// Image detection, the host side (plain C++, no HIP; checked by tests/cpp/image_place_host.cpp): what follows the device stages
// alva_image_match / alva_image_homography (include/alvaar_hip.h) -- the re-count under the refined pose, the quad, and the scale and
// placement of a picture whose pose is known in units of its own width.
//
// The picture's frame: origin at its centre, x to its right, y down, z = x cross y (away from a viewer facing it), one unit = its width;
// a picture of w x h pixels covers |x| <= 1/2, |y| <= h / (2 w).  (R, t): X_cam = R p + t, R row-major with the columns r1 r2 r3.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>
#include "se3.hpp"

namespace alva_slam {

constexpr int IMAGE_MIN_SCALE_POINTS = 8;

// the pairs (x, y picture pixels, u, v undistorted frame pixels) within threshold_px of the pose's projection; mask [m] may be null
inline int image_count_inliers(const double *R, const double *t, int w, int h, const double *calib4, const double *xy4, int m, double threshold_px,
                               unsigned char *mask) {
    int count = 0;
    for (int i = 0; i < m; i++) {
        const double px = (xy4[4 * i] - (double) w / 2) / (double) w, py = (xy4[4 * i + 1] - (double) h / 2) / (double) w;
        const double X = (R[0] * px + R[1] * py) + t[0], Y = (R[3] * px + R[4] * py) + t[1], Z = (R[6] * px + R[7] * py) + t[2];
        bool in = false;
        if (Z > 0) {
            const double du = (calib4[0] * X / Z + calib4[2]) - xy4[4 * i + 2], dv = (calib4[1] * Y / Z + calib4[3]) - xy4[4 * i + 3];
            in = du * du + dv * dv <= threshold_px * threshold_px;
        }
        if (mask) mask[i] = in ? 1 : 0;
        count += in ? 1 : 0;
    }
    return count;
}

// the four corners (top-left, top-right, bottom-right, bottom-left) in undistorted frame pixels; false when one is not in front
inline bool image_quad(const double *R, const double *t, double aspect, const double *calib4, float *quad8) {
    const double cx[4] = {-0.5, 0.5, 0.5, -0.5}, cy[4] = {-0.5 * aspect, -0.5 * aspect, 0.5 * aspect, 0.5 * aspect};
    bool ok = true;
    for (int k = 0; k < 4; k++) {
        const double X = (R[0] * cx[k] + R[1] * cy[k]) + t[0], Y = (R[3] * cx[k] + R[4] * cy[k]) + t[1], Z = (R[6] * cx[k] + R[7] * cy[k]) + t[2];
        if (!(Z > 0)) ok = false;
        quad8[2 * k] = (float) (calib4[0] * X / Z + calib4[2]);
        quad8[2 * k + 1] = (float) (calib4[1] * Y / Z + calib4[3]);
    }
    return ok;
}

// For every point (camera coordinates, map units) in front of the camera: its ray is intersected with the picture's plane; where the
// intersection lies inside the picture (borders included), the ratio map depth / unit-width depth is kept
inline void image_scale_ratios(const double *R, const double *t, double aspect, const double *pts_cam, int n, std::vector<double> &ratios) {
    ratios.clear();
    const double r1[3] = {R[0], R[3], R[6]}, r2[3] = {R[1], R[4], R[7]}, r3[3] = {R[2], R[5], R[8]};
    const double nt = (r3[0] * t[0] + r3[1] * t[1]) + r3[2] * t[2];
    for (int i = 0; i < n; i++) {
        const double *P = pts_cam + 3 * i;
        if (!(P[2] > 0)) continue;   // behind the camera
        const double d[3] = {P[0] / P[2], P[1] / P[2], 1.0};
        const double nd = (r3[0] * d[0] + r3[1] * d[1]) + r3[2] * d[2];
        if (!(std::fabs(nd) > 1e-12)) continue;   // the ray runs along the plane
        const double lam = nt / nd;   // (d.z = 1: lam is the unit-width depth)
        if (!(lam > 0)) continue;
        const double q[3] = {lam * d[0] - t[0], lam * d[1] - t[1], lam * d[2] - t[2]};
        const double x = (r1[0] * q[0] + r1[1] * q[1]) + r1[2] * q[2], y = (r2[0] * q[0] + r2[1] * q[1]) + r2[2] * q[2];
        if (std::fabs(x) <= 0.5 && std::fabs(y) <= 0.5 * aspect) ratios.push_back(P[2] / lam);
    }
}

// the element of rank c / 2 (0-based, ascending) of the c ratios: the picture's width in map units.  False when c < IMAGE_MIN_SCALE_POINTS
inline bool image_width_from_ratios(std::vector<double> ratios, double *width) {
    const size_t c = ratios.size();
    if (c < (size_t) IMAGE_MIN_SCALE_POINTS) return false;
    std::nth_element(ratios.begin(), ratios.begin() + c / 2, ratios.end());
    *width = ratios[c / 2];
    return true;
}

// the world pose of the picture: the camera pose composed with the scaled picture pose.  pose16 in alva_find_plane's layout
// (out[4 c + r] = Rot[r][c], out[12..14] = the centre, out[15] = 1) with the columns x = the picture's right, y = its normal towards the
// viewer (= -r3), z = down the picture (ARCore's convention; x cross y = z)
inline void image_world_pose(const double *R, const double *t, double width, const SE3 &Twc, float *pose16) {
    double Rwc[9];
    quat_to_rot(Twc.q, Rwc);
    const double col[3][3] = {{R[0], R[3], R[6]}, {-R[2], -R[5], -R[8]}, {R[1], R[4], R[7]}};
    for (int c = 0; c < 3; c++)
        for (int r = 0; r < 3; r++) pose16[4 * c + r] = (float) ((Rwc[3 * r] * col[c][0] + Rwc[3 * r + 1] * col[c][1]) + Rwc[3 * r + 2] * col[c][2]);
    for (int r = 0; r < 3; r++)
        pose16[12 + r] = (float) (((Rwc[3 * r] * (width * t[0]) + Rwc[3 * r + 1] * (width * t[1])) + Rwc[3 * r + 2] * (width * t[2])) + Twc.t[r]);
    pose16[3] = pose16[7] = pose16[11] = 0.f;
    pose16[15] = 1.f;
}

// (R, t) of the picture in the camera <-> the camera's pose in the picture's frame (t, q = x y z w), the form alva_pnp_refine works on
inline void image_pose_to_twc7(const double *R, const double *t, double *pose7) {
    SE3 T;
    double Rt[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) Rt[3 * r + c] = R[3 * c + r];
    rot_to_quat(Rt, T.q);
    for (int r = 0; r < 3; r++) T.t[r] = -((Rt[3 * r] * t[0] + Rt[3 * r + 1] * t[1]) + Rt[3 * r + 2] * t[2]);
    se3_to_pose7(T, pose7);
}
inline void image_pose_from_twc7(const double *pose7, double *R, double *t) {
    const SE3 T = se3_from_pose7(pose7);
    double Rwc[9];
    quat_to_rot(T.q, Rwc);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) R[3 * r + c] = Rwc[3 * c + r];
    for (int r = 0; r < 3; r++) t[r] = -((R[3 * r] * T.t[0] + R[3 * r + 1] * T.t[1]) + R[3 * r + 2] * T.t[2]);
}

}  // namespace alva_slam
