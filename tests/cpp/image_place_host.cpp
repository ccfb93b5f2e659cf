// The host side of image detection (alvaar_amd/csrc/slam/image_place.hpp): the median rank of the scale, the inside test at the
// picture's border, c = 7 against c = 8, a point behind the camera, the axes of the world pose and their handedness, the quad's corner
// order, the re-count at its threshold, and the pose <-> Twc round trip.
#include "../../alvaar_amd/csrc/slam/image_place.hpp"
#include <cstdio>

static int fails = 0, checked = 0;
#define CHECK(c)                                        \
    do {                                                \
        checked++;                                      \
        if (!(c)) {                                     \
            fails++;                                    \
            printf("line %d: %s\n", __LINE__, #c);      \
        }                                               \
    } while (0)

using namespace alva_slam;

static bool near(double a, double b, double tol = 1e-12) { return std::fabs(a - b) <= tol; }

int main() {
    // a picture facing the camera squarely, two widths away: R = I (x right, y down, z away), t = (0, 0, 2); 4 : 3, so |y| <= 0.375
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 2};
    const double aspect = 0.75;
    std::vector<double> ratios;

    // ---- the inside test, borders included: a map point whose ray meets the plane at (x, y) lies at (x d / 2, y d / 2, d) for any depth d
    auto point = [](double x, double y, double d, double *P) { P[0] = x * d / 2; P[1] = y * d / 2; P[2] = d; };
    {
        double P[6 * 3];
        point(0.5, 0.0, 10, P);          // on the right border: in
        point(-0.5, 0.375, 10, P + 3);   // on the bottom-left corner: in
        point(0.5000001, 0.0, 10, P + 6);    // a hair outside in x
        point(0.0, -0.3750001, 10, P + 9);   // a hair outside in y
        point(0.1, 0.1, -10, P + 12);    // behind the camera (the ray would meet the picture)
        point(0.0, 0.0, 4, P + 15);      // the centre
        image_scale_ratios(I, t, aspect, P, 6, ratios);
        CHECK(ratios.size() == 3);
        CHECK(near(ratios[0], 5) && near(ratios[1], 5) && near(ratios[2], 2));   // map depth / unit-width depth (2)
    }
    // ---- the rank c / 2 of the ratios; c = 7 is refused, c = 8 is not
    {
        const double depth[9] = {9, 1, 8, 2, 7, 3, 6, 4, 5};   // ratios = depth / 2
        double P[9 * 3], width = -1;
        for (int i = 0; i < 9; i++) point(0.01 * i, -0.01 * i, depth[i], P + 3 * i);
        image_scale_ratios(I, t, aspect, P, 7, ratios);
        CHECK(ratios.size() == 7 && !image_width_from_ratios(ratios, &width) && width == -1);
        image_scale_ratios(I, t, aspect, P, 8, ratios);   // {9 1 8 2 7 3 6 4} / 2: rank 4 of the sorted {1 2 3 4 6 7 8 9} is 6
        CHECK(ratios.size() == 8 && image_width_from_ratios(ratios, &width) && near(width, 3.0));
        image_scale_ratios(I, t, aspect, P, 9, ratios);   // rank 4 of {1 .. 9} is 5
        CHECK(image_width_from_ratios(ratios, &width) && near(width, 2.5));
    }
    // ---- a ray along the plane and a plane behind the camera give nothing
    {
        const double Redge[9] = {0, 0, 1, 0, 1, 0, -1, 0, 0};   // the picture seen edge-on: r3 = (1, 0, 0)
        const double P[3] = {0, 0.1, 5}, tb[3] = {0, 0, -2};
        image_scale_ratios(Redge, t, aspect, P, 1, ratios);     // the ray (0, 0.02, 1) runs along the plane x = 0
        CHECK(ratios.empty());
        image_scale_ratios(I, tb, aspect, P, 1, ratios);        // lam < 0
        CHECK(ratios.empty());
    }
    // ---- the world pose: camera at (1, 2, 3) looking along the world's x axis (camera x = world -y ... a proper rotation), width 3
    {
        SE3 Twc;
        const double Rwc[9] = {0, 0, 1, -1, 0, 0, 0, -1, 0};   // columns: camera x = (0,-1,0), y = (0,0,-1), z = (1,0,0)
        rot_to_quat(Rwc, Twc.q);
        Twc.t[0] = 1; Twc.t[1] = 2; Twc.t[2] = 3;
        float pose[16];
        image_world_pose(I, t, 3.0, Twc, pose);
        // x = the picture's right = camera x; y = the normal towards the viewer = -camera z; z = down the picture = camera y
        CHECK(near(pose[0], 0, 1e-6) && near(pose[1], -1, 1e-6) && near(pose[2], 0, 1e-6));
        CHECK(near(pose[4], -1, 1e-6) && near(pose[5], 0, 1e-6) && near(pose[6], 0, 1e-6));
        CHECK(near(pose[8], 0, 1e-6) && near(pose[9], 0, 1e-6) && near(pose[10], -1, 1e-6));
        // the centre: 3 x 2 = 6 map units along the camera's z = world x
        CHECK(near(pose[12], 7, 1e-6) && near(pose[13], 2, 1e-6) && near(pose[14], 3, 1e-6));
        CHECK(pose[3] == 0 && pose[7] == 0 && pose[11] == 0 && pose[15] == 1);
        // right-handed: x cross y = z; and the normal looks back at the camera
        const float *x = pose, *y = pose + 4, *z = pose + 8;
        CHECK(near(x[1] * y[2] - x[2] * y[1], z[0], 1e-6) && near(x[2] * y[0] - x[0] * y[2], z[1], 1e-6) && near(x[0] * y[1] - x[1] * y[0], z[2], 1e-6));
        CHECK(y[0] * (Twc.t[0] - pose[12]) + y[1] * (Twc.t[1] - pose[13]) + y[2] * (Twc.t[2] - pose[14]) > 0);
    }
    // ---- the quad: top-left, top-right, bottom-right, bottom-left; a corner behind the camera is refused
    {
        const double calib[4] = {500, 500, 320, 240};
        float quad[8];
        CHECK(image_quad(I, t, aspect, calib, quad));
        CHECK(near(quad[0], 320 - 125, 1e-4) && near(quad[1], 240 - 93.75, 1e-4) && near(quad[2], 320 + 125, 1e-4) && near(quad[3], 240 - 93.75, 1e-4));
        CHECK(near(quad[4], 320 + 125, 1e-4) && near(quad[5], 240 + 93.75, 1e-4) && near(quad[6], 320 - 125, 1e-4) && near(quad[7], 240 + 93.75, 1e-4));
        const double Rtilt[9] = {0, 0, 1, 0, 1, 0, -1, 0, 0}, tnear[3] = {0, 0, 0.25};   // the right half reaches behind the camera
        CHECK(!image_quad(Rtilt, tnear, aspect, calib, quad));
        // ---- the re-count: picture 200 x 150, the pair (100, 75) is the centre and projects to (320, 240)
        const double xy[4 * 4] = {100, 75, 320, 240, 100, 75, 323, 240, 100, 75, 323, 240.1, 100, 75, 320, 237};
        unsigned char mask[4];
        CHECK(image_count_inliers(I, t, 200, 150, calib, xy, 4, 3.0, mask) == 3);   // 3 px exactly is in, a hair more is out
        CHECK(mask[0] == 1 && mask[1] == 1 && mask[2] == 0 && mask[3] == 1);
        const double tb[3] = {0, 0, -2};
        CHECK(image_count_inliers(I, tb, 200, 150, calib, xy, 4, 1e9, nullptr) == 0);   // behind the camera
    }
    // ---- (R, t) <-> the camera's pose in the picture's frame, and back
    {
        const double c = std::cos(0.3), s = std::sin(0.3);
        const double R[9] = {c, 0, s, 0, 1, 0, -s, 0, c}, tt[3] = {0.1, -0.2, 1.7};
        double pose7[7], R2[9], t2[3];
        image_pose_to_twc7(R, tt, pose7);
        // the camera sits at -R^T t
        CHECK(near(pose7[0], -(c * 0.1 - s * 1.7)) && near(pose7[1], 0.2) && near(pose7[2], -(s * 0.1 + c * 1.7)));
        image_pose_from_twc7(pose7, R2, t2);
        bool same = true;
        for (int i = 0; i < 9; i++) same = same && near(R[i], R2[i], 1e-12);
        for (int i = 0; i < 3; i++) same = same && near(tt[i], t2[i], 1e-12);
        CHECK(same);
    }
    printf("%d %d failures\n", checked, fails);
    return fails ? 1 : 0;
}
