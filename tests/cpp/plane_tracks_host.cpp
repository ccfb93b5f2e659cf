// The host bookkeeping of plane tracking (alvaar_amd/csrc/slam/plane_tracks.hpp): ids kept and dropped, ages, a fresh id after a loss,
// the merge at 9 degrees and none at 11, a merge refused by each offset test alone, a subsumed plane that subsumes nothing, clearing on
// a generation change, and ids never reused.
#include "../../alvaar_amd/csrc/slam/plane_tracks.hpp"
#include <cstdio>
#include <initializer_list>

static int fails = 0, checked = 0;
#define CHECK(c)                                        \
    do {                                                \
        checked++;                                      \
        if (!(c)) {                                     \
            fails++;                                    \
            printf("line %d: %s\n", __LINE__, #c);      \
        }                                               \
    } while (0)

using alva_slam::PlaneTracks;

// a record whose normal is (sin a, 0, -cos a) (a in degrees) and whose centre is p
static void record(float *rec, double a_deg, double px, double py, double pz) {
    for (int k = 0; k < 24; k++) rec[k] = 0.f;
    const double a = a_deg * 3.14159265358979323846 / 180.0;
    rec[4] = (float) std::sin(a); rec[6] = (float) -std::cos(a);
    rec[12] = (float) px; rec[13] = (float) py; rec[14] = (float) pz; rec[15] = 1.f;
}

struct Call {
    float planes[8 * 24];
    int info[8 * 8], ids[8], merged[8];
    Call() {
        for (float &v: planes) v = 0.f;
        for (int &v: info) v = 0;
        for (int s = 0; s < 8; s++) info[8 * s] = 5;
    }
    void plane(int s, int code, double a_deg = 0, double px = 0, double py = 0, double pz = 0) {
        info[8 * s] = code;
        if (code == 0) record(planes + 24 * s, a_deg, px, py, pz);
    }
};

int main() {
    const double th = 0.01;
    PlaneTracks T;
    CHECK(T.n == 0 && T.next_id == 0);
    float pri[8 * 24];
    CHECK(T.priors(pri) == 0);

    // two new planes, far apart: ids 0 and 1, age 0
    {
        Call c;
        c.plane(0, 0, 0, 0, 0, 4);
        c.plane(1, 0, 90, 2, 0, 3);
        c.plane(2, 3);
        CHECK(T.apply(c.planes, c.info, 0, 4, th, c.ids, c.merged) == 2);
        CHECK(c.ids[0] == 0 && c.ids[1] == 1 && c.ids[2] == -1 && c.ids[3] == -1);
        CHECK(c.merged[0] == -1 && c.merged[1] == -1 && c.merged[2] == -1);
        CHECK(T.n == 2 && T.tracks[0].id == 0 && T.tracks[1].id == 1 && T.tracks[0].age == 0 && T.tracks[1].age == 0 && T.next_id == 2);
        CHECK(T.priors(pri) == 2 && pri[14] == 4.f && pri[24 + 12] == 2.f && pri[24 + 15] == 1.f);
    }
    // both kept: same ids, age 1, the new records; a third one found: id 2
    {
        Call c;
        c.plane(0, 0, 0, 0, 0, 4.5);
        c.plane(1, 0, 90, 2, 0, 3);
        c.plane(2, 0, 45, -5, 0, 9);
        CHECK(T.apply(c.planes, c.info, 2, 4, th, c.ids, c.merged) == 3);
        CHECK(c.ids[0] == 0 && c.ids[1] == 1 && c.ids[2] == 2 && c.ids[3] == -1);
        CHECK(T.tracks[0].age == 1 && T.tracks[1].age == 1 && T.tracks[2].age == 0 && T.tracks[0].rec[14] == 4.5f);
    }
    // codes 7, 8 and 9 drop their tracks; the plane found afterwards gets a FRESH id, not a dropped one
    for (int code: {7, 8, 9}) {
        PlaneTracks U = T;
        Call c;
        c.plane(0, 0, 0, 0, 0, 4.5);
        c.plane(1, code);
        c.plane(2, 0, 45, -5, 0, 9);
        c.plane(3, 0, 90, 2, 0, 3);   // (the very plane that was lost, found anew)
        CHECK(U.apply(c.planes, c.info, 3, 4, th, c.ids, c.merged) == 3);
        CHECK(c.ids[0] == 0 && c.ids[1] == -1 && c.ids[2] == 2 && c.ids[3] == 3);
        CHECK(U.n == 3 && U.tracks[0].id == 0 && U.tracks[1].id == 2 && U.tracks[2].id == 3 && U.next_id == 4);
        CHECK(U.tracks[0].age == 2 && U.tracks[1].age == 1 && U.tracks[2].age == 0);
    }

    // merge: normals 9 degrees apart, each centre inside the other's slab; none at 11 degrees
    for (double deg: {9.0, 11.0}) {
        PlaneTracks U;
        Call c;
        c.plane(0, 0, 0, 0, 0, 4);
        c.plane(1, 0, deg, 0, 1, 4);   // the centres differ along y only: perpendicular to both normals
        U.apply(c.planes, c.info, 0, 2, th, c.ids, c.merged);
        CHECK(c.ids[0] == 0 && c.ids[1] == 1 && c.merged[0] == -1);
        if (deg < 10) CHECK(c.merged[1] == 0 && U.n == 1 && U.tracks[0].id == 0 && U.next_id == 2);
        else CHECK(c.merged[1] == -1 && U.n == 2);
    }
    // the opposite normal merges too (|n_a . n_b|)
    {
        PlaneTracks U;
        Call c;
        c.plane(0, 0, 0, 0, 0, 4);
        c.plane(1, 0, 180, 0, 1, 4);
        U.apply(c.planes, c.info, 0, 2, th, c.ids, c.merged);
        CHECK(c.merged[1] == 0 && U.n == 1);
    }
    // each offset test alone refuses: b = (a, 0, 4 + e) with normal n_b = (sin 9, 0, -cos 9)
    //   |n_a . (p_b - p_a)| = e, |n_b . (p_a - p_b)| = |a sin 9 - e cos 9|
    {
        const double s9 = std::sin(9 * 3.14159265358979323846 / 180), c9 = std::cos(9 * 3.14159265358979323846 / 180);
        struct { double a, e; bool first_ok, second_ok; } cases[] = {
            {0, 0.005, true, true},                       // both pass: merged
            {0.02 * c9 / s9, 0.02, false, true},          // a's slab misses b's centre; b's plane passes through a's centre
            {0.5, 0.005, true, false},                    // b's centre lies in a's slab, a's centre is 0.073 off b's plane
        };
        for (const auto &k: cases) {
            PlaneTracks U;
            Call c;
            c.plane(0, 0, 0, 0, 0, 4);
            c.plane(1, 0, 9, k.a, 0, 4 + k.e);
            U.apply(c.planes, c.info, 0, 2, th, c.ids, c.merged);
            const float *ra = c.planes, *rb = c.planes + 24;
            const double d1 = std::fabs(((double) ra[4] * ((double) rb[12] - ra[12]) + (double) ra[5] * ((double) rb[13] - ra[13])) +
                                        (double) ra[6] * ((double) rb[14] - ra[14]));
            const double d2 = std::fabs(((double) rb[4] * ((double) ra[12] - rb[12]) + (double) rb[5] * ((double) ra[13] - rb[13])) +
                                        (double) rb[6] * ((double) ra[14] - rb[14]));
            CHECK((d1 <= th) == k.first_ok && (d2 <= th) == k.second_ok);
            CHECK((c.merged[1] == 0) == (k.first_ok && k.second_ok));
            CHECK(U.n == (k.first_ok && k.second_ok ? 1 : 2));
        }
    }
    // a subsumed plane subsumes nothing: normals at 0, 8 and 16 degrees, the same centre.  1 goes into 0; 2 is within 10 degrees of 1
    // only, and stays
    {
        PlaneTracks U;
        Call c;
        c.plane(0, 0, 0, 0, 0, 4);
        c.plane(1, 0, 8, 0, 0, 4);
        c.plane(2, 0, 16, 0, 0, 4);
        U.apply(c.planes, c.info, 0, 3, th, c.ids, c.merged);
        CHECK(c.merged[0] == -1 && c.merged[1] == 0 && c.merged[2] == -1);
        CHECK(U.n == 2 && U.tracks[0].id == 0 && U.tracks[1].id == 2);
        // next call: the two survivors are priors 0 and 1 and keep their ids
        Call d;
        d.plane(0, 0, 0, 0, 0, 4);
        d.plane(1, 0, 16, 0, 0, 4);
        U.apply(d.planes, d.info, 2, 3, th, d.ids, d.merged);
        CHECK(d.ids[0] == 0 && d.ids[1] == 2 && d.ids[2] == -1 && U.tracks[1].age == 1);
    }
    // a tracked plane can be subsumed by an earlier tracked one; a new plane near it whose own slab misses that plane's centre is not
    {
        PlaneTracks U;
        Call c;
        c.plane(0, 0, 0, 0, 0, 4);
        c.plane(1, 0, 0, 0, 0, 5);
        U.apply(c.planes, c.info, 0, 3, th, c.ids, c.merged);
        CHECK(U.n == 2);
        Call d;
        d.plane(0, 0, 0, 0, 0, 4);
        d.plane(1, 0, 0, 0, 0, 4.004);   // drifted onto plane 0
        d.plane(2, 0, 2, 3, 0, 4.002);   // new, 2 degrees off and 3 away: plane 0's centre is 0.10 off its plane
        U.apply(d.planes, d.info, 2, 3, th, d.ids, d.merged);
        CHECK(d.ids[0] == 0 && d.ids[1] == 1 && d.ids[2] == 2 && d.merged[1] == 0 && d.merged[2] == -1);   // (n_b . (p_a - p_b) = 3 sin 2 for the new one)
        CHECK(U.n == 2 && U.tracks[0].id == 0 && U.tracks[1].id == 2);
    }

    // a generation change clears the list; the same generation does not; ids go on
    {
        PlaneTracks U = T;
        const int next = U.next_id;
        U.sync(U.generation);
        CHECK(U.n == 3);
        U.sync(U.generation + 1);
        CHECK(U.n == 0 && U.next_id == next && U.generation == T.generation + 1);
        Call c;
        c.plane(0, 0, 0, 0, 0, 4);
        U.apply(c.planes, c.info, 0, 1, th, c.ids, c.merged);
        CHECK(c.ids[0] == next && U.next_id == next + 1);
        U.clear();
        CHECK(U.n == 0 && U.next_id == next + 1);
    }
    // ids are never reused: over 20 calls that each lose the plane and find it again
    {
        PlaneTracks U;
        int last = -1;
        for (int k = 0; k < 20; k++) {
            Call c;
            if (U.n) c.plane(0, 7);
            c.plane(U.n, 0, 0, 0, 0, 4);
            U.apply(c.planes, c.info, U.n, 2, th, c.ids, c.merged);
            const int id = c.ids[0] >= 0 ? c.ids[0] : c.ids[1];
            CHECK(id > last);
            last = id;
        }
        CHECK(U.next_id == 20 && U.n == 1);
    }
    printf("%d %d failures\n", checked, fails);
    return fails != 0;
}
