// The planes a session keeps between calls of alva_system_track_planes: ids, ages and merging (ARCore's Plane trackables with
// getSubsumedBy, ARKit's ARPlaneAnchor updates, WebXR's XRPlane set).  Plain C++, no HIP: the stage (alva_track_planes) refits and finds,
// this list only names.  tests/cpp/plane_tracks_host.cpp checks it.
//
// The list holds at most 8 tracks in ascending id.  A call hands priors() to the stage -- track k becomes prior k and keeps slot k -- and
// the stage's answer to apply():
//   a tracked slot (< n_prior) with code 0   keeps its id, takes the new record, age + 1
//   a tracked slot with another code          (7 lost, 8 lost after the refit, 9 unusable record) leaves the list
//   a new slot (>= n_prior) with code 0       gets the id next_id++ and age 0
//   merge        over the surviving planes in slot order: plane b is subsumed by the first earlier survivor a (a < b) that is not itself
//                subsumed and for which, with the records cast to double, n = rec[4..6], p = rec[12..14] and every dot product
//                associated (x + y) + z:   |n_a . n_b| >= cos 10 deg,   |n_a . (p_b - p_a)| <= thickness,   |n_b . (p_a - p_b)| <= thickness.
//                out_merged_into[b] = a's id; b's record, id and labels are still the caller's for this call, but b leaves the list, so
//                the next call's claim hands its points to a.  A subsumed plane subsumes nothing
// Ids are never reused: clear() empties the list and leaves next_id alone.  The list belongs to one map: sync() clears it when the
// map's generation has moved on.
#pragma once
#include <cmath>
#include <cstring>

namespace alva_slam {

struct PlaneTrack {
    float rec[24];
    int id;
    int age;
};

struct PlaneTracks {
    static constexpr int MAX_TRACKS = 8;
    static constexpr double COS_MERGE = 0.98480775301220802;   // cos 10 deg
    PlaneTrack tracks[MAX_TRACKS];
    int n = 0;
    int next_id = 0;
    long generation = 0;

    void clear() { n = 0; }
    void sync(long map_generation) {
        if (map_generation != generation) clear();
        generation = map_generation;
    }
    // the records in list order, into out24 [n][24]; returns n
    int priors(float *out24) const {
        for (int k = 0; k < n; k++) std::memcpy(out24 + 24 * k, tracks[k].rec, sizeof(tracks[k].rec));
        return n;
    }

    static double dot3(const double *a, const double *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
    static bool subsumes(const float *ra, const float *rb, double thickness) {
        double na[3], nb[3], ab[3], ba[3];
        for (int k = 0; k < 3; k++) {
            na[k] = (double) ra[4 + k];
            nb[k] = (double) rb[4 + k];
            ab[k] = (double) rb[12 + k] - (double) ra[12 + k];
            ba[k] = (double) ra[12 + k] - (double) rb[12 + k];
        }
        return std::fabs(dot3(na, nb)) >= COS_MERGE && std::fabs(dot3(na, ab)) <= thickness && std::fabs(dot3(nb, ba)) <= thickness;
    }

    // planes24 [max_planes][24], info8 [max_planes][8]: the stage's answer to priors(); n_prior == n.  out_ids, out_merged_into
    // [max_planes]: the id of every code-0 slot and the id of the plane that subsumed it, -1 otherwise.  Returns the new list length
    int apply(const float *planes24, const int *info8, int n_prior, int max_planes, double thickness, int *out_ids, int *out_merged_into) {
        PlaneTrack alive[MAX_TRACKS];
        int slot_of[MAX_TRACKS], m = 0;
        for (int s = 0; s < max_planes; s++) {
            out_ids[s] = out_merged_into[s] = -1;
            if (info8[8 * s] != 0 || m == MAX_TRACKS) continue;
            PlaneTrack t;
            std::memcpy(t.rec, planes24 + 24 * s, sizeof(t.rec));
            if (s < n_prior && s < n) {
                t.id = tracks[s].id;
                t.age = tracks[s].age + 1;
            } else {
                t.id = next_id++;
                t.age = 0;
            }
            out_ids[s] = t.id;
            slot_of[m] = s;
            alive[m++] = t;
        }
        bool gone[MAX_TRACKS] = {false};
        for (int b = 1; b < m; b++)
            for (int a = 0; a < b; a++)
                if (!gone[a] && subsumes(alive[a].rec, alive[b].rec, thickness)) {
                    gone[b] = true;
                    out_merged_into[slot_of[b]] = alive[a].id;
                    break;
                }
        n = 0;
        for (int k = 0; k < m; k++)
            if (!gone[k]) tracks[n++] = alive[k];
        return n;
    }
};

}  // namespace alva_slam
