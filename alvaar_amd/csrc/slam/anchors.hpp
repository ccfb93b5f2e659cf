// The anchors a session keeps between calls of alva_system_create_anchors / alva_system_update_anchors (ARCore's Anchor, ARKit's
// ARAnchor, WebXR's XRAnchor).  Plain C++, no HIP: the stages (alva_anchor_attach, alva_anchor_update) find the supports and the motion,
// this list only names and keeps.  tests/cpp/anchors_host.cpp checks it.
//
// The list holds at most 64 anchors in ascending id.  Per anchor: its id and age, the reference pose (the pose it had when its supports
// were chosen), K and the number of supports chosen then, the supports that are still alive -- map point ids in alva_anchor_attach's
// order with their positions at that time -- and the last pose delivered.
//   add          a new anchor at the list's end under the id next_id++; -1 when the list is full (the 65th is refused)
//   attach       the anchor's reference pose and supports: at creation, and again when it is re-attached
//   gather       what alva_anchor_update needs: for every support whose id `find` still knows, the reference and the current position, in
//                the list's order; a support that `find` does not know (culled, or absorbed by a merge) is dropped FOR GOOD
//   deliver      the pose of an update: kept as the last delivered pose, age + 1
//   wants_attach after an update: fewer supports alive than half the number at attach, alive < (count_at_attach + 1) / 2
// Ids are never reused: clear() empties the list and leaves next_id alone.  The list belongs to one map: sync() clears it when the map's
// generation has moved on.
#pragma once
#include <cstring>

namespace alva_slam {

struct Anchor {
    static constexpr int MAX_SUPPORT = 64;
    int id, age;
    int max_support;       // K
    int count_at_attach;   // min(K, points looked at) when the supports were chosen
    int alive;             // supports still in the list: sup_id[0 .. alive), sup_ref[0 .. alive)
    float ref_pose[16], last_pose[16];
    int sup_id[MAX_SUPPORT];
    double sup_ref[MAX_SUPPORT][3];
};

struct Anchors {
    static constexpr int MAX_ANCHORS = 64;
    Anchor list[MAX_ANCHORS];
    int n = 0;
    int next_id = 0;
    long generation = 0;

    void clear() { n = 0; }
    void sync(long map_generation) {
        if (map_generation != generation) clear();
        generation = map_generation;
    }
    bool full() const { return n == MAX_ANCHORS; }

    // the new anchor's place in the list, or -1 when it is full; it has no supports until attach()
    int add(const float *pose16, int max_support) {
        if (full()) return -1;
        Anchor &a = list[n];
        a.id = next_id++;
        a.age = 0;
        a.max_support = max_support;
        a.count_at_attach = a.alive = 0;
        std::memcpy(a.ref_pose, pose16, sizeof(a.ref_pose));
        std::memcpy(a.last_pose, pose16, sizeof(a.last_pose));
        return n++;
    }
    // ids [count], xyz [count][3]: alva_anchor_attach's support, in its order, and where those points are now
    void attach(int k, const float *pose16, int count, const int *ids, const double *xyz) {
        Anchor &a = list[k];
        std::memcpy(a.ref_pose, pose16, sizeof(a.ref_pose));
        std::memcpy(a.last_pose, pose16, sizeof(a.last_pose));
        a.count_at_attach = a.alive = count;
        std::memcpy(a.sup_id, ids, (size_t) count * sizeof(int));
        std::memcpy(a.sup_ref, xyz, (size_t) count * 3 * sizeof(double));
    }
    // find(id, xyz3) -> bool: whether map point id is a 3-D point of the map now, and where.  ref, cur: [MAX_SUPPORT][3], the first
    // `alive` rows are written.  Returns alive
    template <class Find>
    int gather(int k, Find &&find, double *ref, double *cur) {
        Anchor &a = list[k];
        int m = 0;
        for (int j = 0; j < a.alive; j++) {
            double now[3];
            if (!find(a.sup_id[j], now)) continue;
            a.sup_id[m] = a.sup_id[j];
            std::memmove(a.sup_ref[m], a.sup_ref[j], sizeof(a.sup_ref[m]));
            std::memcpy(ref + 3 * m, a.sup_ref[m], sizeof(a.sup_ref[m]));
            std::memcpy(cur + 3 * m, now, sizeof(now));
            m++;
        }
        return a.alive = m;
    }
    void deliver(int k, const float *pose16) {
        std::memcpy(list[k].last_pose, pose16, sizeof(list[k].last_pose));
        list[k].age++;
    }
    bool wants_attach(int k) const { return list[k].alive < (list[k].count_at_attach + 1) / 2; }
    // 1: removed (the later anchors move up, the order stays), 0: no such id
    int remove(int id) {
        for (int k = 0; k < n; k++)
            if (list[k].id == id) {
                for (int j = k + 1; j < n; j++) list[j - 1] = list[j];
                n--;
                return 1;
            }
        return 0;
    }
};

}  // namespace alva_slam
