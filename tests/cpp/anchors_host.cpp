// The host list of the anchors (alvaar_amd/csrc/slam/anchors.hpp): ids never reused, supports dropped for good and in order, the
// re-attach trigger at exactly half, clearing on a generation change, the 65th anchor refused, removal keeps the order.
#include "../../alvaar_amd/csrc/slam/anchors.hpp"
#include <cstdio>
#include <set>

static int fails = 0, checked = 0;
#define CHECK(c)                                        \
    do {                                                \
        checked++;                                      \
        if (!(c)) {                                     \
            fails++;                                    \
            printf("line %d: %s\n", __LINE__, #c);      \
        }                                               \
    } while (0)

using alva_slam::Anchor;
using alva_slam::Anchors;

static Anchors L;   // (static: 64 anchors of 2.3 KB each)

// supports with the ids base, base + 1, ..; support j at (j, 2 j, 3 j)
static void attach_n(Anchors &A, int k, const float *pose, int count, int base) {
    int ids[64];
    double xyz[64][3];
    for (int j = 0; j < count; j++) {
        ids[j] = base + j;
        xyz[j][0] = j; xyz[j][1] = 2 * j; xyz[j][2] = 3 * j;
    }
    A.attach(k, pose, count, ids, &xyz[0][0]);
}

int main() {
    float pose[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0.5f, 0.25f, 2.f, 1};
    double ref[64 * 3], cur[64 * 3];
    CHECK(L.n == 0 && L.next_id == 0 && !L.full());

    // ---- ids ascend and are not reused: not after a removal, not after clear()
    const int k0 = L.add(pose, 32), k1 = L.add(pose, 8), k2 = L.add(pose, 64);
    CHECK(k0 == 0 && k1 == 1 && k2 == 2 && L.n == 3);
    CHECK(L.list[0].id == 0 && L.list[1].id == 1 && L.list[2].id == 2 && L.list[1].max_support == 8 && L.list[0].age == 0);
    CHECK(L.list[0].alive == 0 && L.list[0].count_at_attach == 0);
    CHECK(L.remove(1) == 1 && L.n == 2 && L.list[0].id == 0 && L.list[1].id == 2 && L.list[1].max_support == 64);   // the order stays
    CHECK(L.remove(1) == 0 && L.remove(77) == 0 && L.n == 2);
    CHECK(L.list[L.add(pose, 16)].id == 3);
    L.clear();
    CHECK(L.n == 0 && L.next_id == 4);
    CHECK(L.list[L.add(pose, 16)].id == 4);
    L.clear();

    // ---- supports: kept in order, dropped for good
    {
        const int k = L.add(pose, 32);
        attach_n(L, k, pose, 10, 100);
        CHECK(L.list[k].alive == 10 && L.list[k].count_at_attach == 10 && !L.wants_attach(k));
        std::set<int> gone = {102, 107};
        auto find = [&](int id, double *xyz) {
            if (gone.count(id)) return false;
            xyz[0] = id; xyz[1] = -id; xyz[2] = 0.5 * id;
            return true;
        };
        CHECK(L.gather(k, find, ref, cur) == 8 && L.list[k].alive == 8 && L.list[k].count_at_attach == 10);
        const int want[8] = {100, 101, 103, 104, 105, 106, 108, 109};
        bool same = true;
        for (int j = 0; j < 8; j++) {
            const int was = want[j] - 100;   // the support's place at attach time: its reference position travels with it
            same = same && L.list[k].sup_id[j] == want[j] && ref[3 * j] == was && ref[3 * j + 1] == 2 * was && ref[3 * j + 2] == 3 * was;
            same = same && cur[3 * j] == want[j] && cur[3 * j + 1] == -want[j] && cur[3 * j + 2] == 0.5 * want[j];
        }
        CHECK(same);
        gone.clear();   // the two come back to the map: not to the anchor
        CHECK(L.gather(k, find, ref, cur) == 8 && L.list[k].sup_id[2] == 103);
        float moved[16];
        for (int c = 0; c < 16; c++) moved[c] = pose[c] + (c == 12 ? 1.f : 0.f);
        L.deliver(k, moved);
        CHECK(L.list[k].age == 1 && L.list[k].last_pose[12] == 1.5f && L.list[k].ref_pose[12] == 0.5f);
        L.clear();
    }

    // ---- the trigger: alive < (count_at_attach + 1) / 2 -- at exactly half nothing happens yet
    for (int count: {9, 10, 64}) {
        const int k = L.add(pose, 64), half = (count + 1) / 2;
        attach_n(L, k, pose, count, 0);
        int limit = count;
        auto find = [&](int id, double *xyz) {
            xyz[0] = xyz[1] = xyz[2] = 0;
            return id < limit;
        };
        limit = half;   // 9 -> 5 alive, 10 -> 5, 64 -> 32
        CHECK(L.gather(k, find, ref, cur) == half && !L.wants_attach(k));
        limit = half - 1;
        CHECK(L.gather(k, find, ref, cur) == half - 1 && L.wants_attach(k));
        // re-attached: the new count is what the trigger compares with from now on
        attach_n(L, k, pose, 6, 500);
        CHECK(L.list[k].alive == 6 && L.list[k].count_at_attach == 6 && !L.wants_attach(k) && L.list[k].sup_id[5] == 505);
        L.clear();
    }
    {   // nothing left alive
        const int k = L.add(pose, 8);
        attach_n(L, k, pose, 8, 0);
        auto none = [](int, double *) { return false; };
        CHECK(L.gather(k, none, ref, cur) == 0 && L.wants_attach(k));
        L.clear();
    }

    // ---- one map: the list clears when the generation moves on, and only then
    {
        L.sync(0);
        L.add(pose, 8);
        L.add(pose, 8);
        const int next = L.next_id;
        L.sync(0);
        CHECK(L.n == 2);
        L.sync(1);
        CHECK(L.n == 0 && L.generation == 1 && L.next_id == next);
        L.add(pose, 8);
        L.sync(1);
        CHECK(L.n == 1 && L.list[0].id == next);
        L.clear();
    }

    // ---- at most 64: the 65th is refused and takes no id
    {
        const int first = L.next_id;
        for (int k = 0; k < Anchors::MAX_ANCHORS; k++) CHECK(L.add(pose, 8) == k);
        CHECK(L.full() && L.n == 64 && L.next_id == first + 64);
        CHECK(L.add(pose, 8) == -1 && L.n == 64 && L.next_id == first + 64);
        CHECK(L.remove(first + 10) == 1 && !L.full());
        CHECK(L.add(pose, 8) == 63 && L.list[63].id == first + 64 && L.list[10].id == first + 11);
    }

    printf("%d %d failures\n", checked, fails);
    return fails ? 1 : 0;
}
