// The host list behind alva_system_mesh_blocks (G2 - G6 of include/alvaar_system.h): the present blocks of the last successful call, key ->
// digest, and what a new digest pass changes in it.  Plain C++, no HIP: the stages (alva_mesh_block_digest / alva_mesh_extract_blocks)
// are the caller's.  A call is begin (G2), plan (G4, G5: const, so an over-cap call leaves the table as it was) and commit (G6).
// tests/cpp/mesh_blocks_host.cpp drives it against the restatement in tests/mesh_block_cases.py.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace alva_slam {

struct MeshBlockList {
    struct Entry {
        int key[3];   // (b_x, b_y, b_z)
        uint64_t digest;
    };
    struct Report {
        int key[3];
        int state;    // 0 unchanged (ALL only), 1 new, 2 changed, 3 no surface any more, 4 left the cube
        int nv, nt;   // zero for states 3 and 4
        uint64_t digest;
    };
    struct Plan {
        std::vector<Report> reports;   // the blocks to extract, in ascending key order, then the gone ones, in ascending key order
        int n_extract = 0, vertices = 0, triangles = 0, gone = 0, present = 0;
        int code = 0;   // 0, or 3: more reports than max_blocks, or more vertices or triangles than their caps
    };

    std::vector<Entry> table;   // ascending (b_z, b_y, b_x)
    int epoch = 0, min_weight = 0, block = 0;
    long long generation = -1;   // the volume's (what empties, places or replaces it moves it on); -1: no call yet

    static bool less(const int *a, const int *b) {
        return a[2] != b[2] ? a[2] < b[2] : a[1] != b[1] ? a[1] < b[1] : a[0] < b[0];
    }
    static int floor_div(int g, int B) { return g >= 0 ? g / B : -((-g + B - 1) / B); }

    // alva_system_reset_mesh_blocks: everything is reported anew
    void reset() {
        table.clear();
        epoch++;
    }

    // G2: the table is of one volume, one min_weight and one block edge.  A shift is none of these
    void begin(long long volume_generation, int min_weight_, int block_) {
        if (volume_generation != generation || min_weight_ != min_weight || block_ != block) reset();
        generation = volume_generation;
        min_weight = min_weight_;
        block = block_;
    }

    // L1's grid of a volume of N^3 voxels at `lattice`
    static void grid(const int *lattice, int N, int B, int *bmin, int *nb) {
        for (int a = 0; a < 3; a++) {
            bmin[a] = floor_div(lattice[a], B);
            nb[a] = floor_div(lattice[a] + N - 1, B) - bmin[a] + 1;
        }
    }

    // G4, G5: digest [nb] and counts [nb][2] = (nv, nq) are the digest stage's, in the grid's order
    void plan(const int *lattice, int N, const uint64_t *digest, const int *counts, bool all, int max_blocks, int max_vertices, int max_triangles,
              Plan &P) const {
        int bmin[3], nb[3];
        grid(lattice, N, block, bmin, nb);
        P = Plan();
        std::vector<Report> gone;
        size_t t = 0;   // the table and the grid are both ascending: one merge
        long long sv = 0, st = 0;
        const auto leave = [&](const Entry &e) {
            bool in_grid = true;
            for (int a = 0; a < 3; a++) in_grid = in_grid && e.key[a] >= bmin[a] && e.key[a] < bmin[a] + nb[a];
            gone.push_back(Report{{e.key[0], e.key[1], e.key[2]}, in_grid ? 3 : 4, 0, 0, e.digest});
        };
        int at = 0;
        for (int z = 0; z < nb[2]; z++)
            for (int y = 0; y < nb[1]; y++)
                for (int x = 0; x < nb[0]; x++, at++) {
                    if (counts[2 * at + 1] <= 0) continue;   // L4: not present
                    const int key[3] = {bmin[0] + x, bmin[1] + y, bmin[2] + z};
                    P.present++;
                    while (t < table.size() && less(table[t].key, key)) leave(table[t++]);
                    int state = 1;
                    if (t < table.size() && !less(key, table[t].key)) state = table[t++].digest == digest[at] ? 0 : 2;
                    if (state == 0 && !all) continue;
                    P.reports.push_back(Report{{key[0], key[1], key[2]}, state, counts[2 * at], 2 * counts[2 * at + 1], digest[at]});
                    sv += counts[2 * at];
                    st += 2 * (long long) counts[2 * at + 1];
                }
        while (t < table.size()) leave(table[t++]);
        P.n_extract = (int) P.reports.size();
        P.gone = (int) gone.size();
        P.reports.insert(P.reports.end(), gone.begin(), gone.end());
        const long long cap = 0x7fffffff;
        P.vertices = (int) (sv < cap ? sv : cap);
        P.triangles = (int) (st < cap ? st : cap);
        P.code = (long long) P.reports.size() > max_blocks || sv > max_vertices || st > max_triangles ? 3 : 0;
    }

    // G6: the table becomes the present blocks' digests
    void commit(const int *lattice, int N, const uint64_t *digest, const int *counts) {
        int bmin[3], nb[3];
        grid(lattice, N, block, bmin, nb);
        table.clear();
        int at = 0;
        for (int z = 0; z < nb[2]; z++)
            for (int y = 0; y < nb[1]; y++)
                for (int x = 0; x < nb[0]; x++, at++)
                    if (counts[2 * at + 1] > 0) table.push_back(Entry{{bmin[0] + x, bmin[1] + y, bmin[2] + z}, digest[at]});
    }
};

}  // namespace alva_slam
