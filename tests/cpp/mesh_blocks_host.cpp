// The host list of the block meshes (alvaar_amd/csrc/slam/mesh_blocks.hpp) driven by a script on stdin, so that
// tests/test_mesh_block_cases.py can compare it with the restatement of G2 - G6 call by call.  The script's lines:
//   reset
//   call <generation> <min_weight> <block> <all> <max_blocks> <max_vertices> <max_triangles> <N> <lx> <ly> <lz> <nb>
//        followed by nb lines "<digest> <nv> <nq>" in the grid's order
// A call prints "info <code> <reported> <vertices> <triangles> <gone> <epoch> <present> <block>" and, unless the code is 3, one line
// "<kx> <ky> <kz> <state> <v0> <nv> <t0> <nt> <digest>" per report; the table is committed unless the code is 3.
#include "../../alvaar_amd/csrc/slam/mesh_blocks.hpp"
#include <cinttypes>
#include <cstdio>
#include <cstring>

using alva_slam::MeshBlockList;

int main() {
    MeshBlockList L;
    char word[16];
    while (scanf("%15s", word) == 1) {
        if (!strcmp(word, "reset")) {
            L.reset();
            continue;
        }
        if (strcmp(word, "call")) return 2;
        long long gen;
        int mw, B, all, max_blocks, max_v, max_t, N, lat[3], nb;
        if (scanf("%lld %d %d %d %d %d %d %d %d %d %d %d", &gen, &mw, &B, &all, &max_blocks, &max_v, &max_t, &N, &lat[0], &lat[1], &lat[2], &nb) != 12)
            return 2;
        int bmin[3], nb3[3];
        MeshBlockList::grid(lat, N, B, bmin, nb3);
        if (nb != nb3[0] * nb3[1] * nb3[2]) return 3;
        std::vector<uint64_t> digest((size_t) nb);
        std::vector<int> counts(2 * (size_t) nb);
        for (int b = 0; b < nb; b++)
            if (scanf("%" SCNu64 " %d %d", &digest[(size_t) b], &counts[2 * (size_t) b], &counts[2 * (size_t) b + 1]) != 3) return 2;
        L.begin(gen, mw, B);
        MeshBlockList::Plan P;
        L.plan(lat, N, digest.data(), counts.data(), all != 0, max_blocks, max_v, max_t, P);
        printf("info %d %d %d %d %d %d %d %d\n", P.code, (int) P.reports.size(), P.vertices, P.triangles, P.gone, L.epoch, P.present, L.block);
        if (P.code == 3) continue;
        int v0 = 0, t0 = 0;
        for (const MeshBlockList::Report &r: P.reports) {
            printf("%d %d %d %d %d %d %d %d %" PRIu64 "\n", r.key[0], r.key[1], r.key[2], r.state, r.nv ? v0 : 0, r.nv, r.nt ? t0 : 0, r.nt, r.digest);
            v0 += r.nv;
            t0 += r.nt;
        }
        L.commit(lat, N, digest.data(), counts.data());
    }
    return 0;
}
