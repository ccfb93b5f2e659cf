// The compaction's slicing rule (alvaar_amd/csrc/track_slices.hpp) for every slot count a frame can have: the slices of both launch
// shapes cover [0, n); the fused pose launch's are never empty, fit its 512-thread workgroup, and keep the grid it had up to 6144 slots.
#include "../../alvaar_amd/csrc/track_slices.hpp"
#include <algorithm>
#include <cstdio>

static int fails = 0;
#define CHECK(c, ...)                              \
    do {                                           \
        if (!(c) && fails++ < 20) {                \
            printf("n=%d: %s: ", n, #c);           \
            printf(__VA_ARGS__);                   \
            printf("\n");                          \
        }                                          \
    } while (0)

int main() {
    long checked = 0;
    for (int n = 1; n <= 19000; n++) {
        for (int shape = 0; shape < 2; shape++) {
            const int G = shape ? track_pose_all_grid(n) : track_compact_grid(n);
            const int per = track_slice_len(n, G);
            CHECK(G >= 1 && per % 64 == 0, "G=%d per=%d", G, per);
            int next = 0;   // the slices in workgroup order: contiguous, no gap, no overlap
            for (int g = 0; g < G; g++) {
                const int lo = g * per, hi = std::min(n, lo + per);
                if (lo < hi) {
                    CHECK(lo == next, "shape %d slice %d starts at %d, expected %d", shape, g, lo, next);
                    next = hi;
                } else {
                    CHECK(shape == 0, "fused launch: slice %d of %d is empty (per=%d)", g, G, per);
                }
            }
            CHECK(next == n, "shape %d covers [0, %d)", shape, next);
            if (shape == 1) {
                CHECK(per <= 512, "per=%d", per);
                CHECK(G <= 96, "G=%d", G);
                if (n <= 6144) CHECK(G == std::min(96, (n + 63) / 64), "G=%d", G);
            } else {
                CHECK(G == std::max(1, std::min(CMP_MAX_WG, (n + 255) / 256)), "G=%d", G);
            }
            checked++;
        }
    }
    printf("%ld %d failures\n", checked, fails);
    return fails != 0;
}
