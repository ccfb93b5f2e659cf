// The host-compilable part of the plane fitters' shared header (alvaar_amd/csrc/plane_fit.hpp): the sample hash against the
// hand-computed values of tests/test_hit_cases.py, the word-to-index map at its ends, the plane through three points, and the host
// eigen-solve on matrices whose answer is exact.
#include "../../alvaar_amd/csrc/plane_fit.hpp"
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

int main() {
    // the hash: see test_hash32_against_hand_computed_values for the derivations
    CHECK(alva_hash32(0u) == 0u);
    CHECK(alva_hash32(1u) == 0x688990C0u);
    CHECK(alva_hash32(12345u) == 0x912EFCF7u);

    // the index map floor(w m / 2^32): m = 1 has one index, m = 2048 takes the top 11 bits, the largest word gives m - 1
    for (uint32_t w: {0u, 1u, 0x7fffffffu, 0x80000000u, 0xffffffffu}) {
        CHECK(alva_sample_index(w, 1) == 0);
        CHECK(alva_sample_index(w, 2048) == (int) (w >> 21));
    }
    for (int m: {1, 7, 24, 2048, 16384}) CHECK(alva_sample_index(0xffffffffu, m) == m - 1);

    // three indices of hypothesis k: word 3 k + j of the stream, hashed or explicit; equal indices are refused
    {
        int idx[3];
        const uint32_t seed = 12345u;
        CHECK(alva_sample3(nullptr, seed, 1u, 2048, idx));
        for (uint32_t j = 0; j < 3; j++) CHECK(idx[j] == (int) (alva_hash32(seed ^ ((3u + j) * 0x9E3779B9u)) >> 21));
        const uint32_t words[6] = {0u, 0u, 0u, 0u, 0x80000000u, 0xffffffffu};
        CHECK(!alva_sample3(words, seed, 0u, 24, idx));
        CHECK(alva_sample3(words, seed, 1u, 24, idx) && idx[0] == 0 && idx[1] == 12 && idx[2] == 23);
    }

    // the plane through three points
    {
        double q0[3], nh[3] = {7, 7, 7};
        const double a[3] = {1, 2, 3}, b[3] = {2, 4, 6}, c[3] = {-1, -2, -3};   // collinear
        CHECK(!plane_through3(a, b, c, q0, nh));
        CHECK(!plane_through3(a, a, b, q0, nh));
        // u = (1, 0, 0), w = (0, 3, 4): u x w = (0, -4, 3) of length 5
        const double p1[3] = {2, 2, 3}, p2[3] = {1, 5, 7};
        CHECK(plane_through3(a, p1, p2, q0, nh));
        CHECK(q0[0] == 1 && q0[1] == 2 && q0[2] == 3);
        CHECK(nh[0] == 0 && nh[1] == -0.8 && nh[2] == 0.6);
        CHECK(plane_through3(a, p2, p1, q0, nh) && nh[0] == 0 && nh[1] == 0.8 && nh[2] == -0.6);
    }

    // the eigen-solve on diagonal matrices: no rotation is made, the answer is the unit vector on the smallest entry
    {
        const double M3[9] = {3, 0, 0, 0, 1, 0, 0, 0, 2};
        double v3[3];
        smallest_eigvec<3>(M3, v3);
        CHECK(v3[0] == 0 && v3[1] == 1 && v3[2] == 0);
        const double M4[16] = {4, 0, 0, 0, 0, 3, 0, 0, 0, 0, 0.5, 0, 0, 0, 0, 2};
        double v4[4];
        smallest_eigvec<4>(M4, v4);
        CHECK(v4[0] == 0 && v4[1] == 0 && v4[2] == 1 && v4[3] == 0);
    }
    printf("%d %d failures\n", checked, fails);
    return fails != 0;
}
