// The three blocks of the fused tracking step (alvaar_amd/csrc/track_step.hpp) against a literal restatement of the arithmetic they
// replaced -- the size sums of track_reserve and the three pointer walks of track_begin, track_pin() and track_in() -- for every capacity
// track_reserve can produce and for a null and a 256-aligned base: same offsets, same sizes; fields disjoint and inside the block; room for
// the carry index; the completion words inside the header; 16-byte alignment from d_is3d on; the two tables track_in_bytes apart.
//   track_layout <TRK_HDR_EARLY> <TRK_HDR_DONE>      (int offsets into o_hdr, track_slots.hpp)
#include "../../alvaar_amd/csrc/track_step.hpp"
#include <cstdio>
#include <cstdlib>
#include <vector>

static long checked = 0;
static int fails = 0;
#define CHECK(c, ...)                                            \
    do {                                                         \
        checked++;                                               \
        if (!(c) && fails++ < 20) {                              \
            printf("cap=%zu base=%#zx: %s: ", cap, base, #c);    \
            printf(__VA_ARGS__);                                 \
            printf("\n");                                        \
        }                                                        \
    } while (0)

struct Field {
    const char *name;
    size_t got, want, bytes;   // offsets from the base
};

static void check_block(const char *block, size_t cap, size_t base, const std::vector<Field> &f, size_t got_bytes, size_t want_bytes) {
    CHECK(got_bytes == want_bytes, "%s: %zu bytes, restated %zu", block, got_bytes, want_bytes);
    for (size_t i = 0; i < f.size(); i++) {
        CHECK(f[i].got == f[i].want, "%s.%s at %zu, restated %zu", block, f[i].name, f[i].got, f[i].want);
        CHECK(f[i].got + f[i].bytes <= got_bytes, "%s.%s ends at %zu of %zu", block, f[i].name, f[i].got + f[i].bytes, got_bytes);
        for (size_t j = 0; j < i; j++)
            CHECK(f[i].got >= f[j].got + f[j].bytes || f[j].got >= f[i].got + f[i].bytes, "%s.%s overlaps %s", block, f[i].name, f[j].name);
    }
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    const int hdr_word[2] = {atoi(argv[1]), atoi(argv[2])};
    const size_t bases[2] = {0, (size_t) 0x7f0012345600};
    for (int n = 1; n <= 65535; n++) {
        const size_t cap = (size_t) (((n + 1023) / 1024 + 1) * 1024), c = cap;
        for (size_t base: bases) {
            const void *B = reinterpret_cast<const void *>(base);
            auto off = [&](const void *p) { return (size_t) ((uintptr_t) p - (uintptr_t) base); };
            uintptr_t b;
            {   // the device block: track_reserve's dev_bytes, track_begin's walk (sizeof(TrackCounters) = 1024)
                const size_t dev_bytes = 1024 + c * 2 + 256 + c * (8 + 1 + 8 + 8 + 24 + 24 + 24 + 16 + 24) + 256 + c * 8;
                b = base;
                const uintptr_t cnt = b; b += 1024;
                const uintptr_t code = b; b += c;
                const uintptr_t is3d = b; b += c;
                b += 256 - (b & 255);
                const uintptr_t pts = b; b += c * 8;
                const uintptr_t retried = b; b += c;
                const uintptr_t px = b; b += c * 8;
                const uintptr_t unpx = b; b += c * 8;
                const uintptr_t bv = b; b += c * 24;
                const uintptr_t wpt = b; b += c * 24;
                const uintptr_t Pbv = b; b += c * 24;
                const uintptr_t Puv = b; b += c * 16;
                const uintptr_t Pwpt = b; b += c * 24;
                b += 256 - (b & 255);
                const uintptr_t px_alt = b; b += c * 8;
                const TrackDevBlock D(B, cap);
                const std::vector<Field> f = {
                    {"cnt", off(D.cnt), cnt - base, 1024},        {"code", off(D.code), code - base, c},
                    {"is3d", off(D.is3d), is3d - base, c},        {"pts", off(D.pts), pts - base, c * 8},
                    {"retried", off(D.retried), retried - base, c}, {"px[0]", off(D.px[0]), px - base, c * 8},
                    {"unpx", off(D.unpx), unpx - base, c * 8},    {"bv", off(D.bv), bv - base, c * 24},
                    {"wpt", off(D.wpt), wpt - base, c * 24},      {"Pbv", off(D.Pbv), Pbv - base, c * 24},
                    {"Puv", off(D.Puv), Puv - base, c * 16},      {"Pwpt", off(D.Pwpt), Pwpt - base, c * 24},
                    {"px[1]", off(D.px[1]), px_alt - base, c * 8}};
                check_block("dev", cap, base, f, TrackDevBlock::bytes(cap), dev_bytes);
                CHECK(TRK_COUNTERS_BYTES == 1024, "%zu", TRK_COUNTERS_BYTES);
                for (size_t i = 2; i < f.size(); i++)   // k_track_stage_in copies in 16-byte units
                    CHECK((base + f[i].got) % 16 == 0, "dev.%s at %zu", f[i].name, f[i].got);
            }
            {   // the pinned block: track_reserve's pin_bytes, track_pin()
                const size_t pin_bytes = c * 8 + c + 64 + c * 24 + 256 + c + 64 + c * 16 + c * 24 + 256;
                b = base;
                const uintptr_t in_px = b; b += c * 8;
                const uintptr_t in_is3d = b; b += c + 64 - (c & 63);
                const uintptr_t in_wpt = b; b += c * 24;
                const uintptr_t o_hdr = b; b += 256;
                const uintptr_t o_code = b; b += c + 64 - (c & 63);
                const uintptr_t o_px = b; b += c * 8;
                const uintptr_t o_unpx = b; b += c * 8;
                const uintptr_t o_bv = b; b += c * 24;
                const TrackPinBlock P(B, cap);
                const std::vector<Field> f = {
                    {"in.px", off(P.in.px), in_px - base, c * 8},    {"in.is3d", off(P.in.is3d), in_is3d - base, c},
                    {"in.wpt", off(P.in.wpt), in_wpt - base, c * 24}, {"o_hdr", off(P.o_hdr), o_hdr - base, 256},
                    {"o_code", off(P.o_code), o_code - base, c},     {"o_px", off(P.o_px), o_px - base, c * 8},
                    {"o_unpx", off(P.o_unpx), o_unpx - base, c * 8}, {"o_bv", off(P.o_bv), o_bv - base, c * 24}};
                check_block("pin", cap, base, f, TrackPinBlock::bytes(cap), pin_bytes);
                CHECK(TRK_HDR_BYTES == 256, "%zu", TRK_HDR_BYTES);
                for (int w: hdr_word) {
                    CHECK(w >= 0 && (size_t) (w + 2) * 4 <= TRK_HDR_BYTES, "word at int %d", w);
                    CHECK((base + off(P.o_hdr) + 4 * (size_t) w) % 8 == 0, "word at int %d", w);
                }
                CHECK(hdr_word[0] != hdr_word[1], "%d", hdr_word[0]);
                for (size_t i = 0; i < 3; i++) CHECK((base + f[i].got) % 16 == 0, "pin.%s at %zu", f[i].name, f[i].got);   // the copy kernel's source
            }
            {   // the host-written block: track_reserve's in_bytes, track_in_bytes / track_in(par) / track_carry()
                const size_t tib = c * 8 + c + 256 + c * 24;
                const size_t in_bytes = 2 * tib + c * 2 + 256;
                uintptr_t px[2], is3d[2], wpt[2];
                for (int par = 0; par < 2; par++) {
                    b = base + (size_t) (par & 1) * tib;
                    px[par] = b; b += c * 8;
                    is3d[par] = b; b += c + 256 - (c & 255);
                    wpt[par] = b;
                }
                const uintptr_t carry = base + 2 * tib;
                const TrackInBlock I(B, cap);
                const std::vector<Field> f = {
                    {"table[0].px", off(I.table[0].px), px[0] - base, c * 8},    {"table[0].is3d", off(I.table[0].is3d), is3d[0] - base, c},
                    {"table[0].wpt", off(I.table[0].wpt), wpt[0] - base, c * 24}, {"table[1].px", off(I.table[1].px), px[1] - base, c * 8},
                    {"table[1].is3d", off(I.table[1].is3d), is3d[1] - base, c},  {"table[1].wpt", off(I.table[1].wpt), wpt[1] - base, c * 24},
                    {"carry", off(I.carry), carry - base, c * 2}};
                check_block("in", cap, base, f, TrackInBlock::bytes(cap), in_bytes);
                CHECK(track_in_bytes(cap) == tib, "%zu, restated %zu", track_in_bytes(cap), tib);
                CHECK(off(I.table[1].px) - off(I.table[0].px) == track_in_bytes(cap) && off(I.table[1].is3d) - off(I.table[0].is3d) == track_in_bytes(cap) &&
                          off(I.table[1].wpt) - off(I.table[0].wpt) == track_in_bytes(cap),
                      "the tables are %zu apart", off(I.table[1].px) - off(I.table[0].px));
                CHECK(off(I.carry) + cap * 2 <= TrackInBlock::bytes(cap), "carry at %zu of %zu", off(I.carry), TrackInBlock::bytes(cap));
                for (size_t i = 0; i < 6; i++) CHECK((base + f[i].got) % 16 == 0, "in.%s at %zu", f[i].name, f[i].got);   // the tracker's table
            }
            CHECK(track_block_aligned(B), "the test's own base");
        }
    }
    printf("%ld checks %d failures\n", checked, fails);
    return fails != 0;
}
