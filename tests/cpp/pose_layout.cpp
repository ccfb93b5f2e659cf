// The blocks, the draw schedule and the threshold of the pose solve (alvaar_amd/csrc/pose_layout.hpp) against a literal restatement of the
// arithmetic they replaced in p3p.hip and pnp.hip: for every n in [0, ALVA_P3P_MAX_N] the PnP scratch in its three forms, both heads of
// the pinned pose block, and with sampled H the n-dependent P3P blocks; for every H in [1, 2200] the P3P scratch without masks and the
// H-dependent pinned blocks at sampled n.  Same offsets, same sizes; fields disjoint and inside the block; PnpOut and the selection record
// of a pinned block on a 256-byte line, the scratch's selection record on a 64-byte line, masks and doubles 8-byte aligned.
#include "../../alvaar_amd/csrc/pose_layout.hpp"
#include <cstdio>
#include <cstring>
#include <vector>

static long checked = 0;
static int fails = 0;
#define CHECK(c, ...)                                      \
    do {                                                   \
        checked++;                                         \
        if (!(c) && fails++ < 20) {                        \
            printf("n=%zu H=%zu: %s: ", n, H, #c);         \
            printf(__VA_ARGS__);                           \
            printf("\n");                                  \
        }                                                  \
    } while (0)

struct Field {
    const char *name;
    size_t got, want, bytes, align;   // offsets from the base
};

static const size_t BASE = (size_t) 0x7f0012345600;   // 256-byte aligned, as the allocations are
static size_t off(const void *p) { return (size_t) ((uintptr_t) p - BASE); }
static const void *base() { return reinterpret_cast<const void *>(BASE); }

static void check_block(const char *block, size_t n, size_t H, const std::vector<Field> &f, size_t got_bytes, size_t want_bytes) {
    CHECK(got_bytes == want_bytes, "%s: %zu bytes, restated %zu", block, got_bytes, want_bytes);
    for (size_t i = 0; i < f.size(); i++) {
        CHECK(f[i].got == f[i].want, "%s.%s at %zu, restated %zu", block, f[i].name, f[i].got, f[i].want);
        CHECK(f[i].got + f[i].bytes <= got_bytes, "%s.%s ends at %zu of %zu", block, f[i].name, f[i].got + f[i].bytes, got_bytes);
        CHECK((BASE + f[i].got) % f[i].align == 0, "%s.%s at %zu, not a multiple of %zu", block, f[i].name, f[i].got, f[i].align);
        for (size_t j = 0; j < i; j++)
            CHECK(f[i].got >= f[j].got + f[j].bytes || f[j].got >= f[i].got + f[i].bytes, "%s.%s overlaps %s", block, f[i].name, f[j].name);
    }
}

// alva_p3p_prepare (masks) / alva_p3p_batch_scratch_bytes, alva_p3p_batch_item_fill, hyp_unpack (no masks)
static void p3p_scratch(size_t n, size_t H, bool masks) {
    size_t off_valid = (size_t) H * 12 * sizeof(double);
    size_t off_pen = (off_valid + (size_t) H * sizeof(int) + 63) / 64 * 64;
    const size_t off_masks = (off_pen + (size_t) H * sizeof(double) + 63) / 64 * 64;
    size_t total = off_masks + (size_t) H * (((size_t) n + 63) / 64) * 8;
    const size_t batch_total = (off_pen + (size_t) H * sizeof(double) + 63) / 64 * 64;
    const P3pScratch S(base(), H, masks ? n : 0);
    std::vector<Field> f = {{"models", off(S.models), 0, H * 96, 8}, {"valid", off(S.valid), off_valid, H * 4, 4}, {"penalty", off(S.penalty), off_pen, H * 8, 64}};
    if (masks) f.push_back({"masks", off(S.masks), off_masks, H * ((n + 63) / 64) * 8, 64});
    else CHECK(S.masks == nullptr, "masks without points");
    check_block(masks ? "p3p scratch" : "p3p batch scratch", n, H, f, P3pScratch::bytes(H, masks ? n : 0), masks ? total : batch_total);
    CHECK(P3pScratch::mask_words(n) == ((size_t) n + 63) / 64, "%zu words", P3pScratch::mask_words(n));
}

// alva_pnp_refine | pose_launch, alva_pose_all_enqueue | alva_pnp_batch_scratch_bytes, alva_pnp_batch_item_fill
static void pnp_scratch(size_t n) {
    const size_t H = 0;
    {
        const size_t off_act = (size_t) n * 8, off_dep = off_act + (size_t) n;
        const PnpScratch S(base(), n, PnpScratch::BARE);
        check_block("pnp scratch, bare", n, H, {{"chi2", off(S.chi2), 0, n * 8, 8}, {"active", off(S.active), off_act, n, 1}, {"depth", off(S.depth), off_dep, n, 1}},
                    PnpScratch::bytes(n, PnpScratch::BARE), off_dep + (size_t) n);
        CHECK(!S.sel && !S.inlier && !S.bad && !S.p3p_outlier, "a tail");
    }
    {
        const size_t off_act = (size_t) n * 8, off_dep = off_act + (size_t) n, off_sel = (off_dep + (size_t) n + 63) / 64 * 64;
        const size_t off_inl = off_sel + 256;
        const PnpScratch S(base(), n, PnpScratch::SESSION);
        check_block("pnp scratch, session", n, H,
                    {{"chi2", off(S.chi2), 0, n * 8, 8}, {"active", off(S.active), off_act, n, 1}, {"depth", off(S.depth), off_dep, n, 1},
                     {"sel", off(S.sel), off_sel, 256, 64}, {"inlier", off(S.inlier), off_inl, n, 1}},
                    PnpScratch::bytes(n, PnpScratch::SESSION), off_inl + (size_t) n);
        CHECK(!S.bad && !S.p3p_outlier, "the batch's tail");
    }
    {
        const size_t total = ((size_t) n * 12 + 63) / 64 * 64;
        const size_t o_active = (size_t) n * 8, o_depth = o_active + n, o_bad = o_depth + n, o_po = o_bad + n;   // it.active = d_scratch + n * 8; it.depth = it.active + n; ...
        const PnpScratch S(base(), n, PnpScratch::BATCH);
        check_block("pnp scratch, batch", n, H,
                    {{"chi2", off(S.chi2), 0, n * 8, 8}, {"active", off(S.active), o_active, n, 1}, {"depth", off(S.depth), o_depth, n, 1},
                     {"bad", off(S.bad), o_bad, n, 1}, {"p3p_outlier", off(S.p3p_outlier), o_po, n, 1}},
                    PnpScratch::bytes(n, PnpScratch::BATCH), total);
        CHECK(!S.sel && !S.inlier, "the session's tail");
        CHECK(total % 64 == 0, "%zu", total);
    }
}

// pose_launch (head = H * 16 bytes of samples) | alva_pose_all_enqueue (head = sizeof(PoseGo), go = true)
static void pose_pin(size_t n, size_t H, bool go) {
    // struct PoseGo { long long word; int n, H; int samples[4 * P3P_INLINE_H]; long long nack; }
    const size_t sizeof_PoseGo = 8 + 4 + 4 + 4 * 4 * 192 + 8;
    const size_t poff_out = go ? (sizeof_PoseGo + 255) / 256 * 256 : ((size_t) H * 16 + 255) / 256 * 256;
    const size_t poff_bad = poff_out + 256;
    const size_t poff_po = poff_bad + (size_t) n;
    const size_t head = go ? POSE_GO_BYTES : pose_samples_bytes(H);
    CHECK(head == (go ? sizeof_PoseGo : H * 16), "head of %zu bytes", head);
    const PosePin P(base(), head, n);
    check_block(go ? "pose pin, PoseGo" : "pose pin, samples", n, H,
                {{"head", off(P.head), 0, head, 8}, {"out", off(P.out), poff_out, 256, 256}, {"bad", off(P.bad), poff_bad, n, 1},
                 {"p3p_outlier", off(P.p3p_outlier), poff_po, n, 1}},
                PosePin::bytes(head, n), poff_po + (size_t) n);
}

// alva_p3p_lmeds | hyp_single (probe = true)
static void p3p_pin(size_t n, size_t H, bool probe) {
    const size_t words = ((size_t) n + 63) / 64;
    const size_t off_out = ((size_t) H * 16 + 255) / 256 * 256, off_inl = off_out + 256;
    const size_t off_cnt = (off_inl + (size_t) n + 63) / 64 * 64, off_scr = off_cnt + 64;
    const size_t off_valid = (size_t) H * 12 * sizeof(double);
    const size_t off_pen = (off_valid + (size_t) H * sizeof(int) + 63) / 64 * 64;
    const size_t off_masks = (off_pen + (size_t) H * sizeof(double) + 63) / 64 * 64;
    const size_t scr_bytes = off_masks + (size_t) H * words * 8;
    const P3pPin B(base(), H, n, probe ? n : 0);
    std::vector<Field> f = {{"samples", off(B.samples), 0, H * 16, 4}, {"sel", off(B.sel), off_out, 256, 256}, {"inlier", off(B.inlier), off_inl, n, 1}};
    if (probe) {
        f.push_back({"counter", off(B.counter), off_cnt, 64, 64});
        f.push_back({"scratch", off(B.scratch), off_scr, scr_bytes, 64});
        // the masks of the scratch block's host copy, as hyp_single reads them
        CHECK(off(P3pScratch(B.scratch, H, n).masks) == off_scr + off_masks, "masks of the copy at %zu", off(P3pScratch(B.scratch, H, n).masks));
    } else {
        CHECK(!B.counter && !B.scratch, "the probe's tail");
    }
    check_block(probe ? "p3p pin, probe" : "p3p pin", n, H, f, P3pPin::bytes(H, n, probe ? n : 0), probe ? off_scr + scr_bytes : off_inl + (size_t) n);
}

static bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof(a)) == 0; }

int main() {
    const size_t MAX_N = ALVA_P3P_MAX_N, MAX_H = 2200;   // 2200 = max draws of 200 iterations
    const size_t some_H[] = {1, 4, 15, 16, 17, 63, 128, 130, 164, 165, 192, 193, 228, 257, 1100, 2200};
    const size_t some_n[] = {0, 1, 4, 5, 63, 64, 65, 255, 256, 257, 2047, 6145, 7168, 7169, 10432, MAX_N};
    for (size_t n = 0; n <= MAX_N; n++) {
        pnp_scratch(n);
        pose_pin(n, 0, true);
        for (size_t H: some_H) {
            pose_pin(n, H, false);
            p3p_pin(n, H, false);
            if (n >= 4) {   // (alva_p3p_prepare refuses fewer; without points there are no masks to tell the forms apart)
                p3p_scratch(n, H, true);
                p3p_pin(n, H, true);
            }
        }
    }
    for (size_t H = 1; H <= MAX_H; H++) {
        p3p_scratch(0, H, false);
        for (size_t n: some_n) {
            pose_pin(n, H, false);
            p3p_pin(n, H, false);
            if (n >= 4) {
                p3p_scratch(n, H, true);
                p3p_pin(n, H, true);
            }
        }
    }
    {
        const size_t n = 0, H = 0;
        CHECK(ALVA_P3P_LDS_DEFAULT_N == 7168 && ALVA_P3P_MAX_N == 19000 && P3P_INLINE_H == 192 && POSE_REC_BYTES == 256, "the limits");
        CHECK(pose_block_aligned(base(), 256) && pose_block_aligned(base(), 64) && !pose_block_aligned((const char *) base() + 64, 256) &&
                  pose_block_aligned((const char *) base() + 64, 64) && !pose_block_aligned((const char *) base() + 8, 64),
              "pose_block_aligned");
        // the draw schedule: p3p.hip alva_p3p_lmeds, pnp.hip pose_params / alva_compute_pose_collect_p3p, track_batch.hip
        for (int iters = 1; iters <= 1000; iters++) {
            const int max_draws = iters + iters * 10;
            int h = max_draws < iters + 28 ? max_draws : iters + 28;   // std::min(max_draws, max_iters + 28)
            CHECK(p3p_max_draws(iters) == max_draws && p3p_max_draws(iters) == iters * 11, "iters %d: %d max draws", iters, p3p_max_draws(iters));
            CHECK(p3p_first_draws(iters) == h, "iters %d: first %d", iters, p3p_first_draws(iters));
            CHECK((p3p_first_draws(iters) <= P3P_INLINE_H) == (iters + 28 <= 192), "iters %d: the fused launch's gate", iters);
            for (int step = 0; step < 8; step++) {
                const int next = max_draws < h * 2 ? max_draws : h * 2;   // std::min(max_draws, H * 2)
                CHECK(p3p_next_draws(h, max_draws) == next, "iters %d: after %d comes %d", iters, h, p3p_next_draws(h, max_draws));
                h = next;
            }
            CHECK(h == max_draws, "iters %d: the prefixes end at %d of %d", iters, h, max_draws);
        }
        CHECK(p3p_first_draws(100) == 128 && p3p_max_draws(100) == 1100 && p3p_max_draws(200) == (int) MAX_H, "the session's and the tests' schedules");
        // the threshold, bit for bit: p3p.hip alva_p3p_prepare / alva_p3p_batch_item_fill
        const float cams[][3] = {{3.0f, 525.0f, 525.0f},    {3.0f, 517.3f, 516.5f},   {3.0f, 458.654f, 457.296f}, {1.5f, 1400.25f, 1399.5f},
                                 {0.1f, 100.0f, 3000.0f},   {8.0f, 0.5f, 0.25f},      {3.0f, 1e-3f, 1e4f},        {2.9999f, 700.1f, 699.9f}};
        for (const auto &c: cams) {
            const float err_threshold = c[0], fx = c[1], fy = c[2];
            float focal = fx + fy;
            focal /= 2.f;
            const double threshold = 1.0 - std::cos(std::atan((double) (err_threshold / focal)));
            CHECK(same_bits(p3p_threshold(err_threshold, fx, fy), threshold), "err %g fx %g fy %g: %.17g, restated %.17g", err_threshold, fx, fy,
                  p3p_threshold(err_threshold, fx, fy), threshold);
        }
    }
    printf("%ld checks %d failures\n", checked, fails);
    return fails != 0;
}
