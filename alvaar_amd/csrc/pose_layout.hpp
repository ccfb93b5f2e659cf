// The pose solve's host side said once (P3P-LMedS -> PnP refinement: p3p.hip, pnp.hip, track_batch.hip): its size limits, the draw schedule
// of the sample stream, P3P's angular threshold, and the memory blocks the launch routes share -- each block described ONCE, by the
// constructor that carves it: the field pointers and the block's size both come from that one walk (as track_step.hpp does for the
// tracking step).  Plain C++ -- a host-only test restates the arithmetic these replaced for every n and H (tests/cpp/pose_layout.cpp).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

// P3P-LMedS keeps its median in LDS: at most this many correspondences per problem (alva_p3p_prepare refuses more; a caller with a larger
// frame solves on the first ones, in its own order)
constexpr int ALVA_P3P_MAX_N = 19000;
// LDS-resident median select: n * 8 B of keys beside ~8 KB of static LDS.  Up to 7168 keys fit the default 64 KB per workgroup; gfx950
// has 160 KB per CU and a workgroup may take it all once the kernel's limit is raised (a 4K frame has ~10 k 3-D keypoints).  Up to here a
// problem may take the fused, the lane and the batch launches; beyond, k_p3p / k_p3p_s alone, with the raised limit.
constexpr int ALVA_P3P_LDS_DEFAULT_N = 7168;
// a single problem's samples travel IN the kernel arguments when it has at most this many hypotheses (p3p_device.hpp P3pInlineSamples)
constexpr int P3P_INLINE_H = 192;

// ---- the draw schedule -----------------------------------------------------------------------------------------------------------------
// max_iters + slack samples are drawn up front; hypotheses whose model fails do not count as an iteration in the reference
// (Lmeds.hpp:88-92), so on the rare shortfall a longer prefix of the same stream is drawn, up to max_skip = 10 x max_iterations more
// (Lmeds.hpp:67).
constexpr int p3p_max_draws(int iters) { return iters + iters * 10; }
constexpr int p3p_first_draws(int iters) { return p3p_max_draws(iters) < iters + 28 ? p3p_max_draws(iters) : iters + 28; }
constexpr int p3p_next_draws(int H, int max_draws) { return max_draws < H * 2 ? max_draws : H * 2; }

// the reprojection threshold in pixels as the angle score P3P compares: 1 - cos(atan(err / focal)), the focal length averaged IN FLOAT
// (multi_view_geometry.cpp:72-76)
inline double p3p_threshold(float err_px, float fx, float fy) {
    float focal = fx + fy;
    focal /= 2.f;
    return 1.0 - std::cos(std::atan((double) (err_px / focal)));
}

// ---- the blocks ------------------------------------------------------------------------------------------------------------------------
struct P3pSelectOut;   // pose_internal.hpp
// the 256-byte slot a result record gets wherever a block holds one (P3pSelectOut, pnp.hip's PnpOut: their files assert that they fit)
constexpr size_t POSE_REC_BYTES = 256;

// Walks a block: typed pointers at running OFFSETS from the base.  A base is aligned as the widest step its block takes -- 256 bytes the
// pinned blocks (hipHostMalloc gives that), 64 the scratch blocks (hipMalloc, or a 64-byte granular slab of the batch); the functions
// that obtain a block check it with pose_block_aligned -- so an offset's alignment is the pointer's.
struct PoseCarve {
    uintptr_t base;
    size_t off = 0;
    template <class T> T *take(size_t bytes) {
        T *p = reinterpret_cast<T *>(base + off);
        off += bytes;
        return p;
    }
    void up(size_t a) { off = (off + a - 1) / a * a; }   // on to the next multiple of a, none when off is one already
};
inline bool pose_block_aligned(const void *base, size_t a) { return ((uintptr_t) base & (a - 1)) == 0; }

// P3P's DEVICE scratch: models [H][12] | valid [H] | penalty [H] | masks [H][ceil(n_masks / 64)].  Only the single launch writes masks
// (P3pArgs::masks); a batch item's block ends in front of them (n_masks = 0: masks is null).  penalty and masks start a 64-byte line.
struct P3pScratch {
    double *models;
    int *valid;
    double *penalty;
    unsigned long long *masks;
    size_t end;
    static constexpr size_t mask_words(size_t n) { return (n + 63) / 64; }
    P3pScratch(const void *base, size_t H, size_t n_masks) {
        PoseCarve k{(uintptr_t) base};
        models = k.take<double>(H * 12 * sizeof(double));
        valid = k.take<int>(H * sizeof(int));
        k.up(64);
        penalty = k.take<double>(H * sizeof(double));
        k.up(64);
        masks = n_masks ? k.take<unsigned long long>(H * mask_words(n_masks) * 8) : nullptr;
        end = k.off;
    }
    static size_t bytes(size_t H, size_t n_masks) { return P3pScratch(nullptr, H, n_masks).end; }
};

// The refinement's DEVICE scratch: chi2 [n] | active [n] | depth [n], and behind them
//   SESSION  the P3P stage's hand-off: selection record (on a 64-byte line) | inlier mask [n] -- bad / p3p_outlier are pinned (PosePin)
//   BATCH    bad [n] | p3p_outlier [n], the block a multiple of 64 bytes -- the hand-off lives in the batch's own slab
//   BARE     nothing (alva_pnp_refine: no P3P stage)
struct PnpScratch {
    enum Form { BARE, SESSION, BATCH };
    double *chi2 = nullptr;
    uint8_t *active = nullptr, *depth = nullptr;
    P3pSelectOut *sel = nullptr;
    uint8_t *inlier = nullptr, *bad = nullptr, *p3p_outlier = nullptr;
    size_t end = 0;
    PnpScratch() = default;
    PnpScratch(const void *base, size_t n, Form form) {
        PoseCarve k{(uintptr_t) base};
        chi2 = k.take<double>(n * 8);
        active = k.take<uint8_t>(n);
        depth = k.take<uint8_t>(n);
        if (form == SESSION) {
            k.up(64);
            sel = k.take<P3pSelectOut>(POSE_REC_BYTES);
            inlier = k.take<uint8_t>(n);
        } else if (form == BATCH) {
            bad = k.take<uint8_t>(n);
            p3p_outlier = k.take<uint8_t>(n);
            k.up(64);
        }
        end = k.off;
    }
    static size_t bytes(size_t n, Form form) { return PnpScratch(nullptr, n, form).end; }
};

// The session's PINNED block, read / written by the kernels directly, no copy commands: head | PnpOut (on a 256-byte line) | bad [n] |
// p3p_outlier [n].  The head is the H x 4 samples of the separate launches (pose_samples_bytes) or the fused launch's PoseGo, which holds
// them (POSE_GO_BYTES); the two routes alternate on one block.
constexpr size_t pose_samples_bytes(size_t H) { return H * 16; }
constexpr size_t POSE_GO_BYTES = 16 + pose_samples_bytes(P3P_INLINE_H) + 8;   // sizeof(PoseGo), pnp.hip
struct PosePin {
    uint8_t *head = nullptr;
    void *out = nullptr;   // PnpOut
    uint8_t *bad = nullptr, *p3p_outlier = nullptr;
    size_t end = 0;
    PosePin() = default;
    PosePin(const void *base, size_t head_bytes, size_t n) {
        PoseCarve k{(uintptr_t) base};
        head = k.take<uint8_t>(head_bytes);
        k.up(256);
        out = k.take<void>(POSE_REC_BYTES);
        bad = k.take<uint8_t>(n);
        p3p_outlier = k.take<uint8_t>(n);
        end = k.off;
    }
    static size_t bytes(size_t head_bytes, size_t n) { return PosePin(nullptr, head_bytes, n).end; }
};

// P3P alone, PINNED (alva_p3p_lmeds): samples [H][4] | selection record (on a 256-byte line) | inlier mask [n], and for the hypothesis
// probe (alva_p3p_hypotheses route 0, n_masks = n) behind them, on 64-byte lines: the arrival counter's host copy | the scratch block's.
struct P3pPin {
    int *samples;
    P3pSelectOut *sel;
    uint8_t *inlier;
    int *counter = nullptr;
    uint8_t *scratch = nullptr;
    size_t end;
    P3pPin(const void *base, size_t H, size_t n, size_t n_masks) {
        PoseCarve k{(uintptr_t) base};
        samples = k.take<int>(pose_samples_bytes(H));
        k.up(256);
        sel = k.take<P3pSelectOut>(POSE_REC_BYTES);
        inlier = k.take<uint8_t>(n);
        if (n_masks) {
            k.up(64);
            counter = k.take<int>(64);
            scratch = k.take<uint8_t>(P3pScratch::bytes(H, n_masks));
        }
        end = k.off;
    }
    static size_t bytes(size_t H, size_t n, size_t n_masks) { return P3pPin(nullptr, H, n, n_masks).end; }
};

// what the kernels count on, beyond an aligned base: a record slot keeps the line of whatever precedes it, a model row and a mask
// word keep doubles 8-byte aligned
static_assert(POSE_REC_BYTES % 256 == 0 && 12 * sizeof(double) % 8 == 0 && sizeof(unsigned long long) == 8, "pose blocks: alignment");
static_assert(ALVA_P3P_LDS_DEFAULT_N <= ALVA_P3P_MAX_N && p3p_first_draws(100) <= P3P_INLINE_H, "the session's frame takes the fused launch");
