// a8: P3P (Kneip) + least-median-of-squares absolute pose, hypothesis-parallel, FP64.
//
// Replaces MultiViewGeometry::p3pRansac (src/slam/src/multi_view_geometry.cpp:24-127) =
// opengv::sac::Lmeds<AbsolutePoseSacProblem(KNEIP)>::computeModel
// (src/libs/opengv/include/opengv/sac/implementation/Lmeds.hpp:43-195), with
//   sampling   SampleConsensusProblem.hpp:40-120 (std::mt19937 + prefix Fisher-Yates; done on the HOST with
//              the same libstdc++ classes, so the index stream is the reference's by construction)
//   model      AbsolutePoseSacProblem.cpp:35-163 (Kneip P3P on samples 0..2, disambiguate on the 4th)
//   p3p        src/absolute_pose/modules/main.cpp:50-205, quartic src/math/roots.cpp:88-135
//   score      AbsolutePoseSacProblem.cpp:165-199  (1 - f . normalize(R^T (X - t)))
//
// The reference evaluates hypotheses one after another; they are independent, so here
//   k_p3p      ONE launch, one workgroup per drawn sample: hypothesis (4 lanes = 4 quartic roots) -> N squared scores
//              into LDS, radix-select of the median -> the last workgroup to finish replays the sequential
//              "first max_iters valid, strict <" selection and classifies the winner's inliers
// FP64 VALU work (100 x N x ~40 flop); bytes are negligible (48 N read once per hypothesis,
// L2-resident).  No MFMA: nothing here is GEMM-shaped.
#include "common.hpp"
#include "multi_kernel.hpp"
#include <atomic>
#include "pose_internal.hpp"
#include <cmath>
#include <ctime>
#include <random>

#include "p3p_device.hpp"

namespace {

// The single-problem kernel runs P3P_NT threads per workgroup: ~130 workgroups never fill the chip (one per CU), so the scoring pass, the
// select and the winner's inlier pass -- all strided by the workgroup size -- shorten with it (stamps, 2300 points, 256 -> 512 threads:
// score 3.6 us, select 5.3 us, inliers 5.1 us per workgroup before).
constexpr int P3P_NT = 512;
__global__ void __launch_bounds__(P3P_NT) k_p3p(P3pArgs A) { (void) p3p_block<0, P3P_NT>(A, blockIdx.x); }
// several sessions' problems in one launch (lane.hpp): the samples come through A.samples (pinned host memory), as in k_p3p
ALVA_MULTI_KERNEL(MK_P3P, k_p3p_multi, P3pArgs, dim3(P3P_NT), P3P_NT, (void) p3p_block<0, P3P_NT>(A, bx));
__global__ void __launch_bounds__(P3P_NT) k_p3p_s(P3pArgs A, P3pInlineSamples S) { (void) p3p_block<0, P3P_NT>(A, blockIdx.x, S.v + 4 * blockIdx.x); }

// B independent problems in one launch: blockIdx.y = problem (camera), each with its own correspondences, sample list, scratch
// and arrival counter.  Dynamic LDS is sized for the largest problem.
// In a batch the Kneip solves get their own launch, 16 hypotheses per wave: inside k_p3p they occupy one wave of the four while the
// other three wait, and their register need (120 VGPRs) would cap the scoring kernel at four workgroups per CU.
__global__ void __launch_bounds__(256) k_p3p_hyp_batch(const P3pArgs *__restrict__ args) {
    const P3pArgs A = args[blockIdx.y];
    const int h = (int) (blockIdx.x * 64 + (threadIdx.x >> 2));
    if (h >= A.H) return;  // whole groups of 4 lanes leave together (the xor shuffles stay inside a group)
    (void) p3p_hypothesis(A, h, threadIdx.x & 3, true, nullptr);
}

__global__ void __launch_bounds__(256) k_p3p_batch(const P3pArgs *__restrict__ args) {
    const P3pArgs A = args[blockIdx.y];
    if ((int) blockIdx.x >= A.H) return;
    (void) p3p_block<1, 256>(A, blockIdx.x);
}

__global__ void __launch_bounds__(256) k_p3p_select_batch(const P3pArgs *__restrict__ args) {
    const P3pArgs A = args[blockIdx.x];
    (void) p3p_block<2, 256>(A, 0);
}

// SampleConsensusProblem<M>: rng_dist_ = uniform_int_distribution<>(0, INT_MAX), rng_alg_ = std::mt19937
// seeded with the caller's fixed seed (SessionPose::seed; or time+clock), shuffled_indices_ persists across draws (SampleConsensusProblem.hpp:40-84).
struct Sampler {
    std::mt19937 alg;
    std::uniform_int_distribution<> dist{0, std::numeric_limits<int>::max()};
    std::vector<int> shuffled;
    Sampler(int n, bool random_seed, uint32_t seed) : shuffled((size_t) n) {
        if (random_seed) alg.seed(static_cast<unsigned>(time(0)) + static_cast<unsigned>(clock()));
        else alg.seed(seed);
        for (int i = 0; i < n; i++) shuffled[(size_t) i] = i;
    }
    void draw(int *out4) {
        const size_t index_size = shuffled.size();
        for (unsigned i = 0; i < 4; ++i) std::swap(shuffled[i], shuffled[i + ((size_t) dist(alg) % (index_size - i))]);
        for (int i = 0; i < 4; i++) out4[i] = shuffled[(size_t) i];
    }
};

}  // namespace

// the first `count` outputs of the sampler's generator -- dist(alg) of Sampler::draw, which does not depend on the number of points
int alva_p3p_raw_draws(int count, int do_random, uint32_t seed, int *h_raw) {
    ALVA_ARG(count >= 0 && h_raw);
    Sampler s(0, do_random != 0, seed);
    for (int k = 0; k < count; k++) h_raw[k] = s.dist(s.alg);
    return ALVA_OK;
}

extern "C" int alva_p3p_draw_samples(int n_points, int count, int do_random, uint32_t seed, int *h_samples) {
    ALVA_ARG(n_points >= 4 && count >= 0 && h_samples);
    Sampler s(n_points, do_random != 0, seed);
    for (int k = 0; k < count; k++) s.draw(h_samples + 4 * k);
    return ALVA_OK;
}

// the kernels' argument block of one problem over its carved scratch (P3pScratch with masks: the single launch; without: a batch item)
static P3pArgs p3p_args(const double *d_bearings, const double *d_wpts, const int *samples, int n, int max_iters, float err_threshold, float fx,
                        float fy, int H, const P3pScratch &S, int *counter, P3pSelectOut *out, uint8_t *inlier, unsigned long long *dbg) {
    P3pArgs A{};
    A.bv = d_bearings;
    A.wpt = d_wpts;
    A.samples = samples;
    A.n = n;
    A.H = H;
    A.max_iters = max_iters;
    A.threshold = p3p_threshold(err_threshold, fx, fy);
    A.models = S.models;
    A.valid = S.valid;
    A.penalty = S.penalty;
    A.masks = S.masks;
    A.counter = counter;
    A.out = out;
    A.inlier = inlier;
    A.dbg = dbg;
    return A;
}

int alva_p3p_prepare(alva_ctx *ctx, const double *d_bearings, const double *d_wpts, int n, int max_iters, float err_threshold, int do_random,
                     uint32_t seed, float fx, float fy, int H, int *pin_samples, P3pSelectOut *out, uint8_t *inlier, P3pArgs *args) {
    ALVA_ARG(n >= 4 && n <= ALVA_P3P_MAX_N && args);
    if (pin_samples) {   // (null: the caller draws later, when it knows n -- the fused pose launch sizes everything for an upper bound)
        Sampler smp(n, do_random != 0, seed);
        for (int k = 0; k < H; k++) smp.draw(pin_samples + 4 * k);
    }
    uint8_t *base = nullptr;
    int rc = alva_ctx_scratch(ctx, 2, P3pScratch::bytes((size_t) H, (size_t) n), (void **) &base);
    if (rc) return rc;
    ALVA_ARG(pose_block_aligned(base, 64));
    // (the arrival counter is zero between launches: the last workgroup resets it)
    *args = p3p_args(d_bearings, d_wpts, pin_samples, n, max_iters, err_threshold, fx, fy, H, P3pScratch(base, (size_t) H, (size_t) n),
                     ctx->d_counters + ALVA_CNT_P3P_SELECT, out, inlier, alva_kstamp_buffer());
    return ALVA_OK;
}

int alva_p3p_launch(alva_ctx *ctx, const P3pArgs &A) {
    const int n = A.n, H = A.H;
    if (n > ALVA_P3P_LDS_DEFAULT_N) {
        // the attribute is per DEVICE (one code object per device); sessions on several host threads reach this concurrently
        static std::atomic<bool> raised[64];
        const bool tracked = ctx->device >= 0 && ctx->device < 64;
        if (!tracked || !raised[ctx->device].load(std::memory_order_acquire)) {
            ALVA_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_p3p), hipFuncAttributeMaxDynamicSharedMemorySize, ALVA_P3P_MAX_N * 8));
            ALVA_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_p3p_s), hipFuncAttributeMaxDynamicSharedMemorySize, ALVA_P3P_MAX_N * 8));
            if (tracked) raised[ctx->device].store(true, std::memory_order_release);
        }
    }
    // (the multi kernel keeps the default dynamic-LDS limit)
    ctx->p3p_deferred = n <= ALVA_P3P_LDS_DEFAULT_N && alva_lane_defer(MK_P3P, ctx, (unsigned) H, (unsigned) ((size_t) n * sizeof(double)), &A, sizeof(A));
    if (ctx->p3p_deferred) return ALVA_OK;
    if (H <= P3P_INLINE_H) {
        P3pInlineSamples S;
        memcpy(S.v, A.samples, pose_samples_bytes((size_t) H));
        hipLaunchKernelGGL(k_p3p_s, dim3(H), dim3(P3P_NT), (size_t) n * sizeof(double), ctx->stream, A, S);
    } else {
        hipLaunchKernelGGL(k_p3p, dim3(H), dim3(P3P_NT), (size_t) n * sizeof(double), ctx->stream, A);
    }
    ALVA_LAUNCH_CHECK();
    return ALVA_OK;
}

int alva_p3p_enqueue(alva_ctx *ctx, const double *d_bearings, const double *d_wpts, int n, int max_iters, float err_threshold,
                     int do_random, uint32_t seed, float fx, float fy, int H, int *pin_samples, P3pSelectOut *out, uint8_t *inlier) {
    P3pArgs A{};
    const int rc = alva_p3p_prepare(ctx, d_bearings, d_wpts, n, max_iters, err_threshold, do_random, seed, fx, fy, H, pin_samples, out, inlier, &A);
    if (rc) return rc;
    return alva_p3p_launch(ctx, A);
}

extern "C" int alva_p3p_lmeds(alva_ctx *ctx, const double *d_bearings, const double *d_wpts, int n, int max_iters, float err_threshold,
                              int do_random, uint32_t seed, float fx, float fy, double *h_R, double *h_t, int *h_outliers,
                              int *h_n_outliers, int *h_ok) {
    ALVA_ARG(ctx && h_R && h_t && h_outliers && h_n_outliers && h_ok && max_iters > 0);
    *h_ok = 0;
    *h_n_outliers = 0;
    if (n < 4) return ALVA_OK;  // multi_view_geometry.cpp:41-44
    ALVA_ARG(d_bearings && d_wpts);
    // the draw schedule of pose_layout.hpp: a first prefix of the sample stream, on the rare shortfall a longer one
    const int max_draws = p3p_max_draws(max_iters);
    int H = p3p_first_draws(max_iters);
    SelectOut res{};
    const uint8_t *inl = nullptr;
    for (;;) {
        // pinned (P3pPin): the kernels read / write it directly, no copy commands
        uint8_t *pin = nullptr;
        int rc = alva_ctx_pinned(ctx, P3pPin::bytes((size_t) H, (size_t) n, 0), (void **) &pin);
        if (rc) return rc;
        ALVA_ARG(pose_block_aligned(pin, 256));
        const P3pPin B(pin, (size_t) H, (size_t) n, 0);
        rc = alva_p3p_enqueue(ctx, d_bearings, d_wpts, n, max_iters, err_threshold, do_random, seed, fx, fy, H, B.samples, B.sel, B.inlier);
        if (rc) return rc;
        ALVA_HIP(alva_stream_sync(ctx->stream));
        memcpy(&res, B.sel, sizeof(res));
        inl = B.inlier;
        if (res.n_valid_used >= max_iters || H >= max_draws) break;
        H = p3p_next_draws(H, max_draws);
    }
    if (!res.have_model) return ALVA_OK;
    if (res.n_inliers < 5) return ALVA_OK;  // multi_view_geometry.cpp:82-85
    // Sophus::isOrthogonal(R): ||R R^T - I||_F < 1e-10 (:88-91; sophus/rotation_matrix.hpp:17-27)
    const double *R = res.model;
    double e = 0;
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            double v = R[3 * r] * R[3 * c] + R[3 * r + 1] * R[3 * c + 1] + R[3 * r + 2] * R[3 * c + 2] - (r == c ? 1.0 : 0.0);
            e += v * v;
        }
    if (!(std::sqrt(e) < 1e-10)) return ALVA_OK;
    for (int k = 0; k < 9; k++) h_R[k] = R[k];
    for (int k = 0; k < 3; k++) h_t[k] = res.model[9 + k];
    int no = 0;
    for (int i = 0; i < n; i++)
        if (!inl[i]) h_outliers[no++] = i;  // :109-124: outliers = complement of the inlier list
    *h_n_outliers = no;
    *h_ok = 1;
    return ALVA_OK;
}

// ---- batch of problems (internal: track_batch.hip) --------------------------------------------------------------------------
size_t alva_p3p_batch_item_size() { return sizeof(P3pArgs); }

size_t alva_p3p_batch_scratch_bytes(int H) { return P3pScratch::bytes((size_t) H, 0); }

int alva_p3p_batch_item_fill(void *dst, const double *d_bearings, const double *d_wpts, int n, int max_iters, float err_threshold, float fx,
                             float fy, int H, const int *d_samples, uint8_t *d_scratch, int *d_counter, P3pSelectOut *d_out,
                             uint8_t *d_inlier) {
    ALVA_ARG(dst && d_bearings && d_wpts && n >= 4 && n <= ALVA_P3P_LDS_DEFAULT_N && H > 0 && d_samples && d_scratch && d_counter && d_out &&
             d_inlier && pose_block_aligned(d_scratch, 64));
    const P3pArgs A = p3p_args(d_bearings, d_wpts, d_samples, n, max_iters, err_threshold, fx, fy, H, P3pScratch(d_scratch, (size_t) H, 0), d_counter,
                               d_out, d_inlier, nullptr);
    memcpy(dst, &A, sizeof(A));
    return ALVA_OK;
}

int alva_p3p_batch_enqueue(alva_ctx *ctx, const void *d_items, int count, int H_max, int n_max) {
    ALVA_ARG(ctx && d_items && count > 0 && count <= 65535 && H_max > 0 && n_max >= 4 && n_max <= ALVA_P3P_LDS_DEFAULT_N);
    hipLaunchKernelGGL(k_p3p_hyp_batch, dim3(alva_divup(H_max, 64), count), dim3(256), 0, ctx->stream, (const P3pArgs *) d_items);
    hipLaunchKernelGGL(k_p3p_batch, dim3(H_max, count), dim3(256), (size_t) n_max * sizeof(double), ctx->stream, (const P3pArgs *) d_items);
    hipLaunchKernelGGL(k_p3p_select_batch, dim3(count), dim3(256), 0, ctx->stream, (const P3pArgs *) d_items);
    ALVA_LAUNCH_CHECK();
    return ALVA_OK;
}

// ---- the hypothesis stage made visible (tests) -------------------------------------------------------------------------------
// Caller-supplied samples through the production launches; everything the selection decides on is copied back per hypothesis.
namespace {

// models | valid | penalty of one problem, as alva_p3p_prepare / alva_p3p_batch_item_fill lay them out, to the caller's arrays.  A
// hypothesis without a model has penalty +inf on every route (the single launch publishes validity as penalty -1) and a zero model row.
void hyp_unpack(const uint8_t *h_scratch, bool valid_in_penalty, alva_p3p_hyp_problem &P) {
    const int H = P.H;
    const P3pScratch S(h_scratch, (size_t) H, 0);
    memcpy(P.h_models, S.models, (size_t) H * 12 * sizeof(double));
    memcpy(P.h_penalty, S.penalty, (size_t) H * sizeof(double));
    if (!valid_in_penalty) memcpy(P.h_valid, S.valid, (size_t) H * sizeof(int));
    for (int h = 0; h < H; h++) {
        if (valid_in_penalty) P.h_valid[h] = !(P.h_penalty[h] < 0);
        if (!P.h_valid[h]) {
            P.h_penalty[h] = INFINITY;
            memset(P.h_models + 12 * (size_t) h, 0, 12 * sizeof(double));
        }
    }
}

void hyp_select(const P3pSelectOut &s, alva_p3p_hyp_problem &P) {
    P.best = s.best;
    P.n_valid_used = s.n_valid_used;
    P.n_inliers = s.n_inliers;
    P.have_model = s.have_model;
    memcpy(P.model, s.model, sizeof(s.model));
}

// route 0: alva_p3p_prepare + alva_p3p_launch, the samples copied into the pinned block instead of drawn
int hyp_single(alva_ctx *ctx, alva_p3p_hyp_problem &P, float err_threshold, float fx, float fy) {
    const int n = P.n, H = P.H;
    ALVA_ARG(P.h_masks);
    const size_t words = P3pScratch::mask_words((size_t) n);
    uint8_t *pin = nullptr;
    int rc = alva_ctx_pinned(ctx, P3pPin::bytes((size_t) H, (size_t) n, (size_t) n), (void **) &pin);
    if (rc) return rc;
    ALVA_ARG(pose_block_aligned(pin, 256));
    const P3pPin B(pin, (size_t) H, (size_t) n, (size_t) n);
    memcpy(B.samples, P.h_samples, pose_samples_bytes((size_t) H));
    P3pArgs A{};
    rc = alva_p3p_prepare(ctx, P.d_bearings, P.d_wpts, n, P.max_iters, err_threshold, 0, 0u, fx, fy, H, nullptr, B.sel, B.inlier, &A);
    if (rc) return rc;
    A.samples = B.samples;
    rc = alva_p3p_launch(ctx, A);
    if (rc) return rc;
    if (ctx->p3p_deferred) ALVA_HIP(alva_stream_sync(ctx->stream));   // (a lane's deposit: issued and finished before the copies are queued)
    // the scratch block begins with the models; its host copy has alva_p3p_prepare's layout
    ALVA_HIP(hipMemcpyAsync(B.scratch, A.models, P3pScratch::bytes((size_t) H, (size_t) n), hipMemcpyDeviceToHost, ctx->stream));
    ALVA_HIP(hipMemcpyAsync(B.counter, A.counter, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    ALVA_HIP(alva_stream_sync(ctx->stream));
    hyp_unpack(B.scratch, true, P);
    const unsigned long long *masks = P3pScratch(B.scratch, (size_t) H, (size_t) n).masks;
    for (int h = 0; h < H; h++) {
        if (P.h_valid[h]) memcpy(P.h_masks + (size_t) h * words, masks + (size_t) h * words, words * 8);
        else memset(P.h_masks + (size_t) h * words, 0, words * 8);   // (a hypothesis without a model writes no mask)
    }
    P3pSelectOut sel;
    memcpy(&sel, B.sel, sizeof(sel));
    hyp_select(sel, P);
    memcpy(P.h_inlier, B.inlier, (size_t) n);
    memcpy(&P.counter_after, B.counter, sizeof(int));
    return ALVA_OK;
}

// route 1: every problem an item of ONE alva_p3p_batch_enqueue.  One device block: items | per problem samples, scratch, counter,
// selection record, inlier bytes; its image is staged in pinned memory, copied in, and the whole block copied back after the launches.
int hyp_batch(alva_ctx *ctx, alva_p3p_hyp_problem *problems, int count, float err_threshold, float fx, float fy) {
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    struct Off {
        size_t samples, scratch, counter, sel, inlier;
    };
    std::vector<Off> off((size_t) count);
    size_t total = up(sizeof(P3pArgs) * (size_t) count);
    int H_max = 0, n_max = 0;
    for (int c = 0; c < count; c++) {
        const alva_p3p_hyp_problem &P = problems[c];
        ALVA_ARG(P.n <= ALVA_P3P_LDS_DEFAULT_N);
        Off &o = off[(size_t) c];
        o.samples = total;
        o.scratch = o.samples + up(pose_samples_bytes((size_t) P.H));
        o.counter = o.scratch + up(alva_p3p_batch_scratch_bytes(P.H));
        o.sel = o.counter + 256;
        o.inlier = o.sel + 256;
        total = o.inlier + up((size_t) P.n);
        H_max = std::max(H_max, P.H);
        n_max = std::max(n_max, P.n);
    }
    uint8_t *pin = nullptr, *dev = nullptr;
    int rc = alva_ctx_pinned(ctx, total, (void **) &pin);
    if (rc) return rc;
    rc = alva_ctx_scratch(ctx, 2, total, (void **) &dev);
    if (rc) return rc;
    memset(pin, 0, total);
    for (int c = 0; c < count; c++) {
        const alva_p3p_hyp_problem &P = problems[c];
        const Off &o = off[(size_t) c];
        memcpy(pin + o.samples, P.h_samples, (size_t) P.H * 16);
        rc = alva_p3p_batch_item_fill(pin + sizeof(P3pArgs) * (size_t) c, P.d_bearings, P.d_wpts, P.n, P.max_iters, err_threshold, fx, fy, P.H,
                                      (const int *) (dev + o.samples), dev + o.scratch, (int *) (dev + o.counter),
                                      (P3pSelectOut *) (dev + o.sel), dev + o.inlier);
        if (rc) return rc;
    }
    ALVA_HIP(hipMemcpyAsync(dev, pin, total, hipMemcpyHostToDevice, ctx->stream));
    rc = alva_p3p_batch_enqueue(ctx, dev, count, H_max, n_max);
    if (rc) return rc;
    ALVA_HIP(hipMemcpyAsync(pin, dev, total, hipMemcpyDeviceToHost, ctx->stream));
    ALVA_HIP(alva_stream_sync(ctx->stream));
    for (int c = 0; c < count; c++) {
        alva_p3p_hyp_problem &P = problems[c];
        const Off &o = off[(size_t) c];
        hyp_unpack(pin + o.scratch, false, P);
        P3pSelectOut sel;
        memcpy(&sel, pin + o.sel, sizeof(sel));
        hyp_select(sel, P);
        memcpy(P.h_inlier, pin + o.inlier, (size_t) P.n);
        memcpy(&P.counter_after, pin + o.counter, sizeof(int));
    }
    return ALVA_OK;
}

}  // namespace

extern "C" int alva_p3p_hypotheses(alva_ctx *ctx, alva_p3p_hyp_problem *problems, int count, float err_threshold, float fx, float fy, int route) {
    ALVA_ARG(ctx && problems && count > 0 && count <= 65535 && (route == 0 || route == 1));
    for (int c = 0; c < count; c++) {
        const alva_p3p_hyp_problem &P = problems[c];
        ALVA_ARG(P.n >= 4 && P.n <= ALVA_P3P_MAX_N && P.H > 0 && P.max_iters > 0);
        ALVA_ARG(P.d_bearings && P.d_wpts && P.h_samples && P.h_models && P.h_valid && P.h_penalty && P.h_inlier);
        for (int k = 0; k < 4 * P.H; k++) ALVA_ARG(P.h_samples[k] >= 0 && P.h_samples[k] < P.n);   // the kernels index with them unchecked
    }
    if (route == 1) return hyp_batch(ctx, problems, count, err_threshold, fx, fy);
    for (int c = 0; c < count; c++) {
        const int rc = hyp_single(ctx, problems[c], err_threshold, fx, fy);
        if (rc) return rc;
    }
    return ALVA_OK;
}
