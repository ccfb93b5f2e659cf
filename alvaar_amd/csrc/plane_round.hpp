// What k_plane_round (detect_planes.hip) and the claim kernel in front of it with the one launcher of both (track_planes.hip) share: the
// rounds' argument block, the device words, the pinned record, the last-arriver hand-over and the extents' wave reduction.
#pragma once
#include "common.hpp"
#include "plane_fit.hpp"

constexpr int PL_NT = 512, PL_WAVES = PL_NT / 64, PL_TILE = 2048, PL_MAX_GRID = 256;
constexpr int PL_N_CAP = 16384, PL_MAX_PLANES = 8, PL_MAX_ITERS = 4096, PL_SCRATCH_SLOT = 9;   // slot 9: alva_find_plane's, also synchronous

struct PlaneRecord {   // one per round, in pinned memory
    float plane[24];
    int info[8];
    double mom[10];
};

struct PlaneState {    // device words shared by the rounds of one call (zeroed per call)
    int counter;       // arrivals of the running round (its last workgroup resets it)
    int stopped;       // a round stopped: the later launches return at once
    int m;             // live points of the next round
    int pad;
};

struct PlaneArgs {
    const double *pts;        // [n][3]: round 0's live list
    double *live[2];          // [3][cap] SoA coordinates, read by round r from live[r & 1] (r >= 1), written to live[(r + 1) & 1]
    int *live_idx[2];         // [cap] the points' indices in pts
    int *counts;              // [iters] consensus counts of the running round, -1: skipped
    PlaneState *state;
    int *labels;              // [n] or null
    const uint32_t *rand3;    // [max_planes * iters][3] explicit sample words (pinned), or null
    PlaneRecord *out;         // [max_planes]
    int n, cap, iters, min_inliers, grid;
    int seeded;               // 1: round 0 reads live[0] / live_idx[0] and PlaneState::m, as the later rounds do (the claim kernel has
                              // compacted the unclaimed points there); 0: round 0 reads pts (no priors: alva_detect_planes)
    int slot_base;            // round r writes out[slot_base + r] and the label slot_base + r; its sample stream counts r from 0
    uint32_t seed;
    double thickness;
    double t[3], a[3], b[3];  // camera centre, R_wc[:, 0], R_wc[:, 1]
};

// queues `rounds` launches of k_plane_round (rounds 0 .. rounds - 1) on the context's stream, back to back; no wait.  Internal to the
// library: not exported
__attribute__((visibility("hidden"))) int plane_rounds_enqueue(alva_ctx *ctx, const PlaneArgs &A, int rounds);

// The hand-over of a grid of `grid` workgroups: this one's agent-scope stores are released, it arrives at `counter`, and the one that
// arrives last acquires the others' and resets the counter for the launch behind it (stream order).  True, for the whole workgroup,
// in the last one; no workgroup waits for another.  s_last: one LDS word
__device__ __forceinline__ bool plane_last_arriver(int *counter, int grid, int &s_last) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int last = __hip_atomic_fetch_add(counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == grid - 1;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_store(counter, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        s_last = last;
    }
    __syncthreads();
    return s_last;
}

// the extents lo_x hi_x lo_z hi_z over the wave's 64 lanes, in every lane (min / max: exact whatever the order)
__device__ __forceinline__ void plane_ext_wave(double (&ext)[4]) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        ext[0] = fmin(ext[0], __shfl_xor(ext[0], o)); ext[1] = fmax(ext[1], __shfl_xor(ext[1], o));
        ext[2] = fmin(ext[2], __shfl_xor(ext[2], o)); ext[3] = fmax(ext[3], __shfl_xor(ext[3], o));
    }
}
