// The per-call staging of the HIP stages (stages_hip.hip) and the scene stages (scene_stages.hip): host arrays cross into device memory
// through two bump arenas that are reset per call -- a pinned host arena (staging both ways, so every copy is asynchronous on the stream)
// and a device arena.  A session has ONE pair (HipStages owns it, HipStages::carve hands it out); a call plans its buffers first (sizes),
// then the arenas are grown once and carved.
#pragma once
#include "common.hpp"

namespace alva_slam {

struct Arena {
    uint8_t *base = nullptr;
    size_t cap = 0, used = 0;
    bool pinned = false;
    int grow(size_t need, hipStream_t st) {
        if (need <= cap) return ALVA_OK;
        if (base) {
            ALVA_HIP(alva_stream_sync(st));
            if (pinned) ALVA_HIP(hipHostFree(base));
            else ALVA_HIP(hipFree(base));
            base = nullptr;
        }
        size_t c = cap ? cap : (size_t) 1 << 20;
        cap = 0;   // nothing is held while the allocation below can still fail (a failed grow must not leave cap > 0 with base == nullptr)
        while (c < need) c *= 2;
        if (pinned) ALVA_HIP(hipHostMalloc((void **) &base, c, hipHostMallocDefault));
        else ALVA_HIP(hipMalloc((void **) &base, c));
        cap = c;
        return ALVA_OK;
    }
    void release() {
        if (base) {
            if (pinned) (void) hipHostFree(base);
            else (void) hipFree(base);
        }
        base = nullptr;
        cap = used = 0;
    }
};

struct StagePlan {
    std::vector<size_t> sizes;
    size_t add(size_t bytes) {
        sizes.push_back((bytes + 255) / 256 * 256);
        return sizes.size() - 1;
    }
};

}  // namespace alva_slam

// planned buffer i of a carve (d, h) on stream st: up = host array -> pinned -> device, down = device -> pinned (read h[i] after the wait)
#define UP(st, i, src, bytes)                                                                     \
    do {                                                                                          \
        if ((bytes) > 0) {                                                                        \
            memcpy(h[i], (src), (bytes));                                                         \
            ALVA_HIP(hipMemcpyAsync(d[i], h[i], (bytes), hipMemcpyHostToDevice, (st)));           \
        }                                                                                         \
    } while (0)
#define DOWN(st, i, bytes)                                                                        \
    do {                                                                                          \
        if ((bytes) > 0) ALVA_HIP(hipMemcpyAsync(h[i], d[i], (bytes), hipMemcpyDeviceToHost, (st))); \
    } while (0)
