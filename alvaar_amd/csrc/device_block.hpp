// One owned device allocation: the pointer and its size, freed by the destructor.  Not copyable; movable, so two blocks can be swapped.
// WHEN a block is replaced -- once, when a call needs more, when a key changes -- is its owner's policy; the type does not know it.
// (Arena, stage_arena.hpp, is the per-call staging with its own doubling growth; this is for state kept between calls.)
#pragma once
#include "common.hpp"
#include <utility>

namespace alva_slam {

struct DeviceBlock {
    uint8_t *ptr = nullptr;
    size_t bytes = 0;   // what was asked for, rounded up to 256; 0 exactly when ptr is null
    DeviceBlock() = default;
    DeviceBlock(const DeviceBlock &) = delete;
    DeviceBlock &operator=(const DeviceBlock &) = delete;
    DeviceBlock(DeviceBlock &&o) noexcept { *this = std::move(o); }
    DeviceBlock &operator=(DeviceBlock &&o) noexcept {
        std::swap(ptr, o.ptr);
        std::swap(bytes, o.bytes);
        return *this;
    }
    ~DeviceBlock() {
        if (ptr) (void) hipFree(ptr);
    }
    explicit operator bool() const { return ptr != nullptr; }

    // an EMPTY block gets its memory: nothing on the device reads it yet, so there is nothing to wait for.  The size is recorded only
    // after the allocation succeeded
    int allocate(size_t need) {
        if (ptr) return ALVA_ERR_STATE;
        const size_t b = (need + 255) / 256 * 256;
        ALVA_HIP(hipMalloc((void **) &ptr, b));
        bytes = b;
        return ALVA_OK;
    }
    // the block replaced by one of `need` bytes.  What is enqueued on `st` may still read the old one, so the stream is waited for
    // first; from the free on the block is empty, and stays so when the allocation fails: the owner's next call allocates again.
    // -> ALVA_OK or the library's error code
    int replace(size_t need, hipStream_t st) {
        ALVA_HIP(alva_stream_sync(st));
        if (ptr) ALVA_HIP(hipFree(ptr));
        ptr = nullptr;
        bytes = 0;
        return allocate(need);
    }
    // freed now, behind whatever `st` still has to do with it
    int release(hipStream_t st) {
        if (!ptr) return ALVA_OK;
        ALVA_HIP(alva_stream_sync(st));
        ALVA_HIP(hipFree(ptr));
        ptr = nullptr;
        bytes = 0;
        return ALVA_OK;
    }
};

}  // namespace alva_slam
