// work_arena.h -- the work space of a device entry point, cut into 256-byte aligned regions.  One layout function per family of entry points (abi.hip) takes
// its regions from a WorkArena: run on the caller's d_work it yields the pointers, run on a null base it only counts, and bytes() of that run is what the
// entry point's crc_*_work_bytes function returns.  Size and carve-up cannot disagree: they are the same statements.
#pragma once
#include <cstddef>
#include <cstdint>

class WorkArena {
    uintptr_t base_;        // 0: counting only
    size_t used_ = 0;
public:
    // d_work may be any address: the first region starts at the next 256-byte boundary (bytes() includes the 256 bytes that can cost)
    explicit WorkArena(void *d_work = nullptr) : base_(((uintptr_t)d_work + 255) & ~(uintptr_t)255) {}
    template <class T> T *take(size_t count)
    {
        const size_t at = used_;
        used_ += (count * sizeof(T) + 255) & ~(size_t)255;
        return base_ ? (T *)(base_ + at) : nullptr;
    }
    size_t bytes() const { return used_ + 256; }
};
