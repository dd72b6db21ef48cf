// stage_layout.h — byte layout of one staging block that exists twice with identical offsets: in pinned host memory and on the
// device (SlamitScratch, slamit_internal.h).  Regions are taken in order: inputs, then outputs, then device-only workspace.
// Plain C++17 (no HIP): the host-pointer entry points and the CPU test of the layouts (tests/test_stage_layout.py) both build it.
#ifndef SLAMIT_STAGE_LAYOUT_H
#define SLAMIT_STAGE_LAYOUT_H
#include <stddef.h>

// `count` elements of T at byte `off` of the block; the host and the device pointer of a region both come from its one span
template <typename T>
struct StageSpan {
    size_t off = 0, count = 0;
    T* at(unsigned char* base) const { return reinterpret_cast<T*>(base + off); }
    size_t bytes() const { return sizeof(T) * count; }
};

struct StageLayout {
    size_t in_bytes = 0;    // [0, in_bytes) goes up
    size_t out_off = 0;     // [out_off, io_bytes) comes down
    size_t io_bytes = 0;    // size of the pinned block
    size_t dev_bytes = 0;   // size of the device block: everything taken so far
    template <typename T>
    StageSpan<T> take(size_t count, size_t align = 256) {   // `align`: a power of two; take(0) is an empty span at a valid offset
        if (align < alignof(T)) align = alignof(T);
        StageSpan<T> s;
        s.off = dev_bytes = (dev_bytes + align - 1) & ~(align - 1);
        s.count = count;
        dev_bytes += sizeof(T) * count;
        return s;
    }
    // the outputs start on a boundary of their own, so the copy down never starts in the middle of a line
    void end_inputs(size_t out_align = 256) { in_bytes = dev_bytes; out_off = dev_bytes = (dev_bytes + out_align - 1) & ~(out_align - 1); }
    void end_outputs() { io_bytes = dev_bytes; }   // what is taken after this lives on the device only
};

#endif
