// stage_binder.h — names every array of a staged call once.  An entry point writes ONE describe function that mentions each array
// of its C-ABI together with its element count; the binder runs it twice over the same StageBinder:
//
//   plan pass   (a fresh binder)     measures the three regions of the block only; every call returns null, nothing is copied
//   bind pass   (after bind())       hands out the device pointers, copies the inputs into the pinned block and notes where the
//                                    outputs have to go; unpack() copies those down after the wait
//
// The block is StageLayout's: [inputs | outputs from a 256-byte boundary | device-only], every array on a 16-byte boundary, one copy
// each way.  A describe function that asks for other sizes in the bind pass than in the plan pass is a bug: such a call gets null,
// copies nothing, and bound() reports it, so that nothing is launched.  Plain C++17 (no HIP): the entry points and the CPU test
// (tests/test_stage_binder.py) both build it.  The binder knows nothing of address spaces (slamit_internal.h: slamit_global).
#ifndef SLAMIT_STAGE_BINDER_H
#define SLAMIT_STAGE_BINDER_H
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "stage_layout.h"

// `count` elements in the pinned block that came down with the outputs
template <typename T>
struct StageView {
    const T* data = nullptr;
    size_t count = 0;
};

class StageBinder {
public:
    // An input: `count` elements of `src` go up.  A null src or a count of 0 takes no room; a null src returns null.
    template <typename T>
    T* in(const T* src, size_t count) {
        if (!src) return nullptr;
        T* host;
        T* const d = take<T>(IN, count, &host);
        if (host && count) memcpy(host, src, sizeof(T) * count);
        return d;
    }
    // An input the caller writes itself (a transpose, rows without their padding, the records): *host is where, or null in the plan pass.
    template <typename T>
    T* in_fill(size_t count, T** host) { return take<T>(IN, count, host); }
    // An output: `count` elements come down into `dst` in unpack().  A null dst takes no room and returns null.
    template <typename T>
    T* out(T* dst, size_t count) {
        if (!dst) return nullptr;
        T* host;
        T* const d = take<T>(OUT, count, &host);
        if (!binding_) ++n_down_;
        else if (host && count) down_.push_back(Down{dst, host, sizeof(T) * count});
        return d;
    }
    // An output the entry point reads itself after the wait (wave counts, counters): v->data is where, or null in the plan pass.
    template <typename T>
    T* out_view(size_t count, StageView<T>* v) {
        T* h;
        T* const d = take<T>(OUT, count, &h);
        v->data = h; v->count = count;
        return d;
    }
    // Workspace that lives on the device only.
    template <typename T>
    T* scratch(size_t count) { return take<T>(DEV, count, nullptr); }

    // Ends the plan pass: the layout of the block to reserve.
    StageLayout plan() {
        StageLayout L;
        L.take<unsigned char>(cur_[IN], ALIGN);
        L.end_inputs();
        L.take<unsigned char>(cur_[OUT], ALIGN);
        L.end_outputs();
        const size_t dev_off = L.take<unsigned char>(cur_[DEV]).off;
        const size_t base[3] = {0, L.out_off, dev_off};   // multiples of 256, so an offset is aligned in the block as it was in its region
        for (int r = 0; r < 3; ++r) { end_[r] = base[r] + cur_[r]; cur_[r] = base[r]; }
        return L;
    }
    // Starts the bind pass on the two copies of the block.
    void bind(unsigned char* host, unsigned char* dev) {
        host_ = reinterpret_cast<uintptr_t>(host); dev_ = reinterpret_cast<uintptr_t>(dev);
        binding_ = true;
        down_.reserve(n_down_);
    }
    // After the bind pass: did it take exactly what the plan pass measured?
    bool bound() const { return binding_ && !bad_ && cur_[IN] == end_[IN] && cur_[OUT] == end_[OUT] && cur_[DEV] == end_[DEV]; }
    // After the copy down: the outputs into the caller's arrays.
    void unpack() const {
        for (const Down& d : down_) memcpy(d.dst, d.src, d.bytes);
    }

private:
    enum { IN, OUT, DEV };
    static constexpr size_t ALIGN = 16;
    struct Down { void* dst; const void* src; size_t bytes; };

    // `count` elements of T in region r: the device pointer and, where asked for, the host one; null in the plan pass and after a mismatch.
    // An empty array takes no room and sits at the region's cursor.
    template <typename T>
    T* take(int r, size_t count, T** host) {
        static_assert(alignof(T) <= ALIGN, "every array starts on a 16-byte boundary");
        size_t off = cur_[r];
        if (count) {
            off = (off + ALIGN - 1) & ~(ALIGN - 1);
            cur_[r] = off + sizeof(T) * count;
            if (binding_ && cur_[r] > end_[r]) bad_ = true;   // more than planned: the block has no room for it
        }
        const bool live = binding_ && !bad_;
        if (host) *host = live ? reinterpret_cast<T*>(host_ + off) : nullptr;
        return live ? reinterpret_cast<T*>(dev_ + off) : nullptr;
    }

    size_t cur_[3] = {0, 0, 0};   // plan pass: bytes taken of each region; bind pass: the region's cursor in the block
    size_t end_[3] = {0, 0, 0};   // where the plan says each region ends
    uintptr_t host_ = 0, dev_ = 0;
    bool binding_ = false, bad_ = false;
    size_t n_down_ = 0;
    std::vector<Down> down_;
};

// the sum of a wave-count array
inline int stage_sum(const int32_t* v, size_t count) {
    int acc = 0;
    for (size_t w = 0; w < count; ++w) acc += v[w];
    return acc;
}

#endif
