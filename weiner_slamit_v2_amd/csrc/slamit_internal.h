// slamit_internal.h — error plumbing, the global-pointer qualifier and the staged-call helper shared by the translation units.
#ifndef SLAMIT_INTERNAL_H
#define SLAMIT_INTERNAL_H
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../include/slamit.h"
#include "stage_binder.h"

int slamit_fail(int code, const char* msg);                 // records msg, returns code
int slamit_refuse(const char* where, const char* what, int code = SLAMIT_ERR_ARG);   // records "<where>: <what>", returns code
int slamit_fail_hip(hipError_t e, const char* where);       // records "<where>: <hip error>", returns SLAMIT_ERR_DEVICE

// `where` (an entry point, or the expression itself) goes into the error text
#define HIP_TRY_AT(where, expr)                                              \
    do {                                                                     \
        hipError_t _e = (expr);                                              \
        if (_e != hipSuccess) return slamit_fail_hip(_e, where);             \
    } while (0)
#define HIP_TRY(expr) HIP_TRY_AT(#expr, expr)

// Qualifier of a device pointer that a kernel reads out of a record in memory (BaWin, PoseFrame, Sim3Prob, Sim3RansacProb): the global
// address space in the device pass, nothing on the host.  Without it such a pointer is GENERIC to the compiler and every access through
// it a flat_load / flat_store (slower to issue, and counted in lgkmcnt, so LDS waits also wait for outstanding HBM loads).  Host code
// that fills a record is parsed in the device pass too: it casts (`(SLAMIT_GLOBAL double*)p`, a no-op on the host).
#if defined(__HIP_DEVICE_COMPILE__)
#define SLAMIT_GLOBAL __attribute__((address_space(1)))
#else
#define SLAMIT_GLOBAL
#endif
// the same cast for any element type: a record's field takes slamit_global(pointer the binder returned)
template <typename T>
inline SLAMIT_GLOBAL T* slamit_global(T* p) { return (SLAMIT_GLOBAL T*)p; }

// Every entry point works on the device it is given and leaves the caller's current device as it found it (a torch
// host thread must not have its device changed under it).
struct SlamitDeviceGuard {
    int prev;
    hipError_t err;
    explicit SlamitDeviceGuard(int device) : prev(-1), err(hipSuccess) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (device != prev) err = hipSetDevice(device);
    }
    ~SlamitDeviceGuard() { int cur = -1; if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) hipSetDevice(prev); }
    SlamitDeviceGuard(const SlamitDeviceGuard&) = delete;
    SlamitDeviceGuard& operator=(const SlamitDeviceGuard&) = delete;
};
#define SLAMIT_USE_DEVICE(device)                                                  \
    SlamitDeviceGuard slamit_device_guard_(device);                                \
    if (slamit_device_guard_.err != hipSuccess) return slamit_fail_hip(slamit_device_guard_.err, "hipSetDevice")

// frustum.hip: d_count[f] = number of nonzero flags among the first min(d_m[f], q_cap) of d_valid[f][q_cap], one wavefront per frame
hipError_t slamit_launch_valid_count(const uint8_t* d_valid, const int32_t* d_m, int q_cap, int nframes, int32_t* d_count, hipStream_t stream);

struct slamit_orb;
int slamit_orb_device_of(const slamit_orb* h);   // orb_api.hip: the device of a handle (-1 for none)

int slamit_default_device();   // slamit_set_device() of this thread, or the current device

// The library's environment switches, read by slamit_read_switches() when a handle is created.
// The first six let a test force a second path on the same input; the last three print diagnostics on stderr.
struct SlamitSwitches {
    bool resize_no8;       // SLAMIT_RESIZE_NO8=1: the four-pixel resize kernel on every level
    bool blur_no_stream;   // SLAMIT_BLUR_NO_STREAM=1: the tile blur kernel on every level
    bool ba_no_band;       // SLAMIT_BA_NO_BAND: every window through the blocked reduced solve
    bool ba_no_sf;         // SLAMIT_BA_SF=0: the tiled Schur product for every window
    int ba_sf_cap;         // SLAMIT_BA_SF_CAP: k slabs per floating-window group (0: the default)
    bool ba_keep_order;    // SLAMIT_BA_KEEP_ORDER: the caller's keyframe order, never renumbered
    bool ba_timing;        // SLAMIT_BA_TIMING: host phases of every solve
    bool ba_diag;          // SLAMIT_BA_DIAG: in-kernel clock and phases of the last LDLt launch (BA_DIAG_STAMPS builds)
    bool ba_diag_waves;    // SLAMIT_BA_DIAG_WAVES: busy cycles of the LDLt waves (BA_DIAG_WAVES builds)
};
SlamitSwitches slamit_read_switches();

// One pinned staging block, one device slab and one stream per host thread and call site, kept between calls: the
// per-frame entry points (pose, Sim3, guided search ...) are called every frame by a tracking thread, and a fresh
// hipMalloc / hipFree pair per call costs more than their kernels.  The blocks are released when the thread exits
// (or by slamit_release_thread_scratch(), which every call site registers with).
struct SlamitScratch {
    int device = -1;
    unsigned char* host = nullptr; size_t host_bytes = 0;
    unsigned char* dev = nullptr; size_t dev_bytes = 0;
    hipStream_t st = nullptr;
    void release() {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess) { host = nullptr; dev = nullptr; st = nullptr; host_bytes = dev_bytes = 0; return; }   // runtime already gone (process exit)
        if (st) hipStreamSynchronize(st);
        if (host) hipHostFree(host);
        if (dev) hipFree(dev);
        if (st) hipStreamDestroy(st);
        host = nullptr; dev = nullptr; st = nullptr; host_bytes = dev_bytes = 0; device = -1;
    }
    ~SlamitScratch() { release(); }
};
void slamit_scratch_register(SlamitScratch* s);   // so that slamit_release_thread_scratch() finds it

// the caller has made `device` current; host_bytes of pinned memory, dev_bytes of device memory
inline hipError_t slamit_scratch_reserve(SlamitScratch& S, int device, size_t host_bytes, size_t dev_bytes) {
    if (S.device == device && S.host_bytes >= host_bytes && S.dev_bytes >= dev_bytes && S.st) return hipSuccess;
    if (S.device == -1 && !S.st && !S.host && !S.dev) slamit_scratch_register(&S);
    if (S.st) hipStreamSynchronize(S.st);
    if (S.host) hipHostFree(S.host);
    if (S.dev) hipFree(S.dev);
    if (S.st && S.device != device) { hipStreamDestroy(S.st); S.st = nullptr; }   // a stream belongs to the device it was created on
    S.host = nullptr; S.dev = nullptr; S.host_bytes = S.dev_bytes = 0; S.device = device;
    hipError_t e = hipSuccess;
    if (!S.st) e = hipStreamCreateWithFlags(&S.st, hipStreamNonBlocking);
    const size_t hw = host_bytes + host_bytes / 2 + 4096, dw = dev_bytes + dev_bytes / 2 + 4096;
    if (e == hipSuccess) e = hipHostMalloc((void**)&S.host, hw, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc((void**)&S.dev, dw);
    if (e == hipSuccess) { S.host_bytes = hw; S.dev_bytes = dw; }
    return e;
}

// A staged call (the host-pointer entry points): lay the block out (StageLayout: inputs | outputs | device-only), reserve, pack the
// inputs into S.host through their spans, upload, launch on S.st with pointers from the same spans at S.dev, download and wait,
// unpack the outputs from S.host.  One copy each way; each step returns the first error.  The single-problem entry points and the
// pose / Sim3 blocks (lm_layout.h) spell these steps out over their own spans; the batch-of-problems ones go through
// slamit_staged_batch below, where a StageBinder does the layout, the packing, the pointers and the unpacking from one mention per array.
inline hipError_t slamit_stage_reserve(SlamitScratch& S, int device, const StageLayout& L) { return slamit_scratch_reserve(S, device, L.io_bytes, L.dev_bytes); }
inline hipError_t slamit_stage_upload(SlamitScratch& S, const StageLayout& L) { return hipMemcpyAsync(S.dev, S.host, L.in_bytes, hipMemcpyHostToDevice, S.st); }
inline hipError_t slamit_stage_download_and_wait(SlamitScratch& S, const StageLayout& L) {   // the launches' error, the copy down, the stream
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(S.host + L.out_off, S.dev + L.out_off, L.io_bytes - L.out_off, hipMemcpyDeviceToHost, S.st);
    if (e == hipSuccess) e = hipStreamSynchronize(S.st);
    return e;
}

// A staged call over a batch of `nrec` records of type Rec (the "batch of problems" entry points), with the arrays named once
// (stage_binder.h).  describe(StageBinder& b, int f, Rec& q) fills the zeroed record q of problem f and names every array of the problem
// as b.in / b.in_fill / b.out / b.out_view / b.scratch, whose result goes into q through slamit_global().  It runs twice per
// problem: first to measure, with q a dummy and null from every call, then, once the block is reserved, with q in the pinned record
// array, which is the first thing of the input region.  It must ask for the same sizes both times; what it does with a host pointer
// (a transpose into an in_fill array) it does only when that pointer is not null.  launch(const Rec* d_recs) starts the kernels on
// S.st and returns their launch error.  When this returns SLAMIT_OK the b.out arrays are in the caller's hands and the views that
// b.out_view filled can be read.  A describe function that changed between the passes fails the call before anything is uploaded.
template <typename Rec, typename Describe, typename Launch>
int slamit_staged_batch(const char* where, SlamitScratch& S, int device, int nrec, Describe describe, Launch launch) {
    StageBinder b;
    auto pass = [&]() -> const Rec* {
        Rec dummy;
        Rec* q = nullptr;
        const Rec* const d_recs = b.in_fill<Rec>((size_t)nrec, &q);
        memset(q ? q : &dummy, 0, sizeof(Rec) * (q ? (size_t)nrec : 1));
        for (int f = 0; f < nrec; ++f) describe(b, f, q ? q[f] : dummy);
        return d_recs;
    };
    pass();
    const StageLayout L = b.plan();
    HIP_TRY_AT(where, slamit_stage_reserve(S, device, L));
    b.bind(S.host, S.dev);
    const Rec* const d_recs = pass();
    if (!b.bound()) return slamit_fail(SLAMIT_ERR_STATE, "staged call: the arrays of the bind pass are not those of the plan pass");
    HIP_TRY_AT(where, slamit_stage_upload(S, L));
    HIP_TRY_AT(where, launch(d_recs));
    HIP_TRY_AT(where, slamit_stage_download_and_wait(S, L));
    b.unpack();
    return SLAMIT_OK;
}

// An in / out array of a host form (covis.hip, upkeep.hip): staged down as an input, copied on the stream into the output that is
// staged back, so that what the kernels leave alone returns as the caller gave it.  describe() clears `io` and names the arrays
// through slamit_inout; launch() calls slamit_copy_inouts first.
struct SlamitInOut { void* dst; const void* src; size_t bytes; };
template <typename T>
static T* slamit_inout(StageBinder& b, std::vector<SlamitInOut>& io, T* host, size_t count) {
    const T* const src = b.in(host, count);
    T* const dst = b.out(host, count);
    if (dst && count) io.push_back({dst, src, sizeof(T) * count});
    return dst;
}
static inline hipError_t slamit_copy_inouts(const std::vector<SlamitInOut>& io, hipStream_t st) {
    for (const SlamitInOut& c : io) {
        const hipError_t e = hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

#endif
