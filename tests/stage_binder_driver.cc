// stage_binder_driver.cc — drives csrc/stage_binder.h without a device (tests/test_stage_binder.py builds it as a shared library).  The
// "device" is a second malloc'ed block: upload = memcpy of [0, in_bytes), the "kernel" writes a pattern through the device pointers the
// binder returned, download = memcpy of [out_off, io_bytes).  With -DSTAGE_BINDER_MAIN it is a program that runs a fixed set of
// scenarios and returns non-zero on the first failure, for a sanitizer build:
//   g++ -std=c++17 -Wall -g -fsanitize=address,undefined -fno-sanitize-recover=all -DSTAGE_BINDER_MAIN -I <csrc> stage_binder_driver.cc
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "stage_binder.h"

struct Kp20 { float a, b, c, d; int32_t e; };
struct alignas(16) Rec112 { unsigned char b[112]; };
static_assert(sizeof(Kp20) == 20 && alignof(Kp20) == 4 && sizeof(Rec112) == 112 && alignof(Rec112) == 16, "the test's element types");

enum { K_IN, K_IN_FILL, K_OUT, K_OUT_VIEW, K_SCRATCH };
enum { OK_PLAN_NULL = 1, OK_INPUT = 2, OK_OUTPUT = 4, OK_GUARDS = 8 };
static const size_t GUARD = 64;
static const int64_t BUMP = 64;   // the most a test adds to a count between the passes
static const uint64_t NONE = ~0ull;

struct Req { int64_t prob, kind, type, count, null; };   // null: in / out get a null src / dst
struct Got { void* dev; void* host; };

static unsigned char in_byte(size_t r, size_t j) { return (unsigned char)(r * 37 + j * 11 + 5); }
static unsigned char out_byte(size_t r, size_t j) { return (unsigned char)(r * 53 + j * 7 + 1); }

template <typename T>
static Got ask(StageBinder& b, int kind, size_t count, void* user, bool only_offsets) {
    Got g = {nullptr, nullptr};
    T* h = nullptr;
    StageView<T> v;
    if (only_offsets && kind == K_IN) kind = K_IN_FILL;    // nothing is allocated: nothing may be copied
    if (only_offsets && kind == K_OUT) kind = K_OUT_VIEW;
    switch (kind) {
        case K_IN: g.dev = b.in(static_cast<const T*>(user), count); break;
        case K_IN_FILL: g.dev = b.in_fill<T>(count, &h); g.host = h; break;
        case K_OUT: g.dev = b.out(static_cast<T*>(user), count); break;
        case K_OUT_VIEW: g.dev = b.out_view<T>(count, &v); g.host = const_cast<T*>(v.data); break;
        default: g.dev = b.scratch<T>(count); break;
    }
    return g;
}

static size_t size_of(int type) {
    static const size_t s[6] = {1, 2, 4, 8, sizeof(Kp20), sizeof(Rec112)};
    return s[type];
}

static Got ask_any(StageBinder& b, const Req& q, size_t count, void* user, bool only_offsets) {
    switch (q.type) {
        case 0: return ask<uint8_t>(b, (int)q.kind, count, user, only_offsets);
        case 1: return ask<uint16_t>(b, (int)q.kind, count, user, only_offsets);
        case 2: return ask<int32_t>(b, (int)q.kind, count, user, only_offsets);
        case 3: return ask<double>(b, (int)q.kind, count, user, only_offsets);
        case 4: return ask<Kp20>(b, (int)q.kind, count, user, only_offsets);
        default: return ask<Rec112>(b, (int)q.kind, count, user, only_offsets);
    }
}

// Runs the k requests of nprob problems through both passes, problem by problem as an entry point's describe function would.
//   bump_req / bump_by: request bump_req asks for count + bump_by in the bind pass (-1: none), which the binder has to report
//   only_offsets: nothing is allocated and nothing copied; the blocks are two made-up addresses (for totals beyond 4 GiB)
//   report: k x (device offset, host offset (both ~0 for null), OK_ flags, bytes); sizes: in_bytes, out_off, io_bytes, dev_bytes, bound()
// Returns 0, or the number of the first check that failed.
extern "C" int drv_run(int nprob, int k, const int64_t* reqs, int bump_req, int64_t bump_by, int only_offsets, uint64_t* report, uint64_t* sizes) {
    const Req* rq = reinterpret_cast<const Req*>(reqs);
    std::vector<unsigned char*> user(k, nullptr);   // an in's source, an out's destination (inside its guards)
    std::vector<Got> got(k);
    int fail = 0;
    if (!only_offsets)
        for (int r = 0; r < k; ++r) {
            const size_t bytes = size_of((int)rq[r].type) * (size_t)rq[r].count;
            if (rq[r].null) continue;
            if (rq[r].kind == K_IN) {
                user[r] = (unsigned char*)malloc(bytes + BUMP * size_of((int)rq[r].type) + 1);   // a bumped bind pass may read that far
                for (size_t j = 0; j < bytes; ++j) user[r][j] = in_byte(r, j);
            } else if (rq[r].kind == K_OUT) {
                user[r] = (unsigned char*)malloc(GUARD + bytes + GUARD);
                memset(user[r], 0xC3, GUARD + bytes + GUARD);
            }
        }
    auto user_ptr = [&](int r) -> void* { return !user[r] ? nullptr : rq[r].kind == K_OUT ? user[r] + GUARD : user[r]; };
    StageBinder b;
    auto pass = [&](bool binding) {
        for (int f = 0; f < nprob; ++f)
            for (int r = 0; r < k; ++r) {
                if (rq[r].prob != f) continue;
                const size_t count = (size_t)(rq[r].count + (binding && r == bump_req ? bump_by : 0));
                // an address that is never read stands for the caller's array where nothing is allocated
                void* u = only_offsets && !rq[r].null ? (void*)&fail : user_ptr(r);
                got[r] = ask_any(b, rq[r], count, u, only_offsets != 0);
                if (binding && got[r].host && rq[r].kind == K_IN_FILL && !only_offsets)
                    for (size_t j = 0; j < size_of((int)rq[r].type) * count; ++j) ((unsigned char*)got[r].host)[j] = in_byte(r, j);
                if (!binding) report[4 * r + 2] = (!got[r].dev && !got[r].host) ? OK_PLAN_NULL : 0;
            }
    };
    pass(false);
    const StageLayout L = b.plan();
    sizes[0] = L.in_bytes; sizes[1] = L.out_off; sizes[2] = L.io_bytes; sizes[3] = L.dev_bytes;
    unsigned char* host = only_offsets ? reinterpret_cast<unsigned char*>(uintptr_t(1) << 20) : (unsigned char*)malloc(L.io_bytes + 1);
    unsigned char* dev = only_offsets ? reinterpret_cast<unsigned char*>(uintptr_t(1) << 52) : (unsigned char*)malloc(L.dev_bytes + 1);
    if (!only_offsets) { memset(host, 0xEE, L.io_bytes); memset(dev, 0xDD, L.dev_bytes); }
    b.bind(host, dev);
    pass(true);
    sizes[4] = b.bound();
    for (int r = 0; r < k; ++r) {
        report[4 * r] = got[r].dev ? (uint64_t)((uintptr_t)got[r].dev - (uintptr_t)dev) : NONE;
        report[4 * r + 1] = got[r].host ? (uint64_t)((uintptr_t)got[r].host - (uintptr_t)host) : NONE;
        report[4 * r + 3] = size_of((int)rq[r].type) * (uint64_t)rq[r].count;
    }
    if (b.bound() && !only_offsets) {
        memcpy(dev, host, L.in_bytes);                                                   // upload
        for (int r = 0; r < k; ++r) {                                                    // the kernel: reads the inputs, writes everything else
            const size_t bytes = (size_t)report[4 * r + 3];
            unsigned char* d = (unsigned char*)got[r].dev;
            if (!d) continue;
            if (rq[r].kind == K_IN || rq[r].kind == K_IN_FILL) {
                bool same = true;
                for (size_t j = 0; j < bytes; ++j) same = same && d[j] == in_byte(r, j);
                if (same) report[4 * r + 2] |= OK_INPUT;
                else if (!fail) fail = 100 + r;
            } else {
                for (size_t j = 0; j < bytes; ++j) d[j] = out_byte(r, j);
            }
        }
        memcpy(host + L.out_off, dev + L.out_off, L.io_bytes - L.out_off);               // download
        b.unpack();
        for (int r = 0; r < k; ++r) {
            const size_t bytes = (size_t)report[4 * r + 3];
            if (rq[r].kind == K_OUT && user[r]) {
                bool same = true, guards = true;
                for (size_t j = 0; j < bytes; ++j) same = same && user[r][GUARD + j] == out_byte(r, j);
                for (size_t j = 0; j < GUARD; ++j) guards = guards && user[r][j] == 0xC3 && user[r][GUARD + bytes + j] == 0xC3;
                report[4 * r + 2] |= (same ? OK_OUTPUT : 0) | (guards ? OK_GUARDS : 0);
                if ((!same || !guards) && !fail) fail = 200 + r;
            } else if (rq[r].kind == K_OUT_VIEW && got[r].host) {
                bool same = true;
                for (size_t j = 0; j < bytes; ++j) same = same && ((unsigned char*)got[r].host)[j] == out_byte(r, j);
                report[4 * r + 2] |= same ? OK_OUTPUT : 0;
                if (!same && !fail) fail = 300 + r;
            }
        }
    }
    if (!only_offsets) { free(host); free(dev); }
    for (int r = 0; r < k; ++r) free(user[r]);
    return fail;
}

#ifdef STAGE_BINDER_MAIN
// every count of the test through every call and type, in batches of one problem and of three with an empty one in the middle; then
// the describe functions that change between the passes
int main() {
    static const int64_t counts[6] = {0, 1, 63, 64, 65, 257};
    int runs = 0;
    for (int nprob : {1, 3})
        for (int c = 0; c < 6; ++c) {
            std::vector<int64_t> reqs;
            for (int f = 0; f < nprob; ++f) {
                if (nprob == 3 && f == 1) continue;   // the empty problem asks for nothing but empty arrays
                for (int kind = 0; kind < 5; ++kind)
                    for (int type = 0; type < 6; ++type) {
                        const int64_t q[5] = {f, kind, type, counts[(c + type + f) % 6], (kind + type + c) % 7 == 0};
                        reqs.insert(reqs.end(), q, q + 5);
                    }
            }
            if (nprob == 3)
                for (int kind = 0; kind < 5; ++kind) { const int64_t q[5] = {1, kind, kind, 0, 0}; reqs.insert(reqs.end(), q, q + 5); }
            const int k = (int)(reqs.size() / 5);
            std::vector<uint64_t> report(4 * k);
            uint64_t sizes[5];
            for (int bump = -1; bump < k; bump += (bump < 0 ? 1 : 7)) {
                // 64 more elements, or none at all: either moves what follows, or the region's end (a change that hides in the padding
                // in front of the next array changes no total and does no harm)
                const int64_t by = bump < 0 ? 0 : (bump % 2 ? BUMP : -reqs[5 * bump + 3]);
                const bool changes = bump >= 0 && !reqs[5 * bump + 4] && by != 0;
                if (bump >= 0 && !changes) continue;
                const int rc = drv_run(nprob, k, reqs.data(), bump, by, 0, report.data(), sizes);
                ++runs;
                if (rc || (sizes[4] != 0) == changes) {
                    printf("FAILED: nprob %d count set %d bump %d: check %d, bound %d\n", nprob, c, bump, rc, (int)sizes[4]);
                    return 1;
                }
            }
        }
    printf("stage_binder_driver: %d runs passed\n", runs);
    return 0;
}
#endif
