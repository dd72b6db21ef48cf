// ba_api.hip — C-ABI of the local bundle adjustment (include/slamit.h, slamit_ba_*).
// Host side of Optimizer::LocalBundleAdjustment (ORB_SLAM2/src/Optimizer.cc:453-778) from the
// point where the graph is assembled (:507) to the point where results are written back (:759):
// upload of the POD window, the two-stage schedule (:659-707), download.  All numerics run in
// ba_kernels.hip; there is no CPU solve path.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <exception>
#include <thread>
#include <vector>

#include "../../include/slamit.h"
#include "ba_plan.h"
#include "ba_schedule.h"
#include "ba_types.h"
#include "slamit_internal.h"

size_t bak_ldlt_smem(int Npad);
hipError_t bak_prepare(int Npad);
void bak_import(hipStream_t st, BaWin* wins, const BaIo* io, const BaBatchPlan& B);
void bak_stage_begin(hipStream_t st, BaWin* wins, const BaBatchPlan& B, int stage, int max_it);
void bak_slot(hipStream_t st, BaWin* wins, const BaBatchPlan& B, bool first, hipEvent_t* ev);
void bak_final(hipStream_t st, BaWin* wins, const BaIo* io, const BaBatchPlan& B);

static_assert(BA_MAX_ITS == SLAMIT_BA_MAX_ITS, "stats capacity");
static_assert(BA_MAX_FREE_KF == SLAMIT_BA_MAX_FREE_KF && BA_NPAD_CEIL == (6 * BA_MAX_FREE_KF + 1 + BA_TILE - 1) / BA_TILE * BA_TILE, "free keyframe ceiling");
static_assert(sizeof(BaState) % 8 == 0, "BaState is copied as 64-bit words");

struct slamit_ba {
    int device;
    hipStream_t stream;
    hipEvent_t ev[2];          // state read-backs of the LM chunks in flight
    int max_kf, max_pt, max_edge, max_batch;
    int max_free_kf;           // free keyframes of a window (the reduced system: Npad_max); max_kf counts free and fixed ones
    int Npad_max, Kpad_max, n_part;
    size_t win_bytes;          // device bytes of one window slab: io section (inputs | outputs) then the workspace
    size_t io_cap;             // bytes of the io section
    uint8_t* d_slab;           // max_batch * win_bytes
    BaWin* d_wins;             // max_batch
    BaState* d_states;         // max_batch
    BaIo* d_io;                // max_batch
    uint8_t* h_pin;            // pinned: every window's packed inputs, then outputs, then 2 x max_batch LM states
    size_t pin_bytes;
    // slamit_ba_profile: six timing events per LM slot of the current solve, and the phase sums of the last profiled one
    bool prof;
    std::vector<hipEvent_t> pev;
    slamit_ba_profile_out prof_last;
    SlamitSwitches sw;         // the environment switches, read when the handle is created
};

namespace {

// Runs fn(b) for every window b of a batch on up to 16 host threads, the caller's own among them (`spread` false: on the caller's alone).
// Nothing thrown in here may cross the C boundary: returns false when fn threw (bad_alloc in a worker's vectors); a thread that cannot
// be created leaves its share to the threads that exist and to the caller's own.
template <typename F>
bool for_each_window(int nwin, bool spread, F&& fn) {
    const int nthreads = spread ? std::max(1, std::min(std::min(nwin, 16), (int)std::thread::hardware_concurrency())) : 1;
    std::atomic<int> next(0);
    std::atomic<bool> failed(false);
    auto work = [&]() {
        for (int b = next.fetch_add(1); b < nwin; b = next.fetch_add(1)) {
            try { fn(b); } catch (...) { failed = true; }
        }
    };
    std::vector<std::thread> pool;
    try {
        for (int t = 1; t < nthreads; ++t) pool.emplace_back(work);
    } catch (...) {}
    work();
    for (std::thread& t : pool) t.join();
    return !failed;
}

// One call of slamit_ba_solve_batch: the arguments, and what its steps hand on to each other.
struct BaSolve {
    slamit_ba* h; int nwin; const slamit_ba_problem* probs; const slamit_ba_opts* opts; slamit_ba_result* results;
    BaBatchPlan B;
    std::vector<BaWin> wins; std::vector<BaIo> io; std::vector<BaWindowPlan> plans;   // per window: the device's record, its io table entry, the host's plan
    size_t pev_used = 0;   // profiling solves: six events per queued slot
    bool stopped = false;  // the caller's stop flag was seen up
};

double tclk() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// every check that does not touch the device (ba_batch_check, ba_plan.cc)
int ba_validate(const BaSolve& s) {
    const BaRefusal r = ba_batch_check(s.probs, s.results, s.nwin, BaCaps{s.h->max_kf, s.h->max_free_kf, s.h->max_pt, s.h->max_edge, s.h->max_batch});
    return r.code == SLAMIT_OK ? SLAMIT_OK : slamit_fail(r.code, r.msg);
}

// the handle's pinned block, grown (with a quarter to spare) when the batch needs more
int ba_grow_pinned(slamit_ba* h, size_t need) {
    if (need <= h->pin_bytes) return SLAMIT_OK;
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (h->h_pin) hipHostFree(h->h_pin);
    h->h_pin = nullptr; h->pin_bytes = 0;
    HIP_TRY(hipHostMalloc((void**)&h->h_pin, need + need / 4, hipHostMallocDefault));
    h->pin_bytes = need + need / 4;
    return SLAMIT_OK;
}

// Per-window preparation (the plan, CSR lists, packing into the pinned block) is host work of ~10 ns per edge: windows are
// independent, so a batch is prepared by a few host threads; the copies are queued afterwards, in order.
int ba_prepare_windows(BaSolve& s) {
    slamit_ba* h = s.h;
    const BaBatchPlan& B = s.B;
    s.wins.resize(s.nwin); s.io.resize(s.nwin); s.plans.resize(s.nwin);
    const BaPlanLimits lim{h->Npad_max, s.nwin, h->sw.ba_keep_order, h->sw.ba_no_sf, h->sw.ba_no_band, h->sw.ba_sf_cap};
    std::atomic<bool> bad_index(false);
    auto prepare = [&](int b) {
        const slamit_ba_problem& P = s.probs[b];
        BaWin& w = s.wins[b];
        BaIo& io = s.io[b];
        memset(&w, 0, sizeof(w));
        if (!ba_plan_window(P, lim, w, s.plans[b])) { bad_index = true; return; }
        ba_pack_inputs(P, s.plans[b], carve_io(h->h_pin + B.in_off[b], P.n_kf, P.n_pt, P.n_edge, P.edge_ur != nullptr, B.side_w[b]));   // the device's packing, in the pinned block
        carve_work(h->d_slab + (size_t)b * h->win_bytes + h->io_cap, w, h->max_kf, h->max_pt, h->max_edge, h->Npad_max, h->Kpad_max, h->n_part, h->max_free_kf);
        const IoLayout& D = B.dio[b];
        w.side = D.side;   // (null unless the window's structure outgrows BaWin's inline arrays)
        w.intr = D.intr; w.pose_col = D.pose_col; w.e_kf = D.e_kf; w.e_pt = D.e_pt; w.e_uv = D.e_uv; w.e_w = D.e_w;
        w.pt_edges = D.pt_edges; w.kf_edges = D.kf_edges; w.pt_ptr = D.pt_ptr; w.kf_ptr = D.kf_ptr;
        w.e_ur = D.e_ur; w.bf = D.bf;
        io.in_pose = D.in_pose; io.in_pt = D.in_pt; io.out_pose = D.out_pose; io.out_pt = D.out_pt;
        io.out_chi2 = D.out_chi2; io.out_flag = D.out_flag; io.out_out1 = D.out_out1; io.out_state = D.out_state;
        w.n_part = h->n_part;
        w.huber_delta = s.opts->huber_delta; w.chi2_gate = s.opts->chi2_gate;
        // stereo observations (EdgeStereoSE3ProjectXYZ): three residual rows per edge in this window, own Huber width and gate
        w.huber_delta_s = s.opts->huber_delta_stereo > 0 ? s.opts->huber_delta_stereo : (double)(float)sqrt(7.815);   // Optimizer.cc:570
        w.chi2_gate_s = s.opts->chi2_gate_stereo > 0 ? s.opts->chi2_gate_stereo : 7.815;                           // Optimizer.cc:696, 740
        w.nrow = P.edge_ur ? 3 : 2;
        w.st = reinterpret_cast<BaState*>(h->d_wins) - (b + 1);
    };
    if (!for_each_window(s.nwin, true, prepare))
        return slamit_fail(SLAMIT_ERR_DEVICE, "slamit_ba_solve_batch: out of host memory while preparing the windows");
    if (bad_index) return slamit_fail(SLAMIT_ERR_ARG, "slamit_ba_solve_batch: edge index out of range");
    return SLAMIT_OK;
}

// one copy per window into its input section, the window and io tables, and the import (which also zeroes the Schur operands' ranges and the LM states)
int ba_queue_uploads(BaSolve& s) {
    slamit_ba* h = s.h;
    for (int b = 0; b < s.nwin; ++b)
        HIP_TRY(hipMemcpyAsync(h->d_slab + (size_t)b * h->win_bytes, h->h_pin + s.B.in_off[b], s.B.dio[b].in_bytes, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->d_wins, s.wins.data(), sizeof(BaWin) * s.nwin, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->d_io, s.io.data(), sizeof(BaIo) * s.nwin, hipMemcpyHostToDevice, h->stream));
    bak_import(h->stream, h->d_wins, h->d_io, s.B);
    return SLAMIT_OK;
}

// profiling solves: the six events of the next slot (null otherwise, or when no event can be had)
hipEvent_t* ba_slot_events(BaSolve& s) {
    slamit_ba* h = s.h;
    if (!h->prof) return nullptr;
    while (h->pev.size() < s.pev_used + 6) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        h->pev.push_back(e);
    }
    s.pev_used += 6;
    return h->pev.data() + s.pev_used - 6;
}

// One stage of the two-stage schedule (Optimizer.cc:659-707), its trial slots queued in the chunks BaStageSchedule deals (ba_schedule.h).
// *stop is polled before every chunk like SparseOptimizer::terminate() (sparse_optimizer.cpp:376) is before every iteration.
int ba_run_stage(BaSolve& s, int stage) {
    slamit_ba* h = s.h;
    const int nwin = s.nwin;
    hipStream_t st = h->stream;
    BaState* hs[2] = {reinterpret_cast<BaState*>(h->h_pin + s.B.st_off), reinterpret_cast<BaState*>(h->h_pin + s.B.st_off) + nwin};
    const int its = stage == 0 ? s.opts->its_robust : s.opts->its_final;
    bak_stage_begin(st, h->d_wins, s.B, stage, its);
    BaStageSchedule sched(stage, its);
    for (bool over = false; !over;) {
        if (s.opts->stop && *s.opts->stop) { s.stopped = true; break; }
        const BaChunk c = sched.next();
        for (int sl = 0; sl < c.nslots; ++sl) bak_slot(st, h->d_wins, s.B, c.first && sl == 0, ba_slot_events(s));
        if (c.nslots) {
            HIP_TRY(hipMemcpyAsync(hs[c.qbuf], reinterpret_cast<BaState*>(h->d_wins) - nwin, sizeof(BaState) * nwin, hipMemcpyDeviceToHost, st));   // (reverse order: only `done` of all is read)
            HIP_TRY(hipEventRecord(h->ev[c.qbuf], st));
        }
        bool all_done = false;
        if (c.wbuf >= 0) {
            HIP_TRY(hipEventSynchronize(h->ev[c.wbuf]));
            all_done = true;
            for (int b = 0; b < nwin; ++b) all_done = all_done && hs[c.wbuf][b].done;
        }
        over = sched.finished(all_done);
    }
    HIP_TRY(hipGetLastError());
    return SLAMIT_OK;
}

// results: one copy per window out of its output section
int ba_download(BaSolve& s) {
    slamit_ba* h = s.h;
    bak_final(h->stream, h->d_wins, h->d_io, s.B);
    for (int b = 0; b < s.nwin; ++b)
        HIP_TRY(hipMemcpyAsync(h->h_pin + s.B.out_off[b], h->d_slab + (size_t)b * h->win_bytes + s.B.dio[b].out_off, s.B.dio[b].bytes - s.B.dio[b].out_off,
                               hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return SLAMIT_OK;
}

// slamit_ba_profile: the phase sums of the solve's slots
void ba_profile_sums(const BaSolve& s) {
    slamit_ba_profile_out& O = s.h->prof_last;
    memset(&O, 0, sizeof(O));
    O.nwin = s.nwin; O.slots = (int32_t)(s.pev_used / 6);
    for (size_t s0 = 0; s0 + 6 <= s.pev_used; s0 += 6)
        for (int ph = 0; ph < SLAMIT_BA_PHASES; ++ph) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, s.h->pev[s0 + ph], s.h->pev[s0 + ph + 1]) == hipSuccess) O.phase_ms[ph] += ms;
        }
    for (int b = 0; b < s.nwin; ++b) O.schur_exec_mflop += s.plans[b].exec_mflop;
}

// window b's output section as the host sees it: same carve, shifted so that its output part starts at out_off[b]
IoLayout ba_host_outputs(const BaSolve& s, int b) {
    const slamit_ba_problem& P = s.probs[b];
    return carve_io(s.h->h_pin + s.B.out_off[b] - s.B.dio[b].out_off, P.n_kf, P.n_pt, P.n_edge, P.edge_ur != nullptr, s.B.side_w[b]);
}

void ba_unpack(BaSolve& s) {
    auto unpack = [&](int b) { ba_unpack_outputs(s.probs[b], s.plans[b], ba_host_outputs(s, b), s.results[b]); };
    for_each_window(s.nwin, s.nwin >= 4, unpack);   // by the host threads that prepared the windows (nothing in it throws)
}

// The diagnostics on stderr (SlamitSwitches::ba_diag_waves, ba_diag, ba_timing; tools/diag/* parse them): window 0's in-kernel stamps, and the
// host phases of the call between the stamps t[0 .. 4] = entry, validated, prepared, uploads queued, LM loop over, and now
void ba_diagnostics(const BaSolve& s, const double* t) {
    const SlamitSwitches& sw = s.h->sw;
    const BaState& S0 = *ba_host_outputs(s, 0).out_state;
    if (sw.ba_diag_waves) fprintf(stderr, "[ba diag] busy cycles of waves 0..7: %llu %llu %llu %llu %llu %llu %llu %llu\n", S0.dbg[0], S0.dbg[1], S0.dbg[2], S0.dbg[3], S0.dbg[4], S0.dbg[5], S0.dbg[6], S0.dbg[7]);
    if (sw.ba_diag) {  // diagnostic builds only: in-kernel clock and phases of the last LDLt launch
        fprintf(stderr, "[ba diag] ldlt shader cycles %llu, realtime ticks (100 MHz) %llu -> %.0f MHz, %.1f us\n",
                S0.dbg[2] - S0.dbg[0], S0.dbg[3] - S0.dbg[1],
                100.0 * (double)(S0.dbg[2] - S0.dbg[0]) / (double)(S0.dbg[3] - S0.dbg[1] + 1), (double)(S0.dbg[3] - S0.dbg[1]) / 100.0);
        fprintf(stderr, "[ba diag] ldlt phase cycles: load %llu factor %llu rows %llu writeback / wave-0 busy %llu trailing / rhs-wave busy %llu backsub %llu, pivot-wave busy %llu\n",
                S0.dbg[4] >> 32, S0.dbg[4] & 0xffffffffull, S0.dbg[5] >> 32, S0.dbg[5] & 0xffffffffull, S0.dbg[6] >> 32, S0.dbg[6] & 0xffffffffull, S0.dbg[7]);
    }
    if (sw.ba_timing)
        fprintf(stderr, "[ba timing] %d windows: validate %.3f | prepare + pack %.3f | queue uploads %.3f | LM loop %.3f | download + unpack %.3f ms\n",
                s.nwin, t[1] - t[0], t[2] - t[1], t[3] - t[2], t[4] - t[3], tclk() - t[4]);
}

int ba_solve_batch_impl(slamit_ba* h, int nwin, const slamit_ba_problem* probs, const slamit_ba_opts* opts, slamit_ba_result* results) {
    if (!h || !opts) return slamit_fail(SLAMIT_ERR_ARG, "slamit_ba_solve_batch: bad argument");
    SLAMIT_USE_DEVICE(h->device);
    BaSolve s{h, nwin, probs, opts, results};
    double t[5] = {tclk()};
    if (int rc = ba_validate(s)) return rc;
    if (nwin == 0) return SLAMIT_OK;
    t[1] = tclk();
    ba_batch_layout(probs, nwin, h->win_bytes, h->d_slab, s.B);
    if (int rc = ba_grow_pinned(h, s.B.pin_need)) return rc;
    if (int rc = ba_prepare_windows(s)) return rc;
    t[2] = tclk();
    ba_batch_launches(s.wins.data(), s.plans.data(), s.B);
    if (int rc = ba_queue_uploads(s)) return rc;
    t[3] = tclk();
    s.stopped = opts->stop && *opts->stop;  // Optimizer.cc:655-657
    for (int stage = 0; stage < 2 && !s.stopped; ++stage)
        if (int rc = ba_run_stage(s, stage)) return rc;
    t[4] = tclk();
    if (int rc = ba_download(s)) return rc;
    if (h->prof) ba_profile_sums(s);
    ba_unpack(s);
    ba_diagnostics(s, t);
    return SLAMIT_OK;
}

}  // namespace

extern "C" {

static int ba_create(int max_kf, int max_free_kf, int max_pt, int max_edge, int max_batch, int device, slamit_ba** out, const char* who) {
    *out = nullptr;
    SLAMIT_USE_DEVICE(device);
    slamit_ba* h = new slamit_ba();
    h->device = device;
    h->sw = slamit_read_switches();
    h->max_kf = max_kf; h->max_free_kf = max_free_kf; h->max_pt = max_pt; h->max_edge = max_edge; h->max_batch = max_batch;
    h->Npad_max = (int)ba_rup((size_t)6 * max_free_kf + 1, BA_TILE);
    h->Kpad_max = (int)ba_rup((size_t)3 * max_pt, (size_t)BA_KC * BA_SPLITS);
    h->n_part = std::max((max_edge + 255) / 256, (std::max(8 * max_pt, max_kf) + 255) / 256) + 1;   // 8 = BA_PG lanes per point
    {
        BaWin probe;
        const size_t side_max = ba_side_needed(h->Npad_max, 6 * max_free_kf) ? ba_side_words(h->Npad_max, 6 * max_free_kf) : 0;
        h->io_cap = carve_io(nullptr, max_kf, max_pt, max_edge, true, side_max).bytes;
        h->win_bytes = h->io_cap + carve_work(nullptr, probe, max_kf, max_pt, max_edge, h->Npad_max, h->Kpad_max, h->n_part, max_free_kf);
    }
    hipError_t e = hipMalloc((void**)&h->d_slab, h->win_bytes * (size_t)max_batch);
    // one block: the LM states in REVERSE order right in front of the window table (state b = (BaState*)d_wins - (b + 1)): a kernel
    // finds its state from the table's address alone (BA_ST, ba_kernels.hip)
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_states, (sizeof(BaState) + sizeof(BaWin)) * (size_t)max_batch);
    if (e == hipSuccess) h->d_wins = reinterpret_cast<BaWin*>(h->d_states + max_batch);
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_io, sizeof(BaIo) * max_batch);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    for (int i = 0; i < 2 && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&h->ev[i], hipEventDisableTiming);
    // (the LDS-resident solves only take windows of up to BA_BLOCKED_MAX_NPAD rows; larger ones take the tiled solve, which needs no attribute)
    if (e == hipSuccess) e = bak_prepare(std::min(h->Npad_max, BA_BLOCKED_MAX_NPAD));
    if (e != hipSuccess) {
        slamit_ba_destroy(h);
        return slamit_fail_hip(e, who);
    }
    *out = h;
    return SLAMIT_OK;
}

int slamit_ba_create(int max_kf, int max_pt, int max_edge, int max_batch, int device, slamit_ba** out) {
    if (!out || max_kf < 1 || max_pt < 1 || max_edge < 1 || max_batch < 1)
        return slamit_fail(SLAMIT_ERR_ARG, "slamit_ba_create: bad argument");
    *out = nullptr;
    const int Npad_max = (int)ba_rup((size_t)6 * max_kf + 1, BA_TILE);
    if (bak_ldlt_smem(Npad_max) > 160 * 1024 - 2048 || Npad_max > BA_TILE * BA_MAX_TILES || Npad_max > 32 * BA_MAX_PANELS)
        return slamit_fail(SLAMIT_ERR_ARG, "slamit_ba_create: max_kf too large for the LDS-resident LDLt panel");
    return ba_create(max_kf, max_kf, max_pt, max_edge, max_batch, device, out, "slamit_ba_create");
}

int slamit_ba_create_ex(int max_kf, int max_free_kf, int max_pt, int max_edge, int max_batch, int device, slamit_ba** out) {
    if (!out || max_kf < 1 || max_free_kf < 1 || max_free_kf > max_kf || max_pt < 1 || max_edge < 1 || max_batch < 1)
        return slamit_fail(SLAMIT_ERR_ARG, "slamit_ba_create_ex: bad argument (1 <= max_free_kf <= max_kf, every maximum >= 1)");
    *out = nullptr;
    if (max_free_kf > BA_MAX_FREE_KF)
        return slamit_fail(SLAMIT_ERR_ARG, "slamit_ba_create_ex: max_free_kf above SLAMIT_BA_MAX_FREE_KF (341: a reduced system of 2048 rows)");
    return ba_create(max_kf, max_free_kf, max_pt, max_edge, max_batch, device, out, "slamit_ba_create_ex");
}

void slamit_ba_destroy(slamit_ba* h) {
    if (!h) return;
    SlamitDeviceGuard guard(h->device);
    hipFree(h->d_slab); hipFree(h->d_states); hipFree(h->d_io);
    if (h->h_pin) hipHostFree(h->h_pin);
    for (int i = 0; i < 2; ++i) if (h->ev[i]) hipEventDestroy(h->ev[i]);
    for (hipEvent_t e : h->pev) hipEventDestroy(e);
    if (h->stream) hipStreamDestroy(h->stream);
    delete h;
}

int slamit_ba_solve_batch(slamit_ba* h, int nwin, const slamit_ba_problem* probs, const slamit_ba_opts* opts,
                          slamit_ba_result* results) {
    try {
        return ba_solve_batch_impl(h, nwin, probs, opts, results);
    } catch (const std::exception& e) {   // (host containers: std::bad_alloc, std::length_error)
        return slamit_fail(SLAMIT_ERR_DEVICE, e.what());
    } catch (...) {
        return slamit_fail(SLAMIT_ERR_DEVICE, "slamit_ba_solve_batch: unexpected exception");
    }
}

int slamit_ba_solve(slamit_ba* h, const slamit_ba_problem* prob, const slamit_ba_opts* opts, slamit_ba_result* res) {
    return slamit_ba_solve_batch(h, 1, prob, opts, res);
}

int slamit_ba_profile(slamit_ba* h, int on) {
    if (!h) return slamit_fail(SLAMIT_ERR_ARG, "slamit_ba_profile: null handle");
    h->prof = on != 0;
    return SLAMIT_OK;
}

int slamit_ba_profile_read(slamit_ba* h, slamit_ba_profile_out* out) {
    if (!h || !out) return slamit_fail(SLAMIT_ERR_ARG, "slamit_ba_profile_read: bad argument");
    *out = h->prof_last;
    return SLAMIT_OK;
}

}  // extern "C"
