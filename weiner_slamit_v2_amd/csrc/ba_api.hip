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
#include "ba_types.h"
#include "slamit_internal.h"

size_t bak_ldlt_smem(int Npad);
hipError_t bak_prepare(int Npad);
void bak_import(hipStream_t st, BaWin* wins, const BaIo* io, int max_kf, int max_pt, int max_edge, int Npad, int nwin);
void bak_stage_begin(hipStream_t st, BaWin* wins, int nwin, int max_edge, int stage, int max_it, int robust, bool gate);
void bak_slot(hipStream_t st, BaWin* wins, int nwin, int max_kf, int max_pt, int max_edge, int Npad, int Npad_ldlt, const int* tl_grid, int tl_npanel,
              bool first, unsigned solvers, hipEvent_t* ev);
void bak_final(hipStream_t st, BaWin* wins, const BaIo* io, int nwin, int max_kf, int max_pt, int max_edge);

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

static int ba_solve_batch_impl(slamit_ba* h, int nwin, const slamit_ba_problem* probs, const slamit_ba_opts* opts, slamit_ba_result* results);

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

static int ba_solve_batch_impl(slamit_ba* h, int nwin, const slamit_ba_problem* probs, const slamit_ba_opts* opts,
                               slamit_ba_result* results) {
    if (!h || !probs || !opts || !results || nwin < 0) return slamit_fail(SLAMIT_ERR_ARG, "slamit_ba_solve_batch: bad argument");
    if (nwin > h->max_batch) return slamit_fail(SLAMIT_ERR_CAPACITY, "slamit_ba_solve_batch: nwin > max_batch");
    if (nwin == 0) return SLAMIT_OK;
    SLAMIT_USE_DEVICE(h->device);
    hipStream_t st = h->stream;
    const auto tclk = []() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t_in = tclk();
    double t_val = 0, t_prep = 0, t_queue = 0, t_loop = 0;
    // ---- validate ----
    int mk = 1, mp = 1, me = 1, Npad = BA_TILE, Npad_ldlt = BA_TILE;
    for (int b = 0; b < nwin; ++b) {
        const slamit_ba_problem& P = probs[b];
        if (P.n_kf < 1 || P.n_pt < 0 || P.n_edge < 0 || P.n_kf > h->max_kf || P.n_pt > h->max_pt || P.n_edge > h->max_edge)
            return slamit_fail(SLAMIT_ERR_CAPACITY, "slamit_ba_solve_batch: window exceeds the handle's capacity");
        if (!P.kf_pose || !P.kf_fixed || !P.kf_intr || (P.n_pt && !P.pt_xyz) ||
            (P.n_edge && (!P.edge_kf || !P.edge_pt || !P.edge_uv || !P.edge_inv_sigma2)))
            return slamit_fail(SLAMIT_ERR_ARG, "slamit_ba_solve_batch: null input array");
        int nfree = 0;
        for (int k = 0; k < P.n_kf; ++k) nfree += P.kf_fixed[k] ? 0 : 1;
        if (nfree > h->max_free_kf)
            return slamit_fail(SLAMIT_ERR_CAPACITY, "slamit_ba_solve_batch: window has more free keyframes than the handle's max_free_kf");
        if (P.edge_ur && !P.kf_bf)
            return slamit_fail(SLAMIT_ERR_ARG, "slamit_ba_solve_batch: stereo observations (edge_ur) without the keyframes' bf (kf_bf)");
        if (!results[b].kf_pose || (P.n_pt && !results[b].pt_xyz))
            return slamit_fail(SLAMIT_ERR_ARG, "slamit_ba_solve_batch: null output array");
        mk = std::max(mk, P.n_kf); mp = std::max(mp, P.n_pt); me = std::max(me, P.n_edge);
    }
    // (the edges' indices are checked by the threads that prepare the windows, before anything is packed)
    t_val = tclk();
    // ---- one pinned block: [inputs of window 0 | inputs of window 1 | ...][outputs ...][2 x nwin LM states] ----
    std::vector<size_t> in_off(nwin), out_off(nwin), side_w(nwin);
    std::vector<IoLayout> dio(nwin);   // device addresses inside the slabs
    size_t pin_need = 0;
    for (int b = 0; b < nwin; ++b) {
        side_w[b] = ba_io_side_words(probs[b]);
        dio[b] = carve_io(h->d_slab + (size_t)b * h->win_bytes, probs[b].n_kf, probs[b].n_pt, probs[b].n_edge, probs[b].edge_ur != nullptr, side_w[b]);
        in_off[b] = pin_need; pin_need += dio[b].in_bytes;
    }
    for (int b = 0; b < nwin; ++b) { out_off[b] = pin_need; pin_need += dio[b].bytes - dio[b].out_off; }
    const size_t st_off = ba_rup(pin_need, 256);
    pin_need = st_off + 2 * sizeof(BaState) * (size_t)nwin;
    if (pin_need > h->pin_bytes) {
        HIP_TRY(hipStreamSynchronize(st));
        if (h->h_pin) hipHostFree(h->h_pin);
        h->h_pin = nullptr; h->pin_bytes = 0;
        HIP_TRY(hipHostMalloc((void**)&h->h_pin, pin_need + pin_need / 4, hipHostMallocDefault));
        h->pin_bytes = pin_need + pin_need / 4;
    }
    std::vector<BaWin> wins(nwin);
    std::vector<BaIo> io(nwin);
    std::vector<BaWindowPlan> plans(nwin);
    const BaPlanLimits lim{h->Npad_max, nwin, h->sw.ba_keep_order, h->sw.ba_no_sf, h->sw.ba_no_band, h->sw.ba_sf_cap};
    // per-window preparation (the plan, CSR lists, packing into the pinned block) is host work of ~10 ns per edge: windows
    // are independent, so a batch is prepared by a few host threads; the copies are queued afterwards, in order
    std::atomic<bool> bad_index(false);
    auto prepare = [&](int b) {
        const slamit_ba_problem& P = probs[b];
        BaWin& w = wins[b];
        memset(&w, 0, sizeof(w));
        if (!ba_plan_window(P, lim, w, plans[b])) { bad_index = true; return; }
        ba_pack_inputs(P, plans[b], carve_io(h->h_pin + in_off[b], P.n_kf, P.n_pt, P.n_edge, P.edge_ur != nullptr, side_w[b]));   // the device's packing, in the pinned block
        carve_work(h->d_slab + (size_t)b * h->win_bytes + h->io_cap, w, h->max_kf, h->max_pt, h->max_edge, h->Npad_max, h->Kpad_max, h->n_part, h->max_free_kf);
        const IoLayout& D = dio[b];
        w.side = D.side;   // (null unless the window's structure outgrows BaWin's inline arrays)
        w.intr = D.intr; w.pose_col = D.pose_col; w.e_kf = D.e_kf; w.e_pt = D.e_pt; w.e_uv = D.e_uv; w.e_w = D.e_w;
        w.pt_edges = D.pt_edges; w.kf_edges = D.kf_edges; w.pt_ptr = D.pt_ptr; w.kf_ptr = D.kf_ptr;
        w.e_ur = D.e_ur; w.bf = D.bf;
        io[b].in_pose = D.in_pose; io[b].in_pt = D.in_pt; io[b].out_pose = D.out_pose; io[b].out_pt = D.out_pt;
        io[b].out_chi2 = D.out_chi2; io[b].out_flag = D.out_flag; io[b].out_out1 = D.out_out1; io[b].out_state = D.out_state;
        w.n_part = h->n_part;
        w.huber_delta = opts->huber_delta; w.chi2_gate = opts->chi2_gate;
        // stereo observations (EdgeStereoSE3ProjectXYZ): three residual rows per edge in this window, own Huber width and gate
        w.huber_delta_s = opts->huber_delta_stereo > 0 ? opts->huber_delta_stereo : (double)(float)sqrt(7.815);   // Optimizer.cc:570
        w.chi2_gate_s = opts->chi2_gate_stereo > 0 ? opts->chi2_gate_stereo : 7.815;                           // Optimizer.cc:696, 740
        w.nrow = P.edge_ur ? 3 : 2;
        w.st = reinterpret_cast<BaState*>(h->d_wins) - (b + 1);
    };
    if (!for_each_window(nwin, true, prepare))
        return slamit_fail(SLAMIT_ERR_DEVICE, "slamit_ba_solve_batch: out of host memory while preparing the windows");
    if (bad_index) return slamit_fail(SLAMIT_ERR_ARG, "slamit_ba_solve_batch: edge index out of range");
    t_prep = tclk();
    unsigned solvers = 0;
    // the tiled solve's launches per panel step: {panel workgroups, update workgroups} for the largest need among its windows
    std::vector<int> tl_grid;
    for (int b = 0; b < nwin; ++b) {
        Npad = std::max(Npad, wins[b].Npad);
        solvers |= 1u << wins[b].solver;
        HIP_TRY(hipMemcpyAsync(h->d_slab + (size_t)b * h->win_bytes, h->h_pin + in_off[b], dio[b].in_bytes, hipMemcpyHostToDevice, st));
        if (wins[b].solver != BA_SOLVER_TILED) { Npad_ldlt = std::max(Npad_ldlt, wins[b].Npad); continue; }
        BaWin wh = wins[b];
        wh.side = plans[b].side.data();
        const int n = wh.nS, np = (n + 31) / 32;
        if ((int)tl_grid.size() < 2 * np) tl_grid.resize(2 * np, 0);
        for (int i = 0; i < np; ++i) {
            const int base = std::min(32 * i + 32, n), below = std::max(ba_panel_hi(wh, i) + 1 - base, 0);
            tl_grid[2 * i] = std::max(tl_grid[2 * i], (below + 1 + BA_TL_CHUNK - 1) / BA_TL_CHUNK);
            tl_grid[2 * i + 1] = std::max(tl_grid[2 * i + 1], ldlt_tiled_ntiles(below));
        }
    }
    HIP_TRY(hipMemcpyAsync(h->d_wins, wins.data(), sizeof(BaWin) * nwin, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(h->d_io, io.data(), sizeof(BaIo) * nwin, hipMemcpyHostToDevice, st));
    bak_import(st, h->d_wins, h->d_io, mk, mp, me, Npad, nwin);   // also zeroes the Schur operands' ranges and the LM states

    // ---- two-stage schedule (Optimizer.cc:659-707) ----
    // LM trial slots are enqueued in chunks; the windows' states come back through the pinned block one chunk LATE (the
    // next chunk is already queued when the host looks at the previous one: no bubble between chunks), and *stop is polled
    // before every chunk like SparseOptimizer::terminate() (sparse_optimizer.cpp:376) is before every iteration.  Slots of
    // a finished stage return at once, but a slot queued in vain still costs its eleven launches (~30 us): the first chunk
    // of a stage is the number of trials the stage cannot do without (one per iteration in the robust stage; three in the
    // final one, whose "no progress three times" rule can end it that early), the chunks after it are single slots.
    // (Chunks of two throughout queued 20 slots for the 14 trials of a window-8 solve.)
    t_queue = tclk();
    BaState* hs[2] = {reinterpret_cast<BaState*>(h->h_pin + st_off), reinterpret_cast<BaState*>(h->h_pin + st_off) + nwin};
    bool stopped = opts->stop && *opts->stop;  // :655-657
    size_t pev_used = 0;   // profiling solves: six events per queued slot
    auto slot_events = [&]() -> hipEvent_t* {
        if (!h->prof) return nullptr;
        while (h->pev.size() < pev_used + 6) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) return nullptr;
            h->pev.push_back(e);
        }
        pev_used += 6;
        return h->pev.data() + pev_used - 6;
    };
    for (int stage = 0; stage < 2 && !stopped; ++stage) {
        const int its = stage == 0 ? opts->its_robust : opts->its_final;
        bak_stage_begin(st, h->d_wins, nwin, me, stage, its, stage == 0 ? 1 : 0, stage == 1);
        int budget = its * 10 + 1;  // at most 10 LM trials per iteration
        int cur = 0, pending = -1;
        bool all_done = false, first = true;
        while (!all_done) {
            if (opts->stop && *opts->stop) { stopped = true; break; }
            if (budget > 0) {
                const int want = first ? std::max(1, std::min(stage == 0 ? its : 3, std::min(its, 4))) : 1;
                const int nslots = std::min(want, budget);
                const bool was_first = first;
                first = false;
                for (int sl = 0; sl < nslots; ++sl)
                    bak_slot(st, h->d_wins, nwin, mk, mp, me, Npad, Npad_ldlt, tl_grid.data(), (int)tl_grid.size() / 2, was_first && sl == 0, solvers, slot_events());
                budget -= nslots;
                HIP_TRY(hipMemcpyAsync(hs[cur], reinterpret_cast<BaState*>(h->d_wins) - nwin, sizeof(BaState) * nwin, hipMemcpyDeviceToHost, st));   // (reverse order: only `done` of all is read)
                HIP_TRY(hipEventRecord(h->ev[cur], st));
            }
            if (pending >= 0) {
                HIP_TRY(hipEventSynchronize(h->ev[pending]));
                all_done = true;
                for (int b = 0; b < nwin; ++b) all_done = all_done && hs[pending][b].done;
            }
            if (budget <= 0 && pending == cur) break;   // nothing new was queued: the last read-back has been looked at
            pending = cur;
            if (budget > 0) cur ^= 1;
        }
        HIP_TRY(hipGetLastError());
    }
    t_loop = tclk();
    // ---- results: one copy per window out of its output section ----
    bak_final(st, h->d_wins, h->d_io, nwin, mk, mp, me);
    for (int b = 0; b < nwin; ++b)
        HIP_TRY(hipMemcpyAsync(h->h_pin + out_off[b], h->d_slab + (size_t)b * h->win_bytes + dio[b].out_off, dio[b].bytes - dio[b].out_off,
                               hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (h->prof) {
        slamit_ba_profile_out& O = h->prof_last;
        memset(&O, 0, sizeof(O));
        O.nwin = nwin; O.slots = (int32_t)(pev_used / 6);
        for (size_t s0 = 0; s0 + 6 <= pev_used; s0 += 6)
            for (int ph = 0; ph < SLAMIT_BA_PHASES; ++ph) {
                float ms = 0.f;
                if (hipEventElapsedTime(&ms, h->pev[s0 + ph], h->pev[s0 + ph + 1]) == hipSuccess) O.phase_ms[ph] += ms;
            }
        for (int b = 0; b < nwin; ++b) O.schur_exec_mflop += plans[b].exec_mflop;
    }
    auto unpack = [&](int b) {
        const slamit_ba_problem& P = probs[b];
        // the output section as the host sees it: same carve, shifted so that its output part starts at out_off[b]
        const IoLayout H = carve_io(h->h_pin + out_off[b] - dio[b].out_off, P.n_kf, P.n_pt, P.n_edge, P.edge_ur != nullptr, side_w[b]);
        ba_unpack_outputs(P, plans[b], H, results[b]);
        const BaState& S0 = *H.out_state;
        if (b == 0 && h->sw.ba_diag_waves) fprintf(stderr, "[ba diag] busy cycles of waves 0..7: %llu %llu %llu %llu %llu %llu %llu %llu\n", S0.dbg[0], S0.dbg[1], S0.dbg[2], S0.dbg[3], S0.dbg[4], S0.dbg[5], S0.dbg[6], S0.dbg[7]);
        if (b == 0 && h->sw.ba_diag) {  // diagnostic builds only: in-kernel clock and phases of the last LDLt launch
            fprintf(stderr, "[ba diag] ldlt shader cycles %llu, realtime ticks (100 MHz) %llu -> %.0f MHz, %.1f us\n",
                    S0.dbg[2] - S0.dbg[0], S0.dbg[3] - S0.dbg[1],
                    100.0 * (double)(S0.dbg[2] - S0.dbg[0]) / (double)(S0.dbg[3] - S0.dbg[1] + 1), (double)(S0.dbg[3] - S0.dbg[1]) / 100.0);
            fprintf(stderr, "[ba diag] ldlt phase cycles: load %llu factor %llu rows %llu writeback / wave-0 busy %llu trailing / rhs-wave busy %llu backsub %llu, pivot-wave busy %llu\n",
                    S0.dbg[4] >> 32, S0.dbg[4] & 0xffffffffull, S0.dbg[5] >> 32, S0.dbg[5] & 0xffffffffull, S0.dbg[6] >> 32, S0.dbg[6] & 0xffffffffull, S0.dbg[7]);
        }
    };
    for_each_window(nwin, nwin >= 4, unpack);   // by the host threads that prepared the windows (nothing in it throws)
    if (h->sw.ba_timing) {   // diagnostic: host phases of the call on stderr
        const double t_out = tclk();
        fprintf(stderr, "[ba timing] %d windows: validate %.3f | prepare + pack %.3f | queue uploads %.3f | LM loop %.3f | download + unpack %.3f ms\n",
                nwin, t_val - t_in, t_prep - t_val, t_queue - t_prep, t_loop - t_queue, t_out - t_loop);
    }
    return SLAMIT_OK;
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
