// ba_plan.h — host-side planning of one local-BA window: how it is laid out on the device (column and point order, the Schur
// product's k ranges and floating-window groups, the LDLt row envelope and solver), and how its inputs and outputs are packed; and of a
// batch of them (BaBatchPlan: the windows' places in the slabs and the pinned block, the launch maxima, the checks that refuse a batch).
// Plain C++17 (no HIP): the solve (ba_api.hip) and the CPU tests of the plan (tests/test_ba_plan.py, test_ba_batch_plan.py) both build it.
#ifndef SLAMIT_BA_PLAN_H
#define SLAMIT_BA_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/slamit.h"
#include "ba_types.h"

inline size_t ba_rup(size_t v, size_t a) { return (v + a - 1) / a * a; }   // v rounded up to a multiple of a

// carve arrays out of a block; `base` may be null (size query)
struct Carver {
    uint8_t* base;
    size_t off;
    template <typename T>
    T* take(size_t n) {
        off = ba_rup(off, 256);
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += sizeof(T) * n;
        return p;
    }
};

// The io section of a window: the arrays the host writes (packed for the ACTUAL sizes of the problem, so one copy moves
// exactly what is needed) followed by the arrays it reads back.
struct IoLayout {
    // inputs
    double* in_pose; double* intr; int32_t* pose_col; double* in_pt; int32_t* e_kf; int32_t* e_pt; double* e_uv; double* e_w;
    double* e_ur; double* bf;   // stereo windows only (slamit_ba_problem::edge_ur / kf_bf)
    int32_t* pt_edges; int32_t* kf_edges; int32_t* pt_ptr; int32_t* kf_ptr;
    int32_t* side;   // the window's structure beyond BaWin's inline arrays (BaWin::side), null when it needs none
    size_t in_bytes;
    // outputs
    size_t out_off;
    double* out_pose; double* out_pt; double* out_chi2; uint8_t* out_flag; uint8_t* out_out1; BaState* out_state;
    size_t bytes;
};

// `side_words`: length of the window's side table (ba_side_words; 0: none), the last of the inputs
IoLayout carve_io(uint8_t* base, int n_kf, int n_pt, int n_edge, bool stereo, size_t side_words = 0);
// side_words for window P: 0 unless its structure outgrows BaWin's inline arrays
size_t ba_io_side_words(const slamit_ba_problem& P);
// the workspace of a window (sized for the handle's maxima; the pose blocks Hpp / bp for max_free_kf keyframes, < 0: max_kf); returns bytes used
size_t carve_work(uint8_t* base, BaWin& w, int max_kf, int max_pt, int max_edge, int Npad, int Kpad, int n_part, int max_free_kf = -1);

// What steers the plan besides the window itself: the handle's reduced-system capacity, the batch size, and the four BA switches
// (SlamitSwitches::ba_keep_order, ba_no_sf, ba_no_band, ba_sf_cap).
struct BaPlanLimits {
    int Npad_max;
    int nwin;
    bool keep_order, no_sf, no_band;
    int sf_cap;
};

// The plan's host-side results besides the BaWin fields.
struct BaWindowPlan {
    std::vector<int32_t> col;       // n_kf: column block of each keyframe among the free ones, -1 if fixed (after any renumbering)
    std::vector<int32_t> new2old;   // device point index -> caller's point index
    std::vector<int32_t> old2new;
    double exec_mflop = 0;          // what the Schur product multiplies per trial (slamit_ba_profile_out)
    std::vector<int32_t> side;      // every structural entry in BaWin::side's layout (ba_side_words), whether or not the window needs the table
};

// Plans window P.  Fills the structural fields of `w` (n_*, nS, Npad, Kpad, tile_*, panel_hi, back_lo, band, solver, sf_*), which
// comes in zeroed, and `plan`; w.side is left null (the caller points it at the device copy of plan.side when ba_side_needed).  Returns false, with nothing planned, when an edge names a keyframe or point outside the window.
bool ba_plan_window(const slamit_ba_problem& P, const BaPlanLimits& L, BaWin& w, BaWindowPlan& plan);

// The window's inputs into the input part of H (carve_io of P's sizes): poses, intrinsics, the column table, points in device order,
// the edges, the CSR lists by point and by keyframe (counting sort, caller order kept inside each list), and the side table when H has one.
void ba_pack_inputs(const slamit_ba_problem& P, const BaWindowPlan& plan, const IoLayout& H);

// The output part of H back to the caller: poses, points in the caller's order, the edge arrays R asks for, and R.stats from the LM state.
void ba_unpack_outputs(const slamit_ba_problem& P, const BaWindowPlan& plan, const IoLayout& H, slamit_ba_result& R);

// ---- a batch of windows ----

// The capacities of a handle that a batch is checked against.
struct BaCaps {
    int max_kf, max_free_kf, max_pt, max_edge, max_batch;
};

// A refused batch: the code slamit_ba_solve_batch returns and the text slamit_last_error gives (code SLAMIT_OK, msg null: accepted).
struct BaRefusal {
    int code;
    const char* msg;
};

// Every check of a batch that does not touch the device: the arrays are there, the batch and each window fit the handle, stereo
// observations come with their bf.  (The edges' indices are checked by ba_plan_window, before anything is packed.)
BaRefusal ba_batch_check(const slamit_ba_problem* probs, const slamit_ba_result* results, int nwin, const BaCaps& caps);

// What a batch needs beyond its windows: where each window sits in the device slabs and in the pinned block
//   [inputs of window 0 | inputs of window 1 | ...][outputs ...][2 x nwin LM states, on a 256-byte boundary]
// and the maxima its launches are sized by (the grids themselves: ba_kernels.hip).
struct BaBatchPlan {
    int nwin;
    // ba_batch_layout
    std::vector<size_t> side_w;     // per window: ba_io_side_words
    std::vector<IoLayout> dio;      // its io section at its device address
    std::vector<size_t> in_off;     // its packed inputs in the pinned block (dio.in_bytes of them)
    std::vector<size_t> out_off;    // its outputs there (dio.bytes - dio.out_off)
    size_t st_off;                  // the two buffers of LM states
    size_t pin_need;                // bytes of the pinned block
    int mk, mp, me;                 // largest n_kf, n_pt, n_edge (>= 1)
    // ba_batch_launches
    int Npad;                       // largest reduced system (grids of the Schur product and its reduction)
    int Npad_ldlt;                  // largest among the windows of the LDS-resident solves (their dynamic LDS, <= BA_BLOCKED_MAX_NPAD)
    unsigned solvers;               // bit BA_SOLVER_* set when a window takes that reduced solve
    std::vector<int> tl_grid;       // per panel step of the tiled solve {k_ldlt_tiled_panel, k_ldlt_tiled_update} workgroups: the largest need among its windows
};

// Before the windows are planned.  `slab`: the device address of window 0's slab, one every `win_bytes` (null: sizes and offsets only).
void ba_batch_layout(const slamit_ba_problem* probs, int nwin, size_t win_bytes, uint8_t* slab, BaBatchPlan& B);
// After: from the planned windows and their host side tables (BaWindowPlan::side; wins[b].side itself may point anywhere).
void ba_batch_launches(const BaWin* wins, const BaWindowPlan* plans, BaBatchPlan& B);

#endif
