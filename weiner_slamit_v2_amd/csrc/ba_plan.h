// ba_plan.h — host-side planning of one local-BA window: how it is laid out on the device (column and point order, the Schur
// product's k ranges and floating-window groups, the LDLt row envelope and solver), and how its inputs and outputs are packed.
// Plain C++17 (no HIP): the solve (ba_api.hip) and the CPU test of the plan (tests/test_ba_plan.py) both build it.
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

#endif
