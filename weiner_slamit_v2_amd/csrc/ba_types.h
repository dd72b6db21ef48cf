// ba_types.h — host/device shared layout of one local-BA window in HBM, and the rules the host's planning (ba_plan.cc) and the
// kernels (ba_kernels.hip) both apply to it.  Plain C++ outside a HIP compile.
#ifndef SLAMIT_BA_TYPES_H
#define SLAMIT_BA_TYPES_H

#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define BA_HD __host__ __device__
#else
#define BA_HD
#endif

#define BA_MAX_ITS 32       // == SLAMIT_BA_MAX_ITS
#define BA_TILE 64          // Schur macro tile (rows/cols of S per workgroup)
#define BA_KC 32            // k-depth of one staged slab
#define BA_SPLITS 16        // split-K factor of the Schur GEMM
#define BA_MAX_TILES 10     // 64-row tiles of the reduced system (slamit_ba_create refuses larger handles)
#define BA_MAX_PANELS 20    // 32-column LDLt panels
#define BA_JAC_MONO 21      // doubles per edge record: A (2x3) B (2x6) wO r0 r1
#define BA_JAC_STEREO 31    // ... of a window with stereo observations: A (3x3) B (3x6) wO r0 r1 r2 (a monocular edge's third row is zero)
#define BA_SF_MAXG 256      // groups of k slabs of the floating-window Schur product (BaWin::sf_*)
#define BA_SF_ROWS 63       // matrix rows one window holds (row 64 of its B operand is the right-hand side's row)
#define BA_SOLVER_BAND 0      // narrow row envelope: block LDLt inside LDS (k_ldlt_band)
#define BA_SOLVER_BLOCKED 1   // any other structure: 32-column panels through L2 (k_ldlt_blocked)
#define BA_SOLVER_TILED 2     // a reduced system too large for k_ldlt_blocked's LDS panel: one launch per panel step (k_ldlt_tiled_*)
#define BA_BLOCKED_MAX_NPAD 512   // largest Npad whose rows below a panel k_ldlt_blocked keeps in LDS (bak_ldlt_smem within 160 KiB)
#define BA_MAX_FREE_KF 341        // == SLAMIT_BA_MAX_FREE_KF: free keyframes of a handle (slamit_ba_create_ex); Npad 2048
#define BA_NPAD_CEIL 2048         // rup(6 * BA_MAX_FREE_KF + 1, BA_TILE)
#define BA_TL_CHUNK 128           // rows below a panel per workgroup of k_ldlt_tiled_panel
#define BA_BAND_MAX 59        // widest half bandwidth k_ldlt_band takes: the reachable rows k + 4 .. k + 3 + bw stay within five block rows of the pivot's
#define LD_BAND_LDS (150 * 1024)     // dynamic LDS k_ldlt_band may use (bak_ldlt_smem requests at least this much when it fits)

// The banded solve's LDS image (ba_kernels.hip, banded path).  Row stride EVEN: a column of the band, A(c, k) for c = k + 1, k + 2, .., is a walk
// of RS - 1 doubles per row, and an odd number of doubles per step spreads 32 lanes over 32 different bank pairs (with RS = 49 they all fell on two).
BA_HD inline int ldlt_band_rs(int bw) { return (bw + 5) & ~1; }
BA_HD inline int ldlt_band_ylen(int n) { return (n + 9) & ~1; }
BA_HD inline size_t ldlt_band_bytes(int n, int bw) {
    return sizeof(double) * ((size_t)(n + 1) * ldlt_band_rs(bw) + ldlt_band_ylen(n) + 16 * (size_t)((n + 3) / 4 + 1));
}
BA_HD inline bool ldlt_band_ok(int n, int bw) { return n > 0 && bw >= 8 && bw <= BA_BAND_MAX && ldlt_band_bytes(n, bw) <= LD_BAND_LDS; }

// the reduced solve a window takes: its structure decides (`no_band`: SLAMIT_BA_NO_BAND, every window takes the blocked kernel)
// A system of more than BA_BLOCKED_MAX_NPAD padded rows takes the tiled solve whatever its band: the LDS-resident kernels launch with
// bak_ldlt_smem of their windows' Npad, which only fits a CU up to that size (ldlt_band_ok alone admits narrow bands of ~900 rows).
inline int bak_solver_kind(int n, int band, bool no_band) {
    if ((n + 1 + BA_TILE - 1) / BA_TILE * BA_TILE > BA_BLOCKED_MAX_NPAD) return BA_SOLVER_TILED;
    return !no_band && ldlt_band_ok(n, band) ? BA_SOLVER_BAND : BA_SOLVER_BLOCKED;
}

// split-K of the tiled Schur product (gridDim.y of its launch): a batch brings its own parallelism (64 windows: 2 / 4 / 8 / 16 splits -> 47.8k /
// 49.7k / 52.8k / 50.0k LM it/s)
inline int bak_nsplit(int nwin) { return nwin >= 16 ? 8 : BA_SPLITS; }

// LM control block of one window (device resident; the host only reads it back between chunks
// of enqueued trial slots).  Mirrors the locals of OptimizationAlgorithmLevenberg::solve
// (g2o/core/optimization_algorithm_levenberg.cpp:61-164).
struct BaState {
    int32_t done;            // stage finished (iterations exhausted / Terminate / nothing active)
    int32_t need_linearize;  // next slot starts a new iteration: Jacobians + normal equations
    int32_t it;              // iteration index inside the stage
    int32_t max_it;
    int32_t qmax;            // LM trials used so far in this iteration
    int32_t nBad;
    int32_t robust;          // Huber kernel on (stage 1) / off (stage 2)
    int32_t ok2;             // last factorisation succeeded
    int32_t n_active;        // active edges of the stage
    int32_t stage;
    double lambda, ni;
    double currentChi, iniChi, tempChi;
    unsigned long long maxdiag_bits;  // max |H_jj| as ordered bits (non-negative doubles)
    // per-stage statistics (slamit_ba_stats)
    int32_t n_its[2];
    double chi2[2][BA_MAX_ITS];
    double lam[2][BA_MAX_ITS];
    int32_t trials[2][BA_MAX_ITS];
    double chi2_init[2];
    unsigned long long dbg[8];  // diagnostic stamps (s_memtime / s_memrealtime); written only when BA_DIAG_STAMPS is defined
};

// One window.  All pointers are device addresses inside the handle's slabs.  In the kernels they carry SLAMIT_GLOBAL
// (slamit_internal.h).  Only the kernel translation unit asks for it, by defining BA_GLOBAL_POINTERS after including that header:
// ba_api.hip fills the struct from plain pointers in code the device pass parses too, and ba_plan.cc is plain C++.
#if defined(BA_GLOBAL_POINTERS)
#define BA_G SLAMIT_GLOBAL
#else
#define BA_G
#endif
struct BaWin {
    int32_t n_kf, n_pt, n_edge, n_free;
    int32_t nS;        // 6 * n_free
    int32_t Npad;      // rows/cols of the padded reduced system, multiple of BA_TILE, >= nS + 1
    int32_t Kpad;      // padded k extent (3 * n_pt rounded up to BA_KC * BA_SPLITS)
    int32_t n_part;    // partial-sum slots of the chi2 reduction
    double huber_delta, chi2_gate;
    double huber_delta_s, chi2_gate_s;   // stereo edges (Optimizer.cc:570, :696)
    int32_t nrow;      // residual rows per edge record: 2 (every edge monocular) or 3 (the window has stereo observations)
    int32_t pad0;
    // Structure of the window (host, ba_plan.cc), conservative for both stages.  Points are stored sorted by the first
    // free keyframe that observes them, so the non-zeros of a 64-row tile of the Schur operand GA sit in ONE k range, and the reduced
    // system has a row envelope (first coupled column per pose) that LDLt without pivoting never leaves.
    int32_t tile_alo[BA_MAX_TILES], tile_ahi[BA_MAX_TILES];   // k range (multiples of BA_KC) of GA's rows 64 t .. 64 t + 63
    int32_t tile_blo[BA_MAX_TILES], tile_bhi[BA_MAX_TILES];   // ... as the product's B operand (the tile that holds row nS, the right-hand side's row, spans every point)
    int16_t panel_hi[BA_MAX_PANELS];   // last matrix row with an entry in the 32 columns of LDLt panel i (>= the panel's last row)
    int16_t back_lo[BA_MAX_PANELS];    // first column any row of panel i's 32 rows reaches (back-substitution)
    int32_t band;      // half bandwidth of the reduced system's row envelope: max over rows r of r - first column of r (nS - 1: full)
    int32_t solver;    // which reduced solve takes the window (host, from nS and band): BA_SOLVER_*; one launch per kind present in a batch
    // Schur product over FLOATING row windows (host, ba_plan.cc; sf_groups == 0: 64 x 64 tile pairs over k ranges as above).  The points are sorted
    // by their first observing keyframe, so the rows with non-zeros in one k slab of 32 (about eleven points) are a short run -- 48 rows
    // when every point is seen by eight consecutive keyframes.  Consecutive slabs whose rows fit ONE run of BA_SF_ROWS rows form a group:
    // one workgroup multiplies GA(rows, slabs) GA(rows + the right-hand side's row, slabs)^T into a 64 x 64 partial tile, and
    // k_schur_reduce adds, for an entry (r, c), the tiles of the groups whose window holds both rows -- a contiguous run of groups,
    // in group order.  Aligned 64 x 64 tile pairs multiply 3.8 x as many zeros on such a window.
    int32_t sf_groups, pad1;
    int16_t sf_row[BA_SF_MAXG];                       // first matrix row of group g's window
    int16_t sf_k0[BA_SF_MAXG], sf_k1[BA_SF_MAXG];     // its slabs [k0, k1), in units of BA_KC
    int16_t sf_glo[BA_MAX_TILES * BA_TILE], sf_ghi[BA_MAX_TILES * BA_TILE];   // per matrix row: the groups whose window holds it (glo > ghi: none)
    // vertices
    BA_G double* pose;      // n_kf x 7: q(x,y,z,w), t
    BA_G double* pose_bak;
    BA_G double* intr;      // n_kf x 4
    BA_G int32_t* pose_col; // n_kf: column block among free poses or -1
    BA_G double* pt;        // n_pt x 3
    BA_G double* pt_bak;
    // edges (caller order) + CSR by point and by free pose
    BA_G int32_t* e_kf; BA_G int32_t* e_pt;
    BA_G double* e_uv;      // n_edge x 2
    BA_G double* e_w;       // n_edge
    BA_G double* e_ur;      // n_edge: right-image column, < 0 on a monocular edge (stereo windows only)
    BA_G double* bf;        // n_kf: baseline x fx (stereo windows only)
    BA_G uint8_t* e_active;
    BA_G uint8_t* e_out1;   // stage-1 outlier flag
    BA_G double* e_chi2;    // chi2 of the last evaluated trial
    BA_G double* e_jac;     // n_edge x 21: A(2x3) B(2x6) wO r0 r1  (x 31 in a stereo window: BA_JAC_STEREO)
    BA_G int32_t* pt_ptr; BA_G int32_t* pt_edges;     // CSR: edges of each point
    BA_G int32_t* kf_ptr; BA_G int32_t* kf_edges;     // CSR: edges of each keyframe
    // normal equations
    BA_G double* Hll;       // n_pt x 6 (xx xy xz yy yz zz)
    BA_G double* bl;        // n_pt x 3
    BA_G double* Dinv;      // n_pt x 6
    BA_G double* Hpp;       // n_free x 36
    BA_G double* bp;        // n_free x 6
    BA_G double* GA;        // Npad x Kpad : the Schur operand G = Hpl Ci^T scattered (row = pose dof, col = 3*pt + j; Ci = inverse Cholesky factor of Hll + lambda I,
                            // ba_kernels.hip point_chol): S = Hpp - G G^T; row nS holds Ci bl, so that G (row nS)^T is the right-hand side's coefficient
    BA_G double* part;      // BA_SPLITS x Npad x Npad partial products
    BA_G double* S;         // Npad x Npad reduced system (symmetric, full)
    BA_G double* Sb;        // (Npad + 1) x 64: the same system as the banded solve's LDS image (rows of ldlt_band_rs(band) doubles; k_schur_reduce
                            // writes the in-band entries, the zeros around them are laid once per solve by k_import); a window of the tiled solve
                            // keeps its factored 32 x 32 diagonal blocks there instead, panel i at i x 1024 (k_ldlt_tiled_panel)
    BA_G double* rhs;       // Npad : b_schur in, x_pose out
    BA_G double* x_l;       // n_pt x 3 landmark increments
    BA_G double* chi_part;  // n_part partial robust-cost sums
    BA_G double* scale_part;// n_part partial sums of x(lambda x + b) over landmarks
    BA_G BaState* st;
    // Structure of a window beyond the inline arrays above (more than BA_MAX_TILES row tiles or BA_MAX_PANELS panels; null otherwise): a side
    // table in the window's io section, int32 [tile_alo T | tile_ahi T | tile_blo T | tile_bhi T | panel_hi P | back_lo P] with T = Npad / BA_TILE,
    // P = ba_npanel(nS) -- every entry, the inline ones included.  Read through the accessors below.
    BA_G const int32_t* side;
};

// Where one window's inputs and outputs sit in its slab (device addresses): the host fills / reads them with ONE copy each.
struct BaIo {
    const double* in_pose;   // n_kf x 12 (R|t)
    const double* in_pt;     // n_pt x 3, device point order
    double* out_pose;        // n_kf x 12
    double* out_pt;          // n_pt x 3, device point order
    double* out_chi2;        // n_edge
    uint8_t* out_flag;       // n_edge
    uint8_t* out_out1;       // n_edge
    BaState* out_state;
};

// the side table (BaWin::side): its length in int32, and whether a window needs one
BA_HD inline int ba_npanel(int nS) { return nS > 0 ? (nS + 31) / 32 : 1; }
BA_HD inline size_t ba_side_words(int Npad, int nS) { return 4 * (size_t)(Npad / BA_TILE) + 2 * (size_t)ba_npanel(nS); }
BA_HD inline bool ba_side_needed(int Npad, int nS) { return Npad / BA_TILE > BA_MAX_TILES || ba_npanel(nS) > BA_MAX_PANELS; }

// One accessor per structural array: the inline entry where there is one, else the side table's.  Kernels and host use these.
BA_HD inline int ba_tile_alo(const BaWin& W, int t) { return t < BA_MAX_TILES ? W.tile_alo[t] : W.side[t]; }
BA_HD inline int ba_tile_ahi(const BaWin& W, int t) { return t < BA_MAX_TILES ? W.tile_ahi[t] : W.side[W.Npad / BA_TILE + t]; }
BA_HD inline int ba_tile_blo(const BaWin& W, int t) { return t < BA_MAX_TILES ? W.tile_blo[t] : W.side[2 * (W.Npad / BA_TILE) + t]; }
BA_HD inline int ba_tile_bhi(const BaWin& W, int t) { return t < BA_MAX_TILES ? W.tile_bhi[t] : W.side[3 * (W.Npad / BA_TILE) + t]; }
BA_HD inline int ba_panel_hi(const BaWin& W, int i) { return i < BA_MAX_PANELS ? W.panel_hi[i] : W.side[4 * (W.Npad / BA_TILE) + i]; }
BA_HD inline int ba_back_lo(const BaWin& W, int i) {
    return i < BA_MAX_PANELS ? W.back_lo[i] : W.side[4 * (W.Npad / BA_TILE) + ba_npanel(W.nS) + i];
}

// k_ldlt_tiled_update's workgroups for panel rows `below` (+ the right-hand side's row): the lower 64 x 64 tiles (rt, ct), ct <= min(rt, CT - 1)
BA_HD inline int ldlt_tiled_ntiles(int below) {
    const int RT = (below + 1 + BA_TILE - 1) / BA_TILE, CT = (below + BA_TILE - 1) / BA_TILE;
    int nt = 0;
    for (int rt = 0; rt < RT; ++rt) nt += rt + 1 < CT ? rt + 1 : CT;
    return nt;
}

// does the reduced system need tile pair (I, J), I <= J, of the product?  Not when the two row tiles share no k range (the block
// is zero: k_schur_reduce writes the zeros itself), and not when the banded solver takes the window and the whole tile lies
// outside the band (nobody reads it) -- except for the tile column that holds the right-hand side (row nS of the operand)
BA_HD inline bool schur_tile_needed(const BaWin& W, int I, int J) {
    const int alo = ba_tile_alo(W, I), blo = ba_tile_blo(W, J), ahi = ba_tile_ahi(W, I), bhi = ba_tile_bhi(W, J);
    const int klo = alo > blo ? alo : blo;
    const int khi = ahi < bhi ? ahi : bhi;
    if (klo >= khi) return false;
    if (W.solver == BA_SOLVER_BAND && BA_TILE * J - (BA_TILE * I + BA_TILE - 1) > W.band && W.nS / BA_TILE != J) return false;
    return true;
}

#endif
