// ba_plan.cc — host-side planning of one local-BA window (ba_plan.h).  g2o's BlockSolver / SimplicialLDLT exploit the same sparsity on
// the CPU (block_solver.hpp:381-432, linear_solver_eigen.h:94-124).  Points are stored on the device sorted by the first free keyframe
// that observes them: the rows of the Schur operand GA that belong to a 64-row tile then have their non-zeros in one k range, the
// Schur product skips the rest, and the reduced system has a row envelope (first coupled column per pose) that LDLt without pivoting
// never leaves.
#include "ba_plan.h"

#include <limits.h>
#include <string.h>

#include <algorithm>

IoLayout carve_io(uint8_t* base, int n_kf, int n_pt, int n_edge, bool stereo, size_t side_words) {
    Carver c{base, 0};
    IoLayout L;
    L.e_ur = nullptr; L.bf = nullptr; L.side = nullptr;
    L.in_pose = c.take<double>(12 * (size_t)n_kf); L.intr = c.take<double>(4 * (size_t)n_kf); L.pose_col = c.take<int32_t>(n_kf);
    L.in_pt = c.take<double>(3 * (size_t)std::max(n_pt, 1));
    L.e_kf = c.take<int32_t>(std::max(n_edge, 1)); L.e_pt = c.take<int32_t>(std::max(n_edge, 1));
    L.e_uv = c.take<double>(2 * (size_t)std::max(n_edge, 1)); L.e_w = c.take<double>(std::max(n_edge, 1));
    L.pt_edges = c.take<int32_t>(std::max(n_edge, 1)); L.kf_edges = c.take<int32_t>(std::max(n_edge, 1));
    L.pt_ptr = c.take<int32_t>((size_t)n_pt + 1); L.kf_ptr = c.take<int32_t>((size_t)n_kf + 1);
    if (stereo) { L.e_ur = c.take<double>(std::max(n_edge, 1)); L.bf = c.take<double>(n_kf); }
    if (side_words) L.side = c.take<int32_t>(side_words);
    L.in_bytes = ba_rup(c.off, 256);
    c.off = L.in_bytes;
    L.out_off = c.off;
    L.out_pose = c.take<double>(12 * (size_t)n_kf); L.out_pt = c.take<double>(3 * (size_t)std::max(n_pt, 1));
    L.out_chi2 = c.take<double>(std::max(n_edge, 1)); L.out_flag = c.take<uint8_t>(std::max(n_edge, 1));
    L.out_out1 = c.take<uint8_t>(std::max(n_edge, 1)); L.out_state = c.take<BaState>(1);
    L.bytes = ba_rup(c.off, 4096);
    return L;
}

size_t ba_io_side_words(const slamit_ba_problem& P) {
    int nfree = 0;
    for (int k = 0; k < P.n_kf; ++k) nfree += P.kf_fixed[k] ? 0 : 1;
    const int nS = 6 * nfree, Npad = (int)ba_rup((size_t)nS + 1, BA_TILE);
    return ba_side_needed(Npad, nS) ? ba_side_words(Npad, nS) : 0;
}

size_t carve_work(uint8_t* base, BaWin& w, int max_kf, int max_pt, int max_edge, int Npad, int Kpad, int n_part, int max_free_kf) {
    if (max_free_kf < 0) max_free_kf = max_kf;
    Carver c{base, 0};
    w.pose = c.take<double>(7 * (size_t)max_kf); w.pose_bak = c.take<double>(7 * (size_t)max_kf);
    w.pt = c.take<double>(3 * (size_t)max_pt); w.pt_bak = c.take<double>(3 * (size_t)max_pt);
    w.e_active = c.take<uint8_t>(max_edge); w.e_out1 = c.take<uint8_t>(max_edge);
    w.e_chi2 = c.take<double>(max_edge); w.e_jac = c.take<double>(BA_JAC_STEREO * (size_t)max_edge);
    w.Hll = c.take<double>(6 * (size_t)max_pt); w.bl = c.take<double>(3 * (size_t)max_pt);
    w.Dinv = c.take<double>(6 * (size_t)max_pt);
    w.Hpp = c.take<double>(36 * (size_t)max_free_kf); w.bp = c.take<double>(6 * (size_t)max_free_kf + 8);
    w.GA = c.take<double>((size_t)Npad * Kpad);
    w.part = c.take<double>((size_t)BA_SPLITS * Npad * Npad);
    w.S = c.take<double>((size_t)Npad * Npad); w.Sb = c.take<double>(((size_t)Npad + 1) * 64); w.rhs = c.take<double>(Npad);
    w.x_l = c.take<double>(3 * (size_t)max_pt);
    w.chi_part = c.take<double>(n_part); w.scale_part = c.take<double>(n_part);
    return ba_rup(c.off, 4096);
}

namespace {

bool edges_valid(const slamit_ba_problem& P) {
    for (int e = 0; e < P.n_edge; ++e)
        if (P.edge_kf[e] < 0 || P.edge_kf[e] >= P.n_kf || P.edge_pt[e] < 0 || P.edge_pt[e] >= P.n_pt) return false;
    return true;
}

// column block of each keyframe among the free ones in the caller's order, -1 if fixed; returns their number
int free_columns(const slamit_ba_problem& P, std::vector<int32_t>& col) {
    col.resize(P.n_kf);
    int nfree = 0;
    for (int k = 0; k < P.n_kf; ++k) col[k] = P.kf_fixed[k] ? -1 : nfree++;
    return nfree;
}

// per point: the first and last free column it is seen from (INT32_MAX / -1: none), and (`seen_by`, when given) from how many free edges
void point_columns(const slamit_ba_problem& P, const std::vector<int32_t>& col, std::vector<int32_t>& minc, std::vector<int32_t>& maxc,
                   std::vector<int32_t>* seen_by) {
    minc.assign(P.n_pt, INT32_MAX); maxc.assign(P.n_pt, -1);
    if (seen_by) seen_by->assign(P.n_pt, 0);
    for (int e = 0; e < P.n_edge; ++e) {
        const int c = col[P.edge_kf[e]], p = P.edge_pt[e];
        if (c < 0) continue;
        minc[p] = std::min(minc[p], c); maxc[p] = std::max(maxc[p], c);
        if (seen_by) ++(*seen_by)[p];
    }
}

// Column order of the free keyframes in the reduced system.  The banded solve and the floating-window Schur product want keyframes that share
// points to be NEIGHBOURS in that order; a caller that lists its local window by co-visibility weight (Optimizer.cc:456-470 walks
// GetVectorCovisibleKeyFrames) instead of along the trajectory gives the same graph in a scattered order.  If a reverse Cuthill-McKee
// order of the co-visibility graph (free keyframes; an edge = a shared point) has a narrower band than the caller's, `col` is renumbered
// to it; g2o orders the same system by approximate minimum degree (linear_solver_eigen.h:77-92) -- any order gives the same solution up
// to rounding.  The caller's order is kept when the banded solve takes it as it is, or when no order is narrower (`keep_order`: always).
// `span` = the widest point of the caller's order (last - first column it is seen from), `complete` = some point is seen from every
// free keyframe (the graph is complete: no order is narrower): both come out of the pass over the edges the caller makes anyway, and
// decide without one of their own -- an order whose band the banded solve already takes (<= 9 keyframes) is kept as it is.
bool ba_order_columns(const slamit_ba_problem& P, int32_t* col, int nfree, int span, bool complete, bool keep_order) {
    if (nfree < 3 || complete || 6 * span + 5 <= BA_BAND_MAX || keep_order) return false;
    const int W64 = (nfree + 63) / 64;
    std::vector<uint64_t> adj((size_t)nfree * W64, 0), seen((size_t)std::max(P.n_pt, 1) * W64, 0);
    for (int e = 0; e < P.n_edge; ++e) {
        const int c = col[P.edge_kf[e]];
        if (c >= 0) seen[(size_t)P.edge_pt[e] * W64 + (c >> 6)] |= 1ull << (c & 63);
    }
    for (int p = 0; p < P.n_pt; ++p) {
        const uint64_t* m = &seen[(size_t)p * W64];
        for (int w = 0; w < W64; ++w)
            for (uint64_t bits = m[w]; bits; bits &= bits - 1) {
                const int c = 64 * w + __builtin_ctzll(bits);
                for (int v = 0; v < W64; ++v) adj[(size_t)c * W64 + v] |= m[v];
            }
    }
    auto has = [&](int a, int b2) { return (adj[(size_t)a * W64 + (b2 >> 6)] >> (b2 & 63)) & 1ull; };
    auto band_of = [&](const std::vector<int>& pos) {   // max over columns of (position - leftmost coupled position), in keyframes
        int band = 0;
        for (int a = 0; a < nfree; ++a)
            for (int b2 = 0; b2 < nfree; ++b2)
                if (a != b2 && has(a, b2)) band = std::max(band, pos[a] - pos[b2]);
        return band;
    };
    std::vector<int> ident(nfree), deg(nfree, 0);
    for (int a = 0; a < nfree; ++a) {
        ident[a] = a;
        for (int w = 0; w < W64; ++w) deg[a] += __builtin_popcountll(adj[(size_t)a * W64 + w]);
    }
    const int band0 = band_of(ident);
    if (band0 <= 1) return false;
    // Cuthill-McKee per component from a node of minimum degree, neighbours by increasing degree (ties: the caller's order), then reversed
    std::vector<int> order; order.reserve(nfree);
    std::vector<char> used(nfree, 0);
    while ((int)order.size() < nfree) {
        int start = -1;
        for (int a = 0; a < nfree; ++a) if (!used[a] && (start < 0 || deg[a] < deg[start])) start = a;
        size_t head = order.size();
        order.push_back(start); used[start] = 1;
        while (head < order.size()) {
            const int a = order[head++];
            const size_t first = order.size();
            for (int b2 = 0; b2 < nfree; ++b2) if (!used[b2] && has(a, b2)) { order.push_back(b2); used[b2] = 1; }
            std::stable_sort(order.begin() + first, order.end(), [&](int x, int y) { return deg[x] < deg[y]; });
        }
    }
    std::reverse(order.begin(), order.end());
    std::vector<int> pos(nfree);
    for (int i = 0; i < nfree; ++i) pos[order[i]] = i;
    if (band_of(pos) >= band0) return false;
    for (int k = 0; k < P.n_kf; ++k) if (col[k] >= 0) col[k] = pos[col[k]];
    return true;
}

// device point order: by first, then last free column (stable: caller order inside a run)
void point_order(const std::vector<int32_t>& minc, const std::vector<int32_t>& maxc, BaWindowPlan& plan) {
    const int n_pt = (int)minc.size();
    plan.new2old.resize(n_pt);
    plan.old2new.resize(n_pt);
    for (int p = 0; p < n_pt; ++p) plan.new2old[p] = p;
    std::stable_sort(plan.new2old.begin(), plan.new2old.end(),
                     [&](int a, int b) { return minc[a] != minc[b] ? minc[a] < minc[b] : maxc[a] < maxc[b]; });
    for (int p = 0; p < n_pt; ++p) plan.old2new[plan.new2old[p]] = p;
}

// per free column: the range of (sorted) points it observes (plo > phi: none), and the first column it is coupled with
struct ColumnReach {
    std::vector<int32_t> plo, phi, fcol;
};

ColumnReach column_reach(const slamit_ba_problem& P, const BaWindowPlan& plan, const std::vector<int32_t>& minc, int nfree) {
    ColumnReach R;
    R.plo.assign(std::max(nfree, 1), INT32_MAX); R.phi.assign(std::max(nfree, 1), -1); R.fcol.resize(std::max(nfree, 1));
    for (int c = 0; c < nfree; ++c) R.fcol[c] = c;
    for (int e = 0; e < P.n_edge; ++e) {
        const int c = plan.col[P.edge_kf[e]], po = P.edge_pt[e];
        if (c < 0) continue;
        const int pn = plan.old2new[po];
        R.plo[c] = std::min(R.plo[c], pn); R.phi[c] = std::max(R.phi[c], pn);
        R.fcol[c] = std::min(R.fcol[c], minc[po]);
    }
    return R;
}

// The structural arrays of a window as the planner fills them: every entry, in BaWin::side's layout (ba_side_words), copied into BaWin's inline
// arrays once planned (side_to_inline)
struct SideView {
    int32_t *alo, *ahi, *blo, *bhi, *panel_hi, *back_lo;
    SideView(std::vector<int32_t>& s, int T, int P)
        : alo(s.data()), ahi(alo + T), blo(ahi + T), bhi(blo + T), panel_hi(bhi + T), back_lo(panel_hi + P) {}
};

void side_to_inline(const SideView& S, int T, int P, BaWin& w) {
    for (int t = 0; t < std::min(T, BA_MAX_TILES); ++t) { w.tile_alo[t] = S.alo[t]; w.tile_ahi[t] = S.ahi[t]; w.tile_blo[t] = S.blo[t]; w.tile_bhi[t] = S.bhi[t]; }
    for (int i = 0; i < BA_MAX_PANELS; ++i) {   // (panels past the window's own: the defaults ldlt_envelope gives them)
        w.panel_hi[i] = (int16_t)(i < P ? S.panel_hi[i] : std::max(w.nS - 1, 0));
        w.back_lo[i] = (int16_t)(i < P ? S.back_lo[i] : 0);
    }
}

// k range (multiples of BA_KC) of each 64-row tile of GA: the points its pose rows observe; the tile holding row nS (the right-hand side's) spans
// every point as the B operand
void tile_k_ranges(const ColumnReach& R, int nfree, const BaWin& w, const SideView& S) {
    const int T = w.Npad / BA_TILE, kmax = w.Kpad;
    for (int t = 0; t < T; ++t) {
        int lo = INT32_MAX, hi = -1;
        for (int c = 0; c < nfree; ++c) {
            if (6 * c + 5 < BA_TILE * t || 6 * c >= BA_TILE * (t + 1) || R.phi[c] < 0) continue;   // pose rows outside the tile / no points
            lo = std::min(lo, 3 * R.plo[c]); hi = std::max(hi, 3 * R.phi[c] + 3);
        }
        if (hi < 0) { lo = 0; hi = 0; }
        lo = lo / BA_KC * BA_KC; hi = std::min((hi + BA_KC - 1) / BA_KC * BA_KC, kmax);
        S.alo[t] = lo; S.ahi[t] = hi; S.blo[t] = lo; S.bhi[t] = hi;
        if (w.nS >= BA_TILE * t && w.nS < BA_TILE * (t + 1)) { S.blo[t] = 0; S.bhi[t] = kmax; }
    }
}

// LDLt: row envelope.  first[r] = 6 * fcol[r / 6]; panel i (columns 32 i ..) only touches rows r with first[r] < 32 i + 32.  A window whose
// keyframes only share points with their neighbours has a narrow band: LDLt inside LDS
void ldlt_envelope(const ColumnReach& R, int nfree, bool no_band, BaWin& w, const SideView& S) {
    const int n = w.nS;
    for (int i = 0; i < ba_npanel(n); ++i) { S.panel_hi[i] = std::max(n - 1, 0); S.back_lo[i] = 0; }
    for (int i = 0; 32 * i < n; ++i) {
        const int jb = 32 * i, pend = std::min(jb + 32, n);
        int hi = pend - 1, lo = jb;
        for (int c = 0; c < nfree; ++c) {
            if (6 * R.fcol[c] < pend) hi = std::max(hi, 6 * c + 5);                               // row block c reaches into the panel's columns
            if (6 * c + 5 >= jb && 6 * c < pend) lo = std::min(lo, 6 * R.fcol[c]);               // rows of the panel: leftmost column
        }
        S.panel_hi[i] = std::min(hi, n - 1);
        S.back_lo[i] = lo;
    }
    int band = 0;
    for (int c = 0; c < nfree; ++c) band = std::max(band, 6 * c + 5 - 6 * R.fcol[c]);
    w.band = std::min(band, std::max(n - 1, 0));
    w.solver = bak_solver_kind(n, w.band, no_band);
}

// The Schur product over floating row windows (BaWin::sf_*), when every k slab's rows fit one: consecutive slabs whose rows fit one
// run of BA_SF_ROWS form a group.  Leaves sf_groups at 0 (the tiled product) when they do not, or when the groups outnumber what the
// launch and the partial buffer hold.  Widens the tiles' k ranges to what the groups read: k_zero_operands clears those once per solve.
void float_groups(const slamit_ba_problem& P, const BaPlanLimits& L, const BaWindowPlan& plan, const std::vector<int32_t>& minc,
                  const std::vector<int32_t>& maxc, BaWin& w, const SideView& S) {
    const int T = w.Npad / BA_TILE, nslab_all = w.Kpad / BA_KC;
    std::vector<int32_t> slo(nslab_all, INT32_MAX), shi(nslab_all, -1);
    for (int pn = 0; pn < P.n_pt; ++pn) {
        const int po = plan.new2old[pn];
        if (maxc[po] < 0) continue;   // no free keyframe observes it: its columns stay zero
        for (int j = 0; j < 3; ++j) {
            const int sl = (3 * pn + j) / BA_KC;
            slo[sl] = std::min(slo[sl], 6 * minc[po]); shi[sl] = std::max(shi[sl], 6 * maxc[po] + 5);
        }
    }
    // a single window wants many short workgroups (latency), a batch fewer partial tiles to write and to add
    const int cap = L.sf_cap > 0 ? L.sf_cap : L.nwin >= 16 ? 8 : 4;
    const int maxg = (int)std::min<size_t>(std::min<size_t>(BA_SF_MAXG, (size_t)BA_SPLITS * L.Npad_max * L.Npad_max / (BA_TILE * BA_TILE)),   // what `part` holds
                                           (size_t)(T * (T + 1) / 2) * bak_nsplit(L.nwin));                                          // workgroups of the launch
    bool ok = true;
    int G = 0, cnt = 0, clo = 0, chi = 0, kstart = 0;
    auto close = [&](int kend) {
        if (!cnt) return;
        if (G == maxg) { ok = false; return; }
        w.sf_row[G] = (int16_t)clo; w.sf_k0[G] = (int16_t)kstart; w.sf_k1[G] = (int16_t)kend;
        ++G; cnt = 0;
    };
    for (int sl = 0; sl < nslab_all && ok; ++sl) {
        if (shi[sl] < 0) { close(sl); continue; }
        if (shi[sl] - slo[sl] + 1 > BA_SF_ROWS || nslab_all > INT16_MAX) { ok = false; break; }
        if (cnt && (std::max(chi, shi[sl]) - std::min(clo, slo[sl]) + 1 > BA_SF_ROWS || cnt == cap)) close(sl);
        if (!cnt) { clo = slo[sl]; chi = shi[sl]; kstart = sl; }
        else { clo = std::min(clo, slo[sl]); chi = std::max(chi, shi[sl]); }
        ++cnt;
    }
    if (ok) close(nslab_all);
    for (int g = 1; g < G && ok; ++g) if (w.sf_row[g] < w.sf_row[g - 1]) ok = false;   // (sorted points: cannot happen)
    if (!ok || G == 0) return;
    w.sf_groups = G;
    int ga = 0, gb = -1;   // groups whose window reaches row r (first) / has begun at row r (last)
    for (int r = 0; r < w.Npad; ++r) {
        while (ga < G && w.sf_row[ga] + BA_SF_ROWS - 1 < r) ++ga;
        while (gb + 1 < G && w.sf_row[gb + 1] <= r) ++gb;
        w.sf_glo[r] = (int16_t)ga; w.sf_ghi[r] = (int16_t)gb;
    }
    auto widen = [](int32_t& lo, int32_t& hi, int klo, int khi) {
        if (hi <= lo) { lo = klo; hi = khi; }
        else { lo = std::min(lo, klo); hi = std::max(hi, khi); }
    };
    for (int g = 0; g < G; ++g) {
        const int t0 = w.sf_row[g] / BA_TILE, t1 = std::min(w.sf_row[g] + BA_SF_ROWS - 1, w.Npad - 1) / BA_TILE;
        for (int t = t0; t <= t1; ++t) {
            widen(S.alo[t], S.ahi[t], w.sf_k0[g] * BA_KC, w.sf_k1[g] * BA_KC);
            widen(S.blo[t], S.bhi[t], w.sf_k0[g] * BA_KC, w.sf_k1[g] * BA_KC);
        }
    }
}

// what the Schur product multiplies per trial: the groups' slabs, or the 64 x 64 tile pairs (I <= J) it computes (schur_tile_needed)
// over the k range both tiles have non-zeros in
double executed_mflop(const BaWin& w) {
    double mflop = 0;
    if (w.sf_groups) {
        for (int g = 0; g < w.sf_groups; ++g) mflop += 2.0 * BA_TILE * BA_TILE * BA_KC * (w.sf_k1[g] - w.sf_k0[g]) * 1e-6;
        return mflop;
    }
    const int T = w.Npad / BA_TILE;
    for (int I = 0; I < T; ++I)
        for (int J = I; J < T; ++J)
            if (schur_tile_needed(w, I, J))
                mflop += 2.0 * BA_TILE * BA_TILE * (std::min(ba_tile_ahi(w, I), ba_tile_bhi(w, J)) - std::max(ba_tile_alo(w, I), ba_tile_blo(w, J))) * 1e-6;
    return mflop;
}

}  // namespace

bool ba_plan_window(const slamit_ba_problem& P, const BaPlanLimits& L, BaWin& w, BaWindowPlan& plan) {
    if (!edges_valid(P)) return false;
    const int nfree = free_columns(P, plan.col);
    w.n_kf = P.n_kf; w.n_pt = P.n_pt; w.n_edge = P.n_edge;
    w.n_free = nfree; w.nS = 6 * nfree;
    w.Npad = (int)ba_rup((size_t)w.nS + 1, BA_TILE);
    w.Kpad = (int)ba_rup((size_t)std::max(3 * P.n_pt, 1), (size_t)BA_KC * BA_SPLITS);
    std::vector<int32_t> minc, maxc, seen_by;
    point_columns(P, plan.col, minc, maxc, &seen_by);
    int span = 0;
    bool complete = false;
    for (int p = 0; p < P.n_pt; ++p) {
        if (maxc[p] >= 0) span = std::max(span, maxc[p] - minc[p]);
        complete = complete || (maxc[p] - minc[p] + 1 == nfree && seen_by[p] >= nfree);
    }
    if (ba_order_columns(P, plan.col.data(), nfree, span, complete, L.keep_order))
        point_columns(P, plan.col, minc, maxc, nullptr);   // renumbered: the points' column ranges once more
    point_order(minc, maxc, plan);
    const ColumnReach R = column_reach(P, plan, minc, nfree);
    const int T = w.Npad / BA_TILE, NP = ba_npanel(w.nS);
    plan.side.assign(ba_side_words(w.Npad, w.nS), 0);
    const SideView S(plan.side, T, NP);
    tile_k_ranges(R, nfree, w, S);
    ldlt_envelope(R, nfree, L.no_band, w, S);
    w.sf_groups = 0;
    // (floating windows: only a system BaWin::sf_glo / sf_ghi cover; a larger one takes the tile pairs)
    if (!L.no_sf && nfree > 0 && w.Npad <= BA_TILE * BA_MAX_TILES) float_groups(P, L, plan, minc, maxc, w, S);
    side_to_inline(S, T, NP, w);
    w.side = plan.side.data();   // (the accessors read the host table while planning)
    plan.exec_mflop = executed_mflop(w);
    w.side = nullptr;
    return true;
}

void ba_pack_inputs(const slamit_ba_problem& P, const BaWindowPlan& plan, const IoLayout& H) {
    memcpy(H.pose_col, plan.col.data(), sizeof(int32_t) * (size_t)P.n_kf);
    memcpy(H.in_pose, P.kf_pose, sizeof(double) * 12 * (size_t)P.n_kf);
    memcpy(H.intr, P.kf_intr, sizeof(double) * 4 * (size_t)P.n_kf);
    for (int p = 0; p < P.n_pt; ++p) for (int j = 0; j < 3; ++j) H.in_pt[3 * (size_t)p + j] = P.pt_xyz[3 * (size_t)plan.new2old[p] + j];
    if (P.n_edge) {
        memcpy(H.e_kf, P.edge_kf, sizeof(int32_t) * (size_t)P.n_edge);
        memcpy(H.e_uv, P.edge_uv, sizeof(double) * 2 * (size_t)P.n_edge);
        memcpy(H.e_w, P.edge_inv_sigma2, sizeof(double) * (size_t)P.n_edge);
        if (P.edge_ur) memcpy(H.e_ur, P.edge_ur, sizeof(double) * (size_t)P.n_edge);
    }
    if (P.edge_ur) memcpy(H.bf, P.kf_bf, sizeof(double) * (size_t)P.n_kf);
    int32_t* pptr = H.pt_ptr; int32_t* kptr = H.kf_ptr;
    for (int p = 0; p <= P.n_pt; ++p) pptr[p] = 0;
    for (int k = 0; k <= P.n_kf; ++k) kptr[k] = 0;
    for (int e = 0; e < P.n_edge; ++e) { H.e_pt[e] = plan.old2new[P.edge_pt[e]]; ++pptr[H.e_pt[e] + 1]; ++kptr[P.edge_kf[e] + 1]; }
    for (int p = 0; p < P.n_pt; ++p) pptr[p + 1] += pptr[p];
    for (int k = 0; k < P.n_kf; ++k) kptr[k + 1] += kptr[k];
    std::vector<int32_t> pc(pptr, pptr + P.n_pt), kc(kptr, kptr + P.n_kf);
    for (int e = 0; e < P.n_edge; ++e) { H.pt_edges[pc[H.e_pt[e]]++] = e; H.kf_edges[kc[P.edge_kf[e]]++] = e; }
    if (H.side) memcpy(H.side, plan.side.data(), sizeof(int32_t) * plan.side.size());
}

void ba_unpack_outputs(const slamit_ba_problem& P, const BaWindowPlan& plan, const IoLayout& H, slamit_ba_result& R) {
    memcpy(R.kf_pose, H.out_pose, sizeof(double) * 12 * (size_t)P.n_kf);
    for (int p = 0; p < P.n_pt; ++p)
        for (int j = 0; j < 3; ++j) R.pt_xyz[3 * (size_t)plan.new2old[p] + j] = H.out_pt[3 * (size_t)p + j];
    if (P.n_edge) {
        if (R.edge_chi2) memcpy(R.edge_chi2, H.out_chi2, sizeof(double) * (size_t)P.n_edge);
        if (R.edge_outlier) memcpy(R.edge_outlier, H.out_flag, (size_t)P.n_edge);
        if (R.edge_stage1_outlier) memcpy(R.edge_stage1_outlier, H.out_out1, (size_t)P.n_edge);
    }
    slamit_ba_stats* S = R.stats;
    if (!S) return;
    const BaState& S0 = *H.out_state;
    memset(S, 0, sizeof(*S));
    for (int sg = 0; sg < 2; ++sg) {
        S->n_its[sg] = S0.n_its[sg];
        S->chi2_init[sg] = S0.chi2_init[sg];
        for (int i = 0; i < SLAMIT_BA_MAX_ITS; ++i) { S->chi2[sg][i] = S0.chi2[sg][i]; S->lambda[sg][i] = S0.lam[sg][i]; S->trials[sg][i] = S0.trials[sg][i]; }
    }
}

// ---- a batch of windows ----

BaRefusal ba_batch_check(const slamit_ba_problem* probs, const slamit_ba_result* results, int nwin, const BaCaps& caps) {
    if (!probs || !results || nwin < 0) return {SLAMIT_ERR_ARG, "slamit_ba_solve_batch: bad argument"};
    if (nwin > caps.max_batch) return {SLAMIT_ERR_CAPACITY, "slamit_ba_solve_batch: nwin > max_batch"};
    for (int b = 0; b < nwin; ++b) {
        const slamit_ba_problem& P = probs[b];
        if (P.n_kf < 1 || P.n_pt < 0 || P.n_edge < 0 || P.n_kf > caps.max_kf || P.n_pt > caps.max_pt || P.n_edge > caps.max_edge)
            return {SLAMIT_ERR_CAPACITY, "slamit_ba_solve_batch: window exceeds the handle's capacity"};
        if (!P.kf_pose || !P.kf_fixed || !P.kf_intr || (P.n_pt && !P.pt_xyz) ||
            (P.n_edge && (!P.edge_kf || !P.edge_pt || !P.edge_uv || !P.edge_inv_sigma2)))
            return {SLAMIT_ERR_ARG, "slamit_ba_solve_batch: null input array"};
        int nfree = 0;
        for (int k = 0; k < P.n_kf; ++k) nfree += P.kf_fixed[k] ? 0 : 1;
        if (nfree > caps.max_free_kf)
            return {SLAMIT_ERR_CAPACITY, "slamit_ba_solve_batch: window has more free keyframes than the handle's max_free_kf"};
        if (P.edge_ur && !P.kf_bf)
            return {SLAMIT_ERR_ARG, "slamit_ba_solve_batch: stereo observations (edge_ur) without the keyframes' bf (kf_bf)"};
        if (!results[b].kf_pose || (P.n_pt && !results[b].pt_xyz))
            return {SLAMIT_ERR_ARG, "slamit_ba_solve_batch: null output array"};
    }
    return {SLAMIT_OK, nullptr};
}

void ba_batch_layout(const slamit_ba_problem* probs, int nwin, size_t win_bytes, uint8_t* slab, BaBatchPlan& B) {
    B.nwin = nwin;
    B.side_w.resize(nwin); B.dio.resize(nwin); B.in_off.resize(nwin); B.out_off.resize(nwin);
    B.mk = B.mp = B.me = 1;
    size_t off = 0;
    for (int b = 0; b < nwin; ++b) {
        const slamit_ba_problem& P = probs[b];
        B.mk = std::max(B.mk, P.n_kf); B.mp = std::max(B.mp, P.n_pt); B.me = std::max(B.me, P.n_edge);
        B.side_w[b] = ba_io_side_words(P);
        B.dio[b] = carve_io(slab ? slab + (size_t)b * win_bytes : nullptr, P.n_kf, P.n_pt, P.n_edge, P.edge_ur != nullptr, B.side_w[b]);
        B.in_off[b] = off; off += B.dio[b].in_bytes;
    }
    for (int b = 0; b < nwin; ++b) { B.out_off[b] = off; off += B.dio[b].bytes - B.dio[b].out_off; }
    B.st_off = ba_rup(off, 256);
    B.pin_need = B.st_off + 2 * sizeof(BaState) * (size_t)nwin;
    B.Npad = B.Npad_ldlt = BA_TILE; B.solvers = 0; B.tl_grid.clear();
}

void ba_batch_launches(const BaWin* wins, const BaWindowPlan* plans, BaBatchPlan& B) {
    B.Npad = B.Npad_ldlt = BA_TILE; B.solvers = 0; B.tl_grid.clear();
    for (int b = 0; b < B.nwin; ++b) {
        B.Npad = std::max(B.Npad, wins[b].Npad);
        B.solvers |= 1u << wins[b].solver;
        if (wins[b].solver != BA_SOLVER_TILED) { B.Npad_ldlt = std::max(B.Npad_ldlt, wins[b].Npad); continue; }
        BaWin wh = wins[b];
        wh.side = plans[b].side.data();   // (ba_panel_hi reads the host copy of the side table)
        const int n = wh.nS, np = (n + 31) / 32;
        if ((int)B.tl_grid.size() < 2 * np) B.tl_grid.resize(2 * np, 0);
        for (int i = 0; i < np; ++i) {
            const int base = std::min(32 * i + 32, n), below = std::max(ba_panel_hi(wh, i) + 1 - base, 0);
            B.tl_grid[2 * i] = std::max(B.tl_grid[2 * i], (below + 1 + BA_TL_CHUNK - 1) / BA_TL_CHUNK);
            B.tl_grid[2 * i + 1] = std::max(B.tl_grid[2 * i + 1], ldlt_tiled_ntiles(below));
        }
    }
}
