// essential_plan.cc — see essential_plan.h.
#include "essential_plan.h"

#include <algorithm>
#include <set>
#include <utility>

namespace {

bool csr_ok(const int32_t* ptr, const int32_t* val, int n) {
    if (!ptr || ptr[0] != 0) return false;
    for (int i = 0; i < n; ++i)
        if (ptr[i + 1] < ptr[i]) return false;
    if (ptr[n] > 0 && !val) return false;
    for (int k = 0; k < ptr[n]; ++k)
        if (val[k] < 0 || val[k] >= n) return false;
    return true;
}

bool in_row(const int32_t* ptr, const int32_t* val, int i, int j) {
    for (int k = ptr[i]; k < ptr[i + 1]; ++k)
        if (val[k] == j) return true;
    return false;
}

}  // namespace

int eg_check_graph(const slamit_eg_graph& g, const char** why) {
    const int n = g.n_kf;
    if (n < 0 || g.row_cap < 0) { *why = "negative count"; return SLAMIT_ERR_ARG; }
    if (n == 0) return SLAMIT_OK;
    if (!g.kf_bad || !g.kf_id || !g.kf_parent || !g.ord_n || (g.row_cap > 0 && (!g.ord_kf || !g.ord_w))) { *why = "null table"; return SLAMIT_ERR_ARG; }
    if (g.loop_kf < 0 || g.loop_kf >= n || g.cur_kf < 0 || g.cur_kf >= n) { *why = "loop_kf / cur_kf outside [0, n_kf)"; return SLAMIT_ERR_ARG; }
    if (!csr_ok(g.child_ptr, g.child_kf, n)) { *why = "children CSR"; return SLAMIT_ERR_ARG; }
    if (!csr_ok(g.loop_ptr, g.loop_kf_list, n)) { *why = "loop-edge CSR"; return SLAMIT_ERR_ARG; }
    if (!csr_ok(g.conn_ptr, g.conn_kf, n)) { *why = "LoopConnections CSR"; return SLAMIT_ERR_ARG; }
    for (int i = 0; i < n; ++i) {
        if (g.kf_parent[i] < -1 || g.kf_parent[i] >= n) { *why = "parent outside [-1, n_kf)"; return SLAMIT_ERR_ARG; }
        if (g.ord_n[i] < 0 || g.ord_n[i] > g.row_cap) { *why = "ord_n outside [0, row_cap]"; return SLAMIT_ERR_ARG; }
        for (int k = 0; k < g.ord_n[i]; ++k) {
            const int j = g.ord_kf[(size_t)i * g.row_cap + k];
            if (j < 0 || j >= n) { *why = "covisible keyframe outside [0, n_kf)"; return SLAMIT_ERR_ARG; }
        }
    }
    return SLAMIT_OK;
}

int eg_plan_edges(const slamit_eg_graph& g, std::vector<EgEdge>& edges, const char** why) {
    const int n = g.n_kf;
    edges.clear();
    if (n == 0) return SLAMIT_OK;
    const int32_t* id = g.kf_id;
    auto weight = [&](int i, int j) {   // KeyFrame::GetWeight, read from the ordered row
        for (int k = 0; k < g.ord_n[i]; ++k)
            if (g.ord_kf[(size_t)i * g.row_cap + k] == j) return g.ord_w[(size_t)i * g.row_cap + k];
        return 0;
    };
    auto add = [&](int i, int j, int kind) {
        if (g.kf_bad[i] || g.kf_bad[j]) return false;
        edges.push_back(EgEdge{i, j, kind});
        return true;
    };
    std::set<std::pair<int32_t, int32_t>> inserted;   // sInsertedEdges, on mnIds
    // :852-880, LoopConnections: ascending slot for the map and for each set
    for (int i = 0; i < n; ++i) {
        std::vector<int32_t> row(g.conn_kf + g.conn_ptr[i], g.conn_kf + g.conn_ptr[i + 1]);
        std::sort(row.begin(), row.end());
        row.erase(std::unique(row.begin(), row.end()), row.end());
        for (const int j : row) {
            if ((id[i] != id[g.cur_kf] || id[j] != id[g.loop_kf]) && weight(i, j) < g.min_feat) continue;
            if (!add(i, j, SLAMIT_EG_LOOP_CONNECTION)) { *why = "a LoopConnections edge names a bad keyframe"; return SLAMIT_ERR_ARG; }
            inserted.insert(std::make_pair(std::min(id[i], id[j]), std::max(id[i], id[j])));
        }
    }
    // :883-983, per keyframe
    for (int i = 0; i < n; ++i) {
        if (g.kf_bad[i]) continue;
        const int par = g.kf_parent[i];
        if (par >= 0 && !add(i, par, SLAMIT_EG_NORMAL)) { *why = "a keyframe's parent is bad"; return SLAMIT_ERR_ARG; }
        std::vector<int32_t> le(g.loop_kf_list + g.loop_ptr[i], g.loop_kf_list + g.loop_ptr[i + 1]);
        std::sort(le.begin(), le.end());
        le.erase(std::unique(le.begin(), le.end()), le.end());
        for (const int l : le)
            if (id[l] < id[i] && !add(i, l, SLAMIT_EG_NORMAL)) { *why = "a loop edge names a bad keyframe"; return SLAMIT_ERR_ARG; }
        // GetCovisiblesByWeight(minFeat): the row up to the first weight below minFeat, and nothing when there is none
        int cut = -1;
        for (int k = 0; k < g.ord_n[i] && cut < 0; ++k)
            if (g.min_feat > g.ord_w[(size_t)i * g.row_cap + k]) cut = k;
        for (int k = 0; k < cut; ++k) {
            const int j = g.ord_kf[(size_t)i * g.row_cap + k];
            if (j == par || in_row(g.child_ptr, g.child_kf, i, j) || std::binary_search(le.begin(), le.end(), j)) continue;
            if (g.kf_bad[j] || !(id[j] < id[i])) continue;
            if (inserted.count(std::make_pair(std::min(id[i], id[j]), std::max(id[i], id[j])))) continue;
            add(i, j, SLAMIT_EG_NORMAL);
        }
    }
    return SLAMIT_OK;
}

int eg_check_edges(int32_t n_kf, const uint8_t* bad, int32_t n_edge, const int32_t* v0, const int32_t* v1, const int32_t* kind, const char** why) {
    for (int e = 0; e < n_edge; ++e) {
        if (v0[e] < 0 || v0[e] >= n_kf || v1[e] < 0 || v1[e] >= n_kf) { *why = "an edge names a keyframe outside [0, n_kf)"; return SLAMIT_ERR_ARG; }
        if (bad[v0[e]] || bad[v1[e]]) { *why = "an edge names a bad keyframe"; return SLAMIT_ERR_ARG; }
        if (v0[e] == v1[e]) { *why = "an edge from a keyframe to itself"; return SLAMIT_ERR_ARG; }
        if (kind[e] != SLAMIT_EG_NORMAL && kind[e] != SLAMIT_EG_LOOP_CONNECTION) { *why = "unknown edge kind"; return SLAMIT_ERR_ARG; }
    }
    return SLAMIT_OK;
}

void eg_incidence(int32_t n_kf, int32_t n_edge, const int32_t* v0, const int32_t* v1, int32_t* inc_ptr, int32_t* inc_edge) {
    for (int i = 0; i <= n_kf; ++i) inc_ptr[i] = 0;
    for (int e = 0; e < n_edge; ++e) { ++inc_ptr[v0[e] + 1]; ++inc_ptr[v1[e] + 1]; }
    for (int i = 0; i < n_kf; ++i) inc_ptr[i + 1] += inc_ptr[i];
    std::vector<int32_t> at(inc_ptr, inc_ptr + n_kf);
    for (int e = 0; e < n_edge; ++e) {   // ascending e per slot: list order
        inc_edge[at[v0[e]]++] = 2 * e;
        inc_edge[at[v1[e]]++] = 2 * e + 1;
    }
}

bool eg_incidence_matches(int32_t n_kf, int32_t n_edge, const int32_t* v0, const int32_t* v1, const int32_t* inc_ptr, const int32_t* inc_edge) {
    std::vector<int32_t> p((size_t)n_kf + 1), q((size_t)2 * n_edge + 1);
    eg_incidence(n_kf, n_edge, v0, v1, p.data(), q.data());
    return std::equal(p.begin(), p.end(), inc_ptr) && std::equal(q.begin(), q.begin() + 2 * (size_t)n_edge, inc_edge);
}
