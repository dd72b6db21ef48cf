// essential_plan_driver.cc — C entry points over csrc/essential_plan.cc for tests/test_essential_plan.py (ctypes), and with
// -DEG_PLAN_MAIN a stand-alone program that plans a few graphs, for the -fsanitize=address,undefined run.  No GPU, no HIP.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "essential_plan.h"

extern "C" int eg_plan_c(const slamit_eg_graph* g, int32_t cap, int32_t* v0, int32_t* v1, int32_t* kind, int32_t* n_edge, int32_t* inc_ptr,
                         int32_t* inc_edge, const char** why) {
    static const char* none = "";
    *why = none;
    int rc = eg_check_graph(*g, why);
    if (rc != SLAMIT_OK) return rc;
    std::vector<EgEdge> e;
    rc = eg_plan_edges(*g, e, why);
    if (rc != SLAMIT_OK) return rc;
    *n_edge = (int32_t)e.size();
    if ((int32_t)e.size() > cap) return SLAMIT_ERR_CAPACITY;
    for (size_t k = 0; k < e.size(); ++k) { v0[k] = e[k].v0; v1[k] = e[k].v1; kind[k] = e[k].kind; }
    rc = eg_check_edges(g->n_kf, g->kf_bad, *n_edge, v0, v1, kind, why);
    if (rc != SLAMIT_OK) return rc;
    eg_incidence(g->n_kf, *n_edge, v0, v1, inc_ptr, inc_edge);
    return eg_incidence_matches(g->n_kf, *n_edge, v0, v1, inc_ptr, inc_edge) ? SLAMIT_OK : SLAMIT_ERR_STATE;
}

extern "C" int eg_check_edges_c(int32_t n_kf, const uint8_t* bad, int32_t n_edge, const int32_t* v0, const int32_t* v1, const int32_t* kind) {
    const char* why = "";
    return eg_check_edges(n_kf, bad, n_edge, v0, v1, kind, &why);
}

#ifdef EG_PLAN_MAIN
// a chain of n keyframes with covisibility to the next two, one loop connection, optionally a bad keyframe and an out-of-range slot
static int plan_chain(int n, int bad_slot, int wild_parent) {
    std::vector<uint8_t> bad(n, 0);
    std::vector<int32_t> id(n), par(n), cptr(n + 1, 0), ckf, lptr(n + 1, 0), lkf, okf((size_t)n * 4, -1), ow((size_t)n * 4, 0), on(n, 0), qptr(n + 1, 0), qkf;
    for (int i = 0; i < n; ++i) {
        id[i] = 2 * i + 1; par[i] = i - 1;
        if (i + 1 < n) ckf.push_back(i + 1);
        cptr[i + 1] = (int32_t)ckf.size();
        int k = 0;
        for (int d = 1; d <= 2; ++d)
            for (int s = -1; s <= 1; s += 2) {
                const int j = i + s * d;
                if (j >= 0 && j < n) { okf[4 * i + k] = j; ow[4 * i + k] = d == 1 ? 150 : 90; ++k; }
            }
        on[i] = k;
        if (i == n - 1 && n > 1) qkf.push_back(0);
        qptr[i + 1] = (int32_t)qkf.size();
    }
    if (bad_slot >= 0) bad[bad_slot] = 1;
    if (wild_parent) par[n / 2] = n + 7;
    slamit_eg_graph g;
    memset(&g, 0, sizeof(g));
    g.n_kf = n; g.row_cap = 4; g.loop_kf = 0; g.cur_kf = n - 1; g.min_feat = 100;
    g.kf_bad = bad.data(); g.kf_id = id.data(); g.kf_parent = par.data(); g.child_ptr = cptr.data(); g.child_kf = ckf.data();
    g.loop_ptr = lptr.data(); g.loop_kf_list = lkf.data(); g.ord_kf = okf.data(); g.ord_w = ow.data(); g.ord_n = on.data();
    g.conn_ptr = qptr.data(); g.conn_kf = qkf.data();
    const int cap = 8 * n + 8;
    std::vector<int32_t> v0(cap), v1(cap), kind(cap), ip(n + 1), ie(2 * (size_t)cap);
    int32_t ne = 0;
    const char* why = "";
    const int rc = eg_plan_c(&g, cap, v0.data(), v1.data(), kind.data(), &ne, ip.data(), ie.data(), &why);
    printf("n %d bad %d wild %d -> rc %d edges %d %s\n", n, bad_slot, wild_parent, rc, ne, why);
    return rc;
}

int main() {
    int fails = 0;
    fails += plan_chain(1, -1, 0) != SLAMIT_OK;
    fails += plan_chain(9, -1, 0) != SLAMIT_OK;
    fails += plan_chain(300, -1, 0) != SLAMIT_OK;
    fails += plan_chain(9, 4, 0) != SLAMIT_ERR_ARG;    // keyframe 5's parent is bad
    fails += plan_chain(9, -1, 1) != SLAMIT_ERR_ARG;   // a parent outside the table
    printf("%s\n", fails ? "FAILED" : "ok");
    return fails;
}
#endif
