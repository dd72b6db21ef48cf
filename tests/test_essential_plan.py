"""csrc/essential_plan.cc on the CPU: built with g++ beside tests/essential_plan_driver.cc, its edge list must equal the literal Python
restatement of Optimizer.cc:847-983 (tests/essential_ref.plan_edges) edge for edge, in order, on graphs that hit every exclusion; the
same sources as a stand-alone program run clean under -fsanitize=address,undefined."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import essential_ref as er
from tests.helpers import ROOT

CSRC = os.path.join(ROOT, "weiner_slamit_v2_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "essential_plan_driver.cc"), os.path.join(CSRC, "essential_plan.cc")]
ERR_ARG, ERR_CAPACITY = -1, -3


@pytest.fixture(scope="module")
def plib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("eg_plan") / "libeg_plan.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC] + SOURCES + ["-o", so])
    return C.CDLL(so)


def run_plan(plib, g, cap=None):
    from weiner_slamit_v2_amd import api

    n = int(g["n_kf"])
    keep = {k: np.ascontiguousarray(g[k], dt) for k, dt in api._EG_GRAPH_ARRAYS}
    rec = api.EgGraph(n, int(g["row_cap"]), int(g["loop_kf"]), int(g["cur_kf"]), int(g["min_feat"]), 0,
                      *[keep[k].ctypes.data_as(C.c_void_p) for k, _ in api._EG_GRAPH_ARRAYS])
    cap = 8 * n + 8 if cap is None else cap
    v0, v1, kind = (np.zeros(max(cap, 1), np.int32) for _ in range(3))
    ip, ie = np.zeros(n + 1, np.int32), np.zeros(2 * max(cap, 1), np.int32)
    ne, why = C.c_int32(0), C.c_char_p()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = plib.eg_plan_c(C.byref(rec), cap, p(v0), p(v1), p(kind), C.byref(ne), p(ip), p(ie), C.byref(why))
    e = ne.value
    return rc, list(zip(v0[:e].tolist(), v1[:e].tolist(), kind[:e].tolist())) if rc == 0 else e, ip, ie[:2 * e]


def as_lists(g):
    """the tables of slamit_eg_graph as plan_edges wants them"""
    n = int(g["n_kf"])
    rows = lambda ptr, val: [list(map(int, val[ptr[i]:ptr[i + 1]])) for i in range(n)]
    conn = rows(g["conn_ptr"], g["conn_kf"])
    return dict(kf_bad=list(map(int, g["kf_bad"])), kf_id=list(map(int, g["kf_id"])), kf_parent=list(map(int, g["kf_parent"])),
                children=rows(g["child_ptr"], g["child_kf"]), loop_edges=rows(g["loop_ptr"], g["loop_kf_list"]),
                covis=[[(int(g["ord_kf"][i][k]), int(g["ord_w"][i][k])) for k in range(int(g["ord_n"][i]))] for i in range(n)],
                loop_connections={i: conn[i] for i in range(n) if conn[i]}, loop_kf=int(g["loop_kf"]), cur_kf=int(g["cur_kf"]),
                min_feat=int(g["min_feat"]))


GRAPHS = [dict(n_kf=12, seed=1), dict(n_kf=4, seed=3, n_corrected=1), dict(n_kf=40, seed=6, mixed=True), dict(n_kf=24, seed=9, mixed=True),
          dict(n_kf=75, seed=8), dict(n_kf=50, seed=2, chain=True), dict(n_kf=30, seed=5, min_feat=130)]


@pytest.mark.parametrize("kw", GRAPHS, ids=lambda kw: "-".join("%s%s" % (k[:3], v) for k, v in kw.items()))
def test_plan_equals_the_restatement(plib, kw):
    from weiner_slamit_v2_amd import synth

    g = synth.synth_essential(n_pt=4, **kw)
    rc, edges, ip, ie = run_plan(plib, g)
    assert rc == 0
    want = er.plan_edges(as_lists(g))
    assert edges == want and len(edges) >= int(g["n_kf"]) - 2
    # the incidence lists: per slot its edges ascending, the side bit right
    for i in range(int(g["n_kf"])):
        mine = [2 * e + s for e, (a, b, _) in enumerate(want) for s, v in ((0, a), (1, b)) if v == i]
        assert ie[ip[i]:ip[i + 1]].tolist() == sorted(mine)


def test_the_mixed_graph_hits_every_odd_place(plib):
    """What the synthetic graph is for, checked on the restatement itself so that a generator change cannot hollow the comparison out."""
    from weiner_slamit_v2_amd import synth

    g = synth.synth_essential(n_kf=40, seed=6, mixed=True, n_pt=4)
    L = as_lists(g)
    edges = er.plan_edges(L)
    n, cur, loop, mf = 40, 39, 0, 100
    w = lambda i, j: dict(L["covis"][i]).get(j, 0)
    lc = [(a, b) for a, b, k in edges if k == er.EG_LOOP_CONNECTION]
    assert (cur, loop) in lc and w(cur, loop) < mf                                       # exempt from the weight gate
    assert any(w(i, j) < mf for i, js in L["loop_connections"].items() for j in js if (i, j) not in lc)   # ... which drops others
    pairs = [(a, b) for a, b, _ in edges]
    assert len(set(pairs)) < len(pairs) and (cur - 1, loop + 1) in lc and pairs.count((cur - 1, loop + 1)) == 2   # parallel edges
    assert (n - 10, 4) in pairs and pairs.count((n - 10, 4)) == 1 and w(n - 10, 4) >= mf      # old loop edge once: sLoopEdges.count
    assert L["kf_bad"][20] and all(20 not in p for p in pairs)                              # the slot gap
    assert (7, 8) in pairs and L["kf_id"][8] < L["kf_id"][7]                                 # `<` on mnId, not on the slot
    assert all(w_ >= mf for _, w_ in L["covis"][15]) and not any(a == 15 and (b != L["kf_parent"][15]) for a, b in pairs)   # the all-above row
    covis_only = [(a, b) for a, b, k in edges if k == er.EG_NORMAL and b != L["kf_parent"][a] and b not in L["loop_edges"][a]]
    assert covis_only and all(b not in L["children"][a] for a, b in covis_only)              # !hasChild
    ins = {(min(L["kf_id"][a], L["kf_id"][b]), max(L["kf_id"][a], L["kf_id"][b])) for a, b in lc}
    skipped = [(i, j) for i in range(n) for j, w_ in L["covis"][i] if w_ >= mf and (min(L["kf_id"][i], L["kf_id"][j]), max(L["kf_id"][i], L["kf_id"][j])) in ins
               and L["kf_id"][j] < L["kf_id"][i] and j != L["kf_parent"][i]]
    assert skipped and all(pairs.count(p) == (1 if p in lc else 0) for p in skipped)         # sInsertedEdges: covisibility edges only


def test_plan_refuses_what_g2o_would_be_handed_null_for(plib):
    from weiner_slamit_v2_amd import synth

    g = synth.synth_essential(n_kf=12, seed=1, n_pt=4)
    for edit in ("bad_parent", "wild_child", "bad_conn", "wild_cur", "ord_n"):
        h = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in g.items()}
        if edit == "bad_parent":
            h["kf_bad"][5] = 1
        elif edit == "wild_child":
            h["child_kf"][2] = 12
        elif edit == "bad_conn":
            h["kf_bad"][0] = 1
        elif edit == "wild_cur":
            h["cur_kf"] = -1
        else:
            h["ord_n"][3] = h["row_cap"] + 1
        assert run_plan(plib, h)[0] == ERR_ARG, edit
    rc, need, _, _ = run_plan(plib, g, cap=3)
    assert rc == ERR_CAPACITY and need == len(er.plan_edges(as_lists(g)))
    p = lambda a: np.asarray(a).ctypes.data_as(C.c_void_p)
    bad = np.zeros(4, np.uint8)
    ok = lambda v0, v1, k, b=bad: plib.eg_check_edges_c(4, p(b), len(v0), p(np.array(v0, np.int32)), p(np.array(v1, np.int32)), p(np.array(k, np.int32)))
    assert ok([1, 2], [0, 1], [0, 1]) == 0
    assert ok([1, 4], [0, 1], [0, 1]) == ERR_ARG and ok([1, -1], [0, 1], [0, 1]) == ERR_ARG and ok([1], [1], [0]) == ERR_ARG and ok([1], [0], [2]) == ERR_ARG
    assert ok([1], [0], [0], np.array([1, 0, 0, 0], np.uint8)) == ERR_ARG


def test_plan_program_runs_clean_under_sanitizers(tmp_path):
    exe = str(tmp_path / "eg_plan_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DEG_PLAN_MAIN", "-I", CSRC] + SOURCES + ["-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert out.returncode == 0 and out.stdout.decode().strip().endswith("ok"), out.stdout.decode()
