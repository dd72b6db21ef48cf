"""The host-side plan of a local-BA window (csrc/ba_plan.cc) on the CPU: ba_plan.cc is built with g++ together with a small C driver,
and the plan is compared to a pinned record (tests/golden/ba_plans.json) and checked against the rules the kernels rely on."""
import ctypes as C
import glob
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import ROOT, load_ba_golden

CSRC = os.path.join(ROOT, "weiner_slamit_v2_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "ba_plans.json")

BA_TILE, BA_KC, BA_SF_ROWS, BA_SOLVER_BAND = 64, 32, 63, 0
SCALARS = ("n_kf", "n_pt", "n_edge", "n_free", "nS", "Npad", "Kpad", "band", "solver", "sf_groups")
ARRAYS = (("tile_alo", 10), ("tile_ahi", 10), ("tile_blo", 10), ("tile_bhi", 10), ("panel_hi", 20), ("back_lo", 20),
          ("sf_row", 256), ("sf_k0", 256), ("sf_k1", 256), ("sf_glo", 640), ("sf_ghi", 640))
NFIELDS = len(SCALARS) + sum(n for _, n in ARRAYS)

# BaWin's structural fields, in the order above, as one int32 array; the planner's other results beside them
DRIVER = r'''
#include <string.h>
#include <vector>
#include "ba_plan.h"

static void fields_out(const BaWin& w, int32_t* o) {
    const int32_t s[] = {w.n_kf, w.n_pt, w.n_edge, w.n_free, w.nS, w.Npad, w.Kpad, w.band, w.solver, w.sf_groups};
    for (int32_t v : s) *o++ = v;
#define PUT(a) for (size_t i = 0; i < sizeof(w.a) / sizeof(w.a[0]); ++i) *o++ = w.a[i];
    PUT(tile_alo) PUT(tile_ahi) PUT(tile_blo) PUT(tile_bhi) PUT(panel_hi) PUT(back_lo) PUT(sf_row) PUT(sf_k0) PUT(sf_k1) PUT(sf_glo) PUT(sf_ghi)
}

static BaPlanLimits limits(const int32_t* l) { return BaPlanLimits{l[0], l[1], l[2] != 0, l[3] != 0, l[4] != 0, l[5]}; }

extern "C" size_t drv_io_bytes(const slamit_ba_problem* P) { return carve_io(nullptr, P->n_kf, P->n_pt, P->n_edge, P->edge_ur != nullptr).bytes; }

extern "C" int drv_band_ok(int n, int bw) { return ldlt_band_ok(n, bw); }

// io: drv_io_bytes() zeroed bytes; the packed inputs land at its start
extern "C" int drv_plan(const slamit_ba_problem* P, const int32_t* lim, int32_t* fields, double* mflop, int32_t* col, int32_t* new2old,
                        uint8_t* io, size_t* in_bytes) {
    BaWin w;
    memset(&w, 0, sizeof(w));
    BaWindowPlan plan;
    if (!ba_plan_window(*P, limits(lim), w, plan)) return 0;
    const IoLayout H = carve_io(io, P->n_kf, P->n_pt, P->n_edge, P->edge_ur != nullptr);
    ba_pack_inputs(*P, plan, H);
    *in_bytes = H.in_bytes;
    fields_out(w, fields);
    *mflop = plan.exec_mflop;
    memcpy(col, plan.col.data(), sizeof(int32_t) * P->n_kf);
    memcpy(new2old, plan.new2old.data(), sizeof(int32_t) * P->n_pt);
    return 1;
}

// pack, hand the packed poses / points / edge weights / a state back as the outputs, unpack into R
extern "C" int drv_round_trip(const slamit_ba_problem* P, const int32_t* lim, slamit_ba_result* R) {
    BaWin w;
    memset(&w, 0, sizeof(w));
    BaWindowPlan plan;
    if (!ba_plan_window(*P, limits(lim), w, plan)) return 0;
    std::vector<uint8_t> io(carve_io(nullptr, P->n_kf, P->n_pt, P->n_edge, P->edge_ur != nullptr).bytes, 0);
    const IoLayout H = carve_io(io.data(), P->n_kf, P->n_pt, P->n_edge, P->edge_ur != nullptr);
    ba_pack_inputs(*P, plan, H);
    memcpy(H.out_pose, H.in_pose, sizeof(double) * 12 * P->n_kf);
    memcpy(H.out_pt, H.in_pt, sizeof(double) * 3 * P->n_pt);
    memcpy(H.out_chi2, H.e_w, sizeof(double) * P->n_edge);
    for (int e = 0; e < P->n_edge; ++e) { H.out_flag[e] = (uint8_t)(H.e_kf[e] & 1); H.out_out1[e] = 1; }
    H.out_state->n_its[0] = 5; H.out_state->n_its[1] = 7; H.out_state->chi2_init[1] = 2.5; H.out_state->trials[1][6] = 3;
    ba_unpack_outputs(*P, plan, H, *R);
    return 1;
}
'''


def build_plan_lib(tmp, sources):
    """g++ the planner (or another translation unit that exports the driver's functions) with DRIVER into a shared library."""
    drv = os.path.join(tmp, "plan_driver.cc")
    with open(drv, "w") as f:
        f.write(DRIVER)
    so = os.path.join(tmp, "libplan_driver.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                           drv] + list(sources) + ["-o", so])
    L = C.CDLL(so)
    L.drv_io_bytes.restype = C.c_size_t
    L.drv_plan.restype = C.c_int
    return L


@pytest.fixture(scope="module")
def plib(tmp_path_factory):
    return build_plan_lib(str(tmp_path_factory.mktemp("ba_plan")), [os.path.join(CSRC, "ba_plan.cc")])


def _ptr(a):
    return C.c_void_p(a.ctypes.data)


def npad_max(max_kf):
    return -(-(6 * max_kf + 1) // BA_TILE) * BA_TILE


def limits(max_kf=64, nwin=1, keep_order=0, no_sf=0, no_band=0, sf_cap=0):
    return np.array([npad_max(max_kf), nwin, keep_order, no_sf, no_band, sf_cap], np.int32)


def plan(L, prob, lim):
    """-> dict of the structural fields (per-row arrays trimmed to their used length), exec_mflop, col, new2old, packed input bytes;
    None when the planner rejects the window."""
    from weiner_slamit_v2_amd import api

    p, keep = api._ba_problem(prob)
    fields = np.zeros(NFIELDS, np.int32)
    col = np.zeros(max(p.n_kf, 1), np.int32)
    new2old = np.zeros(max(p.n_pt, 1), np.int32)
    io = np.zeros(L.drv_io_bytes(C.byref(p)), np.uint8)
    mflop, in_bytes = C.c_double(), C.c_size_t()
    if not L.drv_plan(C.byref(p), _ptr(lim), _ptr(fields), C.byref(mflop), _ptr(col), _ptr(new2old), _ptr(io), C.byref(in_bytes)):
        return None
    out, i = {}, 0
    for k in SCALARS:
        out[k] = int(fields[i])
        i += 1
    for k, n in ARRAYS:
        out[k] = fields[i:i + n]
        i += n
    T, npanel, G = out["Npad"] // BA_TILE, -(-out["nS"] // 32), out["sf_groups"]
    used = {"tile_alo": T, "tile_ahi": T, "tile_blo": T, "tile_bhi": T, "panel_hi": npanel, "back_lo": npanel,
            "sf_row": G, "sf_k0": G, "sf_k1": G, "sf_glo": out["Npad"] if G else 0, "sf_ghi": out["Npad"] if G else 0}
    for k, _ in ARRAYS:
        out[k] = [int(v) for v in out[k][:used[k]]]
    out["exec_mflop"] = mflop.value
    out["col"] = col[:p.n_kf]
    out["new2old"] = new2old[:p.n_pt]
    out["packed"] = io[:in_bytes.value].tobytes()
    return out


def record(o):
    """What the pin keeps of a plan."""
    r = {k: o[k] for k in SCALARS}
    r.update({k: o[k] for k, _ in ARRAYS})
    r["exec_mflop"] = o["exec_mflop"]
    r["packed_sha256"] = hashlib.sha256(o["packed"]).hexdigest()
    r["new2old_sha256"] = hashlib.sha256(np.ascontiguousarray(o["new2old"], np.int32).tobytes()).hexdigest()
    return r


def pinned_cases():
    """name -> (problem, limits) of every pinned plan."""
    from weiner_slamit_v2_amd import synth

    cases = {}
    for f in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "ba_*.npz"))):
        name = os.path.basename(f)[:-4]
        cases[name] = (load_ba_golden(f)[0], limits())
    cases["synth_50_2000_8"] = (synth.synth_ba(50, 2000, 8), limits())
    cases["synth_50_2000_dense"] = (synth.synth_ba(50, 2000, None), limits())
    for name in ("ba_window8", "ba_shuffled", "ba_stereo_window8"):
        prob = cases[name][0]
        for tag, lim in (("nwin16", limits(nwin=16)), ("keep_order", limits(keep_order=1)), ("no_sf", limits(no_sf=1)),
                         ("no_band", limits(no_band=1)), ("sf_cap2", limits(sf_cap=2))):
            cases["%s:%s" % (name, tag)] = (prob, lim)
    return cases


def shuffled_keyframes(prob, seed):
    """The same window with its keyframes listed in a random order."""
    perm = np.random.RandomState(seed).permutation(len(prob["kf_fixed"]))   # new keyframe i = old keyframe perm[i]
    inv = np.argsort(perm).astype(np.int32)
    q = dict(prob)
    for k in ("kf_pose", "kf_fixed", "kf_intr", "kf_bf"):
        if k in prob:
            q[k] = prob[k][perm]
    q["edge_kf"] = inv[prob["edge_kf"]]
    return q


def property_cases():
    from weiner_slamit_v2_amd import synth

    cases = pinned_cases()
    for s in range(4):
        rs = np.random.RandomState(100 + s)
        n_kf = int(rs.randint(3, 40))
        prob = synth.synth_ba(n_kf, int(rs.randint(20, 600)), int(rs.randint(2, 10)), seed=200 + s, n_fixed=int(rs.randint(0, 3)),
                              stereo_frac=0.5 * (s % 2))
        cases["random%d" % s] = (prob, limits())
        cases["random%d:shuffled" % s] = (shuffled_keyframes(prob, 300 + s), limits())
    return cases


def test_plan_matches_the_pinned_record(plib):
    want = json.load(open(GOLDEN))["cases"]
    cases = pinned_cases()
    assert sorted(want) == sorted(cases)
    for name, (prob, lim) in cases.items():
        got, ref = record(plan(plib, prob, lim)), want[name]
        assert got["exec_mflop"] == pytest.approx(ref["exec_mflop"], rel=1e-12, abs=0), name
        for k in ref:
            if k != "exec_mflop":
                assert got[k] == ref[k], (name, k)


def _point_columns(prob, col):
    n_pt = len(prob["pt_xyz"])
    c = col[prob["edge_kf"]]
    free = c >= 0
    minc = np.full(n_pt, np.iinfo(np.int32).max, np.int64)
    maxc = np.full(n_pt, -1, np.int64)
    np.minimum.at(minc, prob["edge_pt"][free], c[free])
    np.maximum.at(maxc, prob["edge_pt"][free], c[free])
    return minc, maxc


def _coupled_columns(prob, col, nfree):
    """nfree x nfree: free columns a, b share a point"""
    seen = np.zeros((len(prob["pt_xyz"]), max(nfree, 1)), bool)
    c = col[prob["edge_kf"]]
    free = c >= 0
    seen[prob["edge_pt"][free], c[free]] = True
    s = seen.astype(np.int64)
    return (s.T @ s) > 0


def test_plan_properties(plib):
    for name, (prob, lim) in property_cases().items():
        o = plan(plib, prob, lim)
        nfree, nS, Npad, Kpad = o["n_free"], o["nS"], o["Npad"], o["Kpad"]
        n_pt = len(prob["pt_xyz"])
        # the device point order: a permutation, sorted by (first, last) free column
        n2o = np.asarray(o["new2old"])
        assert sorted(n2o.tolist()) == list(range(n_pt)), name
        minc, maxc = _point_columns(prob, o["col"])
        key = list(zip(minc[n2o].tolist(), maxc[n2o].tolist()))
        assert key == sorted(key), name
        o2n = np.argsort(n2o)
        # every non-zero of the Schur operand GA (pose row 6 c + d, point column 3 pn + j) lies in its tile's k range, as A and B operand
        c = o["col"][prob["edge_kf"]]
        free = c >= 0
        for cc, pn in set(zip(c[free].tolist(), o2n[prob["edge_pt"][free]].tolist())):
            for t in {(6 * cc) // BA_TILE, (6 * cc + 5) // BA_TILE}:
                assert o["tile_alo"][t] <= 3 * pn and 3 * pn + 3 <= o["tile_ahi"][t], (name, cc, pn)
                assert o["tile_blo"][t] <= 3 * pn and 3 * pn + 3 <= o["tile_bhi"][t], (name, cc, pn)
        if nS:
            assert (o["tile_blo"][nS // BA_TILE], o["tile_bhi"][nS // BA_TILE]) == (0, Kpad), name   # the right-hand side's row: every point
        # floating groups: consecutive slabs in row order, each group's rows within BA_SF_ROWS of its first
        G = o["sf_groups"]
        for g in range(G):
            assert o["sf_k0"][g] < o["sf_k1"][g] and (g == 0 or o["sf_k1"][g - 1] <= o["sf_k0"][g]), (name, g)
            assert g == 0 or o["sf_row"][g - 1] <= o["sf_row"][g], (name, g)
            for pn in range(o["sf_k0"][g] * BA_KC // 3, min(-(-o["sf_k1"][g] * BA_KC // 3), n_pt)):
                po = n2o[pn]
                if maxc[po] >= 0:
                    assert o["sf_row"][g] <= 6 * minc[po] and 6 * maxc[po] + 5 < o["sf_row"][g] + BA_SF_ROWS, (name, g, pn)
        # the LDLt row envelope covers every coupled row: entry (row block a, column block b), b <= a
        cp = _coupled_columns(prob, o["col"], nfree)
        for a, b in zip(*np.nonzero(np.tril(cp[:nfree, :nfree]))):
            assert o["band"] >= min(6 * a + 5 - 6 * b, nS - 1), (name, a, b)
            for x in range(6):
                assert o["panel_hi"][(6 * b + x) // 32] >= 6 * a + 5, (name, a, b)
                assert o["back_lo"][(6 * a + x) // 32] <= 6 * b, (name, a, b)
        # the solver: banded exactly when its LDS image takes the band and the switch allows it
        assert (o["solver"] == BA_SOLVER_BAND) == (bool(plib.drv_band_ok(nS, o["band"])) and not lim[4]), name
        # a renumbering never widens the band
        if not lim[2]:
            kept = lim.copy()
            kept[2] = 1
            assert o["band"] <= plan(plib, prob, kept)["band"], name


def test_round_trip_restores_the_callers_order(plib):
    from weiner_slamit_v2_amd import api

    cases = property_cases()
    reordered = 0
    for name in ("ba_shuffled", "ba_stereo_window8", "random1:shuffled", "random2:shuffled"):
        prob, lim = cases[name]
        p, keep = api._ba_problem(prob)
        r, out, st = api.Optimizer._result(p.n_kf, p.n_pt, p.n_edge)
        assert plib.drv_round_trip(C.byref(p), _ptr(lim), C.byref(r))
        assert np.array_equal(out["kf_pose"], keep["kf_pose"].reshape(-1, 12)), name
        assert np.array_equal(out["pt_xyz"], keep["pt_xyz"].reshape(-1, 3)), name
        assert np.array_equal(out["edge_chi2"], keep["edge_inv_sigma2"]), name
        assert np.array_equal(out["edge_outlier"], keep["edge_kf"] & 1) and np.all(out["edge_stage1_outlier"] == 1), name
        reordered += not np.array_equal(plan(plib, prob, lim)["new2old"], np.arange(p.n_pt))
        s = api.Optimizer._stats(st)
        assert s["n_its"] == [5, 7] and s["chi2_init"] == [0.0, 2.5] and list(s["trials"][1]) == [0] * 6 + [3], name
    assert reordered   # (the points went through the device order and back)


def test_out_of_range_edge_index_is_rejected(plib):
    from weiner_slamit_v2_amd import synth

    prob = synth.synth_ba(6, 60, 4, seed=3)
    assert plan(plib, prob, limits()) is not None
    for key, bad in (("edge_kf", 6), ("edge_kf", -1), ("edge_pt", 60), ("edge_pt", -2)):
        q = dict(prob)
        q[key] = prob[key].copy()
        q[key][17] = bad
        assert plan(plib, q, limits()) is None, (key, bad)
