"""CPU: the plan of BA windows beyond 85 keyframes (csrc/ba_plan.cc built with g++): the tiled solver kind exactly past k_ldlt_blocked's
LDS panel (Npad > 512), the side table of structure past BaWin's inline arrays, the row envelope the tiled LDLt skips by (a numpy model),
the synth_map geometry, and the slamit_ba_create_ex declaration."""
import ctypes as C
import gzip
import json
import os
import zlib
import re
import subprocess

import numpy as np
import pytest

from tests.helpers import ROOT
from weiner_slamit_v2_amd import api, synth

CSRC = os.path.join(ROOT, "weiner_slamit_v2_amd", "csrc")
BA_SOLVER_BAND, BA_SOLVER_BLOCKED, BA_SOLVER_TILED = 0, 1, 2

DRIVER = r'''
#include <string.h>
#include "ba_plan.h"

// out: nS, Npad, solver, side words, side needed, sf_groups | the side table | inline tile_alo/ahi/blo/bhi (10 each), panel_hi/back_lo (20 each) | col
extern "C" int drv_large_plan(const slamit_ba_problem* P, int npad_max, int32_t* out, int cap) {
    BaWin w;
    memset(&w, 0, sizeof(w));
    BaWindowPlan plan;
    if (!ba_plan_window(*P, BaPlanLimits{npad_max, 1, false, false, false, 0}, w, plan)) return 0;
    const int need = 6 + (int)plan.side.size() + 80 + P->n_kf;
    if (need > cap) return -need;
    int32_t* o = out;
    *o++ = w.nS; *o++ = w.Npad; *o++ = w.solver; *o++ = (int32_t)plan.side.size(); *o++ = ba_side_needed(w.Npad, w.nS); *o++ = w.sf_groups;
    for (int32_t v : plan.side) *o++ = v;
    for (int t = 0; t < 10; ++t) *o++ = w.tile_alo[t];
    for (int t = 0; t < 10; ++t) *o++ = w.tile_ahi[t];
    for (int t = 0; t < 10; ++t) *o++ = w.tile_blo[t];
    for (int t = 0; t < 10; ++t) *o++ = w.tile_bhi[t];
    for (int i = 0; i < 20; ++i) *o++ = w.panel_hi[i];
    for (int i = 0; i < 20; ++i) *o++ = w.back_lo[i];
    for (int k = 0; k < P->n_kf; ++k) *o++ = plan.col[k];
    return 1;
}

// packed input bytes of the window with and without its side table; returns the offset of the side table (0: none)
extern "C" size_t drv_large_pack(const slamit_ba_problem* P, uint8_t* io, size_t* in_bytes) {
    BaWin w;
    memset(&w, 0, sizeof(w));
    BaWindowPlan plan;
    if (!ba_plan_window(*P, BaPlanLimits{2048, 1, false, false, false, 0}, w, plan)) return 0;
    const IoLayout H = carve_io(io, P->n_kf, P->n_pt, P->n_edge, P->edge_ur != nullptr, ba_io_side_words(*P));
    ba_pack_inputs(*P, plan, H);
    *in_bytes = H.in_bytes;
    return H.side ? (size_t)((uint8_t*)H.side - io) : 0;
}

extern "C" size_t drv_large_io_bytes(const slamit_ba_problem* P) {
    return carve_io(nullptr, P->n_kf, P->n_pt, P->n_edge, P->edge_ur != nullptr, ba_io_side_words(*P)).bytes;
}
'''

# the windows of the large-BA GPU tests and their reference-g2o fixture (tools/gen_ba_large_golden.py)
REF = json.loads(gzip.open(os.path.join(ROOT, "tests", "golden", "ba_large_ref.json.gz")).read())["cases"]
WINDOWS = {name: c["synth_map"] for name, c in REF.items()}


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("ba_large_plan"))
    drv = os.path.join(tmp, "drv.cc")
    with open(drv, "w") as f:
        f.write(DRIVER)
    so = os.path.join(tmp, "libdrv.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                           drv, os.path.join(CSRC, "ba_plan.cc"), "-o", so])
    L = C.CDLL(so)
    L.drv_large_pack.restype = C.c_size_t
    L.drv_large_io_bytes.restype = C.c_size_t
    return L


@pytest.fixture(scope="module")
def maps():
    return {name: synth.synth_map(**kw) for name, kw in WINDOWS.items()}


def plan(L, prob, npad_max=2048):
    p, keep = api._ba_problem(prob)
    out = np.zeros(200000, np.int32)
    assert L.drv_large_plan(C.byref(p), npad_max, out.ctypes.data_as(C.c_void_p), len(out)) == 1
    nS, Npad, solver, nside, needed, G = (int(v) for v in out[:6])
    side = out[6:6 + nside]
    inl = out[6 + nside:6 + nside + 80]
    T, P = Npad // 64, max(-(-nS // 32), 1)
    return {"nS": nS, "Npad": Npad, "solver": solver, "needed": bool(needed), "sf_groups": G, "T": T, "P": P,
            "alo": side[:T], "ahi": side[T:2 * T], "blo": side[2 * T:3 * T], "bhi": side[3 * T:4 * T],
            "panel_hi": side[4 * T:4 * T + P], "back_lo": side[4 * T + P:4 * T + 2 * P],
            "inline": (inl[:10], inl[10:20], inl[20:30], inl[30:40], inl[40:60], inl[60:80]),
            "col": out[6 + nside + 80:6 + nside + 80 + len(prob["kf_fixed"])].copy()}


def test_solver_kind_is_tiled_exactly_past_512_rows(lib, maps):
    want = {"fixed150": 128, "stereo_fixed70": 128, "free90": 576, "sparse100": 640, "global150": 896, "global300": 1856}
    assert sorted(want) == sorted(maps)
    for name, npad in want.items():
        o = plan(lib, maps[name])
        assert o["Npad"] == npad, name
        assert (o["solver"] == BA_SOLVER_TILED) == (o["Npad"] > 512), name
        assert o["needed"] == (o["Npad"] > 640), name   # the side table travels only past BaWin's inline arrays
        if o["Npad"] > 640:
            assert o["sf_groups"] == 0, name             # floating windows only within sf_glo / sf_ghi's 640 rows
    # narrow bands past 512 rows (points seen by 2 .. 4 consecutive keyframes): ldlt_band_ok alone would admit them to the banded
    # kernel, whose LDS (bak_ldlt_smem of their Npad) no longer fits a CU -- the tiled solve takes them
    extra = [synth.synth_map(150, 1500, 2, 1, seed=1), synth.synth_map(90, 900, 3, 0, seed=2, loop=False),
             synth.synth_map(100, 1000, 4, 10, seed=3, loop=False)]
    extra += [synth.synth_ba(n_kf, 30 * n_kf, 3, seed=n_kf) for n_kf in (60, 85, 86, 95, 120)]
    kinds = set()
    for prob in extra:
        o = plan(lib, prob)
        kinds.add(o["solver"])
        assert (o["solver"] == BA_SOLVER_TILED) == (o["Npad"] > 512), o["Npad"]
        assert o["solver"] == BA_SOLVER_TILED or o["Npad"] <= 512
    assert BA_SOLVER_BAND in kinds and BA_SOLVER_TILED in kinds   # (the rule is exercised on both sides of 512 rows)


def test_fixture_problems_are_what_synth_map_makes(maps):
    for name, prob in maps.items():
        got = {k: zlib.crc32(np.ascontiguousarray(prob[k]).tobytes()) for k in REF[name]["crc32"]}
        assert got == REF[name]["crc32"], name
        assert ("edge_ur" in prob) == ("edge_ur" in REF[name]["crc32"]), name


def test_side_table_equals_the_inline_arrays(lib, maps):
    probs = [maps["fixed150"], maps["stereo_fixed70"], synth.synth_ba(50, 2000, 8), synth.synth_ba(85, 3000, 10, seed=3)]
    for prob in probs + [maps["free90"], maps["global150"]]:
        o = plan(lib, prob)
        alo, ahi, blo, bhi, phi, blo_ = o["inline"]
        t = min(o["T"], 10)
        p = min(o["P"], 20)
        assert np.array_equal(o["alo"][:t], alo[:t]) and np.array_equal(o["ahi"][:t], ahi[:t])
        assert np.array_equal(o["blo"][:t], blo[:t]) and np.array_equal(o["bhi"][:t], bhi[:t])
        assert np.array_equal(o["panel_hi"][:p], phi[:p]) and np.array_equal(o["back_lo"][:p], blo_[:p])
        # the envelope: every panel reaches at least its own rows, and no further than the matrix
        n = o["nS"]
        for i in range(o["P"]):
            if 32 * i < n:
                assert min(32 * i + 31, n - 1) <= o["panel_hi"][i] <= n - 1
                assert 0 <= o["back_lo"][i] <= 32 * i


def test_packing_carries_the_side_table_only_past_the_inline_arrays(lib, maps):
    for name in ("fixed150", "global150"):
        p, keep = api._ba_problem(maps[name])
        io = np.zeros(lib.drv_large_io_bytes(C.byref(p)), np.uint8)
        n_in = C.c_size_t()
        off = lib.drv_large_pack(C.byref(p), io.ctypes.data_as(C.c_void_p), C.byref(n_in))
        o = plan(lib, maps[name])
        if name == "fixed150":
            assert off == 0
        else:
            nside = 4 * o["T"] + 2 * o["P"]
            side = io[off:off + 4 * nside].view(np.int32)
            assert np.array_equal(side, np.concatenate([o["alo"], o["ahi"], o["blo"], o["bhi"], o["panel_hi"], o["back_lo"]]))
            assert off + 4 * nside <= n_in.value


def _reduced_pattern(prob, col, nfree):
    """Free-keyframe coupling of the reduced system (block (a, b) non-zero when a point is seen from both) in the plan's column order."""
    vis = {}
    for k, p in zip(prob["edge_kf"], prob["edge_pt"]):
        c = col[k]
        if c >= 0:
            vis.setdefault(int(p), set()).add(int(c))
    B = np.zeros((nfree, nfree), bool)
    for cs in vis.values():
        cs = sorted(cs)
        B[np.ix_(cs, cs)] = True
    return B


def test_envelope_model_global300(lib, maps):
    """LDLt without pivoting of a random SPD matrix with global300's structure, tiled as k_ldlt_tiled_* does (32-column panels, rows
    to panel_hi only, back-substitution from back_lo): equal to the dense LDLt to rounding, and what it skips is exactly zero there."""
    prob = maps["global300"]
    o = plan(lib, prob)
    n, P = o["nS"], o["P"]
    nfree = n // 6
    B = _reduced_pattern(prob, o["col"], nfree)
    rs = np.random.RandomState(7)
    mask = np.kron(B, np.ones((6, 6), bool))
    A = rs.standard_normal((n, n)) * mask
    A = 0.5 * (A + A.T) + np.diag(np.abs(A).sum(1) + 1.0)
    b = rs.standard_normal(n)
    # dense reference: LDLt from the Cholesky factor
    Lc = np.linalg.cholesky(A)
    d = np.diag(Lc) ** 2
    Ld = Lc / np.diag(Lc)
    # the tiled model: right-looking, panels of 32, rows past panel_hi untouched; the right-hand side as the extra row
    M = np.zeros((n + 1, n + 1))
    M[:n, :n] = A
    M[n, :n] = b
    Lt = np.eye(n)
    D = np.zeros(n)
    for i in range(P):
        jb = 32 * i
        pe = min(jb + 32, n)
        hi = int(o["panel_hi"][i])
        blk = M[jb:pe, jb:pe].copy()
        Lb = np.linalg.cholesky(blk)
        Db = np.diag(Lb) ** 2
        L11 = Lb / np.diag(Lb)
        rows = list(range(pe, hi + 1)) + [n]
        Wr = np.linalg.solve(L11, M[rows, jb:pe].T).T   # w = a L11^-T
        L21 = Wr / Db
        D[jb:pe] = Db
        Lt[jb:pe, jb:pe] = L11
        Lt[pe:hi + 1, jb:pe] = L21[:-1]
        M[rows, jb:pe] = L21
        cols = list(range(pe, hi + 1))
        M[np.ix_(rows, cols)] -= L21 @ (L21[:-1] * Db).T
        # rows past the envelope: exactly zero in the dense factor (LDLt without pivoting never fills there)
        assert not Ld[hi + 1:, jb:pe].any(), i
    assert np.allclose(Lt, Ld, rtol=0, atol=1e-10)
    assert np.allclose(D, d, rtol=1e-10)
    # back-substitution from back_lo: the columns left of it are zero in every row of the panel
    y = M[n, :n].copy()
    x = y.copy()
    for i in reversed(range(P)):
        jb, pe = 32 * i, min(32 * i + 32, n)
        lo = int(o["back_lo"][i])
        assert not Ld[jb:pe, :lo].any(), i
        x[jb:pe] = np.linalg.solve(Lt[jb:pe, jb:pe].T, x[jb:pe])
        x[lo:jb] -= Lt[jb:pe, lo:jb].T @ x[jb:pe]
    assert np.allclose(x, np.linalg.solve(A, b), rtol=1e-8, atol=1e-10)


def test_synth_map_geometry(maps):
    for name, prob in maps.items():
        tp, P = prob["truth_pose"], prob["truth_pt"]
        R = tp[:, :9].reshape(-1, 3, 3)
        t = tp[:, 9:]
        Xc = np.einsum("eij,ej->ei", R[prob["edge_kf"]], P[prob["edge_pt"]]) + t[prob["edge_kf"]]
        assert (Xc[:, 2] > 0).all(), name
        fx, fy, cx, cy = synth.INTRINSICS
        u, v = fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy
        assert ((u >= 0) & (u < 640) & (v >= 0) & (v < 480)).all(), name
        assert ((prob["edge_uv"][:, 0] >= 0) & (prob["edge_uv"][:, 0] < 640)).all(), name
        assert ((prob["edge_uv"][:, 1] >= 0) & (prob["edge_uv"][:, 1] < 480)).all(), name
        assert np.bincount(prob["edge_pt"]).min() >= 2, name
        n_kf = len(prob["kf_fixed"])
        # the loop closes: some point is seen from both the first and the last tenth of the trajectory
        first = {int(p) for k, p in zip(prob["edge_kf"], prob["edge_pt"]) if k < n_kf // 10}
        last = {int(p) for k, p in zip(prob["edge_kf"], prob["edge_pt"]) if k >= n_kf - n_kf // 10}
        assert first & last, name
        assert int(prob["kf_fixed"].sum()) == WINDOWS[name]["n_fixed"], name
    a, b = synth.synth_map(**WINDOWS["global150"]), maps["global150"]
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    arc = synth.synth_map(60, 400, 6, 1, seed=3, loop=False)
    first = {int(p) for k, p in zip(arc["edge_kf"], arc["edge_pt"]) if k < 6}
    last = {int(p) for k, p in zip(arc["edge_kf"], arc["edge_pt"]) if k >= 54}
    assert not first & last


def test_create_ex_is_declared_and_exported():
    h = open(os.path.join(ROOT, "include", "slamit.h")).read()
    assert re.search(r"int slamit_ba_create_ex\(int max_kf, int max_free_kf, int max_pt, int max_edge, int max_batch, int device,\s*slamit_ba\*\* out\);", h)
    assert re.search(r"#define SLAMIT_BA_MAX_FREE_KF 341\b", h)
    assert "slamit_ba_create_ex" in api.EXPORTS
    types = open(os.path.join(CSRC, "ba_types.h")).read()
    assert re.search(r"#define BA_MAX_FREE_KF 341\b", types) and re.search(r"#define BA_NPAD_CEIL 2048\b", types)
