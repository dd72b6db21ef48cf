"""The banded pyramid's host plan (csrc/orb_plan.cc: orb_plan_band_segment and the segments orb_plan chooses) on the CPU: which
rows of which level a (frame, band) workgroup of pyramid_bands_kernel computes and stores.  The kernel reads a source row of a level
>= the segment's second from the band's LDS tile of the level below WITHOUT a bounds check, so everything it relies on is checked
here against the row tables it uses."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import ROOT
from weiner_slamit_v2_amd import api

CSRC = os.path.join(ROOT, "weiner_slamit_v2_amd", "csrc")
LDS_BUDGET = 78 * 1024   # ORB_BAND_LDS_BUDGET
SLACK = 16               # ORB_BAND_SLACK

DRIVER = r'''
#include <string.h>
#include <vector>
#include "orb_plan.h"

static OrbPlan g_plan;
static OrbBandSeg g_seg;

extern "C" int bnd_budget() { return ORB_BAND_LDS_BUDGET; }
extern "C" int bnd_slack() { return ORB_BAND_SLACK; }
// 0: refused by orb_plan; else the number of levels
extern "C" int bnd_plan(const slamit_orb_params* p) {
    const char* w = "";
    return orb_plan(*p, OrbPlanOptions{false}, g_plan, &w) ? (int)g_plan.levels.size() : 0;
}
extern "C" int bnd_nsegs() { return (int)g_plan.bands.size(); }
extern "C" void bnd_level(int l, int32_t* o) { o[0] = g_plan.levels[l].w; o[1] = g_plan.levels[l].h; o[2] = g_plan.band_tab.lv[l].pitch; o[3] = g_plan.band_tab.lv[l].ngroups; }
extern "C" const uint32_t* bnd_rowtab(int l) { return g_plan.rs[l].row4.data(); }
static void seg_out(const OrbBandSeg& G, int32_t* o, const uint16_t** rows) {
    o[0] = G.first; o[1] = G.last; o[2] = G.nbands; o[3] = G.tile0; o[4] = G.smem;
    *rows = reinterpret_cast<const uint16_t*>(G.rows.data());
}
extern "C" void bnd_seg(int i, int32_t* o, const uint16_t** rows) { seg_out(g_plan.bands[i], o, rows); }
// a segment of the caller's choice over the planned tables; 0 when the planner refuses it
extern "C" int bnd_try(int first, int last, int nbands, size_t budget, int32_t* o, const uint16_t** rows) {
    if (!orb_plan_band_segment(g_plan, first, last, nbands, budget, g_seg)) return 0;
    seg_out(g_seg, o, rows);
    return 1;
}
'''

# 296 x 224 is the smallest 4:3 geometry the planner accepts with 8 levels of scale 1.2 (level 7 must hold one 30 x 30 FAST cell inside its
# 16-pixel border: 62 rows); 200 x 152 is refused (test_small_geometry_is_refused)
GEOMETRIES = [(640, 480), (752, 480), (1241, 376), (1280, 720), (296, 224)]


@pytest.fixture(scope="module")
def blib(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("orb_bands"))
    drv = os.path.join(tmp, "bands_driver.cc")
    with open(drv, "w") as f:
        f.write(DRIVER)
    so = os.path.join(tmp, "libbands_driver.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-I", CSRC, "-I", os.path.join(ROOT, "include"), drv,
                           os.path.join(CSRC, "orb_plan.cc"), "-o", so])
    L = C.CDLL(so)
    L.bnd_rowtab.restype = C.POINTER(C.c_uint32)
    return L


def _plan(L, w, h, nl=8, sf=1.2):
    p = api.OrbParams(1000, sf, nl, 20, 7, w, h, 1)
    return L.bnd_plan(C.byref(p))


def _level(L, l):
    o = (C.c_int32 * 4)()
    L.bnd_level(l, o)
    return dict(w=o[0], h=o[1], pitch=o[2], ngroups=o[3])


def _source_rows(L, l, h):
    """(sy0, sy1) of every row of level l, as the kernel unpacks the row table"""
    t = np.ctypeslib.as_array(L.bnd_rowtab(l), shape=(2 * h,)).reshape(h, 2)[:, 0].astype(np.int64)
    return t & 0xFFFF, t >> 16


def _seg(o, rows):
    first, last, nb, tile0, smem = o[0], o[1], o[2], o[3], o[4]
    r = np.ctypeslib.as_array(rows, shape=(nb * (last - first) * 4,)).reshape(nb, last - first, 4).astype(np.int64).copy()
    return dict(first=first, last=last, nbands=nb, tile0=tile0, smem=smem, rows=r)   # rows[band][l - first - 1] = own0, own1, cmp0, cmp1


def _planned_segments(L):
    out = []
    for i in range(L.bnd_nsegs()):
        o, rows = (C.c_int32 * 5)(), C.POINTER(C.c_uint16)()
        L.bnd_seg(i, o, C.byref(rows))
        out.append(_seg(o, rows))
    return out


def _try(L, first, last, nbands, budget):
    o, rows = (C.c_int32 * 5)(), C.POINTER(C.c_uint16)()
    if not L.bnd_try(first, last, nbands, C.c_size_t(budget), o, C.byref(rows)):
        return None
    return _seg(o, rows)


def _check_segment(L, G, budget):
    first, last, nb, R = G["first"], G["last"], G["nbands"], G["rows"]
    tiles = [G["tile0"], G["smem"] - G["tile0"]]
    assert G["tile0"] % 16 == 0 and G["smem"] % 16 == 0 and G["smem"] <= budget
    for l in range(first + 1, last + 1):
        V, k = _level(L, l), l - first - 1
        own0, own1, cmp0, cmp1 = R[:, k, 0], R[:, k, 1], R[:, k, 2], R[:, k, 3]
        # owned ranges: [0, h) exactly once, in band order, none empty
        assert own0[0] == 0 and own1[-1] == V["h"] and (own0[1:] == own1[:-1]).all() and (own1 > own0).all(), l
        # computed ranges hold the owned ones and stay inside the level
        assert (cmp0 <= own0).all() and (own1 <= cmp1).all() and (cmp0 >= 0).all() and (cmp1 <= V["h"]).all(), l
        if l == last:
            assert (cmp0 == own0).all() and (cmp1 == own1).all()   # nothing reads the last level: no halo
        # every source row of every computed row lies in the band's computed rows of the level below ([0, h) of the source plane
        # for the segment's first level, which is read from HBM)
        sy0, sy1 = _source_rows(L, l, V["h"])
        hs = _level(L, l - 1)["h"]
        for b in range(nb):
            lo, hi = sy0[cmp0[b]:cmp1[b]].min(), sy1[cmp0[b]:cmp1[b]].max()
            if l == first + 1:
                assert 0 <= lo and hi < hs, (l, b)
            else:
                assert R[b, k - 1, 2] <= lo and hi < R[b, k - 1, 3], (l, b)
        # the tile: whole 8-byte groups in a row, rows on 16-byte boundaries, every computed range (and the slack behind it for the
        # 16-byte window of a row's last group) inside the tile of the level's parity
        assert V["pitch"] % 16 == 0 and V["pitch"] >= 8 * V["ngroups"] >= V["w"]
        if l < last:
            assert ((cmp1 - cmp0) * V["pitch"] + SLACK <= tiles[k & 1]).all(), l
    return True


def test_constants_match_the_header(blib):
    assert (blib.bnd_budget(), blib.bnd_slack()) == (LDS_BUDGET, SLACK)


@pytest.mark.parametrize("w,h", GEOMETRIES)
def test_planned_segments(blib, w, h):
    """The segments a handle gets: between them levels 1 .. 7 once, each segment starting where the one before ended."""
    assert _plan(blib, w, h) == 8
    segs = _planned_segments(blib)
    assert segs, "banded plan expected"
    assert segs[0]["first"] == 0 and segs[-1]["last"] == 7 and all(a["last"] == b["first"] for a, b in zip(segs, segs[1:]))
    for G in segs:
        assert _check_segment(blib, G, LDS_BUDGET)
    if (w, h) == (640, 480):   # the benchmark's geometry: 8 bands, two workgroups and more per CU
        assert [G["nbands"] for G in segs] == [8] * len(segs) and max(G["smem"] for G in segs) <= 64 * 1024


@pytest.mark.parametrize("w,h", GEOMETRIES)
@pytest.mark.parametrize("first,last,nbands", [(0, 7, 8), (0, 7, 5), (0, 3, 8), (3, 7, 8), (2, 5, 3), (0, 7, 1), (6, 7, 16)])
def test_any_segment_the_planner_accepts_holds_the_rules(blib, w, h, first, last, nbands):
    assert _plan(blib, w, h) == 8
    G = _try(blib, first, last, nbands, 160 * 1024)
    if G is None:   # refused: then a band's tiles do pass the budget (one band of a whole frame, say)
        assert _try(blib, first, last, nbands, 64 << 20)["smem"] > 160 * 1024
        return
    assert (G["first"], G["last"], G["nbands"]) == (first, last, nbands)
    assert _check_segment(blib, G, 160 * 1024)


def test_refuses_rather_than_truncates(blib):
    assert _plan(blib, 640, 480) == 8
    G = _try(blib, 0, 7, 8, LDS_BUDGET)
    assert G is not None
    assert _try(blib, 0, 7, 8, G["smem"]) is not None       # fits exactly
    assert _try(blib, 0, 7, 8, G["smem"] - 1) is None       # one byte short: refused, not shortened
    assert _try(blib, 0, 7, 1, LDS_BUDGET) is None          # a whole frame in one band
    assert _try(blib, 0, 7, 135, 160 * 1024) is None        # more bands than level 7 has rows (134)
    assert _try(blib, 0, 8, 8, LDS_BUDGET) is None and _try(blib, 3, 3, 8, LDS_BUDGET) is None   # no such levels
    # 2000 x 2000: level 1 rows are 1,672 bytes; the handle gets thinner bands, never a cut range
    assert _plan(blib, 2000, 2000) == 8
    for G in _planned_segments(blib):
        assert _check_segment(blib, G, LDS_BUDGET)


def test_no_banded_plan_without_rows8_tables(blib):
    """Scale factor 1.5: the sixteen taps of eight pixels do not fit one 16-byte window, the levels keep the four-pixel kernel."""
    assert _plan(blib, 640, 480, nl=3, sf=1.5) == 3
    assert blib.bnd_nsegs() == 0


def test_small_geometry_is_refused(blib):
    assert _plan(blib, 200, 152) == 0   # level 7 would be 56 x 42: smaller than one FAST cell
    assert _plan(blib, 296, 224) == 8
