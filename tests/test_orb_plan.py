"""The host-side plan of an ORB extractor handle (csrc/orb_plan.cc) on the CPU: orb_plan.cc is built with g++ together with a small
C driver, and the plan is compared to a pinned record (tests/golden/orb_plans.json), to the ORB oracle, and to the rules the
kernels rely on."""
import ctypes as C
import hashlib
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from oracle import bindings as ob
from tests.helpers import ROOT
from weiner_slamit_v2_amd import api, synth

CSRC = os.path.join(ROOT, "weiner_slamit_v2_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "orb_plans.json")

# The plan as named sections (name, NUL, u64 size, bytes); the tables as the planner holds them.
DRIVER = r'''
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include "orb_plan.h"

static std::vector<uint8_t> g_blob;
static void put(const std::string& name, const void* p, size_t n) {
    g_blob.insert(g_blob.end(), name.begin(), name.end());
    g_blob.push_back(0);
    const uint64_t k = n;
    g_blob.insert(g_blob.end(), (const uint8_t*)&k, (const uint8_t*)&k + 8);
    if (n) g_blob.insert(g_blob.end(), (const uint8_t*)p, (const uint8_t*)p + n);
}
template <typename V> static void put_vec(const std::string& name, const V& v) { put(name, v.data(), sizeof(v[0]) * v.size()); }

extern "C" void drv_sizes(int32_t* o) { o[0] = sizeof(OrbLevel); o[1] = sizeof(PyrBox); o[2] = sizeof(FastTab); o[3] = sizeof(PyrTabs); }

// returns 0 with the reason in `why` when the planner refuses p
extern "C" int drv_plan(const slamit_orb_params* p, int no8, char* why, const uint8_t** blob, size_t* n) {
    OrbPlan P;
    const char* w = "";
    g_blob.clear();
    if (!orb_plan(*p, OrbPlanOptions{no8 != 0}, P, &w)) { snprintf(why, 256, "%s", w); return 0; }
    const int nl = (int)P.levels.size();
    const int64_t sc[] = {P.max_out, P.node_cap, P.oct_key_cap, P.max_kp_level, P.max_wcell, P.max_hcell, (int64_t)P.pyr_frame_total,
                          (int64_t)P.blur_frame_total, (int64_t)P.cand_frame_stride, (int64_t)P.kp_frame_stride, P.rows4_ok, P.pyr_regions,
                          P.pyr_bufA, P.pyr_smem};
    put("scalars", sc, sizeof(sc));
    put_vec("levels", P.levels);
    put_vec("scale", P.scale); put_vec("inv_scale", P.inv_scale); put_vec("sigma2", P.sigma2); put_vec("inv_sigma2", P.inv_sigma2);
    put_vec("per_level", P.per_level);
    put_vec("cells", P.cells);
    put("fast", &P.fast, sizeof(P.fast));
    const OrbStrips* S[3] = {&P.blur_all, &P.blur_str, &P.blur_edge};
    const char* sn[3] = {"blur_all", "blur_str", "blur_edge"};
    for (int i = 0; i < 3; ++i) { put_vec(sn[i], S[i]->tab); put(std::string(sn[i]) + "_base", S[i]->base, sizeof(int) * (nl + 1)); }
    std::vector<int64_t> offs = {(int64_t)P.levels_off, (int64_t)P.cells_off, (int64_t)P.blur_all.off, (int64_t)P.blur_str.off,
                                 (int64_t)P.blur_edge.off, (int64_t)P.boxes_off, (int64_t)P.tabs_off, (int64_t)P.table_bytes};
    for (int l = 1; l < nl; ++l) {
        const OrbResizeTabs& T = P.rs[l];
        const std::string s = "/" + std::to_string(l);
        put_vec("xofs" + s, T.xofs); put_vec("ialpha" + s, T.ialpha); put_vec("yofs" + s, T.yofs); put_vec("ibeta" + s, T.ibeta);
        put_vec("col4" + s, T.col4); put_vec("row4" + s, T.row4); put_vec("col8" + s, T.col8);
        for (size_t o : {T.xofs_off, T.ialpha_off, T.yofs_off, T.ibeta_off, T.col4_off, T.row4_off, T.col8_off}) offs.push_back((int64_t)o);
    }
    put_vec("boxes", P.boxes);
    put_vec("offsets", offs);
    std::vector<uint8_t> img;
    orb_plan_image(P, nullptr, img);
    put_vec("image", img);
    *blob = g_blob.data();
    *n = g_blob.size();
    return 1;
}
'''

SCALARS = ("max_out", "node_cap", "oct_key_cap", "max_kp_level", "max_wcell", "max_hcell", "pyr_frame_total", "blur_frame_total",
           "cand_frame_stride", "kp_frame_stride", "rows4_ok", "pyr_regions", "pyr_bufA", "pyr_smem")
RS_TABLES = ("xofs", "ialpha", "yofs", "ibeta", "col4", "row4", "col8")
LEVEL = np.dtype([("w", "<i4"), ("h", "<i4"), ("stride", "<i4"), ("quota", "<i4"), ("plane_off", "<u8"), ("plane_bytes", "<u8"),
                  ("blur_off", "<u8"), ("blur_bytes", "<u8"), ("nCols", "<i4"), ("nRows", "<i4"), ("wCell", "<i4"), ("hCell", "<i4"),
                  ("maxBorderX", "<i4"), ("maxBorderY", "<i4"), ("cell_base", "<i4"), ("ncells", "<i4"), ("blur_tile_base", "<i4"),
                  ("cand_off", "<u8"), ("cand_cap", "<i4"), ("nIni", "<i4"), ("hX", "<f4"), ("rootUL", "<i4", 8), ("rootUR", "<i4", 8),
                  ("boxH", "<i4"), ("kp_off", "<i4"), ("kp_cap", "<i4"), ("scale", "<f4"), ("patch_size", "<f4")], align=True)
BOX = np.dtype([(k, "<i2") for k in ("ox0", "oy0", "ox1", "oy1", "nx0", "ny0", "nx1", "ny1")])
MIN_BORDER = 16

# (name, width, height, nfeatures, scale factor, nlevels, resize_no8)
PINNED = [
    ("vga", 640, 480, 1000, 1.2, 8, 0),
    ("720p", 1280, 720, 2000, 1.2, 8, 0),
    ("odd_317x251", 317, 251, 500, 1.2, 4, 0),
    ("odd_752x480", 752, 480, 1200, 1.2, 8, 0),
    ("odd_640x480_sf1.5", 640, 480, 300, 1.5, 3, 0),
    ("odd_200x340", 200, 340, 400, 1.3, 3, 0),
    ("odd_534x402", 534, 402, 600, 1.2, 8, 0),
    ("odd_535x403", 535, 403, 600, 1.2, 8, 0),
    ("533x401", 533, 401, 1000, 1.2, 8, 0),
    ("2000x2000", 2000, 2000, 1000, 1.2, 8, 0),
    ("vga_sf2.5_nl3", 640, 480, 1000, 2.5, 3, 0),        # rows4 refused; a fourth level would be smaller than one cell
    ("vga_no8", 640, 480, 1000, 1.2, 8, 1),
    ("vga_nl1", 640, 480, 1000, 1.2, 1, 0),
    ("8192x8192_sf2", 8192, 8192, 1000, 2.0, 8, 0),      # accepted, but the fused plan fails (level 7 is 64 rows for 86 regions)
    ("empty", 640, 0, 1000, 1.2, 8, 0),
    ("tiny", 100, 80, 1000, 1.2, 8, 0),                  # refused: top levels smaller than one FAST cell (test_gpu_abi.py)
    ("tall", 100, 400, 1000, 1.2, 2, 0),                 # refused: octree roots
    ("vga_nfeatures_huge", 640, 480, 100000, 1.2, 8, 0), # refused: the LDS octree
]
REFUSALS = {"tiny": "slamit_orb_create: pyramid level smaller than one 30x30 FAST cell",
            "tall": "slamit_orb_create: unsupported aspect ratio (octree roots)",
            "vga_nfeatures_huge": "slamit_orb_create: nfeatures too large for the LDS octree"}


def build_plan_lib(tmp, sources, include=()):
    """g++ the planner (or another translation unit that exports the driver's functions) with DRIVER into a shared library."""
    drv = os.path.join(tmp, "plan_driver.cc")
    with open(drv, "w") as f:
        f.write(DRIVER)
    so = os.path.join(tmp, "libplan_driver.so")
    inc = [a for d in list(include) + [CSRC, os.path.join(ROOT, "include")] for a in ("-I", d)]
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC"] + inc + [drv] + list(sources) + ["-o", so])
    L = C.CDLL(so)
    L.drv_plan.restype = C.c_int
    return L


@pytest.fixture(scope="module")
def plib(tmp_path_factory):
    return build_plan_lib(str(tmp_path_factory.mktemp("orb_plan")), [os.path.join(CSRC, "orb_plan.cc")])


def plan(L, w, h, nf, sf, nl, no8=0):
    """-> {section name: bytes}, or the refusal message (str)."""
    p = api.OrbParams(nf, sf, nl, 20, 7, w, h, 1)
    why = C.create_string_buffer(256)
    blob, n = C.POINTER(C.c_uint8)(), C.c_size_t()
    if not L.drv_plan(C.byref(p), no8, why, C.byref(blob), C.byref(n)):
        return why.value.decode()
    raw = C.string_at(blob, n.value)
    out, i = {}, 0
    while i < len(raw):
        j = raw.index(b"\0", i)
        size = struct.unpack_from("<Q", raw, j + 1)[0]
        out[raw[i:j].decode()] = raw[j + 9:j + 9 + size]
        i = j + 9 + size
    return out


def levels(sec):
    return np.frombuffer(sec["levels"], LEVEL)


def u32(sec, name):
    return np.frombuffer(sec[name], np.uint32)


def record(sec):
    """The pinned form of a plan: scalars, every OrbLevel field, the strip bases, and a sha256 of every table's bytes.  The block
    layout (offsets, image) is checked by test_table_block_holds_every_table, not pinned."""
    if isinstance(sec, str):
        return {"refused": sec}
    sc = struct.unpack("<%dq" % len(SCALARS), sec["scalars"])
    lv = [{k: (v.tolist() if isinstance(v, np.ndarray) else v.item()) for k, v in zip(LEVEL.names, (L[k] for k in LEVEL.names))}
          for L in levels(sec)]
    tables = {k: hashlib.sha256(v).hexdigest() for k, v in sorted(sec.items())
              if k not in ("scalars", "levels", "offsets", "image") and not k.endswith("_base")}
    bases = {k: np.frombuffer(v, np.int32).tolist() for k, v in sec.items() if k.endswith("_base")}
    return {"scalars": dict(zip(SCALARS, sc)), "levels": lv, "bases": bases, "tables": tables}


def test_plan_matches_the_pinned_record(plib):
    golden = json.load(open(GOLDEN))
    assert sorted(golden) == sorted(c[0] for c in PINNED)
    for name, w, h, nf, sf, nl, no8 in PINNED:
        got = record(plan(plib, w, h, nf, sf, nl, no8))
        assert got == golden[name], name


def test_layouts_match_the_driver(plib):
    sizes = (C.c_int32 * 4)()
    plib.drv_sizes(sizes)
    assert (sizes[0], sizes[1]) == (LEVEL.itemsize, BOX.itemsize)


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals(plib, name):
    case = [c for c in PINNED if c[0] == name][0]
    assert plan(plib, *case[1:]) == REFUSALS[name]


@pytest.mark.parametrize("nf,sf,nl", [(1000, 1.2, 8), (2000, 1.2, 8), (500, 1.2, 4), (300, 1.5, 3), (1200, 1.3, 5), (1000, 2.5, 3), (777, 1.1, 12)])
def test_scale_tables_and_quotas_equal_the_oracle(plib, nf, sf, nl):
    """The CPU twin of test_gpu_orb.py::test_tables_match_oracle: bit-equal float tables and quotas."""
    sec = plan(plib, 640, 480, nf, sf, nl)
    t = ob.OrbOracle(nf, sf, nl, 20, 7).tables()
    for k in ("scale", "inv_scale", "sigma2", "inv_sigma2"):
        assert np.frombuffer(sec[k], np.float32).tobytes() == t[k].astype(np.float32).tobytes(), k
    assert np.frombuffer(sec["per_level"], np.int32).tolist() == t["per_level"].tolist()


ACCEPTED = [c for c in PINNED if c[0] not in REFUSALS and c[0] != "empty"]


@pytest.mark.parametrize("case", [c for c in ACCEPTED if c[1] * c[2] <= 2000 * 2000], ids=lambda c: c[0])
def test_level_sizes_equal_the_oracle(plib, case):
    _, w, h, nf, sf, nl, no8 = case
    orc = ob.OrbOracle(nf, sf, nl, 20, 7)
    orc.extract(np.zeros((h, w), np.uint8))
    assert [(int(L["w"]), int(L["h"])) for L in levels(plan(plib, w, h, nf, sf, nl, no8))] == [orc.level_size(l) for l in range(nl)]


def test_empty_image_plans_no_levels_and_no_tables(plib):
    sec = plan(plib, 640, 0, 1000, 1.2, 8)
    assert len(sec["levels"]) == 0 and len(sec["cells"]) == 0 and len(sec["image"]) == 0
    assert all(len(sec[k]) == 0 for k in ("blur_all", "blur_str", "blur_edge", "boxes"))


# ---- resize tables: a numpy interpreter of rs_item / rs_item8 (orb_kernels.hip) -----------------------------------------------

def _vertical(rowtab, hz, dh):
    """hz[source row] -> dst rows: ((b0 * h0 >> 16) + (b1 * h1 >> 16) + 2) >> 2 with the row table's rows and weights."""
    rt = rowtab.reshape(-1, 2)[:dh].astype(np.int64)
    sy0, sy1, b0, b1 = rt[:, 0] & 0xFFFF, rt[:, 0] >> 16, rt[:, 1] & 0xFFFF, rt[:, 1] >> 16
    v = (((b0[:, None] * hz[sy0]) >> 16) + ((b1[:, None] * hz[sy1]) >> 16) + 2) >> 2
    return (v & 0xFF).astype(np.uint8)


def _perm_dot(win, sel, al):
    """v_perm of each group's 8-byte window (selector byte 0x0C reads as zero) as two u16 taps, dot2 with the alpha pair, >> 4."""
    g = np.arange(win.shape[1])
    b = []
    for k in range(4):
        s = (sel >> (8 * k)) & 0xFF
        assert ((s < 8) | (s == 0x0C)).all()
        b.append(np.where(s == 0x0C, 0, win[:, g, np.minimum(s, 7)]))
    lo, hi = b[0] | (b[1] << 8), b[2] | (b[3] << 8)
    return (lo * (al & 0xFFFF) + hi * (al >> 16)) >> 4


def _windows(src, base, nbytes):
    """the nbytes of every source row at byte `base` of each group, past the row end zero (no selector picks those bytes)"""
    pad = np.zeros((src.shape[0], src.shape[1] + 64), np.int64)
    pad[:, :src.shape[1]] = src
    return pad[:, base[:, None] + np.arange(nbytes)[None, :]]


def interp_rows4(src, col, row, dw, dh):
    c = col.reshape(-1, 12).astype(np.int64)
    base, sh = c[:, 0] & 0xFFFF, (c[:, 0] >> 16) & 3
    win = _windows(src, base + sh, 8)   # alignbyte by the shift: the 8 bytes from base + shift
    hz = np.stack([_perm_dot(win, c[:, 1 + j], c[:, 5 + j]) for j in range(4)], 2).reshape(src.shape[0], -1)[:, :dw]
    return _vertical(row, hz, dh)


def interp_rows8(src, col, row, dw, dh):
    c = col.reshape(-1, 20).astype(np.int64)
    base, sh = c[:, 0] & 0xFFFF, (c[:, 0] >> 16) & 3
    win = _windows(src, base + sh, 12)  # pixels 0 .. 3 read bytes 0 .. 7, pixels 4 .. 7 bytes 4 .. 11
    hz = np.stack([_perm_dot(win[:, :, (4 if j >= 4 else 0):][:, :, :8], c[:, 1 + j], c[:, 9 + j]) for j in range(8)], 2)
    return _vertical(row, hz.reshape(src.shape[0], -1)[:, :dw], dh)


@pytest.mark.parametrize("case", [c for c in ACCEPTED if c[1] * c[2] <= 2000 * 2000], ids=lambda c: c[0])
def test_resize_tables_decode_to_cv_resize(plib, case):
    _, w, h, nf, sf, nl, no8 = case
    sec = plan(plib, w, h, nf, sf, nl, no8)
    L = levels(sec)
    prev = synth.synth_frame(w, h, 5)
    checked = 0
    for l in range(1, nl):
        dw, dh = int(L[l]["w"]), int(L[l]["h"])
        ref = ob.resize(prev, dw, dh)
        col4, row4, col8 = (u32(sec, "%s/%d" % (k, l)) for k in ("col4", "row4", "col8"))
        if len(col4):
            assert np.array_equal(interp_rows4(prev, col4, row4, dw, dh), ref), (l, "rows4")
            checked += 1
        if len(col8):
            assert len(row4) and np.array_equal(interp_rows8(prev, col8, row4, dw, dh), ref), (l, "rows8")
            checked += 1
        prev = ref
    scalars = dict(zip(SCALARS, struct.unpack("<%dq" % len(SCALARS), sec["scalars"])))
    assert checked or nl == 1 or not scalars["rows4_ok"]


# ---- properties -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ACCEPTED, ids=lambda c: c[0])
def test_plan_properties(plib, case):
    _, w, h, nf, sf, nl, no8 = case
    sec = plan(plib, w, h, nf, sf, nl, no8)
    L = levels(sec)
    # FAST cells: the reference's visiting order (level, row, column) and its skips (ORBextractor.cc:810,819)
    want = []
    for l, V in enumerate(L):
        for i in range(V["nRows"]):
            iniY = MIN_BORDER + i * V["hCell"]
            if iniY >= V["maxBorderY"] - 3:
                continue
            for j in range(V["nCols"]):
                iniX = MIN_BORDER + j * V["wCell"]
                if iniX >= V["maxBorderX"] - 6:
                    continue
                cw, ch = min(V["wCell"] + 6, V["maxBorderX"] - iniX), min(V["hCell"] + 6, V["maxBorderY"] - iniY)
                g = max((cw - 6 + 3) >> 2, 1)
                want += [l | ((i * V["nCols"] + j) << 8), iniX | (iniY << 16), cw | (ch << 8), (1 << 20) // g + 1]
    assert u32(sec, "cells").tolist() == want
    # blur strips: per level the stream strips and the edge strips are exactly all strips, and the bases agree
    tabs = {k: u32(sec, k).reshape(-1, 4) for k in ("blur_all", "blur_str", "blur_edge")}
    base = {k: np.frombuffer(sec[k + "_base"], np.int32) for k in tabs}
    assert base["blur_all"][:-1].tolist() == L["blur_tile_base"].tolist()
    for l, V in enumerate(L):
        part = {k: tabs[k][base[k][l]:base[k][l + 1]] for k in tabs}
        assert all((t[:, 0] == l).all() for t in part.values())
        every = [(bx, by) for by in range(0, V["h"], 64) for bx in range(0, V["w"], 64)]
        assert [tuple(t) for t in part["blur_all"][:, 1:3].tolist()] == every
        inside = [(bx, by) for bx, by in every if bx >= 4 and bx + 68 <= V["w"]]
        assert [tuple(t) for t in part["blur_str"][:, 1:3].tolist()] == inside
        assert [tuple(t) for t in part["blur_edge"][:, 1:3].tolist()] == [s for s in every if s not in inside]
    # fused pyramid: own boxes tile every level >= 1, need boxes cover the own boxes and what the next level reads
    sc = dict(zip(SCALARS, struct.unpack("<%dq" % len(SCALARS), sec["scalars"])))
    if nl > 1 and w * h <= 2000 * 2000:
        assert sc["pyr_regions"] > 0, "fused plan expected"
    if not sc["pyr_regions"]:
        assert len(sec["boxes"]) == 0
        return
    B = np.frombuffer(sec["boxes"], BOX).reshape(sc["pyr_regions"], nl)
    for l in range(1, nl):
        cover = np.zeros((L[l]["h"], L[l]["w"]), np.int32)
        for b in B[:, l]:
            cover[b["oy0"]:b["oy1"], b["ox0"]:b["ox1"]] += 1
            assert b["nx0"] <= b["ox0"] and b["ox1"] <= b["nx1"] and b["ny0"] <= b["oy0"] and b["oy1"] <= b["ny1"]
        assert (cover == 1).all(), l
        xo, yo = np.frombuffer(sec["xofs/%d" % l], np.int32), np.frombuffer(sec["yofs/%d" % l], np.int32)
        sw, sh = int(L[l - 1]["w"]), int(L[l - 1]["h"])
        for r in range(B.shape[0]):
            b, s = B[r, l], B[r, l - 1]
            x = xo[b["nx0"]:b["nx1"]]
            y = yo[b["ny0"]:b["ny1"]]
            cols = np.concatenate([x, np.minimum(x + 1, sw - 1)])
            rows = np.clip(np.concatenate([y, y + 1]), 0, sh - 1)
            assert s["nx0"] <= cols.min() and cols.max() < s["nx1"] and s["ny0"] <= rows.min() and rows.max() < s["ny1"], (l, r)


@pytest.mark.parametrize("case", ACCEPTED + [c for c in PINNED if c[0] == "empty"], ids=lambda c: c[0])
def test_table_block_holds_every_table(plib, case):
    """Every read-only table sits at its offset in the one block (256-byte aligned, no overlap); PyrTabs hold the offsets of the
    level's xofs / ialpha / yofs / ibeta tables (level 0: none)."""
    _, w, h, nf, sf, nl, no8 = case
    sec = plan(plib, w, h, nf, sf, nl, no8)
    offs, img = np.frombuffer(sec["offsets"], np.int64).tolist(), sec["image"]
    nlv = len(levels(sec))
    named = [("levels", offs[0]), ("cells", offs[1]), ("blur_all", offs[2]), ("blur_str", offs[3]), ("blur_edge", offs[4]),
             ("boxes", offs[5])]
    for l in range(1, nlv):
        named += [("%s/%d" % (k, l), offs[8 + 7 * (l - 1) + i]) for i, k in enumerate(RS_TABLES)]
    spans = []
    for name, off in named:
        n = len(sec[name])
        assert off % 256 == 0 and img[off:off + n] == sec[name], name
        spans.append((off, off + n))
    sc = dict(zip(SCALARS, struct.unpack("<%dq" % len(SCALARS), sec["scalars"])))
    if sc["pyr_regions"]:
        tabs = np.frombuffer(img[offs[6]:offs[6] + 32 * nlv], np.uint64).reshape(nlv, 4)
        assert offs[6] % 256 == 0 and not tabs[0].any()
        for l in range(1, nlv):
            assert tabs[l].tolist() == [offs[8 + 7 * (l - 1) + i] for i in range(4)]
        spans.append((offs[6], offs[6] + 32 * nlv))
    spans = sorted(s for s in spans if s[1] > s[0])
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and (not spans or spans[-1][1] <= offs[7] == len(img))
