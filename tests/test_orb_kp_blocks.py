"""The per-level workgroup table of the orientation and descriptor passes (orb_plan_kp_blocks, csrc/orb_plan.cc) on the CPU:
orb_plan.cc is built with g++ and a small driver, as tests/test_orb_plan.py does, and the table is held to the rule the kernels
rely on: level l owns ceil(kp_cap[l] / per) consecutive workgroups of a frame, and every keypoint slot lies in exactly one."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import ROOT
from tests.test_orb_plan import PINNED, REFUSALS
from weiner_slamit_v2_amd import api

CSRC = os.path.join(ROOT, "weiner_slamit_v2_amd", "csrc")
MAX_LEVELS = 16

DRIVER = r'''
#include "orb_plan.h"

extern "C" void drv_consts(int32_t* o) { o[0] = ORB_MAX_LEVELS; o[1] = ORB_IC_KP_PER_WG; o[2] = ORB_DESC_KP_PER_WG; o[3] = sizeof(KpBlockTab); }

// -> the number of levels, -1 when the planner refuses p, -2 when the table does; first: the table for `per`; ic / desc: the plan's own
extern "C" int drv_kp_blocks(const slamit_orb_params* p, int no8, int per, int32_t* kp_cap, uint16_t* first, uint16_t* ic, uint16_t* desc) {
    OrbPlan P;
    const char* w = "";
    if (!orb_plan(*p, OrbPlanOptions{no8 != 0}, P, &w)) return -1;
    KpBlockTab T;
    if (!orb_plan_kp_blocks(P.levels, per, T)) return -2;
    for (size_t l = 0; l < P.levels.size(); ++l) kp_cap[l] = P.levels[l].kp_cap;
    for (int l = 0; l <= ORB_MAX_LEVELS; ++l) { first[l] = T.first[l]; ic[l] = P.ic_blocks.first[l]; desc[l] = P.desc_blocks.first[l]; }
    return (int)P.levels.size();
}
'''

# (name, width, height, nfeatures, scale factor, nlevels, resize_no8): every geometry of test_orb_plan.py that the planner accepts,
# a plan whose levels are smaller than one workgroup, and one with twelve levels
CASES = [c for c in PINNED if c[0] not in REFUSALS] + [("vga_60", 640, 480, 60, 1.2, 8, 0), ("vga_777_sf1.1_nl12", 640, 480, 777, 1.1, 12, 0)]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("orb_kp_blocks"))
    drv, so = os.path.join(tmp, "kp_blocks_driver.cc"), os.path.join(tmp, "libkp_blocks_driver.so")
    with open(drv, "w") as f:
        f.write(DRIVER)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-I", CSRC, "-I", os.path.join(ROOT, "include"), drv,
                           os.path.join(CSRC, "orb_plan.cc"), "-o", so])
    return C.CDLL(so)


def blocks(lib, case, per):
    """-> (kp_cap per level, first[0 .. 16], the plan's orientation table, the plan's descriptor table)"""
    _, w, h, nf, sf, nl, no8 = case
    p = api.OrbParams(nf, sf, nl, 20, 7, w, h, 1)
    cap = (C.c_int32 * MAX_LEVELS)()
    first, ic, desc = ((C.c_uint16 * (MAX_LEVELS + 1))() for _ in range(3))
    n = lib.drv_kp_blocks(C.byref(p), no8, per, cap, first, ic, desc)
    assert n >= 0, (case[0], n)
    return list(cap)[:n], list(first), list(ic), list(desc)


def test_constants_match_the_driver(lib):
    c = (C.c_int32 * 4)()
    lib.drv_consts(c)
    assert list(c)[:3] == [MAX_LEVELS, 32, 16] and c[3] >= 2 * (MAX_LEVELS + 1)


@pytest.mark.parametrize("per", [16, 32])
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_every_keypoint_slot_has_one_workgroup(lib, case, per):
    cap, first, ic, desc = blocks(lib, case, per)
    nl = len(cap)
    assert nl == (0 if case[0] == "empty" else case[5])
    assert first[0] == 0
    for l in range(nl):
        assert first[l + 1] - first[l] == -(-cap[l] // per), l
        owner = np.zeros(cap[l], np.int32)   # how many workgroups of the level hold slot i
        for kb in range(first[l + 1] - first[l]):
            assert kb * per < cap[l], (l, kb)            # no workgroup starts at or beyond the level's capacity
            owner[kb * per:(kb + 1) * per] += 1
        assert (owner == 1).all(), l
    assert all(f == first[nl] for f in first[nl:])       # behind the last level: the workgroups per frame
    assert (ic if per == 32 else desc) == first          # the plan carries the same two tables


def test_the_walk_of_the_kernels_finds_level_and_block(lib):
    """kp_block_level (orb_kernels.hip) restated: the last level whose first workgroup is not behind `local`."""
    for case in CASES:
        for per in (16, 32):
            cap, first, _, _ = blocks(lib, case, per)
            want = [(l, kb) for l in range(len(cap)) for kb in range(-(-cap[l] // per))]
            got = []
            for local in range(first[MAX_LEVELS]):
                lv = max([0] + [l for l in range(1, MAX_LEVELS) if local >= first[l]])
                got.append((lv, local - first[lv]))
            assert got == want, (case[0], per)


def test_vga_totals(lib):
    vga = [c for c in CASES if c[0] == "vga"][0]
    cap, first32, _, _ = blocks(lib, vga, 32)
    assert cap == [221, 185, 155, 130, 109, 91, 77, 64]
    assert first32[8] == 35 and blocks(lib, vga, 16)[1][8] == 67
    p720 = [c for c in CASES if c[0] == "720p"][0]
    assert blocks(lib, p720, 32)[1][8] == 66 and blocks(lib, p720, 16)[1][8] == 131
