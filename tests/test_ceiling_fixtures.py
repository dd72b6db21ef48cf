"""CPU: the conditions on the inputs of tests/test_gpu_ceilings.py (tests/ceiling_fixtures.py), stated on the references alone.

The pose and Sim3 bars demand identical outlier / inlier flags, and rounding may flip an edge that sits on its chi-square gate: the
seeds are such that, in the oracle's own run, no edge comes within 1e-6 (relative) of the gate at any of the relabellings.  The RANSAC
problems meet tests/sim3_ransac_ref.py's admissibility rule; the triangulation and frustum problems hold every status code their
fixtures hold at working size; the planted BoW and Hamming cases are what the oracle says they are."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import bindings as ob
from tests import ceiling_fixtures as cf
from tests import sim3_ransac_ref as rref
from tests.helpers import ROOT


def test_the_header_states_the_pose_and_sim3_ceilings(tmp_path):
    from weiner_slamit_v2_amd import api

    src = '#include <stdio.h>\n#include "slamit.h"\nint main(void) {\n'
    src += '    printf("%d %d %d %d %d %d %d\\n", SLAMIT_POSE_MAX_N, SLAMIT_SIM3_MAX_N, SLAMIT_FRAME_MAX_KP, SLAMIT_HAMMING_MAX_TRAIN, SLAMIT_BOW_MAX_GROUP,\n'
    src += '           SLAMIT_SIM3_RANSAC_MAX_N, SLAMIT_SIM3_RANSAC_MAX_HYP);\n    return 0;\n}\n'
    c, exe = str(tmp_path / "c.c"), str(tmp_path / "c")
    open(c, "w").write(src)
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
    v = [int(x) for x in subprocess.check_output([exe]).split()]
    assert v == [api.POSE_MAX_N, api.SIM3_MAX_N, api.FRAME_MAX_KP, api.HAMMING_MAX_TRAIN, api.BOW_MAX_GROUP, api.SIM3_RANSAC_MAX_N, api.SIM3_RANSAC_MAX_HYP]
    assert v == [cf.POSE_MAX_N, cf.SIM3_MAX_N, 30000, 65535, cf.BOW_MAX_GROUP, cf.RANSAC_MAX_N, cf.RANSAC_MAX_HYP]
    assert (api.TRIANGULATE_MAX_N, api.FRUSTUM_MAX_N, api.VOC_MAX_FEATURES) == (cf.TRIANGULATE_MAX_N, cf.FRUSTUM_MAX_N, max(cf.KFDB_CAPS))
    # the LDS the ceilings were derived from: n + 16 bytes of flags beside the kernels' static LDS, inside a gfx950 workgroup's 160 KiB
    assert cf.POSE_MAX_N + 16 + 1496 <= 160 * 1024 and cf.SIM3_MAX_N + 16 + 3680 <= 160 * 1024


def test_no_pose_edge_of_the_ceiling_problem_sits_on_its_gate():
    pr, o = cf.pose_ceiling(), cf.pose_oracle("ceiling")
    assert len(pr["inv_sigma2"]) == cf.POSE_MAX_N and len(o["gate_margin"]) == cf.POSE_MAX_N
    print("pose ceiling: least gate margin %.3e, %d inliers, iterations %s" % (o["gate_margin"].min(), o["n_inliers"], o["n_its"]))
    assert o["gate_margin"].min() > cf.GATE_BAND
    assert all(n > 0 for n in o["n_its"]) and 0.7 * cf.POSE_MAX_N < o["n_inliers"] < cf.POSE_MAX_N      # both kinds of edge, every round iterates
    plain = ob.pose_solve(pr)                                                                              # the margins change nothing
    assert np.array_equal(plain["pose"], o["pose"]) and np.array_equal(plain["outlier"], o["outlier"])


def test_no_sim3_pair_of_the_ceiling_problem_sits_on_its_gate():
    pr, o = cf.sim3_ceiling(), cf.sim3_oracle("ceiling")
    assert pr["n"] == cf.SIM3_MAX_N and len(o["gate_margin"]) == cf.SIM3_MAX_N
    print("sim3 ceiling: least gate margin %.3e, %d inliers, iterations %s" % (o["gate_margin"].min(), o["n_inliers"], o["n_its"]))
    assert o["gate_margin"].min() > cf.GATE_BAND
    assert all(n > 0 for n in o["n_its"]) and 0.7 * cf.SIM3_MAX_N < o["n_inliers"] < cf.SIM3_MAX_N
    plain = ob.sim3_solve(pr)
    assert np.array_equal(plain["r12"], o["r12"]) and np.array_equal(plain["inlier"], o["inlier"])


def test_the_batches_hold_the_sizes_the_ceiling_shares_its_launch_with():
    assert [len(p["inv_sigma2"]) for p in cf.pose_batch()] == [cf.POSE_MAX_N, 9, 0, 1000]
    assert [len(p["inv_sigma2_1"]) for p in cf.sim3_batch()] == [cf.SIM3_MAX_N, 9, 0, 1000]


@pytest.mark.parametrize("name", sorted(cf.RANSAC))
def test_ransac_ceiling_fixture_is_admissible(name):
    pr, a = cf.ransac(name)
    n, nh = len(pr["max_err1"]), len(pr["triples"])
    assert (n, nh) == cf.RANSAC[name][:1] + cf.RANSAC[name][3:4]
    assert rref.distinct(pr["triples"]).all() and len({frozenset(t) for t in pr["triples"].tolist()}) == nh
    assert a["undecided_frac"] <= 0.02, a["undecided_frac"]
    assert a["scan32"][0] >= 0 and a["scan32"][:2] == a["scan64"][:2], (a["scan32"], a["scan64"])
    for h in a["recorded"]:
        assert a["decided"][h].all(), (h, int((~a["decided"][h]).sum()))
    assert rref.admissible(a)
    if name == "n8152":
        assert n % 64 == 24 and a["r32"]["flags"][:, n - 24:].any()          # inliers inside the half-filled last ballot
    if name == "hyp1024":
        assert nh == cf.RANSAC_MAX_HYP and len(np.unique(a["r32"]["counts"])) > 10


def test_triangulation_problems_at_the_ceiling_hold_every_reachable_code():
    from tests import triangulate_ref as tref

    seen = set()
    for k in range(len(cf.TRIANGULATE)):
        pr = cf.triangulate_problem(k)
        assert pr["n"] == cf.TRIANGULATE_MAX_N
        seen |= set(int(s) for s in tref.evaluate(pr, "32j")["status"])
    assert seen == {0, 1, 3, 4, 5, 6, 8}, seen                                 # what tests/test_triangulate_ref.py's fixtures reach


def test_the_frustum_problem_at_the_ceiling_holds_every_code():
    from tests import frustum_ref as fref

    pr = cf.frustum_problem()
    assert pr["n"] == cf.FRUSTUM_MAX_N
    h = fref.host_points(pr)
    counts = np.bincount(h["status"], minlength=8)
    assert (counts > 0).all() and counts[0] > 5000, counts
    assert set(int(s) for s in h["status"][-256:]) >= {0, 1}                   # the last of the 256 workgroups has work of both kinds


@pytest.mark.parametrize("mode", [0, 1])
def test_the_full_bow_group_holds_its_planted_cases(mode):
    for tie in (False, True):
        s1, s2, g, epi, p = cf.bow_full_group(mode, tie)
        nc = np.diff(g["c_ptr"])
        assert nc.tolist() == [cf.BOW_MAX_GROUP, 80] and g["c_idx"][0] == p["first"] and g["c_idx"][cf.BOW_MAX_GROUP - 1] == p["last"]
        kw = dict(mode=1, th=50, epi=epi) if mode else dict(mode=0, th=50, th_inclusive=True, nnratio=1.5)
        m, d, nm = ob.bow_search(s1, s2, g, **kw)
        second_group = g["q_idx"][g["q_ptr"][1]:]
        assert (m[second_group] >= cf.BOW_MAX_GROUP).sum() > 5 and (m[g["q_idx"][:g["q_ptr"][1]]] < cf.BOW_MAX_GROUP).all()
        if mode == 1:
            assert m[p["s"]] == p["last"] and d[p["s"]] == 2                   # the last of equal candidates wins (:731)
        elif tie:
            assert m[p["s"]] == p["first"] and m[p["s2"]] == p["last"] and d[p["s"]] == d[p["s2"]] == 2   # first wins; then taken
        else:
            assert m[p["s"]] == p["last"] and d[p["s"]] == 2 and m[p["s2"]] != p["last"]
    if mode == 0:   # under the usual ratio a tie is refused, and nothing is taken
        s1, s2, g, epi, p = cf.bow_full_group(0, True)
        m, d, nm = ob.bow_search(s1, s2, g, mode=0, th=50, th_inclusive=True, nnratio=0.6)
        assert m[p["s"]] == -1 and m[p["s2"]] == -1 and d[p["s"]] == d[p["s2"]] == 2


def test_kfdb_keyframes_reach_every_query_length():
    kfs = cf.kfdb_keyframes()
    assert len(kfs) == cf.KFDB_SLOTS and max(len(k.mBowVec[0]) for k in kfs if k is not None) == cf.KFDB_MAX_WORDS == max(cf.KFDB_CAPS)
    for cap in cf.KFDB_CAPS:
        q = cf.kfdb_query(cap)
        assert len(q[0]) == cap
        common, first, score = cf.kfdb_reference(cap)
        assert (common == cap).sum() == 1                                       # its own copy
        assert ((common == 1) & (first == q[0][-1])).sum() >= 1 and ((common == 1) & (first == q[0][0])).sum() >= 1
        assert (common[:9] > 0).sum() >= 6 and common[0] == 0
