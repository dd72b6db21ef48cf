#!/usr/bin/env python3
"""Generates tests/golden/ref_g2o_cases.json.gz: the REFERENCE's own g2o (oracle/_ref/libba_ref.so) on the synthesized
problems that tests/test_oracle_ba.py and tests/test_oracle_pose.py compare the oracle with, so that those tests run
where the reference build does not exist.  Needs that build (oracle/Makefile.ref)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import bindings as ob  # noqa: E402
from tests import test_oracle_ba, test_oracle_pose  # noqa: E402
from tests.helpers import REF_CASES_GOLDEN, save_ref_cases  # noqa: E402
from weiner_slamit_v2_amd import synth  # noqa: E402


def main():
    assert ob.ba_ref_available()
    cases = {}
    for k, p, o, seed, nfix in test_oracle_ba.REF_CASES:
        prob = synth.synth_ba(k, p, o, seed=seed, n_fixed=nfix)
        cases["ba%s" % ((k, p, o, seed, nfix),)] = (prob, ob.ba_ref_solve(prob))
    for seed in test_oracle_ba.SIM3_REF_SEEDS:
        prob = test_oracle_ba.sim3_ref_problem(seed)
        cases["sim3(%d,)" % seed] = (prob, ob.sim3_ref_solve(prob))
    for n, of, seed, pert in test_oracle_pose.REF_CASES:
        prob = synth.synth_pose(n, of, seed, pert)
        cases["pose%s" % ((n, of, seed, pert),)] = (prob, ob.pose_ref_solve(prob))
    save_ref_cases(cases)
    print("%d cases -> %s (%d bytes)" % (len(cases), os.path.relpath(REF_CASES_GOLDEN, ROOT), os.path.getsize(REF_CASES_GOLDEN)))


if __name__ == "__main__":
    main()
