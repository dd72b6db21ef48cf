#!/usr/bin/env python3
"""Writes tests/golden/orb_ref_*.npz: the outputs of the REFERENCE's own ORB_SLAM2/src/ORBextractor.cc, compiled where it lies and run
under a monotone allocator by oracle/orb_ref_harness.cc (oracle/Makefile.ref; authoring container only), on the fixtures of
tests/orb_ref_fixtures.py.

AUTHORITATIVE for the reference's own half of the extractor (constructor tables, pyramid views, cell walk, FAST retry, DistributeOctTree
and DivideNode, IC_Angle, computeOrbDescriptor, the order of operator()); NOT for the six OpenCV primitives (FAST, resize, GaussianBlur,
copyMakeBorder, fastAtan2, cvRound), which the harness takes from oracle/orb_oracle.cc: those stay restated and unpinned.

Data only (allow_pickle=False).  Frames that weiner_slamit_v2_amd.synth makes are stored as a CRC-32, the others as bytes.  Before it
writes anything the script asserts, from the oracle alone, the premises the fixtures exist for (every octree exit taken, ten or more
cases decided by the tie order, ...), and that the harness equals the oracle; a difference is a finding, not something to record.

    python tools/gen_orb_ref_golden.py
"""
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import bindings as ob  # noqa: E402
from tests import orb_ref_fixtures as fx  # noqa: E402


def save(stem, **arrays):
    path = fx.golden_path(stem)
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size < fx.MAX_FILE_BYTES, "%s: %d bytes" % (path, size)
    return size


def octree_golden():
    exits, decisive = fx.octree_premises()
    fx.assert_octree_premises(exits, decisive)
    results = []
    for c in fx.OCTREE_CASES:
        b = c["borders"]
        r = ob.orb_ref_octree(c["keys"], b[0], b[1], b[2], b[3], c["n"], c["level"])
        assert np.array_equal(r, fx.octree_oracle(c)), "octree %s: the reference differs from the oracle" % c["name"]
        assert np.array_equal(r, r.astype(np.int16)), "octree results are integers"
        results.append(r.astype(np.int16))
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in results])]).astype(np.int32)
    size = save("octree", names=np.array([c["name"] for c in fx.OCTREE_CASES]), inputs_crc=np.uint32(fx.octree_inputs_crc()),
                result=np.concatenate(results), result_ptr=ptr)
    kinds = {k: sum(1 for v in exits.values() if v == k) for k in ob.OCTREE_EXITS}
    print("octree: %d cases, exits %s, %d decided by the tie order, %d bytes" % (len(results), kinds, len(decisive), size))


def extract_golden(name):
    made_by_synth, nf, sf, nl, ini, mn = fx.EXTRACT_CASES[name][1:]
    img = fx.extract_image(name)
    o = fx.oracle_extract(name, img)
    fx.extract_premises(name, o)
    r = ob.orb_ref_extract(img, nf, sf, nl, ini, mn)
    fx.assert_same_extract(o, r, name)
    out = {"params": np.array([nf, nl, ini, mn], np.int32), "scale": np.float32(sf), "img_crc": np.uint32(fx.crc(img)), "desc": r["desc"],
           "level_crc": np.array([fx.crc(p) for p in r["levels"]], np.uint32),
           "level_ptr": np.concatenate([[0], np.cumsum([len(k) for k in r["level_kps"]])]).astype(np.int32)}
    if not made_by_synth:
        out["image"] = img
    lk = np.concatenate(r["level_kps"])
    for f in fx.KP_FIELDS:
        out["kp_" + f] = np.ascontiguousarray(r["kps"][f]).view(np.uint32)
        out["lk_" + f] = np.ascontiguousarray(lk[f]).view(np.uint32)
    for k in fx.TABLES:
        out["t_" + k] = r["tables"][k]
    assert np.array_equal(r["levels"][0][19:-19, 19:-19], img)
    # interiors of levels 1.., packed into as few files as stay below the limit (rich frames barely compress)
    groups, budget = [], int(fx.MAX_FILE_BYTES * 0.9)
    for l in range(1, nl):
        interior = np.ascontiguousarray(r["levels"][l][19:-19, 19:-19])
        assert np.array_equal(fx.pad19(interior), r["levels"][l])
        if not groups or groups[-1][0] + interior.size > budget:
            groups.append([0, {}])
        groups[-1][0] += interior.size
        groups[-1][1]["level%d" % l] = interior
    out["n_pyr_files"] = np.int32(len(groups))
    sizes = [save(name, **out)] + [save("%s_pyr%d" % (name, k), **g[1]) for k, g in enumerate(groups)]
    print("%s: %d keypoints, per level %s, exits %s, files %s bytes" % (name, len(r["kps"]), [len(k) for k in r["level_kps"]], o["exits"], sizes))


if __name__ == "__main__":
    assert ob.orb_ref_available(), "oracle/_ref/orb_ref_harness is built only where the reference's sources are (oracle/Makefile.ref)"
    for old in glob.glob(fx.golden_path("*")):
        os.remove(old)
    octree_golden()
    for case in fx.EXTRACT_CASES:
        extract_golden(case)
