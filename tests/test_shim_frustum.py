"""shim/Tracking.h: SearchLocalPoints over mock frame and map-point types (shim_test frustum) against the g++-built csrc/frustum.h and a
Python path through the same device entry points: the members the reference's isInFrustum stores, the IncreaseVisible calls, the
frame's own points, and the matches of the search that follows."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import frustum_ref as ref
from tests.helpers import ROOT

SHIM = os.path.join(ROOT, "weiner_slamit_v2_amd", "shim")
EXE = os.path.join(SHIM, "shim_test")
FIXTURE = 6          # 513 points, th = 3: the widened window


def _build():
    from weiner_slamit_v2_amd import build as hb

    hb.build()
    subprocess.check_call(["make", "-s", "-C", SHIM, "-f", "Makefile", "all"])


def scenario():
    pr = dict(ref.fixture(FIXTURE))
    n = int(pr["n"])
    rs = np.random.RandomState(77)
    skip = pr["skip"].copy()
    skip[skip != 0] = rs.randint(1, 3, int((skip != 0).sum()))              # 1 = bad, 2 = seen in this frame already
    pr["skip"] = skip
    frame, qdesc, takes = ref.search_side(pr, ref.host_points(pr), 60)
    nkp = len(frame["kp_xy"])
    state = np.zeros(nkp, np.int32)
    state[rs.rand(nkp) < 0.12] = 1
    state[(state == 0) & (rs.rand(nkp) < 0.05)] = 2
    state[(state == 0) & (rs.rand(nkp) < 0.05)] = 3
    frame = dict(frame, kp_taken=(state == 1).astype(np.uint8))
    nobs = takes.astype(np.int32) * 2                                       # Observations() > 0 is the takes flag
    return pr, frame, qdesc, nobs, state


def blob(pr, frame, qdesc, nobs, state, nnratio):
    n, nkp = int(pr["n"]), len(frame["kp_xy"])
    out = [ref.problem_blob(pr), b"\0" * ((4 - n % 4) % 4), nobs.astype(np.int32).tobytes(), qdesc.tobytes(),
           struct.pack("<ifff", nkp, nnratio, frame["inv_w"], frame["inv_h"]), frame["kp_xy"].astype(np.float32).tobytes(),
           frame["kp_octave"].astype(np.int32).tobytes(), state.tobytes(), frame["desc"].tobytes()]
    return b"".join(out)


@pytest.mark.gpu
def test_search_local_points_keeps_the_reference_order(tmp_path):
    from weiner_slamit_v2_amd import api

    _build()
    pr, frame, qdesc, nobs, state = scenario()
    n, nkp = int(pr["n"]), len(frame["kp_xy"])
    pin, pout = tmp_path / "fru.bin", tmp_path / "fru.out"
    pin.write_bytes(blob(pr, frame, qdesc, nobs, state, 0.8))
    p = subprocess.run([EXE, "frustum", str(pin), str(pout)], stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr
    raw = pout.read_bytes()
    status, nm, ninview = struct.unpack("<iii", raw[:12])
    assert status == 0, p.stderr
    rec = np.frombuffer(raw, np.uint8, 28 * n, 12).reshape(n, 28)
    ints, flts = rec[:, :12].copy().view(np.int32), rec[:, 12:].copy().view(np.float32)
    owner = np.frombuffer(raw, np.int32, nkp, 12 + 28 * n)
    tail = np.frombuffer(raw, np.int32, 4, 12 + 28 * n + 4 * nkp)
    assert len(raw) == 12 + 28 * n + 4 * nkp + 16

    h = ref.host_points(pr)                                                  # the header: what the reference's isInFrustum stores
    inv, skipped = h["status"] == 0, pr["skip"] != 0
    assert np.array_equal(h["status"] == 1, skipped) and inv.sum() > 100 and (h["status"] == 7).sum() > 10
    assert ninview == int(inv.sum())
    assert np.array_equal(ints[:, 0][~skipped], inv[~skipped].astype(np.int32))             # mbTrackInView; status 7 is false: the departure
    # the reference touches neither skipped points nor the members of rejected ones: a bad point keeps its stale flag, a point seen in this
    # frame the `false` the loop over the frame's own points gave it, and both keep the mock's sentinels in every other member
    assert np.all(ints[:, 0][pr["skip"] == 1] == 1) and np.all(ints[:, 0][pr["skip"] == 2] == 0) and np.all(ints[:, 1][~inv] == -77)
    assert (pr["skip"] == 1).sum() > 3 and (pr["skip"] == 2).sum() > 3
    assert np.all(flts[~inv] == -7.0)
    assert np.array_equal(ints[:, 1][inv], h["level"][inv])
    want = np.stack([h["u"], h["v"], h["uR"], h["viewCos"]], 1)
    assert np.array_equal(flts[inv].view(np.uint32), want[inv].view(np.uint32))
    assert np.array_equal(ints[:, 2], inv.astype(np.int32))                                 # IncreaseVisible: once per point in view
    assert tail.tolist() == [int((state == 1).sum()), int((state == 2).sum()), 1, 1]        # the frame's own points: visible once per keypoint, seen now

    out = api.frustum(pr)                                                    # the Python path: the same two device calls
    assert out["n_in_view"] == ninview
    q = dict(uvr=out["uvr"], level_min=out["level_min"], level_max=out["level_max"], desc=qdesc, valid=out["valid"], takes=(nobs > 0).astype(np.uint8))
    gm, gn, _ = api.ORBmatcher.guided_search(frame, q, 100, True, 0.8)
    assert nm == gn and gn > 50
    want_owner = np.where(state == 1, -2, np.where(state == 2, -3, -1)).astype(np.int32)    # a bad own point was set to NULL
    for k in np.flatnonzero(gm >= 0):
        want_owner[gm[k]] = k
    assert np.array_equal(owner, want_owner)
