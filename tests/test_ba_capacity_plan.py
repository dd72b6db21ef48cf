"""The local-BA windows that tests/test_gpu_ba.py runs at a handle's capacity (max_kf = 85), planned on the CPU: each must still reach
the variant of the kernels it is there for, so that a change to synth or to the planner (csrc/ba_plan.cc) cannot quietly move the GPU
tests back to the shapes the max_kf = 64 handle already covers (Npad <= 320, Kpad <= 6144, <= 10 LDLt panels)."""
import os

import pytest

from tests.helpers import BA_CAPACITY, fixed_keyframes_last
from tests.test_ba_plan import BA_SOLVER_BAND, CSRC, build_plan_lib, limits, npad_max, plan
from weiner_slamit_v2_amd import synth

BA_SOLVER_BLOCKED = 1 - BA_SOLVER_BAND
LDS_LIMIT = 160 * 1024 - 2048                 # slamit_ba_create: bak_ldlt_smem(Npad_max) must fit in this
LD_NB, LD_P, LD_BAND_LDS = 32, 33, 150 * 1024   # the blocked LDLt's panel width and LDS row pitch, the banded one's budget (bak_ldlt_smem)


@pytest.fixture(scope="module")
def plib(tmp_path_factory):
    return build_plan_lib(str(tmp_path_factory.mktemp("ba_capacity_plan")), [os.path.join(CSRC, "ba_plan.cc")])


def _plan(L, name, **lim):
    prob = synth.synth_ba(**BA_CAPACITY[name])
    if name == "fixed40":
        prob, _ = fixed_keyframes_last(prob)
    o = plan(L, prob, limits(85, **lim))
    assert o is not None, name
    return o


def test_the_ceiling_is_85_keyframes():
    """Npad_max = rup(6 max_kf + 1, 64): 85 keyframes give 512 rows, 86 give 576, whose blocked-LDLt panel no longer fits in LDS."""
    assert npad_max(64) == 448 and npad_max(85) == 512 and npad_max(86) == 576
    smem = lambda npad: max(8 * (LD_NB * LD_P + (npad + 16) * LD_P), LD_BAND_LDS)
    assert smem(512) <= LDS_LIMIT < smem(576) == 164736


def test_capacity_windows_reach_their_variants(plib):
    o = _plan(plib, "band512")
    assert (o["nS"], o["Npad"], o["solver"]) == (504, 512, BA_SOLVER_BAND) and o["sf_groups"] > 0
    assert len(o["panel_hi"]) == 16 and len(o["tile_alo"]) == 8       # LDLt panels 11-16, Schur tiles 6-8

    o = _plan(plib, "blocked512")
    assert (o["nS"], o["Npad"], o["solver"]) == (504, 512, BA_SOLVER_BLOCKED) and len(o["panel_hi"]) == 16
    assert o["sf_groups"] > 0 and o["Kpad"] <= 6144
    assert _plan(plib, "blocked512", nwin=16)["sf_groups"] > 0       # (a batch of 16: fewer groups, still floating windows)
    assert _plan(plib, "blocked512", no_sf=1)["sf_groups"] == 0      # SLAMIT_BA_SF=0: the same window over tile pairs

    o = _plan(plib, "tiles512")
    assert (o["Npad"], o["solver"], o["sf_groups"], o["band"]) == (512, BA_SOLVER_BLOCKED, 0, 503)   # 8 x 8 tile pairs, every panel dense

    o = _plan(plib, "kpad12k")
    assert o["Npad"] == 512 and o["Kpad"] > 6144 and o["Kpad"] == 12288 and o["sf_groups"] > 0

    o = _plan(plib, "kf70")
    assert (o["nS"], o["Npad"], o["solver"]) == (414, 448, BA_SOLVER_BAND) and len(o["panel_hi"]) == 13

    o = _plan(plib, "fixed40")   # fixed keyframes listed last: they count toward max_kf, not toward the reduced system
    assert (o["n_kf"], o["n_free"], o["nS"], o["Npad"], o["solver"]) == (85, 45, 270, 320, BA_SOLVER_BAND)

    o = _plan(plib, "stereo512")
    assert o["Npad"] == 512 and o["nS"] == 504

