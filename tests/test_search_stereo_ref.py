"""The numpy restatement of the guided search with the right-image gate (tests/search_stereo_ref.py): pinned to the C++ oracle
where no keypoint is stereo, to hand-made cases at every edge of the two rules, and the condition the GPU fixtures must meet."""
import numpy as np
import pytest

from oracle import bindings as ob
from tests import search_stereo_fixtures as fx
from tests import search_stereo_ref as ref
from weiner_slamit_v2_amd import synth

SEEDS = ((0, {}), (1, dict(crowd=True)), (4, {}))


def _same(a, b):
    assert np.array_equal(a[0], b[0])
    assert a[1] == b[1]
    assert np.array_equal(a[2], b[2])


@pytest.mark.parametrize("seed,kw", SEEDS)
def test_model_is_the_oracle_without_stereo_keypoints(seed, kw):
    f, q = synth.synth_search(seed=seed, **kw)
    n, m = len(f["kp_xy"]), len(q["uvr"])
    o = ob.guided_search(f, q, 100, True, 0.8)
    assert o[1] > 20
    _same(ref.guided_search(f, q, 100, True, 0.8), o)
    mono = np.full(n, -1, np.float32)
    q_ur = np.random.RandomState(seed).uniform(0, 640, m).astype(np.float32)
    _same(ref.guided_search(f, q, 100, True, 0.8, er_mode=fx.RADIUS, kp_ur=mono, q_ur=q_ur), o)


@pytest.mark.parametrize("seed,kw", SEEDS)
def test_model_is_the_oracle_fuse_gate_without_stereo_keypoints(seed, kw):
    f, q = synth.synth_search(seed=seed, **kw)
    n, m = len(f["kp_xy"]), len(q["uvr"])
    sig = synth._inv_sigma2_table()
    o = ob.guided_search(f, q, 50, False, 0.6, chi2_gate=5.99, inv_level_sigma2=sig)
    assert o[1] > 10
    q_ur = np.random.RandomState(seed).uniform(0, 640, m).astype(np.float32)
    _same(ref.guided_search(f, q, 50, False, 0.6, chi2_gate=5.99, inv_level_sigma2=sig, er_mode=fx.CHI2, kp_ur=np.full(n, -1, np.float32),
                            q_ur=q_ur), o)


HAND = fx.hand_cases()


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_hand_made_cases(case):
    _, frame, queries, rule, st, expect = case
    match, nm, out4 = ref.guided_search(frame, queries, **rule, **fx.model_kw(st))
    assert match[0] == expect
    assert nm == (expect >= 0)
    # without the gate every one of these windows has a candidate: the gate is what decides
    mono = ref.guided_search(frame, queries, **dict(rule, chi2_gate=0.0))
    assert mono[0][0] >= 0


def test_q_ur_stride():
    f, q, st = fx.fixture(fx.RADIUS, 300)
    wide = np.zeros((fx.M, 3), np.float32)
    wide[:, 2] = st["q_ur"]
    a = ref.guided_search(f, q, **fx.rule(fx.RADIUS, st), **fx.model_kw(st))
    b = ref.guided_search(f, q, **fx.rule(fx.RADIUS, st), **dict(fx.model_kw(st), q_ur=wide.reshape(-1)[2:], q_ur_stride=3))
    _same(a, b)


@pytest.mark.parametrize("key", fx.GATED, ids=["mode%d-n%d%s" % (k[0], k[1], "-crowd" if k[2] else "") for k in fx.GATED])
def test_fixture_condition(key):
    """Counts (differ, removed) of the fixtures as chosen -- RADIUS: n63 (22, 61), n64 (21, 51), n65 (20, 55), n300 (30, 55), crowd
    (34, 68; 26 windows over 128 candidates, 4 of them re-walked); CHI2: n63 (25, 61), n64 (21, 54), n65 (22, 43), n300 (34, 56)."""
    er_mode, n, crowd = key
    f, q, st = fx.fixture(*key)
    kur = st["kp_ur"]
    stereo = kur > 0 if er_mode == fx.RADIUS else kur >= 0
    assert 0.3 * n <= stereo.sum() <= 0.7 * n          # about half the keypoints are stereo
    assert (kur == 0).sum() >= 2                        # a few are exactly 0.0f
    rule = fx.rule(er_mode, st)
    mono = ref.guided_search(f, q, **rule)
    stats = {}
    ster = ref.guided_search(f, q, stats=stats, **rule, **fx.model_kw(st))
    differ = int((mono[0] != ster[0]).sum())
    print(key, "differ", differ, "removed", stats["gate_removed_best"], "matches", mono[1], ster[1])
    assert differ >= 20
    assert stats["gate_removed_best"] >= 10
    # the gate also keeps: some accepted matches sit on stereo keypoints
    kept = ster[0][ster[0] >= 0]
    assert stereo[kept].sum() >= 3
    if crowd:   # windows that hold more candidates than the batch form's stored list (SLAMIT_SEARCH_BATCH_CAND = 128)
        print("over 128:", int((stats["candidates"] > 128).sum()), "re-walks:", stats["rewalks_over_128"])
        assert (stats["candidates"] > 128).sum() >= 10
        assert stats["rewalks_over_128"] >= 3           # ... and the gate goes through the re-walk
