"""Known answers of tests/kfdb_ref.py, the restatement of KeyFrameDatabase.cc and L1Scoring::score that the GPU tests compare with, and
the admissibility of its fixtures: each must be able to tell a wrong implementation from a right one, by the restatement alone."""
import numpy as np
import pytest

from tests import kfdb_ref as ref


def _vec(words, values):
    return np.array(words, np.int32), np.array(values, np.float64)


def test_score_of_a_vector_with_itself_is_its_sequential_l1_norm():
    for pool, n, seed in ((64, 30, 1), (400, 200, 2), (1000, 256, 3)):
        v = ref.bow(pool, n, seed)
        norm = 0.0
        for x in v[1]:
            norm += abs(float(x))                           # each term is |0| - |x| - |x| = -2|x|, and halving is exact
        assert ref.score(v, v) == norm and abs(norm - 1.0) < 1e-12


def test_disjoint_vectors_walk_nothing():
    a, b = _vec([1, 5, 9], [0.2, 0.3, 0.5]), _vec([0, 4, 8, 10], [0.25, 0.25, 0.25, 0.25])
    assert ref.score(a, b) == 0.0 and ref.score(b, a) == 0.0
    assert ref.score(a, _vec([], [])) == 0.0
    kf = ref.KeyFrame(0, b)
    assert [x.tolist() for x in ref.dense([kf, None], a)] == [[0, -1], [-1, -1], [0.0, 0.0]]


def test_three_shared_words_by_hand():
    a = _vec([2, 3, 7, 11], [0.5, 0.25, 0.125, 0.125])
    b = _vec([1, 3, 7, 11, 12], [0.125, 0.5, 0.125, 0.0625, 0.1875])
    # word 3: |0.25 - 0.5| - 0.25 - 0.5 = -0.5; word 7: 0 - 0.125 - 0.125 = -0.25; word 11: 0.0625 - 0.125 - 0.0625 = -0.125
    assert ref.score(a, b) == 0.4375 == ref.score(b, a)
    c, f, s = ref.dense([ref.KeyFrame(0, b)], a)
    assert (c[0], f[0], s[0]) == (3, 3, 0.4375)


def test_erase_keeps_the_order_of_the_rest():
    db = ref.KeyFrameDatabase()
    kfs = [ref.KeyFrame(i, _vec([4, 6 + i], [0.5, 0.5])) for i in range(5)]
    for kf in kfs:
        db.add(kf)
    db.erase(kfs[1])
    db.erase(kfs[1])                                        # absent: nothing happens
    assert [k.mnId for k in db.mvInvertedFile[4]] == [0, 2, 3, 4] and db.mvInvertedFile[7] == []
    db.add(kfs[1])
    assert [k.mnId for k in db.mvInvertedFile[4]] == [0, 2, 3, 4, 1]
    got = db.DetectRelocalizationCandidates(ref.Frame(9, _vec([4], [1.0])))
    assert [k.mnId for k in db.last["sharing"]] == [0, 2, 3, 4, 1] and len(got) >= 1


def test_min_common_words_is_a_float_product_truncated():
    f = np.float32(0.8)
    for m in range(1, 20001):
        want = int(np.float32(np.float32(m) * f))           # (int)((float)m * 0.8f)
        assert ref.min_common_words(m) == want and (m * 4) // 5 <= want <= (m * 4) // 5 + 1   # 0.8f > 0.8: never below the exact floor
    assert ref.min_common_words(5) == 4 and ref.min_common_words(10) == 8 and ref.min_common_words(1) == 0


@pytest.mark.parametrize("pool", [64, 400, 1000])
def test_scoring_fixtures_tell_the_sum_order(pool):
    pairs = ref.scoring_pairs(pool)
    fwd = np.array([ref.score(a, b) for a, b in pairs])
    rev = np.array([ref.score_reversed(a, b) for a, b in pairs])
    assert (fwd != rev).sum() * 3 >= len(pairs)             # a sum in another order shows in the double ...
    assert np.array_equal(fwd.astype(np.float32), rev.astype(np.float32))   # ... and not in a float: why the ABI returns doubles
    assert np.allclose(fwd, rev, rtol=0, atol=1e-14) and (fwd > 0).all()


def _facts(name):
    sc = ref.SCENARIOS[name]
    out, notes = ref.run_scenario(sc)
    return sc, out, notes


@pytest.mark.parametrize("name", sorted(ref.SCENARIOS))
def test_every_query_of_a_scenario_returns_candidates(name):
    sc, out, notes = _facts(name)
    for cands in out:
        assert len(cands) >= 3 and len(set(cands)) == len(cands)
    assert any(c != sorted(c) for c in out) or name == "loop"   # the order is the walk's, not the ids'


def test_scenarios_reach_every_branch():
    best_elsewhere = duplicates = min_score_cut = 0
    for name in ref.SCENARIOS:
        sc, out, notes = _facts(name)
        for q, n in zip(sc["queries"], notes):
            best_elsewhere += sum(1 for (_, kf), (_, best) in zip(n["scored"], n["acc"]) if kf is not best)
            duplicates += n["duplicates"]
            if q[0] == "loop":
                min_score_cut += n["nscores"] - len(n["scored"])
    assert best_elsewhere > 0 and duplicates > 0 and min_score_cut > 0


@pytest.mark.parametrize("name", ["reloc_stale", "mixed"])
def test_a_second_relocalisation_reads_scores_an_earlier_one_left(name):
    """KeyFrameDatabase.cc:292-295: a neighbour that shares a word but missed minCommonWords adds the mRelocScore of an earlier query.
    With the scores zeroed before every query the second query's outcome is another one: the state has to live in the keyframe."""
    sc = ref.SCENARIOS[name]
    kept, _ = ref.run_scenario(sc)
    reset, _ = ref.run_scenario(sc, reset_scores=True)
    assert kept[0] == reset[0] and kept[1] != reset[1]
