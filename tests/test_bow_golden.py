"""CPU: the two restatements the rest of the suite leans on -- tests/bow_voc_ref.py (TemplatedVocabulary::transform) and the scoring part
of tests/kfdb_ref.py (L1Scoring::score) -- and the text loader of csrc/voc_pack.cc against tests/golden/bow_*.npz, which the reference's
own DBoW2 computed (tools/gen_bow_golden.py), and, where oracle/_ref/libdbow_ref.so was built, against that library itself on fresh
trees.  Bar: every array equal, doubles as bit patterns."""
import numpy as np
import pytest

from oracle import bindings as ob
from tests import bow_voc_ref as ref
from tests import kfdb_ref
from tests.bow_golden import CASES, golden, same
from tests.test_voc_pack import _same as same_voc
from tests.test_voc_pack import drv, load   # noqa: F401  (drv: the module-scoped fixture that compiles voc_pack.cc with g++)


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


@pytest.mark.parametrize("name", CASES)
def test_the_restatement_reproduces_the_reference_transform(name):
    g = golden(name)
    V = ref.Vocabulary(g.voc)
    assert g.info == {"k": g.voc["k"], "L": g.voc["L"], "scoring": 0, "weighting": g.voc["weighting"], "n_nodes": len(g.voc["parent"]), "n_words": V.n_words}
    for f in range(len(g.frames)):
        d = g.desc(f)
        for ls in g.levelsups:
            got = V.transform(d, ls)
            same(got, g.expected(f, ls), "%s frame %d levelsup %d" % (name, f, ls))
            per = [V.transform_feature(x, ls) for x in d]
            assert [p[0] for p in per] == g.raw(f, ls, "word_id").tolist()             # the word of a stopped feature too
            assert np.array_equal(bits(np.array([p[1] for p in per])), bits(g.raw(f, ls, "word_weight")))
            unset = g.unset(f, ls)
            # where the reference never wrote the node id the project's is the leaf's own (include/slamit.h): a leaf, reached above level L - levelsup
            assert (g.voc["is_leaf"][got["node_id"][unset] - 1] > 0).all() and np.array_equal(got["node_id"][unset], g.leaf_node[g.raw(f, ls, "word_id")[unset]])
            assert name == "unbalanced" or not unset.any()
            if not g.has_fv:
                assert "fv_node" not in g.expected(f, ls)


def test_the_goldens_hold_what_they_are_there_for():
    """Read from the files alone (the generator asserts the same before it writes them)."""
    g = golden("k10L3")
    assert (g.raw(0, 1, "word_weight") == 0).any() and len(g.raw(0, 1, "bow_word")) < (g.raw(0, 1, "word_weight") > 0).sum()
    assert len(g.bow(6)[0]) == 0 and len(g.bow(4)[0]) == 1                          # a frame of one stopped feature; a one-word frame
    assert all(g.unset(0, ls).any() for ls in golden("unbalanced").levelsups for g in [golden("unbalanced")])
    assert (golden("k3L2").raw(1, 3, "node_id") == 0).all() and (golden("k3L2").voc["is_leaf"][golden("k3L2").raw(1, 0, "node_id") - 1] > 0).all()   # levelsup L + 1: the root; 0: the leaves
    assert not golden("unbalanced").has_fv and all(golden(n).has_fv for n in CASES if n != "unbalanced")
    assert all(not golden(n).text.endswith(b"\n") for n in CASES)
    assert golden("tf").voc["weighting"] == 1 and golden("k20L2").voc["k"] == 20 and golden("k3L6").levelsups == [4]


@pytest.mark.parametrize("name", CASES)
def test_the_restatement_reproduces_the_reference_score_in_both_argument_orders(name):
    g = golden(name)
    bows = [g.bow(f) for f in range(len(g.frames))]
    for i, a in enumerate(bows):
        for j, b in enumerate(bows):
            want = g.score[i, j]                                                    # score(a, b): [j, i] is the other order
            assert bits(kfdb_ref.score(a, b)) == want, "%s score(%d, %d)" % (name, i, j)
            shared = len(np.intersect1d(a[0], b[0]))
            if shared <= 2:                                                        # up to two terms: their order cannot matter
                assert bits(kfdb_ref.score_reversed(a, b)) == want
            if shared == 0:
                assert want == bits(-0.0)                                          # -(0.0) / 2.0 of an empty sum
            if i == j and shared:
                assert abs(np.uint64(want).view(np.float64) - 1.0) < 1e-12


def test_the_score_goldens_tell_the_sum_order_and_the_argument_order():
    """Somewhere in the goldens the terms added from the largest word id down give other bits than the reference's, and somewhere
    score(a, b) and score(b, a) differ: a sum in another order, or the other side's value first, does not pass."""
    other_order = other_side = 0
    for name in CASES:
        g = golden(name)
        bows = [g.bow(f) for f in range(len(g.frames))]
        for i, a in enumerate(bows):
            for j, b in enumerate(bows):
                other_order += bits(kfdb_ref.score_reversed(a, b)) != g.score[i, j]
                other_side += g.score[i, j] != g.score[j, i]
    assert other_order >= 1 and other_side >= 1, (other_order, other_side)


@pytest.mark.parametrize("name", CASES)
def test_voc_pack_parses_the_golden_text_into_the_golden_arrays(drv, tmp_path, name):   # noqa: F811
    g = golden(name)
    p = tmp_path / "voc.txt"
    p.write_bytes(g.text)
    got, why = load(drv, str(p))
    assert got is not None, why
    assert same_voc(got, g.voc) and len(got["parent"]) == g.info["n_nodes"] and int((got["is_leaf"] > 0).sum()) == g.info["n_words"]


def _fresh_tree(seed):
    """Random k in 2..20, L in 1..5 (the depth cut where k ** L would pass 2,000 leaves), stops and duplicated siblings."""
    rs = np.random.RandomState(9000 + seed)
    k = int(rs.randint(2, 21))
    L = int(rs.randint(1, 6))
    while k ** L > 2000:
        L -= 1
    voc = ref.full_tree(k, L, 100 + seed, stop_frac=float(rs.choice([0.0, 0.2, 0.5])), dup_siblings=bool(seed % 2), order=("dfs", "bfs")[seed % 3 == 0])
    return voc, int(rs.randint(0, L + 2)), rs


@pytest.mark.skipif(not ob.dbow_ref_available(), reason="oracle/_ref/libdbow_ref.so is built only where the reference's sources are (oracle/Makefile.ref)")
@pytest.mark.parametrize("seed", range(20))
def test_live_the_restatement_equals_the_reference_on_fresh_trees(seed, tmp_path):
    voc, levelsup, rs = _fresh_tree(seed)
    p = str(tmp_path / "voc.txt")
    ref.write_text(voc, p, trailing_newline=False)
    R = ob.DbowRef(p)
    V = ref.Vocabulary(voc)
    q = np.concatenate([ref.queries(voc, 90, 300 + seed), ref.equidistant_queries(voc, 10, 400 + seed)])
    want, per = R.transform(q, levelsup), R.features(q, levelsup)
    assert (per["node_id"] >= 0).all()                                             # full trees: the reference writes every node id
    want.update(word_id=np.where(per["weight"] > 0, per["word_pub"], -1), node_id=per["node_id"])
    same(V.transform(q, levelsup), want, "seed %d k %d L %d levelsup %d" % (seed, voc["k"], voc["L"], levelsup))
    cuts = [(int(s), int(c)) for s, c in zip(rs.randint(0, 60, 12), rs.randint(1, 41, 12))]
    bows = [R.transform_bow(q[s:s + c]) for s, c in cuts]
    for (s, c), b in zip(cuts, bows):
        mine = V.transform(q[s:s + c], levelsup)
        assert np.array_equal(mine["bow_word"], b[0]) and np.array_equal(bits(mine["bow_value"]), bits(b[1]))
    for _ in range(50):
        i, j = (int(v) for v in rs.randint(0, len(cuts), 2))
        assert bits(kfdb_ref.score(bows[i], bows[j])) == bits(R.score(bows[i], bows[j])), (seed, i, j)
    R.close()
