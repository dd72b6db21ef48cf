"""Known-answer cases for tests/bow_voc_ref.py, the restatement of DBoW2's vocabulary transform that the device is checked against
(no GPU).  The answers are worked out by hand from the reference's rules, not by the code under test."""
import numpy as np

from tests import bow_voc_ref as ref


def _d(*ones):
    """A 32-byte descriptor with the given bit positions set."""
    bits = np.zeros(256, np.uint8)
    bits[list(ones)] = 1
    return np.packbits(bits)


def _two_level():
    """k = 2, L = 2.  File order: 1 = A (root's child), 2 = B (root's child), 3, 4 = A's leaves (words 0, 1), 5, 6 = B's (words 2, 3).
    A = no bits, B = bits 0..7; leaves differ from their parent in bits 100.. ."""
    parent = [0, 0, 1, 1, 2, 2]
    is_leaf = [0, 0, 1, 1, 1, 1]
    B = list(range(8))
    desc = [_d(), _d(*B), _d(100), _d(101, 102), _d(*B, 100), _d(*B, 101, 102)]
    weight = [0.0, 0.0, 0.5, 0.25, 2.0, 0.0]    # word 3 (node 6) is stopped
    return ref._voc(2, 2, parent, is_leaf, desc, weight)


def test_two_level_tree_by_hand():
    v = ref.Vocabulary(_two_level())
    assert v.n_words == 4 and v.children[0] == [1, 2] and v.children[1] == [3, 4] and v.children[2] == [5, 6]
    q = np.stack([_d(100),              # A (0 < 8), then node 3 (0 < 3): word 0, weight 0.5
                  _d(0, 1, 2, 3, 4),    # B (3 < 5), then node 5 (4 < 5): word 2, weight 2.0
                  _d(101, 102),         # A, node 4: word 1, weight 0.25
                  _d(100)])             # word 0 again
    r = v.transform(q, levelsup=1)      # node level 2 - 1 = 1: A = 1, B = 2
    assert r["word_id"].tolist() == [0, 2, 1, 0] and r["node_id"].tolist() == [1, 2, 1, 1]
    assert r["bow_word"].tolist() == [0, 1, 2]
    # values (0.5 + 0.5), 0.25, 2.0; norm ((0 + 1.0) + 0.25) + 2.0 = 3.25: all exact in binary
    assert r["bow_value"].tolist() == [1.0 / 3.25, 0.25 / 3.25, 2.0 / 3.25]
    assert r["fv_node"].tolist() == [1, 2] and r["fv_ptr"].tolist() == [0, 3, 4] and r["fv_items"].tolist() == [0, 2, 3, 1]
    r0 = v.transform(q, levelsup=0)     # node level 2: the leaves themselves
    assert r0["node_id"].tolist() == [3, 5, 4, 3] and r0["fv_node"].tolist() == [3, 4, 5] and r0["fv_items"].tolist() == [0, 3, 2, 1]


def test_a_tie_between_siblings_goes_to_the_first():
    v = ref.Vocabulary(_two_level())
    q = _d(0, 1, 2, 3)                  # 4 from A and 4 from B: strict '<' keeps A; then 1 from node 3 and 2 from node 4
    assert v.transform_feature(q, 1) == (0, 0.5, 1)
    voc = _two_level()
    voc["desc"][3] = voc["desc"][2]     # duplicated sibling centroids: always the first
    assert ref.Vocabulary(voc).transform_feature(_d(100), 0)[0] == 0


def test_a_stopped_word_enters_neither_vector():
    v = ref.Vocabulary(_two_level())
    q = np.stack([_d(*range(8), 101, 102), _d(100)])   # feature 0 -> node 6, word 3, weight 0
    r = v.transform(q, levelsup=1)
    assert r["word_id"].tolist() == [-1, 0] and r["node_id"].tolist() == [2, 1]
    assert r["bow_word"].tolist() == [0] and r["bow_value"].tolist() == [1.0]
    assert r["fv_node"].tolist() == [1] and r["fv_items"].tolist() == [1] and r["fv_ptr"].tolist() == [0, 1]
    only = v.transform(q[:1], levelsup=1)
    assert len(only["bow_word"]) == 0 and len(only["fv_node"]) == 0 and only["fv_ptr"].tolist() == [0]


def test_levelsup_at_or_beyond_L_gives_the_root():
    v = ref.Vocabulary(_two_level())
    q = np.stack([_d(100), _d(0, 1, 2, 3, 4)])
    for levelsup in (2, 3, 7):
        r = v.transform(q, levelsup)
        assert r["node_id"].tolist() == [0, 0] and r["fv_node"].tolist() == [0] and r["fv_items"].tolist() == [0, 1]
        assert r["word_id"].tolist() == [0, 2]


def test_a_leaf_above_the_node_level_reports_itself():
    voc = ref.unbalanced_tree(3)
    v = ref.Vocabulary(voc)
    assert not v.children[1] and all(not v.children[c] for c in v.children[2])
    q = voc["desc"][[0, 1]]             # the level-1 leaf's own centroid; node 2's, whose children are leaves at level 2
    assert v.transform_feature(q[0], 2)[2] == 1 and v.transform_feature(q[0], 0)[2] == 1
    leaf = v.transform_feature(q[1], 2)[2]          # node level 4 - 2 = 2: exactly the leaf's level
    assert leaf in (4, 5, 6)
    assert v.transform_feature(q[1], 1)[2] == leaf  # node level 3 lies below the leaf


def test_bow_values_sum_to_one_within_rounding():
    voc = ref.full_tree(4, 3, seed=5, stop_frac=0.2)
    r = ref.Vocabulary(voc).transform(ref.queries(voc, 300, 6), 1)
    s = 0.0
    for x in r["bow_value"]:
        s += float(x)
    # each quotient is off by at most half an ulp of a value < 1, and so is each of the partial sums
    assert len(r["bow_word"]) > 20 and abs(s - 1.0) <= len(r["bow_value"]) * 2.0 ** -52
    assert np.all(np.diff(r["bow_word"]) > 0) and np.all(np.diff(r["fv_node"]) > 0)
    assert sorted(r["fv_items"].tolist()) == np.flatnonzero(r["word_id"] >= 0).tolist()
    assert (r["word_id"] < 0).any()


def test_text_format_round_trip(tmp_path):
    voc = ref.full_tree(3, 2, seed=1)
    p = str(tmp_path / "v.txt")
    ref.write_text(voc, p)
    lines = open(p).read().split("\n")
    assert lines[0] == "3 2 0 0" and lines[-1] == "" and len(lines) == 1 + 12 + 1
    tok = lines[1].split()
    assert len(tok) == 35 and tok[0] == "0" and tok[1] == "0" and [int(t) for t in tok[2:34]] == voc["desc"][0].tolist()
    assert float(tok[34]) == voc["weight"][0]
