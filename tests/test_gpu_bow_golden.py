"""GPU parity against the reference's own DBoW2: the vocabulary transform (csrc/voc.hip), the text loader (csrc/voc_pack.cc through
slamit_voc_load_text) and the score pass of the keyframe database (csrc/kfdb.hip) against tests/golden/bow_*.npz, which
tools/gen_bow_golden.py recorded from the reference's code (tests/bow_golden.py reads them).  The expected values are the golden
arrays, not tests/bow_voc_ref.py or tests/kfdb_ref.py.  Bar: every array equal, the doubles as bit patterns."""
import numpy as np
import pytest

from tests.bow_golden import CASES, golden, same
from weiner_slamit_v2_amd import api

pytestmark = pytest.mark.gpu

SENT_I, SENT_D = -777, -7.5
_VOCS = {}


def device_voc(name):
    if name not in _VOCS:
        v = golden(name).voc
        _VOCS[name] = api.ORBVocabulary.from_arrays(v["k"], v["L"], v["parent"], v["is_leaf"], v["desc"], v["weight"], scoring=v["scoring"],
                                                    weighting=v["weighting"])
    return _VOCS[name]


def check_every_frame(v, g, tag):
    for f in range(len(g.frames)):
        for ls in g.levelsups:
            got = v.transform(g.desc(f), ls)
            same(got, g.expected(f, ls), "%s %s frame %d levelsup %d" % (tag, g.name, f, ls))
            unset = g.unset(f, ls)                             # the reference never wrote the node id: here it is the leaf's own
            assert np.array_equal(got["node_id"][unset], g.leaf_node[g.raw(f, ls, "word_id")[unset]])


@pytest.mark.parametrize("name", CASES)
def test_from_arrays_transform_equals_the_reference(name):
    g = golden(name)
    check_every_frame(device_voc(name), g, "from_arrays")
    if name == "unbalanced":
        assert all(g.unset(0, ls).any() for ls in g.levelsups)


@pytest.mark.parametrize("name", CASES)
def test_load_text_of_the_golden_text_equals_the_reference(name, tmp_path):
    g = golden(name)
    p = tmp_path / "voc.txt"
    p.write_bytes(g.text)
    v = api.ORBVocabulary.load_text(str(p))
    assert v.info() == {k: g.info[k] for k in ("k", "L", "n_nodes", "n_words")}
    check_every_frame(v, g, "load_text")
    v.close()


def _transform_tensors(torch, g, cap):
    nf = len(g.frames)
    desc = np.full((nf, cap, 32), 0xA5, np.uint8)              # rows past a frame's count are not descriptors
    for f in range(nf):
        desc[f, :g.frames[f][1]] = g.desc(f)
    i32 = lambda *shape: torch.full(shape, SENT_I, dtype=torch.int32, device="cuda")   # noqa: E731
    return {"desc": torch.from_numpy(desc).cuda(), "n": torch.tensor([c for _, c in g.frames], dtype=torch.int32, device="cuda"),
            "word_id": i32(nf, cap), "node_id": i32(nf, cap), "bow_n": i32(nf), "bow_word": i32(nf, cap),
            "bow_value": torch.full((nf, cap), SENT_D, dtype=torch.float64, device="cuda"), "fv_n": i32(nf), "fv_node": i32(nf, cap),
            "fv_ptr": i32(nf, cap + 1), "fv_items": i32(nf, cap),
            "workspace": torch.zeros(api.ORBVocabulary.transform_workspace(nf, cap), dtype=torch.uint8, device="cuda")}


@pytest.mark.parametrize("name", CASES)
def test_transform_batch_dev_equals_the_reference_frame_by_frame(name):
    """All frames of the vocabulary in one launch, cap above every count; what lies past a frame's counts keeps its sentinel."""
    import torch

    g = golden(name)
    v = device_voc(name)
    cap = max(c for _, c in g.frames) + 3
    for ls in g.levelsups:
        t = _transform_tensors(torch, g, cap)
        v.transform_batch_dev(t, levelsup=ls)
        torch.cuda.synchronize()
        h = {k: a.cpu().numpy() for k, a in t.items()}
        for f, (_, n) in enumerate(g.frames):
            nb, nfv = int(h["bow_n"][f]), int(h["fv_n"][f])
            assert 0 <= nb <= n and 0 <= nfv <= n
            items = int(h["fv_ptr"][f, nfv])
            got = {"word_id": h["word_id"][f, :n], "node_id": h["node_id"][f, :n], "bow_word": h["bow_word"][f, :nb], "bow_value": h["bow_value"][f, :nb],
                   "fv_node": h["fv_node"][f, :nfv], "fv_ptr": h["fv_ptr"][f, :nfv + 1], "fv_items": h["fv_items"][f, :items]}
            same(got, g.expected(f, ls), "%s frame %d levelsup %d" % (name, f, ls))
            assert items == int((got["word_id"] >= 0).sum())
            assert (h["word_id"][f, n:] == SENT_I).all() and (h["node_id"][f, n:] == SENT_I).all()
            assert (h["bow_word"][f, nb:] == SENT_I).all() and (h["bow_value"][f, nb:] == SENT_D).all()
            assert (h["fv_node"][f, nfv:] == SENT_I).all() and (h["fv_ptr"][f, nfv + 1:] == SENT_I).all() and (h["fv_items"][f, items:] == SENT_I).all()


def _check_scores(g, i, common, score, tag):
    """Row i: frame i's BowVector is the query, so its value is vi (include/slamit.h) -- the golden's score[i, j]."""
    bows = [g.bow(f) for f in range(len(g.frames))]
    want = np.array([len(np.intersect1d(bows[i][0], b[0])) for b in bows], np.int32)   # the shared words, from the golden's ids
    assert np.array_equal(common, want), "%s %s query %d common" % (tag, g.name, i)
    m = want >= 1
    assert np.array_equal(score.view(np.uint64)[m], g.score[i][m]), "%s %s query %d score bits" % (tag, g.name, i)


@pytest.mark.parametrize("name", CASES)
def test_kfdb_scores_equal_the_reference_in_the_stated_argument_order(name):
    g = golden(name)
    nf = len(g.frames)
    db = api.KeyFrameDatabase(nf, max(max(len(g.bow(f)[0]) for f in range(nf)), 1))
    for f in range(nf):
        assert db.add(*g.bow(f)) == f
    for i in range(nf):
        common, first, seq, score = db.query(*g.bow(i))
        _check_scores(g, i, common, score, "host form")
    db.close()


@pytest.mark.parametrize("name", CASES)
def test_kfdb_resident_chain_equals_the_reference(name):
    """transform_batch_dev -> add_dev of every frame -> query_batch_dev fed with the transform's own outputs, nothing through the host."""
    import torch

    g = golden(name)
    v = device_voc(name)
    nf = len(g.frames)
    cap = max(c for _, c in g.frames) + 3
    t = _transform_tensors(torch, g, cap)
    db = api.KeyFrameDatabase(nf, cap)
    out = {"common": torch.full((nf, nf), SENT_I, dtype=torch.int32, device="cuda"), "first_word": torch.full((nf, nf), SENT_I, dtype=torch.int32, device="cuda"),
           "score": torch.full((nf, nf), SENT_D, dtype=torch.float64, device="cuda")}
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    v.transform_batch_dev(t, levelsup=g.levelsups[0], stream=s.cuda_stream)
    for f in range(nf):
        assert db.add_dev(t["bow_n"][f:f + 1], t["bow_word"][f], t["bow_value"][f], stream=s.cuda_stream) == f
    db.query_batch_dev({"bow_n": t["bow_n"], "bow_word": t["bow_word"], "bow_value": t["bow_value"], **out}, stream=s.cuda_stream)
    s.synchronize()
    for i in range(nf):
        _check_scores(g, i, out["common"][i].cpu().numpy(), out["score"][i].cpu().numpy(), "resident")
    db.close()
