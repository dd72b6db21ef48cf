"""Writes tests/golden/bow_*.npz: what the REFERENCE's own DBoW2 (oracle/_ref/libdbow_ref.so, built by oracle/Makefile.ref in the
authoring container; oracle/dbow_ref_harness.cc) computes for small vocabularies, one file per vocabulary.  Every expected array in
these files came out of the reference's code; tests/bow_voc_ref.py and tests/kfdb_ref.py supply the INPUTS only (their builders).

    python tools/gen_bow_golden.py            # regenerates byte-identical files, prints sizes and the conditions checked

Layout of a file (tests/bow_golden.py reads it):
  k L scoring weighting parent is_leaf desc weight   the vocabulary, the array form of slamit_voc_desc
  text                                               (bytes,) u8: the exact text handed to loadFromTextFile -- no trailing newline:
                                                     with one the reference makes a phantom node whose descriptor real OpenCV
                                                     leaves uninitialised
  q                                                  (N, 32) u8 descriptors
  frames                                             (F, 2) i32: frame f is q[start : start + count]
  levelsups                                          (nl,) i32
  info                                               k L scoring weighting n_nodes n_words as the reference reports them
  f{f}_l{levelsup}_{name} per frame and levelsup:
    word_id       transform(feature) (public, T:1057): the word, also where it is stopped
    word_weight   the weight the protected transform(feature, id, weight, &nid, levelsup) returns (0 = stopped word)
    node_id       its nid, preset to -1: -1 = the reference never wrote it
    bow_word bow_value(u64 bit patterns) fv_node fv_ptr fv_items       transform(features, v, fv, levelsup)
  unbalanced tree: bow_* from transform(features, v); no fv_* (the reference keys it by an indeterminate id there, and the call that
    would is not made)
  score                                              (F, F) u64: bits of score(frame i's BowVector, frame j's): [i, j] and [j, i]
                                                     are the two argument orders
"""
import io
import os
import sys
import tempfile
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import bindings as ob          # noqa: E402
from tests import bow_voc_ref as ref       # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
LIMIT = 383 * 1024                         # the largest fixture tests/golden held before these


def _k10():
    voc = ref.full_tree(10, 3, 11, stop_frac=0.2)
    return voc, ref.queries(voc, 300, 21), [(0, 300), (0, 150), (100, 200), (250, 50), (1, 1), (2, 1), (7, 1)], (1, 2)   # two one-word frames; one whose only word is stopped


def _k3l6():
    voc = ref.full_tree(3, 6, 12, stop_frac=0.2)   # k4 L6 does not fit the size limit: 5,460 nodes, ~500 KB with its text
    return voc, ref.queries(voc, 300, 22), [(0, 300), (0, 160), (140, 160)], (4,)


def _k20():
    voc = ref.full_tree(20, 2, 14, stop_frac=0.2)
    return voc, ref.queries(voc, 100, 24), [(0, 100), (0, 60), (40, 60)], (1,)


def _k3l2():
    voc = ref.full_tree(3, 2, 13)
    return voc, ref.queries(voc, 66, 23), [(0, 1), (1, 65)], (0, 1, 3)


def _ties():
    voc = ref.full_tree(5, 3, 16, dup_siblings=True)
    return voc, np.concatenate([ref.queries(voc, 120, 26), ref.equidistant_queries(voc, 80, 27)]), [(0, 200), (0, 120), (60, 140)], (1,)


def _tf():
    voc = ref.full_tree(4, 2, 17, stop_frac=0.2)
    voc["weighting"] = 1
    voc["weight"] = np.where(voc["weight"] > 0, 1.0, 0.0)    # what DBoW2's setNodeWeights gives a TF vocabulary, and stopWords
    return voc, ref.queries(voc, 100, 31), [(0, 100), (0, 50), (30, 70)], (1,)


def _ordered():
    voc = ref.full_tree(3, 2, 18)
    leaves = np.flatnonzero(voc["is_leaf"] > 0)
    voc["weight"][leaves] = np.random.RandomState(19).permutation(10.0 ** np.linspace(-2.0, 2.0, len(leaves)))   # four decades
    return voc, ref.queries(voc, 1500, 32), [(0, 1500), (0, 700), (500, 1000)], (1,)


def _unbalanced():
    voc = ref.unbalanced_tree(15)
    return voc, ref.queries(voc, 200, 25, near=0.9), [(0, 200), (0, 100), (80, 120)], (2, 1)


CASES = (("k10L3", _k10), ("k3L6", _k3l6), ("k20L2", _k20), ("k3L2", _k3l2), ("ties", _ties), ("tf", _tf), ("ordered", _ordered),
         ("unbalanced", _unbalanced))


def write_npz(path, arrays):
    """np.savez_compressed with fixed member dates and order, so the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            a = np.asarray(arrays[name])
            np.lib.format.write_array(buf, a if a.ndim == 0 else np.ascontiguousarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def tied_descents(voc, q, word_id):
    """From the inputs and the reference's word ids alone: the queries for which, at some level of the path to the reference's leaf,
    two or more children lie at the least distance."""
    leaves = np.flatnonzero(voc["is_leaf"] > 0) + 1
    kids = {}
    for i, p in enumerate(voc["parent"]):
        kids.setdefault(int(p), []).append(i + 1)
    n = 0
    for d, w in zip(q, word_id):
        nid, tie = int(leaves[w]), False
        while nid:
            pid = int(voc["parent"][nid - 1])
            dist = [int(_POP[voc["desc"][c - 1] ^ d].sum()) for c in kids[pid]]
            tie |= dist.count(min(dist)) > 1
            nid = pid
        n += tie
    return n


def generate(name, make, checks):
    voc, q, frames, levelsups = make()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "voc.txt")
        ref.write_text(voc, path, trailing_newline=False)
        text = open(path, "rb").read()
        assert not text.endswith(b"\n")
        R = ob.DbowRef(path)
    info = R.info()
    assert info["n_nodes"] == len(voc["parent"]) and info["n_words"] == int((voc["is_leaf"] > 0).sum()), (name, info)
    g = {"k": voc["k"], "L": voc["L"], "scoring": voc["scoring"], "weighting": voc["weighting"], "parent": voc["parent"].astype(np.int32),
         "is_leaf": voc["is_leaf"].astype(np.uint8), "desc": voc["desc"].astype(np.uint8), "weight": voc["weight"].astype(np.float64),
         "text": np.frombuffer(text, np.uint8), "q": q.astype(np.uint8), "frames": np.asarray(frames, np.int32),
         "levelsups": np.asarray(levelsups, np.int32), "info": np.array([info[k] for k in ("k", "L", "scoring", "weighting", "n_nodes", "n_words")], np.int32)}
    bows = []
    for f, (s, c) in enumerate(frames):
        d = q[s:s + c]
        two = R.transform_bow(d)
        bows.append(two)
        for ls in levelsups:
            per = R.features(d, ls)
            assert np.array_equal(per["word_pub"], per["word_id"]), "the reference's two per-feature overloads disagree"
            rec = {"word_id": per["word_pub"], "word_weight": per["weight"], "node_id": per["node_id"]}
            if name == "unbalanced":
                rec.update(bow_word=two[0], bow_value=two[1].view(np.uint64))
            else:
                assert (per["node_id"] >= 0).all(), "%s: an unset node id in a tree that is not the unbalanced one" % name
                full = R.transform(d, ls)
                assert np.array_equal(full["bow_word"], two[0]) and np.array_equal(full["bow_value"].view(np.uint64), two[1].view(np.uint64))
                rec.update(bow_word=full["bow_word"], bow_value=full["bow_value"].view(np.uint64), fv_node=full["fv_node"], fv_ptr=full["fv_ptr"],
                           fv_items=full["fv_items"])
            for k, a in rec.items():
                g["f%d_l%d_%s" % (f, ls, k)] = a
    nf = len(frames)
    score = np.zeros((nf, nf), np.float64)
    for i in range(nf):
        for j in range(nf):
            score[i, j] = R.score(bows[i], bows[j])
    g["score"] = score.view(np.uint64)
    R.close()

    # ---- what this golden must be able to catch, from the inputs and the reference's outputs alone ----
    ls0 = levelsups[0]
    wid, ww = g["f0_l%d_word_id" % ls0], g["f0_l%d_word_weight" % ls0]
    if name == "ordered":
        differs = 0
        for f in range(nf):
            w_, wt = g["f%d_l%d_word_id" % (f, ls0)], g["f%d_l%d_word_weight" % (f, ls0)]
            words = np.unique(w_[wt > 0])
            vals = np.array([np.sum(wt[(w_ == x) & (wt > 0)]) for x in words])      # the same terms, added pairwise
            pairwise = vals / np.sum(np.abs(vals))
            differs += int(not np.array_equal(pairwise.view(np.uint64), g["f%d_l%d_bow_value" % (f, ls0)]))
        assert differs >= 1, "ordered: np.sum gives the reference's bits on every frame: the case cannot catch a pairwise sum"
        span = voc["weight"][voc["is_leaf"] > 0]
        assert span.max() / span.min() > 9999.0
        checks.append("ordered sum: %d of %d BowVectors differ in bits from np.sum of the same terms; leaf weights span %.1e" % (differs, nf, span.max() / span.min()))
    if name == "ties":
        t = tied_descents(voc, q, wid)
        assert t >= 20, "ties: only %d queries reach two children at equal least distance" % t
        checks.append("ties: %d of %d queries reach two children at equal least distance" % (t, len(q)))
    if name == "k10L3":
        stopped, twice = int((ww == 0).sum()), int(((ww > 0).sum()) - len(g["f0_l%d_bow_word" % ls0]))
        assert stopped > 0 and twice > 0
        checks.append("k10L3: %d stopped features; %d features fall on a word that another feature already hit" % (stopped, twice))
    if name == "unbalanced":
        unset = {ls: int((g["f0_l%d_node_id" % ls] == -1).sum()) for ls in levelsups}
        assert all(v >= 1 for v in unset.values()), unset
        checks.append("unbalanced: node ids the reference never wrote (-1), per levelsup: %s" % unset)
    kinds = {"identical": 0, "one_word": 0, "disjoint": 0, "orders_differ": 0}
    for i in range(nf):
        for j in range(nf):
            shared = len(np.intersect1d(bows[i][0], bows[j][0]))
            kinds["identical"] += int(i == j and len(bows[i][0]) > 0)
            kinds["one_word"] += int(i != j and shared == 1)
            kinds["disjoint"] += int(i < j and shared == 0)
            kinds["orders_differ"] += int(i < j and g["score"][i, j] != g["score"][j, i])
    path = os.path.join(OUT, "bow_%s.npz" % name)
    write_npz(path, g)
    size = os.path.getsize(path)
    assert size < LIMIT, "%s: %d bytes" % (path, size)
    print("%-28s %7d bytes  nodes %5d words %5d  frames %s levelsups %s  score pairs %s" % (
        os.path.relpath(path, ROOT), size, info["n_nodes"], info["n_words"], [c for _, c in frames], list(levelsups), kinds))
    return kinds


def main():
    if not ob.dbow_ref_available():
        sys.exit("oracle/_ref/libdbow_ref.so is missing: make -C oracle -f Makefile.ref (authoring container only)")
    checks, total = [], {}
    for name, make in CASES:
        for k, v in generate(name, make, checks).items():
            total[k] = total.get(k, 0) + int(v)
    for c in checks:
        print("checked:", c)
    for k in ("identical", "one_word", "disjoint"):
        assert total[k] >= 1, "no score pair of kind %s in any golden" % k
    print("checked: score pairs over all files:", total)
    if total["orders_differ"] == 0:
        print("NOTE: no pair of sub-frames scores differently in its two argument orders; both orders are compared anyway")


if __name__ == "__main__":
    main()
