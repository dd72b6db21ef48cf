"""Reader of tests/golden/bow_*.npz (tools/gen_bow_golden.py): what the reference's own DBoW2 computed for eight small vocabularies.
Nothing here restates the reference; the two places where the project's outputs are DEFINED differently from the raw reference
outputs are spelled out in expected():
  - word_id is -1 for a stopped word (the reference returns the word and a weight of 0, and then skips the feature, T:1164);
  - node_id is the leaf's own id where the reference never wrote one (include/slamit.h; the golden records -1 there)."""
import os

import numpy as np

from tests.helpers import ROOT

CASES = ("k10L3", "k3L6", "k20L2", "k3L2", "ties", "tf", "ordered", "unbalanced")
KEYS = ("word_id", "node_id", "bow_word", "bow_value", "fv_node", "fv_ptr", "fv_items")

_CACHE = {}


class Golden:
    def __init__(self, name):
        z = np.load(os.path.join(ROOT, "tests", "golden", "bow_%s.npz" % name))
        self.name = name
        self.a = {k: z[k] for k in z.files}
        for v in self.a.values():
            v.setflags(write=False)
        a = self.a
        self.voc = {"k": int(a["k"]), "L": int(a["L"]), "scoring": int(a["scoring"]), "weighting": int(a["weighting"]), "parent": a["parent"],
                    "is_leaf": a["is_leaf"], "desc": a["desc"], "weight": a["weight"]}
        self.text = a["text"].tobytes()
        self.frames = [(int(s), int(c)) for s, c in a["frames"]]
        self.levelsups = [int(v) for v in a["levelsups"]]
        self.info = dict(zip(("k", "L", "scoring", "weighting", "n_nodes", "n_words"), (int(v) for v in a["info"])))
        self.leaf_node = (np.flatnonzero(a["is_leaf"] > 0) + 1).astype(np.int32)      # word id -> node id: the leaves in file order
        self.score = a["score"]                                                      # (F, F) u64
        self.has_fv = "f0_l%d_fv_node" % self.levelsups[0] in a

    def desc(self, f):
        s, c = self.frames[f]
        return self.a["q"][s:s + c]

    def raw(self, f, levelsup, key):
        return self.a["f%d_l%d_%s" % (f, levelsup, key)]

    def unset(self, f, levelsup):
        return self.raw(f, levelsup, "node_id") == -1

    def expected(self, f, levelsup):
        """The golden of (frame, levelsup) in the layout of api.ORBVocabulary.transform; bow_value as float64 of the golden's bits."""
        word, weight, node = (self.raw(f, levelsup, k) for k in ("word_id", "word_weight", "node_id"))
        out = {"word_id": np.where(weight > 0, word, -1).astype(np.int32),
               "node_id": np.where(node == -1, self.leaf_node[word], node).astype(np.int32),
               "bow_word": self.raw(f, levelsup, "bow_word"), "bow_value": self.raw(f, levelsup, "bow_value").view(np.float64)}
        if self.has_fv:
            out.update({k: self.raw(f, levelsup, k) for k in ("fv_node", "fv_ptr", "fv_items")})
        return out

    def bow(self, f):
        e = self.expected(f, self.levelsups[0])
        return e["bow_word"], e["bow_value"]


def golden(name):
    if name not in _CACHE:
        _CACHE[name] = Golden(name)
    return _CACHE[name]


def same(got, want, tag=""):
    """Every array of `want` equal in `got`; the BowVector's doubles as bit patterns."""
    for k in KEYS:
        if k not in want:
            continue
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if k == "bow_value":
            g, w = g.view(np.uint64), w.view(np.uint64)
        assert g.shape == w.shape and np.array_equal(g, w), "%s %s differs at %s" % (
            tag, k, np.flatnonzero(g != w)[:8] if g.shape == w.shape else (g.shape, w.shape))

