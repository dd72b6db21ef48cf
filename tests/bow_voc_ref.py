"""Line-by-line numpy / Python restatement of the vocabulary transform of the reference's vendored DBoW2 (no GPU, no reference access
at run time).  Paths are relative to oRB_SLAM2_Android/src/main/jni/; T = Thirdparty/DBoW2/include/DBoW2/TemplatedVocabulary.h.

A vocabulary is the array form of include/slamit.h (slamit_voc_desc): dict k, L, scoring, weighting, parent (n) i32, is_leaf (n) u8,
desc (n, 32) u8, weight (n) f64; entry i is node id i + 1, the root is 0, word ids count the leaves in order.  Sums are Python float
(IEEE double) additions one after the other, in the reference's order: never np.sum, which adds pairwise."""
import numpy as np

_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def distance(a, b):
    """FORB::distance (Thirdparty/DBoW2/src/FORB.cpp:81-101): the Hamming distance of two 32-byte descriptors."""
    return int(_POP[np.bitwise_xor(a, b)].sum())   # (an integer count: the order of this sum cannot matter)


class Vocabulary:
    """m_nodes of T:1345-1440 as loadFromTextFile leaves them: children in push_back order, word ids for the leaves."""

    def __init__(self, voc):
        self.k, self.L = int(voc["k"]), int(voc["L"])
        self.parent = np.asarray(voc["parent"], np.int64)
        n = len(self.parent)
        self.desc = np.concatenate([np.zeros((1, 32), np.uint8), np.asarray(voc["desc"], np.uint8).reshape(n, 32)])
        self.weight = np.concatenate([[0.0], np.asarray(voc["weight"], np.float64)])
        self.children = [[] for _ in range(n + 1)]
        self.word_id = np.full(n + 1, -1, np.int64)
        nw = 0
        for i in range(n):                                   # T:1396-1438
            nid, pid = i + 1, int(self.parent[i])
            self.children[pid].append(nid)                   # :1410
            if voc["is_leaf"][i] > 0:                        # :1426-1433
                self.word_id[nid] = nw
                nw += 1
        self.n_words = nw

    def transform_feature(self, feature, levelsup):
        """T:1225-1266 -> (word_id, weight, nid).  The reference leaves nid unset when the leaf lies above level L - levelsup
        (:1158, :1258); the project defines it as the leaf's own id there (include/slamit.h)."""
        nid_level = self.L - levelsup                        # :1233
        nid = 0 if nid_level <= 0 else None                  # :1234
        final_id, current_level = 0, 0                       # :1236-1237
        while True:                                          # do { ... } while (!isLeaf())
            current_level += 1
            nodes = self.children[final_id]                  # :1242
            final_id = nodes[0]
            best_d = distance(feature, self.desc[final_id])  # :1245
            for cid in nodes[1:]:                            # :1247-1256
                d = distance(feature, self.desc[cid])
                if d < best_d:
                    best_d, final_id = d, cid
            if current_level == nid_level:                   # :1258
                nid = final_id
            if not self.children[final_id]:                  # :1261, isLeaf() = children.empty()
                break
        if nid is None:
            nid = final_id
        return int(self.word_id[final_id]), float(self.weight[final_id]), nid

    def transform(self, features, levelsup):
        """T:1133-1201 for TF_IDF / TF with L1_NORM -> dict in the layout of api.ORBVocabulary.transform."""
        features = np.asarray(features, np.uint8).reshape(-1, 32)
        n = len(features)
        word = np.full(n, -1, np.int32)
        node = np.zeros(n, np.int32)
        v, fv = {}, {}
        for i in range(n):                                   # :1155-1169
            wid, w, nid = self.transform_feature(features[i], levelsup)
            node[i] = nid
            if w > 0:                                        # :1164 not stopped
                word[i] = wid
                add_weight(v, wid, w)
                add_feature(fv, nid, i)
        normalize_l1(v)                                      # :1200 (L1_NORM: mustNormalize)
        return pack(word, node, v, fv)


def add_weight(v, wid, w):
    """BowVector::addWeight (Thirdparty/DBoW2/src/BowVector.cpp:34-46): the first feature inserts, the later ones add."""
    if wid in v:
        v[wid] += w
    else:
        v[wid] = w


def normalize_l1(v):
    """BowVector::normalize, L1 (BowVector.cpp:62-84): norm over ascending word ids from 0.0, then a division per value."""
    norm = 0.0
    for wid in sorted(v):
        norm += abs(v[wid])
    if norm > 0.0:
        for wid in v:
            v[wid] /= norm


def add_feature(fv, nid, i_feature):
    """FeatureVector::addFeature (Thirdparty/DBoW2/src/FeatureVector.cpp:31-45)."""
    fv.setdefault(nid, []).append(i_feature)


def pack(word, node, v, fv):
    """The two std::maps in iteration (ascending key) order: BowVector as two arrays, FeatureVector as CSR."""
    wids, nids = sorted(v), sorted(fv)
    ptr = np.zeros(len(nids) + 1, np.int32)
    for j, nid in enumerate(nids):
        ptr[j + 1] = ptr[j] + len(fv[nid])
    items = np.array([i for nid in nids for i in fv[nid]], np.int32)
    return {"word_id": word, "node_id": node, "bow_word": np.array(wids, np.int32), "bow_value": np.array([v[w] for w in wids], np.float64),
            "fv_node": np.array(nids, np.int32), "fv_ptr": ptr, "fv_items": items}


def groups(fv1, fv2):
    """The nodes two FeatureVectors share, ascending (the lower_bound walk of ORBmatcher.cc:178-270), as bow_search groups."""
    n2 = {int(nid): j for j, nid in enumerate(fv2["fv_node"])}
    g = {"q_ptr": [0], "q_idx": [], "c_ptr": [0], "c_idx": []}
    for a, nid in enumerate(fv1["fv_node"]):
        if int(nid) in n2:
            b = n2[int(nid)]
            g["q_idx"] += list(fv1["fv_items"][fv1["fv_ptr"][a]:fv1["fv_ptr"][a + 1]])
            g["c_idx"] += list(fv2["fv_items"][fv2["fv_ptr"][b]:fv2["fv_ptr"][b + 1]])
            g["q_ptr"].append(len(g["q_idx"]))
            g["c_ptr"].append(len(g["c_idx"]))
    return {k: np.asarray(v, np.int32) for k, v in g.items()}


def write_text(voc, path, trailing_newline=True):
    """The format loadFromTextFile reads (T:1366-1375 header 'k L scoring weighting', :1407-1424 'parent is_leaf 32 bytes weight').
    repr() of a double round-trips, so the loaded weights are the written ones."""
    lines = ["%d %d %d %d" % (voc["k"], voc["L"], voc["scoring"], voc["weighting"])]
    for i in range(len(voc["parent"])):
        lines.append("%d %d %s %s" % (voc["parent"][i], voc["is_leaf"][i], " ".join(str(int(b)) for b in voc["desc"][i]), repr(float(voc["weight"][i]))))
    with open(path, "w") as f:
        f.write("\n".join(lines) + ("\n" if trailing_newline else ""))


# ---- fixture builders: a seed -> the array form -------------------------------------------------------------------------------

def _voc(k, L, parent, is_leaf, desc, weight):
    return {"k": k, "L": L, "scoring": 0, "weighting": 0, "parent": np.asarray(parent, np.int32), "is_leaf": np.asarray(is_leaf, np.uint8),
            "desc": np.asarray(desc, np.uint8).reshape(-1, 32), "weight": np.asarray(weight, np.float64)}


def tree_from_shape(k, L, kids_of, seed, stop_frac=0.0, dup_siblings=False, order="dfs"):
    """kids_of(node id, level) -> number of children.  Nodes are numbered depth first (as DBoW2 saves a trained tree's nodes the ids
    of siblings are not adjacent) or breadth first; random centroids, positive random weights, stop_frac of the leaves at weight 0;
    dup_siblings: the second child of every node repeats the first one's centroid."""
    rs = np.random.RandomState(seed)
    parent, level = [], []
    if order == "dfs":
        def grow(pid, lev):
            for _ in range(kids_of(pid, lev)):
                parent.append(pid)
                level.append(lev + 1)
                grow(len(parent), lev + 1)
        grow(0, 0)
    else:
        frontier = [(0, 0)]
        while frontier:
            nxt = []
            for pid, lev in frontier:
                for _ in range(kids_of(pid, lev)):
                    parent.append(pid)
                    level.append(lev + 1)
                    nxt.append((len(parent), lev + 1))
            frontier = nxt
    n = len(parent)
    has_kids = np.zeros(n + 1, bool)
    has_kids[np.asarray(parent)] = True
    is_leaf = (~has_kids[1:]).astype(np.uint8)
    desc = rs.randint(0, 256, (n, 32)).astype(np.uint8)
    if dup_siblings:
        seen = {}
        for i, p in enumerate(parent):
            c = seen.setdefault(p, [i, 0])
            if c[1] == 1:
                desc[i] = desc[c[0]]
            c[1] += 1
    weight = rs.uniform(0.05, 9.0, n)
    weight[rs.uniform(size=n) < stop_frac] = 0.0
    return _voc(k, L, parent, is_leaf, desc, weight)


def full_tree(k, L, seed, **kw):
    return tree_from_shape(k, L, lambda nid, lev: k if lev < L else 0, seed, **kw)


def unbalanced_tree(seed, L=4):
    """k = 3, header L = 4: the root's first child is a leaf (level 1), its second child's children are leaves (level 2 = L - 2:
    exactly the FeatureVector's level at levelsup 2), the rest is full."""
    def kids(nid, lev):
        if lev == 0:
            return 3
        if nid == 1:
            return 0
        if lev == 1 and nid == 2:
            return 3
        if lev == 2 and kids.under2 > 0:
            kids.under2 -= 1
            return 0
        return 3 if lev < L else 0
    kids.under2 = 3
    return tree_from_shape(3, L, kids, seed, order="bfs")


def queries(voc, n, seed, near=0.7):
    """n descriptors: a share `near` are centroids of random nodes with a few bits flipped (so descents spread over the tree and reach
    every level), the rest random."""
    rs = np.random.RandomState(seed)
    q = rs.randint(0, 256, (n, 32)).astype(np.uint8)
    pick = rs.uniform(size=n) < near
    src = voc["desc"][rs.randint(0, len(voc["desc"]), n)]
    flips = np.zeros((n, 32), np.uint8)
    for _ in range(6):
        flips[np.arange(n), rs.randint(0, 32, n)] ^= (1 << rs.randint(0, 8, n)).astype(np.uint8)
    q[pick] = (src ^ flips)[pick]
    return q


def equidistant_queries(voc, n, seed):
    """Queries at the same distance from the first two children of the root: the centroid of one with half of the bits in which the two
    differ taken from the other (an odd number of differing bits leaves a distance of one: still a valid query)."""
    rs = np.random.RandomState(seed)
    kids = [i for i, p in enumerate(voc["parent"]) if p == 0][:2]
    a, b = voc["desc"][kids[0]], voc["desc"][kids[1]]
    diff = np.flatnonzero(np.unpackbits(a ^ b))
    out = np.zeros((n, 32), np.uint8)
    for i in range(n):
        bits = np.unpackbits(a)
        take = rs.permutation(diff)[:len(diff) // 2]
        bits[take] ^= 1
        out[i] = np.packbits(bits)
    return out
