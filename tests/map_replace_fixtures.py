"""The maps and op lists of the map-replace tests, the smallest shapes that can go wrong.  A fixture is dict(name, t, x, ops): t in the
layout of slamit_map_index, x the columns beside it (obs_idx, obs_octave, obs_weight, mp_nobs, mp_ref_kf of tests/map_edit_fixtures.py
and mp_found, mp_visible, mp_replaced), ops tuples (kind, a, b, idx, octave, weight).  The maps are built by build_map of the map-edit
fixtures: consistent, with free keypoints at the end of every keyframe's row for adds."""
import functools

import numpy as np

from tests.map_edit_fixtures import build_map, free_idx, idx_of
from tests.map_replace_ref import ADD_OBS, REPLACE


def with_counters(t, x, seed=1, replaced=None, found=None, visible=None):
    rng = np.random.default_rng(seed)
    n_mp = t["n_mp"]
    x = dict(x, mp_found=rng.integers(0, 50, n_mp).astype(np.int32), mp_visible=rng.integers(50, 100, n_mp).astype(np.int32), mp_replaced=np.full(n_mp, -1, np.int32))
    for key, vals in (("mp_replaced", replaced), ("mp_found", found), ("mp_visible", visible)):
        for p, v in (vals or {}).items():
            x[key][p] = v
    return t, x


def R(a, b):
    return (REPLACE, a, b, 0, 0, 0)


def A(t, p, k, j=0, octave=3, weight=1):
    return (ADD_OBS, p, k, free_idx(t, k, j), octave, weight)


def single():
    """Every single-Replace case of the issue in one interleaved list over disjoint groups of points."""
    rows = [[0, 1, 2], [3, 4],          # 0 -> 1    disjoint observers: all move
            [0, 1, 5], [1, 5, 6],       # 2 -> 3    overlapping: keyframes 1 and 5 die, 0 moves
            [2, 3],                     # 4 -> 4    a == b
            [4, 6], [0], [1],           # 5 -> 6, then 5 -> 7: S already replaced moves nothing, the counters add again, mp_replaced is overwritten
            [2, 7], [3],                # 8 -> 9    D bad
            [4, 5], [],                 # 10 -> 11  D an empty slot
            [7, 3, 1], [0],             # 12 -> 13  S stored out of slot order: D receives 1, 3, 7
            [], [6, 2],                 # 14 -> 15  S replaced before the call (bad, empty, mp_replaced = 2)
            [0, 1], [0, 1]]             # 16 -> 17  the same observers: all die
    t, x = build_map(8, rows, weights={(0, 1): 2, (2, 5): 2, (12, 3): 2}, bad=(9, 14), nobs={14: 4, 9: 1})
    t, x = with_counters(t, x, 3, replaced={14: 2}, found={0: 2 ** 31 - 1, 1: 5, 8: -2 ** 31, 9: -1})   # 0 -> 1 wraps upwards, 8 -> 9 downwards
    ops = [R(12, 13), R(5, 6), R(0, 1), R(4, 4), R(10, 11), R(2, 3), R(14, 15), R(5, 7), R(8, 9), R(16, 17)]
    return {"name": "single", "t": t, "x": x, "ops": ops}


def chains():
    """A -> B, B -> C in both list orders, and the cycle A -> B, B -> A."""
    rows = [[0, 1], [1, 2], [2, 3],     # 0 -> 1 then 1 -> 2: the sums are carried along
            [0, 4], [4, 5], [5, 6],     # 4 -> 5 then 3 -> 4: 3's entries stop at 4, which is bad by then
            [1, 6], [6, 7]]             # 6 -> 7 then 7 -> 6: everything returns to the bad 6
    t, x = with_counters(*build_map(8, rows), seed=4)
    return {"name": "chains", "t": t, "x": x, "ops": [R(0, 1), R(4, 5), R(6, 7), R(3, 4), R(1, 2), R(7, 6)]}


def deep(depth=300):
    """A chain `depth` deep, i -> i + 1: more rounds than wavefronts, one ready op per round."""
    n_kf = 40
    rows = [[(3 * p) % n_kf, (3 * p + 7) % n_kf] for p in range(depth + 1)]
    t, x = with_counters(*build_map(n_kf, rows, spare=2), seed=5)
    return {"name": "deep", "t": t, "x": x, "ops": [R(i, i + 1) for i in range(depth)]}


def fan(n_src):
    """n_src sources into point 0, which the list names n_src times."""
    n_kf = 2 * n_src + 2
    rows = [[0, 1]] + [[1 + s, 2 + s + n_src] for s in range(n_src)]   # source 0 shares keyframe 1 with the target
    t, x = with_counters(*build_map(n_kf, rows, spare=1), seed=6)
    order = np.random.default_rng(n_src).permutation(n_src) + 1
    return {"name": "fan%d" % n_src, "t": t, "x": x, "ops": [R(int(s), 0) for s in order]}


def row_ceiling(name, len_d, len_s, add=False):
    """D holds len_d keyframes, S len_s others, and two more reach S from point 2 first: the ceiling is met through a chain."""
    n_kf = 600
    rows = [list(range(len_d)), list(range(len_d, len_d + len_s)), [598, 597]]
    t, x = with_counters(*build_map(n_kf, rows, spare=1), seed=7)
    ops = [R(2, 1), R(1, 0), A(t, 0, 5)]                                # the add of a present observer needs no room
    if add:
        ops.append(A(t, 0, 599))                                        # one onto MAX_OBS entries
    return {"name": name, "t": t, "x": x, "ops": ops}


def add_order():
    """ADD_OBS of k onto D before Replace(S -> D) with S holding k: S's entry dies.  After it: the add is a no-op on the row."""
    rows = [[0, 1], [2],                # S = 0, D = 1: add (1, kf 0) first
            [0, 1], [2],                # S = 2, D = 3: add (3, kf 0) afterwards
            [3]]
    t, x = with_counters(*build_map(4, rows), seed=8)
    ops = [A(t, 1, 0, 0, 5, 2), R(2, 3), R(0, 1), A(t, 3, 0, 1, 6, 1), A(t, 4, 3, 0, 1, 1), A(t, 4, 2, 0, 2, 2)]
    return {"name": "add_order", "t": t, "x": x, "ops": ops}


def shared():
    """Two points hold one (k, idx), as Fuse leaves them before its Replace: the write with the largest list index stays."""
    rows = [[0, 1], [0, 2], [3], [4], [0, 5], [0, 6], [0, 5]]
    t, x = with_counters(*build_map(7, rows), seed=9)
    x = dict(x, obs_idx=x["obs_idx"].copy())
    for p, q in ((0, 1), (4, 5)):                                       # q's keypoint in keyframe 0 becomes p's
        x["obs_idx"][t["obs_ptr"][q]] = idx_of(t, x, p, 0)
    # 0 -> 2 writes 2 there, then 1 -> 3 writes 3; 5 -> 6 (6 observes 0: dies, -1) then 4 -> 6 (dies too)
    return {"name": "shared", "t": t, "x": x, "ops": [R(0, 2), R(5, 6), R(1, 3), R(4, 6)]}


def random_fixture(name, seed, n_kf, n_mp, n_ops, density=3.0, independent=False, kp_spare=8):
    """A random consistent map and a random shuffled list of both kinds; independent: no point is named twice."""
    rng = np.random.default_rng(seed)
    lens = np.minimum(rng.poisson(density, n_mp), n_kf)
    rows = [sorted(rng.choice(n_kf, int(l), replace=False).tolist(), key=lambda k: (k * 7) % 5) for l in lens]
    t, x = build_map(n_kf, rows, spare=kp_spare, weights={(p, rows[p][0]): 2 for p in range(0, n_mp, 5) if rows[p]})
    t, x = with_counters(t, x, seed)
    perm = rng.permutation(n_mp).tolist()
    ops, spare_used, named = [], {}, {}
    while len(ops) < n_ops:
        if independent:
            a, b = perm.pop(), perm.pop()
        else:
            a, b = (int(v) for v in rng.integers(0, min(n_mp, max(4 * n_ops, 8)), 2))
            if len(ops) % 2 == 0:                                       # the table's far end too
                a, b = n_mp - 1 - a, n_mp - 1 - b
        if rng.random() < 0.55:
            if not independent and (named.get(a, 0) > 40 or named.get(b, 0) > 40):
                continue
            named[a], named[b] = named.get(a, 0) + 1, named.get(b, 0) + 1
            ops.append(R(a, b))
        else:
            if not independent and named.get(a, 0) > 40:
                continue
            named[a] = named.get(a, 0) + 1
            k = int(rng.integers(0, n_kf))
            j = spare_used.get(k, 0)
            spare_used[k] = (j + 1) % kp_spare
            ops.append(A(t, a, k, j, int(rng.integers(0, 8)), int(rng.integers(1, 3))))
    return {"name": name, "t": t, "x": x, "ops": ops}


@functools.lru_cache(maxsize=None)
def all_fixtures():
    fxs = [single(), chains(), deep(), fan(20), fan(64), fan(65), add_order(), shared(),
           row_ceiling("row512", 500, 10), row_ceiling("row513", 500, 11), row_ceiling("row513_in", 3, 513), row_ceiling("row512_add", 500, 10, add=True),
           random_fixture("indep", 21, 30, 900, 400, independent=True),
           random_fixture("ops0", 22, 9, 30, 0), random_fixture("ops1", 23, 12, 255, 1), random_fixture("ops63", 24, 12, 256, 63),
           random_fixture("ops64", 25, 12, 257, 64), random_fixture("ops65", 26, 20, 300, 65),
           random_fixture("ops1025", 27, 64, 65537, 1025, density=1.5)]
    return tuple(fxs)


@functools.lru_cache(maxsize=None)
def ceiling_fixtures():
    """Lists of MAX_OPS ops: one of independent ops (a single round, the most involved points a list can name) and one chain MAX_OPS
    deep (as many rounds as ops)."""
    from tests.map_replace_ref import MAX_OPS

    wide = random_fixture("ceiling_wide", 28, 30, 2 * MAX_OPS + 5, MAX_OPS, density=1.5, independent=True)
    return wide, dict(deep(MAX_OPS), name="ceiling_deep")


def by_name(name):
    return next(fx for fx in all_fixtures() if fx["name"] == name)


@functools.lru_cache(maxsize=None)
def expected(name, cap_delta=None):
    """The restatement's result on a fixture, computed once and shared.  cap_delta: obs_cap_out = the need + cap_delta."""
    from tests.map_replace_ref import apply

    fx = by_name(name)
    if cap_delta is None:
        return apply(fx["t"], fx["x"], fx["ops"])
    return apply(fx["t"], fx["x"], fx["ops"], expected(name)["n_obs_out"] + cap_delta)
