"""Maps and op lists for the KeyFrame::SetBadFlag tests: the smallest shapes at which the walk can go wrong, each with what it pins.
A fixture is {"name", "t": tables in the layout of slamit_map_index, "x": the arrays of slamit_tree_index, "ops": [(kind, kf, parent)]}."""
import functools

import numpy as np

from tests.kf_erase_ref import SET_BAD, SET_PARENT

BEST = 10


def full_order(row):
    """UpdateBestCovisibles of a cw row {slot: weight}: descending weight, descending slot within equal weight."""
    return [(j, w) for w, j in sorted(((w, j) for j, w in row.items()), reverse=True)]


def sym(edges):
    cw = {}
    for a, b, w in edges:
        cw.setdefault(a, {})[b] = w
        cw.setdefault(b, {})[a] = w
    return cw


def make(name, n_kf, parent, cw, ops, ords=None, kf_mp=None, children=None, origin=0, not_erase=(), bad=(), to_be_erased=(), row_cap=8, n_mp=None, what=""):
    """parent: list (or dict) of parent slots, -1 none; cw: {j: {k: w}}; ords: {j: [(slot, weight)]} where a row is not the full sort of
    cw; kf_mp: {k: [point or -1]} (default: two points of its own per keyframe); children: {k: [slots]} where a row is not what
    `parent` implies."""
    par = [parent.get(k, -1) for k in range(n_kf)] if isinstance(parent, dict) else list(parent)
    assert len(par) == n_kf
    ords, kf_mp, children = ords or {}, kf_mp or {}, children or {}
    x = {"row_cap": row_cap, "origin_kf": origin, "kf_not_erase": np.zeros(n_kf, np.uint8), "kf_to_be_erased": np.zeros(n_kf, np.uint8)}
    for key in ("cw_kf", "cw_w", "ord_kf", "ord_w"):
        x[key] = np.full((n_kf, row_cap), -77, np.int32)    # what lies past a row's count is never read
    x["cw_n"], x["ord_n"] = np.zeros(n_kf, np.int32), np.zeros(n_kf, np.int32)
    x["kf_best"] = np.full((n_kf, BEST), -1, np.int32)
    for k in not_erase:
        x["kf_not_erase"][k] = 1
    for k in to_be_erased:
        x["kf_to_be_erased"][k] = 1
    for j in range(n_kf):
        row = sorted(cw.get(j, {}).items())
        assert len(row) <= row_cap
        x["cw_n"][j] = len(row)
        for e, (k, w) in enumerate(row):
            x["cw_kf"][j, e], x["cw_w"][j, e] = k, w
        order = ords[j] if j in ords else full_order(cw.get(j, {}))
        x["ord_n"][j] = len(order)
        for e, (k, w) in enumerate(order):
            x["ord_kf"][j, e], x["ord_w"][j, e] = k, w
            if e < BEST:
                x["kf_best"][j, e] = k
    rows = [children[k] if k in children else [c for c in range(n_kf) if par[c] == k] for k in range(n_kf)]
    kp = [list(kf_mp[k]) if k in kf_mp else [2 * k, 2 * k + 1] for k in range(n_kf)]
    t = {"n_kf": n_kf, "n_mp": n_mp if n_mp is not None else max([p for r in kp for p in r] + [0]) + 1,
         "kf_mp_ptr": np.cumsum([0] + [len(r) for r in kp]).astype(np.int32), "kf_mp": np.array([p for r in kp for p in r], np.int32),
         "kf_child_ptr": np.cumsum([0] + [len(r) for r in rows]).astype(np.int32), "kf_child": np.array([c for r in rows for c in r], np.int32),
         "kf_bad": np.zeros(n_kf, np.uint8), "kf_parent": np.array(par, np.int32)}
    for k in bad:
        t["kf_bad"][k] = 1
    return {"name": name, "t": t, "x": x, "ops": [tuple(op) + (-1,) * (3 - len(op)) for op in ops], "what": what}


def bad_of(k):
    return (SET_BAD, k, -1)


def star(n_children, name):
    """Keyframe 1 under the origin with n_children children 2 .., every second one linked to the origin (weight 20 + its slot), the others
    linked to nothing: the rounds pick the linked ones in descending weight, the rest fall back."""
    n = 2 + n_children
    edges = [(0, 1, 30)] + [(c, 0, 20 + c) for c in range(2, n, 2)] + [(c, 1, 5) for c in range(2, n)]
    return make(name, n, [-1, 0] + [1] * n_children, sym(edges), [bad_of(1)], row_cap=max(8, n), what="%d children: the LDS row, its last wavefront" % n_children)


def chain(n_kf, name, ops):
    """Keyframe i under i - 1, linked to i - 1 and i + 1 (weight 16) and to i - 2 and i + 2 (weight 15)."""
    edges = [(i, i + 1, 16) for i in range(n_kf - 1)] + [(i, i + 2, 15) for i in range(n_kf - 2)]
    return make(name, n_kf, [i - 1 for i in range(n_kf)], sym(edges), ops, what="%d keyframes: the blocks of the per-keyframe kernels" % n_kf)


def single():
    F = []
    # a leaf: its two neighbours lose it and are sorted again, it leaves its parent's row; nothing else moves
    F.append(make("leaf", 4, [-1, 0, 0, 1], sym([(3, 1, 20), (3, 0, 17), (1, 0, 30), (2, 0, 16)]), [bad_of(3)], what="a leaf with a symmetric graph"))
    F.append(make("origin", 3, [-1, 0, 1], sym([(0, 1, 20), (1, 2, 20)]), [bad_of(0)], what="the origin: nothing happens"))
    F.append(make("not_erase", 3, [-1, 0, 1], sym([(0, 1, 20), (1, 2, 20)]), [bad_of(1)], not_erase=[1], what="mbNotErase: mbToBeErased only"))
    F.append(make("no_parent", 3, [-1, 0, -1], sym([(0, 2, 20), (1, 2, 20)]), [bad_of(2)], what="no parent and not the origin: skipped whole"))
    # 2's row holds 1, 1's row lacks 2: 2 is left alone with its stale entry.  1's row holds 3, 3's row lacks 1: 3 stays byte for byte
    cw = sym([(0, 1, 20)])
    cw.setdefault(2, {})[1] = 18
    cw[1][3] = 19
    cw.setdefault(3, {})[0] = 16
    F.append(make("asymmetric", 4, [-1, 0, 0, 0], cw, [bad_of(1)], what="both asymmetric links"))
    # 2's ord row is what UpdateConnections left: the entries >= 15 only.  Losing 1 lists its whole cw row, 3 (weight 4) included
    F.append(make("thresholded", 4, [-1, 0, 0, 0], sym([(2, 1, 20), (2, 0, 16), (2, 3, 4), (1, 0, 25)]), [bad_of(1)], ords={2: [(1, 20), (0, 16)]},
                  what="a thresholded ord row grows to the whole row"))
    F.append(make("equal_weights", 5, [-1, 0, 0, 0, 0], sym([(1, 2, 20), (2, 0, 16), (2, 3, 16), (2, 4, 16), (1, 0, 21)]), [bad_of(1)],
                  what="equal weights in a neighbour's row: descending slot"))
    F.append(make("row_cap", 10, [-1] + [0] * 9, sym([(1, j, 10 + j) for j in range(2, 10)] + [(2, j, 30 + j) for j in range(3, 10)] + [(1, 0, 9)]), [bad_of(2)], row_cap=9,
                  what="a neighbour's row at row_cap"))
    F.append(make("one_to_zero", 3, [-1, 0, 0], sym([(1, 2, 20)]), [bad_of(2)], what="a row going from one entry to none: kf_best all -1"))
    F.append(make("child_to_parent", 4, [-1, 0, 1, 0], sym([(1, 0, 30), (2, 1, 25), (2, 0, 18)]), [bad_of(1)], what="one child linked to the parent"))
    # 3 reaches only its sibling 2, which becomes a candidate in round one
    F.append(make("via_sibling", 5, [-1, 0, 1, 1, 0], sym([(1, 0, 30), (2, 0, 18), (3, 2, 22), (2, 1, 20), (3, 1, 20)]), [bad_of(1)],
                  what="a child that reaches a candidate only through a sibling: the candidates grow"))
    F.append(make("equal_children", 5, [-1, 0, 1, 1, 0], sym([(1, 0, 30), (2, 0, 18), (3, 0, 18), (2, 3, 40)]), [bad_of(1)],
                  what="two children with equal best weight: the first in row order wins the round"))
    # 4's row lists the candidates 0 and 2 with equal weight, 0 first in ord order (an ord row the caller left in that order)
    F.append(make("equal_candidates", 5, [-1, 0, 1, 0, 1], sym([(1, 0, 30), (2, 0, 50), (4, 0, 18), (4, 2, 18)]), [bad_of(1)], ords={4: [(0, 18), (2, 18)]},
                  what="two candidates with equal weight in one child's row: the first in ord order wins"))
    # ord_w says 2 is nearer to 0 than 3 is; cw says the opposite
    # and who is picked first decides who ends under whom: by cw 3 goes to 0 and 2 to 3, by ord_w 2 would go to 0 and 3 to 2
    F.append(make("ord_w_disagrees", 4, [-1, 0, 1, 1], sym([(1, 0, 30), (2, 0, 15), (3, 0, 25), (2, 3, 40)]), [bad_of(1)],
                  ords={2: [(0, 99), (3, 40)], 3: [(0, 1), (2, 40)]}, what="ord_w disagreeing with cw_w: cw wins"))
    F.append(make("ord_not_in_cw", 4, [-1, 0, 1, 0], sym([(1, 0, 30), (2, 3, 17)]), [bad_of(1)], ords={2: [(0, 33), (3, 17)]},
                  what="an ord entry absent from cw: weight 0, still picked over -1"))
    F.append(make("bad_child", 4, [-1, 0, 1, 1], sym([(1, 0, 30), (2, 0, 40), (3, 0, 20)]), [bad_of(1)], bad=[2], what="a bad child: skipped, then falls back to the parent"))
    F.append(make("unlinked_child", 4, [-1, 0, 1, 0], sym([(1, 0, 30), (2, 3, 17)]), [bad_of(1)], what="an unlinked child falls back and STAYS in k's row"))
    for n in (0, 1, 63, 64, 65):
        F.append(star(n, "children_%d" % n))
    return F


def lists():
    base = dict(n_kf=6, parent=[-1, 0, 1, 2, 1, 0], cw=sym([(0, 1, 30), (1, 2, 28), (2, 3, 26), (1, 4, 24), (0, 5, 22), (2, 0, 17), (3, 1, 16), (4, 0, 15), (3, 4, 19)]))
    F = [make("then_child", ops=[bad_of(1), bad_of(2)], what="the second keyframe is a child of the first", **base),
         make("then_parent", ops=[bad_of(2), bad_of(1)], what="the second keyframe is the parent of the first", **base),
         make("then_neighbour", ops=[bad_of(3), bad_of(4)], what="the second keyframe is a neighbour of the first", **base),
         make("twice", ops=[bad_of(2), bad_of(2)], what="the same keyframe twice: the walk runs again over what its rows then hold", **base),
         make("parent_before", ops=[(SET_PARENT, 3, 5), bad_of(3)], what="SET_PARENT before the SET_BAD that names it", **base),
         make("parent_after", ops=[bad_of(3), (SET_PARENT, 3, 5)], what="SET_PARENT after the SET_BAD that names it", **base),
         make("parent_present", ops=[(SET_PARENT, 2, 1), (SET_PARENT, 4, 0), (SET_PARENT, 4, 0)], what="SET_PARENT of a child already present; an insert in the middle", **base),
         make("parent_heals", ops=[bad_of(2), (SET_PARENT, 2, 0), bad_of(2)], n_kf=3, parent=[-1, 0, -1], cw=sym([(0, 2, 20), (1, 2, 20)]),
              what="NO_PARENT, then a parent, then the walk: emission depends on the tree as the list left it"),
         make("empty", ops=[], what="an empty list: the children table comes out as it went in", **base)]
    return F


def emission():
    base = dict(n_kf=3, parent=[-1, 0, 1], cw=sym([(0, 1, 20), (1, 2, 20)]))
    return [make("nulls", ops=[bad_of(2), bad_of(1)], kf_mp={1: [-1, 4, -1, -1, 2], 2: [3, -1, 1]}, what="a row with -1 entries; two ops in list order", **base),
            make("held_twice", ops=[bad_of(1)], kf_mp={1: [5, 2, 5]}, what="a point held twice: two edits", **base),
            make("all_null", ops=[bad_of(1), bad_of(2)], kf_mp={1: [-1, -1, -1], 2: []}, what="an all-null row and an empty one", **base),
            make("long_row", ops=[bad_of(1)], kf_mp={1: [p if p % 3 else -1 for p in range(150)]}, what="a row above two wavefronts: the ballot's offsets", **base)]


def sizes():
    return [make("n_kf_1", 1, [-1], {}, [bad_of(0)], what="one keyframe"),
            chain(64, "n_kf_64", [bad_of(63), bad_of(31)]), chain(65, "n_kf_65", [bad_of(64), bad_of(1)]), chain(257, "n_kf_257", [bad_of(256), bad_of(128), bad_of(255)])]


@functools.lru_cache(maxsize=None)
def seeded(seed=7, n_kf=40, n_ops=12):
    """A 40-keyframe map whose graph and tree the restated UpdateConnections (tests/covis_ref.py) built, keyframe after keyframe, and a
    seeded list of about a dozen ops over it."""
    from tests import covis_ref

    rng = np.random.RandomState(seed)
    n_mp = 10 * n_kf + 120
    kfs = [covis_ref.KeyFrame(k, k) for k in range(n_kf)]     # mnId 0 is slot 0
    mps = [covis_ref.MapPoint(p, False, 0) for p in range(n_mp)]
    for k, kf in enumerate(kfs):
        seen = sorted(rng.choice(np.arange(10 * k, 10 * k + 120), 50, replace=False).tolist())
        kf.mp = [mps[p] for p in seen]
        for i, p in enumerate(seen):
            mps[p].obs[kf] = i
        kf.first_connection = True
        kf.UpdateConnections()
    row_cap = max(len(kf.cw) for kf in kfs) + 1
    cw = {kf.addr: {j.addr: w for j, w in kf.cw.items()} for kf in kfs}
    ords = {kf.addr: [(j.addr, w) for j, w in zip(kf.ord_kf, kf.ord_w)] for kf in kfs}
    parent = [kf.parent.addr if kf.parent is not None else -1 for kf in kfs]
    kf_mp = {kf.addr: [mp.slot if rng.rand() < 0.9 else -1 for mp in kf.mp] for kf in kfs}
    ops = []
    for k in rng.choice(np.arange(1, n_kf), n_ops, replace=False).tolist():
        ops.append(bad_of(k) if rng.rand() < 0.8 else (SET_PARENT, k, int((k + 1 + rng.randint(0, n_kf - 1)) % n_kf)))
    return make("seeded", n_kf, parent, cw, ops, ords=ords, kf_mp=kf_mp, row_cap=row_cap, n_mp=n_mp, not_erase=[ops[3][1]],
                what="a seeded list on a map the restated UpdateConnections built")


def fan(n_children, name):
    """Keyframe 1 under the origin with n_children children, every eighth linked to the origin: rows stay far below row_cap while the
    children row meets SLAMIT_KF_ERASE_MAX_CHILD."""
    n = 2 + n_children
    edges = [(0, 1, 30)] + [(c, 0, 20 + c % 50) for c in range(2, n, 8)]
    return make(name, n, [-1, 0] + [1] * n_children, sym(edges), [bad_of(1)], row_cap=n_children // 8 + 8, what="%d children: the ceiling of one SET_BAD" % n_children)


@functools.lru_cache(maxsize=None)
def ceiling_fixtures():
    """AT the ceilings: 1,024 children of one SET_BAD keyframe, one more (the op is skipped whole), and 1,024 ops in one list (SET_PARENT
    back and forth between two parents, SET_BAD of a leaf every 64th op)."""
    ops = []
    for i in range(1024):
        c = 3 + i % 40
        ops.append(bad_of(60 + i // 64) if i % 64 == 63 else (SET_PARENT, c, 1 + (i // 40) % 2))
    edges = [(0, 1, 30), (0, 2, 28)] + [(k, 1 + k % 2, 16) for k in range(3, 80)]
    many = make("ops_1024", 80, [-1, 0, 0] + [1 + k % 2 for k in range(3, 80)], sym(edges), ops, row_cap=48, what="1,024 ops: the ceiling of a list")
    return (fan(1024, "children_1024"), fan(1025, "children_1025"), many)


@functools.lru_cache(maxsize=None)
def all_fixtures():
    return tuple(single() + lists() + emission() + sizes() + [seeded()])


def by_name(name):
    return next(fx for fx in all_fixtures() if fx["name"] == name)
