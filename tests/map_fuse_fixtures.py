"""The maps and op lists of the map-fuse tests, the smallest shapes that can go wrong.  A fixture is dict(name, t, x, ops, claims, events,
status): t, x and ops as tests/map_replace_fixtures.py lays them out (ops may be of all three kinds), claims {op index: the outcome the
fixture is named for}, events the names the reference walk must report, status what the call must answer.
test_the_fixtures_hold_what_they_claim (tests/test_map_fuse_ref.py) checks every claim against tests/map_fuse_ref.py, so no fixture
misses its case by an accident of its numbers."""
import functools

import numpy as np

from tests.map_edit_fixtures import build_map, free_idx, idx_of
from tests.map_fuse_ref import ADDED, FUSE, MAX_OPS, NOMATCH, OCCUPANT_BAD, P_REPLACED, Q_REPLACED, SKIP_BAD, SKIP_IN_KF
from tests.map_replace_fixtures import A, R, with_counters
from tests.map_replace_ref import OBS_OVERFLOW


def F(p, k, idx, octave=3, weight=1):
    return (FUSE, p, k, idx, octave, weight)


def fixture(name, t, x, ops, claims=None, events=(), status=0):
    return {"name": name, "t": t, "x": x, "ops": ops, "claims": claims or {}, "events": tuple(events), "status": status}


def put(t, k, idx, p):
    """kf_mp[k][idx] = p on a copy: a table that holds something its rows do not."""
    t = dict(t, kf_mp=t["kf_mp"].copy())
    t["kf_mp"][t["kf_mp_ptr"][k] + idx] = p
    return t


def outcomes():
    """Every outcome alone, over disjoint groups of points, and the tie."""
    rows = [[0, 1],                     # 0   no match
            [],                         # 1   bad
            [0, 2],                     # 2   already in keyframe 2
            [0, 1],                     # 3   added to keyframe 3, a stereo keypoint
            [0], [4],                   # 4   onto 5, which is bad but still stands in keyframe 4
            [0, 1], [3, 4, 5],          # 6   onto 7 with more observations: 6 -> 7
            [0, 1, 2], [3, 4],          # 8   onto 9 with fewer: 9 -> 8
            [0, 1], [4, 5]]             # 10  onto 11 with as many: 11 -> 10
    t, x = build_map(6, rows, bad=(1, 5), nobs={1: 2})
    t, x = with_counters(t, x, 41)
    ops = [F(0, 2, -1), F(1, 2, free_idx(t, 2)), F(2, 2, free_idx(t, 2, 1)), F(3, 3, free_idx(t, 3), 5, 2), F(4, 4, idx_of(t, x, 5, 4)), F(6, 3, idx_of(t, x, 7, 3)),
           F(8, 3, idx_of(t, x, 9, 3)), F(10, 4, idx_of(t, x, 11, 4))]
    claims = dict(enumerate((NOMATCH, SKIP_BAD, SKIP_IN_KF, ADDED, OCCUPANT_BAD, P_REPLACED, Q_REPLACED, Q_REPLACED)))
    return fixture("outcomes", t, x, ops, claims, ("fuse_tie",))


def same_point():
    """kf_mp[2][idx] names point 0, whose row lacks keyframe 2: P == Q, Replace of a point by itself."""
    t, x = with_counters(*build_map(4, [[0, 1], [3]]), seed=42)
    i = free_idx(t, 2)
    return fixture("same_point", put(t, 2, i, 0), x, [F(0, 2, i)], {0: Q_REPLACED}, ("fuse_same_point", "replace_self"))


def flipped():
    """The direction is read from mp_nobs as the earlier ops left it.  Alone, each second op would be 'P replaced'."""
    rows = [[0, 1], [2, 3, 4],          # a weight-2 add raises 0 to 4 observations, past 1's 3: 1 -> 0
            [0, 1], [2, 3, 4], [5, 6]]  # 4 -> 2 raises 2 to 4, past 3's 3: 3 -> 2
    t, x = with_counters(*build_map(7, rows), seed=43)
    ops = [F(0, 5, free_idx(t, 5), 2, 2), F(0, 2, idx_of(t, x, 1, 2)), R(4, 2), F(2, 2, idx_of(t, x, 3, 2))]
    return dict(fixture("flipped", t, x, ops, {0: ADDED, 1: Q_REPLACED, 3: Q_REPLACED}), alone={1: P_REPLACED, 3: P_REPLACED})


def added_then_met():
    """The occupant exists only because an earlier op of the list added it at the same (k, idx)."""
    t, x = with_counters(*build_map(4, [[0], [1, 2]]), seed=44)
    i = free_idx(t, 3)
    return fixture("added_then_met", t, x, [F(0, 3, i, 1, 1), F(1, 3, i, 2, 2)], {0: ADDED, 1: Q_REPLACED}, ("fuse_tie",))


def rewritten():
    """The occupant is what an earlier REPLACE wrote there: its D, and -1 where the entry died."""
    rows = [[0, 1], [2], [3, 4, 5],     # 0 -> 1 writes 1 at 0's keypoint of keyframe 0; 2 meets 1 there (3 observations each: 1 -> 2)
            [0, 1], [0], [2]]           # 3 -> 4: 3's entry of keyframe 0 dies, -1; 5 is ADDED there
    t, x = with_counters(*build_map(6, rows), seed=45)
    ops = [R(0, 1), F(2, 0, idx_of(t, x, 0, 0)), R(3, 4), F(5, 0, idx_of(t, x, 3, 0), 4, 1)]
    return fixture("rewritten", t, x, ops, {1: Q_REPLACED, 3: ADDED}, ("replace_some_die", "fuse_tie"))


def turned():
    """What an earlier op did to P or to the occupant decides the exit."""
    rows = [[0, 1], [2],                # 0 -> 1, then 0 again: bad by now
            [3], [0],                   # 2 -> 3 moves keyframe 3 onto 3, then 3 into keyframe 3: in it by now
            [4], [5], [0, 1]]           # 4 -> 5 while keyframe 2 still names 4 at a free keypoint: the occupant is bad by now
    t, x = with_counters(*build_map(6, rows), seed=46)
    i = free_idx(t, 2, 2)
    ops = [R(0, 1), F(0, 5, free_idx(t, 5)), R(2, 3), F(3, 3, free_idx(t, 3)), R(4, 5), F(6, 2, i)]
    return fixture("turned", put(t, 2, i, 4), x, ops, {1: SKIP_BAD, 3: SKIP_IN_KF, 5: OCCUPANT_BAD})


def shared():
    """Points 0 and 1 both hold keyframe 4 at ONE keypoint, as Fuse leaves them; kf_mp names 0."""
    rows = [[0, 4], [1, 4], [2, 3, 5], [0]]
    t, x = with_counters(*build_map(6, rows), seed=47)
    i = idx_of(t, x, 0, 4)
    x = dict(x, obs_idx=x["obs_idx"].copy())
    x["obs_idx"][t["obs_ptr"][1] + 1] = i
    # 2 meets 0 there: 0 -> 2, the keypoint names 2.  1 -> 2: 2 holds keyframe 4, the entry dies, -1.  3 is ADDED on the dead keypoint.
    return fixture("shared", put(t, 4, i, 0), x, [F(2, 4, i), R(1, 2), F(3, 4, i, 6, 2)], {0: Q_REPLACED, 2: ADDED}, ("replace_some_die",))


def chain(depth=300, name="chain"):
    """Every op's occupant is the receiver of the op before, and the occupant changes hands: whoever stands at (keyframe 0, its keypoint)
    meets one new point per op.  Even ops bring a point with more observations than anything met so far (mp_nobs is the caller's
    column: 10,000 + 100 per op, its row one keyframe), so the occupant gives way and the keypoint is REWRITTEN to the newcomer; odd ops
    bring a point with one observation, which is swallowed.  Every op reads what the op before wrote into kf_mp."""
    n_kf = 40
    rows = [[0, 1]] + [[2 + (p * 7) % (n_kf - 2)] for p in range(depth)]    # after 38 ops entries die instead of moving
    t, x = with_counters(*build_map(n_kf, rows, spare=2, nobs={1 + j: 10000 + 100 * j for j in range(0, depth, 2)}), seed=48)
    i = idx_of(t, x, 0, 0)
    claims = {j: P_REPLACED if j % 2 else Q_REPLACED for j in (0, 1, 2, 3, depth // 2, depth // 2 + 1, depth - 2, depth - 1)}
    return fixture(name, t, x, [F(1 + j, 0, i) for j in range(depth)], claims, ("replace_all_move", "replace_some_die"))


def mixed():
    """One list of all three kinds on the same points."""
    rows = [[0, 1], [2, 3], [4], [0, 5], [1], [3, 5]]
    t, x = with_counters(*build_map(6, rows), seed=49)
    ops = [A(t, 2, 0, 0, 2, 2),                         # 2 enters keyframe 0 at a free keypoint: 3 observations
           F(0, 2, idx_of(t, x, 1, 2)),                 # 0 meets 1, a tie: 1 -> 0
           R(4, 2),                                     # 2 takes keyframe 1
           F(2, 3, idx_of(t, x, 1, 3)),                 # keyframe 3's keypoint names 0 by now, 4 observations against 2's 4: a tie, 0 -> 2
           F(3, 4, -1),
           A(t, 5, 0, 1, 1, 1),
           F(5, 4, idx_of(t, x, 2, 4))]                 # 2 holds 6 observations by now, 5 three: 5 -> 2, its keyframes 0 and 3 die, 5 moves
    return fixture("mixed", t, x, ops, {1: Q_REPLACED, 3: Q_REPLACED, 4: NOMATCH, 6: P_REPLACED}, ("replace_some_die",))


def random_fuse(name, seed, n_kf, n_mp, n_ops, density=3.0, kp_spare=8, plain=0.0, nomatch=0.3):
    """A random consistent map and a random list: FUSE ops of any point into any keypoint (occupied or free) of any keyframe, a share of
    them without a match, and a share `plain` of REPLACE and ADD_OBS ops."""
    rng = np.random.default_rng(seed)
    lens = np.minimum(rng.poisson(density, n_mp), n_kf)
    rows = [sorted(rng.choice(n_kf, int(l), replace=False).tolist(), key=lambda k: (k * 7) % 5) for l in lens]
    t, x = build_map(n_kf, rows, spare=kp_spare, weights={(p, rows[p][0]): 2 for p in range(0, n_mp, 5) if rows[p]}, bad=tuple(range(3, n_mp, 17)))
    t, x = with_counters(t, x, seed)
    width = np.diff(t["kf_mp_ptr"])
    ops = []
    hot = min(n_mp, max(3 * n_ops, 8))                                  # few enough points that ops meet each other
    for i in range(n_ops):
        a, b = (int(v) for v in rng.integers(0, hot, 2))
        if i % 2:
            a, b = n_mp - 1 - a, n_mp - 1 - b                           # the table's far end too
        k, r = int(rng.integers(0, n_kf)), rng.random()
        if r < plain / 2:
            ops.append(R(a, b))
        elif r < plain:
            ops.append(A(t, a, k, int(rng.integers(0, kp_spare)), int(rng.integers(0, 8)), int(rng.integers(1, 3))))
        else:
            idx = -1 if rng.random() < nomatch else int(rng.integers(0, width[k]))
            ops.append(F(a, k, idx, int(rng.integers(0, 8)), int(rng.integers(1, 3))))
    return fixture(name, t, x, ops)


def neighbours(name="neighbours", seed=60, n_kf=6, n_mp=14, per_kf=5):
    """SearchInNeighbors (LocalMapping.cc): the current keyframe 0's points fused into every neighbour, the targets back to back, then
    the neighbours' points into keyframe 0.  A match is an occupied keypoint, a free one, or none."""
    rng = np.random.default_rng(seed)
    rows = [sorted(rng.choice(n_kf, int(rng.integers(1, 4)), replace=False).tolist()) for _ in range(n_mp)]
    t, x = with_counters(*build_map(n_kf, rows, spare=per_kf), seed=seed)
    width = np.diff(t["kf_mp_ptr"])
    in_kf = lambda k: [p for p in range(n_mp) if k in rows[p]]
    pick = lambda k: -1 if rng.random() < 0.3 else int(rng.integers(0, width[k]))
    ops, bases = [], []
    for k in range(1, 4):
        bases.append(len(ops))
        ops += [F(p, k, pick(k), int(rng.integers(0, 8)), int(rng.integers(1, 3))) for p in in_kf(0)]
    bases.append(len(ops))
    ops += [F(p, 0, pick(0), int(rng.integers(0, 8)), 1) for p in sorted({p for k in range(1, 4) for p in in_kf(k)})]
    return dict(fixture(name, t, x, ops), bases=bases)


def row_ceiling(name, len_p, len_q, status):
    """Point 0 = P with len_p observers, point 1 = Q with len_q others and more observations: `replace` sends P's onto Q's row; with
    len_q == 0 the op adds one observer to P instead."""
    n_kf = 600
    rows = [list(range(len_p)), list(range(len_p, len_p + len_q)), [598]]
    t, x = with_counters(*build_map(n_kf, rows, spare=1), seed=50)
    if len_q:
        return fixture(name, t, x, [F(0, len_p, idx_of(t, x, 1, len_p))], {} if status else {0: P_REPLACED}, (), status)
    return fixture(name, t, x, [F(0, 599, free_idx(t, 599), 1, 1)], {} if status else {0: ADDED}, (), status)


def row_in(name, occupant):
    """A row of 513 on input: P's own, or the initial occupant's, which the op would not even touch (P is bad)."""
    rows = [list(range(513)), [598], []]
    t, x = build_map(600, rows, spare=1, bad=(2,), nobs={2: 1})
    t, x = with_counters(t, x, 51)
    ops = [F(2, 0, idx_of(t, x, 0, 0))] if occupant else [F(0, 599, -1), F(0, 598, idx_of(t, x, 1, 598))]
    return fixture(name, t, x, ops, {}, (), OBS_OVERFLOW)


@functools.lru_cache(maxsize=None)
def all_fixtures():
    fxs = [outcomes(), same_point(), flipped(), added_then_met(), rewritten(), turned(), shared(), chain(), mixed(), neighbours(),
           row_ceiling("row512_add", 511, 0, 0), row_ceiling("row513_add", 512, 0, OBS_OVERFLOW),
           row_ceiling("row512_rep", 12, 500, 0), row_ceiling("row513_rep", 13, 500, OBS_OVERFLOW), row_in("row513_in", False), row_in("row513_in_occupant", True),
           random_fuse("ops0", 61, 6, 12, 0), random_fuse("ops1", 62, 6, 255, 1, nomatch=0.0), random_fuse("ops63", 63, 6, 256, 63),
           random_fuse("ops64", 64, 6, 257, 64, plain=0.3), random_fuse("ops65", 65, 8, 40, 65, plain=0.2), random_fuse("ops1025", 66, 30, 700, 1025, plain=0.1)]
    return tuple(fxs)


@functools.lru_cache(maxsize=None)
def ceiling_fixtures():
    """Lists of MAX_OPS ops: one of ops that never meet (every op its own point, twice MAX_OPS involved points at the most) and one
    single chain MAX_OPS deep."""
    n_kf, n_mp = 32, 2 * MAX_OPS + 5
    rows = [[p % n_kf] for p in range(n_mp)]
    t, x = with_counters(*build_map(n_kf, rows, spare=MAX_OPS // 4 // n_kf + 1), seed=67)
    ops = []
    for i in range(MAX_OPS):
        p, q, u = 2 * i, 2 * i + 1, i // 4
        if i % 2 == 0:
            ops.append(F(p, q % n_kf, idx_of_row0(t, x, q)))            # onto the keypoint of a point no other op names
        elif i % 4 == 1:
            ops.append(F(p, u % n_kf, free_idx(t, u % n_kf, u // n_kf), i % 8, 1 + u % 2))   # onto a free keypoint of its own
        else:
            ops.append(F(p, u % n_kf, -1))
    return fixture("ceiling_wide", t, x, ops), chain(MAX_OPS, "ceiling_chain")


def idx_of_row0(t, x, p):
    return int(x["obs_idx"][t["obs_ptr"][p]])


def by_name(name):
    return next(fx for fx in all_fixtures() if fx["name"] == name)


@functools.lru_cache(maxsize=None)
def expected(name, cap_delta=None):
    """The restatement's result on a fixture, computed once and shared.  cap_delta: obs_cap_out = the need + cap_delta."""
    from tests.map_fuse_ref import apply

    fx = by_name(name)
    if cap_delta is None:
        return apply(fx["t"], fx["x"], fx["ops"])
    return apply(fx["t"], fx["x"], fx["ops"], expected(name)["n_obs_out"] + cap_delta)
