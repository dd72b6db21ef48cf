"""Inputs of tests/test_gpu_ceilings.py: every C-ABI capacity of include/slamit.h exercised AT its documented ceiling.

Everything here is built on the CPU from seeds; tests/test_ceiling_fixtures.py asserts, without a GPU, the conditions the seeds were
chosen for (no pose / Sim3 edge on its chi-square gate, admissible RANSAC problems, every status code present).  Nothing in this file
has seen a device result."""
import functools

import numpy as np

from tests import sim3_ransac_ref as rref

# ---- pose / Sim3 optimisation -----------------------------------------------------------------------------------------------------
POSE_MAX_N = SIM3_MAX_N = 65536
GATE_BAND = 1e-6          # the bars compare outlier / inlier flags exactly: no edge of the oracle's run may come this close to its gate
POSE_CEILING = dict(n=POSE_MAX_N, outlier_frac=0.15, seed=7, perturb=0.02)
SIM3_CEILING = dict(n=SIM3_MAX_N, outlier_frac=0.15, seed=0, perturb=0.03)
POSE_BATCH = ((9, 0.0, 61, 0.02), (1000, 0.25, 100, 0.04))      # the small frames beside the ceiling one: synth_pose arguments
SIM3_BATCH = ((9, 0.0, 4, 0.03), (1000, 0.15, 101, 0.03))       # synth_sim3 arguments


@functools.lru_cache(maxsize=None)
def pose_ceiling():
    from weiner_slamit_v2_amd import synth

    return synth.synth_pose(**POSE_CEILING)


@functools.lru_cache(maxsize=None)
def sim3_ceiling():
    from weiner_slamit_v2_amd import synth

    return synth.synth_sim3(**SIM3_CEILING)


def pose_head(pr, n):
    return dict(pr, xw=pr["xw"][:n].copy(), uv=pr["uv"][:n].copy(), inv_sigma2=pr["inv_sigma2"][:n].copy())


def sim3_head(pr, n):
    out = dict(pr, n=n)
    for k in ("p1", "p2", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2"):
        out[k] = pr[k][:n].copy()
    return out


def pose_batch():
    """[ceiling, 9, 0, 1000] correspondences: the LDS size of the largest frame serves the small ones."""
    from weiner_slamit_v2_amd import synth

    small, mid = (synth.synth_pose(*a) for a in POSE_BATCH)
    return [pose_ceiling(), small, pose_head(small, 0), mid]


def sim3_batch():
    from weiner_slamit_v2_amd import synth

    small, mid = (synth.synth_sim3(*a) for a in SIM3_BATCH)
    return [sim3_ceiling(), small, sim3_head(small, 0), mid]


@functools.lru_cache(maxsize=None)
def pose_oracle(which):
    """The CPU oracle's result, with its per-edge gate margins, on the ceiling problem (which = "ceiling") -- computed once."""
    from oracle import bindings as ob

    assert which == "ceiling"
    return ob.pose_solve_margin(pose_ceiling())


@functools.lru_cache(maxsize=None)
def sim3_oracle(which):
    from oracle import bindings as ob

    assert which == "ceiling"
    return ob.sim3_solve_margin(sim3_ceiling())


# ---- Sim3 RANSAC ------------------------------------------------------------------------------------------------------------------
RANSAC_MAX_N, RANSAC_MAX_HYP = 8192, 1024
# name -> (n, outlier_frac, fix_scale, n_hyp, seed, distinct): the layout of tests/sim3_ransac_ref.FIXTURES plus "every triple distinct".
# Seeds chosen on the CPU (the first of 300.., 310.., 320.. that tests/sim3_ransac_ref.admissible() accepts).
RANSAC = {
    "n8192": (RANSAC_MAX_N, 0.3, False, 8, 300, True),
    "n8152": (RANSAC_MAX_N - 40, 0.3, True, 8, 311, True),     # n % 64 = 24: the last ballot half-filled, the last 32-bit word too
    "hyp1024": (64, 0.2, False, RANSAC_MAX_HYP, 320, True),
}


def distinct_triples(n, count, seed):
    """count different triples of three different indices below n (as sets), in a seeded random order."""
    rs = np.random.RandomState(78000 + seed)
    seen, out = set(), []
    while len(out) < count:
        t = tuple(int(v) for v in rs.choice(n, 3, replace=False))
        if frozenset(t) not in seen:
            seen.add(frozenset(t))
            out.append(t)
    return np.array(out, np.int32)


@functools.lru_cache(maxsize=None)
def ransac(name):
    """(problem, admissibility) of one RANSAC ceiling fixture, as tests/sim3_ransac_ref.fixture / admissibility build them."""
    from weiner_slamit_v2_amd import synth

    n, of, fix, nh, seed, _ = RANSAC[name]
    pr = synth.synth_sim3_ransac(n, of, seed, rref.NOISE_PX, fix)
    pr["triples"] = distinct_triples(n, nh, seed)
    pr["min_inliers"] = rref.min_inliers(n, of)
    pr["max_its"] = rref.ransac_iterations(n, 0.99, pr["min_inliers"], nh)
    pr["seed"] = seed
    return pr, rref.admissibility(pr)


# ---- triangulation and frustum ------------------------------------------------------------------------------------------------------
TRIANGULATE_MAX_N, FRUSTUM_MAX_N = 8192, 65536
# tests/triangulate_ref.FIXTURES 8 (codes 3 and 8 among the usual ones) and 9 (forward motion: code 4) drawn at the ceiling; a tiny
# share of far points supplies code 1.  synth.synth_triangulation arguments.
TRIANGULATE = (
    (TRIANGULATE_MAX_N, 8, 0.4, 0.1, 0.5, {"behind_frac": 0.25, "octave_jump_frac": 0.25, "depth": (1.5, 60.0)}),
    (TRIANGULATE_MAX_N, 9, 2.5, 0.1, 0.5, {"direction": (0.05, 0.02, 1.0), "depth": (1.2, 9.0)}),
)
FRUSTUM = (0, FRUSTUM_MAX_N, 1.0)     # tests/frustum_ref.FIXTURES[MIXED]'s seed and th at the ceiling: synth.synth_frustum arguments
FRUSTUM_SMALL = 17                    # points of the second frame of the device form


@functools.lru_cache(maxsize=None)
def triangulate_problem(k):
    from weiner_slamit_v2_amd import synth

    n, seed, baseline, outl, noise, opts = TRIANGULATE[k]
    return synth.synth_triangulation(n, seed, baseline, outl, noise, **opts)


@functools.lru_cache(maxsize=None)
def frustum_problem():
    from weiner_slamit_v2_amd import synth

    return synth.synth_frustum(*FRUSTUM)


# ---- BoW search: a group of exactly SLAMIT_BOW_MAX_GROUP candidates -------------------------------------------------------------------
BOW_MAX_GROUP = 2048


def _flip(row, bits):
    out = row.copy()
    for b in bits:
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def bow_full_group(mode, tie, seed=1):
    """synth.synth_bow with every side-2 feature in ONE node (2048 candidates, ~100 queries), a second, small group behind it, and
    three planted features: query s; candidate `last` at list position 2047, s's best by far (2 bits away, on s's epipolar line);
    with tie, candidate `first` at list position 0, a copy of `last`; and a later query s2 with s's descriptor.
    Mode 0 with a ratio test that lets a tie through: s takes `first` (first one wins), s2 finds it taken and takes `last`; without the
    tie s takes `last`.  Mode 1: the last of equal candidates wins, `last` either way.
    -> (side1, side2, groups, epi, dict(s, s2, first, last))"""
    from weiner_slamit_v2_amd import synth

    assert seed % 3 != 0                                          # (seed % 3 == 0 is synth_bow's degenerate F12 = 0)
    s1, s2, g, epi = synth.synth_bow(300, BOW_MAX_GROUP, 3, seed, mode=mode, big_group=BOW_MAX_GROUP)
    assert len(g["q_ptr"]) == 2 and g["c_ptr"][1] == BOW_MAX_GROUP
    e1, e2, eg, _ = synth.synth_bow(60, 80, 1, seed + 1, mode=mode)   # the second group: 60 queries, 80 candidates, one node
    assert len(eg["q_ptr"]) == 2
    q_idx = g["q_idx"].copy()
    v1 = s1["valid"].copy()
    d1, d2 = s1["desc"].copy(), s2["desc"].copy()
    # candidate i is a noisy copy of side-1 feature src[i] (and, in mode 1, its image): the nearest side-1 descriptor
    pop = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(1).astype(np.int32)
    src = np.array([pop[d1 ^ d2[i]].sum(1).argmin() for i in range(BOW_MAX_GROUP)])
    in_group = set(q_idx.tolist())
    last = None
    for i in range(2, BOW_MAX_GROUP):                             # (rows 0 and 1 are synth_bow's own duplicates)
        s = int(src[i])
        if s not in in_group or s == int(q_idx[-1]):
            continue
        if mode == 1:
            xy1, xy2 = s1["kp_xy"][s], s2["kp_xy"][i]
            if abs(float(xy2[1] - xy1[1])) > 0.3 or np.hypot(xy2[0] - epi["ex"], xy2[1] - epi["ey"]) < 150:
                continue
        last = i
        break
    assert last is not None
    later = [int(v) for v in q_idx if v > s]
    s_2 = later[0]
    first = 2 if last != 2 else 3
    v1[s] = v1[s_2] = 1
    d2[last] = _flip(d1[s], (3, 77))
    d1[s_2] = d1[s]
    side2 = dict(s2, desc=d2)
    if side2.get("valid") is not None:
        side2["valid"] = side2["valid"].copy()
        side2["valid"][[first, last]] = 1
    if tie:
        d2[first] = d2[last]
        if mode == 1:
            side2["kp_xy"], side2["kp_octave"] = s2["kp_xy"].copy(), s2["kp_octave"].copy()
            side2["kp_xy"][first], side2["kp_octave"][first] = s2["kp_xy"][last], s2["kp_octave"][last]
    # candidate order: `first` at position 0, `last` at position 2047, the rest as they were
    rest = [i for i in range(BOW_MAX_GROUP) if i not in (first, last)]
    c_idx = np.array([first] + rest + [last], np.int32)
    # append the second group's features behind both sides
    n1, n2 = 300, BOW_MAX_GROUP
    side1 = dict(s1, desc=np.concatenate([d1, e1["desc"]]), valid=np.concatenate([v1, e1["valid"]]))
    side2["desc"] = np.concatenate([side2["desc"], e2["desc"]])
    if side2.get("valid") is not None:
        side2["valid"] = np.concatenate([side2["valid"], e2["valid"] if e2.get("valid") is not None else np.ones(80, np.uint8)])
    if mode == 1:
        side1["kp_xy"] = np.concatenate([s1["kp_xy"], e1["kp_xy"]])
        side2["kp_xy"] = np.concatenate([side2["kp_xy"], e2["kp_xy"]])
        side2["kp_octave"] = np.concatenate([side2["kp_octave"], e2["kp_octave"]])
    groups = dict(q_ptr=np.array([0, len(q_idx), len(q_idx) + 60], np.int32), q_idx=np.concatenate([q_idx, n1 + eg["q_idx"]]).astype(np.int32),
                  c_ptr=np.array([0, n2, n2 + 80], np.int32), c_idx=np.concatenate([c_idx, n2 + eg["c_idx"]]).astype(np.int32))
    return side1, side2, groups, epi, dict(s=s, s2=s_2, first=first, last=last)


# ---- keyframe database --------------------------------------------------------------------------------------------------------------
KFDB_CAPS = (4095, 4096, 8191)        # 12 cap + 8 bytes of LDS: 49,148 and 49,160 on the two sides of 48 KiB, 98,300 at the ceiling
KFDB_POOL, KFDB_MAX_WORDS, KFDB_SLOTS = 20000, 8191, 24


@functools.lru_cache(maxsize=None)
def kfdb_query(cap):
    from tests import kfdb_ref as ref

    return ref.bow(KFDB_POOL, cap, 6000 + cap)


@functools.lru_cache(maxsize=None)
def kfdb_keyframes():
    """24 slots over one pool: lengths from empty to max_words = 8191 (as long as the longest query), a copy of each query, and per
    query a keyframe that shares only its last word and one that shares only its first."""
    from tests import kfdb_ref as ref

    lengths = (0, 1, 64, 700, 4095, 4096, 8191, 8190, 2500)
    kfs = [ref.KeyFrame(i, ref.bow(KFDB_POOL, n, 700 + i)) for i, n in enumerate(lengths)]
    for cap in KFDB_CAPS:
        q = kfdb_query(cap)
        others = np.setdiff1d(np.arange(KFDB_POOL, dtype=np.int32), q[0])
        low = others[others < q[0][-1]][:99]
        high = others[others > q[0][0]][:70]
        kfs.append(ref.KeyFrame(len(kfs), (q[0].copy(), q[1].copy())))
        kfs.append(ref.KeyFrame(len(kfs), (np.concatenate([low, q[0][-1:]]).astype(np.int32), np.full(100, 0.01))))
        kfs.append(ref.KeyFrame(len(kfs), (np.concatenate([q[0][:1], high]).astype(np.int32), np.full(71, 1 / 71))))
    assert len(kfs) <= KFDB_SLOTS
    return kfs + [None] * (KFDB_SLOTS - len(kfs))


@functools.lru_cache(maxsize=None)
def kfdb_reference(cap):
    from tests import kfdb_ref as ref

    return ref.dense(kfdb_keyframes(), kfdb_query(cap))
