"""Maps for the map-point upkeep tests: the smallest shapes at which the update and culling passes can go wrong.  A map is t (the tables
of slamit_map_index) and x (the columns of slamit_point_index); up_map() names one point per case, cull_map() one list per length.
Built once from fixed seeds; do not modify what they return."""
import functools

import numpy as np

N_LEVELS = 8
SCALE = (np.float32(1.2) ** np.arange(N_LEVELS)).astype(np.float32)
MAX_OBS, MAX_DESC = 512, 128
FIRST_BAD_KF = 200                 # up_map: keyframes from this slot on are bad
N_KF, EMPTY_KF = 641, 640          # up_map: slot 640 has no keypoints
CUR_ID = 10


def build_map(n_kf, points, rng, bad_kf=(), empty_kf=(), n_levels=N_LEVELS, octave_of=None, desc_of=None):
    """points: list of dict(obs=[slots in STORED order], ref=slot, bad=0/1, pos=(3,) or None).  Every keyframe but the empty ones starts
    with one keypoint without a point, so keypoint 0 is never an observation; an observation's index is the next free one of its keyframe.
    octave_of / desc_of: {(point, keyframe): value} overrides."""
    rows = [[] if k in empty_kf else [-1] for k in range(n_kf)]
    obs_ptr, obs_kf, obs_idx = [0], [], []
    for p, spec in enumerate(points):
        for k in spec["obs"]:
            obs_kf.append(k); obs_idx.append(len(rows[k])); rows[k].append(p)
        obs_ptr.append(len(obs_kf))
    kf_mp_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    kf_mp = np.array([p for r in rows for p in r], np.int32)
    n_mp, n_kp = len(points), len(kf_mp)
    kf_octave = rng.integers(0, n_levels, n_kp).astype(np.uint8)
    kf_desc = rng.integers(0, 256, (n_kp, 32)).astype(np.uint8)
    obs_kf, obs_idx = np.array(obs_kf, np.int32), np.array(obs_idx, np.int32)
    at = {}
    for p in range(n_mp):
        for o in range(obs_ptr[p], obs_ptr[p + 1]):
            at[(p, int(obs_kf[o]))] = kf_mp_ptr[obs_kf[o]] + obs_idx[o]
    for key, v in (octave_of or {}).items():
        kf_octave[at[key]] = v
    for key, v in (desc_of or {}).items():
        kf_desc[at[key]] = v
    kf_bad = np.zeros(n_kf, np.uint8)
    kf_bad[list(bad_kf)] = 1
    pos = rng.uniform(-5, 5, (n_mp, 3)).astype(np.float32)
    for p, spec in enumerate(points):
        if spec.get("pos") is not None:
            pos[p] = spec["pos"]
    t = {"n_kf": n_kf, "n_mp": n_mp, "obs_ptr": np.array(obs_ptr, np.int32), "obs_kf": obs_kf,
         "mp_bad": np.array([s.get("bad", 0) for s in points], np.uint8), "kf_bad": kf_bad, "kf_mp_ptr": kf_mp_ptr, "kf_mp": kf_mp,
         "kf_best": np.full((n_kf, 10), -1, np.int32), "kf_child_ptr": np.zeros(n_kf + 1, np.int32), "kf_child": np.zeros(0, np.int32),
         "kf_parent": np.full(n_kf, -1, np.int32), "mp_pos": pos,
         # what the planes hold before the call: nothing a pass could produce by accident
         "mp_normal": rng.uniform(2, 3, (n_mp, 3)).astype(np.float32), "mp_max_dist": rng.uniform(100, 200, n_mp).astype(np.float32),
         "mp_min_dist": rng.uniform(-2, -1, n_mp).astype(np.float32)}
    x = {"n_levels": n_levels, "scale_factors": np.concatenate([SCALE, np.zeros(16 - len(SCALE), np.float32)])[:16].copy(),
         "obs_idx": obs_idx, "obs_octave": kf_octave[kf_mp_ptr[obs_kf] + obs_idx] if len(obs_kf) else np.zeros(0, np.uint8), "kf_octave": kf_octave,
         "kf_center": rng.uniform(-20, 20, (n_kf, 3)).astype(np.float32), "kf_desc": kf_desc,
         "mp_ref_kf": np.array([s["ref"] for s in points], np.int32), "mp_nobs": np.array([len(s["obs"]) for s in points], np.int32),
         "mp_found": np.ones(n_mp, np.int32), "mp_visible": np.ones(n_mp, np.int32), "mp_first_kf": np.zeros(n_mp, np.int32),
         "mp_normal": t["mp_normal"], "mp_max_dist": t["mp_max_dist"], "mp_min_dist": t["mp_min_dist"],
         "mp_desc": rng.integers(0, 256, (n_mp, 32)).astype(np.uint8)}
    return t, x


def flipped(base, bits):
    d = np.unpackbits(np.array(base, np.uint8))
    d[list(bits)] ^= 1
    return np.packbits(d)


@functools.lru_cache(maxsize=None)
def up_map():
    """-> dict(t, x, cases {name: point slot}, lists {name: slots to list}).  Keyframes 200.. are bad, 640 has no keypoints."""
    rng = np.random.default_rng(2501)
    cases, points, octave_of, desc_of = {}, [], {}, {}

    def add(name, obs, ref=None, **kw):
        cases[name] = len(points)
        points.append(dict(obs=list(obs), ref=(obs[0] if ref is None else ref), **kw))
        return cases[name]

    add("n1", [5])
    add("n2_descending", [7, 3], ref=7)                                        # N = 2 always ties: the lower slot's row wins
    for n in (63, 64, 65, 128, 129):                                            # 129 good observers: DESC_OVERFLOW, the normal still updated
        add("n%d" % n, rng.permutation(n).tolist() if n != 64 else list(range(63, -1, -1)))
    add("ceiling_many_good", rng.permutation(MAX_OBS).tolist())                 # 512 observers, 200 good
    add("ceiling", (128 + rng.permutation(MAX_OBS)).tolist(), ref=130)          # 512 observers, 72 good: both parts run
    add("above_ceiling", rng.permutation(MAX_OBS + 1).tolist())                 # OBS_OVERFLOW
    add("shuffled", [40, 12, 33, 2, 19, 27, 8], ref=19)
    add("bad_observer", [1, 2, 250, 4], ref=250)                                # counts in n, absent from the descriptor rows
    add("all_observers_bad", [300, 301, 205])
    add("bad_point", [1, 2, 3], bad=1)
    add("no_observations", [], ref=3)
    add("ref_not_observer", [1, 2, 3], ref=9)
    add("ref_none", [4, 6], ref=-1)
    add("ref_without_keypoints", [4, 6], ref=EMPTY_KF)
    p = add("octave_n_levels", [11, 12], ref=11)
    octave_of[(p, 11)] = N_LEVELS
    p = add("tie3", [9, 2, 5], ref=9)                                          # d(a,b) = d(a,c) = 10, d(b,c) = 20: every median is 10
    a = rng.integers(0, 256, 32).astype(np.uint8)
    desc_of.update({(p, 2): a, (p, 5): flipped(a, range(10)), (p, 9): flipped(a, range(100, 110))})
    # a negative component whose product with 1 / norm underflows to -0: 0.0f + (-0) is +0
    add("minus_zero", [6], pos=(np.float32(-1e-45), np.float32(1000), np.float32(0)))
    add("n3_odd", [15, 14, 16], ref=14)
    t, x = build_map(N_KF, points, rng, bad_kf=range(FIRST_BAD_KF, N_KF), empty_kf=(EMPTY_KF,), octave_of=octave_of, desc_of=desc_of)
    x["kf_center"][6] = 0                                                       # minus_zero's only observer
    every = list(range(len(points)))
    lists = {"all": every, "twice": every + [cases["n65"], cases["shuffled"], cases["n65"]], "reversed": every[::-1], "empty": []}
    return {"t": t, "x": x, "cases": cases, "lists": lists}


@functools.lru_cache(maxsize=None)
def small_map():
    """A second, small map for the batch tests: three keyframes, four points."""
    rng = np.random.default_rng(2502)
    points = [dict(obs=[2, 0], ref=0), dict(obs=[1], ref=1), dict(obs=[0, 1, 2], ref=2, bad=1), dict(obs=[1, 2], ref=0)]
    t, x = build_map(3, points, rng, bad_kf=(2,))
    return {"t": t, "x": x, "lists": {"all": [3, 0, 1, 2]}}


def random_map(rng):
    """A small random map with every odd place at some rate."""
    n_kf, n_mp = int(rng.integers(1, 7)), int(rng.integers(1, 6))
    empty = [k for k in range(n_kf) if rng.random() < 0.1]
    full = [k for k in range(n_kf) if k not in empty]
    points, octave_of = [], {}
    for p in range(n_mp):
        obs = rng.permutation(full)[:rng.integers(0, len(full) + 1)].tolist() if full else []
        ref = int(rng.integers(-1, n_kf)) if rng.random() < 0.3 or not obs else int(rng.choice(obs))
        points.append(dict(obs=obs, ref=ref, bad=int(rng.random() < 0.1)))
        for k in obs:
            if rng.random() < 0.05:
                octave_of[(p, k)] = N_LEVELS
    t, x = build_map(n_kf, points, rng, bad_kf=[k for k in range(n_kf) if rng.random() < 0.25], empty_kf=empty, octave_of=octave_of)
    if len(x["kf_desc"]) and rng.random() < 0.3:                                # near-duplicate descriptors: ties among the medians
        x["kf_desc"][:] = x["kf_desc"][0]
        x["kf_desc"][rng.random(len(x["kf_desc"])) < 0.5, 0] ^= 1
    x["mp_found"], x["mp_visible"] = rng.integers(0, 5, n_mp).astype(np.int32), rng.integers(0, 9, n_mp).astype(np.int32)
    x["mp_first_kf"], x["mp_nobs"] = rng.integers(6, 12, n_mp).astype(np.int32), rng.integers(1, 6, n_mp).astype(np.int32)
    return {"t": t, "x": x, "points": rng.integers(0, n_mp, rng.integers(0, 8)).tolist(), "what": int(rng.integers(1, 4)),
            "recent": rng.permutation(n_mp)[:rng.integers(0, n_mp + 1)].tolist(), "monocular": bool(rng.integers(0, 2)), "cur_id": CUR_ID}


CULL_LENGTHS = (0, 1, 63, 64, 65, 1000)


@functools.lru_cache(maxsize=None)
def cull_map():
    """1,200 points without observations whose counters run through every combination the predicate looks at; lists of distinct slots.
    -> dict(t, x, lists {length: slots}, cur_id)."""
    rng = np.random.default_rng(2503)
    combos = [(bad, fv, age, nobs) for bad in (0, 0, 0, 1) for fv in ((0, 0), (3, 0), (1, 4), (1, 5), (5, 5), (2, 9)) for age in (0, 1, 2, 3, 4)
              for nobs in (1, 2, 3, 4)]
    n_mp = 1200
    pick = [combos[i % len(combos)] for i in rng.permutation(n_mp)]
    t, x = build_map(1, [dict(obs=[], ref=-1, bad=c[0]) for c in pick], rng)
    x["mp_found"], x["mp_visible"] = np.array([c[1][0] for c in pick], np.int32), np.array([c[1][1] for c in pick], np.int32)
    x["mp_first_kf"], x["mp_nobs"] = np.array([CUR_ID - c[2] for c in pick], np.int32), np.array([c[3] for c in pick], np.int32)
    lists = {n: rng.permutation(n_mp)[:n].astype(np.int32) for n in CULL_LENGTHS}
    return {"t": t, "x": x, "lists": lists, "cur_id": CUR_ID, "combos": pick}
