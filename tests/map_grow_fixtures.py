"""Fixtures of the map-growth tests: small maps as the tables of slamit_map_index and its column records, frame records, op lists.  Each is
the smallest shape at which the walk can go wrong; chunk_edges is larger because the kernel walks rows and runs of NEW_POINT ops in chunks
of 512 and must be met on both sides of that edge."""
import copy
import functools

import numpy as np

from tests.map_grow_ref import ASSOCIATE, NEW_KF, NEW_POINT, RECENT

BEST = 10
OP_FIELDS = ("kind", "flags", "kf", "src", "kf_id", "cand", "kf_a", "idx_a", "kf_b", "idx_b", "weight_a", "weight_b", "pos")


def op(kind, **kw):
    e = dict(kind=kind, flags=0, kf=0, src=0, kf_id=0, cand=-1, kf_a=0, idx_a=0, kf_b=-1, idx_b=0, weight_a=1, weight_b=1, pos=(0.0, 0.0, 0.0))
    assert set(kw) <= set(e)
    e.update(kw)
    return e


def base_map(n_kp, n_mp, seed, stereo=True, bad=(), observers=None):
    """A consistent map: keyframe k has n_kp[k] keypoints; point p is observed by the keyframes observers[p] (default: a random choice),
    each at a free keypoint."""
    rng = np.random.RandomState(seed)
    n_kf = len(n_kp)
    rows = [[-1] * n for n in n_kp]
    obs = [dict() for _ in range(n_mp)]
    for p in range(n_mp):
        ks = observers[p] if observers is not None else sorted(rng.permutation(n_kf)[:rng.randint(1, max(n_kf, 1) + 1)].tolist()) if n_kf else []
        for k in ks:
            free = [i for i, v in enumerate(rows[k]) if v == -1]
            if free:
                i = free[rng.randint(len(free))]
                rows[k][i], obs[p][int(k)] = p, i
    n_kfmp = sum(n_kp)
    flat = [(k, i) for p in range(n_mp) for k, i in obs[p].items()]
    ptr = np.concatenate([[0], np.cumsum(n_kp)]).astype(np.int32)
    octave = rng.randint(0, 8, n_kfmp).astype(np.uint8)
    uright = (rng.rand(n_kfmp) < 0.5) if stereo else np.zeros(n_kfmp, bool)
    t = {"n_kf": n_kf, "n_mp": n_mp, "kf_mp_ptr": ptr, "kf_mp": np.array([v for r in rows for v in r], np.int32).reshape(-1), "kf_octave": octave,
         "kf_desc": rng.randint(0, 256, (n_kfmp, 32)).astype(np.uint8), "kf_depth": np.where(uright, rng.rand(n_kfmp) * 9 + 1, -1).astype(np.float32) if stereo else None,
         "kf_bad": np.zeros(n_kf, np.uint8), "kf_parent": np.arange(-1, n_kf - 1, dtype=np.int32), "kf_to_be_erased": np.zeros(n_kf, np.uint8),
         "kf_not_erase": (rng.rand(n_kf) < 0.3).astype(np.uint8), "kf_th_depth": np.full(n_kf, 35.0, np.float32) if stereo else None,
         "kf_best": np.full((n_kf, BEST), -1, np.int32), "cw_n": rng.randint(0, 3, n_kf).astype(np.int32), "ord_n": rng.randint(0, 3, n_kf).astype(np.int32),
         "kf_child_ptr": np.minimum(np.arange(n_kf + 1), max(n_kf - 1, 0)).astype(np.int32), "kf_child": np.arange(1, max(n_kf, 1), dtype=np.int32),
         "kf_center": rng.randn(n_kf, 3).astype(np.float32), "mp_pos": rng.randn(n_mp, 3).astype(np.float32), "mp_normal": rng.randn(n_mp, 3).astype(np.float32),
         "mp_max_dist": (rng.rand(n_mp) + 2).astype(np.float32), "mp_min_dist": (rng.rand(n_mp) + 1).astype(np.float32),
         "mp_bad": np.array([1 if p in bad else 0 for p in range(n_mp)], np.uint8).reshape(-1),
         "mp_ref_kf": np.array([min(o) if o else -1 for o in obs], np.int32).reshape(-1), "mp_found": rng.randint(1, 9, n_mp).astype(np.int32),
         "mp_visible": rng.randint(9, 19, n_mp).astype(np.int32), "mp_first_kf": rng.randint(0, 5, n_mp).astype(np.int32), "mp_replaced": np.full(n_mp, -1, np.int32),
         "mp_desc": rng.randint(0, 256, (n_mp, 32)).astype(np.uint8), "obs_ptr": np.concatenate([[0], np.cumsum([len(o) for o in obs])]).astype(np.int32),
         "obs_kf": np.array([k for k, _ in flat], np.int32).reshape(-1), "obs_idx": np.array([i for _, i in flat], np.int32).reshape(-1)}
    t["obs_octave"] = np.array([octave[ptr[k] + i] for k, i in flat], np.uint8).reshape(-1)
    t["obs_weight"] = np.array([2 if uright[ptr[k] + i] else 1 for k, i in flat], np.uint8).reshape(-1)
    t["mp_nobs"] = np.array([int(t["obs_weight"][t["obs_ptr"][p]:t["obs_ptr"][p + 1]].sum()) for p in range(n_mp)], np.int32).reshape(-1)
    for k in range(1, n_kf):
        t["kf_best"][k, 0] = k - 1
    return t


def frame(frame_mp, seed, stereo=True):
    rng = np.random.RandomState(1000 + seed)
    n = len(frame_mp)
    ur = np.where(rng.rand(n) < 0.5, rng.rand(n) * 600, -1).astype(np.float32)
    return {"frame_mp": np.array(frame_mp, np.int32).reshape(-1), "octave": rng.randint(0, 8, n).astype(np.uint8), "desc": rng.randint(0, 256, (n, 32)).astype(np.uint8),
            "depth": np.where(ur >= 0, rng.rand(n) * 9 + 1, -1).astype(np.float32) if stereo else None, "uright": ur if stereo else None,
            "Tcw": np.concatenate([np.linalg.qr(rng.randn(3, 3))[0], rng.randn(3, 1) * 3], axis=1).astype(np.float32).reshape(-1), "th_depth": float(30 + seed)}


def row_frame(t, k, seed):
    """A frame record for ASSOCIATE over the existing keyframe k: n_kp entries, its own uright."""
    return frame(t["kf_mp"][t["kf_mp_ptr"][k]:t["kf_mp_ptr"][k + 1]].tolist(), seed)


def fixture(name, t, frames, ops, cand_status=(), cand_x3d=None, recent=()):
    rng = np.random.RandomState(len(name))
    x3d = rng.randn(len(cand_status), 3).astype(np.float32) if cand_x3d is None else np.array(cand_x3d, np.float32).reshape(-1, 3)
    return {"name": name, "t": t, "frames": frames, "ops": ops, "cand_status": np.array(cand_status, np.uint8).reshape(-1), "cand_x3d": x3d, "recent": list(recent)}


@functools.lru_cache(maxsize=None)
def _all():
    out = []
    # a NEW_KF into a 2-keyframe map, and one without keypoints
    t = base_map([6, 5], 7, 1)
    out.append(fixture("kf_only", t, [frame([0, -1, 3, 3, 6], 1), frame([], 2)], [op(NEW_KF, kf=2, src=0, kf_id=9), op(NEW_KF, kf=3, src=1, kf_id=10)], recent=[4, 1]))
    # the initial map: two keyframes, then pairs whose reference is the second
    t = base_map([], 0, 2, stereo=False)
    f0, f1 = frame([-1] * 9, 3, stereo=False), frame([-1] * 8, 4, stereo=False)
    pairs = [op(NEW_POINT, kf=1, kf_id=1, kf_a=0, idx_a=i + 1, kf_b=1, idx_b=7 - i, pos=(i, 0.5 * i, 2.0 + i)) for i in range(6)]
    out.append(fixture("two_new_kfs", t, [f0, f1], [op(NEW_KF, kf=0, src=0, kf_id=0), op(NEW_KF, kf=1, src=1, kf_id=1)] + pairs))
    # -1 entries, a bad point, good ones: edits in keypoint order
    t = base_map([5, 6, 4], 9, 3, bad=(2,))
    out.append(fixture("associate_plain", t, [frame([-1, 4, 2, -1, 0, 8, 7], 5)], [op(NEW_KF, kf=3, src=0, kf_id=3), op(ASSOCIATE, kf=3, src=0)], recent=[3]))
    out.append(fixture("associate_duplicate", copy.deepcopy(t), [frame([5, -1, 1, 5, 1, 5], 6)], [op(NEW_KF, kf=3, src=0, kf_id=3), op(ASSOCIATE, kf=3, src=0)]))
    # stereo points of Tracking::CreateNewKeyFrame before local mapping associates: both go to the recent list
    t = base_map([5, 6], 8, 4)
    out.append(fixture("associate_after_stereo_points", t, [frame([3, -1, -1, 6, -1, 0], 7)],
                       [op(NEW_KF, kf=2, src=0, kf_id=4), op(NEW_POINT, kf=2, kf_id=4, kf_a=2, idx_a=2, weight_a=2, pos=(1, 2, 3)),
                        op(NEW_POINT, kf=2, kf_id=4, kf_a=2, idx_a=4, weight_a=2, pos=(4, 5, 6)), op(ASSOCIATE, kf=2, src=0)]))
    # the row in the table already holds kf; two entries whose points do not observe it yet
    t = base_map([8, 11, 7], 12, 5, observers=[[0, 1], [1], [0, 2], [1, 2], [0, 1, 2], [2], [1], [0], [0, 1], [1, 2], [0, 2], [1]])
    free = [i for i in range(11) if t["kf_mp"][t["kf_mp_ptr"][1] + i] == -1]
    lack = [p for p in range(12) if 1 not in t["obs_kf"][t["obs_ptr"][p]:t["obs_ptr"][p + 1]].tolist()]
    assert len(free) >= 2 and len(lack) >= 2
    for i, p in zip(free[:2], lack[:2]):
        t["kf_mp"][t["kf_mp_ptr"][1] + i] = p
    out.append(fixture("associate_existing_observer", t, [row_frame(t, 1, 8)], [op(ASSOCIATE, kf=1, src=0)]))
    # candidate statuses 0 1 0 5 0: compact slots, the inert tail, n_new
    t = base_map([7, 7, 6], 10, 6)
    pairs = [op(NEW_POINT, flags=RECENT, kf=2, kf_id=6, kf_a=2, idx_a=i, weight_a=1 + i % 2, kf_b=i % 2, idx_b=6 - i, weight_b=2 - i % 2, cand=i) for i in range(5)]
    out.append(fixture("pairs_mixed_status", t, [], pairs, cand_status=[0, 1, 0, 5, 0], recent=[2]))
    # two accepted points at one (kf, idx): kf_mp holds the later one, both observe
    t = base_map([6, 6], 5, 7)
    out.append(fixture("same_keypoint_twice", t, [], [op(NEW_POINT, kf=1, kf_id=2, kf_a=1, idx_a=3, kf_b=0, idx_b=2, pos=(1, 1, 1)),
                                                     op(NEW_POINT, kf=1, kf_id=2, kf_a=0, idx_a=5, kf_b=1, idx_b=3, pos=(2, 2, 2)),
                                                     op(NEW_POINT, kf=0, kf_id=2, kf_a=0, idx_a=1, kf_b=0, idx_b=1, weight_b=2, pos=(3, 3, 3))]))
    # the wavefront's edges: rows of 63, 64, 65 keypoints, a run of 65 NEW_POINT ops
    t = base_map([66, 5], 10, 8)
    rng = np.random.RandomState(8)
    fr = [frame(rng.randint(-1, 10, n).tolist(), 9 + n) for n in (63, 64, 65)]
    ops = [op(NEW_KF, kf=2 + i, src=i, kf_id=20 + i) for i in range(3)] + [op(ASSOCIATE, kf=2 + i, src=i) for i in range(3)]
    ops += [op(NEW_POINT, flags=RECENT * (i % 3 != 0), kf=4, kf_id=22, kf_a=4, idx_a=i, kf_b=0 if i % 2 else -1, idx_b=i, weight_b=2, cand=i) for i in range(65)]
    out.append(fixture("wave_edges", t, fr, ops + [op(ASSOCIATE, kf=4, src=2)], cand_status=[(i * 7) % 4 % 3 for i in range(65)]))
    # a point with 65 observers: IsInKeyFrame reads its whole row
    t = base_map([2] * 66, 3, 9, observers=[list(range(65)), [65], [0, 65]])
    ops = [op(ASSOCIATE, kf=64, src=0), op(NEW_KF, kf=66, src=1, kf_id=66), op(ASSOCIATE, kf=66, src=1)]
    out.append(fixture("observers_65", t, [row_frame(t, 64, 10), frame([0, 1, 0], 11)], ops))
    # the kernel's own chunk of 512: a row of 520 keypoints, a run of 515 NEW_POINT ops, every keypoint named once or twice
    t = base_map([4, 3], 6, 10)
    fm = (np.arange(520) % 7 - 1).tolist()
    ops = [op(NEW_KF, kf=2, src=0, kf_id=2)] + [op(NEW_POINT, flags=RECENT * (i % 2), kf=2, kf_id=2, kf_a=2, idx_a=(i * 3) % 520, cand=i % 11, weight_a=1 + i % 2) for i in range(515)]
    out.append(fixture("chunk_edges", t, [frame(fm, 12)], ops + [op(ASSOCIATE, kf=2, src=0)], cand_status=[0, 0, 3, 0, 0, 0, 8, 0, 0, 1, 0]))
    return out


def all_fixtures():
    return [copy.deepcopy(fx) for fx in _all()]


def by_name(name):
    return next(copy.deepcopy(fx) for fx in _all() if fx["name"] == name)


def ceiling_fixtures(max_ops=65536, max_frames=16):
    """SLAMIT_GROW_MAX_OPS ops in one list; with the second map SLAMIT_GROW_MAX_FRAMES frame records in one call."""
    fm = (np.arange(600) % 5 - 1).tolist()
    pts = [op(NEW_POINT, flags=RECENT * (i % 3 == 0), kf=2, kf_id=2, kf_a=2, idx_a=(i * 7) % 600, kf_b=0 if i % 4 == 0 else -1, idx_b=i % 3, weight_b=2, cand=i % 13)
           for i in range(max_ops - 2)]
    big = fixture("max_ops", base_map([4, 3], 6, 20), [frame(fm, 20)], [op(NEW_KF, kf=2, src=0, kf_id=2)] + pts + [op(ASSOCIATE, kf=2, src=0)],
                  cand_status=[0, 2, 0, 0, 1, 0, 0, 0, 7, 0, 0, 0, 0])
    many = fixture("max_frames", base_map([3, 3], 4, 21), [frame([i % 4, -1, (i + 1) % 4], 30 + i) for i in range(max_frames - 1)],
                   [op(NEW_KF, kf=2 + i, src=i, kf_id=2 + i) for i in range(max_frames - 1)] + [op(ASSOCIATE, kf=2 + i, src=i) for i in (0, 7, 14)])
    return [big, many]


def bad_fixtures():
    """Every id outside its table, in an op, a row and a source: skipped, never dereferenced (the resident form and csrc/map_grow.h's host
    statement; a host form would refuse them)."""
    base = by_name("associate_plain")
    a = copy.deepcopy(base)
    a["name"] = "wrong_slot"          # the NEW_KF does not name the next free slot; what follows meets a keyframe that does not exist
    a["ops"] = [op(NEW_KF, kf=4, src=0, kf_id=3), op(ASSOCIATE, kf=3, src=0), op(NEW_KF, kf=3, src=0, kf_id=3), op(NEW_KF, kf=3, src=0, kf_id=3), op(ASSOCIATE, kf=3, src=0)]
    b = copy.deepcopy(base)
    b["name"] = "bad_slots"
    b["frames"][0]["frame_mp"][1] = 50                                  # a source entry outside the points
    b["frames"][0]["frame_mp"][4] = -2
    b["t"]["kf_mp"][b["t"]["kf_mp_ptr"][1] + 2] = 1 << 20             # a row entry outside the points
    b["frames"].append(row_frame(b["t"], 1, 13))
    pt = lambda **kw: op(NEW_POINT, **dict(dict(kf=1, kf_id=1, kf_a=1, idx_a=0, pos=(1, 1, 1)), **kw))
    b["ops"] = [op(NEW_KF, kf=3, src=2, kf_id=3), op(NEW_KF, kf=3, src=-1, kf_id=3), op(7, kf=1), op(0), op(ASSOCIATE, kf=1, src=1), op(ASSOCIATE, kf=4, src=0),
                op(ASSOCIATE, kf=-1, src=0), op(ASSOCIATE, kf=1, src=0), op(ASSOCIATE, kf=1, src=5), pt(kf=3), pt(kf=-1), pt(kf_a=3), pt(idx_a=6), pt(idx_a=-1), pt(weight_a=0),
                pt(weight_a=3), pt(kf_b=-2), pt(kf_b=3), pt(kf_b=0, idx_b=5), pt(kf_b=0, idx_b=4, weight_b=0), pt(cand=1000), pt(cand=-2), pt(cand=1), pt(cand=0),
                op(NEW_KF, kf=3, src=0, kf_id=3), op(ASSOCIATE, kf=3, src=0)]
    b["cand_status"], b["cand_x3d"] = np.array([0, 4], np.uint8), np.arange(6, dtype=np.float32).reshape(2, 3)
    return [a, b]
