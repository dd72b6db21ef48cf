"""Seeded small maps and frames for the local-map tests: a chain of keyframes with overlapping point sets, the covisibility graph
and a spanning tree built from them, random bad flags; and hand-built maps for the places where the reference is odd.

A fixture is dict(maps: [tables], frames: [frame], kf_cap, q_cap); tables has the layout of slamit_map_index (api.MAP_INDEX_TABLES),
a frame is dict(map, frame_mp, frame_seen, local_kf, ref_kf): the lists as they stand before the call."""
import functools

import numpy as np

BEST = 10


def tables_from_rows(rows, n_mp, kf_bad=None, mp_bad=None, best=None, parent=None, seed=0):
    """rows[k] = keyframe k's map points by keypoint index (-1 = none).  Observations are the inverse of the rows, listed in a
    shuffled order; best / parent default to the covisibility weights (shared points, then slot) and to the strongest earlier
    keyframe; children are the inverse of the parents, ascending."""
    rng = np.random.default_rng(seed)
    K = len(rows)
    rows = [np.asarray(r, np.int32).reshape(-1) for r in rows]
    obs = [[] for _ in range(n_mp)]
    for k, r in enumerate(rows):
        for p in sorted(set(int(x) for x in r if x >= 0)):
            obs[p].append(k)
    obs = [list(rng.permutation(o)) if o else [] for o in obs]
    weight = [dict() for _ in range(K)]
    for o in obs:
        for a in o:
            for b in o:
                if a != b:
                    weight[a][b] = weight[a].get(b, 0) + 1
    kf_best = np.full((K, BEST), -1, np.int32)
    kf_parent = np.full(K, -1, np.int32)
    for k in range(K):
        order = sorted(weight[k], key=lambda b: (-weight[k][b], b))
        if best is not None and k in best:
            order = list(best[k])
        kf_best[k, :min(BEST, len(order))] = order[:BEST]
        if parent is not None:
            kf_parent[k] = parent.get(k, -1)
        elif k > 0:
            earlier = [b for b in sorted(weight[k], key=lambda b: (-weight[k][b], b)) if b < k]
            kf_parent[k] = earlier[0] if earlier else k - 1
    childs = [[] for _ in range(K)]
    for k in range(K):
        if kf_parent[k] >= 0:
            childs[kf_parent[k]].append(k)

    def csr(lists):
        ptr = np.zeros(len(lists) + 1, np.int32)
        ptr[1:] = np.cumsum([len(x) for x in lists])
        flat = np.array([v for x in lists for v in x], np.int32)
        return ptr, flat

    obs_ptr, obs_kf = csr(obs)
    kf_mp_ptr, kf_mp = csr(rows)
    kf_child_ptr, kf_child = csr(childs)
    f32 = lambda *shape: rng.uniform(-4, 4, shape).astype(np.float32)
    return {"n_kf": K, "n_mp": n_mp, "obs_ptr": obs_ptr, "obs_kf": obs_kf,
            "mp_bad": np.zeros(n_mp, np.uint8) if mp_bad is None else np.asarray(mp_bad, np.uint8),
            "kf_bad": np.zeros(K, np.uint8) if kf_bad is None else np.asarray(kf_bad, np.uint8),
            "kf_mp_ptr": kf_mp_ptr, "kf_mp": kf_mp, "kf_best": kf_best, "kf_child_ptr": kf_child_ptr, "kf_child": kf_child, "kf_parent": kf_parent,
            "mp_pos": f32(n_mp, 3), "mp_normal": f32(n_mp, 3), "mp_max_dist": rng.uniform(4, 9, n_mp).astype(np.float32),
            "mp_min_dist": rng.uniform(0.1, 2, n_mp).astype(np.float32)}


def flags(n, which):
    a = np.zeros(n, np.uint8)
    a[list(which)] = 1
    return a


def chain_map(seed, K, n_mp, kps, width, p_bad_kf=0.1, p_bad_mp=0.05):
    """K keyframes in a chain: keyframe k sees a window of `width` points that slides along the n_mp points, about 80 % of them,
    at random keypoint indices of its kps[k] (or kps) keypoints."""
    rng = np.random.default_rng(seed)
    kps = np.broadcast_to(np.asarray(kps), (K,))
    step = (n_mp - width) / max(K - 1, 1)
    rows = []
    for k in range(K):
        w = max(width, int(kps[k]) + width // 2) if kps[k] > width else width      # a long keyframe sees a wider window
        lo = min(int(k * step), max(n_mp - w, 0))
        pts = rng.permutation(np.arange(lo, min(n_mp, lo + w)))
        pts = pts[rng.random(len(pts)) < 0.8][:int(kps[k])]
        row = np.full(int(kps[k]), -1, np.int32)
        row[rng.permutation(int(kps[k]))[:len(pts)]] = pts
        rows.append(row)
    return tables_from_rows(rows, n_mp, kf_bad=rng.random(K) < p_bad_kf, mp_bad=rng.random(n_mp) < p_bad_mp, seed=seed + 1)


def chain_frame(tables, seed, n, lo, hi, n_seen=0, map_id=0, local_kf=(), ref_kf=-1):
    """A frame of n keypoints tracking about 60 % points of [lo, hi), bad ones among them as the map has them."""
    rng = np.random.default_rng(seed)
    mp = rng.integers(lo, hi, n).astype(np.int32)
    mp[rng.random(n) < 0.4] = -1
    seen = rng.integers(0, tables["n_mp"], n_seen).astype(np.int32)
    return {"map": map_id, "frame_mp": mp, "frame_seen": seen, "local_kf": np.asarray(local_kf, np.int32), "ref_kf": ref_kf}


def frame(frame_mp, local_kf=(), ref_kf=-1, frame_seen=(), map_id=0):
    return {"map": map_id, "frame_mp": np.asarray(frame_mp, np.int32), "frame_seen": np.asarray(frame_seen, np.int32),
            "local_kf": np.asarray(local_kf, np.int32), "ref_kf": ref_kf}


def one(tables, fr, kf_cap=96, q_cap=512):
    return {"maps": [tables], "frames": [fr], "kf_cap": kf_cap, "q_cap": q_cap}


NAMES = ("plain", "no_observer", "all_voted_bad", "tie", "over_80_voted", "exactly_80_voted", "parent_ends_walk", "bad_parent_pushed",
         "shared_by_five", "skip_own_point", "skip_frame_seen", "q_cap_overflow", "long_keyframe", "three_frames_two_maps", "hbm_histogram", "ceilings")


@functools.lru_cache(maxsize=None)
def fixture(name):
    if name == "plain":                  # 1
        t = chain_map(11, 12, 300, 120, 70)
        return one(t, chain_frame(t, 12, 150, 60, 200, n_seen=9, local_kf=[2, 3], ref_kf=2), q_cap=512)
    if name == "no_observer":            # 2: points 8, 9 are in no keyframe
        t = tables_from_rows([[0, 1, 2], [2, 3, -1, 4], [4, 5], [6, 7]], 10)
        return one(t, frame([8, -1, 9, 8], local_kf=[3, 1], ref_kf=1))
    if name == "all_voted_bad":          # 3
        t = tables_from_rows([[0, 1], [1, 2], [3, 4]], 5, kf_bad=flags(3, [0, 1]))
        return one(t, frame([1, 0, -1, 2], local_kf=[2], ref_kf=2))
    if name == "tie":                    # 4: keyframes 1 and 3 get two votes each, keyframe 0 one
        t = tables_from_rows([[0], [1, 2], [5], [3, 4]], 6, best={}, parent={})
        return one(t, frame([0, 1, 2, 3, 4]))
    if name == "over_80_voted":          # 5: 90 keyframes see point 0; their neighbours 90..94 are never visited
        rows = [[0, 1 + k] for k in range(90)] + [[100 + k] for k in range(5)]
        t = tables_from_rows(rows, 105, best={k: [90 + k % 5] for k in range(90)}, parent={})
        return one(t, frame([0]), kf_cap=96)
    if name == "exactly_80_voted":       # 6: keyframe 0's neighbour 80 and child 81 enter, then 82 > 80 stops keyframe 1's neighbour 82
        rows = [[0, 1 + k] for k in range(80)] + [[100], [101], [102]]
        t = tables_from_rows(rows, 103, best={0: [80], 1: [82]}, parent={81: 0})
        return one(t, frame([0]), kf_cap=96)
    if name == "parent_ends_walk":       # 7: voted 1, 2; keyframe 1 adds neighbour 3, then its parent 0 and the walk is over
        t = tables_from_rows([[9], [0, 1], [0, 2], [3], [4]], 10, best={1: [3], 2: [4]}, parent={1: 0, 2: 1})
        return one(t, frame([0]))
    if name == "bad_parent_pushed":      # 8: voted 1; neighbour 2 is bad (skipped), 3 enters; the bad parent 0 enters untested
        t = tables_from_rows([[5, 6], [0, 1], [7], [8]], 9, kf_bad=flags(4, [0, 2]), best={1: [2, 3]}, parent={1: 0})
        return one(t, frame([0, 1]))
    if name == "shared_by_five":         # 9: point 7 in five keyframes at different keypoints
        rows = [[0, -1, 7], [7, 1], [2, 3, 7], [5, 7], [4, 7, 7]]
        t = tables_from_rows(rows, 8, best={}, parent={})
        return one(t, frame([0, 1, 2, 5, 4]))
    if name == "skip_own_point":         # 10
        t = tables_from_rows([[0, 1, 2, 3]], 4, best={}, parent={})
        return one(t, frame([2, -1, 0]))
    if name == "skip_frame_seen":        # 11
        t = tables_from_rows([[0, 1, 2, 3]], 4, best={}, parent={})
        return one(t, frame([2], frame_seen=[3, -1]))
    if name == "q_cap_overflow":         # 12
        t = chain_map(21, 12, 300, 120, 70)
        return one(t, chain_frame(t, 22, 150, 60, 200, n_seen=5), q_cap=64)
    if name == "long_keyframe":          # 13: one keyframe of 2,000 keypoints among 300
        kps = np.full(300, 40)
        kps[150] = 2000
        t = chain_map(31, 300, 6000, kps, 60)
        t["kf_bad"][150] = 0
        return one(t, chain_frame(t, 32, 2000, 2800, 3300, n_seen=20), kf_cap=128, q_cap=4096)
    if name == "three_frames_two_maps":  # 14
        a, b = chain_map(41, 12, 300, 120, 70), chain_map(42, 20, 400, 90, 60)
        frames = [chain_frame(a, 43, 150, 60, 200, n_seen=4, map_id=0, local_kf=[1], ref_kf=1),
                  chain_frame(b, 44, 130, 100, 260, n_seen=7, map_id=1),
                  chain_frame(a, 45, 140, 150, 290, map_id=0, local_kf=[5, 6, 7], ref_kf=6)]
        return {"maps": [a, b], "frames": frames, "kf_cap": 96, "q_cap": 512}
    if name == "hbm_histogram":          # 15: more keyframes than the LDS histogram of the vote pass holds (4,096)
        t = chain_map(51, 4200, 8400, 6, 8, p_bad_kf=0.05)
        return one(t, chain_frame(t, 52, 300, 4000, 4400, n_seen=3), kf_cap=512, q_cap=2048)
    if name == "ceilings":               # 16: every capacity at its ceiling (see ceiling_map)
        return one(ceiling_map(), frame(np.where(np.arange(30000) == 29999, 0, -1)), kf_cap=65535, q_cap=65536)
    raise KeyError(name)


def ceiling_map():
    """SLAMIT_LOCAL_MAP_MAX_KF = 65,535 keyframes that all observe point 0, so one tracked point (at keypoint 29,999 of a frame of
    SLAMIT_FRAME_MAX_KP keypoints) votes for all of them and the list has 65,535 entries; keyframe 0 has SLAMIT_LOCAL_MAP_MAX_ROW = 65,536
    keypoints with a point of its own at the last one, every other keyframe k has point k at keypoint 1.  The local points are
    65,536 = SLAMIT_FRUSTUM_MAX_N, and the first-occurrence keys reach (0 << 16 | 65535) and (65534 << 16 | 1).  No neighbours: with
    more than 80 voted nothing is expanded.  Built directly; the covisibility weights of tables_from_rows would be 65,535 squared."""
    K, row0 = 65535, 65536
    n_mp = K + 1
    rng = np.random.default_rng(61)
    first = np.full(row0, -1, np.int32)
    first[0], first[-1] = 0, K
    rest = np.stack([np.zeros(K - 1, np.int32), np.arange(1, K, dtype=np.int32)], 1).reshape(-1)
    kf_mp_ptr = np.concatenate([[0, row0], row0 + 2 * np.arange(1, K)]).astype(np.int32)
    obs_ptr = np.concatenate([[0], K + np.arange(n_mp)]).astype(np.int32)               # point 0: K observers; every other point: one
    obs_kf = np.concatenate([rng.permutation(K), np.arange(1, K), [0]]).astype(np.int32)
    return {"n_kf": K, "n_mp": n_mp, "obs_ptr": obs_ptr, "obs_kf": obs_kf, "mp_bad": np.zeros(n_mp, np.uint8), "kf_bad": np.zeros(K, np.uint8),
            "kf_mp_ptr": kf_mp_ptr, "kf_mp": np.concatenate([first, rest]), "kf_best": np.full((K, BEST), -1, np.int32),
            "kf_child_ptr": np.zeros(K + 1, np.int32), "kf_child": np.zeros(0, np.int32), "kf_parent": np.full(K, -1, np.int32),
            "mp_pos": rng.uniform(-4, 4, (n_mp, 3)).astype(np.float32), "mp_normal": rng.uniform(-1, 1, (n_mp, 3)).astype(np.float32),
            "mp_max_dist": rng.uniform(4, 9, n_mp).astype(np.float32), "mp_min_dist": rng.uniform(0.1, 2, n_mp).astype(np.float32)}
