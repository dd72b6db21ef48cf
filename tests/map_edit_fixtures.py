"""The maps and edit lists of the map-edit tests.  A fixture is dict(name, t, x, edits): t in the layout of slamit_map_index (every table
MapIndex uploads), x the edit columns (obs_idx, obs_octave, obs_weight, mp_nobs, mp_ref_kf), edits tuples (kind, flags, mp, kf, idx,
octave, weight).  Every map is consistent: kf_mp[kf][idx] == p for every observation (p, kf, idx), and a keyframe's row has free
keypoints past the ones in use, for adds."""
import functools

import numpy as np

from tests.map_edit_ref import ADD_OBS, ERASE_OBS, MATCH, SET_BAD

SCAN_BLOCK = 256   # ME_SCAN_BLOCK


def build_map(n_kf, rows, spare=6, weights=None, bad=(), nobs=None, ref=None):
    """rows[p]: the keyframes observing point p, in row order.  weights[(p, kf)] = 2 marks a stereo observation.  Keypoint indices are
    handed out per keyframe in point order; every keyframe keeps `spare` free keypoints at the end of its row."""
    weights, n_mp = weights or {}, len(rows)
    used = [0] * n_kf
    obs_kf, obs_idx, obs_w, obs_ptr = [], [], [], [0]
    for p, row in enumerate(rows):
        for k in row:
            obs_kf.append(k); obs_idx.append(used[k]); obs_w.append(weights.get((p, k), 1))
            used[k] += 1
        obs_ptr.append(len(obs_kf))
    kf_mp_ptr = np.concatenate([[0], np.cumsum([u + spare for u in used])]).astype(np.int32)
    kf_mp = np.full(kf_mp_ptr[-1], -1, np.int32)
    o = 0
    for p, row in enumerate(rows):
        for k in row:
            kf_mp[kf_mp_ptr[k] + obs_idx[o]] = p
            o += 1
    obs_kf, obs_idx, obs_w = np.array(obs_kf, np.int32).reshape(-1), np.array(obs_idx, np.int32).reshape(-1), np.array(obs_w, np.uint8).reshape(-1)
    obs_ptr = np.array(obs_ptr, np.int32)
    mp_bad = np.zeros(n_mp, np.uint8)
    mp_bad[list(bad)] = 1
    mp_nobs = np.diff(np.concatenate([[0], np.cumsum(obs_w, dtype=np.int64)])[obs_ptr]).astype(np.int32).reshape(-1)
    for p, v in (nobs or {}).items():
        mp_nobs[p] = v
    mp_ref = np.array([row[0] if len(row) else -1 for row in rows], np.int32).reshape(-1)
    for p, v in (ref or {}).items():
        mp_ref[p] = v
    rng = np.random.default_rng(n_kf * 7919 + n_mp)
    t = {"n_kf": n_kf, "n_mp": n_mp, "obs_ptr": obs_ptr, "obs_kf": obs_kf, "mp_bad": mp_bad, "kf_bad": np.zeros(n_kf, np.uint8), "kf_mp_ptr": kf_mp_ptr,
         "kf_mp": kf_mp, "kf_best": np.full((n_kf, 10), -1, np.int32), "kf_child_ptr": np.zeros(n_kf + 1, np.int32), "kf_child": np.zeros(0, np.int32),
         "kf_parent": np.full(n_kf, -1, np.int32), "mp_pos": rng.uniform(-1, 1, (n_mp, 3)).astype(np.float32),
         "mp_normal": rng.uniform(-1, 1, (n_mp, 3)).astype(np.float32), "mp_max_dist": np.full(n_mp, 9, np.float32), "mp_min_dist": np.full(n_mp, 1, np.float32)}
    x = {"obs_idx": obs_idx, "obs_octave": (rng.integers(0, 8, len(obs_kf))).astype(np.uint8), "obs_weight": obs_w, "mp_nobs": mp_nobs, "mp_ref_kf": mp_ref}
    return t, x


def free_idx(t, k, j=0):
    """The j-th free keypoint at the end of keyframe k's row (spare ones are never in use)."""
    return int(t["kf_mp_ptr"][k + 1] - t["kf_mp_ptr"][k]) - 1 - j


def idx_of(t, x, p, k):
    sl = slice(int(t["obs_ptr"][p]), int(t["obs_ptr"][p + 1]))
    return int(x["obs_idx"][sl][list(t["obs_kf"][sl]).index(k)])


def single():
    """Every single-point case and every cross-point order on kf_mp the issue names, in ONE interleaved list."""
    rows = [[0, 1, 2],            # 0  add of a present observer
            [0, 1, 2, 3],         # 1  erase of an absent observer
            [1, 2, 3, 4],         # 2  erase of the reference keyframe with observers left; nobs 4 -> 3 stays
            [2],                  # 3  erase of the reference keyframe as the last observer (nobs kept at 5 by the caller: no cascade)
            [0, 1, 2],            # 4  erase with MATCH: nobs 3 -> 2, cascade
            [0, 1],               # 5  stereo: nobs 4 -> 2 by one weight-2 erase, cascade
            [],                   # 6  a bad point, SET_BAD again
            [0, 1, 2, 3],         # 7  add -> erase -> add of the same keyframe
            [0, 1, 2],            # 8  SET_BAD, then an add onto the point it turned bad
            [0, 1, 3, 4, 5],      # 9  erase|MATCH of (9, kf 3), THEN add|MATCH of point 10 onto the same keypoint
            [0, 1, 2, 4],         # 10
            [0, 1, 2, 4, 5],      # 11 add|MATCH of point 12 onto (kf 4, its keypoint), THEN erase|MATCH of (11, kf 4)
            [0, 1, 2, 3],         # 12
            [5, 6, 7],            # 13 erase of kf 5: cascade wipes (kf 7, its keypoint) ... THEN point 14 is added|MATCH there
            [0, 1, 2, 3],         # 14
            [3, 1, 2]]            # 15 row stored out of slot order: erase of ref 3 -> smallest slot 1, not the first stored
    t, x = build_map(8, rows, weights={(5, 0): 2, (5, 1): 2}, bad=(6,), nobs={6: 3, 3: 5})
    i9, i11, i13 = idx_of(t, x, 9, 3), idx_of(t, x, 11, 4), idx_of(t, x, 13, 7)
    E = [(ERASE_OBS, MATCH, 9, 3, 0, 0, 0),
         (ADD_OBS, 0, 7, 5, free_idx(t, 5), 3, 1),
         (ADD_OBS, MATCH, 12, 4, i11, 1, 1),
         (ADD_OBS, 0, 0, 1, free_idx(t, 1), 2, 1),
         (ERASE_OBS, 0, 13, 5, 0, 0, 0),
         (SET_BAD, 0, 8, 0, 0, 0, 0),
         (ERASE_OBS, 0, 7, 5, 0, 0, 0),
         (ADD_OBS, MATCH, 10, 3, i9, 4, 2),
         (ERASE_OBS, 0, 1, 7, 0, 0, 0),
         (ERASE_OBS, 0, 2, 1, 0, 0, 0),
         (ADD_OBS, MATCH, 14, 7, i13, 5, 1),
         (ERASE_OBS, MATCH, 11, 4, 0, 0, 0),
         (ERASE_OBS, 0, 3, 2, 0, 0, 0),
         (ADD_OBS, MATCH, 7, 5, free_idx(t, 5, 1), 6, 2),
         (ERASE_OBS, MATCH, 4, 2, 0, 0, 0),
         (SET_BAD, 0, 6, 0, 0, 0, 0),
         (ERASE_OBS, 0, 5, 0, 0, 0, 0),
         (ADD_OBS, MATCH, 8, 4, free_idx(t, 4), 7, 1),
         (ERASE_OBS, 0, 15, 3, 0, 0, 0)]
    return {"name": "single", "t": t, "x": x, "edits": E}


def limits():
    """Rows of 0, 1, 63, 64, 65, 511, 512 and 513 observers, each edited; the two overflows; points with 1, 64 and 65 edits."""
    n_kf = 600
    sizes = [0, 1, 63, 64, 65, 511, 512, 512, 513, 513, 4, 40, 4]   # points 0 .. 12
    rows = [list(range(s)) for s in sizes]
    t, x = build_map(n_kf, rows, spare=4, nobs={0: 7})
    E = [(ADD_OBS, MATCH, 0, 599, free_idx(t, 599), 1, 1),                # 0 -> 1
         (ERASE_OBS, 0, 1, 0, 0, 0, 0),                                   # 1 -> 0: cascade on an emptied row
         (ADD_OBS, 0, 2, 598, free_idx(t, 598), 2, 1),                    # 63 -> 64
         (ADD_OBS, MATCH, 3, 597, free_idx(t, 597), 3, 2),                # 64 -> 65: the second lane round
         (ERASE_OBS, MATCH, 4, 64, 0, 0, 0),                              # 65 -> 64: the entry of the second round
         (ADD_OBS, 0, 5, 596, free_idx(t, 596), 4, 1),                    # 511 -> 512: the ceiling itself
         (ADD_OBS, MATCH, 6, 595, free_idx(t, 595), 5, 1),                # 512 + 1: OBS_OVERFLOW, nothing applied, kf_mp not written
         (ERASE_OBS, MATCH, 6, 3, 0, 0, 0),                               #          ... nor this earlier-looking erase of the same point
         (ERASE_OBS, 0, 7, 511, 0, 0, 0), (ADD_OBS, 0, 7, 594, free_idx(t, 594), 6, 1),   # 512 -> 511 -> 512: fits
         (ERASE_OBS, MATCH, 8, 0, 0, 0, 0)]                               # a 513-row with an edit: OBS_OVERFLOW; point 9: a 513-row without
    E.append((ERASE_OBS, MATCH, 10, 2, 0, 0, 0))                          # point 10: one edit
    for j in range(32):                                                   # point 11: 64 edits, adds of new keyframes and erases of old ones
        E.append((ADD_OBS, MATCH if j & 1 else 0, 11, 100 + j, free_idx(t, 100 + j), j & 7, 1 + (j & 1)))
        E.append((ERASE_OBS, MATCH if j & 2 else 0, 11, j, 0, 0, 0))
    for j in range(65):                                                   # point 12: 65 edits: EDIT_OVERFLOW, none applied
        E.append((ADD_OBS, MATCH, 12, 200 + j, free_idx(t, 200 + j), 0, 1) if j % 3 else (ERASE_OBS, MATCH, 12, j % 4, 0, 0, 0))
    E = E[:8] + E[-40:] + E[8:-40]                                        # point 12's tail early in the list: list order is not point order
    return {"name": "limits", "t": t, "x": x, "edits": E}


def random_fixture(name, seed, n_kf, n_mp, n_edits, kp_spare=8, density=3.0, force_points=()):
    """A random consistent map and a random list: every kind, MATCH on half, keyframes present and absent, in shuffled order."""
    rng = np.random.default_rng(seed)
    lens = np.minimum(rng.poisson(density, n_mp), n_kf)
    rows = [sorted(rng.choice(n_kf, int(l), replace=False).tolist(), key=lambda k: (k * 7) % 5) for l in lens]
    t, x = build_map(n_kf, rows, spare=kp_spare, weights={(p, rows[p][0]): 2 for p in range(0, n_mp, 5) if rows[p]})
    pts = np.concatenate([rng.integers(0, n_mp, n_edits - len(force_points)), np.array(force_points, np.int64)]).astype(np.int64)
    pts[: n_edits // 3] = pts[rng.integers(0, max(n_edits // 8, 1), n_edits // 3)]   # some points many times
    rng.shuffle(pts)
    E, spare_used = [], {}
    for p in pts.tolist():
        r = rng.random()
        flags = int(rng.integers(0, 2))
        if r < 0.45:
            k = int(rng.integers(0, n_kf))
            j = spare_used.get(k, 0)
            spare_used[k] = (j + 1) % kp_spare
            E.append((ADD_OBS, flags, p, k, free_idx(t, k, j), int(rng.integers(0, 8)), int(rng.integers(1, 3))))
        elif r < 0.9:
            k = rows[p][int(rng.integers(0, len(rows[p])))] if rows[p] and rng.random() < 0.8 else int(rng.integers(0, n_kf))
            E.append((ERASE_OBS, flags, p, k, 0, 0, 0))
        else:
            E.append((SET_BAD, 0, p, 0, 0, 0, 0))
    return {"name": name, "t": t, "x": x, "edits": E}


def nothing():
    fx = random_fixture("nothing", 5, 12, 40, 0)
    rows = [fx["t"]["obs_kf"][fx["t"]["obs_ptr"][p]:fx["t"]["obs_ptr"][p + 1]].tolist() for p in range(40)]
    E = []
    for p in range(40):
        absent = [k for k in range(12) if k not in rows[p]]
        E.append((ERASE_OBS, MATCH, p, absent[0], 0, 0, 0))
        if rows[p]:
            E.append((ADD_OBS, 0, p, rows[p][-1], free_idx(fx["t"], rows[p][-1]), 1, 1))
    return dict(fx, edits=E[::-1])


def empty():
    return dict(random_fixture("empty", 6, 9, 30, 0), name="empty")


@functools.lru_cache(maxsize=None)
def all_fixtures():
    B = SCAN_BLOCK
    fxs = [single(), limits(), nothing(), empty(), random_fixture("shuffled", 11, 40, 300, 900)]
    for n_mp in (B - 1, B, B + 1):
        fxs.append(random_fixture("scan%d" % n_mp, 100 + n_mp, 20, n_mp, 200, force_points=(0, n_mp - 1, n_mp - 1)))
    # one above the square of the scan block: the partial sums' own scan takes two rounds of its workgroup (and five wavefronts)
    fxs.append(random_fixture("scan%d" % (B * B + 1), 7, 64, B * B + 1, 3000, density=1.5, force_points=(0, B - 1, B, B * B - 1, B * B, B * B)))
    return tuple(fxs)


def by_name(name):
    return next(fx for fx in all_fixtures() if fx["name"] == name)


@functools.lru_cache(maxsize=None)
def expected(name, cap_delta=None):
    """The restatement's result on a fixture, computed once and shared.  cap_delta: obs_cap_out = the need + cap_delta."""
    from tests.map_edit_ref import apply

    fx = by_name(name)
    if cap_delta is None:
        return apply(fx["t"], fx["x"], fx["edits"])
    return apply(fx["t"], fx["x"], fx["edits"], expected(name)["n_obs_out"] + cap_delta)
