"""Seeded and hand-built maps for the covisibility tests (KeyFrame::UpdateConnections, LocalMapping::KeyFrameCulling).

A fixture is dict(t: tables in the layout of slamit_map_index, x: columns and graph rows in the layout of slamit_covis_index plus the
test-only column obs_idx (the keypoint index of an observation, for the mock objects), and either uc: dict(k, first) or
cull: dict(c, monocular)).  Observations are the inverse of the keyframes' rows; the graph before the call is what a fixture says."""
import functools

import numpy as np

BEST = 10
GRAPH = ("cw_kf", "cw_w", "cw_n", "ord_kf", "ord_w", "ord_n", "kf_best")


class Map:
    """Keyframes' rows built point by point.  point([(kf, octave, stereo, depth), ...]) adds a map point seen at a new keypoint of each
    listed keyframe (shorter tuples take octave 0, mono, depth 1)."""

    def __init__(self, n_kf, row_cap=16, origin=-1, seed=0):
        self.n_kf, self.row_cap, self.origin = n_kf, row_cap, origin
        self.rows = [[] for _ in range(n_kf)]       # per keypoint: (point, octave, stereo, depth)
        self.bad = []
        self.cw = [dict() for _ in range(n_kf)]
        self.ord = [None] * n_kf                    # [(kf, w)], None: the sort of the whole cw row
        self.best = {}                              # rows of kf_best that are not the first ten of ord
        self.kf_bad, self.not_erase, self.th_depth = set(), set(), [5.0] * n_kf
        self.rng = np.random.default_rng(seed)

    def point(self, obs, bad=False):
        p = len(self.bad)
        self.bad.append(bad)
        for o in obs:
            kf, octave, stereo, depth = (tuple(o) + (0, False, 1.0)[len(o) - 1:]) if isinstance(o, tuple) else (o, 0, False, 1.0)
            self.rows[kf].append((p, octave, stereo, depth))
        return p

    def points(self, n, obs, **kw):
        return [self.point(obs, **kw) for _ in range(n)]

    def null(self, kf, n=1):
        for _ in range(n):
            self.rows[kf].append((-1, 0, False, 1.0))

    def connect(self, a, b, w):
        self.cw[a][b] = w
        self.cw[b][a] = w

    def shuffle(self, kf):
        self.rows[kf] = [self.rows[kf][i] for i in self.rng.permutation(len(self.rows[kf]))]

    def tables(self):
        K, n_mp, cap = self.n_kf, len(self.bad), self.row_cap
        ptr = np.zeros(K + 1, np.int32)
        ptr[1:] = np.cumsum([len(r) for r in self.rows])
        flat = [e for r in self.rows for e in r]
        col = lambda i, dt: np.array([e[i] for e in flat], dt).reshape(-1)
        obs = [[] for _ in range(n_mp)]
        for k, r in enumerate(self.rows):
            for i, (p, octave, stereo, _) in enumerate(r):
                if p >= 0:
                    obs[p].append((k, i, octave, 2 if stereo else 1))
        obs = [[o[i] for i in self.rng.permutation(len(o))] for o in obs]
        obs_ptr = np.zeros(n_mp + 1, np.int32)
        obs_ptr[1:] = np.cumsum([len(o) for o in obs])
        ocol = lambda i, dt: np.array([e[i] for o in obs for e in o], dt).reshape(-1)
        f32 = lambda *shape: self.rng.uniform(-4, 4, shape).astype(np.float32)
        flag = lambda n, which: np.array([i in which for i in range(n)], np.uint8)
        x = {"row_cap": cap, "origin_kf": self.origin, "obs_octave": ocol(2, np.uint8), "obs_weight": ocol(3, np.uint8), "obs_idx": ocol(1, np.int32),
             "mp_nobs": np.array([sum(e[3] for e in o) for o in obs], np.int32), "kf_octave": col(1, np.uint8), "kf_depth": col(3, np.float32),
             "kf_th_depth": np.array(self.th_depth, np.float32), "kf_not_erase": flag(K, self.not_erase)}
        # the graph as it stands: rows past their count hold sentinels that no call may touch
        x.update(cw_kf=np.full((K, cap), -11, np.int32), cw_w=np.full((K, cap), -12, np.int32), cw_n=np.zeros(K, np.int32),
                 ord_kf=np.full((K, cap), -13, np.int32), ord_w=np.full((K, cap), -14, np.int32), ord_n=np.zeros(K, np.int32),
                 kf_best=np.full((K, BEST), -1, np.int32))
        for k in range(K):
            cw = sorted(self.cw[k].items())
            order = self.ord[k] if self.ord[k] is not None else sorted(cw, key=lambda e: (-e[1], -e[0]))
            x["cw_n"][k], x["ord_n"][k] = len(cw), len(order)
            x["cw_kf"][k, :len(cw)], x["cw_w"][k, :len(cw)] = [e[0] for e in cw], [e[1] for e in cw]
            x["ord_kf"][k, :len(order)], x["ord_w"][k, :len(order)] = [e[0] for e in order], [e[1] for e in order]
            best = self.best.get(k, [e[0] for e in order][:BEST])
            x["kf_best"][k, :len(best)] = best
        t = {"n_kf": K, "n_mp": n_mp, "obs_ptr": obs_ptr, "obs_kf": ocol(0, np.int32), "mp_bad": np.array(self.bad, np.uint8).reshape(-1),
             "kf_bad": flag(K, self.kf_bad), "kf_mp_ptr": ptr, "kf_mp": col(0, np.int32), "kf_best": x["kf_best"],
             "kf_child_ptr": np.zeros(K + 1, np.int32), "kf_child": np.zeros(0, np.int32), "kf_parent": np.full(K, -1, np.int32),
             "mp_pos": f32(n_mp, 3), "mp_normal": f32(n_mp, 3), "mp_max_dist": self.rng.uniform(4, 9, n_mp).astype(np.float32),
             "mp_min_dist": self.rng.uniform(0.1, 2, n_mp).astype(np.float32)}
        return t, x


def uc(m, k, first=False):
    t, x = m.tables()
    return {"t": t, "x": x, "uc": {"k": k, "first": first}}


def cull(m, c, monocular=True):
    t, x = m.tables()
    return {"t": t, "x": x, "cull": {"c": c, "monocular": monocular}}


def seeded(n_kf, n_kp, seed, row_cap=64, span=6, per_point=5, stereo=0.0, bad=0.03, octaves=4):
    """A chain of keyframes: a point is seen by about per_point keyframes within `span` of one another."""
    rng = np.random.default_rng(seed)
    m = Map(n_kf, row_cap=row_cap, origin=0, seed=seed)
    n_points = n_kf * n_kp // per_point
    for _ in range(n_points):
        first = int(rng.integers(0, n_kf))
        who = sorted(set(int(v) for v in np.clip(first + rng.integers(0, span, per_point + int(rng.integers(-2, 3))), 0, n_kf - 1)))
        who = [k for k in who if len(m.rows[k]) < n_kp]
        if who:
            m.point([(k, int(rng.integers(0, octaves)), bool(rng.random() < stereo), float(rng.uniform(-0.5, 7))) for k in who], bad=bool(rng.random() < bad))
    for k in range(n_kf):
        m.null(k, min(n_kp - len(m.rows[k]), int(rng.integers(0, 1 + n_kp // 20))))
        m.shuffle(k)
    return m


def with_graph(m, skip=()):
    """The graph a map has after UpdateConnections ran on every keyframe but `skip`, weights counted from the rows."""
    seen = {}
    for k, r in enumerate(m.rows):
        for e in r:
            if e[0] >= 0 and not m.bad[e[0]]:
                seen.setdefault(e[0], []).append(k)
    w = [dict() for _ in range(m.n_kf)]
    for o in seen.values():
        for a in o:
            for b in o:
                if a != b:
                    w[a][b] = w[a].get(b, 0) + 1
    for a in range(m.n_kf):
        for b, n in w[a].items():
            if a < b and a not in skip and b not in skip and len(m.cw[a]) < m.row_cap and len(m.cw[b]) < m.row_cap:
                m.connect(a, b, n)
    return m


# ---- UpdateConnections ----------------------------------------------------------------------------------------------------------

def shared(m, k, counts, **kw):
    """counts[j] points seen by k and j alone."""
    for j, n in counts.items():
        m.points(n, [k, j], **kw)


def _uc(name):
    if name == "plain":                       # neighbours above and below 15, none of them knows k yet: inserted
        return uc(with_graph(seeded(14, 120, 1, row_cap=16, span=5), skip=(6,)), 6)
    if name == "no_observer":
        m = Map(4)
        m.points(5, [2]); m.points(20, [0, 1]); m.connect(0, 1, 20); m.connect(2, 3, 9)      # k's old rows stay, stale as they are
        return uc(m, 2, first=True)
    if name == "tie_below":                   # nobody reaches 15, two share the maximum: the lowest slot
        m = Map(6)
        shared(m, 2, {1: 3, 3: 7, 4: 7, 5: 2})
        return uc(m, 2)
    if name == "fifteen_fourteen":
        m = Map(5)
        shared(m, 0, {1: 14, 3: 15, 4: 14})
        return uc(m, 0)
    if name == "equal_weights":               # within equal weight the higher slot comes first
        m = Map(8)
        shared(m, 3, {0: 20, 2: 20, 5: 25, 6: 20, 7: 16, 1: 4})
        return uc(m, 3)
    if name == "bad_observer":
        m = Map(4)
        shared(m, 1, {0: 16, 2: 18, 3: 5})
        m.kf_bad = {2}
        return uc(m, 1)
    if name == "skips":                       # NULL and bad points and k itself
        m = Map(5)
        shared(m, 2, {0: 15, 1: 10})
        shared(m, 2, {1: 8, 3: 30}, bad=True)
        m.null(2, 7); m.points(4, [2]); m.shuffle(2)
        return uc(m, 2)
    if name == "neighbour_holds_same":        # (k, w) is there: j's thresholded ord row and its kf_best stay
        m = Map(6)
        shared(m, 1, {4: 17, 2: 16})
        m.cw[4] = {1: 17, 0: 30, 3: 4, 5: 15}
        m.ord[4] = [(0, 30), (1, 17), (5, 15)]            # as UpdateConnections on 4 left it: without (3, 4)
        m.best[4] = [0, 1, 5, 2]                          # not the first ten of anything: it must survive
        return uc(m, 1)
    if name == "neighbour_other_weight":      # re-sorted from the WHOLE cw row: the below-threshold entries are now listed
        m = Map(7)
        shared(m, 1, {4: 17})
        m.cw[4] = {1: 12, 0: 30, 3: 4, 5: 17, 6: 2}
        m.ord[4] = [(0, 30), (5, 17)]
        return uc(m, 1)
    if name == "old_entries_dropped":         # k's cw row shrinks: the entries no longer counted go
        m = Map(8)
        shared(m, 5, {0: 16, 7: 3})
        for j, w in ((1, 40), (2, 22), (3, 15), (4, 9), (6, 1)):
            m.connect(5, j, w)
        return uc(m, 5)
    if name in ("first_origin", "first_other"):
        m = Map(5, origin=2 if name == "first_origin" else 0)
        shared(m, 2, {1: 18, 3: 18, 4: 30})
        return uc(m, 2, first=True)
    if name == "k_row_overflow":              # 17 counted keyframes, rows of 16
        m = Map(20, row_cap=16)
        shared(m, 9, {j: 1 + j for j in range(18) if j != 9})
        m.connect(9, 19, 5)
        return uc(m, 9, first=True)
    if name == "neighbour_row_overflow":      # keyframe 3's row is full and lacks k; keyframe 4 has room
        m = Map(24, row_cap=16)
        shared(m, 0, {3: 20, 4: 21})
        for j in range(5, 21):
            m.connect(3, j, 10 + j)
        return uc(m, 0)
    if name in ("lds_edge", "hbm_counts"):    # on each side of the vote pass' switch from the LDS histogram to HBM atomics
        n_kf = 4096 if name == "lds_edge" else 4100
        m = Map(n_kf, row_cap=16)
        shared(m, 7, {n_kf - 1: 19, n_kf - 2: 15, 4000: 14, 0: 1, 63: 2, 64: 33})
        m.null(7, 300); m.shuffle(7)
        return uc(m, 7, first=True)
    if name == "large":                       # rows of 2,000 keypoints: more than one stride of the vote pass; every keyframe a neighbour
        m = seeded(40, 2000, 5, row_cap=64, span=40, per_point=6)
        m.null(21, 2000 - len(m.rows[21])); m.shuffle(21)
        return uc(with_graph(m, skip=(21,)), 21, first=True)
    raise KeyError(name)


UC_NAMES = ("plain", "no_observer", "tie_below", "fifteen_fourteen", "equal_weights", "bad_observer", "skips", "neighbour_holds_same",
            "neighbour_other_weight", "old_entries_dropped", "first_origin", "first_other", "k_row_overflow", "neighbour_row_overflow", "lds_edge",
            "hbm_counts", "large")

# ---- KeyFrameCulling ------------------------------------------------------------------------------------------------------------
# keyframe 0 is the current one, 1.. the candidates, W.. three or four witnesses that are nobody's candidate
W = (10, 11, 12, 13)


def candidates(m, c, kfs):
    m.ord[c] = [(k, 100 - i) for i, k in enumerate(kfs)]
    m.cw[c] = {k: 100 - i for i, k in enumerate(kfs)}


def redundant(m, kf, n, octave=0):
    m.points(n, [(kf, octave)] + [(w, octave) for w in W[:3]])


def _cull(name):
    m = Map(14)
    if name == "no_cull":
        m = with_graph(seeded(30, 150, 7, row_cap=32, span=5, per_point=4))
        return cull(m, 12)
    if name == "no_cull_stereo":
        m = with_graph(seeded(30, 150, 8, row_cap=32, span=5, per_point=4, stereo=0.5))
        return cull(m, 12, monocular=False)
    if name == "ninety_percent":              # 9 of 10 stays, 10 of 10 goes
        candidates(m, 0, [1, 2])
        redundant(m, 1, 9); m.point([1])
        redundant(m, 2, 10)
        return cull(m, 0)
    if name == "three_observations":          # Observations() == 3: in nMPs only
        candidates(m, 0, [1])
        redundant(m, 1, 9)
        m.point([1, W[0], W[1]])              # 9 of 10 with it, 9 of 9 without: kept only because it counts
        return cull(m, 0)
    if name == "octaves":                     # octave + 1 counts, octave + 2 does not
        candidates(m, 0, [1, 2])
        m.points(10, [(1, 2), (W[0], 3), (W[1], 3), (W[2], 0)])
        m.points(10, [(2, 2), (W[0], 3), (W[1], 4), (W[2], 3), (W[3], 4)])
        return cull(m, 0)
    if name == "self_among_observers":        # the candidate's own observation is not one of the three
        candidates(m, 0, [1])
        m.points(10, [(1, 0), (W[0], 0), (W[1], 0), (W[2], 5)])
        return cull(m, 0)
    if name == "cascade_keeps":               # culling 1 takes 2's third observer away: 2 stays, although alone it would go
        candidates(m, 0, [1, 2])
        redundant(m, 1, 5)
        m.points(10, [1, 2, W[0], W[1]])
        return cull(m, 0)
    if name == "cascade_culls":               # two points of 2 are left with two observations: they leave its nMPs, 9 of 9 goes
        candidates(m, 0, [1, 2, 3])
        redundant(m, 1, 30)
        redundant(m, 2, 9)
        m.points(2, [1, 2, W[0]])
        redundant(m, 3, 9); m.point([3, W[0]])
        return cull(m, 0)
    if name == "stereo_weights":              # weights of 2 in Observations(), and in what a cull takes away
        candidates(m, 0, [1, 2])
        redundant(m, 1, 60)
        m.points(4, [(1, 0, True), (W[0], 0, True)])                 # Observations() 4, one other observer: in nMPs only
        redundant(m, 2, 9)
        m.points(1, [(1, 0, True), 2, W[0]])                         # 4 - 2 = 2: bad once 1 is gone
        m.points(1, [(1, 0, True), 2, (W[0], 0, True), W[1]])        # 6 - 2 = 4 > 3 but two observers left: in nMPs only, 9 of 10
        return cull(m, 0)
    if name == "depth_gate":                  # > th skipped, == th counted, < 0 skipped
        candidates(m, 0, [1, 2])
        m.th_depth[1] = m.th_depth[2] = 3.5
        far = lambda kf, d: m.point([(kf, 0, False, d)])
        redundant(m, 1, 9); far(1, 3.75); far(1, -0.25); far(1, 3.75)     # 9 of 9: goes
        redundant(m, 2, 9); far(2, 3.5)                                     # 9 of 10: stays
        return cull(m, 0, monocular=False)
    if name == "origin":
        m.origin = 1
        candidates(m, 0, [1, 2])
        redundant(m, 1, 10); redundant(m, 2, 10)
        return cull(m, 0)
    if name == "not_erase":                   # verdict 2, and 2 behind it is judged as if 1 were there
        candidates(m, 0, [1, 2])
        m.not_erase = {1}
        redundant(m, 1, 5)
        m.points(10, [1, 2, W[0], W[1]])
        return cull(m, 0)
    if name == "no_points":                   # nMPs == 0: 0 > 0.0 is false
        candidates(m, 0, [1, 2])
        m.null(1, 6); m.points(3, [1, W[0], W[1], W[2]], bad=True)
        redundant(m, 2, 3)
        return cull(m, 0)
    if name == "long_cascade":                # several culls in one call, seeded: dense maps where most keyframes are redundant
        m = with_graph(seeded(40, 200, 9, row_cap=32, span=12, per_point=9, octaves=2, bad=0.0))
        return cull(m, 20)
    raise KeyError(name)


CULL_NAMES = ("no_cull", "no_cull_stereo", "ninety_percent", "three_observations", "octaves", "self_among_observers", "cascade_keeps", "cascade_culls",
              "stereo_weights", "depth_gate", "origin", "not_erase", "no_points", "long_cascade")


@functools.lru_cache(maxsize=None)
def fixture(kind, name):
    """kind: "uc" or "cull".  Computed once per process; do not modify."""
    return _uc(name) if kind == "uc" else _cull(name)
