"""Checker for the device Sim3Solver: a numpy restatement of Sim3Solver::ComputeSim3 (Sim3Solver.cc:226-337), CheckInliers
(:340-364, :382-423), the sampler (:163-177), SetRansacParameters (:114-138) and iterate()'s acceptance scan (:183-204), written
from the reference's text and independent of csrc/sim3_horn.h.  Two precisions:

  ref32  keeps the reference's float / double split operation by operation; the eigenvector of the largest eigenvalue comes from
         numpy.linalg.eigh on the float N (sign fixed to q0 >= 0: q and -q are the same rotation)
  ref64  the same formulas, all double

OpenCV is not available and the reference tree holds no fixture for this class, so parity is against this restatement
("unpinned", like the ORB half): the float/double gap between the two precisions is the yardstick (admissibility, below).
Everything is vectorised over the hypotheses: arrays carry a leading H axis.
"""
import math

import numpy as np

f64 = np.float64


def _dot3(a0, a1, a2, b0, b1, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def compute_sim3(x1, x2, triples, fix_scale, prec):
    """-> dict R (H, 3, 3), t (H, 3), s (H), sR, sRi (H, 3, 3), ti (H, 3) in the working float type of `prec` (32 or 64)."""
    f = np.float32 if prec == 32 else np.float64
    x1, x2, tr = np.asarray(x1, f), np.asarray(x2, f), np.asarray(triples, np.int64).reshape(-1, 3)
    P1, P2 = x1[tr], x2[tr]                                   # (H, point, axis)
    third = f(1.0 / 3.0)
    with np.errstate(all="ignore"):
        O1 = ((P1[:, 0] + P1[:, 1]) + P1[:, 2]) * third       # (H, axis)
        O2 = ((P2[:, 0] + P2[:, 1]) + P2[:, 2]) * third
        Pr1 = np.transpose(P1 - O1[:, None, :], (0, 2, 1))    # (H, axis, point)
        Pr2 = np.transpose(P2 - O2[:, None, :], (0, 2, 1))
        M = np.empty((len(tr), 3, 3), f)                      # M = Pr2 * Pr1^T
        for i in range(3):
            for j in range(3):
                M[:, i, j] = _dot3(Pr2[:, i, 0], Pr2[:, i, 1], Pr2[:, i, 2], Pr1[:, j, 0], Pr1[:, j, 1], Pr1[:, j, 2])
        m = M.astype(f64)                                     # N11 .. N44 are doubles (:247), N is a float matrix (:262)
        N = np.empty((len(tr), 4, 4), f)
        N[:, 0, 0] = m[:, 0, 0] + m[:, 1, 1] + m[:, 2, 2]
        N[:, 0, 1] = N[:, 1, 0] = m[:, 1, 2] - m[:, 2, 1]
        N[:, 0, 2] = N[:, 2, 0] = m[:, 2, 0] - m[:, 0, 2]
        N[:, 0, 3] = N[:, 3, 0] = m[:, 0, 1] - m[:, 1, 0]
        N[:, 1, 1] = m[:, 0, 0] - m[:, 1, 1] - m[:, 2, 2]
        N[:, 1, 2] = N[:, 2, 1] = m[:, 0, 1] + m[:, 1, 0]
        N[:, 1, 3] = N[:, 3, 1] = m[:, 2, 0] + m[:, 0, 2]
        N[:, 2, 2] = -m[:, 0, 0] + m[:, 1, 1] - m[:, 2, 2]
        N[:, 2, 3] = N[:, 3, 2] = m[:, 1, 2] + m[:, 2, 1]
        N[:, 3, 3] = -m[:, 0, 0] - m[:, 1, 1] + m[:, 2, 2]
        q = np.full((len(tr), 4), np.nan, f)
        ok = np.isfinite(N).all(axis=(1, 2))
        if ok.any():
            _, vecs = np.linalg.eigh(N[ok])                   # ascending: the last column belongs to the largest eigenvalue
            q[ok] = vecs[:, :, 3].astype(f)
        q = np.where(q[:, :1] < 0, -q, q)
        qd = q.astype(f64)
        nrm = np.sqrt((qd[:, 1] * qd[:, 1] + qd[:, 2] * qd[:, 2]) + qd[:, 3] * qd[:, 3])
        ang = np.arctan2(nrm, qd[:, 0])
        k = (2.0 * ang) / nrm
        v = (k[:, None] * qd[:, 1:]).astype(f)                # the angle-axis vector, a float matrix
        # cv::Rodrigues in double
        r = v.astype(f64)
        theta = np.sqrt((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2])
        c, s = np.cos(theta), np.sin(theta)
        c1, it = 1.0 - c, 1.0 / theta
        rx, ry, rz = r[:, 0] * it, r[:, 1] * it, r[:, 2] * it
        z = np.zeros_like(rx)
        rrt = np.stack([rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz], 1)
        rxm = np.stack([z, -rz, ry, rz, z, -rx, -ry, rx, z], 1)
        eye = np.eye(3).reshape(1, 9)
        Rd = (c[:, None] * eye + c1[:, None] * rrt) + s[:, None] * rxm
        Rd = np.where((theta < np.finfo(f64).eps)[:, None], eye, Rd)
        R = Rd.astype(f).reshape(-1, 3, 3)
        # scale
        if fix_scale:
            s12 = np.ones(len(tr), f)
        else:
            nom, den = np.zeros(len(tr), f64), np.zeros(len(tr), f64)
            for i in range(3):
                for j in range(3):
                    p3 = _dot3(R[:, i, 0], R[:, i, 1], R[:, i, 2], Pr2[:, 0, j], Pr2[:, 1, j], Pr2[:, 2, j])
                    nom = nom + (Pr1[:, i, j] * p3).astype(f64)
                    den = den + (p3 * p3).astype(f64)
            s12 = (nom / den).astype(f)
        inv_s = 1.0 / s12.astype(f64)
        t = np.empty((len(tr), 3), f)
        for i in range(3):
            t[:, i] = O1[:, i] - s12 * _dot3(R[:, i, 0], R[:, i, 1], R[:, i, 2], O2[:, 0], O2[:, 1], O2[:, 2])
        sR = (s12[:, None, None] * R).astype(f)
        sRi = (inv_s[:, None, None] * np.transpose(R, (0, 2, 1)).astype(f64)).astype(f)
        ti = np.empty((len(tr), 3), f)
        for i in range(3):
            ti[:, i] = -_dot3(sRi[:, i, 0], sRi[:, i, 1], sRi[:, i, 2], t[:, 0], t[:, 1], t[:, 2])
    return dict(R=R, t=t, s=s12, sR=sR, sRi=sRi, ti=ti)


def _image(X, K):
    invz = X.dtype.type(1) / X[..., 2]
    return K[0] * (X[..., 0] * invz) + K[2], K[1] * (X[..., 1] * invz) + K[3]


def _project(A, b, X, K):
    """A (H, 3, 3), b (H, 3), X (n, 3) -> u, v (H, n)"""
    Y = np.stack([_dot3(A[:, i, 0, None], A[:, i, 1, None], A[:, i, 2, None], X[None, :, 0], X[None, :, 1], X[None, :, 2]) + b[:, i, None]
                  for i in range(3)], -1)
    return _image(Y, K)


def errors(hyp, x1, x2, intr1, intr2, prec):
    """err1, err2 (H, n) of CheckInliers under every hypothesis."""
    f = np.float32 if prec == 32 else np.float64
    x1, x2, K1, K2 = np.asarray(x1, f), np.asarray(x2, f), np.asarray(intr1, f), np.asarray(intr2, f)
    with np.errstate(all="ignore"):
        u11, v11 = _image(x1, K1)
        u22, v22 = _image(x2, K2)
        u21, v21 = _project(hyp["sR"], hyp["t"], x2, K1)
        u12, v12 = _project(hyp["sRi"], hyp["ti"], x1, K2)
        d1x, d1y, d2x, d2y = u11[None] - u21, v11[None] - v21, u12 - u22[None], v12 - v22[None]
        return d1x * d1x + d1y * d1y, d2x * d2x + d2y * d2y


def evaluate(problem, prec):
    """Everything one device call returns, plus the errors: dict hyp, err1, err2, flags (H, n) bool, counts (H)."""
    hyp = compute_sim3(problem["x1"], problem["x2"], problem["triples"], problem["fix_scale"], prec)
    e1, e2 = errors(hyp, problem["x1"], problem["x2"], problem["intr1"], problem["intr2"], prec)
    f = e1.dtype.type
    with np.errstate(invalid="ignore"):
        flags = (e1 < np.asarray(problem["max_err1"], f)[None]) & (e2 < np.asarray(problem["max_err2"], f)[None])
    return dict(hyp=hyp, err1=e1, err2=e2, flags=flags, counts=flags.sum(1).astype(np.int32))


def distinct(triples):
    t = np.asarray(triples).reshape(-1, 3)
    return (t[:, 0] != t[:, 1]) & (t[:, 0] != t[:, 2]) & (t[:, 1] != t[:, 2])


def decided(problem, r32, r64):
    """The admissibility measure of a fixture: per hypothesis the float/double gap g_h = max_i |e32 - e64| / max(e64, thr) over both
    errors, and per (h, i) whether |e32 - thr| > 4 g_h max(e32, thr) holds for both errors.  -> (decided (H, n) bool, g (H))."""
    with np.errstate(all="ignore"):
        dec, g = None, np.zeros(len(r32["counts"]))
        pairs = [(r32["err1"].astype(f64), r64["err1"], np.asarray(problem["max_err1"], f64)[None]),
                 (r32["err2"].astype(f64), r64["err2"], np.asarray(problem["max_err2"], f64)[None])]
        for e32, e64, thr in pairs:
            rel = np.abs(e32 - e64) / np.maximum(e64, thr)
            rel = np.where(np.isfinite(rel), rel, np.inf)
            g = np.maximum(g, rel.max(1) if rel.shape[1] else 0)
        for e32, e64, thr in pairs:
            d = np.abs(e32 - thr) > 4 * g[:, None] * np.maximum(e32, thr)
            dec = d if dec is None else dec & d
    return dec, g


# ---- host logic ----------------------------------------------------------------------------------------------------------

def sample_triples(N, count, rand_int):
    """Line by line :163-177.  vAvailableIndices[idx] = back() indexes by the value drawn, not by randi: a value can repeat."""
    out = []
    for _ in range(count):
        vAvailableIndices = list(range(N))   # the vector's storage: pop_back() only lowers `size`, the capacity stays N
        size = N
        tri = []
        for _i in range(3):
            randi = rand_int(0, size - 1)
            idx = vAvailableIndices[randi]
            tri.append(idx)
            vAvailableIndices[idx] = vAvailableIndices[size - 1]   # idx may be >= size: a store into an already popped slot, never read again
            size -= 1
        out.append(tri)
    return np.array(out, np.int32).reshape(-1, 3)


def ransac_iterations(N, probability, minInliers, maxIterations):
    """mRansacMaxIts after SetRansacParameters (:114-138)."""
    with np.errstate(all="ignore"):
        epsilon = np.float32(minInliers) / np.float32(N)          # float epsilon = (float)mRansacMinInliers/N
        if minInliers == N:
            nIterations = 1
        else:
            v = math.log(1 - probability) / np.log(f64(1) - math.pow(float(epsilon), 3))
            v = np.ceil(v)
            nIterations = int(v) if np.isfinite(v) and abs(v) < 2 ** 31 else -2 ** 31   # what (int) gives on x86-64
    return max(1, min(nIterations, maxIterations))


class Scan:
    """iterate() (:140-207) over precomputed per-hypothesis counts."""

    def __init__(self, N, counts, minInliers, maxIts):
        self.N, self.counts, self.minInliers, self.maxIts = N, counts, minInliers, maxIts
        self.mnIterations, self.mnBestInliers, self.best = 0, 0, -1

    def iterate(self, nIterations):
        """-> (accepted hypothesis or -1, bNoMore, nInliers)"""
        if self.N < self.minInliers:
            return -1, True, 0
        nCurrentIterations = 0
        while self.mnIterations < self.maxIts and nCurrentIterations < nIterations:
            nCurrentIterations += 1
            h = self.mnIterations
            self.mnIterations += 1
            if self.counts[h] >= self.mnBestInliers:
                self.mnBestInliers, self.best = int(self.counts[h]), h
                if self.counts[h] > self.minInliers:
                    return h, False, int(self.counts[h])
        return -1, self.mnIterations >= self.maxIts, 0


def run_scan(N, counts, minInliers, maxIts, chunk):
    """Calls iterate(chunk) until a hypothesis is accepted or bNoMore: -> (accepted, nInliers, [bNoMore of every call], best)."""
    s, trace = Scan(N, counts, minInliers, maxIts), []
    while True:
        h, no_more, nin = s.iterate(chunk)
        trace.append(bool(no_more))
        if h >= 0 or no_more:
            return h, nin, trace, s.best


# ---- fixtures ------------------------------------------------------------------------------------------------------------
# (n, outlier_frac, fix_scale, n_hyp, seed): n from 20 to 600, ragged; outlier fractions 0 .. 0.6; both scale modes; 1, 5 and 300
# hypotheses.  The seeds were chosen on the CPU so that the restatement alone meets the admissibility conditions that
# tests/test_sim3_ransac_ref.py asserts; nothing here has seen a device result.  minInliers is three quarters of the expected true matches.
FIXTURES = [
    (20, 0.0, True, 300, 100), (33, 0.1, False, 300, 110), (50, 0.2, True, 5, 120), (64, 0.3, False, 300, 130),
    (65, 0.4, True, 300, 140), (100, 0.5, False, 1, 165), (128, 0.6, True, 300, 160), (150, 0.0, False, 300, 170),
    (200, 0.3, False, 300, 180), (257, 0.2, True, 300, 190), (300, 0.6, False, 300, 200), (350, 0.1, True, 5, 210),
    (400, 0.4, False, 300, 220), (480, 0.5, True, 300, 230), (555, 0.3, False, 1, 249), (600, 0.6, False, 300, 250),
]
NOISE_PX = 0.5


def scripted_rand(seed, count=4096):
    """A RandomInt source over a fixed stream of 32-bit values: RandomInt(lo, hi) = lo + u[k] % (hi - lo + 1)."""
    u = np.random.RandomState(77000 + seed).randint(0, 2 ** 31, count).astype(np.uint32)
    pos = [0]

    def rand_int(lo, hi):
        v = int(u[pos[0]]) if pos[0] < len(u) else 0
        pos[0] += 1
        return lo + v % (hi - lo + 1)
    return rand_int, u


def min_inliers(n, outlier_frac):
    return max(6, int(0.75 * (1.0 - outlier_frac) * n))


def fixture(k):
    """Fixture k: the synthesized problem with its n_hyp triples from the reference's sampler, and its RANSAC parameters."""
    from weiner_slamit_v2_amd import synth
    n, of, fix, nh, seed = FIXTURES[k]
    pr = synth.synth_sim3_ransac(n, of, seed, NOISE_PX, fix)
    rand_int, _ = scripted_rand(seed)
    pr["triples"] = sample_triples(n, nh, rand_int)
    pr["min_inliers"] = min_inliers(n, of)
    pr["max_its"] = ransac_iterations(n, 0.99, pr["min_inliers"], nh)
    pr["seed"] = seed
    return pr


def admissibility(pr):
    """-> dict of what the admissibility conditions are stated on (r32, r64, decided, distinct, the two scans)."""
    r32, r64 = evaluate(pr, 32), evaluate(pr, 64)
    dec, g = decided(pr, r32, r64)
    d = distinct(pr["triples"])
    n = len(pr["max_err1"])
    s32 = run_scan(n, r32["counts"], pr["min_inliers"], pr["max_its"], 5)
    s64 = run_scan(n, r64["counts"], pr["min_inliers"], pr["max_its"], 5)
    und = float((~dec[d]).mean()) if d.any() else 0.0
    # every hypothesis the scan records as best on its way (a prefix maximum under >=) or accepts
    seen, best, stop = [], 0, s32[0] if s32[0] >= 0 else pr["max_its"] - 1
    for h in range(min(stop + 1, len(r32["counts"]))):
        if r32["counts"][h] >= best:
            best = int(r32["counts"][h])
            seen.append(h)
    return dict(r32=r32, r64=r64, decided=dec, g=g, distinct=d, scan32=s32, scan64=s64, undecided_frac=und, recorded=seen)


def admissible(a):
    return (a["undecided_frac"] <= 0.02 and a["scan32"][:2] == a["scan64"][:2] and a["scan32"][0] >= 0
            and all(a["decided"][h].all() for h in a["recorded"]))
