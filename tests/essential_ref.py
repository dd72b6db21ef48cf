"""Numpy restatement of Optimizer::OptimizeEssentialGraph (ORB_SLAM2/src/Optimizer.cc:781-1044) with the g2o it instantiates, on
the arrays of include/slamit.h's slamit_eg_problem: Sim3 exp / log with every branch of Thirdparty/g2o/g2o/types/sim3.h, EdgeSim3's
error log(C * Si * Sj^-1), g2o's central-difference Jacobians (core/base_binary_edge.hpp:131-200, delta 1e-9, fixed vertices
skipped), the quadratic form summed edge by edge in list order, a dense solve of (H + lambda I) x = b, the Levenberg rules of
core/optimization_algorithm_levenberg.cpp:61-164 (the fork's three-bad-iterations stop included), and the recovery of the poses and
points.  Everything is batched over a leading axis, so a 1,024-keyframe chain linearises in one pass.

A Sim3 is (q, t, s): q = (x, y, z, w) as Eigen stores a Quaterniond, never normalised (g2o does not normalise either).

Also here: plan_edges(), the literal restatement of :847-983 (the choice of edges) that csrc/essential_plan.cc is tested against.
"""
import numpy as np

LM_MAX_TRIALS = 10
DBL_MAX = np.finfo(np.float64).max
EG_NORMAL, EG_LOOP_CONNECTION = 0, 1


# ---- quaternions as Eigen has them --------------------------------------------------------------------------------------------
def qmul(a, b):
    ax, ay, az, aw = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bx, by, bz, bw = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bx + ax * bw + ay * bz - az * by,
                     aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx,
                     aw * bw - ax * bx - ay * by - az * bz], -1)


def qrot(q, v):
    qv = q[..., :3]
    uv = 2 * np.cross(qv, v)
    return v + q[..., 3:4] * uv + np.cross(qv, uv)


def qconj(q):
    return q * np.array([-1.0, -1.0, -1.0, 1.0])


def q2R(q):
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    R = np.stack([1 - (tyy + tzz), txy - twz, txz + twy,
                  txy + twz, 1 - (txx + tzz), tyz - twx,
                  txz - twy, tyz + twx, 1 - (txx + tyy)], -1)
    return R.reshape(q.shape[:-1] + (3, 3))


def R2q(R):
    """Quaterniond(R): Eigen's four branches, chosen per matrix."""
    R = np.asarray(R, np.float64)
    m = lambda i, j: R[..., i, j]
    tr = m(0, 0) + m(1, 1) + m(2, 2)
    out = np.zeros(R.shape[:-2] + (4,))
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.sqrt(tr + 1.0)
        h = 0.5 / t
        pos = np.stack([(m(2, 1) - m(1, 2)) * h, (m(0, 2) - m(2, 0)) * h, (m(1, 0) - m(0, 1)) * h, 0.5 * t], -1)
        i = np.where(m(1, 1) > m(0, 0), 1, 0)
        mii = np.where(i == 1, m(1, 1), m(0, 0))
        i = np.where(m(2, 2) > mii, 2, i)
        sel = tr > 0
        out[sel] = pos[sel]
        for I in range(3):
            J, K = (I + 1) % 3, (I + 2) % 3
            t = np.sqrt(m(I, I) - m(J, J) - m(K, K) + 1.0)
            h = 0.5 / t
            c = np.zeros_like(out)
            c[..., I] = 0.5 * t
            c[..., 3] = (m(K, J) - m(J, K)) * h
            c[..., J] = (m(J, I) + m(I, J)) * h
            c[..., K] = (m(K, I) + m(I, K)) * h
            s = (~sel) & (i == I)
            out[s] = c[s]
    return out


def skew(w):
    z = np.zeros_like(w[..., 0])
    return np.stack([z, -w[..., 2], w[..., 1], w[..., 2], z, -w[..., 0], -w[..., 1], w[..., 0], z], -1).reshape(w.shape[:-1] + (3, 3))


# ---- Sim3 (sim3.h) ------------------------------------------------------------------------------------------------------------
def sim3_mul(a, b):
    (qa, ta, sa), (qb, tb, sb) = a, b
    return qmul(qa, qb), sa[..., None] * qrot(qa, tb) + ta, sa * sb


def sim3_inv(a):
    q, t, s = a
    qc = qconj(q)
    return qc, qrot(qc, (-1.0 / s)[..., None] * t), 1.0 / s


def sim3_map(a, x):
    q, t, s = a
    return s[..., None] * qrot(q, x) + t


def _abc(sigma, s, theta, small_theta):
    """A, B, C of sim3.h's exp and log (the same four branches in both)."""
    eps = 0.00001
    small_sigma = np.abs(sigma) < eps
    with np.errstate(invalid="ignore", divide="ignore"):
        theta2, sigma2 = theta * theta, sigma * sigma
        C = np.where(small_sigma, 1.0, (s - 1) / sigma)
        A00, B00 = 0.5, 1.0 / 6.0
        A01 = (1 - np.cos(theta)) / theta2
        B01 = (theta - np.sin(theta)) / (theta2 * theta)
        A10 = ((sigma - 1) * s + 1) / sigma2
        B10 = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma)
        a, b, c = s * np.sin(theta), s * np.cos(theta), theta2 + sigma2
        A11 = (a * sigma + (1 - b) * theta) / (theta * c)
        B11 = (C - ((b - 1) * sigma + a * theta) / c) * 1.0 / theta2
    A = np.where(small_sigma, np.where(small_theta, A00, A01), np.where(small_theta, A10, A11))
    B = np.where(small_sigma, np.where(small_theta, B00, B01), np.where(small_theta, B10, B11))
    return A, B, C


# the two small-angle tests, named so that tests/test_sim3_probes_ref.py can swap them: exp asks theta, log asks d = (tr R - 1) / 2
def exp_small(theta):
    return theta < 0.00001


def log_small(d, theta):
    return d > 1 - 0.00001


def sim3_exp(u):
    """Sim3(const Vector7d& update), sim3.h:70-142."""
    u = np.asarray(u, np.float64)
    omega, ups, sigma = u[..., :3], u[..., 3:6], u[..., 6]
    theta = np.sqrt((omega * omega).sum(-1))
    O = skew(omega)
    O2 = O @ O
    s = np.exp(sigma)
    small = exp_small(theta)
    A, B, C = _abc(sigma, s, theta, small)
    I = np.eye(3)
    with np.errstate(invalid="ignore", divide="ignore"):
        ca = np.where(small, 1.0, np.sin(theta) / theta)
        cb = np.where(small, 1.0, (1 - np.cos(theta)) / (theta * theta))
    R = I + ca[..., None, None] * O + cb[..., None, None] * O2
    W = A[..., None, None] * O + B[..., None, None] * O2 + C[..., None, None] * I
    return R2q(R), (W @ ups[..., None])[..., 0], s


def sim3_log(a):
    """Sim3::log(), sim3.h:148-230."""
    q, t, s = a
    sigma = np.log(s)
    R = q2R(q)
    d = 0.5 * (R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2] - 1)
    dR = np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], -1)
    with np.errstate(invalid="ignore", divide="ignore"):
        theta = np.arccos(d)
        small = log_small(d, theta)
        k = np.where(small, 0.5, theta / (2 * np.sqrt(1 - d * d)))
    omega = k[..., None] * dR
    A, B, C = _abc(sigma, s, theta, small)
    O = skew(omega)
    W = A[..., None, None] * O + B[..., None, None] * (O @ O) + C[..., None, None] * np.eye(3)
    ups = np.linalg.solve(W, t[..., None])[..., 0]
    return np.concatenate([omega, ups, sigma[..., None]], -1)


def sim3_oplus(a, u, fix_scale):
    """VertexSim3Expmap::oplusImpl: estimate <- Sim3(update) * estimate, update[6] zeroed under _fix_scale."""
    u = np.array(u, np.float64)
    if fix_scale:
        u[..., 6] = 0
    return sim3_mul(sim3_exp(u), a)


def from_rts(r, t, s):
    return R2q(np.asarray(r, np.float64).reshape(-1, 3, 3)), np.asarray(t, np.float64).reshape(-1, 3).copy(), np.asarray(s, np.float64).reshape(-1).copy()


def _take(a, idx):
    return a[0][idx], a[1][idx], a[2][idx]


# ---- the optimisation ------------------------------------------------------------------------------------------------------------
def measurements(prob):
    scw = from_rts(prob["scw_r"], prob["scw_t"], prob["scw_s"])
    snc = from_rts(prob["snc_r"], prob["snc_t"], prob["snc_s"])
    v0, v1, kind = prob["edge_v0"], prob["edge_v1"], np.asarray(prob["edge_kind"])
    mc = sim3_mul(_take(scw, v1), sim3_inv(_take(scw, v0)))
    mn = sim3_mul(_take(snc, v1), sim3_inv(_take(snc, v0)))
    lc = kind == EG_LOOP_CONNECTION
    return np.where(lc[:, None], mc[0], mn[0]), np.where(lc[:, None], mc[1], mn[1]), np.where(lc, mc[2], mn[2])


def edge_errors(meas, est, v0, v1):
    return sim3_log(sim3_mul(sim3_mul(meas, _take(est, v0)), sim3_inv(_take(est, v1))))


def linearize(meas, est, v0, v1, fix_scale):
    """J0, J1 [E, 7, 7]: column d = (1 / 2e-9) * (e(+delta on d) - e(-delta on d)) on vertex 0 / vertex 1."""
    E = len(v0)
    delta, scalar = 1e-9, 1.0 / (2 * 1e-9)
    J = []
    for side in (0, 1):
        Js = np.zeros((E, 7, 7))
        for d in range(7):
            ee = []
            for sg in (delta, -delta):
                u = np.zeros((E, 7))
                u[:, d] = sg
                a, b = _take(est, v0), _take(est, v1)
                if side == 0:
                    a = sim3_oplus(a, u, fix_scale)
                else:
                    b = sim3_oplus(b, u, fix_scale)
                ee.append(sim3_log(sim3_mul(sim3_mul(meas, a), sim3_inv(b))))
            Js[:, :, d] = scalar * (ee[0] - ee[1])
        J.append(Js)
    return J


def optimize(prob, record=None):
    """Returns the result arrays of slamit_eg_result (a dict), with `trial_rho` / `trial_chi2` / `trial_lambda` beside them."""
    n = int(prob["n_kf"])
    fix_scale = bool(prob["fix_scale"])
    v0, v1 = np.asarray(prob["edge_v0"], np.int64), np.asarray(prob["edge_v1"], np.int64)
    E = len(v0)
    fixed = np.asarray(prob["fixed"]).astype(bool) | np.asarray(prob["bad"]).astype(bool)
    free = np.flatnonzero(~fixed)
    blk = -np.ones(n, np.int64)
    blk[free] = np.arange(len(free))
    N = 7 * len(free)
    scw = from_rts(prob["scw_r"], prob["scw_t"], prob["scw_s"])
    est = (scw[0].copy(), scw[1].copy(), scw[2].copy())
    meas = measurements(prob) if E else None
    lam, ni, nbad, chi2_init = float(prob["lambda_init"]), 2.0, 0, 0.0
    its_chi2, its_lambda, its_trials, t_rho, t_chi2, t_lambda = [], [], [], [], [], []

    def chi2_of(e):
        c = 0.0
        for v in (e * e).sum(-1):   # activeRobustChi2: edge by edge
            c += v
        return c

    for it in range(int(prob["max_its"])):
        if N == 0 or E == 0:
            break
        e = edge_errors(meas, est, v0, v1)
        cur = chi2_of(e)
        ini = cur
        if it == 0:
            chi2_init = cur
        J0, J1 = linearize(meas, est, v0, v1, fix_scale)
        H, b = np.zeros((N, N)), np.zeros(N)
        for k in range(E):   # constructQuadraticForm, edge by edge in list order
            a, c = blk[v0[k]], blk[v1[k]]
            if a >= 0:
                b[7 * a:7 * a + 7] += J0[k].T @ -e[k]
                H[7 * a:7 * a + 7, 7 * a:7 * a + 7] += J0[k].T @ J0[k]
            if c >= 0:
                b[7 * c:7 * c + 7] += J1[k].T @ -e[k]
                H[7 * c:7 * c + 7, 7 * c:7 * c + 7] += J1[k].T @ J1[k]
            if a >= 0 and c >= 0:
                H[7 * a:7 * a + 7, 7 * c:7 * c + 7] += J0[k].T @ J1[k]
                H[7 * c:7 * c + 7, 7 * a:7 * a + 7] += J1[k].T @ J0[k]
        qmax, rho = 0, 0.0
        while True:
            try:
                A = H.copy()
                A[np.diag_indices(N)] += lam
                x = np.linalg.solve(A, b)
                ok2 = bool(np.all(np.isfinite(x)))
            except np.linalg.LinAlgError:
                x, ok2 = np.zeros(N), False
            if fix_scale:
                x[6::7] = 0
            trial = (est[0].copy(), est[1].copy(), est[2].copy())
            upd = sim3_oplus(_take(est, free), x.reshape(-1, 7), fix_scale)
            for c in range(3):
                trial[c][free] = upd[c]
            last = chi2_of(edge_errors(meas, trial, v0, v1))
            temp = last if ok2 else DBL_MAX
            scale = 0.0
            for j in range(N):
                scale += x[j] * (lam * x[j] + b[j])
            rho = (cur - temp) / (scale + 1e-3)
            t_lambda.append(lam)
            if rho > 0 and np.isfinite(temp):
                alpha = min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0)
                lam *= max(1.0 / 3.0, alpha)
                ni = 2.0
                cur = temp
                est = trial
            else:
                lam *= ni
                ni *= 2
            qmax += 1
            t_rho.append(rho)
            t_chi2.append(last)
            if not (rho < 0 and qmax < LM_MAX_TRIALS):
                break
        its_chi2.append(last)
        its_lambda.append(lam)
        its_trials.append(qmax)
        if qmax == LM_MAX_TRIALS or rho == 0:
            break
        nbad = nbad + 1 if (ini - cur) * 1e3 < ini else 0
        if nbad >= 3:
            break
    out = recover(prob, est)
    out.update(n_its=len(its_chi2), chi2_init=chi2_init, chi2=np.array(its_chi2), lam=np.array(its_lambda), trials=np.array(its_trials, np.int32),
               trial_rho=np.array(t_rho), trial_chi2=np.array(t_chi2), trial_lambda=np.array(t_lambda))
    return out


def cost(prob, sim3_r, sim3_t, sim3_s):
    """chi2 of GIVEN estimates (r, t, s per keyframe) over the problem's edges: one yardstick for results of different implementations"""
    est = from_rts(sim3_r, sim3_t, sim3_s)
    e = edge_errors(measurements(prob), est, np.asarray(prob["edge_v0"], np.int64), np.asarray(prob["edge_v1"], np.int64))
    return float((e * e).sum())


def recover(prob, est):
    """:991-1043 — [R | t / s] per keyframe, and corrected.inverse().map(Scw.map(X)) per good point, narrowed to float."""
    n = int(prob["n_kf"])
    R = q2R(est[0])
    pose = np.concatenate([R.reshape(n, 9), est[1] * (1.0 / est[2])[:, None]], 1)
    out = dict(sim3_r=R.reshape(n, 9), sim3_t=est[1].copy(), sim3_s=est[2].copy(), pose=pose)
    out["points"], out["touched"] = map_points(prob, out["sim3_r"], out["sim3_t"], out["sim3_s"])
    return out


def map_points(prob, sim3_r, sim3_t, sim3_s):
    """The point map restated on GIVEN corrected Sim3s (r, t, s as the result holds them)."""
    pos = np.asarray(prob["pt_pos"], np.float32).reshape(-1, 3)
    ref = np.asarray(prob["pt_ref"], np.int64)
    good = ~np.asarray(prob["pt_bad"]).astype(bool)
    scw = from_rts(prob["scw_r"], prob["scw_t"], prob["scw_s"])
    cor = from_rts(sim3_r, sim3_t, sim3_s)
    pts = pos.copy()
    g = np.flatnonzero(good)
    if len(g):
        x = sim3_map(_take(scw, ref[g]), pos[g].astype(np.float64))
        pts[g] = sim3_map(sim3_inv(_take(cor, ref[g])), x).astype(np.float32)
    return pts, g.astype(np.int32)


# ---- the choice of edges, Optimizer.cc:847-983, literally ----------------------------------------------------------------------------
def plan_edges(g):
    """g: kf_bad, kf_id, kf_parent (slot or -1), children (list of slot lists), loop_edges (list of slot lists), covis (list of
    (slot, weight) rows ordered as mvpOrderedConnectedKeyFrames), loop_connections ({slot: [slots]}: walked in ascending slot, each set
    in ascending slot), loop_kf, cur_kf, min_feat.  Returns [(v0, v1, kind)] in insertion order."""
    n = len(g["kf_bad"])
    kid = g["kf_id"]
    edges, inserted = [], set()
    weight = lambda i, j: dict(g["covis"][i]).get(j, 0)   # KeyFrame::GetWeight
    for i in sorted(g["loop_connections"]):
        for j in sorted(g["loop_connections"][i]):
            if (kid[i] != kid[g["cur_kf"]] or kid[j] != kid[g["loop_kf"]]) and weight(i, j) < g["min_feat"]:
                continue
            edges.append((i, j, EG_LOOP_CONNECTION))
            inserted.add((min(kid[i], kid[j]), max(kid[i], kid[j])))
    for i in range(n):
        if g["kf_bad"][i]:
            continue   # (vpKFs holds no bad keyframe: Map::EraseKeyFrame)
        par = g["kf_parent"][i]
        if par >= 0:
            edges.append((i, par, EG_NORMAL))
        le = sorted(g["loop_edges"][i])
        for l in le:
            if kid[l] < kid[i]:
                edges.append((i, l, EG_NORMAL))
        # KeyFrame::GetCovisiblesByWeight (KeyFrame.cc:188-203): the ordered row up to the first weight below minFeat -- and NOTHING
        # when no weight of the row is below it (upper_bound returns end(), which the reference takes for "none")
        row = g["covis"][i]
        cut = next((k for k, (_, w) in enumerate(row) if g["min_feat"] > w), None)
        for j, w in (row[:cut] if cut is not None else []):
            if j != par and j not in g["children"][i] and j not in le:
                if not g["kf_bad"][j] and kid[j] < kid[i]:
                    if (min(kid[i], kid[j]), max(kid[i], kid[j])) in inserted:
                        continue
                    edges.append((i, j, EG_NORMAL))
    return edges
