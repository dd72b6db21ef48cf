"""Deterministic synthetic inputs for the hot path.

Frames: 3-octave value noise + high-contrast axis-aligned / rotated rectangles and checker
patches + uniform noise, so every pyramid level holds far more FAST-20 corners than its quota
and some cells need the FAST-7 fallback.  Everything is drawn from numpy's frozen legacy
MT19937 stream (RandomState) and built from exact float64 elementwise arithmetic, so the same
seed gives the same bytes on any host.

BA windows: the 50-keyframe x 2000-point problem of SURVEY.md §8d (arc trajectory, reference
intrinsics of Tracking.cc:77-80, float32-rounded inputs widened to float64 the way
Converter.cc:37-47,110-116 does).
"""
import numpy as np

FRAME_SEED = 0xC0FFEE


def _value_noise(rs, h, w, cell, amp):
    gh, gw = h // cell + 2, w // cell + 2
    g = rs.uniform(-1.0, 1.0, size=(gh, gw))
    ys = np.arange(h, dtype=np.float64) / cell
    xs = np.arange(w, dtype=np.float64) / cell
    y0 = np.floor(ys).astype(np.int64)
    x0 = np.floor(xs).astype(np.int64)
    fy = (ys - y0)[:, None]
    fx = (xs - x0)[None, :]
    a = g[y0][:, x0]
    b = g[y0][:, x0 + 1]
    c = g[y0 + 1][:, x0]
    d = g[y0 + 1][:, x0 + 1]
    return amp * ((a * (1 - fx) + b * fx) * (1 - fy) + (c * (1 - fx) + d * fx) * fy)


def synth_frame(width, height, index=0, n_shapes=None, seed=FRAME_SEED, scene="rich"):
    """uint8 (height, width) frame number `index`.  scene "rich" (every test, the benchmarks' default): value noise down to
    4-pixel cells plus 400 hard-edged shapes per VGA frame -- about one pixel in eight is a FAST corner at threshold 20;
    "sparse": the same construction without the 4-pixel noise level and with 150 shapes -- a few percent of corners, closer
    to indoor video (bench.py --scene sparse reports how the FAST pass depends on it)."""
    rs = np.random.RandomState((seed + index) & 0x7FFFFFFF)
    img = np.full((height, width), 128.0)
    sparse = scene == "sparse"
    for cell, amp in (((64, 64.0), (16, 16.0)) if sparse else ((64, 64.0), (16, 32.0), (4, 16.0))):
        img += _value_noise(rs, height, width, cell, amp)
    if n_shapes is None:
        n_shapes = int(round((150.0 if sparse else 400.0) * (width * height) / (640.0 * 480.0)))
    yy, xx = np.mgrid[0:height, 0:width]
    for _ in range(n_shapes):
        kind = rs.randint(0, 3)
        cx, cy = rs.randint(0, width), rs.randint(0, height)
        sw, sh = rs.randint(6, 41), rs.randint(6, 41)
        delta = float(rs.randint(60, 121)) * (1.0 if rs.randint(0, 2) else -1.0)
        x0, x1 = max(cx - 30, 0), min(cx + 31, width)
        y0, y1 = max(cy - 30, 0), min(cy + 31, height)
        lx = (xx[y0:y1, x0:x1] - cx).astype(np.float64)
        ly = (yy[y0:y1, x0:x1] - cy).astype(np.float64)
        if kind == 0:  # axis-aligned rectangle
            m = (np.abs(lx) * 2 <= sw) & (np.abs(ly) * 2 <= sh)
            img[y0:y1, x0:x1] += delta * m
        elif kind == 1:  # rotated rectangle
            th = rs.uniform(0.0, np.pi)
            c, s = np.cos(th), np.sin(th)
            u, v = c * lx + s * ly, -s * lx + c * ly
            m = (np.abs(u) * 2 <= sw) & (np.abs(v) * 2 <= sh)
            img[y0:y1, x0:x1] += delta * m
        else:  # 2x2 checker patch
            m = (np.abs(lx) * 2 <= sw) & (np.abs(ly) * 2 <= sh)
            sign = np.where((lx >= 0) ^ (ly >= 0), 1.0, -1.0)
            img[y0:y1, x0:x1] += delta * m * sign
    img += rs.randint(-2, 3, size=(height, width)) if sparse else rs.randint(-4, 5, size=(height, width))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def warp_frame(frame, index=0, seed=FRAME_SEED):
    """Frame B = frame A under a known similarity (rot +-10 deg, scale 0.9-1.1, shift <= 20 px),
    nearest-neighbour sampled with integer-exact index maps, + noise +-2."""
    h, w = frame.shape
    rs = np.random.RandomState((seed ^ 0x5EED) + index)
    ang = rs.uniform(-10.0, 10.0) * np.pi / 180.0
    sc = rs.uniform(0.9, 1.1)
    tx, ty = rs.uniform(-20, 20, size=2)
    yy, xx = np.mgrid[0:h, 0:w]
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    c, s = np.cos(ang) / sc, np.sin(ang) / sc
    sx = c * (xx - cx - tx) + s * (yy - cy - ty) + cx
    sy = -s * (xx - cx - tx) + c * (yy - cy - ty) + cy
    ix = np.clip(np.rint(sx).astype(np.int64), 0, w - 1)
    iy = np.clip(np.rint(sy).astype(np.int64), 0, h - 1)
    out = frame[iy, ix].astype(np.int64) + rs.randint(-2, 3, size=(h, w))
    return np.clip(out, 0, 255).astype(np.uint8)


def synth_stereo_pair(width, height, index=0, d_min=2.0, d_max=None, seed=FRAME_SEED):
    """A rectified pair for Frame::ComputeStereoMatches: left = synth_frame(width, height, index); right(x, y) = left(x + d(x, y), y)
    with a smooth disparity field d in [d_min, d_max] (d_max: width / 16), linearly interpolated along the row, + noise +-1.
    -> (left, right, d): a left column uL reappears near uR = uL - d in the right image."""
    left = synth_frame(width, height, index, seed=seed)
    rs = np.random.RandomState(((seed ^ 0x57E7E0) + index) & 0x7FFFFFFF)
    if d_max is None:
        d_max = width / 16.0
    d = d_min + (d_max - d_min) * (0.5 + 0.5 * np.clip(_value_noise(rs, height, width, 96, 1.0), -1.0, 1.0))
    sx = np.arange(width, dtype=np.float64)[None, :] + d
    x0 = np.floor(sx)
    fx = sx - x0
    i0 = np.clip(x0.astype(np.int64), 0, width - 1)
    i1 = np.clip(i0 + 1, 0, width - 1)
    rows = np.arange(height)[:, None]
    L = left.astype(np.float64)
    right = L[rows, i0] * (1.0 - fx) + L[rows, i1] * fx + rs.randint(-1, 2, size=(height, width))
    return left, np.ascontiguousarray(np.clip(np.rint(right), 0, 255).astype(np.uint8)), d


def synth_batch(width, height, n, first=0, seed=FRAME_SEED):
    return np.stack([synth_frame(width, height, first + i, seed=seed) for i in range(n)])


def flat_frame(width, height, value=90):
    return np.full((height, width), value, dtype=np.uint8)


def noise_frame(width, height, seed=1):
    return np.random.RandomState(seed).randint(0, 256, size=(height, width)).astype(np.uint8)


# ---------------------------------------------------------------------------------------------
# Bundle-adjustment windows
# ---------------------------------------------------------------------------------------------

INTRINSICS = (526.69, 540.36, 313.07, 238.39)  # Tracking.cc:77-80


def _hat(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype=np.float64)


def se3_exp(xi):
    """xi = [omega(3), upsilon(3)] -> (R, t), same closed form as g2o SE3Quat::exp."""
    w, u = np.asarray(xi[:3], float), np.asarray(xi[3:], float)
    th = np.linalg.norm(w)
    W = _hat(w)
    if th < 1e-5:
        R = np.eye(3) + W + W @ W
        V = R
    else:
        W2 = W @ W
        R = np.eye(3) + np.sin(th) / th * W + (1 - np.cos(th)) / th ** 2 * W2
        V = np.eye(3) + (1 - np.cos(th)) / th ** 2 * W + (th - np.sin(th)) / th ** 3 * W2
    return R, V @ u


def _inv_sigma2_table(nlevels=8, scale=1.2):
    s = np.float32(1.0)
    out = []
    for _ in range(nlevels):
        out.append(np.float32(1.0) / (s * s))
        s = np.float32(s * np.float64(np.float32(scale)))
    return np.array(out, dtype=np.float32)


def synth_ba(n_kf=50, n_pt=2000, obs_per_pt=8, outlier_frac=0.03, seed=12345, n_fixed=1, stereo_frac=0.0, baseline=0.08):
    """Returns a dict of numpy arrays laid out as include/slamit.h:slamit_ba_problem wants them.

    obs_per_pt = None or >= n_kf gives the dense pattern (every point in every keyframe).
    stereo_frac > 0: that fraction of the observations also carries the keypoint's column in the right image (edge_ur; -1 on the
    monocular ones, KeyFrame::mvuRight) and the dict gains kf_bf = baseline x fx per keyframe (KeyFrame::mbf): the window of a
    stereo / RGB-D session, Optimizer.cc:621-650.  The monocular arrays do not depend on stereo_frac (own random stream)."""
    rs = np.random.RandomState(seed)
    fx, fy, cx, cy = INTRINSICS
    Rs, ts = [], []
    for k in range(n_kf):
        R, t = se3_exp([0.0, 0.02 * k, 0.0, -0.1 * k, 0.0, 0.0])
        Rs.append(R)
        ts.append(t)
    pts = np.stack([rs.uniform(0.5, 4.5, n_pt), rs.uniform(-1.5, 1.5, n_pt), rs.uniform(4.0, 8.0, n_pt)], 1)
    dense = obs_per_pt is None or obs_per_pt >= n_kf
    inv_sig = _inv_sigma2_table()
    quota = np.array([217, 181, 151, 126, 105, 87, 73, 60], dtype=np.float64)
    quota /= quota.sum()
    e_kf, e_pt, e_uv, e_is, e_ur = [], [], [], [], []
    rs2 = np.random.RandomState(seed + 777)
    bf = float(np.float32(baseline * fx))
    for p in range(n_pt):
        if dense:
            kfs = range(n_kf)
        else:
            start = rs.randint(0, n_kf - obs_per_pt + 1)
            kfs = range(start, start + obs_per_pt)
        for k in kfs:
            Xc = Rs[k] @ pts[p] + ts[k]
            u = fx * Xc[0] / Xc[2] + cx + rs.normal(0.0, 1.0)
            v = fy * Xc[1] / Xc[2] + cy + rs.normal(0.0, 1.0)
            if rs.uniform() < outlier_frac:
                u += rs.choice([-30.0, 30.0])
                v += rs.choice([-30.0, 30.0])
            octave = rs.choice(8, p=quota)
            e_kf.append(k)
            e_pt.append(p)
            e_uv.append((u, v))
            e_is.append(inv_sig[octave])
            if stereo_frac > 0:
                ur = u - bf / Xc[2] + rs2.normal(0.0, 1.0)
                if rs2.uniform() < outlier_frac:
                    ur += rs2.choice([-20.0, 20.0])
                e_ur.append(ur if rs2.uniform() < stereo_frac else -1.0)
    # perturbed initial estimates, rounded to float32 then widened (Converter.cc)
    poses = np.zeros((n_kf, 12))
    for k in range(n_kf):
        if k < n_fixed:
            R, t = Rs[k], ts[k]
        else:
            dR, dt = se3_exp(rs.normal(0.0, 0.005, 6))
            R, t = dR @ Rs[k], dR @ ts[k] + dt
        poses[k, :9] = R.reshape(-1)
        poses[k, 9:] = t
    poses = poses.astype(np.float32).astype(np.float64)
    pts0 = (pts + rs.normal(0.0, 0.02, pts.shape)).astype(np.float32).astype(np.float64)
    fixed = np.zeros(n_kf, dtype=np.uint8)
    fixed[:n_fixed] = 1
    intr = np.tile(np.array([fx, fy, cx, cy], dtype=np.float32).astype(np.float64), (n_kf, 1))
    extra = {}
    if stereo_frac > 0:
        extra = {"edge_ur": np.array(e_ur, dtype=np.float32).astype(np.float64), "kf_bf": np.full(n_kf, bf)}
    return {
        **extra,
        "kf_pose": np.ascontiguousarray(poses),
        "kf_fixed": fixed,
        "kf_intr": np.ascontiguousarray(intr),
        "pt_xyz": np.ascontiguousarray(pts0),
        "edge_kf": np.array(e_kf, dtype=np.int32),
        "edge_pt": np.array(e_pt, dtype=np.int32),
        "edge_uv": np.array(e_uv, dtype=np.float32).astype(np.float64),
        "edge_inv_sigma2": np.array(e_is, dtype=np.float32).astype(np.float64),
        "truth_pose": np.array([np.concatenate([Rs[k].reshape(-1), ts[k]]) for k in range(n_kf)]),
        "truth_pt": pts,
    }


def synth_pose(n=400, outlier_frac=0.15, seed=7, perturb=0.02, stereo_frac=0.0, baseline=0.08):
    """One PoseOptimization problem (Optimizer.cc:239-451): n map points seen by one frame, pixel
    noise N(0,1), a fraction of gross outliers, initial pose = truth perturbed by exp(N(0, perturb^2)).
    All inputs float32-rounded then widened, as the reference feeds them."""
    rs = np.random.RandomState(seed)
    fx, fy, cx, cy = INTRINSICS
    R, t = se3_exp([0.05, -0.1, 0.02, 0.3, -0.1, 0.2])
    pts_c = np.stack([rs.uniform(-2.5, 2.5, n), rs.uniform(-1.8, 1.8, n), rs.uniform(3.0, 9.0, n)], 1)
    xw = (pts_c - t) @ R  # X_w = R^T (X_c - t)
    u = fx * pts_c[:, 0] / pts_c[:, 2] + cx + rs.normal(0, 1, n)
    v = fy * pts_c[:, 1] / pts_c[:, 2] + cy + rs.normal(0, 1, n)
    bad = rs.uniform(size=n) < outlier_frac
    u[bad] += rs.choice([-1, 1], bad.sum()) * rs.uniform(8, 60, bad.sum())
    v[bad] += rs.choice([-1, 1], bad.sum()) * rs.uniform(8, 60, bad.sum())
    quota = np.array([217, 181, 151, 126, 105, 87, 73, 60], dtype=np.float64)
    inv_sig = _inv_sigma2_table()[rs.choice(8, n, p=quota / quota.sum())]
    dR, dt = se3_exp(rs.normal(0, perturb, 6))
    pose = np.concatenate([(dR @ R).reshape(-1), dR @ t + dt])
    f32 = lambda a: np.ascontiguousarray(np.asarray(a, np.float32).astype(np.float64))
    extra = {}
    if stereo_frac > 0:   # a stereo / RGB-D frame: that fraction of the keypoints has a right-image column (own random stream)
        rs2 = np.random.RandomState(seed + 777)
        bf = float(np.float32(baseline * fx))
        ur = u - bf / pts_c[:, 2] + rs2.normal(0, 1, n)
        bad_r = rs2.uniform(size=n) < outlier_frac
        ur[bad_r] += rs2.choice([-1, 1], bad_r.sum()) * rs2.uniform(8, 40, bad_r.sum())
        ur = np.where(rs2.uniform(size=n) < stereo_frac, ur, -1.0)
        extra = {"ur": f32(ur), "bf": bf}
    return {**extra, "pose": f32(pose), "intr": f32([fx, fy, cx, cy]), "xw": f32(xw), "uv": f32(np.stack([u, v], 1)),
            "inv_sigma2": f32(inv_sig), "truth_pose": np.concatenate([R.reshape(-1), t]), "truth_outlier": bad}


def synth_search(n_kp=1500, m=600, seed=0, width=640, height=480, th=3.0, crowd=False, retarget=True):
    """A guided-search problem in the shape Tracking::SearchLocalPoints hands to
    ORBmatcher::SearchByProjection: a frame's undistorted keypoints + grid constants, and map-point
    queries projected near some of them (several queries may aim at the same keypoint, which is what
    makes the reference's loop order-dependent).  Returns (frame, queries) dicts for api / oracle."""
    rs = np.random.RandomState(1000 + seed)
    # undistorted image bounds are slightly outside the sensor (Frame::ComputeImageBounds)
    min_x, max_x, min_y, max_y = np.float32(-4.3), np.float32(width + 5.1), np.float32(-2.7), np.float32(height + 3.9)
    inv_w = np.float32(64) / np.float32(max_x - min_x)   # Frame.cc:90-91
    inv_h = np.float32(48) / np.float32(max_y - min_y)
    span = 60.0 if crowd else None
    if crowd:
        xy = np.stack([rs.uniform(300, 300 + span, n_kp), rs.uniform(200, 200 + span, n_kp)], 1).astype(np.float32)
    else:
        xy = np.stack([rs.uniform(min_x - 2, max_x + 2, n_kp), rs.uniform(min_y - 2, max_y + 2, n_kp)], 1).astype(np.float32)
    octave = rs.randint(0, 8, n_kp).astype(np.int32)
    desc = rs.randint(0, 256, (n_kp, 32)).astype(np.uint8)
    taken = (rs.rand(n_kp) < 0.15).astype(np.uint8)
    scale = np.float32(1.2) ** np.arange(8, dtype=np.float32)
    tgt = rs.randint(0, max(n_kp, 1), m) if n_kp else np.zeros(m, np.int64)
    if retarget:
        tgt[m // 2:] = tgt[:m - m // 2][rs.permutation(m - m // 2)]    # second half re-targets the first half (worst case for the ordered walk)
    uvr = np.zeros((m, 3), np.float32)
    lmin, lmax = np.zeros(m, np.int32), np.zeros(m, np.int32)
    qdesc = np.zeros((m, 32), np.uint8)
    for q in range(m):
        k = int(tgt[q]) if n_kp else 0
        lvl = int(octave[k]) if n_kp else 0
        pl = int(np.clip(lvl + rs.randint(-1, 2), 0, 7))                 # predicted level
        r = np.float32(th) * np.float32(rs.choice([2.5, 4.0])) * scale[pl]
        base = xy[k] if n_kp else np.zeros(2, np.float32)
        uvr[q] = (base[0] + rs.uniform(-0.7, 0.7) * r, base[1] + rs.uniform(-0.7, 0.7) * r, r)
        mode = rs.randint(0, 4)
        if mode == 0:
            lmin[q], lmax[q] = pl - 1, pl                                # SearchByProjection(F, MPs): [level-1, level]
        elif mode == 1:
            lmin[q], lmax[q] = pl, -1                                    # frame-to-frame, forward motion
        elif mode == 2:
            lmin[q], lmax[q] = 0, pl                                     # backward motion
        else:
            lmin[q], lmax[q] = pl - 1, pl + 1
        d = (desc[k] if n_kp else np.zeros(32, np.uint8)).copy()
        flips = rs.randint(0, 70)                                        # up to ~70 flipped bits around the target
        for b in rs.randint(0, 256, flips):
            d[b >> 3] ^= np.uint8(1 << (b & 7))
        qdesc[q] = d
    valid = (rs.rand(m) < 0.9).astype(np.uint8)
    takes = (rs.rand(m) < 0.95).astype(np.uint8)
    # a few windows entirely outside the grid
    for q in range(0, m, 37):
        uvr[q, 0] = max_x + 500.0 if (q // 37) % 2 else min_x - 500.0
    frame = dict(kp_xy=xy, kp_octave=octave, desc=desc, kp_taken=taken, min_x=float(min_x), min_y=float(min_y),
                 inv_w=float(inv_w), inv_h=float(inv_h))
    queries = dict(uvr=uvr, level_min=lmin, level_max=lmax, desc=qdesc, valid=valid, takes=takes)
    return frame, queries


def synth_search_stereo(n_kp=300, m=200, seed=0, er_mode=1, displaced_frac=0.5, stereo_frac=0.5, zero_count=3, **kw):
    """synth_search with the right-image columns of a stereo frame: (frame, queries, stereo), stereo = dict(er_mode, kp_ur (n_kp) =
    mvuRight, q_ur (m), q_ur_stride = 1, chi2_gate_stereo = 7.8, and for er_mode 2 inv_level_sigma2 (8) and chi2_gate = 5.99).  A
    query's target is the keypoint its descriptor was derived from (the nearest one in Hamming distance).
      * about stereo_frac of the keypoints are stereo (kp_ur = x - disparity > 0), the others carry -1;
      * q_ur sits within a quarter of the window radius of its target's kp_ur (er_mode 2: within half a pixel), so the gate keeps it;
      * displaced_frac of the stereo TARGET keypoints then have kp_ur moved by 200 px, more than any window radius (th * 4 * 1.2^7 =
        43 px at th = 3): the gate removes the Hamming-best candidate of the queries that aim at them;
      * zero_count keypoints carry exactly 0.0f: monocular under RADIUS (`> 0`), stereo under CHI2 (`>= 0`).
    er_mode 2 (Fuse's gate) also re-centres every query within a pixel of its target, where the two-term 5.99 gate passes, so that
    what rejects a candidate is the third term."""
    frame, queries = synth_search(n_kp, m, seed, **kw)
    rs = np.random.RandomState(7000 + seed)
    xy, desc = frame["kp_xy"], frame["desc"]
    if n_kp:
        bits = np.unpackbits(desc, axis=1).astype(np.int16)
        qbits = np.unpackbits(queries["desc"], axis=1).astype(np.int16)
        ham = qbits @ (1 - bits).T + (1 - qbits) @ bits.T
        tgt = np.argmin(ham, axis=1)
    else:
        tgt = np.zeros(m, np.int64)
    disparity = rs.uniform(2.0, 40.0, n_kp).astype(np.float32)
    kp_ur = (xy[:, 0] - disparity).astype(np.float32) if n_kp else np.zeros(0, np.float32)
    mono = (rs.rand(n_kp) >= stereo_frac) | (kp_ur <= 0)
    kp_ur[mono] = np.float32(-1.0)
    q_ur = np.zeros(m, np.float32)
    uvr = queries["uvr"].copy()
    if er_mode == 2 and n_kp:
        off = rs.uniform(-0.6, 0.6, (m, 2)).astype(np.float32)
        grid_out = np.arange(m) % 37 == 0            # synth_search's windows outside the grid stay where they are
        uvr[~grid_out, :2] = xy[tgt[~grid_out]] + off[~grid_out]
    for q in range(m):
        k = int(tgt[q]) if n_kp else 0
        r = uvr[q, 2]
        if n_kp and kp_ur[k] > 0:
            q_ur[q] = kp_ur[k] + np.float32(rs.uniform(-0.25, 0.25)) * (r if er_mode != 2 else np.float32(2.0))
        else:
            q_ur[q] = uvr[q, 0] - np.float32(rs.uniform(2.0, 40.0))
    if n_kp:
        targets = np.unique(tgt)
        st_targets = targets[kp_ur[targets] > 0]
        moved = st_targets[rs.rand(len(st_targets)) < displaced_frac]
        kp_ur[moved] += np.float32(200.0)
        zeros = rs.permutation(targets)[:min(zero_count, len(targets))] if n_kp > 3 else np.zeros(0, np.int64)
        kp_ur[zeros] = np.float32(0.0)
    queries = dict(queries, uvr=uvr)
    stereo = dict(er_mode=int(er_mode), kp_ur=kp_ur, q_ur=q_ur, q_ur_stride=1, chi2_gate_stereo=7.8)
    if er_mode == 2:
        stereo["inv_level_sigma2"] = _inv_sigma2_table(8, 1.2)
        stereo["chi2_gate"] = 5.99
    return frame, queries, stereo


def synth_init_pair(n=1500, seed=0):
    """Two frames for ORBmatcher::SearchForInitialization: F2's keypoints are F1's moved by a few pixels (plus clutter),
    descriptors a few bits apart, so that several F1 keypoints compete for one F2 keypoint (the take-over path)."""
    rs = np.random.RandomState(4000 + seed)
    f2, _ = synth_search(n, 4, 50 + seed)
    f2 = dict(f2)
    f2["kp_octave"] = np.where(rs.rand(n) < 0.7, 0, rs.randint(1, 8, n)).astype(np.int32)
    n1 = n
    src = rs.randint(0, n, n1)
    src[n1 // 2:] = src[:n1 - n1 // 2]                      # pairs of F1 keypoints aiming at the same F2 keypoint
    o1 = np.where(rs.rand(n1) < 0.75, 0, rs.randint(1, 8, n1)).astype(np.int32)
    prev = (f2["kp_xy"][src] + rs.uniform(-25, 25, (n1, 2))).astype(np.float32)
    d1 = f2["desc"][src].copy()
    for j in range(n1):
        for b in rs.randint(0, 256, rs.randint(0, 45)):
            d1[j, b >> 3] ^= np.uint8(1 << (b & 7))
    f1 = dict(kp_octave=o1, desc=d1, angle=rs.uniform(0, 360, n1).astype(np.float32))
    f2["angle"] = rs.uniform(0, 360, n).astype(np.float32)
    return f1, prev, f2


def synth_bow(n1=1000, n2=1000, n_nodes=100, seed=0, mode=0, big_group=0):
    """Two keyframes as the BoW drivers see them: descriptors, per-feature vocabulary node (DBoW2::FeatureVector at
    levelsup 4 puts ~10 features of a 1000-feature frame into each of ~100 nodes), validity masks, and the node groups
    common to both sides in ascending node order (what the reference's while / lower_bound walk visits).  Side 2 holds
    noisy copies of side-1 descriptors (several per source now and then, so queries compete for candidates) that mostly
    share the source's node.  mode 1 adds the SearchForTriangulation geometry: a pure sideways translation between two
    identical pinhole cameras (epipolar lines are image rows), matching features on the same row up to a pixel or two.
    big_group > 0 forces that many candidates into one node (more than one wavefront of them).
    Returns (side1, side2, groups, epi)."""
    rs = np.random.RandomState(5000 + seed)
    d1 = rs.randint(0, 256, (n1, 32)).astype(np.uint8)
    node1 = rs.randint(0, max(n_nodes, 1), n1)
    src = rs.randint(0, max(n1, 1), n2) if n1 else np.zeros(n2, np.int64)
    d2 = d1[src].copy() if n1 else rs.randint(0, 256, (n2, 32)).astype(np.uint8)
    for i in range(n2):
        for b in rs.randint(0, 256, rs.randint(0, 90)):          # up to ~90 flipped bits
            d2[i, b >> 3] ^= np.uint8(1 << (b & 7))
    node2 = np.where(rs.rand(n2) < 0.85, node1[src] if n1 else 0, rs.randint(0, max(n_nodes, 1), n2))
    if big_group and n2:
        node2[:min(big_group, n2)] = node1[0] if n1 else 0
    if n2 > 10:                                                   # exact duplicates: ties in distance
        d2[1] = d2[0]; node2[1] = node2[0]
    side1 = dict(desc=d1, valid=(rs.rand(n1) < 0.8).astype(np.uint8))
    side2 = dict(desc=d2, valid=None if mode == 0 and seed % 2 == 0 else (rs.rand(n2) < 0.85).astype(np.uint8))
    qp, qi, cp, ci = [0], [], [0], []
    for node in sorted(set(node1.tolist()) & set(node2.tolist())):
        a, b = np.nonzero(node1 == node)[0], np.nonzero(node2 == node)[0]
        qi += a.tolist(); ci += b.tolist()
        qp.append(len(qi)); cp.append(len(ci))
    groups = dict(q_ptr=np.array(qp, np.int32), q_idx=np.array(qi, np.int32), c_ptr=np.array(cp, np.int32), c_idx=np.array(ci, np.int32))
    epi = None
    if mode == 1:
        fx, fy, cx, cy = np.float32(517.3), np.float32(516.5), np.float32(318.6), np.float32(255.3)
        xy1 = np.stack([rs.uniform(20, 620, n1), rs.uniform(20, 460, n1)], 1).astype(np.float32)
        # camera 2 = camera 1 shifted along x: x2 = x1 - disparity, y2 = y1 (+ noise; some far off the line)
        disp = rs.uniform(2, 60, n2).astype(np.float32)
        noise = np.where(rs.rand(n2) < 0.75, rs.normal(0, 0.8, n2), rs.normal(0, 12.0, n2)).astype(np.float32)
        xy2 = np.stack([xy1[src, 0] - disp, xy1[src, 1] + noise], 1).astype(np.float32) if n1 else np.zeros((n2, 2), np.float32)
        oct2 = rs.randint(0, 8, n2).astype(np.int32)
        # F12 with x1^T F12 x2 = 0 for t = (b, 0, 0), R = I:  F = K^-T [t]x K^-1  (any scale)
        K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float64)
        tx = np.array([[0, 0, 0], [0, 0, -1.0], [0, 1.0, 0]])
        Ki = np.linalg.inv(K)
        F = (Ki.T @ tx @ Ki).astype(np.float32)
        if seed % 3 == 0:
            F[:, :] = 0                                           # degenerate: den == 0 for every query
        scale = (np.float32(1.2) ** np.arange(8, dtype=np.float32)).astype(np.float32)
        # the epipole of a sideways translation is at infinity; put a finite one inside the image to exercise :737-743
        epi = dict(F12=F.reshape(9), ex=float(xy2[0, 0]) if n2 else 0.0, ey=float(xy2[0, 1]) if n2 else 0.0,
                   scale_factor=scale.tolist(), level_sigma2=(scale * scale).tolist())
        side1["kp_xy"] = xy1
        side2["kp_xy"] = xy2
        side2["kp_octave"] = oct2
    return side1, side2, groups, epi


def synth_bow_stereo(n1=300, n2=620, n_nodes=12, seed=0, group_sizes=(1, 63, 64, 65, 130), near_epipole_frac=0.25, stereo_frac=0.6):
    """Two STEREO keyframes as ORBmatcher::SearchForTriangulation sees them (ORBmatcher.cc:695-793): synth_bow's mode-1 layout
    (side1, side2, groups, epi) with `ur` (mvuRight) on both sides, and a motion with a forward component, so that the epipole of
    camera 1 lies INSIDE image 2 and the epipole test (:747-753) has candidates to reject.  Camera 2 is camera 1 moved by
    (0.06, -0.03, 0.5); every side-1 feature is a point at a depth of 2..15, a share near_epipole_frac of them within 14 px of the
    focus of expansion; side 2 holds noisy copies of side-1 descriptors in the source's node, at the point's projection into camera 2
    (a quarter of them ~12 px off).  The first len(group_sizes) nodes hold exactly group_sizes candidates.  A share stereo_frac of
    the features of each side is stereo (ur = x - bf / z when that is >= 0), the rest has ur = -1, one NaN and one 0.0f per side."""
    rs = np.random.RandomState(19500 + seed)
    f32 = np.float32
    k = len(group_sizes)
    assert n_nodes > k and n1 >= 4 * k and n2 > sum(group_sizes) + 4
    d1 = rs.randint(0, 256, (n1, 32)).astype(np.uint8)
    node1 = rs.randint(0, n_nodes, n1)
    node1[:4 * k] = np.repeat(np.arange(k), 4)                   # at least four queries in each sized group
    node2 = np.concatenate([np.full(sz, j) for j, sz in enumerate(group_sizes)] + [rs.randint(k, n_nodes, n2 - sum(group_sizes))])
    src = np.zeros(n2, np.int64)
    for i in range(n2):
        same = np.flatnonzero(node1 == node2[i])
        src[i] = same[rs.randint(len(same))] if len(same) else rs.randint(n1)
    d2 = d1[src].copy()
    for i in range(n2):
        for b in rs.randint(0, 256, rs.randint(0, 60)):
            d2[i, b >> 3] ^= np.uint8(1 << (b & 7))
    fx, fy, cx, cy = f32(517.3), f32(516.5), f32(318.6), f32(255.3)
    t21 = -np.array([0.06, -0.03, 0.5])                            # X2 = X1 + t21
    ex, ey = float(fx) * t21[0] / t21[2] + float(cx), float(fy) * t21[1] / t21[2] + float(cy)
    xy1 = np.stack([rs.uniform(20, 620, n1), rs.uniform(20, 460, n1)], 1)
    near = rs.rand(n1) < near_epipole_frac
    xy1[near] = np.array([ex, ey]) + rs.uniform(-14, 14, (int(near.sum()), 2))
    xy1 = xy1.astype(f32)
    z1 = rs.uniform(2.0, 15.0, n1)
    X1 = np.stack([(xy1[:, 0] - float(cx)) / float(fx) * z1, (xy1[:, 1] - float(cy)) / float(fy) * z1, z1], 1)
    X2 = X1[src] + t21
    noise = np.where((rs.rand(n2) < 0.75)[:, None], rs.normal(0, 0.8, (n2, 2)), rs.normal(0, 12.0, (n2, 2)))
    xy2 = (np.stack([float(fx) * X2[:, 0] / X2[:, 2] + float(cx), float(fy) * X2[:, 1] / X2[:, 2] + float(cy)], 1) + noise).astype(f32)
    a = sum(group_sizes[:2])                                     # exact duplicates inside the 64-candidate group: a tie, the last one wins
    d2[a + 1], xy2[a + 1], src[a + 1] = d2[a], xy2[a], src[a]
    oct2 = rs.randint(0, 8, n2).astype(np.int32)
    bf = 0.12 * float(fx)
    ur1 = np.where(rs.rand(n1) < stereo_frac, xy1[:, 0] - bf / z1, -1.0)
    ur2 = np.where(rs.rand(n2) < stereo_frac, xy2[:, 0] - bf / X2[:, 2], -1.0)
    ur1, ur2 = np.where(ur1 >= 0, ur1, -1.0).astype(f32), np.where(ur2 >= 0, ur2, -1.0).astype(f32)
    ur1[4 * k], ur1[4 * k + 1], ur2[n2 - 1], ur2[n2 - 2] = np.nan, 0.0, np.nan, 0.0
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float64)
    tx = np.array([[0, -t21[2], t21[1]], [t21[2], 0, -t21[0]], [-t21[1], t21[0], 0]])
    Ki = np.linalg.inv(K)
    F = (Ki.T @ tx.T @ Ki).astype(f32)                           # x2^T [t21]x x1 = 0, so x1^T F12 x2 = 0 with F12 = K^-T [t21]x^T K^-1
    scale = (f32(1.2) ** np.arange(8, dtype=f32)).astype(f32)
    side1 = dict(desc=d1, valid=(rs.rand(n1) < 0.85).astype(np.uint8), kp_xy=xy1, ur=ur1)
    side2 = dict(desc=d2, valid=(rs.rand(n2) < 0.9).astype(np.uint8), kp_xy=xy2, kp_octave=oct2, ur=ur2)
    qp, qi, cp, ci = [0], [], [0], []
    for node in sorted(set(node1.tolist()) & set(node2.tolist())):
        qa, cb = np.nonzero(node1 == node)[0], np.nonzero(node2 == node)[0]
        qi += qa.tolist(); ci += cb.tolist()
        qp.append(len(qi)); cp.append(len(ci))
    groups = dict(q_ptr=np.array(qp, np.int32), q_idx=np.array(qi, np.int32), c_ptr=np.array(cp, np.int32), c_idx=np.array(ci, np.int32))
    epi = dict(F12=F.reshape(9), ex=ex, ey=ey, scale_factor=scale.tolist(), level_sigma2=(scale * scale).tolist())
    return side1, side2, groups, epi


def synth_sim3(n=200, outlier_frac=0.15, seed=0, perturb=0.03, fix_scale=False, scale=1.08):
    """An Optimizer::OptimizeSim3 problem as the reference assembles it (Optimizer.cc:1099-1178): the same physical points as
    map points of two keyframes, each in its own camera frame (p1, p2, float values), their keypoints in both images, a true
    similarity p1 = s R p2 + t and a perturbed initial g2oS12 (what Sim3Solver's RANSAC hands over).  Outliers are wrong
    keypoint associations.  Returns a dict in the layout of slamit_sim3_problem."""
    rs = np.random.RandomState(9000 + seed)
    f32 = np.float32
    intr1 = np.array([517.3, 516.5, 318.6, 255.3], f32).astype(np.float64)
    intr2 = np.array([520.9, 521.0, 325.1, 249.7], f32).astype(np.float64)
    s_true = 1.0 if fix_scale else scale
    R, t = se3_exp(np.array([0.05, -0.08, 0.03, 0.4, -0.1, 0.2]))
    p2 = np.stack([rs.uniform(-2.5, 2.5, n), rs.uniform(-1.8, 1.8, n), rs.uniform(2.5, 9.0, n)], 1)
    p1 = s_true * (p2 @ R.T) + t + rs.normal(0, 0.01, (n, 3))           # two independent estimates of the same points
    p1[:, 2] = np.maximum(p1[:, 2], 0.5)
    p1, p2 = p1.astype(f32).astype(np.float64), p2.astype(f32).astype(np.float64)
    obs1 = np.stack([intr1[0] * p1[:, 0] / p1[:, 2] + intr1[2], intr1[1] * p1[:, 1] / p1[:, 2] + intr1[3]], 1) + rs.normal(0, 0.7, (n, 2))
    obs2 = np.stack([intr2[0] * p2[:, 0] / p2[:, 2] + intr2[2], intr2[1] * p2[:, 1] / p2[:, 2] + intr2[3]], 1) + rs.normal(0, 0.7, (n, 2))
    bad = rs.rand(n) < outlier_frac
    obs1[bad] += rs.uniform(-60, 60, (int(bad.sum()), 2))
    scale_f = f32(1.2) ** np.arange(8, dtype=f32)
    lv1, lv2 = rs.randint(0, 8, n), rs.randint(0, 8, n)
    isig1 = (f32(1) / (scale_f * scale_f))[lv1].astype(np.float64)
    isig2 = (f32(1) / (scale_f * scale_f))[lv2].astype(np.float64)
    dR, dt = se3_exp(rs.normal(0, perturb, 6))
    R0, t0 = dR @ R, dR @ t + dt
    s0 = s_true * (1.0 if fix_scale else float(np.exp(rs.normal(0, perturb))))
    return dict(n=n, p1=p1, p2=p2, obs1=obs1.astype(f32).astype(np.float64), obs2=obs2.astype(f32).astype(np.float64),
                inv_sigma2_1=isig1, inv_sigma2_2=isig2, intr1=intr1, intr2=intr2, r12=R0.reshape(9), t12=t0, s12=s0,
                th2=10.0, fix_scale=int(fix_scale), true=dict(R=R, t=t, s=s_true, bad=bad))


def synth_sim3_ransac(n=200, outlier_frac=0.3, seed=0, noise_px=0.5, fix_scale=False):
    """What the Sim3Solver constructor gathers for one loop candidate (Sim3Solver.cc:62-109): the same physical points as map points
    of two keyframes, each in its own camera frame (x1 = mvX3Dc1, x2 = mvX3Dc2, float32), related by a known similarity
    x1 = s R x2 + t.  Each keyframe's estimate of a point is off by about noise_px pixels of its own image (three times that in
    depth); a fraction outlier_frac of the pairs are wrong associations (x2 is another point).  Every point carries the octave of
    its keypoint in each image: sigma2_1 / sigma2_2 = mvLevelSigma2[octave] and max_err1 / max_err2 = (float)(size_t)(9.210 sigma2),
    the truncated bounds of mvnMaxError1/2.  obs1 / obs2 / inv_sigma2_1 / inv_sigma2_2 are the keypoints, so that the accepted
    similarity can go on to OptimizeSim3.  Layout of slamit_sim3_ransac_problem (without triples)."""
    rs = np.random.RandomState(11000 + seed)
    f32 = np.float32
    intr1 = np.array([517.3, 516.5, 318.6, 255.3], f32)
    intr2 = np.array([520.9, 521.0, 325.1, 249.7], f32)
    s_true = 1.0 if fix_scale else 1.08
    R, t = se3_exp(np.array([0.05, -0.08, 0.03, 0.4, -0.1, 0.2]))
    X2 = np.stack([rs.uniform(-2.5, 2.5, n), rs.uniform(-1.8, 1.8, n), rs.uniform(2.5, 9.0, n)], 1)
    X1 = s_true * (X2 @ R.T) + t
    x1 = X1 + rs.normal(0, noise_px, (n, 3)) * X1[:, 2:3] / float(intr1[0]) * np.array([1.0, 1.0, 3.0])
    x2 = X2 + rs.normal(0, noise_px, (n, 3)) * X2[:, 2:3] / float(intr2[0]) * np.array([1.0, 1.0, 3.0])
    bad = rs.rand(n) < outlier_frac
    nb = int(bad.sum())
    x2[bad] = np.stack([rs.uniform(-2.5, 2.5, nb), rs.uniform(-1.8, 1.8, nb), rs.uniform(2.5, 9.0, nb)], 1)
    x1, x2 = x1.astype(f32), x2.astype(f32)
    scale_f = f32(1.2) ** np.arange(8, dtype=f32)
    sigma2 = (scale_f * scale_f).astype(f32)
    lv1, lv2 = rs.randint(0, 8, n), rs.randint(0, 8, n)
    s1, s2 = sigma2[lv1], sigma2[lv2]
    d1, d2 = x1.astype(np.float64), x2.astype(np.float64)
    obs1 = np.stack([intr1[0] * d1[:, 0] / d1[:, 2] + intr1[2], intr1[1] * d1[:, 1] / d1[:, 2] + intr1[3]], 1) + rs.normal(0, noise_px, (n, 2))
    obs2 = np.stack([intr2[0] * d2[:, 0] / d2[:, 2] + intr2[2], intr2[1] * d2[:, 1] / d2[:, 2] + intr2[3]], 1) + rs.normal(0, noise_px, (n, 2))
    return dict(n=n, x1=x1, x2=x2, sigma2_1=s1, sigma2_2=s2,
                max_err1=np.floor(9.210 * s1.astype(np.float64)).astype(f32), max_err2=np.floor(9.210 * s2.astype(np.float64)).astype(f32),
                intr1=intr1, intr2=intr2, fix_scale=int(fix_scale), obs1=obs1.astype(f32), obs2=obs2.astype(f32),
                inv_sigma2_1=(f32(1) / s1).astype(f32), inv_sigma2_2=(f32(1) / s2).astype(f32),
                true=dict(R=R, t=t, s=s_true, bad=bad))


def synth_triangulation(n=300, seed=0, baseline=0.3, outlier_frac=0.2, noise_px=0.7, depth=(1.5, 12.0), direction=(1.0, 0.05, 0.1),
                        behind_frac=0.0, octave_jump_frac=0.0, octave_jump=4):
    """What LocalMapping::CreateNewMapPoints holds for one (current keyframe, neighbour) pair after SearchForTriangulation
    (LocalMapping.cc:323-346): two posed pinhole keyframes `baseline` apart along `direction` (in keyframe 1's frame) and n matched
    undistorted keypoints.  The points lie at depths drawn log-uniformly from `depth`, so that with a baseline of a few tenths the
    rays' parallax spans the 0.9998 gate; each keypoint sits on an octave 0..7 (octave2 = octave1 +- 1, clipped) and carries pixel
    noise of noise_px times its level's scale factor.  A share outlier_frac of the pairs are gross outliers (keypoint 2 moved by
    8..60 px), behind_frac of the points lie behind keyframe 1 (negative depth, projected all the same), and octave_jump_frac of
    the pairs get octave2 = octave1 +- octave_jump, which the scale-consistency test rejects.  A `direction` along the optical
    axis with a baseline longer than the nearest depth puts points between the two cameras: in front of 1, behind 2.
    Layout of slamit_triangulate_problem."""
    rs = np.random.RandomState(13000 + seed)
    f32 = np.float32
    fx1, fy1, cx1, cy1 = f32(517.3), f32(516.5), f32(318.6), f32(255.3)
    fx2, fy2, cx2, cy2 = f32(520.9), f32(521.0), f32(325.1), f32(249.7)
    intr1 = np.array([fx1, fy1, cx1, cy1, f32(1) / fx1, f32(1) / fy1], f32)
    intr2 = np.array([fx2, fy2, cx2, cy2, f32(1) / fx2, f32(1) / fy2], f32)
    R1, t1 = se3_exp(np.array([0.04, -0.3, 0.02, 0.6, -0.2, 1.1]))               # world -> keyframe 1
    d = np.asarray(direction, np.float64)
    d = d / np.linalg.norm(d)
    R21, _ = se3_exp(np.array([0.02, -0.03, 0.01, 0, 0, 0]))                     # keyframe 1 -> keyframe 2: a small turn, then the baseline
    R2, t2 = R21 @ R1, R21 @ (t1 - baseline * d)
    z = np.exp(rs.uniform(np.log(depth[0]), np.log(depth[1]), n))
    behind = rs.rand(n) < behind_frac
    z[behind] = -z[behind]
    Xc1 = np.stack([rs.uniform(-0.55, 0.55, n) * z, rs.uniform(-0.42, 0.42, n) * z, z], 1)
    Xw = (Xc1 - t1) @ R1                                                         # R1^T (Xc1 - t1)
    Xc2 = Xw @ R2.T + t2
    nlev = 8
    scale_f = f32(1.2) ** np.arange(nlev, dtype=f32)
    sigma2 = (scale_f * scale_f).astype(f32)
    o1 = rs.randint(0, nlev, n)
    o2 = np.clip(o1 + rs.choice([-1, 1], n), 0, nlev - 1)
    jump = rs.rand(n) < octave_jump_frac
    o2[jump] = np.where(o1[jump] >= octave_jump, o1[jump] - octave_jump, np.minimum(o1[jump] + octave_jump, nlev - 1))
    kp1 = np.stack([fx1 * Xc1[:, 0] / Xc1[:, 2] + cx1, fy1 * Xc1[:, 1] / Xc1[:, 2] + cy1], 1) + rs.normal(0, noise_px, (n, 2)) * scale_f[o1][:, None]
    kp2 = np.stack([fx2 * Xc2[:, 0] / Xc2[:, 2] + cx2, fy2 * Xc2[:, 1] / Xc2[:, 2] + cy2], 1) + rs.normal(0, noise_px, (n, 2)) * scale_f[o2][:, None]
    bad = rs.rand(n) < outlier_frac
    ang, r = rs.uniform(0, 2 * np.pi, n), rs.uniform(8, 60, n)
    kp2[bad] += np.stack([r * np.cos(ang), r * np.sin(ang)], 1)[bad]
    T1 = np.concatenate([R1, t1[:, None]], 1).astype(f32).reshape(12)
    T2 = np.concatenate([R2, t2[:, None]], 1).astype(f32).reshape(12)
    return dict(n=n, Tcw1=T1, Tcw2=T2, intr1=intr1, intr2=intr2, kp1_xy=kp1.astype(f32), kp2_xy=kp2.astype(f32),
                octave1=o1.astype(np.int32), octave2=o2.astype(np.int32), n_levels=nlev,
                scale_factors1=scale_f.copy(), level_sigma2_1=sigma2.copy(), scale_factors2=scale_f.copy(), level_sigma2_2=sigma2.copy(),
                ratio_factor=f32(1.5) * f32(1.2), true=dict(X=Xw, bad=bad, behind=behind, jump=jump))


def synth_triangulation_stereo(n=300, seed=0, baseline=0.3, outlier_frac=0.2, noise_px=0.7, mb=0.12, stereo_frac=(0.25, 0.25, 0.25),
                               ur_outlier_frac=0.06, distortion=4e-8, **opts):
    """synth_triangulation(n, seed, baseline, outlier_frac, noise_px, **opts) on stereo keyframes: the same problem plus what
    LocalMapping::CreateNewMapPoints reads of a stereo keypoint (LocalMapping.cc:335-345, KeyFrame::UnprojectStereo).  Shares
    stereo_frac of the pairs are stereo in keyframe 1 only, in keyframe 2 only and in both (the rest in neither), drawn per pair so
    that every wavefront mixes them.  A stereo keypoint has ur = u - bf / z of the true point plus the level's pixel noise, moved by a
    further 2..6 level-scaled pixels for a share ur_outlier_frac (the third error term alone then rejects it), and depth = bf / (u - ur)
    in float as Frame::ComputeStereoMatches stores it; a keypoint whose point is nearer than 0.3 or behind the camera, or whose ur or
    disparity is not positive, stays monocular (ur = depth = -1).  raw*_xy is the distorted keypoint mvKeys: the undistorted one moved
    radially by distortion * r^2 * (p - c), about a pixel at the image border.  mb1 = mb2 = mb, bf = mb * fx1, the current keyframe's."""
    pr = synth_triangulation(n, seed, baseline, outlier_frac, noise_px, **opts)
    rs = np.random.RandomState(19000 + seed)
    f32 = np.float32
    kind = rs.choice(4, n, p=[1.0 - sum(stereo_frac)] + list(stereo_frac))       # 0 neither, 1 keyframe 1, 2 keyframe 2, 3 both
    Xw = pr["true"]["X"]
    out = dict(pr, mb1=f32(mb), mb2=f32(mb), bf=f32(mb) * pr["intr1"][0])
    for side, flag in ((1, (kind == 1) | (kind == 3)), (2, (kind == 2) | (kind == 3))):
        T = pr["Tcw%d" % side].astype(np.float64).reshape(3, 4)
        intr, kp, octv = pr["intr%d" % side], pr["kp%d_xy" % side], pr["octave%d" % side]
        z = Xw @ T[2, :3] + T[2, 3]
        bf = float(f32(mb) * intr[0])
        scale = pr["scale_factors%d" % side][octv].astype(np.float64)
        with np.errstate(all="ignore"):
            u_true = intr[0] * (Xw @ T[0, :3] + T[0, 3]) / z + intr[2]
            ur = u_true - bf / z + rs.normal(0, noise_px, n) * scale
        far = rs.rand(n) < ur_outlier_frac
        ur = np.where(far, ur + rs.choice([-1.0, 1.0], n) * rs.uniform(2.0, 6.0, n) * scale, ur).astype(f32)
        with np.errstate(all="ignore"):
            disp = kp[:, 0] - ur
            depth = (out["bf"] / disp).astype(f32)
        ok = flag & (z > 0.3) & (ur >= 0) & (disp > 0) & np.isfinite(depth)
        out["ur%d" % side] = np.where(ok, ur, f32(-1)).astype(f32)
        out["depth%d" % side] = np.where(ok, depth, f32(-1)).astype(f32)
        c = intr[2:4].astype(np.float64)
        dxy = kp.astype(np.float64) - c
        out["raw%d_xy" % side] = (kp.astype(np.float64) + distortion * (dxy ** 2).sum(1)[:, None] * dxy).astype(f32)
    out["true"] = dict(pr["true"], kind=kind)
    return out


def synth_frustum(seed=0, n=1000, th=1.0, n_levels=8, width=640, height=480, skip_frac=0.05, behind_frac=0.08, frontal_frac=0.3,
                  max_angle_deg=75.0, level_span=(-1.5, 1.5)):
    """What Tracking::SearchLocalPoints holds for one frame (Tracking.cc:1409-1464): a posed pinhole frame and n local map points
    around its view cone, so that every test of Frame::isInFrustum rejects a visible share.  The points are drawn in the camera
    frame -- depth log-uniform in 0.5..20 (a share behind_frac behind the camera), x / y over 1.3 times the field of view -- and
    moved to the world.  Each carries a mean viewing direction (GetNormal) that is its ray turned by an angle: up to 3 degrees for a
    share frontal_frac (viewCos > 0.998, the narrow search window), up to max_angle_deg for the rest (viewingCosLimit 0.5 is 60
    degrees).  Its scale-invariance range is max_dist = dist * 1.2^e with e uniform in [level_span[0], n_levels + level_span[1]]
    and min_dist = max_dist / 1.2^(n_levels - 1), as MapPoint::UpdateNormalAndDepth sets them: e < -1 and e > n_levels + 0.22 fall
    to the distance gate, ceil(e) is the predicted level, and n_levels - 1 < e <= n_levels + 0.22 passes the gate with a level
    outside the table.  skip marks a share skip_frac as bad or already seen.  Layout of slamit_frustum_problem."""
    rs = np.random.RandomState(14000 + seed)
    f32 = np.float32
    fx, fy, cx, cy, bf = f32(517.3), f32(516.5), f32(318.6), f32(255.3), f32(38.6)
    min_x, max_x, min_y, max_y = f32(-4.3), f32(width + 5.1), f32(-2.7), f32(height + 3.9)
    R, t = se3_exp(np.concatenate([rs.uniform(-0.4, 0.4, 3), rs.uniform(-2.0, 2.0, 3)]))
    Rcw, tcw = R.astype(f32), t.astype(f32)
    Ow = (-(Rcw.astype(np.float64).T @ tcw.astype(np.float64))).astype(f32)         # as Frame::UpdatePoseMatrices stores it
    z = np.exp(rs.uniform(np.log(0.5), np.log(20.0), n))
    z[rs.rand(n) < behind_frac] *= -1.0
    hx, hy = 1.3 * 0.5 * width / float(fx), 1.3 * 0.5 * height / float(fy)
    Xc = np.stack([rs.uniform(-hx, hx, n) * np.abs(z), rs.uniform(-hy, hy, n) * np.abs(z), z], 1)
    pos = ((Xc - t) @ R).astype(f32)
    PO = pos.astype(np.float64) - Ow.astype(np.float64)
    dist = np.linalg.norm(PO, axis=1)
    d = PO / dist[:, None]
    ang = np.deg2rad(np.where(rs.rand(n) < frontal_frac, rs.uniform(0.0, 3.0, n), rs.uniform(0.0, max_angle_deg, n)))
    side = rs.normal(size=(n, 3))
    side -= (side * d).sum(1)[:, None] * d
    side /= np.linalg.norm(side, axis=1)[:, None]
    normal = (np.cos(ang)[:, None] * d + np.sin(ang)[:, None] * side).astype(f32)
    e = rs.uniform(level_span[0], n_levels + level_span[1], n)
    max_dist = (dist * 1.2 ** e).astype(f32)
    min_dist = (max_dist / f32(1.2) ** f32(n_levels - 1)).astype(f32)
    skip = (rs.rand(n) < skip_frac).astype(np.uint8)
    scale_f = (f32(1.2) ** np.arange(n_levels, dtype=f32)).astype(f32)
    return dict(n=n, Rcw=Rcw.reshape(9), tcw=tcw, Ow=Ow, fx=fx, fy=fy, cx=cx, cy=cy, bf=bf, min_x=min_x, max_x=max_x, min_y=min_y, max_y=max_y,
                view_cos_limit=f32(0.5), log_scale_factor=f32(np.log(f32(1.2))), th=f32(th), n_levels=n_levels, scale_factors=scale_f,
                pos=pos, normal=normal, max_dist=max_dist, min_dist=min_dist, skip=skip, true=dict(e=e, angle=ang, Xc=Xc))


PROJECT_FORMS = ("LAST_FRAME", "RELOC", "FUSE", "SIM3_PROJ", "SIM3_FUSE", "SIM3_PAIR")   # api.PROJECT_FORMS: the index is slamit_project_camera.form


def synth_project(seed=0, n=1000, form="FUSE", th=3.0, direction=0, n_levels=8, scale=1.3, octave_frac=0.06, **kw):
    """One camera of one of the six projection loops in front of the guided search (csrc/project.h) and n map points around its view
    cone, so that every test of every form rejects a visible share: synth_frustum's construction (its camera, points, normals,
    distance ranges and skip flags; **kw goes to it), recast per form.
      LAST_FRAME  R, t, O are the frame's; octave is uniform over the table, with a share octave_frac each of -1 and of n_levels
                  (the level outside the table); direction 0, 1 (forward) or 2 (backward) picks the level window
      RELOC, FUSE R, t, O are the frame's / keyframe's
      SIM3_PROJ, SIM3_FUSE  Scw = [scale R | scale t] in float32, and R, t, O out of it as sim3detail::decompose takes them
      SIM3_PAIR   the points' keyframe has a pose of its own (R, t); (R2, t2) = (sR21, t21) of SearchBySim3 with s12 = scale, so the
                  point arrives in the searched camera at 1 / scale of its depth; max_dist and min_dist are divided by scale with it
    Arrays the form does not read are None.  Layout of slamit_project_problem."""
    f32, f64 = np.float32, np.float64
    k = PROJECT_FORMS.index(form) if isinstance(form, str) else int(form)
    b = synth_frustum(seed, n, th, n_levels=n_levels, **kw)
    rs = np.random.RandomState(16000 + 8 * seed + k)
    Rcw, tcw = b["Rcw"].reshape(3, 3), b["tcw"]
    out = dict(n=n, form=k, direction=int(direction), R=b["Rcw"], t=tcw, O=b["Ow"], R2=np.zeros(9, f32), t2=np.zeros(3, f32), th=f32(th),
               pos=b["pos"], normal=b["normal"], max_dist=b["max_dist"], min_dist=b["min_dist"], octave=None, skip=b["skip"], true=dict(b["true"]))
    for key in ("fx", "fy", "cx", "cy", "min_x", "max_x", "min_y", "max_y", "log_scale_factor", "n_levels", "scale_factors"):
        out[key] = b[key]
    if k == 0:
        octave = rs.randint(0, n_levels, n).astype(np.int32)
        pick = rs.rand(n)
        octave[pick < octave_frac] = -1
        octave[pick > 1.0 - octave_frac] = n_levels
        out.update(octave=octave, normal=None, max_dist=None, min_dist=None)
    elif k == 1:
        out.update(normal=None)
    elif k in (3, 4):
        Scw = np.concatenate([f32(scale) * Rcw, (f32(scale) * tcw)[:, None]], 1).astype(f32)
        scw = f32(np.sqrt((Scw[0, :3].astype(f64) ** 2).sum()))
        R, t = (Scw[:, :3] / scw).astype(f32), (Scw[:, 3] / scw).astype(f32)
        O = (-(R.astype(f64).T @ t.astype(f64))).astype(f32)
        out.update(R=R.reshape(9), t=t, O=O, true=dict(out["true"], Scw=Scw))
    elif k == 5:
        R1, t1 = se3_exp(np.concatenate([rs.uniform(-0.3, 0.3, 3), rs.uniform(-1.0, 1.0, 3)]))
        R1w, t1w = R1.astype(f32), t1.astype(f32)
        R12 = (R1w.astype(f64) @ Rcw.astype(f64).T).astype(f32)                       # x1 = s12 R12 x2 + t12
        t12 = (t1w.astype(f64) - R12.astype(f64) @ tcw.astype(f64)).astype(f32)
        s12 = f32(scale)
        sR21 = ((1.0 / f64(s12)) * R12.T.astype(f64)).astype(f32)                       # ORBmatcher.cc:1120
        t21 = (-(sR21.astype(f64) @ t12.astype(f64))).astype(f32)                       # :1121
        out.update(R=R1w.reshape(9), t=t1w, O=np.zeros(3, f32), R2=sR21.reshape(9), t2=t21, normal=None,
                   max_dist=(b["max_dist"] / s12).astype(f32), min_dist=(b["min_dist"] / s12).astype(f32))
    return out


def synth_map(n_kf, n_pt, obs_per_pt, n_fixed, seed, stereo_frac=0.0, loop=True, outlier_frac=0.03, baseline=0.08):
    """A map-sized BA window (slamit_ba_problem layout, as synth_ba): n_kf cameras on a circle of radius 2 in the x-z plane, each looking
    outward, and n_pt points on a cylinder of radius 6 around it.  loop=True: the trajectory closes (keyframe k at 2 pi k / n_kf), so the
    last keyframes observe the first keyframes' points again and the reduced system's row envelope is not a band; loop=False: an arc of
    1.6 pi.  Every point is observed by up to obs_per_pt keyframes nearest to it in angle (at least two); every observation has positive
    depth and lands inside a 640 x 480 image.  The first n_fixed keyframes are fixed (0 .. n_fixed - 1).  Deterministic from `seed`."""
    rs = np.random.RandomState(seed)
    rs2 = np.random.RandomState(seed + 777)
    fx, fy, cx, cy = INTRINSICS
    span = 2.0 * np.pi if loop else 1.6 * np.pi
    th = span * np.arange(n_kf) / n_kf
    Rs, ts = [], []
    for a in th:
        z = np.array([np.cos(a), 0.0, np.sin(a)])
        y = np.array([0.0, 1.0, 0.0])
        R = np.stack([np.cross(y, z), y, z])
        c = 2.0 * z
        Rs.append(R)
        ts.append(-R @ c)
    inv_sig = _inv_sigma2_table()
    quota = np.array([217, 181, 151, 126, 105, 87, 73, 60], dtype=np.float64)
    quota /= quota.sum()
    bf = float(np.float32(baseline * fx))
    pts, e_kf, e_pt, e_uv, e_is, e_ur = [], [], [], [], [], []
    margin = 8.0
    while len(pts) < n_pt:
        phi = rs.uniform(0.0, span)
        X = np.array([6.0 * np.cos(phi), rs.uniform(-1.2, 1.2), 6.0 * np.sin(phi)])
        near = np.argsort(np.abs((th - phi + np.pi) % (2.0 * np.pi) - np.pi) if loop else np.abs(th - phi), kind="stable")[:obs_per_pt]
        obs = []
        for k in sorted(int(k) for k in near):
            Xc = Rs[k] @ X + ts[k]
            if not Xc[2] > 0.5:
                continue
            u, v = fx * Xc[0] / Xc[2] + cx, fy * Xc[1] / Xc[2] + cy
            if margin <= u <= 640 - margin and margin <= v <= 480 - margin:
                obs.append((k, Xc))
        if len(obs) < 2:
            continue
        p = len(pts)
        pts.append(X)
        for k, Xc in obs:
            u = fx * Xc[0] / Xc[2] + cx + rs.normal(0.0, 1.0)
            v = fy * Xc[1] / Xc[2] + cy + rs.normal(0.0, 1.0)
            if rs.uniform() < outlier_frac:
                u += rs.choice([-30.0, 30.0])
                v += rs.choice([-30.0, 30.0])
            u = min(max(u, 0.0), 639.0)
            v = min(max(v, 0.0), 479.0)
            e_kf.append(k)
            e_pt.append(p)
            e_uv.append((u, v))
            e_is.append(inv_sig[rs.choice(8, p=quota)])
            if stereo_frac > 0:
                ur = u - bf / Xc[2] + rs2.normal(0.0, 1.0)
                e_ur.append(ur if rs2.uniform() < stereo_frac else -1.0)
    pts = np.array(pts)
    poses = np.zeros((n_kf, 12))
    for k in range(n_kf):
        if k < n_fixed:
            R, t = Rs[k], ts[k]
        else:
            dR, dt = se3_exp(rs.normal(0.0, 0.003, 6))
            R, t = dR @ Rs[k], dR @ ts[k] + dt
        poses[k, :9] = R.reshape(-1)
        poses[k, 9:] = t
    poses = poses.astype(np.float32).astype(np.float64)
    pts0 = (pts + rs.normal(0.0, 0.02, pts.shape)).astype(np.float32).astype(np.float64)
    fixed = np.zeros(n_kf, dtype=np.uint8)
    fixed[:n_fixed] = 1
    intr = np.tile(np.array([fx, fy, cx, cy], dtype=np.float32).astype(np.float64), (n_kf, 1))
    extra = {}
    if stereo_frac > 0:
        extra = {"edge_ur": np.array(e_ur, dtype=np.float32).astype(np.float64), "kf_bf": np.full(n_kf, bf)}
    return {
        **extra,
        "kf_pose": np.ascontiguousarray(poses),
        "kf_fixed": fixed,
        "kf_intr": np.ascontiguousarray(intr),
        "pt_xyz": np.ascontiguousarray(pts0),
        "edge_kf": np.array(e_kf, dtype=np.int32),
        "edge_pt": np.array(e_pt, dtype=np.int32),
        "edge_uv": np.array(e_uv, dtype=np.float32).astype(np.float64),
        "edge_inv_sigma2": np.array(e_is, dtype=np.float32).astype(np.float64),
        "truth_pose": np.array([np.concatenate([Rs[k].reshape(-1), ts[k]]) for k in range(n_kf)]),
        "truth_pt": pts,
    }


# ---------------------------------------------------------------------------------------------
# Hard geometry: post-processing of the problems above (tools/gen_*_golden.py: mirror / starve_kf / starve_pt).  The generators
# above only make well-posed input -- every point in front of its observers, outliers that are gross pixel errors spread evenly.
# A front end also hands over mirrored triangulations (a point behind the cameras that observe it, with a small reprojection
# error: only the depth test removes it) and keyframes / points whose observations all fail the gate.
# ---------------------------------------------------------------------------------------------

def _append_edges(prob, kf, pt, uv, isig, ur=None):
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    q = dict(prob)
    q["edge_kf"] = np.concatenate([prob["edge_kf"], np.asarray(kf, np.int32)])
    q["edge_pt"] = np.concatenate([prob["edge_pt"], np.asarray(pt, np.int32)])
    q["edge_uv"] = np.concatenate([prob["edge_uv"], f32(uv).reshape(-1, 2)])
    q["edge_inv_sigma2"] = np.concatenate([prob["edge_inv_sigma2"], f32(isig)])
    if "edge_ur" in prob:
        q["edge_ur"] = np.concatenate([prob["edge_ur"], f32(ur)])
    return q


def _truth_cam(prob, kf, X):
    tp = prob["truth_pose"][kf]
    return tp[:9].reshape(3, 3) @ X + tp[9:]


def ba_mirror_points(prob, n, obs, seed, stereo_frac=0.0, sigma=1.0, first_kfs=()):
    """`prob` (synth_ba: every camera looks along +z) plus n mirrored triangulations: new points BEHIND `obs` consecutive keyframes
    (depth -8 .. -4 in their frames at the true state), each observed by all of them with u = fx x / z + cx, v likewise (stereo:
    ur = u - bf / z) evaluated at that negative depth, plus N(0, sigma) pixel noise.  The residuals are small at the truth, so only
    the depth test flags these edges.  Point i < len(first_kfs) starts its run of observers at keyframe first_kfs[i] (to put
    mirrored edges on chosen -- e.g. fixed -- keyframes).  -> (problem, indices of the new points, indices of the new edges)."""
    rs = np.random.RandomState(seed)
    fx, fy, cx, cy = INTRINSICS
    n_kf, n_pt0, n_e0 = len(prob["kf_fixed"]), len(prob["pt_xyz"]), len(prob["edge_kf"])
    bf = float(prob["kf_bf"][0]) if "kf_bf" in prob else 0.0
    inv_sig = _inv_sigma2_table()
    X_new, e_kf, e_pt, e_uv, e_is, e_ur = [], [], [], [], [], []
    while len(X_new) < n:
        i = len(X_new)
        start = int(first_kfs[i]) if i < len(first_kfs) else int(rs.randint(0, n_kf - obs + 1))
        z = -rs.uniform(4.0, 8.0)
        Xc = np.array([rs.uniform(-0.4, 0.4) * z, rs.uniform(-0.3, 0.3) * z, z])
        tp = prob["truth_pose"][start + obs // 2]
        X = tp[:9].reshape(3, 3).T @ (Xc - tp[9:])
        cams = [_truth_cam(prob, k, X) for k in range(start, start + obs)]
        uvs = [(fx * c[0] / c[2] + cx, fy * c[1] / c[2] + cy) for c in cams]
        if not all(c[2] < -1.0 and 8 <= u <= 632 and 8 <= v <= 472 for c, (u, v) in zip(cams, uvs)):
            continue
        for k, c, (u, v) in zip(range(start, start + obs), cams, uvs):
            u, v = u + rs.normal(0.0, sigma), v + rs.normal(0.0, sigma)
            e_kf.append(k); e_pt.append(n_pt0 + i); e_uv.append((u, v)); e_is.append(inv_sig[rs.choice(8)])
            ur = u - bf / c[2] + rs.normal(0.0, sigma)
            e_ur.append(ur if rs.uniform() < stereo_frac else -1.0)
        X_new.append(X)
    X_new = np.array(X_new)
    q = _append_edges(prob, e_kf, e_pt, e_uv, e_is, e_ur)
    q["truth_pt"] = np.concatenate([prob["truth_pt"], X_new])
    q["pt_xyz"] = np.concatenate([prob["pt_xyz"], (X_new + rs.normal(0.0, 0.02, X_new.shape)).astype(np.float32).astype(np.float64)])
    return q, np.arange(n_pt0, n_pt0 + n), np.arange(n_e0, len(q["edge_kf"]))


def ba_mirror_edges(prob, n, seed, sigma=1.0, stereo_frac=0.0):
    """`prob` (synth_map: cameras on a circle looking outward) plus n mirrored observations of EXISTING points: a point on the far
    side of the circle lies behind a keyframe and still projects into its image through the pinhole formula at that negative depth.
    The point keeps its observers in front, so it stays well constrained.  -> (problem, indices of the new edges)."""
    rs = np.random.RandomState(seed)
    fx, fy, cx, cy = INTRINSICS
    tp = prob["truth_pose"]
    R, t = tp[:, :9].reshape(-1, 3, 3), tp[:, 9:]
    Xc = np.einsum("kij,pj->kpi", R, prob["truth_pt"]) + t[:, None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = fx * Xc[..., 0] / Xc[..., 2] + cx, fy * Xc[..., 1] / Xc[..., 2] + cy
    ok = (Xc[..., 2] < -1.0) & (u >= 8) & (u <= 632) & (v >= 8) & (v <= 472)
    cand = np.argwhere(ok)
    pick = cand[np.sort(rs.choice(len(cand), n, replace=False))]
    bf = float(prob["kf_bf"][0]) if "kf_bf" in prob else 0.0
    inv_sig = _inv_sigma2_table()
    e_uv, e_is, e_ur = [], [], []
    for k, p in pick:
        uu, vv = u[k, p] + rs.normal(0.0, sigma), v[k, p] + rs.normal(0.0, sigma)
        e_uv.append((uu, vv)); e_is.append(inv_sig[rs.choice(8)])
        ur = uu - bf / Xc[k, p, 2] + rs.normal(0.0, sigma)
        e_ur.append(ur if rs.uniform() < stereo_frac else -1.0)
    n_e0 = len(prob["edge_kf"])
    q = _append_edges(prob, pick[:, 0], pick[:, 1], e_uv, e_is, e_ur)
    return q, np.arange(n_e0, len(q["edge_kf"]))


def _garble(prob, edges, rs, signs=None):
    """Gross outliers on `edges`: 45 .. 90 px off in u and in v (past the +-30 px of synth_ba's own outliers, so that none cancels),
    signs random or as given."""
    q = dict(prob)
    q["edge_uv"] = prob["edge_uv"].copy()
    if signs is None:
        signs = rs.choice([-1.0, 1.0], (len(edges), 2))
    off = signs * rs.uniform(45.0, 90.0, (len(edges), 2))
    q["edge_uv"][edges] = (q["edge_uv"][edges] + off).astype(np.float32).astype(np.float64)
    if "edge_ur" in prob:
        q["edge_ur"] = prob["edge_ur"].copy()
        st = edges[prob["edge_ur"][edges] >= 0]
        q["edge_ur"][st] = (q["edge_ur"][st] + 700.0 + rs.uniform(20.0, 60.0, len(st))).astype(np.float32).astype(np.float64)   # (stays >= 0: stereo)
    return q


def ba_starve_kf(prob, kf, seed):
    """Every observation of keyframe `kf` replaced by a gross outlier (45 .. 90 px off in u and in v, random signs): no pose fits them,
    the gate sends all of the keyframe's edges to level 1 and the second stage runs without it."""
    return _garble(prob, np.flatnonzero(prob["edge_kf"] == kf), np.random.RandomState(seed))


def ba_starve_pt(prob, one, zero, seed):
    """The points in `one` keep one good observation (their first), the points in `zero` none: the others become gross outliers, so
    that the gate leaves them exactly one / no active edge.  A Huber edge pulls with a bounded force however wrong it is, and four
    such pulls would drag the point off its one good observation until that fails the gate too: the wrong observations of a point
    get signs that cancel in pairs and the coarsest pyramid level's weight, the good one of a point in `one` the finest level's."""
    pattern = np.array([(1.0, 1.0), (-1.0, -1.0), (1.0, -1.0), (-1.0, 1.0)])
    inv_sig = _inv_sigma2_table()
    edges, signs, good = [], [], []
    for p in list(one) + list(zero):
        e = np.flatnonzero(prob["edge_pt"] == p)
        if p in one:
            good.append(e[0])
            e = e[1:]
        edges.append(e)
        signs.append(pattern[np.arange(len(e)) % 4])
    edges = np.concatenate(edges)
    q = _garble(prob, edges, np.random.RandomState(seed), np.concatenate(signs))
    q["edge_inv_sigma2"] = prob["edge_inv_sigma2"].copy()
    q["edge_inv_sigma2"][edges] = float(inv_sig[-1])
    q["edge_inv_sigma2"][good] = float(inv_sig[0])
    return q


def pose_mirror(prob, n_small, n_gross, seed):
    """A synth_pose problem whose first n_small + n_gross correspondences (random ones) are mirrored: the map point lies behind the
    frame (depth -9 .. -3 at the true pose), its keypoint is the pinhole formula at that negative depth plus N(0, 1) px; the last
    n_gross of them are 8 .. 60 px further off.  PoseOptimization has no depth test (Optimizer.cc:239-451): the first kind must stay
    inliers, the second is pruned by chi2 alone.  -> (problem, indices small, indices gross)."""
    rs = np.random.RandomState(seed)
    fx, fy, cx, cy = INTRINSICS
    n = len(prob["uv"])
    idx = rs.choice(n, n_small + n_gross, replace=False)
    m = len(idx)
    z = -rs.uniform(3.0, 9.0, m)
    pc = np.stack([rs.uniform(-0.45, 0.45, m) * z, rs.uniform(-0.35, 0.35, m) * z, z], 1)
    R, t = prob["truth_pose"][:9].reshape(3, 3), prob["truth_pose"][9:]
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    q = dict(prob)
    q["xw"], q["uv"] = prob["xw"].copy(), prob["uv"].copy()
    q["xw"][idx] = f32((pc - t) @ R)
    u = fx * pc[:, 0] / pc[:, 2] + cx + rs.normal(0, 1, m)
    v = fy * pc[:, 1] / pc[:, 2] + cy + rs.normal(0, 1, m)
    u[n_small:] += rs.choice([-1, 1], n_gross) * rs.uniform(8, 60, n_gross)
    v[n_small:] += rs.choice([-1, 1], n_gross) * rs.uniform(8, 60, n_gross)
    q["uv"][idx] = f32(np.stack([u, v], 1))
    if "ur" in prob:
        q["ur"] = prob["ur"].copy()
        ur = f32(u - prob["bf"] / pc[:, 2] + rs.normal(0, 1, m))
        q["ur"][idx] = np.where(prob["ur"][idx] >= 0, ur, -1.0)
    q["truth_outlier"] = prob["truth_outlier"].copy()
    q["truth_outlier"][idx] = np.arange(m) >= n_small
    return q, idx[:n_small], idx[n_small:]


def sim3_mirror(prob, n_small, n_gross, seed):
    """A synth_sim3 problem with n_small + n_gross pairs mirrored: p2 behind camera 2 (depth -9 .. -2.5) and p1 = s R p2 + t behind
    camera 1, both keypoints the pinhole formula at the negative depths plus N(0, 0.7) px; the last n_gross carry a wrong keypoint in
    image 1 (20 .. 60 px off).  OptimizeSim3 has no depth test (Optimizer.cc:1046-1247).  -> (problem, indices small, indices gross)."""
    rs = np.random.RandomState(seed)
    n = prob["n"]
    idx = rs.choice(n, n_small + n_gross, replace=False)
    m = len(idx)
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    z = -rs.uniform(2.5, 9.0, m)
    p2 = f32(np.stack([rs.uniform(-0.4, 0.4, m) * z, rs.uniform(-0.3, 0.3, m) * z, z], 1))
    tr = prob["true"]
    p1 = f32(tr["s"] * (p2 @ tr["R"].T) + tr["t"] + rs.normal(0, 0.01, (m, 3)))
    assert (p1[:, 2] < -1.0).all()
    i1, i2 = prob["intr1"], prob["intr2"]
    o1 = np.stack([i1[0] * p1[:, 0] / p1[:, 2] + i1[2], i1[1] * p1[:, 1] / p1[:, 2] + i1[3]], 1) + rs.normal(0, 0.7, (m, 2))
    o2 = np.stack([i2[0] * p2[:, 0] / p2[:, 2] + i2[2], i2[1] * p2[:, 1] / p2[:, 2] + i2[3]], 1) + rs.normal(0, 0.7, (m, 2))
    o1[n_small:] += rs.choice([-1, 1], (n_gross, 2)) * rs.uniform(20, 60, (n_gross, 2))
    q = dict(prob)
    for k, v in (("p1", p1), ("p2", p2), ("obs1", f32(o1)), ("obs2", f32(o2))):
        q[k] = prob[k].copy()
        q[k][idx] = v
    return q, idx[:n_small], idx[n_small:]


def synth_map_hard(synth_map, mirror=None, starve_kf=()):
    """synth_map(**synth_map) with mirror = dict(n, seed) mirrored observations (ba_mirror_edges) and every (keyframe, seed) of starve_kf
    starved (ba_starve_kf).  -> (problem, indices of the mirrored edges)."""
    prob = _synth_map_fn(**synth_map)
    edges = np.zeros(0, np.int64)
    if mirror:
        prob, edges = ba_mirror_edges(prob, stereo_frac=synth_map.get("stereo_frac", 0.0), **mirror)
    for kf, seed in starve_kf:
        prob = ba_starve_kf(prob, kf, seed)
    return prob, edges


_synth_map_fn = synth_map


def synth_pnp(n=200, outlier_frac=0.3, seed=0, noise_px=0.5):
    """What the PnPsolver constructor gathers for one relocalisation candidate (PnPsolver.cc:67-118): n map points in the world
    frame (p3d = mvP3Dw, float32) and the undistorted keypoints they were matched to (p2d = mvP2D), under a known pose
    Xc = R Xw + t.  The points lie in x [-2, 2], y [-1.5, 1.5], z [2, 10] of the camera frame, the rotation angle is 0.1 .. 1 rad
    and the translation in [-1, 1]^3; the keypoints carry noise_px of Gaussian noise, a share outlier_frac of them lie anywhere in
    the 640 x 480 image.  Every keypoint sits on an octave 0 .. 7: sigma2 = 1.44^octave and max_err = (float)(sigma2 * 5.991), the
    bound of mvMaxError.  Layout of slamit_pnp_problem (without quads)."""
    rs = np.random.RandomState(17000 + seed)
    f32 = np.float32
    intr = np.array([500.0, 500.0, 320.0, 240.0], np.float64)
    Xc = np.stack([rs.uniform(-2, 2, n), rs.uniform(-1.5, 1.5, n), rs.uniform(2, 10, n)], 1)
    axis = rs.normal(0, 1, 3)
    axis /= np.linalg.norm(axis)
    R, _ = se3_exp(np.concatenate([axis * rs.uniform(0.1, 1.0), np.zeros(3)]))
    t = rs.uniform(-1, 1, 3)
    Xw = (Xc - t) @ R                                   # R^T (Xc - t)
    uv = np.stack([intr[0] * Xc[:, 0] / Xc[:, 2] + intr[2], intr[1] * Xc[:, 1] / Xc[:, 2] + intr[3]], 1) + rs.normal(0, noise_px, (n, 2))
    bad = rs.rand(n) < outlier_frac
    nb = int(bad.sum())
    uv[bad] = np.stack([rs.uniform(0, 640, nb), rs.uniform(0, 480, nb)], 1)
    octave = rs.randint(0, 8, n)
    sigma2 = (f32(1.44) ** octave.astype(f32)).astype(f32)
    th2 = f32(5.991)
    return dict(n=n, p3d=Xw.astype(f32), p2d=uv.astype(f32), sigma2=sigma2, max_err=(sigma2 * th2).astype(f32), intr=intr, th2=float(th2),
                true=dict(R=R, t=t, bad=bad))


def synth_unproject(seed=0, n=300, n_candidates=None, n_close=None, min_points=100, mode=0, ctor=0, n_levels=8, quantised=True, tracked_frac=0.4,
                    octave_bad_frac=0.06, specials=True, tie_at_cut=False, exact_th=False, all_equal=False, width=640, height=480):
    """What Tracking::UpdateLastFrame / CreateNewKeyFrame / StereoInitialization hold for one stereo or RGB-D frame
    (Tracking.cc:1039-1091, :1334-1396, :712-727): a posed pinhole frame (mRwc, mOw, fx .. invfy), n undistorted keypoints with
    their octaves, their measured depths and the flags of the keypoints that carry a tracked map point.  n_candidates keypoints have
    a depth > 0, n_close of those have !(depth > th_depth); the others hold what a frame holds without one: -1, and with `specials`
    also 0, -0 and NaN, while one candidate is a denormal (mode CLOSEST only, and tracked) and one is +inf (in place of a close and of a
    far depth).
    quantised: depths are multiples of th_depth / 64, so that equal depths are the rule, as on an RGB-D map; else float32 uniform.
    tie_at_cut: the keypoints at walk positions max(c, min_points) - 1 .. + 2 (where they exist and are all far or all close) get the
    depth of position max(c, min_points), so that the index decides which of them is visited.  exact_th: one close depth equals
    th_depth.  all_equal: every candidate has depth th_depth.  A share octave_bad_frac of the octaves is -1 or n_levels (the level
    outside the table).  Layout of slamit_unproject_problem."""
    rs = np.random.RandomState(21000 + seed)
    f32 = np.float32
    fx, fy, cx, cy = f32(517.3), f32(516.5), f32(318.6), f32(255.3)
    invfx, invfy = f32(1.0) / fx, f32(1.0) / fy
    R, t = se3_exp(np.concatenate([rs.uniform(-0.4, 0.4, 3), rs.uniform(-2.0, 2.0, 3)]))
    Rcw, tcw = R.astype(f32), t.astype(f32)
    Rwc = np.ascontiguousarray(Rcw.T)
    Ow = (-(Rcw.astype(np.float64).T @ tcw.astype(np.float64))).astype(f32)
    th = f32(3.25)
    step = f32(3.25 / 64.0)   # 13 / 256: every multiple below 2^11 steps is exact in float32
    M = int(round(0.85 * n)) if n_candidates is None else int(n_candidates)
    M = max(0, min(M, n))
    c = M // 2 if n_close is None else int(n_close)
    c = max(0, min(c, M))
    if quantised:
        close = (rs.randint(1, 65, c).astype(f32) * step).astype(f32)
        far = (rs.randint(65, 600, M - c).astype(f32) * step).astype(f32)
    else:
        close = rs.uniform(0.3, 3.2, c).astype(f32)
        far = rs.uniform(3.3, 40.0, M - c).astype(f32)
    if all_equal:
        close[:] = th
        far[:] = th   # then they are close too: the true counts are in the result
    if exact_th and c > 0:
        close[0] = th
    if specials and not all_equal:
        if c > 1 and mode == 0:
            close[1] = f32(1e-41)        # a denormal: the closest of all, so always visited; it carries a tracked point (below), because
                                         # unprojected it falls on the camera centre, where Pos - Ow is zero and the normal a NaN
        if M - c > 1:
            far[1] = f32(np.inf)
    depth = np.full(n, -1.0, f32)
    cand = rs.permutation(n)[:M]
    depth[cand] = np.concatenate([close, far])[rs.permutation(M)] if M else depth[cand]
    rest = np.setdiff1d(np.arange(n), cand)
    if specials and len(rest) >= 4:
        depth[rest[0]], depth[rest[1]], depth[rest[2]] = f32(0.0), f32(-0.0), f32(np.nan)
    if tie_at_cut and not all_equal:
        key = sorted((float(depth[i]), int(i)) for i in cand if not np.isinf(depth[i]))
        cc = sum(1 for d, _ in key if not d > float(th))
        p = max(cc, min_points)
        if p < len(key):
            for q in (p - 1, p + 1, p + 2):
                if 0 <= q < len(key) and (q >= cc) == (p >= cc):
                    depth[key[q][1]] = depth[key[p][1]]
    kps = np.zeros(n, KP_DTYPE)
    kps["x"] = rs.uniform(0.0, width, n).astype(f32)
    kps["y"] = rs.uniform(0.0, height, n).astype(f32)
    octave = rs.randint(0, n_levels, n).astype(np.int32)
    pick = rs.rand(n)
    octave[pick < octave_bad_frac / 2] = -1
    octave[pick > 1.0 - octave_bad_frac / 2] = n_levels
    kps["octave"] = octave
    kps["size"], kps["angle"], kps["class_id"] = 31.0, rs.uniform(0, 360, n).astype(f32), -1
    tracked = (rs.rand(n) < tracked_frac).astype(np.uint8)
    tracked[depth.view(np.uint32) - 1 < 0x007fffff] = 1
    scale_f = (f32(1.2) ** np.arange(n_levels, dtype=f32)).astype(f32)
    return dict(n=n, fx=fx, fy=fy, cx=cx, cy=cy, invfx=invfx, invfy=invfy, Rwc=Rwc.reshape(9), Ow=Ow, th_depth=th, min_points=int(min_points),
                mode=int(mode), ctor=int(ctor), n_levels=int(n_levels), scale_factors=scale_f, kps_un=kps, depth=depth, tracked=tracked)


KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])   # api.KP_DTYPE


def synth_rgbd(seed=0, n=300, width=64, height=48, kind="u16", factor=1.0 / 5000.0, pad=0, zero_frac=0.15, outside=True):
    """What Frame::ComputeStereoFromRGBD reads (Frame.cc:766-787): a depth plane of `kind` "u16" (raw sensor units, factor
    1 / DepthMapFactor) or "f32" whose rows are `pad` elements longer than `width` (the padding holds a value no keypoint may read),
    n raw keypoints with fractional coordinates, their undistorted twins a little beside them, and mbf.  A share zero_frac of the
    pixels has no measurement (0).  The first keypoints sit on the last row, the last column, both, and on a zero pixel; with
    `outside`, three more lie off the plane (x = width, y = -1.5, x = NaN).  The plane is quantised (a u16 map is; the f32 one is made
    the same way), so equal depths are the rule.  Layout of slamit_rgbd_problem; `plane` is the (height, width) view of `storage`."""
    rs = np.random.RandomState(22000 + seed)
    f32 = np.float32
    raw = rs.randint(400, 60000, (height, width))
    raw[rs.rand(height, width) < zero_frac] = 0
    raw[0, 0] = 0
    if kind == "u16":
        storage = np.full((height, width + pad), 65535, np.uint16)
        storage[:, :width] = raw.astype(np.uint16)
    else:
        storage = np.full((height, width + pad), -7.0, f32)
        storage[:, :width] = (raw.astype(f32) * f32(1.0 / 5000.0)).astype(f32) if factor == 1.0 else raw.astype(f32)
    kps = np.zeros(n, KP_DTYPE)
    kps["x"] = rs.uniform(0.0, width - 0.001, n).astype(f32)
    kps["y"] = rs.uniform(0.0, height - 0.001, n).astype(f32)
    fixed = [(width - 0.25, 3.5), (5.5, height - 0.5), (width - 1.0, height - 1.0), (0.75, 0.25), (-0.5, -0.99)]
    if outside:
        fixed += [(float(width), 2.0), (3.0, -1.5), (np.nan, 1.0), (2.0, float(height)), (3.0e9, 1.0)]
    for i, (x, y) in enumerate(fixed[:n]):
        kps["x"][i], kps["y"][i] = f32(x), f32(y)
    kps["octave"], kps["class_id"], kps["size"] = rs.randint(0, 8, n), -1, 31.0
    kps_un = kps.copy()
    kps_un["x"] = (kps["x"] + rs.uniform(-1.5, 1.5, n).astype(f32)).astype(f32)
    kps_un["y"] = (kps["y"] + rs.uniform(-1.5, 1.5, n).astype(f32)).astype(f32)
    return dict(n=n, storage=storage, plane=storage[:, :width], width=width, height=height, kind=kind, factor=f32(factor), mbf=f32(38.6),
                kps=kps, kps_un=kps_un)


def _rodrigues(w):
    th = float(np.sqrt((w * w).sum()))
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], np.float64)
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / (th * th) * (K @ K)


def synth_essential(n_kf=12, seed=0, drift=0.004, scale_drift=0.01, fix_scale=False, n_corrected=3, n_pt=60, mixed=False, chain=False,
                    min_feat=100):
    """A loop closure for Optimizer::OptimizeEssentialGraph (slamit_eg_graph + slamit_eg_problem without its edge list, which
    slamit_essential_plan derives from the tables here).  n_kf keyframes on a ring (one camera per slot, looking along the tangent),
    the map's poses drifted step by step (rotation noise `drift` rad, translation noise, and a scale that grows by `scale_drift` per
    step unless fix_scale), float32-rounded and widened as Converter::toMatrix3d does.  The last keyframe is pCurKF, slot 0 pLoopKF:
    CorrectedSim3 holds pCurKF (its true pose, at the drifted scale) and its n_corrected spanning-tree ancestors (propagated as
    LoopClosing::CorrectLoop does, Sic * CorrectedScw), NonCorrectedSim3 their map poses.  Spanning tree: slot i's parent is i - 1;
    covisibility rows: the neighbours at distance 1, 2, 3 along the ring with weights around min_feat; LoopConnections: the
    corrected keyframes to the first slots.  chain=True leaves only the tree and the one (cur, loop) connection: the ceiling's graph.

    mixed=True adds what eg_mixed40 covers: a bad keyframe (a slot without a vertex), mnIds that are not the slots' order, an old loop
    edge, a spanning-tree edge beside a LoopConnections edge of the same pair, covisibility pairs that LoopConnections inserted
    first, a row whose weights are all >= min_feat (GetCovisiblesByWeight returns nothing for it), and points whose
    mnCorrectedByKF is pCurKF (their reference slot is then a corrected keyframe's)."""
    rs = np.random.RandomState(0xE55E + 7919 * seed + n_kf)
    n = int(n_kf)
    cur, loop = n - 1, 0
    T = []
    for i in range(n):
        a = 2 * np.pi * i / n
        Rwc = _rodrigues(np.array([0.0, 0.0, a])) @ _rodrigues(np.array([0.1 * np.sin(3 * a), 0.0, 0.0]))
        C = np.array([5 * np.cos(a), 5 * np.sin(a), 0.3 * np.sin(2 * a)])
        R = Rwc.T
        T.append((R, -R @ C))
    Td = [T[0]]
    sc = 1.0
    for i in range(1, n):
        Rrel = T[i][0] @ T[i - 1][0].T
        trel = T[i][1] - Rrel @ T[i - 1][1]
        if not fix_scale:
            sc *= 1.0 + scale_drift
        Rrel = _rodrigues(rs.normal(0, drift, 3)) @ Rrel
        trel = sc * trel + rs.normal(0, drift, 3)
        Td.append((Rrel @ Td[-1][0], Rrel @ Td[-1][1] + trel))
    f32 = lambda x: np.asarray(x, np.float32).astype(np.float64)
    scw_r = np.stack([f32(R).reshape(9) for R, _ in Td])
    scw_t = np.stack([f32(t) for _, t in Td])
    scw_s = np.ones(n)
    snc_r, snc_t, snc_s = scw_r.copy(), scw_t.copy(), scw_s.copy()
    s_c = sc   # the map near pCurKF has grown by sc: Scw = (R, sc t, sc) takes a loop-side point into its units
    Rc, tc = T[cur][0], T[cur][1]
    corrected = [cur - k for k in range(min(n_corrected, n - 2) + 1)]
    for i in corrected:   # Sic = Tiw * Twc (map poses), CorrectedSiw = Sic * CorrectedScw (LoopClosing.cc:447-460)
        Ri, ti = scw_r[i].reshape(3, 3), scw_t[i]
        Rcm, tcm = scw_r[cur].reshape(3, 3), scw_t[cur]
        Ric = Ri @ Rcm.T
        tic = ti - Ric @ tcm
        scw_r[i] = (Ric @ Rc).reshape(9)
        scw_t[i] = Ric @ (s_c * tc) + tic   # the Sim3 product with s_ic = 1: t = R_ic t_c + t_ic, s = s_c
        scw_s[i] = s_c
    kf_id = np.arange(n, dtype=np.int32)
    kf_bad = np.zeros(n, np.uint8)
    parent = np.arange(-1, n - 1, dtype=np.int32)
    loop_edges = [[] for _ in range(n)]
    covis = [dict() for _ in range(n)]
    if not chain:
        for i in range(n):
            for d, w in ((1, 2 * min_feat + 37), (2, min_feat + 20), (3, min_feat - 25)):
                for j in (i - d, i + d):
                    if 0 <= j < n:
                        covis[i][j] = w + int((i + j) % 5)
    conn = {}
    if chain:
        conn[cur] = [loop]
    else:
        for i in corrected[:3]:
            conn[i] = [j for j in (loop, loop + 1, loop + 2) if j < corrected[-1] - 1]
        for i in conn:
            for j in conn[i]:
                w = min_feat + 30 if (i + j) % 2 == 0 or (i == cur and j == loop) else min_feat - 40
                if i == cur and j == loop:
                    w = min_feat - 10   # the pair that is exempt from the weight gate
                covis[i][j] = covis[j][i] = w
    if mixed:
        assert n >= 24
        kf_bad[n // 2] = 1
        kf_id = (3 * np.arange(n) + 5).astype(np.int32)
        kf_id[[7, 8]] = kf_id[[8, 7]]                      # mnId order differs from slot order
        parent[n // 2 + 1] = n // 2 - 1                    # the bad keyframe's child was re-parented (SetBadFlag)
        parent[8], parent[7] = 6, 8                        # the parent has the smaller mnId
        for j in list(covis[n // 2]):
            covis[j].pop(n // 2, None)
        covis[n // 2] = {}
        loop_edges[n - 10].append(4)                       # an old loop: n - 10 <-> 4
        loop_edges[4].append(n - 10)
        covis[n - 10][4] = covis[4][n - 10] = min_feat + 50  # ... which also see each other (excluded by sLoopEdges.count)
        parent[cur - 1] = loop + 1                         # a tree edge beside the LoopConnections edge of the same pair
        conn.setdefault(cur - 1, [])
        if loop + 1 not in conn[cur - 1]:
            conn[cur - 1].append(loop + 1)
        covis[cur - 1][loop + 1] = covis[loop + 1][cur - 1] = min_feat + 60
        covis[15] = {j: w + min_feat for j, w in covis[15].items()}   # no weight below min_feat: the row yields nothing
    children = [[] for _ in range(n)]
    for i in range(n):
        if parent[i] >= 0 and not kf_bad[i]:
            children[parent[i]].append(i)
    row_cap = max(1, max(len(c) for c in covis))
    ord_kf = -np.ones((n, row_cap), np.int32)
    ord_w = np.zeros((n, row_cap), np.int32)
    ord_n = np.zeros(n, np.int32)
    for i in range(n):
        row = sorted(covis[i].items(), key=lambda jw: (-jw[1], jw[0]))
        ord_n[i] = len(row)
        for k, (j, w) in enumerate(row):
            ord_kf[i, k], ord_w[i, k] = j, w

    def csr(rows):
        ptr = np.zeros(n + 1, np.int32)
        flat = []
        for i in range(n):
            flat += sorted(rows[i])
            ptr[i + 1] = len(flat)
        return ptr, np.array(flat, np.int32).reshape(-1)

    child_ptr, child_kf = csr(children)
    loop_ptr, loop_list = csr(loop_edges)
    conn_ptr, conn_kf = csr([conn.get(i, []) for i in range(n)])
    fixed = np.zeros(n, np.uint8)
    fixed[loop] = 1
    good_kf = np.flatnonzero(kf_bad == 0)
    pt_ref = good_kf[rs.randint(0, len(good_kf), n_pt)].astype(np.int32)
    if mixed:
        pt_ref[: n_pt // 4] = np.array(corrected, np.int32)[rs.randint(0, len(corrected), n_pt // 4)]   # mnCorrectedByKF == pCurKF
    pt_pos = np.zeros((n_pt, 3), np.float32)
    for p in range(n_pt):   # a few metres in front of the reference keyframe, in the MAP's (drifted) frame
        R, t = Td[pt_ref[p]]
        pt_pos[p] = (R.T @ (np.array([rs.uniform(-1, 1), rs.uniform(-1, 1), rs.uniform(2, 6)]) - t)).astype(np.float32)
    pt_bad = (rs.uniform(size=n_pt) < 0.1).astype(np.uint8)
    return dict(n_kf=n, row_cap=row_cap, loop_kf=loop, cur_kf=cur, min_feat=min_feat, kf_bad=kf_bad, kf_id=kf_id, kf_parent=parent,
                child_ptr=child_ptr, child_kf=child_kf, loop_ptr=loop_ptr, loop_kf_list=loop_list, ord_kf=ord_kf, ord_w=ord_w,
                ord_n=ord_n, conn_ptr=conn_ptr, conn_kf=conn_kf,
                scw_r=scw_r, scw_t=scw_t, scw_s=scw_s, snc_r=snc_r, snc_t=snc_t, snc_s=snc_s, fixed=fixed, bad=kf_bad.copy(),
                fix_scale=int(bool(fix_scale)), max_its=20, lambda_init=1e-16, pt_pos=pt_pos, pt_ref=pt_ref, pt_bad=pt_bad)


SIM3_PROBE_FAMILIES = ("gn", "damped", "fixscale", "noturn", "edges", "twoedge")


def synth_sim3_probes(family, n_pairs=48, seed=0):
    """A slamit_eg_problem (edge list included, written by hand: no planner) that probes the Sim3 algebra of the essential-graph
    optimisation branch by branch.  n_pairs disjoint pairs: keyframe 2p is fixed, 2p + 1 free, one NORMAL edge (2p, 2p + 1), so the
    system is block diagonal and the error of pair p, log(Snc_j Snc_i^-1 Scw_i Scw_j^-1), is set freely: Snc_i = Scw_i, and
    Snc_j = D Scw_j with D = (R(theta axis), t, exp(sigma)) the pair's relative error.  Rotations and translations are float32-rounded
    and widened as in synth_essential (so a stated theta holds to about 1e-7 rad); scales stay doubles (sigma = 0 is exact).

    Absolute orientations cycle over four kinds, which select the four branches of Quaterniond(R): generic (trace > 0), and within
    0.05 rad of pi about x, about y, about z.  Every keyframe is the reference of one good point; one bad point is appended.

    family: `damped` (theta 0.3 .. 2.5 rad about random axes, sigma +-(0.2 .. 1), a translation error of 0.4 .. 1.2 units, keyframes
    within a unit of the origin; lambda_init 1), `gn` (the same pairs with the angles mapped into 0.3 .. 1.5, lambda_init 1e-16),
    `fixscale` (theta 0.3 .. 2.0, every scale 1, fix_scale; every other edge is (2p + 1, 2p), the free keyframe first), `noturn` (rotation error identity or 3e-6 / 9e-6 rad, sigma +-(0.2 .. 1), a
    third of the pairs with sigma = 0: pure translation, 1 .. 3 units), `edges` (theta in {0.9e-5, 1.1e-5, 4.4e-3, 4.6e-3} x sigma in
    {+-0.9e-5, +-1.1e-5, 0.3}: both sides of every threshold of exp and log), `twoedge` (noturn's rotations with sigma +-(0.2 .. 1)
    on every pair, and per pair a second fixed keyframe 2 n_pairs + p with a second edge to the free one that turns by 0.3 .. 1.5 rad:
    144 keyframes, 96 edges, still block diagonal).  max_its 1.  The sizes are the largest at which the
    reference's g2o and the numpy restatement still agree to 1e-6 (tests/sim3_probe_checks.PROBE_WORST)."""
    assert family in SIM3_PROBE_FAMILIES
    P = int(n_pairs)
    n = 2 * P
    rs = np.random.RandomState(0x51B3 + 101 * seed)   # the same stream for every family: gn and damped are the same pairs
    f32 = lambda x: np.asarray(x, np.float32).astype(np.float64)

    def unit(rs=rs):
        v = rs.normal(size=3)
        return v / np.sqrt((v * v).sum())

    flips = (None, np.diag([1.0, -1.0, -1.0]), np.diag([-1.0, 1.0, -1.0]), np.diag([-1.0, -1.0, 1.0]))

    def orientation(kind, rs=rs):
        if kind == 0:
            return _rodrigues(unit(rs) * rs.uniform(0.2, 1.8))   # below 2 pi / 3: trace > 0
        return flips[kind] @ _rodrigues(unit(rs) * rs.uniform(0.005, 0.05))

    kind_i, kind_j = rs.permutation(np.arange(P) % 4), rs.permutation(np.arange(P) % 4)
    Ri = [orientation(k) for k in kind_i]
    Rj = [orientation(k) for k in kind_j]
    ti, tj = rs.uniform(-1, 1, (P, 3)), rs.uniform(-1, 1, (P, 3))
    axis = np.stack([unit() for _ in range(P)])
    theta = rs.uniform(0.3, 2.5, P)
    sign = np.where(rs.uniform(size=P) < 0.5, -1.0, 1.0)
    sigma = sign * rs.uniform(0.2, 1.0, P)
    td = np.stack([unit() for _ in range(P)]) * rs.uniform(0.4, 1.2, P)[:, None]
    fix_scale, lambda_init = 0, 1.0
    p = np.arange(P)
    if family == "gn":
        # the undamped step carries the noise of the 1e-9 differences in full, in proportion to the error's size: beyond 1.5 rad the
        # reference's g2o and the numpy restatement land more than 1e-6 apart (2.1e-6 at 2.5 rad), so gn maps the angles into 0.3 .. 1.5
        lambda_init, theta = 1e-16, 0.3 + (theta - 0.3) * (1.2 / 2.2)
    elif family == "fixscale":
        # (angles into 0.3 .. 2.0: a reversed pair's translation error is the larger one, and with it beyond 2 rad the reference and the
        # restatement part by 2e-6)
        sigma, fix_scale, theta = np.zeros(P), 1, 0.3 + (theta - 0.3) * (1.7 / 2.2)
    elif family == "noturn":
        theta = np.array([0.0, 3e-6, 9e-6])[p % 3]
        sigma = np.where((p // 3) % 3 == 2, 0.0, sigma)
        td = 2.5 * td   # 1 .. 3 units: with W = C I the translation is all these pairs have, and they stay well conditioned
    elif family == "twoedge":
        theta, td = np.array([0.0, 3e-6, 9e-6])[p % 3], 2.5 * td
    elif family == "edges":
        c = p % 20
        theta = np.array([0.9e-5, 1.1e-5, 4.4e-3, 4.6e-3])[c % 4]
        sigma = np.array([0.9e-5, -0.9e-5, 1.1e-5, -1.1e-5, 0.3])[c // 4]
        # |sigma| just above the threshold with a small theta takes sim3.h's B = (sigma^2 / 2 - sigma + 1) s / sigma^3, which lacks the
        # series' "- 1": 7.5e14 at 1.1e-5, so W = C + A O + B O^2 has a condition of 1e5 .. 1e10 at these thetas and any translation
        # makes the reference's own 1e-9 differences rounding noise.  Those pairs carry an error without translation, exactly.
        still = np.abs(np.abs(sigma) - 1.1e-5) < 1e-12
        td[still], tj[still] = 0.0, 0.0
    scw_r, scw_t, scw_s = np.zeros((n, 9)), np.zeros((n, 3)), np.ones(n)
    for q in range(P):
        scw_r[2 * q], scw_r[2 * q + 1] = f32(Ri[q]).reshape(9), f32(Rj[q]).reshape(9)
        scw_t[2 * q], scw_t[2 * q + 1] = f32(ti[q]), f32(tj[q])
    snc_r, snc_t, snc_s = scw_r.copy(), scw_t.copy(), scw_s.copy()
    for q in range(P):
        j = 2 * q + 1
        sd = float(np.exp(sigma[q]))
        if theta[q] != 0.0:
            Rd = _rodrigues(axis[q] * theta[q])
            snc_r[j] = f32(Rd @ Rj[q]).reshape(9)
        else:
            Rd = np.eye(3)   # (the rotation kept bit for bit: the error's rotation is the identity)
        snc_t[j] = f32(sd * (Rd @ scw_t[j]) + td[q])
        snc_s[j] = sd * scw_s[j]
    fixed = np.zeros(n, np.uint8)
    fixed[0::2] = 1
    v0, v1 = 2 * p, 2 * p + 1
    if family == "fixscale":
        # every other pair reversed, the free keyframe as vertex 0: a scale perturbation of vertex 1 leaves the translation of an error
        # with sigma = 0 alone, so nothing there couples into coordinate 6 and a fix_scale that is not honoured would go unseen
        v0, v1 = np.where(p % 2 == 1, v1, v0), np.where(p % 2 == 1, v0, v1)
    if family == "twoedge":
        # a second fixed keyframe n + p per pair and a second edge (n + p, 2 p + 1): Scw_k = Snc_k G with G a rotation by 0.3 .. 1.5 rad
        # and a short translation, so its error is Snc_j (Snc_k^-1 Scw_k) Scw_j^-1 = D Scw_j G Scw_j^-1, which turns by G's angle.  The
        # first edge's small-theta coefficients then stand in the free keyframe's H beside a gradient that is not small.  (A single edge
        # cannot show A10 to first order: its cost holds A only as A^2 theta^2, theta < 4.5e-3.)
        rs2 = np.random.RandomState(0x2ED6 + 101 * seed)   # its own stream: the pairs stay those of the other families
        Rk = [orientation(k, rs2) for k in rs2.permutation(np.arange(P) % 4)]
        Rg = [_rodrigues(unit(rs2) * a) for a in rs2.uniform(0.3, 1.5, P)]
        tg = np.stack([unit(rs2) for _ in range(P)]) * rs2.uniform(0.1, 0.3, P)[:, None]
        tk = rs2.uniform(-1, 1, (P, 3))
        kr, kt = np.stack([f32(R).reshape(9) for R in Rk]), f32(tk)
        scw_r, snc_r = np.concatenate([scw_r, np.stack([f32(Rk[q] @ Rg[q]).reshape(9) for q in range(P)])]), np.concatenate([snc_r, kr])
        scw_t, snc_t = np.concatenate([scw_t, f32(np.stack([Rk[q] @ tg[q] for q in range(P)]) + kt)]), np.concatenate([snc_t, kt])
        scw_s, snc_s = np.concatenate([scw_s, np.ones(P)]), np.concatenate([snc_s, np.ones(P)])
        fixed = np.concatenate([fixed, np.ones(P, np.uint8)])
        v0, v1 = np.concatenate([v0, n + p]), np.concatenate([v1, 2 * p + 1])
        n += P
    pt_ref = np.concatenate([np.arange(n), [1]]).astype(np.int32)
    pt_pos = np.zeros((n + 1, 3), np.float32)
    for k in range(n + 1):   # a few metres in front of the reference keyframe
        R, t = scw_r[pt_ref[k]].reshape(3, 3), scw_t[pt_ref[k]]
        pt_pos[k] = (R.T @ (np.array([rs.uniform(-1, 1), rs.uniform(-1, 1), rs.uniform(2, 6)]) - t)).astype(np.float32)
    pt_bad = np.zeros(n + 1, np.uint8)
    pt_bad[n] = 1
    return dict(n_kf=n, scw_r=scw_r, scw_t=scw_t, scw_s=scw_s, snc_r=snc_r, snc_t=snc_t, snc_s=snc_s, fixed=fixed, bad=np.zeros(n, np.uint8),
                edge_v0=v0.astype(np.int32), edge_v1=v1.astype(np.int32), edge_kind=np.zeros(len(v0), np.int32),
                fix_scale=fix_scale, max_its=1, lambda_init=lambda_init, pt_pos=pt_pos, pt_ref=pt_ref, pt_bad=pt_bad)
