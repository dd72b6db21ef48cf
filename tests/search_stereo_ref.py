"""A numpy restatement of the guided-search loop WITH the right-image gate of the three stereo drivers, the
reference's own way: grid cells x-major then y, keypoints in insertion order, best / second with strict '<', taken marks set
inside the loop.  float32 where the reference has floats.

    er_mode 0  the monocular loop (ORBmatcher.cc:85-128)
    er_mode 1  RADIUS  :93-98, :1411-1417   mvuRight[idx] > 0 : skip when fabs(q_ur - mvuRight[idx]) > r    (a NaN passes)
    er_mode 2  CHI2    :918-942             mvuRight[idx] >= 0: e2 = ex^2 + ey^2 + er^2 against chi2_gate_stereo (7.8),
                                            else the two-term e2 against chi2_gate (5.99); only with chi2_gate > 0

The CPU tests pin it to oracle.bindings.guided_search where no keypoint is stereo; the GPU tests compare the device with it."""
import numpy as np

GRID_COLS, GRID_ROWS = 64, 48
f32 = np.float32


def _roundf(v):
    """C roundf on a float32 array: half away from zero."""
    t = np.trunc(v)
    return np.where(np.abs(v - t) >= f32(0.5), t + np.sign(v), t)


def _popcount_rows(a):
    return np.unpackbits(a, axis=1).sum(axis=1).astype(np.int64)


def guided_search(frame, queries, th_dist=100, use_ratio=True, nnratio=0.8, chi2_gate=0.0, inv_level_sigma2=None, er_mode=0,
                  kp_ur=None, q_ur=None, q_ur_stride=1, chi2_gate_stereo=7.8, stats=None):
    """-> (match_kp (m) int32, nmatches, out4 (m, 4) int32) as api.ORBmatcher.guided_search returns them.  stats: a dict that
    receives gate_removed_best = the number of queries whose Hamming-best candidate among the free keypoints that pass every
    monocular test was removed by the right-image test, and candidates (m) = the keypoints of each query's window that pass every
    test but the taken mark and the descriptor distance (what the device counts against its stored list), and rewalks_over_128 =
    the queries with more than 128 of those whose best or second-best free-on-entry candidate an earlier query of the call took:
    the device answers these by walking the frame's keypoints again, gate included."""
    xy = np.ascontiguousarray(frame["kp_xy"], f32).reshape(-1, 2)
    octave = np.ascontiguousarray(frame["kp_octave"], np.int32)
    desc = np.ascontiguousarray(frame["desc"], np.uint8).reshape(-1, 32)
    taken = np.ascontiguousarray(frame["kp_taken"], np.uint8).astype(bool).copy()
    taken0 = taken.copy()
    min_x, min_y, inv_w, inv_h = (f32(frame[k]) for k in ("min_x", "min_y", "inv_w", "inv_h"))
    uvr = np.ascontiguousarray(queries["uvr"], f32).reshape(-1, 3)
    m, n = len(uvr), len(xy)
    lmin = np.ascontiguousarray(queries["level_min"], np.int32)
    lmax = np.ascontiguousarray(queries["level_max"], np.int32)
    qdesc = np.ascontiguousarray(queries["desc"], np.uint8).reshape(-1, 32)
    valid = np.ascontiguousarray(queries.get("valid", np.ones(m)), np.uint8)
    takes = np.ascontiguousarray(queries.get("takes", np.ones(m)), np.uint8)
    sig = np.ones(16, f32)
    if inv_level_sigma2 is not None:
        v = np.asarray(inv_level_sigma2, f32)[:16]
        sig[:len(v)] = v
    nnratio, chi2_gate, chi2_gate_stereo = f32(nnratio), f32(chi2_gate), f32(chi2_gate_stereo)
    if er_mode:
        kur = np.ascontiguousarray(kp_ur, f32).reshape(-1)
        qur = np.ascontiguousarray(q_ur, f32).reshape(-1)
    # Frame::AssignFeaturesToGrid / PosInGrid
    with np.errstate(invalid="ignore"):
        posx = _roundf((xy[:, 0] - min_x) * inv_w).astype(np.int64)
        posy = _roundf((xy[:, 1] - min_y) * inv_h).astype(np.int64)
    ingrid = ~((posx < 0) | (posx >= GRID_COLS) | (posy < 0) | (posy >= GRID_ROWS))
    scan_rank = np.lexsort((np.arange(n), posy, posx))   # cells x-major, then y, then the keypoint index

    match = np.full(m, -1, np.int32)
    out4 = np.tile(np.array([256, -1, 256, -1], np.int32), (m, 1))
    nmatches, removed_best, rewalks = 0, 0, 0
    ncand = np.zeros(m, np.int64)
    for q in range(m):
        if not valid[q]:
            continue
        x, y, r = uvr[q]
        c0x = max(0, int(np.floor((x - min_x - r) * inv_w)))
        if c0x >= GRID_COLS:
            continue
        c1x = min(GRID_COLS - 1, int(np.ceil((x - min_x + r) * inv_w)))
        if c1x < 0:
            continue
        c0y = max(0, int(np.floor((y - min_y - r) * inv_h)))
        if c0y >= GRID_ROWS:
            continue
        c1y = min(GRID_ROWS - 1, int(np.ceil((y - min_y + r) * inv_h)))
        if c1y < 0:
            continue
        distx, disty = xy[:, 0] - x, xy[:, 1] - y
        hit = ingrid & (posx >= c0x) & (posx <= c1x) & (posy >= c0y) & (posy <= c1y)
        hit &= ~(octave < lmin[q])
        if lmax[q] >= 0:
            hit &= ~(octave > lmax[q])
        hit &= (np.abs(distx) < r) & (np.abs(disty) < r)
        # the per-candidate tests of the three loops; the taken test (:89-91) comes first there, which changes nothing
        free = ~taken
        e2 = distx * distx + disty * disty
        if chi2_gate > 0:
            two_term = ~(e2 * sig[octave & 15] > chi2_gate)
        else:
            two_term = np.ones(n, bool)
        gate = two_term
        if er_mode == 1:
            with np.errstate(invalid="ignore"):
                er = np.abs(qur[q * q_ur_stride] - kur)
                gate = two_term & ~((kur > 0) & (er > r))
        elif er_mode == 2 and chi2_gate > 0:
            with np.errstate(invalid="ignore"):
                er = qur[q * q_ur_stride] - kur
                e3 = e2 + er * er
                gate = np.where(kur >= 0, ~(e3 * sig[octave & 15] > chi2_gate_stereo), two_term)
        ok = hit & free & gate
        ncand[q] = int((hit & gate).sum())
        if not hit.any():
            continue
        idxs = scan_rank[ok[scan_rank]]
        if stats is not None and er_mode:
            base = scan_rank[(hit & free & two_term)[scan_rank]]
            if len(base):
                d0 = _popcount_rows(desc[base] ^ qdesc[q])
                b0 = base[int(np.argmin(d0))]   # argmin: the first of the smallest, as the strict '<' keeps it
                if d0.min() < 256 and not ok[b0]:
                    removed_best += 1
        if stats is not None and ncand[q] > 128:
            entry = scan_rank[(hit & ~taken0 & gate)[scan_rank]]
            if len(entry):
                order = np.argsort(_popcount_rows(desc[entry] ^ qdesc[q]), kind="stable")[:2]
                rewalks += bool(taken[entry[order]].any())
        best, best_l, best2, best2_l, best_i = 256, -1, 256, -1, -1
        if len(idxs):
            d = _popcount_rows(desc[idxs] ^ qdesc[q])
            for j in range(len(idxs)):
                dist = int(d[j])
                if dist < best:
                    best2, best2_l = best, best_l
                    best, best_l, best_i = dist, int(octave[idxs[j]]), int(idxs[j])
                elif dist < best2:
                    best2, best2_l = dist, int(octave[idxs[j]])
        out4[q] = (best, best_l, best2, best2_l)
        if best <= th_dist:
            if use_ratio and best_l == best2_l and f32(best) > nnratio * f32(best2):
                continue
            match[q] = best_i
            if takes[q]:
                taken[best_i] = True
            nmatches += 1
    if stats is not None:
        stats["gate_removed_best"] = removed_best
        stats["candidates"] = ncand
        stats["rewalks_over_128"] = rewalks
    return match, nmatches, out4
