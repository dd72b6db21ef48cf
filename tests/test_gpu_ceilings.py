"""GPU: every C-ABI capacity of include/slamit.h run AT its documented ceiling, not one past it ("Limits").

Every comparison is against the CPU oracle, a g++ build of the header the kernel compiles, or a restatement under tests/ -- never
against the library's own output at another size -- and under the bars the suite already applies at working sizes.  The inputs are
tests/ceiling_fixtures.py's; tests/test_ceiling_fixtures.py checks on the CPU what they must contain."""
import numpy as np
import pytest

from oracle import bindings as ob
from tests import ceiling_fixtures as cf
from tests import frustum_ref as fref
from tests import kfdb_ref
from tests import sim3_ransac_ref as rref
from tests.helpers import sim3_close
from tests.test_gpu_frame import CAM_REF
from weiner_slamit_v2_amd import api

pytestmark = pytest.mark.gpu


# ---- 1. frame epilogue: SLAMIT_FRAME_MAX_KP = 30000 -------------------------------------------------------------------------------------
# LDS of frame_finish_kernel: 12,308 B of declared static arrays (12,320 B as built) + 2 B per keypoint slot.
FF_48K = (18416, 18417, 18422, 18423)      # (48 KiB - 12,320) / 2 = 18,416 and (48 KiB - 12,308) / 2 = 18,422: the last size under, the first over
FF_64K = (26608, 26609, 26614, 26615)      # the same around 64 KiB


def _bounds():
    return api.Frame.ComputeImageBounds(CAM_REF, 640, 480)


def _uniform_kps(n, seed):
    """Uniform over the image plus a 40-pixel margin: some keypoints fall outside the grid."""
    rs = np.random.RandomState(seed)
    k = np.zeros(n, api.KP_DTYPE)
    k["x"], k["y"] = rs.uniform(-40, 680, n).astype(np.float32), rs.uniform(-40, 520, n).astype(np.float32)
    k["octave"], k["response"], k["class_id"] = rs.randint(0, 8, n), rs.uniform(7, 200, n).astype(np.float32), -1
    return k


def _one_cell_kps(n):
    """Every in-grid keypoint in ONE cell (the serial placement's worst case), every 50th outside the grid."""
    k = np.zeros(n, api.KP_DTYPE)
    k["x"], k["y"] = 320.25, 240.5
    k["x"][::50], k["y"][::50] = 640, 480
    return k


def _same_finish(kps):
    min_x, _, min_y, _, inv_w, inv_h = _bounds()
    gu, gs, gi = api.Frame.finish(CAM_REF, kps, min_x, min_y, inv_w, inv_h)
    ou, os_, oi = ob.frame_finish(CAM_REF, kps, min_x, min_y, inv_w, inv_h)
    assert np.array_equal(gu.view(np.uint8), ou.view(np.uint8))
    assert np.array_equal(gs, os_) and np.array_equal(gi, oi)
    return gs, gi


def test_frame_finish_at_30000_keypoints_uniform():
    start, items = _same_finish(_uniform_kps(api.FRAME_MAX_KP, 21))
    assert 0.7 * api.FRAME_MAX_KP < start[-1] < api.FRAME_MAX_KP and (np.diff(start) > 0).sum() > 3000     # inside and outside; the grid is full


def test_frame_finish_at_30000_keypoints_in_one_cell():
    start, items = _same_finish(_one_cell_kps(api.FRAME_MAX_KP))
    assert start[-1] == api.FRAME_MAX_KP - 600 and (np.diff(start) > 0).sum() == 1 and (np.diff(items) > 0).all()


@pytest.mark.parametrize("sizes", [FF_48K, FF_64K], ids=["48KiB", "64KiB"])
def test_frame_finish_on_both_sides_of_an_lds_limit(sizes):
    for n in sizes:
        _same_finish(_uniform_kps(n, n))


def test_frame_finish_batch_dev_with_cap_30000():
    import torch

    cap, counts = api.FRAME_MAX_KP, [api.FRAME_MAX_KP, 0, 17]
    kps = np.zeros((3, cap), api.KP_DTYPE)
    kps[0] = _uniform_kps(cap, 22)
    kps[1, :40] = _uniform_kps(40, 23)                            # beyond d_n: not read
    kps[2, :17] = _uniform_kps(17, 24)
    d_kps = torch.from_numpy(kps.view(np.float32).reshape(3, cap, 7)).cuda()
    d_un = torch.full_like(d_kps, -7.0)
    d_n = torch.tensor(counts, dtype=torch.int32, device="cuda")
    d_start = torch.full((3, api.GRID_COLS * api.GRID_ROWS + 1), -7, dtype=torch.int32, device="cuda")
    d_items = torch.full((3, cap), -7, dtype=torch.int32, device="cuda")
    b = _bounds()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    api.Frame.finish_batch_dev(CAM_REF, d_kps, d_n, b[0], b[2], b[4], b[5], d_un, d_start, d_items, stream=s.cuda_stream)
    s.synchronize()
    for f, n in enumerate(counts):
        ou, os_, oi = ob.frame_finish(CAM_REF, kps[f, :n], b[0], b[2], b[4], b[5])
        gu = d_un[f, :n].cpu().numpy().view(np.uint8).reshape(-1, 28)
        assert np.array_equal(gu, ou.view(np.uint8).reshape(-1, 28)), f
        gs = d_start[f].cpu().numpy()
        assert np.array_equal(gs, os_) and np.array_equal(d_items[f, :gs[-1]].cpu().numpy(), oi), f
        assert (d_items[f, gs[-1]:] == -7).all() and (d_un[f, n:] == -7.0).all()                        # nothing written past the counts


# ---- 2. Hamming: SLAMIT_HAMMING_MAX_TRAIN = 65535 train rows (the xor / popcount kernel) ----------------------------------------------
def _flip(row, bits):
    out = row.copy()
    for b in bits:
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def _hamming_sets():
    """70 queries against 65535 random train rows (about 128 bits from everything), with planted rows:
    query 0: best at row 65534 (1 bit), second best row 0 (3 bits);  query 1: best at row 32768, the first index that needs bit 15;
    query 2: rows 0 and 65534 both 1 bit away, the first index wins;  query 3: best at row 20 (1 bit), SECOND best at row 65534 (4 bits)."""
    rs = np.random.RandomState(31)
    nt = api.HAMMING_MAX_TRAIN
    t = rs.randint(0, 256, (nt, 32)).astype(np.uint8)
    q = rs.randint(0, 256, (70, 32)).astype(np.uint8)
    T = t[nt - 1].copy()
    t[0] = _flip(T, (10, 200))
    q[0] = _flip(T, (33,))
    q[1] = _flip(t[32768], (5, 6))
    q[2] = _flip(T, (10,))
    q[3] = _flip(T, (60, 61, 62, 63))
    t[20] = _flip(q[3], (100,))
    return q, t


HAMMING_PLANTED = {0: (65534, 1, 3), 1: (32768, 2, None), 2: (0, 1, 1), 3: (20, 1, 4)}     # query -> (index, best, second)


def _planted(idx, best, second):
    for k, (i, b, s2) in HAMMING_PLANTED.items():
        assert (int(idx[k]), int(best[k])) == (i, b) and (s2 is None or int(second[k]) == s2), k


@pytest.mark.parametrize("nq", [5, 70])
def test_hamming_best2_at_65535_train_rows(nq):
    q, t = _hamming_sets()
    gi, gb, gs = api.ORBmatcher.best2(q[:nq], t)
    oi, obest, osec = ob.best2(q[:nq], t)
    assert np.array_equal(gi, oi) and np.array_equal(gb, obest) and np.array_equal(gs, osec)
    _planted(gi, gb, gs)


def test_hamming_every_distance_256_at_65535_train_rows():
    """A query whose every distance is 256: best = second = 256 as the oracle's, and index 0 -- the library counts a row 256 bits away
    as a row (include/slamit.h), where the reference's loop, which starts from 256 and takes only closer rows, keeps -1."""
    rs = np.random.RandomState(32)
    nt = api.HAMMING_MAX_TRAIN
    q = rs.randint(0, 256, (5, 32)).astype(np.uint8)
    t = np.repeat((255 - q[2])[None], nt, axis=0)
    gi, gb, gs = api.ORBmatcher.best2(q, t)
    oi, obest, osec = ob.best2(q, t)
    assert np.array_equal(gb, obest) and np.array_equal(gs, osec)
    rest = np.arange(5) != 2
    assert np.array_equal(gi[rest], oi[rest]) and (gi[rest] == 0).all() and np.array_equal(gb[rest], gs[rest])   # identical rows: index 0
    assert (gi[2], gb[2], gs[2]) == (0, 256, 256) and (oi[2], obest[2], osec[2]) == (-1, 256, 256)


def test_hamming_best2_batch_dev_with_65535_and_1_train_rows():
    import torch

    q, t = _hamming_sets()
    nt = len(t)
    nq = [70, 33]
    tq = np.zeros((2, 70, 32), np.uint8)
    tq[0], tq[1, :33] = q, q[:33]
    tt = np.zeros((2, nt, 32), np.uint8)
    tt[0], tt[1, 0] = t, t[5]
    d_q, d_t = torch.from_numpy(tq).cuda(), torch.from_numpy(tt).cuda()
    d_nq = torch.tensor(nq, dtype=torch.int32, device="cuda")
    d_nt = torch.tensor([nt, 1], dtype=torch.int32, device="cuda")
    d_idx, d_best, d_second = (torch.full((2, 70), -7, dtype=torch.int32, device="cuda") for _ in range(3))
    api.ORBmatcher.best2_batch_dev(d_q, d_nq, d_t, d_nt, d_idx, d_best, d_second, nt)
    torch.cuda.synchronize()
    for p, (a, b) in enumerate(((q, t), (q[:33], t[5:6]))):
        oi, obest, osec = ob.best2(a, b)
        n = len(a)
        assert np.array_equal(d_idx[p, :n].cpu().numpy(), oi) and np.array_equal(d_best[p, :n].cpu().numpy(), obest), p
        assert np.array_equal(d_second[p, :n].cpu().numpy(), osec), p
        assert (d_idx[p, n:] == -7).all()
    _planted(d_idx[0].cpu().numpy(), d_best[0].cpu().numpy(), d_second[0].cpu().numpy())
    assert (d_idx[1, :33] == 0).all() and (d_second[1, :33] == 256).all()


# ---- 3. BoW search: a group of exactly SLAMIT_BOW_MAX_GROUP = 2048 candidates ---------------------------------------------------------
def _bow_both(s1, s2, g, **kw):
    a = api.ORBmatcher.bow_search(s1, s2, g, **kw)
    o = ob.bow_search(s1, s2, g, **kw)
    assert np.array_equal(a[0], o[0]), "match12 differs at %s" % np.nonzero(a[0] != o[0])[0][:8]
    assert np.array_equal(a[1], o[1]), "dist12 differs at %s" % np.nonzero(a[1] != o[1])[0][:8]
    assert a[2] == o[2] == int((o[0] >= 0).sum())
    return a


@pytest.mark.parametrize("tie", [False, True], ids=["winner_at_2047", "tie_0_and_2047"])
def test_search_by_bow_with_a_group_of_2048(tie):
    s1, s2, g, _, p = cf.bow_full_group(0, tie)
    assert (np.diff(g["c_ptr"]) == [api.BOW_MAX_GROUP, 80]).all()
    for nnratio in (1.5, 0.6):
        m, d, nm = _bow_both(s1, s2, g, mode=0, th=50, th_inclusive=True, nnratio=nnratio)
        if nnratio == 1.5:
            assert m[p["s"]] == (p["first"] if tie else p["last"]) and (m[p["s2"]] == p["last"]) == tie
        assert (m[g["q_idx"][g["q_ptr"][1]:]] >= api.BOW_MAX_GROUP).sum() > 5          # the group after the full one matches in its own range


@pytest.mark.parametrize("tie", [False, True], ids=["winner_at_2047", "tie_0_and_2047"])
def test_search_for_triangulation_with_a_group_of_2048(tie):
    s1, s2, g, epi, p = cf.bow_full_group(1, tie)
    m, d, nm = _bow_both(s1, s2, g, mode=1, th=50, epi=epi)
    assert m[p["s"]] == p["last"] and d[p["s"]] == 2


# ---- 4. keyframe database: query cap 4095 / 4096 (both sides of the 48 KiB branch) and 8191 (SLAMIT_VOC_MAX_FEATURES) ------------------
_KFDB = {}


def _kfdb():
    if "db" not in _KFDB:
        db = api.KeyFrameDatabase(cf.KFDB_SLOTS, cf.KFDB_MAX_WORDS)
        for i, kf in enumerate(k for k in cf.kfdb_keyframes() if k is not None):
            assert db.add(*kf.mBowVec) == i
        _KFDB["db"] = db
    return _KFDB["db"]


def _same_dense(got, want, tag):
    common, first, score = got
    wc, wf, ws = want
    assert np.array_equal(common, wc), "%s common differs at %s" % (tag, np.flatnonzero(common != wc)[:8])
    assert np.array_equal(first, wf), "%s first_word differs at %s" % (tag, np.flatnonzero(first != wf)[:8])
    m = wc >= 1
    assert np.array_equal(score[m].view(np.uint64), ws[m].view(np.uint64)), "%s score bits differ" % tag
    assert (score[~m] == 0.0).all()


@pytest.mark.parametrize("cap", cf.KFDB_CAPS)
def test_kfdb_query_with_a_vector_of_cap_words(cap):
    common, first, seq, score = _kfdb().query(*cf.kfdb_query(cap))
    _same_dense((common, first, score), cf.kfdb_reference(cap), "query %d" % cap)
    live = sum(k is not None for k in cf.kfdb_keyframes())
    assert seq.tolist() == list(range(live)) + [-1] * (cf.KFDB_SLOTS - live)


@pytest.mark.parametrize("cap", cf.KFDB_CAPS)
def test_kfdb_query_batch_dev_with_cap(cap):
    import torch

    short = kfdb_ref.bow(cf.KFDB_POOL, 131, 8)
    queries = [cf.kfdb_query(cap), short, (np.zeros(0, np.int32), np.zeros(0))]
    w, v = np.full((3, cap), -7, np.int32), np.full((3, cap), -7.5)
    for i, (qw, qv) in enumerate(queries):
        w[i, :len(qw)], v[i, :len(qw)] = qw, qv
    t = {"bow_n": torch.tensor([len(q[0]) for q in queries], dtype=torch.int32, device="cuda"), "bow_word": torch.from_numpy(w).cuda(),
         "bow_value": torch.from_numpy(v).cuda(), "common": torch.full((3, cf.KFDB_SLOTS), -777, dtype=torch.int32, device="cuda"),
         "first_word": torch.full((3, cf.KFDB_SLOTS), -777, dtype=torch.int32, device="cuda"),
         "score": torch.full((3, cf.KFDB_SLOTS), -7.5, dtype=torch.float64, device="cuda")}
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    _kfdb().query_batch_dev(t, stream=s.cuda_stream)
    s.synchronize()
    got = [(t["common"][i].cpu().numpy(), t["first_word"][i].cpu().numpy(), t["score"][i].cpu().numpy()) for i in range(3)]
    _same_dense(got[0], cf.kfdb_reference(cap), "batch %d" % cap)
    _same_dense(got[1], kfdb_ref.dense(cf.kfdb_keyframes(), short), "batch %d, short query" % cap)
    _same_dense(got[2], kfdb_ref.dense(cf.kfdb_keyframes(), queries[2]), "batch %d, empty query" % cap)


# ---- 5. pose and Sim3 optimisation: SLAMIT_POSE_MAX_N = SLAMIT_SIM3_MAX_N = 65536 --------------------------------------------------------
def _pose_close(res, ref, tag):
    """tests/test_gpu_pose.py's _close(..., strict=False)."""
    err = np.abs(res["pose"] - ref["pose"]).max() / max(np.abs(ref["pose"]).max(), 1.0)
    assert err <= 1e-5, "%s pose rel err %g" % (tag, err)
    assert np.array_equal(res["outlier"], ref["outlier"]), tag
    assert res["n_inliers"] == ref["n_inliers"], tag
    assert all(abs(a - b) <= 1 for a, b in zip(res["n_its"], ref["n_its"])), tag
    assert np.allclose(res["chi2"], ref["chi2"], rtol=1e-5, atol=1e-9), tag


def test_pose_optimization_at_65536_correspondences():
    got = api.Optimizer.PoseOptimization(cf.pose_ceiling())
    _pose_close(got, cf.pose_oracle("ceiling"), "pose ceiling")


def test_pose_batch_shares_the_ceiling_frames_launch():
    probs = cf.pose_batch()
    outs = api.Optimizer.PoseOptimization(probs)
    for i, (pr, o) in enumerate(zip(probs, outs)):
        one = api.Optimizer.PoseOptimization(pr)
        assert np.array_equal(o["pose"], one["pose"]) and np.array_equal(o["outlier"], one["outlier"]), i
        assert o["n_inliers"] == one["n_inliers"] and o["n_its"] == one["n_its"] and o["chi2"] == one["chi2"], i
    _pose_close(outs[3], ob.pose_solve(probs[3]), "batch[3]")
    assert outs[2]["n_inliers"] == 0 and np.array_equal(outs[2]["pose"], probs[2]["pose"])


def test_pose_above_the_ceiling_is_refused():
    pr = cf.pose_ceiling()
    big = dict(pr, xw=np.concatenate([pr["xw"], pr["xw"][:1]]), uv=np.concatenate([pr["uv"], pr["uv"][:1]]),
               inv_sigma2=np.concatenate([pr["inv_sigma2"], pr["inv_sigma2"][:1]]))
    with pytest.raises(api.SlamitError, match="SLAMIT_POSE_MAX_N") as e:
        api.Optimizer.PoseOptimization(big)
    assert "(-3)" in str(e.value)                                 # SLAMIT_ERR_CAPACITY


def test_sim3_optimization_at_65536_correspondences():
    got = api.Optimizer.OptimizeSim3(cf.sim3_ceiling())
    sim3_close(got, cf.sim3_oracle("ceiling"), tol=1e-5, strict_its=False)


def test_sim3_batch_shares_the_ceiling_problems_launch():
    probs = cf.sim3_batch()
    outs = api.Optimizer.OptimizeSim3(probs)
    for i, (pr, o) in enumerate(zip(probs, outs)):
        one = api.Optimizer.OptimizeSim3(pr)
        assert np.array_equal(o["r12"], one["r12"]) and np.array_equal(o["t12"], one["t12"]) and o["s12"] == one["s12"], i
        assert np.array_equal(o["inlier"], one["inlier"]) and o["n_inliers"] == one["n_inliers"] and o["n_its"] == one["n_its"] and o["chi2"] == one["chi2"], i
    sim3_close(outs[3], ob.sim3_solve(probs[3]), tol=1e-5, strict_its=False)
    assert outs[1]["n_inliers"] == 0 and outs[2]["n_inliers"] == 0    # fewer than 10 pairs: the reference returns 0


def test_sim3_above_the_ceiling_is_refused():
    pr = cf.sim3_ceiling()
    big = dict(pr, n=pr["n"] + 1, **{k: np.concatenate([pr[k], pr[k][:1]]) for k in ("p1", "p2", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2")})
    with pytest.raises(api.SlamitError, match="SLAMIT_SIM3_MAX_N") as e:
        api.Optimizer.OptimizeSim3(big)
    assert "(-3)" in str(e.value)


# ---- 6. Sim3 RANSAC: n = 8192, n = 8152 (n % 64 = 24) and 1024 distinct hypotheses -----------------------------------------------------
@pytest.mark.parametrize("name", sorted(cf.RANSAC))
def test_sim3_ransac_at_its_ceilings(name):
    """tests/test_gpu_sim3_ransac.py::test_flags_and_counts_against_ref32 on the ceiling fixtures."""
    pr, a = cf.ransac(name)
    g = api.Sim3Solver.evaluate(pr)
    n, nh = len(pr["max_err1"]), len(pr["triples"])
    flags = np.unpackbits(g["inlier_bits"].view(np.uint8), axis=1, bitorder="little")
    assert not flags[:, n:].any()                                                # the bits past n of the last word stay clear
    flags = flags[:, :n].astype(bool)
    assert np.array_equal(flags.sum(1), g["n_inliers"])
    d, dec = a["distinct"], a["decided"]
    assert d.all()
    und = (~dec).sum(1)
    wrong = (flags != a["r32"]["flags"]) & dec
    print("%s: n %d hyp %d, flag differences on decided pairs %d, on undecided %d" % (name, n, nh, int(wrong.sum()), int(((flags != a["r32"]["flags"]) & ~dec).sum())))
    assert not wrong.any()
    diff = np.abs(g["n_inliers"] - a["r32"]["counts"])
    assert np.all(diff <= und)
    assert np.array_equal(g["n_inliers"][und == 0], a["r32"]["counts"][und == 0])
    assert rref.admissible(a)


# ---- 7. triangulation at 8192 pairs, frustum at 65536 points ------------------------------------------------------------------------------
def test_triangulate_at_8192_pairs(tmp_path):
    """Both problems in one launch (32 workgroups each) against the g++ build of csrc/triangulate.h, bit for bit."""
    from tests.test_triangulate_ref import host_pairs

    probs = [cf.triangulate_problem(k) for k in range(len(cf.TRIANGULATE))]
    outs = api.triangulate_batch(probs)
    seen = set()
    for k, (pr, out) in enumerate(zip(probs, outs)):
        st, x = host_pairs(tmp_path, pr)
        assert out["status"].shape == (cf.TRIANGULATE_MAX_N,)
        assert np.array_equal(out["status"], st), (k, np.flatnonzero(out["status"] != st)[:8])
        assert np.array_equal(out["x3d"].view(np.uint32), x.view(np.uint32)), k
        assert out["n_accepted"] == int((st == 0).sum())
        one = api.triangulate(pr)
        assert np.array_equal(one["status"], out["status"]) and np.array_equal(one["x3d"].view(np.uint32), out["x3d"].view(np.uint32))
        seen |= set(int(s) for s in out["status"])
    assert seen == {0, 1, 3, 4, 5, 6, 8}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_as_header(out, h, n):
    """tests/test_gpu_frustum.py's same_as_header."""
    assert out["status"].shape == (n,) and out["proj"].shape == (n, 3) and out["uvr"].shape == (n, 3)
    assert np.array_equal(out["status"], h["status"][:n]), np.flatnonzero(out["status"] != h["status"][:n])[:8]
    assert np.array_equal(out["level"], h["level"][:n])
    assert np.array_equal(_bits(out["proj"]), _bits(h["proj"][:n])) and np.array_equal(_bits(out["view_cos"]), _bits(h["viewCos"][:n]))
    assert np.array_equal(_bits(out["uvr"]), _bits(h["uvr"][:n])) and np.array_equal(_bits(out["uvr"][:, 2]), _bits(h["r"][:n]))
    assert np.array_equal(out["level_min"], h["level_min"][:n]) and np.array_equal(out["level_max"], h["level_max"][:n])
    assert np.array_equal(out["valid"], h["valid"][:n])


_FRUSTUM = {}


def _frustum_header():
    if "h" not in _FRUSTUM:
        _FRUSTUM["h"] = fref.host_points(cf.frustum_problem())
    return _FRUSTUM["h"]


def test_frustum_at_65536_points():
    pr, h = cf.frustum_problem(), _frustum_header()
    out = api.frustum(pr)
    _same_as_header(out, h, cf.FRUSTUM_MAX_N)
    assert out["n_in_view"] == int((h["status"] == 0).sum()) and set(int(s) for s in out["status"]) == set(range(8))


def test_frustum_batch_dev_with_q_cap_65536():
    import torch

    pr, h = cf.frustum_problem(), _frustum_header()
    q_cap, m = cf.FRUSTUM_MAX_N, [cf.FRUSTUM_MAX_N, cf.FRUSTUM_SMALL]
    frames = np.zeros(2, api.FRUSTUM_FRAME_DTYPE)
    frames[0] = frames[1] = api.frustum_frame_record(pr)[0]
    t = dict(pos=np.zeros((2, 3, q_cap), np.float32), normal=np.zeros((2, 3, q_cap), np.float32), max_dist=np.zeros((2, q_cap), np.float32),
             min_dist=np.zeros((2, q_cap), np.float32), skip=np.zeros((2, q_cap), np.uint8))
    for f, n in enumerate(m):
        lo = 0 if f == 0 else 100                                               # the second frame: points 100 .. 116 of the same problem
        t["pos"][f, :, :n], t["normal"][f, :, :n] = pr["pos"][lo:lo + n].T, pr["normal"][lo:lo + n].T
        t["max_dist"][f, :n], t["min_dist"][f, :n], t["skip"][f, :n] = pr["max_dist"][lo:lo + n], pr["min_dist"][lo:lo + n], pr["skip"][lo:lo + n]
    d = {k: torch.from_numpy(v).cuda() for k, v in t.items()}
    d["frames"] = torch.from_numpy(frames.view(np.float32).reshape(2, -1)).cuda()
    d["m"] = torch.tensor(m, dtype=torch.int32, device="cuda")
    d.update(uvr=torch.full((2, q_cap, 3), -7.0, device="cuda"), level_min=torch.full((2, q_cap), -7, dtype=torch.int32, device="cuda"),
             level_max=torch.full((2, q_cap), -7, dtype=torch.int32, device="cuda"), valid=torch.full((2, q_cap), 7, dtype=torch.uint8, device="cuda"),
             status=torch.full((2, q_cap), 99, dtype=torch.uint8, device="cuda"), proj=torch.full((2, q_cap, 3), -7.0, device="cuda"),
             view_cos=torch.full((2, q_cap), -7.0, device="cuda"), level=torch.full((2, q_cap), -7, dtype=torch.int32, device="cuda"),
             n_in_view=torch.full((2,), -7, dtype=torch.int32, device="cuda"))
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    api.frustum_batch_dev(d, stream=s.cuda_stream)
    s.synchronize()
    for f, n in enumerate(m):
        lo = 0 if f == 0 else 100
        out = {k: d[k][f, :n].cpu().numpy() for k in ("status", "proj", "view_cos", "level", "uvr", "level_min", "level_max", "valid")}
        hh = {k: v[lo:lo + n] for k, v in h.items()}
        _same_as_header(out, hh, n)
        valid = d["valid"][f, :n].cpu().numpy()
        assert int(d["n_in_view"][f]) == int(valid.sum()) == int((hh["status"] == 0).sum())      # frustum_count_kernel over a full q_cap
        assert (d["status"][f, n:] == 99).all() and (d["valid"][f, n:] == 7).all()
    assert int(d["n_in_view"][0]) > 5000
