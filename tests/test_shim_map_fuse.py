"""shim/LocalMapping.h: FuseMapPoints over the mock map-point and keyframe types of tests/test_shim_map_replace.py (addresses not in
creation order), against the tail of ORBmatcher::Fuse restated in this test's C++ over the reference's own mutators: two identical
worlds, one walked op by op by the plain loop and one by the shim's single call, compared object for object -- mObservations, nObs,
mbBad, mpReplaced, mnFound, mnVisible, mvpMapPoints, the points erased from the map -- and in nFused."""
import os
import re
import subprocess

import pytest

from tests.helpers import ROOT
from tests.test_shim_map_replace import DRIVER as REPLACE_DRIVER

SHIM = os.path.join(ROOT, "weiner_slamit_v2_amd", "shim")
MOCKS = REPLACE_DRIVER[:REPLACE_DRIVER.index("typedef ORB_SLAM2::LocalMapping::ReplaceOp")]                              # MP, KF, MapT with the reference's mutators
STATE = REPLACE_DRIVER[REPLACE_DRIVER.index("// everything the mutators may touch, by id"):REPLACE_DRIVER.index("struct Seen")]

DRIVER = MOCKS + r"""
typedef ORB_SLAM2::LocalMapping::FuseOp<MP, KF> Op;

struct World { std::vector<KF> kfPool; std::vector<MP> mpPool; std::vector<KF*> kf; std::vector<MP*> mp; MapT map; std::vector<Op> ops; };
static unsigned rnd(unsigned& s) { s = s * 1664525u + 1013904223u; return s >> 8; }
static void build(World& W, unsigned seed, int K, int P, int perPoint, int nOps) {
    unsigned s = seed;
    W.kfPool.resize(K); W.mpPool.resize(P); W.kf.resize(K); W.mp.resize(P);
    std::vector<int> ko(K), po(P);
    for (int i = 0; i < K; ++i) ko[i] = i;
    for (int i = 0; i < P; ++i) po[i] = i;
    for (int i = K - 1; i > 0; --i) std::swap(ko[i], ko[rnd(s) % (i + 1)]);
    for (int i = P - 1; i > 0; --i) std::swap(po[i], po[rnd(s) % (i + 1)]);
    const int N = 2 * P * perPoint / K + 8;                                   // keypoints per keyframe: about half of them taken
    for (int i = 0; i < K; ++i) {
        KF* k = W.kf[i] = &W.kfPool[ko[i]];
        k->id = i; k->mvpMapPoints.assign(N, (MP*)NULL); k->mvuRight.resize(N); k->mvKeysUn.resize(N);
        for (int j = 0; j < N; ++j) { k->mvuRight[j] = rnd(s) % 3 == 0 ? 10.f : -1.f; k->mvKeysUn[j] = cv::KeyPoint(0, 0, 1, -1, 0, (int)(rnd(s) % 8)); }
    }
    for (int p = 0; p < P; ++p) {
        MP* m = W.mp[p] = &W.mpPool[po[p]];
        m->id = p; m->mbBad = false; m->nObs = 0; m->mpReplaced = NULL; m->mpMap = &W.map;
        m->mnFound = (int)(rnd(s) % 40); m->mnVisible = 40 + (int)(rnd(s) % 40);
        const int n = p % 11 == 0 ? 0 : 1 + (int)(rnd(s) % (2 * perPoint));
        for (int e = 0; e < n; ++e) {
            KF* k = W.kf[rnd(s) % K];
            const size_t idx = rnd(s) % N;
            if (m->mObservations.count(k) || k->mvpMapPoints[idx]) continue;
            m->AddObservation(k, idx); k->AddMapPoint(m, idx);
        }
        if (p % 13 == 0) m->mbBad = true;                                      // a bad point that still stands in its keyframes
        else W.map.points.insert(p);
    }
    for (int e = 0; e < nOps; ++e) {
        Op op;
        op.pMP = e % 17 == 0 ? (MP*)NULL : W.mp[rnd(s) % (e % 4 == 0 ? std::min(P, 16) : P)];   // a few points many times
        op.pKF = W.kf[rnd(s) % K];
        op.bestIdx = rnd(s) % 100 < 25 ? -1 : (int)(rnd(s) % N);
        W.ops.push_back(op);
    }
}
static bool shuffled(const World& W) {
    bool k = false, p = false;
    for (size_t i = 1; i < W.kf.size(); ++i) k = k || W.kf[i] < W.kf[i - 1];
    for (size_t i = 1; i < W.mp.size(); ++i) p = p || W.mp[i] < W.mp[i - 1];
    return k && p;
}
""" + STATE + r"""
struct Seen { int fused, added, p_rep, q_rep, occ_bad, skipped; };
// the loop body of ORBmatcher::Fuse around its search (ORBmatcher.cc:848-854, :955-975) over the mocks' mutators
static Seen plain_apply(World& W) {
    Seen z = {0, 0, 0, 0, 0, 0};
    for (size_t i = 0; i < W.ops.size(); ++i) {
        MP* pMP = W.ops[i].pMP; KF* pKF = W.ops[i].pKF; const int bestIdx = W.ops[i].bestIdx;
        if (!pMP) continue;
        if (pMP->mbBad || pMP->IsInKeyFrame(pKF)) { ++z.skipped; continue; }
        if (bestIdx < 0) continue;                                             // bestDist > TH_LOW
        MP* pMPinKF = pKF->mvpMapPoints[bestIdx];
        if (pMPinKF) {
            if (!pMPinKF->mbBad) {
                if (pMPinKF->nObs > pMP->nObs) { pMP->Replace(pMPinKF); ++z.p_rep; }
                else { pMPinKF->Replace(pMP); ++z.q_rep; }
            } else ++z.occ_bad;
        } else {
            pMP->AddObservation(pKF, bestIdx);
            pKF->AddMapPoint(pMP, bestIdx);
            ++z.added;
        }
        ++z.fused;
    }
    return z;
}

int main(int argc, char** argv) {
    if (argc != 6) return 2;
    const unsigned seed = (unsigned)atoi(argv[1]);
    const int K = atoi(argv[2]), P = atoi(argv[3]), perPoint = atoi(argv[4]), nOps = atoi(argv[5]);
    World A, B;
    build(A, seed, K, P, perPoint, nOps);
    build(B, seed, K, P, perPoint, nOps);   // the same pools' shuffle: the same relative address order
    const std::vector<long> before = state(A);
    const bool same_start = before == state(B);
    const size_t in_map = A.map.points.size();
    const Seen z = plain_apply(A);
    printf("map_fuse keyframes=%d points=%d ops=%zu addresses_shuffled=%d same_start=%d fused=%d added=%d p_replaced=%d q_replaced=%d occupant_bad=%d skipped=%d erased=%zu changed=%d\n",
           K, P, A.ops.size(), shuffled(A) && shuffled(B) ? 1 : 0, same_start ? 1 : 0, z.fused, z.added, z.p_rep, z.q_rep, z.occ_bad, z.skipped, in_map - A.map.points.size(),
           before != state(A) ? 1 : 0);
#ifdef PLAIN_ONLY   // both worlds through the plain loop: what the worlds hold, without a device
    const int nb = plain_apply(B).fused, st = 0;
#else
    const int nb = ORB_SLAM2::LocalMapping::FuseMapPoints(B.ops, &B.map);
    const int st = ORB_SLAM2::LocalMapping::LastStatus();
    if (st != 0) fprintf(stderr, "fuse_map_points failed: %s\n", slamit_last_error());
#endif
    printf("fuse_map_points: status=%d fused=%d %s\n", st, nb, state(A) == state(B) ? "MATCH" : "DIFFER");
    return 0;
}
"""


def _build(tmp_path, *defines):
    from weiner_slamit_v2_amd import build as hb

    lib = hb.build()
    src, exe = str(tmp_path / "shim_map_fuse.cc"), str(tmp_path / ("shim_map_fuse" + "".join(defines)))
    open(src, "w").write(DRIVER)
    subprocess.check_call(["g++", "-O2"] + list(defines) + ["-std=c++11", "-Wall", "-Wno-unused-function", "-I", SHIM, "-I", os.path.join(ROOT, "include"), src,
                           "-o", exe, lib, "-L/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib", "-lpthread"])
    return exe


def test_the_shim_declares_the_function(tmp_path):
    """No GPU: the function is there, says what it costs, ORBmatcher::Fuse in the shim is not routed through it, and the driver builds."""
    txt = open(os.path.join(SHIM, "LocalMapping.h")).read()
    assert re.search(r"static int FuseMapPoints\(const std::vector<FuseOp<MapPointT, KeyFrameT> >& ops, MapT\* pMap, int device = 0\)", txt)
    assert "NOTHING IS SAVED THROUGH THE SHIM" in txt and "slamit_map_fuse_apply(" in txt
    assert "FuseMapPoints" not in open(os.path.join(SHIM, "ORBmatcher.h")).read()
    assert os.path.exists(_build(tmp_path))


WORLDS = [(3, 10, 60, 3, 120), (2, 25, 400, 5, 700)]


def _check(exe, seed, kfs, points, per_point, ops):
    p = subprocess.run([exe, str(seed), str(kfs), str(points), str(per_point), str(ops)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    out = p.stdout.decode()
    assert p.returncode == 0, (out, p.stderr)
    lines = out.splitlines()
    m = re.match(r"map_fuse keyframes=\d+ points=\d+ ops=\d+ addresses_shuffled=1 same_start=1 fused=(\d+) added=(\d+) p_replaced=(\d+) q_replaced=(\d+) occupant_bad=(\d+) "
                 r"skipped=(\d+) erased=(\d+) changed=1$", lines[0])
    assert m and all(int(m.group(g)) > 0 for g in range(1, 8)), out           # every branch of the tail is walked
    assert re.match(r"fuse_map_points: status=0 fused=%s MATCH$" % m.group(1), lines[1]), (out, p.stderr)


@pytest.mark.parametrize("world", WORLDS)
def test_the_worlds_hold_what_the_comparison_needs(tmp_path, world):
    """No GPU: the driver with the plain loop on both worlds -- every branch of Fuse's tail is taken."""
    _check(_build(tmp_path, "-DPLAIN_ONLY"), *world)


@pytest.mark.gpu
@pytest.mark.parametrize("world", WORLDS)
def test_fuse_map_points_equals_the_reference_loop(tmp_path, world):
    _check(_build(tmp_path), *world)
