"""GPU parity: HIP ORB extractor + Hamming matcher (through the C-ABI) vs the CPU oracle.

Bar: bit-exact keypoints (position, octave, response, angle bits, size), descriptors, pyramid
bytes, FAST candidate lists, match indices/distances.
"""
import numpy as np
import pytest

from oracle import bindings as ob
from weiner_slamit_v2_amd import api, synth

pytestmark = pytest.mark.gpu


def _assert_same(kg, dg, ko, do, tag=""):
    assert len(kg) == len(ko), "%s keypoint count %d vs oracle %d" % (tag, len(kg), len(ko))
    for f in ("octave", "x", "y", "response", "size", "class_id"):
        assert np.array_equal(kg[f], ko[f]), "%s field %s differs" % (tag, f)
    assert np.array_equal(kg["angle"].view(np.uint32), ko["angle"].view(np.uint32)), "%s angle bits differ" % tag
    assert np.array_equal(dg, do), "%s descriptors differ" % tag


def _check_frame(ext, orc, img, tag, stages=True):
    kg, dg = ext(img)
    ko, do = orc.extract(img)
    if stages:
        for l in range(orc.nlevels):
            assert np.array_equal(ext.level(0, l), orc.level(l)), "%s pyramid level %d differs" % (tag, l)
            assert np.array_equal(ext.blurred(0, l), orc.blurred(l)), "%s blurred level %d differs" % (tag, l)
            cg, co = ext.debug_candidates(0, l), orc.candidates(l)
            assert np.array_equal(cg, co), "%s FAST candidates level %d differ (%d vs %d)" % (tag, l, len(cg), len(co))
    _assert_same(kg, dg, ko, do, tag)
    return kg, dg


def test_tables_match_oracle():
    ext = api.ORBextractor(1000, 1.2, 8, 20, 7)
    t = ob.OrbOracle(1000).tables()
    assert np.array_equal(ext.GetScaleFactors(), t["scale"])
    assert np.array_equal(ext.GetInverseScaleFactors(), t["inv_scale"])
    assert np.array_equal(ext.GetScaleSigmaSquares(), t["sigma2"])
    assert np.array_equal(ext.GetInverseScaleSigmaSquares(), t["inv_sigma2"])
    assert np.array_equal(ext.features_per_level(), t["per_level"])
    assert ext.GetLevels() == 8 and abs(ext.GetScaleFactor() - 1.2) < 1e-7


@pytest.mark.parametrize("index", [0, 1, 2])
def test_vga_1000_bit_exact(index):
    """BASELINE config 2 (extract half): 640x480, 1000 features, 8 levels."""
    ext, orc = api.ORBextractor(1000, 1.2, 8, 20, 7), ob.OrbOracle(1000)
    kg, _ = _check_frame(ext, orc, synth.synth_frame(640, 480, index), "vga[%d]" % index)
    assert len(kg) >= 1000


def test_vga_2000_initializer_extractor():
    ext, orc = api.ORBextractor(2000, 1.2, 8, 20, 7), ob.OrbOracle(2000)
    _check_frame(ext, orc, synth.synth_frame(640, 480, 5), "vga2000")


def test_720p_2000():
    """BASELINE config 3 geometry: 1280x720, 2000 features (two octree roots)."""
    ext, orc = api.ORBextractor(2000, 1.2, 8, 20, 7), ob.OrbOracle(2000)
    _check_frame(ext, orc, synth.synth_frame(1280, 720, 7), "720p", stages=True)


def test_dense_candidates_take_the_hbm_key_workspace():
    """More level-0 candidates than the octree's LDS key arrays hold (10240): the kernel's HBM-workspace variant."""
    ext, orc = api.ORBextractor(2000, 1.2, 8, 20, 7), ob.OrbOracle(2000)
    img = synth.noise_frame(1280, 720, 5)
    _check_frame(ext, orc, img, "noise720p", stages=False)
    assert len(ext.debug_candidates(0, 0)) > 10240


def test_edge_images():
    ext, orc = api.ORBextractor(1000, 1.2, 8, 20, 7), ob.OrbOracle(1000)
    # flat: zero keypoints on every level
    k, d = ext(synth.flat_frame(640, 480))
    assert len(k) == 0 and d.shape == (0, 32)
    # pure noise: worst-case candidate count, many equal-score ties
    _check_frame(ext, orc, synth.noise_frame(640, 480, 3), "noise")
    # low contrast: cells that need the minThFAST retry
    low = ((synth.synth_frame(640, 480, 1).astype(np.int32) - 128) // 6 + 128).astype(np.uint8)
    _check_frame(ext, orc, low, "lowcontrast")
    c = ext.debug_candidates(0, 0)
    assert ((c[:, 2] >= 7) & (c[:, 2] < 20)).any()
    # saturated blocks: blur saturation and score ties
    blocks = (np.kron(np.random.RandomState(9).randint(0, 2, (30, 40)), np.ones((16, 16))) * 255).astype(np.uint8)
    _check_frame(ext, orc, blocks, "blocks")
    # sparse: fewer candidates than the quota on the top levels (octree ends early)
    sparse = np.full((480, 640), 100, np.uint8)
    rs = np.random.RandomState(4)
    for _ in range(60):
        x, y = rs.randint(30, 600), rs.randint(30, 440)
        sparse[y:y + 9, x:x + 9] = 220
    _check_frame(ext, orc, sparse, "sparse")
    # empty image (ORBextractor.cc:1068)
    k, d = ext(np.zeros((0, 0), np.uint8))
    assert len(k) == 0


@pytest.mark.parametrize("w,h,nf,nl,sf", [(317, 251, 500, 4, 1.2), (752, 480, 1200, 8, 1.2), (640, 480, 300, 3, 1.5),
                                          (200, 340, 400, 3, 1.3), (534, 402, 600, 8, 1.2), (535, 403, 600, 8, 1.2)])
def test_odd_geometries(w, h, nf, nl, sf):
    ext, orc = api.ORBextractor(nf, sf, nl, 20, 7), ob.OrbOracle(nf, sf, nl, 20, 7)
    _check_frame(ext, orc, synth.synth_frame(w, h, 11), "%dx%d" % (w, h))


def test_pyramid_and_blur_through_their_second_kernels():
    """The pyramid levels come from resize_rows8_kernel (eight dst pixels per lane) wherever a level's taps fit its 16-byte
    windows -- every level at scale factor 1.2 -- and from resize_rows4_kernel otherwise (e.g. scale factor 1.5 above); the
    blurred planes come from blur_stream_kernel (a thread walks a column group down a strip) when the planes are 4-byte
    aligned and from the tile kernel blur_all_kernel otherwise (the unaligned-view test below).  SLAMIT_RESIZE_NO8=1 and
    SLAMIT_BLUR_NO_STREAM=1 (read once, hence the child process) send everything through the four-pixel resize and the
    tile blur: same bytes."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, numpy as np; sys.path.insert(0, %r)\n"
            "from oracle import bindings as ob\n"
            "from weiner_slamit_v2_amd import api, synth\n"
            "for (w, h, nf) in ((640, 480, 1000), (1280, 720, 2000), (317, 251, 500), (533, 401, 600)):\n"
            "    ext, orc = api.ORBextractor(nf, 1.2, 8, 20, 7), ob.OrbOracle(nf)\n"
            "    img = synth.synth_frame(w, h, 3)\n"
            "    kg, dg = ext(img); ko, do = orc.extract(img)\n"
            "    assert all(np.array_equal(ext.level(0, l), orc.level(l)) for l in range(8)), (w, h)\n"
            "    assert all(np.array_equal(ext.blurred(0, l), orc.blurred(l)) for l in range(8)), (w, h)\n"
            "    assert np.array_equal(dg, do) and len(kg) == len(ko)\n"
            "print('same bytes')\n" % root)
    out = subprocess.check_output([sys.executable, "-c", code], env=dict(os.environ, SLAMIT_RESIZE_NO8="1", SLAMIT_BLUR_NO_STREAM="1"), cwd=root, timeout=300)
    assert b"same bytes" in out


def test_thresholds_other_than_default():
    ext, orc = api.ORBextractor(800, 1.2, 6, 35, 12), ob.OrbOracle(800, 1.2, 6, 35, 12)
    _check_frame(ext, orc, synth.synth_frame(640, 480, 13), "th35/12")


def test_batch_equals_single_and_oracle():
    frames = np.stack([synth.synth_frame(640, 480, 20), synth.flat_frame(640, 480), synth.noise_frame(640, 480, 2),
                       synth.synth_frame(640, 480, 21)])
    ext, orc = api.ORBextractor(1000, 1.2, 8, 20, 7, max_batch=4), ob.OrbOracle(1000)
    ks, ds = ext.extract_batch(frames)
    for i in range(len(frames)):
        ko, do = orc.extract(frames[i])
        _assert_same(ks[i], ds[i], ko, do, "batch[%d]" % i)
    # the handle is reusable and deterministic
    ks2, ds2 = ext.extract_batch(frames)
    for i in range(len(frames)):
        assert np.array_equal(ks[i], ks2[i]) and np.array_equal(ds[i], ds2[i])


def test_large_batch_launch_shape_is_bit_exact():
    """From 96 frames per call the octree pass runs 256-thread workgroups with LDS room for 2,048 keys (five per CU), so the long
    lists of the low levels take the HBM key workspace while the short ones stay in LDS: same keypoints as the oracle, whichever
    frame of the batch."""
    kinds = [synth.synth_frame(640, 480, 40), synth.noise_frame(640, 480, 6), synth.synth_frame(640, 480, 41), synth.flat_frame(640, 480)]
    frames = np.stack([kinds[i % 4] for i in range(96)])
    ext, orc = api.ORBextractor(1000, 1.2, 8, 20, 7, max_batch=96), ob.OrbOracle(1000)
    ks, ds = ext.extract_batch(frames)
    want = [orc.extract(f) for f in kinds]
    for i in (0, 1, 2, 3, 49, 94, 95):
        _assert_same(ks[i], ds[i], want[i % 4][0], want[i % 4][1], "batch96[%d]" % i)
    for i in range(4, 96):
        assert np.array_equal(ks[i], ks[i % 4]) and np.array_equal(ds[i], ds[i % 4]), i
    assert len(ext.debug_candidates(0, 0)) > 2048


def test_batch_sizes_around_the_xcd_grids():
    """From 16 frames per call the FAST, orientation and descriptor launches are 1-D grids that deal whole frames to the eight XCDs
    (frame = 8 (k / P) + ((w + k / P) mod 8)); frame counts that are no multiple of eight leave padding workgroups that must do nothing, and
    smaller calls keep the (work, frames) grids: every slot of 15, 16, 20 and 27 frames equals the same frame extracted alone."""
    kinds = [synth.synth_frame(640, 480, 44 + i) for i in range(3)]
    one = api.ORBextractor(1000, 1.2, 8, 20, 7)
    want = [one(f) for f in kinds]
    for n in (15, 16, 20, 27):
        frames = np.stack([kinds[i % 3] for i in range(n)])
        ext = api.ORBextractor(1000, 1.2, 8, 20, 7, max_batch=n)
        ks, ds = ext.extract_batch(frames)
        for i in range(n):
            assert np.array_equal(ks[i], want[i % 3][0]) and np.array_equal(ds[i], want[i % 3][1]), (n, i)


def test_device_buffer_entry_point():
    import torch

    frames = np.stack([synth.synth_frame(640, 480, 30 + i) for i in range(3)])
    ext, orc = api.ORBextractor(1000, 1.2, 8, 20, 7, max_batch=3), ob.OrbOracle(1000)
    ext._bind(640, 480, 3)
    cap = ext.max_keypoints
    d_frames = torch.from_numpy(frames).cuda()
    d_kps = torch.zeros((3, cap, 7), dtype=torch.float32, device="cuda")
    d_desc = torch.zeros((3, cap, 32), dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(3, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    # a caller-owned, non-default stream: extract and the all-pairs match of frames (0,1), (1,2) are enqueued back
    # to back with no host synchronisation in between (the bench's pattern); only the stream orders them
    s = torch.cuda.Stream()
    d_idx = torch.zeros((2, cap), dtype=torch.int32, device="cuda")
    d_best = torch.zeros((2, cap), dtype=torch.int32, device="cuda")
    d_second = torch.zeros((2, cap), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert s.cuda_stream != 0
    ext.extract_batch_dev(d_frames, d_kps, d_desc, d_n, stream=s.cuda_stream)
    api.ORBmatcher.best2_batch_dev(d_desc[0:2], d_n[0:2], d_desc[1:3], d_n[1:3], d_idx, d_best, d_second, cap,
                                   device=0, stream=s.cuda_stream)
    s.synchronize()
    n = d_n.cpu().numpy()
    kps = d_kps.cpu().numpy().view(np.uint8).reshape(3, cap, 28)
    descs = []
    for i in range(3):
        ko, do = orc.extract(frames[i])
        kg = kps[i, :n[i]].copy().view(api.KP_DTYPE).reshape(-1)
        _assert_same(kg, d_desc[i, :n[i]].cpu().numpy(), ko, do, "dev[%d]" % i)
        descs.append(do)
    for p in range(2):
        oi, obest, osec = ob.best2(descs[p], descs[p + 1])
        assert np.array_equal(d_idx[p, :n[p]].cpu().numpy(), oi) and np.array_equal(d_best[p, :n[p]].cpu().numpy(), obest)
        assert np.array_equal(d_second[p, :n[p]].cpu().numpy(), osec)


def test_device_buffer_unaligned_views():
    """Caller-owned device images that are NOT 4-byte aligned (odd row pitch, odd base address): the extractor
    takes its byte-wise staging paths and the fused-pyramid fallback; results stay bit-exact."""
    import torch

    frames = np.stack([synth.synth_frame(640, 480, 60 + i) for i in range(2)])
    ext, orc = api.ORBextractor(1000, 1.2, 8, 20, 7, max_batch=2), ob.OrbOracle(1000)
    ext._bind(640, 480, 2)
    cap = ext.max_keypoints
    for pitch, lead in ((643, 1), (641, 0), (644, 2)):
        big = torch.zeros((2, 481, pitch), dtype=torch.uint8, device="cuda")
        flat = big.view(-1)[lead:lead + 2 * 481 * pitch - pitch]
        view = flat.as_strided((2, 480, 640), (481 * pitch, pitch, 1))
        view.copy_(torch.from_numpy(frames).cuda())
        d_kps = torch.zeros((2, cap, 7), dtype=torch.float32, device="cuda")
        d_desc = torch.zeros((2, cap, 32), dtype=torch.uint8, device="cuda")
        d_n = torch.zeros(2, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ext.extract_batch_dev(view, d_kps, d_desc, d_n, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        n = d_n.cpu().numpy()
        kps = d_kps.cpu().numpy().view(np.uint8).reshape(2, cap, 28)
        for i in range(2):
            ko, do = orc.extract(frames[i])
            kg = kps[i, :n[i]].copy().view(api.KP_DTYPE).reshape(-1)
            _assert_same(kg, d_desc[i, :n[i]].cpu().numpy(), ko, do, "pitch%d+%d[%d]" % (pitch, lead, i))


# ---- Hamming ------------------------------------------------------------------------------------

def test_hamming_random_and_ties():
    rs = np.random.RandomState(0)
    q = rs.randint(0, 256, (1003, 32)).astype(np.uint8)
    t = rs.randint(0, 256, (997, 32)).astype(np.uint8)
    t[500] = q[3]
    t[600] = t[100]      # duplicate train rows: the first index must win
    t[601] = t[100]
    q[7] = t[100]
    gi, gb, gs = api.ORBmatcher.best2(q, t)
    oi, obest, osec = ob.best2(q, t)
    assert np.array_equal(gi, oi) and np.array_equal(gb, obest) and np.array_equal(gs, osec)
    assert gb[7] == 0 and gi[7] == 100 and gs[7] == 0
    assert np.array_equal(api.ORBmatcher.distance_matrix(q[:70], t[:130]), ob.matrix(q[:70], t[:130]))
    assert api.ORBmatcher.DescriptorDistance(q[0], t[0]) == ob.distance(q[0], t[0])


@pytest.mark.parametrize("nq,nt", [(1, 1), (5, 0), (64, 3), (65, 257), (2, 1000), (300, 2)])
def test_hamming_ragged(nq, nt):
    rs = np.random.RandomState(nq * 1000 + nt)
    q = rs.randint(0, 4, (nq, 32)).astype(np.uint8)  # few distinct values: lots of equal distances
    t = rs.randint(0, 4, (nt, 32)).astype(np.uint8)
    gi, gb, gs = api.ORBmatcher.best2(q, t)
    oi, obest, osec = ob.best2(q, t)
    assert np.array_equal(gi, oi) and np.array_equal(gb, obest) and np.array_equal(gs, osec)


def test_hamming_every_bit_position_extremes_and_the_large_set_kernel():
    """The matrix-core kernel permutes the 256 bit positions onto its K axis: every position must count exactly once
    (one-hot rows), distances 0 and 256 must survive the key packing, and train sets above its 8192-row limit take
    the xor / popcount kernel with the same answers."""
    onehot = np.zeros((256, 32), np.uint8)
    for b in range(256):
        onehot[b, b >> 3] = 1 << (b & 7)
    q = np.concatenate([np.zeros((1, 32), np.uint8), np.full((1, 32), 255, np.uint8), onehot[::7]])
    t = np.concatenate([onehot, 255 - onehot, np.full((1, 32), 255, np.uint8)])
    gi, gb, gs = api.ORBmatcher.best2(q, t)
    oi, obest, osec = ob.best2(q, t)
    assert np.array_equal(gi, oi) and np.array_equal(gb, obest) and np.array_equal(gs, osec)
    assert gb[0] == 1 and gi[0] == 0 and gs[0] == 1 and gb[1] == 0 and gi[1] == 512
    gi, gb, gs = api.ORBmatcher.best2(np.zeros((3, 32), np.uint8), np.full((40, 32), 255, np.uint8))
    assert (gb == 256).all() and (gs == 256).all() and (gi == 0).all()       # 256 is a real distance here, not "none"
    rs = np.random.RandomState(5)
    q = rs.randint(0, 256, (70, 32)).astype(np.uint8)
    t = rs.randint(0, 256, (8300, 32)).astype(np.uint8)
    t[8250] = q[5]
    for nt in (8192, 8193, 8300):
        gi, gb, gs = api.ORBmatcher.best2(q, t[:nt])
        oi, obest, osec = ob.best2(q, t[:nt])
        assert np.array_equal(gi, oi) and np.array_equal(gb, obest) and np.array_equal(gs, osec), nt
    assert gi[5] == 8250 and gb[5] == 0


def test_extract_then_match_pair():
    """BASELINE config 2 end to end: frame A vs its warped copy B, all-pairs best/second +
    TH_LOW / ratio 0.9 acceptance, indices identical to the oracle's."""
    a = synth.synth_frame(640, 480, 40)
    b = synth.warp_frame(a, 40)
    ext, orc = api.ORBextractor(1000, 1.2, 8, 20, 7), ob.OrbOracle(1000)
    ka, da = ext(a)
    kb, db = ext(b)
    _assert_same(kb, db, *orc.extract(b), "warped")
    m = api.ORBmatcher(0.9, True)
    qi, ti = m.match(da, db)
    oi, obest, osec = ob.best2(da, db)
    ok = (obest <= 50) & (obest.astype(np.float32) < np.float32(0.9) * osec.astype(np.float32))
    assert np.array_equal(qi, np.nonzero(ok)[0]) and np.array_equal(ti, oi[ok])
    assert len(qi) > 100  # the warp is mild: many true matches


def test_distinctive_descriptors_batch():
    rs = np.random.RandomState(21)
    desc, offs = [], [0]
    for p in range(400):
        n = int(rs.choice([0, 1, 2, 3, 5, 9, 17, 33, 64, 65, 100, 128]))
        base = rs.randint(0, 256, (1, 32)).astype(np.uint8)
        d = base ^ (rs.randint(0, 256, (n, 32)) < rs.randint(4, 60)).astype(np.uint8)  # clustered: many equal medians
        desc.append(d)
        offs.append(offs[-1] + n)
    desc = np.concatenate(desc)
    gi, gm = api.ORBmatcher.distinctive(desc, offs)
    oi, om = ob.distinctive(desc, offs)
    assert np.array_equal(gi, oi) and np.array_equal(gm, om)
    with pytest.raises(api.SlamitError):
        api.ORBmatcher.distinctive(rs.randint(0, 256, (129, 32)).astype(np.uint8), [0, 129])


# ---- guided search ------------------------------------------------------------------------------

def _search_same(frame, queries, th, use_ratio, nnratio=0.8):
    gm, gn, g4 = api.ORBmatcher.guided_search(frame, queries, th, use_ratio, nnratio)
    om, on, o4 = ob.guided_search(frame, queries, th, use_ratio, nnratio)
    assert np.array_equal(gm, om) and gn == on
    assert np.array_equal(g4, o4)
    return gm, gn


@pytest.mark.parametrize("seed,n,m,crowd", [(0, 1500, 600, False), (1, 300, 900, True), (2, 0, 10, False), (3, 5, 0, False),
                                             (4, 2500, 400, False), (5, 8191, 3000, False), (6, 1000, 2000, True)])
def test_guided_search_synthetic(seed, n, m, crowd):
    frame, queries = synth.synth_search(n, m, seed, th=6.0 if crowd else 3.0, crowd=crowd)
    for use_ratio, th in ((True, 100), (False, 100), (True, 50)):
        _search_same(frame, queries, th, use_ratio)


def test_guided_search_kat_and_limits():
    xy = np.array([[100, 100], [102, 101], [300, 300], [100.4, 99.6]], np.float32)
    desc = np.zeros((4, 32), np.uint8)
    desc[1, 0], desc[2], desc[3, 1] = 0x0F, 0xFF, 0x01
    frame = dict(kp_xy=xy, kp_octave=np.array([1, 1, 0, 5], np.int32), desc=desc, kp_taken=np.zeros(4, np.uint8),
                 min_x=0.0, min_y=0.0, inv_w=0.1, inv_h=0.1)
    q = dict(uvr=np.array([[101, 100, 5], [101, 100, 5], [101, 100, 5], [300, 300, 0.5]], np.float32),
             level_min=np.zeros(4, np.int32), level_max=np.array([1, 1, 1, -1], np.int32), desc=np.zeros((4, 32), np.uint8))
    gm, gn = _search_same(frame, q, 100, False)
    assert gm.tolist() == [0, 1, -1, -1] and gn == 2
    big = synth.synth_search(8192, 4, 9)
    with pytest.raises(api.SlamitError):
        api.ORBmatcher.guided_search(big[0], big[1])
    # Every keypoint in every window: 1500 candidates, more than the SLAMIT_SEARCH_MAX_CAND (1024) entries a query's stored
    # list holds.  The (best, second) pair is reduced over ALL hits, so the result is exact -- and must equal the oracle,
    # which like the reference has no such limit; when an earlier query of the call took one of the two, the query walks the
    # frame's keypoints again instead of its truncated list: still the oracle's answer.
    f, qq = synth.synth_search(1500, 4, 10, crowd=True)
    qq["uvr"][:, 2] = 500.0
    qq["level_min"][:] = 0
    qq["level_max"][:] = -1
    qq["valid"][:] = 1
    qq["takes"][:] = 1
    free = np.flatnonzero(f["kp_taken"] == 0)[:4]
    qq["desc"][:] = f["desc"][free]                       # four different keypoints, each query an exact copy of "its" one
    gm, gn = _search_same(f, qq, 100, False)
    assert gm.tolist()[1:] == free.tolist()[1:] and gn >= 3   # (query 0's window lies outside the grid by construction)
    qq["desc"][2] = qq["desc"][1]                         # the third query now wants the keypoint the second one just took
    gm2, gn2 = _search_same(f, qq, 100, False)            # (_search_same asserts equality with the oracle)
    assert gm2[2] != gm2[1] and gm2[1] == free[1]


def test_guided_search_on_extracted_frames():
    """Tracking-shaped use: keypoints of frame B searched with frame A's keypoints as 'map points'
    projected through the known warp (here: identity + jitter), windows from the keypoint's octave."""
    a = synth.synth_frame(640, 480, 50)
    ext = api.ORBextractor(1000, 1.2, 8, 20, 7)
    ka, da = ext(a)
    kb, db = ext(synth.warp_frame(a, 50))
    scale = ext.GetScaleFactors()
    frame = dict(kp_xy=np.stack([kb["x"], kb["y"]], 1), kp_octave=kb["octave"], desc=db, kp_taken=np.zeros(len(kb), np.uint8),
                 min_x=0.0, min_y=0.0, inv_w=float(np.float32(64) / np.float32(640)), inv_h=float(np.float32(48) / np.float32(480)))
    r = (np.float32(15.0) * scale[ka["octave"]]).astype(np.float32)
    q = dict(uvr=np.stack([ka["x"], ka["y"], r], 1), level_min=ka["octave"] - 1, level_max=ka["octave"] + 1, desc=da)
    gm, gn = _search_same(frame, q, 100, False)
    assert gn > 50
    won = gm[gm >= 0]
    assert len(np.unique(won)) == len(won)        # a keypoint is handed out once


def _search_batch_tensors(problems, kp_cap, q_cap):
    import torch

    B = len(problems)
    kps = np.zeros((B, kp_cap), api.KP_DTYPE)
    t = dict(n=np.zeros(B, np.int32), desc=np.zeros((B, kp_cap, 32), np.uint8), kp_taken=np.zeros((B, kp_cap), np.uint8),
             m=np.zeros(B, np.int32), uvr=np.zeros((B, q_cap, 3), np.float32), level_min=np.zeros((B, q_cap), np.int32),
             level_max=np.zeros((B, q_cap), np.int32), qdesc=np.zeros((B, q_cap, 32), np.uint8), valid=np.zeros((B, q_cap), np.uint8),
             takes=np.ones((B, q_cap), np.uint8))
    for i, (f, q) in enumerate(problems):
        n, m = len(f["kp_xy"]), len(q["uvr"])
        t["n"][i], t["m"][i] = n, m
        kps["x"][i, :n], kps["y"][i, :n], kps["octave"][i, :n] = f["kp_xy"][:, 0], f["kp_xy"][:, 1], f["kp_octave"]
        t["desc"][i, :n], t["kp_taken"][i, :n] = f["desc"], f["kp_taken"]
        t["uvr"][i, :m], t["level_min"][i, :m], t["level_max"][i, :m] = q["uvr"], q["level_min"], q["level_max"]
        t["qdesc"][i, :m], t["valid"][i, :m], t["takes"][i, :m] = q["desc"], q["valid"], q["takes"]
    d = {k: torch.from_numpy(v).cuda() for k, v in t.items()}
    d["kps_un"] = torch.from_numpy(kps.view(np.float32).reshape(B, kp_cap, 7)).cuda()
    d["match_kp"] = torch.full((B, q_cap), -7, dtype=torch.int32, device="cuda")
    d["nmatches"] = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    d["out4"] = torch.zeros((B, q_cap, 4), dtype=torch.int32, device="cuda")
    d["workspace"] = torch.zeros(api.ORBmatcher.guided_search_workspace(B, q_cap), dtype=torch.uint8, device="cuda")
    return d


def test_guided_search_batch_dev():
    """Frames of different sizes in one launch (one wavefront resolves each frame), data resident on the device."""
    import torch

    shapes = [(1500, 600, False), (300, 900, True), (0, 10, False), (5, 0, False), (2500, 400, False), (1000, 1000, False)]
    problems = [synth.synth_search(n, m, 40 + i, th=6.0 if crowd else 3.0, crowd=crowd) for i, (n, m, crowd) in enumerate(shapes)]
    bounds = tuple(problems[0][0][k] for k in ("min_x", "min_y", "inv_w", "inv_h"))
    d = _search_batch_tensors(problems, 2560, 1024)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    for use_ratio, th in ((True, 100), (False, 100)):
        api.ORBmatcher.guided_search_batch_dev(d, bounds, th, use_ratio, 0.8, stream=s.cuda_stream)
        s.synchronize()
        nm = d["nmatches"].cpu().numpy()
        for i, (f, q) in enumerate(problems):
            om, on, o4 = ob.guided_search(f, q, th, use_ratio, 0.8)
            m = len(q["uvr"])
            # (frame 1: crowded windows with more than SLAMIT_SEARCH_BATCH_CAND candidates -- queries whose tentative pair was taken
            #  walk the frame's keypoints again; same result as the reference's unlimited lists)
            assert nm[i] == on
            assert np.array_equal(d["match_kp"][i, :m].cpu().numpy(), om) and np.array_equal(d["out4"][i, :m].cpu().numpy(), o4)
    with pytest.raises(api.SlamitError):   # workspace too small
        d2 = dict(d, workspace=d["workspace"][:1024])
        api.ORBmatcher.guided_search_batch_dev(d2, bounds)


def test_guided_search_fuse_gate():
    frame, queries = synth.synth_search(1500, 800, 9, th=3.0)
    frame = dict(frame, kp_taken=np.zeros(1500, np.uint8))
    queries = dict(queries, takes=np.zeros(800, np.uint8))
    sig = (1.0 / (np.float32(1.2) ** np.arange(16, dtype=np.float32)) ** 2).astype(np.float32)
    gm, gn, g4 = api.ORBmatcher.guided_search(frame, queries, 50, False, 0.6, chi2_gate=5.99, inv_level_sigma2=sig)
    om, on, o4 = ob.guided_search(frame, queries, 50, False, 0.6, 5.99, sig)
    assert np.array_equal(gm, om) and gn == on and np.array_equal(g4, o4) and gn > 0


def _assert_init_case_walks_the_frame(f1, prev, f2, window, om, oacc):
    """The fixture really reaches mode 1's re-scan of a TRUNCATED candidate list: more level-0 keypoints in every window than
    SLAMIT_SEARCH_MAX_CAND (1024), a take-over, and a query whose tentative best is excluded at its turn.  From the inputs and the
    oracle's result alone."""
    x2, o2 = np.asarray(f2["kp_xy"], np.float32), np.asarray(f2["kp_octave"])
    cell = [np.floor(((x2[:, a] - np.float32(f2[lo])) * np.float32(f2[inv])).astype(np.float64) + 0.5) for a, lo, inv in ((0, "min_x", "inv_w"), (1, "min_y", "inv_h"))]
    cand = np.nonzero((o2 == 0) & (cell[0] >= 0) & (cell[0] < 64) & (cell[1] >= 0) & (cell[1] < 48))[0]   # Frame::PosInGrid, level [0, 0]
    assert len(cand) > 1024, "fixture: a window must hold more than SLAMIT_SEARCH_MAX_CAND candidates"
    queries = np.nonzero(np.asarray(f1["kp_octave"]) <= 0)[0]
    assert (np.abs(x2[cand][None] - np.asarray(prev, np.float32)[queries][:, None]) < np.float32(window)).all(), "fixture: the window must cover the frame"
    assert ((oacc >= 0) & (om < 0)).any(), "fixture: no take-over"
    cand = cand[np.lexsort((cand, cell[1][cand], cell[0][cand]))]                 # GetFeaturesInArea's scan order: first minimum wins
    bits = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(1)
    d1, d2 = np.asarray(f1["desc"], np.uint8), np.asarray(f2["desc"], np.uint8)
    dist = bits[d1[queries][:, None, :] ^ d2[cand][None, :, :]].sum(2)
    nearest, dmin = cand[dist.argmin(1)], dist.min(1)
    held = np.full(len(o2), np.iinfo(np.int32).max)                              # distance of each keypoint's current match
    stale = 0
    for q, kp, d in zip(queries, nearest, dmin):
        stale += held[kp] <= d
        if oacc[q] >= 0:
            held[oacc[q]] = bits[d1[q] ^ d2[oacc[q]]].sum()
    assert stale >= 1, "fixture: no query finds its tentative best excluded"


@pytest.mark.parametrize("n,seed,window", [(900, 1, 40), (2000, 2, 100), (300, 3, 10), (64, 4, 1000), (1600, 5, 2000)])
def test_search_for_initialization_mode(n, seed, window):
    """Guided-search mode 1 == ORBmatcher::SearchForInitialization's loop (matched-distance gate, take-over).  The last case puts
    more keypoints into every window than a stored candidate list holds, so stale queries walk the frame again."""
    f1, prev, f2 = synth.synth_init_pair(n, seed)
    om, on, oacc = ob.search_for_initialization(f1, prev, f2, window, 0.9, 50)
    if window == 2000:
        _assert_init_case_walks_the_frame(f1, prev, f2, window, om, oacc)
    gm, gn, gacc = api.ORBmatcher.search_for_initialization(f1, prev, f2, window, 0.9, 50)
    assert np.array_equal(gm, om) and gn == on and np.array_equal(gacc, oacc)


@pytest.mark.parametrize("name", ["vga", "vga2000", "720p"])
def test_hip_reproduces_orb_golden(name):
    """The HIP path against the committed vectors of tests/golden/orb_*.npz (the restatement's outputs, frozen;
    non-authoritative regression guards)."""
    from tests.helpers import assert_matches_orb_golden, crc32, load_orb_golden
    z, img = load_orb_golden(name)
    ext = api.ORBextractor(int(z["params"][2]), 1.2, 8, 20, 7)
    kps, desc = ext(img)
    assert_matches_orb_golden(z, kps, desc, name)
    for l in range(8):
        c = ext.debug_candidates(0, l)
        assert len(c) == int(z["cand_n"][l]) and crc32(c) == int(z["cand_crc"][l]), "level %d candidates" % l
        assert crc32(ext.level(0, l)) == int(z["level_crc"][l]), "level %d pyramid plane" % l
        assert crc32(ext.blurred(0, l)) == int(z["blur_crc"][l]), "level %d blurred plane" % l


def test_720p_batch64_and_2000x2000_match():
    """BASELINE config 3 at its full shape: 64 frames of 1280x720 with the 2000-feature extractor in ONE batch call
    (Tracking.cc:162 really runs 2000 features), then every frame matched against its predecessor (2000 x 2000
    best / second).  Every frame of the batch must equal the same frame extracted alone; three distinct frames (first,
    middle, last slot) and the matches of two pairs must equal the oracle."""
    B = 64
    uniq = [synth.synth_frame(1280, 720, 40 + i) for i in range(6)] + [synth.warp_frame(synth.synth_frame(1280, 720, 40), 0)]
    order = [(i * 5 + 3) % len(uniq) for i in range(B)]
    order[0], order[1], order[31], order[63] = 0, 6, 3, 5   # (0, 6) is a real frame pair: B = warp(A)
    frames = np.stack([uniq[k] for k in order])
    ext = api.ORBextractor(2000, 1.2, 8, 20, 7, max_batch=B)
    ks, ds = ext.extract_batch(frames)
    single = api.ORBextractor(2000, 1.2, 8, 20, 7)
    alone = {}
    for k in sorted(set(order)):
        alone[k] = single(uniq[k])
    for i, k in enumerate(order):
        _assert_same(ks[i], ds[i], alone[k][0], alone[k][1], "batch slot %d (frame %d)" % (i, k))
        assert len(ks[i]) >= 2000
    orc = ob.OrbOracle(2000)
    oracle_out = {}
    for slot in (0, 1, 31, 63):
        ko, do = orc.extract(frames[slot])
        oracle_out[slot] = do
        _assert_same(ks[slot], ds[slot], ko, do, "batch slot %d vs oracle" % slot)
    for q, t in ((1, 0), (63, 31)):   # a warped pair (many accepted matches) and an unrelated pair
        gi, gb, gs = api.ORBmatcher.best2(ds[q], ds[t])
        oi, obest, osec = ob.best2(oracle_out[q], oracle_out[t])
        assert len(gi) >= 2000 and len(ds[t]) >= 2000
        assert np.array_equal(gi, oi) and np.array_equal(gb, obest) and np.array_equal(gs, osec), "2000x2000 best2 pair (%d, %d)" % (q, t)
    acc = (gb <= 50) & (gb < 0.9 * gs)
    gi, gb, gs = api.ORBmatcher.best2(ds[1], ds[0])
    assert int(((gb <= 50) & (gb < 0.9 * gs)).sum()) > 200, "the warped pair must produce accepted matches"
