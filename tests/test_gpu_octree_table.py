"""octree_kernel's two ways through a (frame, level): from the path table (csrc/octree_table.h: one sweep over the keys, the node passes
on wavefront 0, the picks from the per-bin best keys) and, when a pass needs a depth the table does not hold, the walk over the keys
from the start.  Every case is compared with the oracle level by level and as a whole extract, and ORBextractor.debug_octree_path
says which way each level went, so that the inputs are known to take the path they are named for."""
import numpy as np
import pytest

from oracle import bindings as ob
from weiner_slamit_v2_amd import api, synth

pytestmark = pytest.mark.gpu


def _squares60():
    """tests/test_gpu_orb.py::test_edge_images' sparse image: 60 bright 9 x 9 squares, fewer corners than the quota on the top levels."""
    img = np.full((480, 640), 100, np.uint8)
    rs = np.random.RandomState(4)
    for _ in range(60):
        x, y = rs.randint(30, 600), rs.randint(30, 440)
        img[y:y + 9, x:x + 9] = 220
    return img


def _paths(ext, frame, nlevels):
    return [ext.debug_octree_path(frame, l) for l in range(nlevels)]


def _check(ext, orc, img, tag):
    """The extract of `img` against the oracle: every level's list (count, level coordinates, response, in list order), then all
    fields and descriptors.  -> (keypoints, descriptors, path per level)"""
    kg, dg = ext(img)
    ko, do = orc.extract(img)
    scale = ext.GetScaleFactors()
    for l in range(orc.nlevels):
        g, lk = kg[kg["octave"] == l], orc.level_kps(l)
        assert len(g) == len(lk), "%s level %d: %d keypoints, the oracle keeps %d" % (tag, l, len(g), len(lk))
        assert np.array_equal(g["response"], lk["response"]), "%s level %d: responses or their order differ" % (tag, l)
        for f in ("x", "y"):
            assert np.array_equal(g[f], (lk[f] * np.float32(scale[l])).astype(np.float32)), "%s level %d: %s differs" % (tag, l, f)
    assert len(kg) == len(ko), tag
    for f in ("octave", "x", "y", "response", "size", "class_id"):
        assert np.array_equal(kg[f], ko[f]), "%s field %s differs" % (tag, f)
    assert np.array_equal(kg["angle"].view(np.uint32), ko["angle"].view(np.uint32)), "%s angle bits differ" % tag
    assert np.array_equal(dg, do), "%s descriptors differ" % tag
    return kg, dg, _paths(ext, 0, orc.nlevels)


@pytest.fixture(scope="module")
def vga1000():
    return api.ORBextractor(1000, 1.2, 8, 20, 7), ob.OrbOracle(1000)


@pytest.fixture(scope="module")
def vga_kinds():
    """The four VGA frames of the batch cases, each extracted alone once: (image, keypoints, descriptors, paths)."""
    one = api.ORBextractor(1000, 1.2, 8, 20, 7)
    out = []
    for img in (synth.synth_frame(640, 480, 0), _squares60(), synth.noise_frame(640, 480, 3), synth.synth_frame(640, 480, 5)):
        k, d = one(img)
        out.append((img, k, d, _paths(one, 0, 8)))
    return out


def test_vga_frame_stays_in_the_table(vga1000):
    _, _, paths = _check(*vga1000, synth.synth_frame(640, 480, 0), "vga")
    assert paths == [(4, False)] * 7 + [(3, False)], paths   # three full passes and one "largest first" pass; level 7 ends a pass sooner


def test_squares_leave_the_table_above_level_0(vga1000):
    _, _, paths = _check(*vga1000, _squares60(), "squares60")
    assert not paths[0][1] and paths[0][0] >= 1, paths
    assert all(left for _, left in paths[1:]), paths   # few corners in small clusters: the walk goes below depth 4
    assert all(p >= 4 for p, _ in paths[1:]), paths    # ... and no pass before the fifth can meet a node of depth 4


def test_vga_2000_leaves_at_the_careful_pass():
    ext, orc = api.ORBextractor(2000, 1.2, 8, 20, 7), ob.OrbOracle(2000)
    _, _, paths = _check(ext, orc, synth.synth_frame(640, 480, 5), "vga2000")
    assert paths[:3] == [(4, True)] * 3, paths   # four full passes from the table; the "largest first" pass needs depth 5
    assert orc.octree_exits()[:3] == ["sorted_stage"] * 3
    assert all(not left for _, left in paths[3:]), paths


def test_small_lists():
    ext, orc = api.ORBextractor(500, 1.2, 4, 20, 7), ob.OrbOracle(500, 1.2, 4, 20, 7)
    _, _, paths = _check(ext, orc, synth.synth_frame(317, 251, 11), "317x251")
    assert all(1 <= p <= 4 for p, _ in paths), paths


def test_720p_two_roots():
    ext, orc = api.ORBextractor(2000, 1.2, 8, 20, 7), ob.OrbOracle(2000)
    _, _, paths = _check(ext, orc, synth.synth_frame(1280, 720, 7), "720p")
    assert all(not left and p >= 3 for p, left in paths), paths   # both roots' tables fit, and the frame stays inside them


def test_noise_ties_and_a_list_beyond_the_lds_key_room(vga1000):
    ext, orc = vga1000
    _, _, paths = _check(ext, orc, synth.noise_frame(640, 480, 3), "noise")
    assert len(ext.debug_candidates(0, 0)) > 10240   # more than any LDS key array holds
    c = orc.candidates(0)[:, 2]
    assert len(c) - len(np.unique(c)) > len(c) // 2   # most responses repeat: the first maximum in list order decides
    assert all(not left for _, left in paths), paths


def test_96_frames_take_the_256_thread_shape(vga_kinds):
    frames = np.stack([vga_kinds[i % 4][0] for i in range(96)])
    ext = api.ORBextractor(1000, 1.2, 8, 20, 7, max_batch=96)
    ks, ds = ext.extract_batch(frames)
    for i in range(96):
        _, k, d, paths = vga_kinds[i % 4]
        assert np.array_equal(ks[i], k) and np.array_equal(ds[i], d), i
        assert _paths(ext, i, 8) == paths, i
    assert any(left for _, left in vga_kinds[1][3]) and not any(left for _, left in vga_kinds[0][3])


def test_3_frames_take_the_1024_thread_shape(vga_kinds):
    frames = np.stack([vga_kinds[i][0] for i in (1, 0, 2)])
    ext = api.ORBextractor(1000, 1.2, 8, 20, 7, max_batch=3)
    ks, ds = ext.extract_batch(frames)
    for slot, i in enumerate((1, 0, 2)):
        _, k, d, paths = vga_kinds[i]
        assert np.array_equal(ks[slot], k) and np.array_equal(ds[slot], d), slot
        assert _paths(ext, slot, 8) == paths, slot
