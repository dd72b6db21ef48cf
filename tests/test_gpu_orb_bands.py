"""GPU parity of the banded pyramid (pyramid_bands_kernel: levels 1 .. 7 in one launch per segment, a workgroup per (frame, band of
rows), levels >= a segment's second out of LDS) against the oracle's pyramid, byte for byte on every level, through the getter
test_gpu_orb.py's _check_frame uses (slamit_orb_level); and of the paths that stay beside it (a level-0 view that is not 4-byte
aligned)."""
import numpy as np
import pytest

from oracle import bindings as ob
from weiner_slamit_v2_amd import api, synth

pytestmark = pytest.mark.gpu

NL = 8


def _columns(w, h):
    img = np.zeros((h, w), np.uint8)
    img[:, 1::2] = 255
    return img


def _images(w, h):
    """name -> frame: three textured frames, constant 255 and alternating 0 / 255 columns (the rounding at both extremes)"""
    d = {"s%d" % i: synth.synth_frame(w, h, 70 + i) for i in range(3)}
    d["white"] = np.full((h, w), 255, np.uint8)
    d["columns"] = _columns(w, h)
    return d


@pytest.fixture(scope="module")
def ref():
    """{(w, h): {name: (frame, [oracle level 0 .. 7, padded planes])}}, computed once"""
    out = {}
    orc = ob.OrbOracle(1000)
    for w, h in ((640, 480), (1241, 376)):   # 1241: odd width, the last column group of most levels is partial; 376 rows: 5 .. 47 per band
        out[(w, h)] = {}
        for name, img in _images(w, h).items():
            orc.extract(img)
            out[(w, h)][name] = (img, [orc.level(l).copy() for l in range(NL)])
    return out


@pytest.fixture(scope="module")
def alone(ref):
    """{(w, h): {name: (keypoints, descriptors)}} of every frame extracted alone (one frame per call)"""
    out = {}
    for geo, frames in ref.items():
        ext = api.ORBextractor(1000, 1.2, NL, 20, 7)
        out[geo] = {name: ext(img) for name, (img, _) in frames.items()}
    return out


def _check_levels(ext, slot, want, tag):
    for l in range(NL):
        got = ext.level(slot, l)
        assert got.shape == want[l].shape and np.array_equal(got, want[l]), "%s: pyramid level %d differs" % (tag, l)


@pytest.mark.parametrize("geo", [(640, 480), (1241, 376)], ids=lambda g: "%dx%d" % g)
@pytest.mark.parametrize("n", [1, 3, 17])   # 17: the grid that deals whole frames to the XCDs (from 16), one frame into the third group of eight
def test_every_level_of_every_slot_equals_the_oracle(ref, alone, geo, n):
    names = ["s0", "white", "columns", "s1", "s2"]
    order = [names[i % len(names)] for i in range(n)]
    frames = np.stack([ref[geo][k][0] for k in order])
    ext = api.ORBextractor(1000, 1.2, NL, 20, 7, max_batch=n)
    ks, ds = ext.extract_batch(frames)
    for i, k in enumerate(order):
        _check_levels(ext, i, ref[geo][k][1], "%dx%d batch %d slot %d (%s)" % (geo + (n, i, k)))
        assert np.array_equal(ks[i], alone[geo][k][0]) and np.array_equal(ds[i], alone[geo][k][1]), (geo, n, i, k)


def _extract_view(ext, view):
    import torch

    n, cap = view.shape[0], ext.max_keypoints
    d_kps = torch.zeros((n, cap, 7), dtype=torch.float32, device="cuda")
    d_desc = torch.zeros((n, cap, 32), dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ext.extract_batch_dev(view, d_kps, d_desc, d_n, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    cnt = d_n.cpu().numpy()
    kps = d_kps.cpu().numpy().view(np.uint8).reshape(n, cap, 28)
    return [(kps[i, :cnt[i]].copy().view(api.KP_DTYPE).reshape(-1), d_desc[i, :cnt[i]].cpu().numpy()) for i in range(n)]


@pytest.mark.parametrize("pitch,lead,rows", [(704, 0, 483),    # 4-byte aligned, row pitch and frame pitch larger than the image: the banded path
                                             (1288, 8, 480),   # ... and a base address that is 8 but not 16 bytes aligned
                                             (643, 1, 481)],   # odd pitch, odd base: NOT 4-byte aligned, the fused fallback builds the pyramid
                         ids=["pitch704", "pitch1288+8", "unaligned643+1"])
def test_level0_views(ref, alone, pitch, lead, rows):
    import torch

    geo, order = (640, 480), ["s1", "columns", "s2"]
    frames = np.stack([ref[geo][k][0] for k in order])
    ext = api.ORBextractor(1000, 1.2, NL, 20, 7, max_batch=3)
    ext._bind(640, 480, 3)
    big = torch.full((3 * rows * pitch + 64,), 77, dtype=torch.uint8, device="cuda")
    view = big[lead:lead + 3 * rows * pitch].as_strided((3, 480, 640), (rows * pitch, pitch, 1))
    assert (view.data_ptr() % 4 == 0 and pitch % 4 == 0) == (pitch != 643)
    view.copy_(torch.from_numpy(frames).cuda())
    got = _extract_view(ext, view)
    for i, k in enumerate(order):
        _check_levels(ext, i, ref[geo][k][1], "pitch %d + %d slot %d (%s)" % (pitch, lead, i, k))
        assert np.array_equal(got[i][0], alone[geo][k][0]) and np.array_equal(got[i][1], alone[geo][k][1]), (pitch, lead, i, k)


def test_other_geometries_through_the_bands():
    """752 x 480 (level widths that are multiples of eight next to ones that are not), 1280 x 720 (sixteen bands in the first segment: the tiles
    of eight would not fit) and 296 x 224, the smallest 4:3 frame with eight levels (level 7: 62 rows, 7 or 8 per band)."""
    for w, h, nf in ((752, 480, 1200), (1280, 720, 2000), (296, 224, 300)):
        ext, orc = api.ORBextractor(nf, 1.2, NL, 20, 7), ob.OrbOracle(nf)
        img = synth.synth_frame(w, h, 90)
        kg, dg = ext(img)
        ko, do = orc.extract(img)
        for l in range(NL):
            assert np.array_equal(ext.level(0, l), orc.level(l)), (w, h, l)
        assert np.array_equal(dg, do) and len(kg) == len(ko)
