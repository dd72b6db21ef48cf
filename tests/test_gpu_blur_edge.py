"""GPU parity of the blur's EDGE strips, planes and not only keypoints: a lane of an edge strip makes ONE 12-byte load per row, at
an offset shifted by 4 where its window would leave the row, and builds its window with byte permutes (csrc/blur_window.h; the plan
itself is checked on the CPU for every width, tests/test_blur_window.py).  The level widths below put every kind of edge lane on
the device:

  one strip that is the left AND the right edge (62, 64 columns; 64 = a full strip whose last lane's load is shifted),
  two strips of which the right one is a single lane (65 .. 67 columns, and 64 k + 1 .. 64 k + 4: one to four stored columns),
  widths with w % 4 = 0, 1, 2, 3,
  a width of exactly 64 k (256): a full right strip whose last lane's window meets the pitch,
  frames wider than 256, where strips inside the level and edge strips share a call and a launch.

A host frame is staged at a pitch of roundup64(w); frames handed over on the device keep the caller's pitch: back to back with
pitch = width (a read past a row's end lands in the next row or frame and shows as a wrong byte), and with a pitch wider than
the row and pad bytes no image holds."""
import numpy as np
import pytest

from oracle import bindings as ob
from weiner_slamit_v2_amd import api, synth

pytestmark = pytest.mark.gpu

NF, SF = 300, 1.2

# (w, h, levels) -> (w, h) of every level at scale factor 1.2
EDGE = {
    (388, 190, 7): [(388, 190), (323, 158), (269, 132), (225, 110), (187, 92), (156, 76), (130, 64)],   # 388 = 384 + 4, 323 = 320 + 3, 130 = 128 + 2
    (257, 80, 2): [(257, 80), (214, 67)],     # 257 = 256 + 1: a right strip of one lane with one stored column
    (307, 80, 2): [(307, 80), (256, 67)],     # 256: a full right strip, its last lane's window ends at the pitch
    (77, 76, 2): [(77, 76), (64, 63)],        # 64: ONE strip, left and right edge, last lane shifted
    (74, 75, 2): [(74, 75), (62, 62)],        # 62: one strip, the smallest level there is
    (80, 78, 2): [(80, 78), (67, 65)],        # 67 = 64 + 3, 80 = 64 + 16: level 0 at pitch = width has a shifted last lane
}


def _assert_same(kg, dg, ko, do, tag=""):
    assert len(kg) == len(ko), "%s keypoint count %d vs oracle %d" % (tag, len(kg), len(ko))
    for f in ("octave", "x", "y", "response", "size", "class_id"):
        assert np.array_equal(kg[f], ko[f]), "%s field %s differs" % (tag, f)
    assert np.array_equal(kg["angle"].view(np.uint32), ko["angle"].view(np.uint32)), "%s angle bits differ" % tag
    assert np.array_equal(dg, do), "%s descriptors differ" % tag


def _blocks(w, h, seed):
    """saturated 16 x 16 blocks: the blur's clamp at 255 and its rounding at 0"""
    cells = np.random.RandomState(seed).randint(0, 2, ((h + 15) // 16, (w + 15) // 16))
    return (np.kron(cells, np.ones((16, 16)))[:h, :w] * 255).astype(np.uint8)


def _check_planes(ext, slot, orc, nl, tag):
    for l in range(nl):
        got, want = ext.level(slot, l), orc.level(l)
        assert got.shape == want.shape and np.array_equal(got, want), "%s: pyramid level %d differs" % (tag, l)
        got, want = ext.blurred(slot, l), orc.blurred(l)
        if want is None:   # the oracle keeps the blurred plane of a level only where the level has keypoints: its blur of its own level then
            want = ob.blur(orc.level(l)[19:-19, 19:-19])
        assert got.shape == want.shape, "%s: blurred level %d is %s, oracle %s" % (tag, l, got.shape, want.shape)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, "%s: blurred level %d (%d x %d) differs at (row, column) %s" % (tag, l, got.shape[1], got.shape[0], bad[:6].tolist())


class _Oracle:
    """The oracle's result for one image, computed once: keypoints, descriptors and its planes stay in the object."""

    def __init__(self, img, nl, sizes):
        self.orc, self.nl = ob.OrbOracle(NF, SF, nl, 20, 7), nl
        self.k, self.d = self.orc.extract(img)
        assert [self.orc.level_size(l) for l in range(nl)] == sizes, "the level sizes this case was chosen for"

    def check(self, ext, slot, kg, dg, tag):
        _check_planes(ext, slot, self.orc, self.nl, tag)
        _assert_same(kg, dg, self.k, self.d, tag)


def _contents(w, h):
    return [("synth", synth.synth_frame(w, h, 90)), ("blocks", _blocks(w, h, 12)), ("white", np.full((h, w), 255, np.uint8))]


@pytest.mark.parametrize("geo", sorted(EDGE), ids=lambda g: "%dx%dx%d" % g)
def test_edge_lanes(geo):
    w, h, nl = geo
    ext = api.ORBextractor(NF, SF, nl, 20, 7)
    for name, img in _contents(w, h):
        kg, dg = ext(img)
        _Oracle(img, nl, EDGE[geo]).check(ext, 0, kg, dg, "%s %dx%d" % (name, w, h))


def test_cases_are_all_there():
    widths = {s[0] for sizes in EDGE.values() for s in sizes}
    assert all(s[0] >= 62 and s[1] >= 62 for sizes in EDGE.values() for s in sizes)
    assert any(62 <= x <= 64 for x in widths) and any(65 <= x <= 67 for x in widths)      # one strip that is both edges; two strips, the right one a single lane
    assert all(any(x > 64 and x % 64 == r for x in widths) for r in (1, 2, 3, 4))         # a right strip of one lane with 1 .. 4 stored columns
    assert {x % 4 for x in widths} == {0, 1, 2, 3}
    assert any(x >= 128 and x % 64 == 0 for x in widths) and 64 in widths                 # full right strips: the shifted load
    assert any(g[0] > 256 for g in EDGE)                                                  # inner and edge strips in one call
    assert any(g[0] % 4 == 0 and g[0] % 64 for g in EDGE)                                 # a level 0 that can lie at pitch = width with a shifted last lane


def test_batch_of_17_shares_the_launch():
    """The strips of all frames share the launch; every frame is checked, the first and the last among them."""
    geo = (388, 190, 7)
    w, h, nl = geo
    kinds = _contents(w, h) + [("synth2", synth.synth_frame(w, h, 91))]
    orcs = [_Oracle(img, nl, EDGE[geo]) for _, img in kinds]
    ext = api.ORBextractor(NF, SF, nl, 20, 7, max_batch=17)
    ks, ds = ext.extract_batch(np.stack([kinds[i % 4][1] for i in range(17)]))
    for i in range(17):
        orcs[i % 4].check(ext, i, ks[i], ds[i], "batch 17 slot %d (%s)" % (i, kinds[i % 4][0]))


def _extract_view(ext, view):
    import torch

    ext._bind(view.shape[2], view.shape[1], view.shape[0])
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


@pytest.mark.parametrize("geo", [(388, 190, 7), (80, 78, 2)], ids=lambda g: "%dx%dx%d" % g)
def test_frames_back_to_back_at_pitch_equal_to_width(geo):
    """Level 0 is the caller's tensor: three frames with no byte between rows or frames.  The last lane of a row (x0 = w - 4) loads
    the row's last 12 bytes; had it loaded its window as it lies, columns w .. w + 3 would be the next row's (the next frame's) first."""
    import torch

    w, h, nl = geo
    kinds = _contents(w, h)
    frames = torch.from_numpy(np.stack([img for _, img in kinds])).cuda()
    assert frames.is_contiguous() and frames.stride(1) == w and frames.stride(0) == w * h and frames.data_ptr() % 4 == 0
    ext = api.ORBextractor(NF, SF, nl, 20, 7, max_batch=3)
    got = _extract_view(ext, frames)
    for i, (name, img) in enumerate(kinds):
        _Oracle(img, nl, EDGE[geo]).check(ext, i, got[i][0], got[i][1], "back to back %s %dx%d" % (name, w, h))


@pytest.mark.parametrize("pad", [4, 12], ids=lambda p: "pitch_w+%d" % p)
def test_padded_level0_pitch(pad):
    """A level-0 pitch wider than the row (the binding passes the tensor's strides): the pad bytes hold 0xA5, which no lane may take
    for a reflected column.  With 4 pad bytes the last lane's window still passes the pitch (shifted), with 12 it does not."""
    import torch

    geo = (388, 190, 7)
    w, h, nl = geo
    kinds = _contents(w, h)[:2]
    pitch = w + pad
    big = torch.full((2, h + 1, pitch), 0xA5, dtype=torch.uint8, device="cuda")
    view = big.view(-1)[4:4 + 2 * (h + 1) * pitch - pitch].as_strided((2, h, w), ((h + 1) * pitch, pitch, 1))
    view.copy_(torch.from_numpy(np.stack([img for _, img in kinds])).cuda())
    assert view.stride(1) == pitch and view.data_ptr() % 4 == 0
    ext = api.ORBextractor(NF, SF, nl, 20, 7, max_batch=2)
    got = _extract_view(ext, view)
    for i, (name, img) in enumerate(kinds):
        _Oracle(img, nl, EDGE[geo]).check(ext, i, got[i][0], got[i][1], "pitch %d %s" % (pitch, name))
