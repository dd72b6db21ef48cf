"""GPU parity of the two filters behind the pyramid, planes and not only keypoints (a wrong border row rarely moves a keypoint):

blur_stream_kernel walks a strip of 64 rows by relative iteration -- three fill steps, one generic step, a steady range with running
pointers, no reflection and unconditional stores, run for the smallest count among a wave's lanes, and a generic tail.  The level
heights below put the seams of that walk on every kind of strip: one short strip that reflects at both ends (62, 63), exactly one
strip (64), a last strip of one or three rows (65, 129; 67), a second-to-last strip whose look-ahead row ylast + 10 is the last
row (64 k + 11), one past it (64 k + 10) or two past it (64 k + 9), both parities; widths 64 k + 1 (a one-column right strip) and
widths that are no multiple of four.  Frames of 257 columns and more have strips inside the level (blur_stream_kernel<false>)
beside the edge strips (<true>).

band_item / rs_item8 run one horizontal pass per distinct source row: a destination row takes over its predecessor's second pass
when the row table names the same source row.  Scale factors 1.2, 1.1 and 1.005 (sharing on nearly every row; at 1.005 the rows map
one to one and the bottom row clamps both of its source rows to the same index) go through pyramid_bands_kernel; 1.43 and 1.5 take the
per-level chain with resize_rows8_kernel on the levels whose taps fit its windows (337, 236 and 115 rows at 1.43, 142 rows at 1.5:
dh % 4 = 1, 0, 3, 2) and 1.9 the chain with the four-pixel kernel throughout (sharing rare); the level heights cover dh % 4 = 1, 2, 3,
where the last group of four repeats clamped rows.  Which path a geometry takes is orb_plan.cc's decision (plan_bands, rows8_table).
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
        bad = np.flatnonzero((got != want).any(axis=1))
        assert len(bad) == 0, "%s: blurred level %d differs in rows %s" % (tag, l, bad[:8].tolist())


def _check(img, nf, sf, nl, sizes, tag):
    ext, orc = api.ORBextractor(nf, sf, nl, 20, 7), ob.OrbOracle(nf, sf, nl, 20, 7)
    kg, dg = ext(img)
    ko, do = orc.extract(img)
    assert [orc.level_size(l) for l in range(nl)] == sizes, "%s: the level sizes this case was chosen for" % tag
    _check_planes(ext, 0, orc, nl, tag)
    _assert_same(kg, dg, ko, do, tag)


# (w, h, levels) -> (w, h) of every level at scale factor 1.2
WALK = {
    (268, 223, 8): [(268, 223), (223, 186), (186, 155), (155, 129), (129, 108), (108, 90), (90, 75), (75, 62)],   # 129 = 128 + 1 both ways, 75 = 64 + 11, 62
    (321, 241, 8): [(321, 241), (268, 201), (223, 167), (186, 139), (155, 116), (129, 97), (108, 81), (90, 67)],  # 321 = 320 + 1; 201 = 192 + 9, 139 = 128 + 11, 67
    (257, 74, 2): [(257, 74), (214, 62)],    # 74 = 64 + 10; 257 = 256 + 1; 214 is no multiple of 4
    (321, 76, 2): [(321, 76), (268, 63)],
    (258, 77, 2): [(258, 77), (215, 64)],
    (263, 78, 2): [(263, 78), (219, 65)],
}


@pytest.mark.parametrize("geo", sorted(WALK), ids=lambda g: "%dx%dx%d" % g)
def test_blur_walk_seams(geo):
    w, h, nl = geo
    _check(synth.synth_frame(w, h, 80), 300, 1.2, nl, WALK[geo], "%dx%d" % (w, h))


def test_walk_cases_are_all_there():
    heights = {s[1] for sizes in WALK.values() for s in sizes}
    widths = {s[0] for sizes in WALK.values() for s in sizes}
    assert {62, 63, 64, 65, 67} <= heights and any(x % 2 for x in heights) and any(x % 2 == 0 for x in heights)
    assert all(any(x > 64 and x % 64 == r for x in heights) for r in (9, 10, 11))
    assert any(x % 64 == 1 for x in widths) and any(x % 4 for x in widths)


@pytest.mark.parametrize("geo", [(268, 223, 8), (257, 74, 2)], ids=lambda g: "%dx%dx%d" % g)
def test_blur_walk_on_saturated_blocks(geo):
    w, h, nl = geo
    _check(_blocks(w, h, 9), 300, 1.2, nl, WALK[geo], "blocks %dx%d" % (w, h))
    _check(np.full((h, w), 255, np.uint8), 300, 1.2, nl, WALK[geo], "white %dx%d" % (w, h))


PYRAMID = [
    # banded: sharing on nearly every row; 205, 187, 170, 154 rows: dh % 4 = 1, 3, 2, 2
    (300, 226, 1.1, 6, [(300, 226), (273, 205), (248, 187), (225, 170), (205, 154), (186, 140)]),
    # banded, rows one to one: every destination row shares, the bottom row clamps both source rows to row 95 (and 95 rows: dh % 4 = 3)
    (268, 96, 1.005, 3, [(268, 96), (267, 96), (265, 95)]),
    # the per-level chain, eight pixels per lane on levels 1, 2 and 4 (337, 236, 115 rows) / on level 3 (142 rows)
    (650, 482, 1.43, 5, [(650, 482), (455, 337), (318, 236), (222, 165), (155, 115)]),
    (641, 480, 1.5, 4, [(641, 480), (427, 320), (285, 213), (190, 142)]),
    # the chain with four pixels per lane: consecutive destination rows rarely share a source row
    (400, 300, 1.9, 3, [(400, 300), (211, 158), (111, 83)]),
]


@pytest.mark.parametrize("case", PYRAMID, ids=lambda c: "%dx%d@%g" % c[:3])
def test_pyramid_row_reuse(case):
    w, h, sf, nl, sizes = case
    _check(synth.synth_frame(w, h, 81), 500, sf, nl, sizes, "%dx%d@%g" % (w, h, sf))
    _check(_blocks(w, h, 10), 500, sf, nl, sizes, "blocks %dx%d@%g" % (w, h, sf))


def test_batch_of_17_through_the_xcd_dealt_grids():
    """From 16 frames the banded pyramid deals whole frames to the XCDs; the blur's strips of all frames share one launch."""
    geo = (268, 223, 8)
    w, h, nl = geo
    kinds = [synth.synth_frame(w, h, 82), _blocks(w, h, 11), synth.synth_frame(w, h, 83), np.full((h, w), 255, np.uint8)]
    orc = ob.OrbOracle(300, 1.2, nl, 20, 7)
    ext = api.ORBextractor(300, 1.2, nl, 20, 7, max_batch=17)
    ks, ds = ext.extract_batch(np.stack([kinds[i % 4] for i in range(17)]))
    for k, img in enumerate(kinds):
        ko, do = orc.extract(img)
        assert [orc.level_size(l) for l in range(nl)] == WALK[geo]
        for i in range(k, 17, 4):
            _check_planes(ext, i, orc, nl, "batch 17 slot %d" % i)
            _assert_same(ks[i], ds[i], ko, do, "batch 17 slot %d" % i)
