"""slamit_stereo_match* on the device against tests/stereo_ref.py's restatement of Frame::ComputeStereoMatches.

Every float of the walk is an IEEE +, -, *, / or roundf of csrc/stereo.h, compiled without contraction on both sides, and every
sum an exact integer: u_right, depth, the integers and the statuses equal the restatement's BIT FOR BIT; no tolerance appears."""
import ctypes as C

import numpy as np
import pytest

from tests import stereo_ref as ref
from weiner_slamit_v2_amd import api, synth

pytestmark = pytest.mark.gpu


def test_hand_made_fixture_at_wavefront_and_workgroup_edges():
    full = ref.mixed(2)
    frames = [ref.head(full, n) for n in (1, 63, 64, 65, 130)] + [ref.head(full, 0), ref.head(full, 130, 0)]
    assert [len(f["kl"]) for f in frames] == [1, 63, 64, 65, 130, 0, 130] and len(frames[-1]["kr"]) == 0
    outs = ref.run_device(frames)
    seen = set()
    for f, out in zip(frames, outs):
        want = ref.restate(f)
        ref.assert_same(out, want, "n_left %d n_right %d" % (len(f["kl"]), len(f["kr"])))
        seen |= set(int(s) for s in out["status"])
    assert seen == {0, 1, 2, 3, 4, 6, 7, 8}
    # without right keypoints every row is empty: status 1, except the left keypoints that are departures on entry
    assert outs[5]["n_matched"] == 0 and outs[6]["n_matched"] == 0 and np.isin(outs[6]["status"], (1, 8)).all() and (outs[6]["status"] == 1).sum() >= 120


def test_every_hand_made_fixture_and_case_in_one_batch():
    frames = [ref.mixed(s) for s in (0, 4)] + [c[1] for c in ref.cases()]
    outs = ref.run_device(frames)
    for i, (f, out) in enumerate(zip(frames, outs)):
        ref.assert_same(out, ref.restate(f), "frame %d" % i)


def _extract_pairs(pitch=None):
    """3 different pairs through two handles and the stereo match, all on one stream -> everything the checks need"""
    import torch

    pairs = [synth.synth_stereo_pair(320, 240, i)[:2] for i in ref.EXTRACTOR_SEEDS]
    imgs = [np.stack([p[side] for p in pairs]) for side in (0, 1)]
    exts = [api.ORBextractor(500, 1.2, 8, 20, 7, max_batch=3) for _ in range(2)]
    for e in exts:
        e._bind(320, 240, 3)
    cap = exts[0].max_keypoints
    d_imgs = []
    for im in imgs:
        if pitch is None:
            d_imgs.append(torch.from_numpy(im).cuda())
        else:                                              # a view into a larger buffer: row stride != width
            big = torch.zeros((3, 241, pitch), dtype=torch.uint8, device="cuda")
            view = big.view(-1).as_strided((3, 240, 320), (241 * pitch, pitch, 1))
            view.copy_(torch.from_numpy(im).cuda())
            d_imgs.append(view)
    t = {}
    for side in ("left", "right"):
        t["kps_" + side] = torch.zeros((3, cap, 7), dtype=torch.float32, device="cuda")
        t["desc_" + side] = torch.zeros((3, cap, 32), dtype=torch.uint8, device="cuda")
        t["n_" + side] = torch.zeros(3, dtype=torch.int32, device="cuda")
    sc, inv = np.zeros(16, np.float32), np.zeros(16, np.float32)
    sc[:8], inv[:8] = exts[0].GetScaleFactors(), exts[0].GetInverseScaleFactors()
    t.update(mb=torch.full((3,), 1.0, device="cuda"), mbf=torch.full((3,), 40.0, device="cuda"), scale=torch.from_numpy(sc).cuda(),
             inv_scale=torch.from_numpy(inv).cuda(), workspace=torch.zeros(api.stereo_match_workspace(3, cap), dtype=torch.uint8, device="cuda"),
             n_matched=torch.full((3,), -7, dtype=torch.int32, device="cuda"))
    for k, dt in (("u_right", torch.float32), ("depth", torch.float32), ("status", torch.uint8), ("best_r", torch.int32), ("ham_dist", torch.int32),
                  ("sad_dist", torch.int32)):
        t[k] = torch.full((3, cap), ref.SENTINEL[k], dtype=dt, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    assert s.cuda_stream != 0
    for e, d_im, side in zip(exts, d_imgs, ("left", "right")):
        e.extract_batch_dev(d_im, t["kps_" + side], t["desc_" + side], t["n_" + side], stream=s.cuda_stream)
    t["left"], t["right"] = exts[0].pyramid_view(), exts[1].pyramid_view()
    api.stereo_match_batch_dev(t, stream=s.cuda_stream)
    s.synchronize()
    # the restatement's frames: the device's keypoints and the planes slamit_orb_level copies out
    frames = []
    for f in range(3):
        side = []
        for e, name in zip(exts, ("left", "right")):
            n = int(t["n_" + name][f])
            k = t["kps_" + name][f, :n].cpu().numpy().view(np.uint8).reshape(n, 28).copy().view(api.KP_DTYPE).reshape(-1)
            side.append((k.astype(ref.KP_DTYPE), t["desc_" + name][f, :n].cpu().numpy(), [np.ascontiguousarray(e.level(f, l)[19:-19, 19:-19]) for l in range(8)]))
        fr = ref.frame_of(side[0][2], side[1][2], side[0][0], side[0][1], side[1][0], side[1][1], 1.0, 40.0)
        fr["scale"], fr["inv_scale"] = sc, inv
        frames.append(fr)
    return exts, t, frames, d_imgs


def test_extract_then_stereo_on_one_stream_device_and_host_forms():
    exts, t, frames, _ = _extract_pairs()
    view = t["left"]
    assert view.nlevels == 8 and view.nframes == 3 and (view.level[0].w, view.level[0].h, view.level[0].stride) == (320, 240, 320)
    outs = ref.device_outputs(t, frames)
    for f, (fr, out) in enumerate(zip(frames, outs)):
        want = ref.restate(fr)
        c = ref.status_counts(want)
        print("pair %d: %d left, %d right, statuses %s" % (f, len(fr["kl"]), len(fr["kr"]), c.tolist()))
        assert c[0] >= 0.3 * len(fr["kl"]) and c[7] >= 1 and c[8] == 0
        ref.assert_same(out, want, "device form, pair %d" % f)
        host = api.stereo_match(exts[0], exts[1], fr["kl"], fr["dl"], fr["kr"], fr["dr"], 1.0, 40.0, frame=f)
        ref.assert_same(host, want, "host form, pair %d" % f)
    assert len({tuple(o["status"][:50]) for o in outs}) == 3            # three different pairs


def test_level_0_from_a_strided_view_of_the_callers_buffer():
    exts, t, frames, d_imgs = _extract_pairs(pitch=352)
    view = t["left"]
    assert view.level[0].stride == 352 and view.level[0].frame_stride == 241 * 352 and view.level[0].plane == d_imgs[0].data_ptr()
    assert view.level[1].stride != 352
    for f, (fr, out) in enumerate(zip(frames, ref.device_outputs(t, frames))):
        ref.assert_same(out, ref.restate(fr), "strided input, pair %d" % f)


def test_view_before_any_extract_and_mismatched_handles():
    ext = api.ORBextractor(500, 1.2, 8, 20, 7)
    ext._bind(320, 240, 1)
    v = api.PyramidView()
    assert api.lib().slamit_orb_pyramid_view(ext._h, C.byref(v)) == -4            # SLAMIT_ERR_STATE
    assert b"no extract call yet" in api.lib().slamit_last_error()
    with pytest.raises(api.SlamitError, match=r"\(-4\)"):
        ext.pyramid_view()
    img = synth.synth_frame(320, 240, 0)
    kps, desc = ext(img)
    assert ext.pyramid_view().nframes == 1
    others = (api.ORBextractor(500, 1.2, 8, 20, 7), synth.synth_frame(352, 240, 0)), (api.ORBextractor(500, 1.2, 7, 20, 7), img), \
        (api.ORBextractor(500, 1.1, 8, 20, 7), img)
    for other, im in others:                                                      # geometry, level count, scale factor
        other(im)
        with pytest.raises(api.SlamitError, match=r"\(-1\).*differ"):
            api.stereo_match(ext, other, kps, desc, kps, desc, 1.0, 40.0)
    # a frame against itself: every keypoint finds itself at SAD 0, so the median and thDist are 0 and no match is below it
    out = api.stereo_match(ext, ext, kps, desc, kps, desc, 1.0, 40.0)
    assert (out["ham_dist"] == 0).all() and (out["best_r"] == np.arange(len(kps))).all() and (out["sad_dist"] == 0).all()
    assert set(int(s) for s in out["status"]) == {6, 7} and out["n_matched"] == 0 and (out["u_right"] == -1).all()
