"""The frame tests/test_gpu_stereo_ceiling.py runs at SLAMIT_STEREO_MAX_KP keypoints per side is admissible (no GPU)."""
import numpy as np

from tests import stereo_ref as ref


def test_the_ceiling_frame_is_at_the_ceiling_and_admissible():
    from weiner_slamit_v2_amd import api

    fr = ref.ceiling_frame()
    assert len(fr["kl"]) == len(fr["kr"]) == ref.CEILING_N == api.STEREO_MAX_KP == 8191
    assert [p.shape for p in fr["left"]] == [(64, 96), (53, 80), (44, 67)]
    r = ref.restate(fr)
    c = ref.status_counts(r)
    print("ceiling frame: statuses %s, median SAD %d" % (c.tolist(), r["median"]))
    assert c[0] >= 0.3 * ref.CEILING_N and c[7] >= 1 and c[2] >= 100 and c[3] >= 1 and c[4] >= 1 and c[6] >= 1
    # the selection's key keeps the right index in 16 bits: matches must reach the last indices on both sides
    assert r["best_r"].max() >= ref.CEILING_N - 64 and np.flatnonzero(r["status"] == 0).max() >= ref.CEILING_N - 64
    ref.assert_same(ref.host_frame(fr), r, "ceiling")
