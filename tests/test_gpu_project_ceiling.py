"""slamit_project at its stated capacity: SLAMIT_PROJECT_MAX_N points in one problem equal the g++-built header bit for bit, and one
point more is refused before anything is launched."""
import ctypes as C

import numpy as np
import pytest

from tests import project_ref as ref
from tests.test_gpu_project import same_as_header
from weiner_slamit_v2_amd import api, synth

pytestmark = pytest.mark.gpu


def test_project_at_65536_points_and_one_past_it():
    n = api.PROJECT_MAX_N
    assert n == 65536
    pr = synth.synth_project(0, n + 1, "FUSE", 3.0)
    at = ref.head(pr, n)
    out = api.project(at)
    h = ref.host_points(at)
    same_as_header(out, h, n)
    assert set(int(s) for s in out["status"]) == set(range(8)) and out["n_valid"] > 5000
    assert out["status"][-1] == h["status"][-1] and np.array_equal(out["uvr"][-64:].view(np.uint32), h["uvr"][-64:].view(np.uint32))   # the last wavefront
    with pytest.raises(api.SlamitError, match="SLAMIT_PROJECT_MAX_N") as e:
        api.project(pr)
    assert "(-1)" in str(e.value)                                    # SLAMIT_ERR_ARG
    rec = api.ProjectBatchRec(1, n + 1)
    assert api.lib().slamit_project_batch_dev(0, C.byref(rec), None) == -1
