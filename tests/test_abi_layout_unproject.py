"""The C-ABI of the RGB-D depth lookup and the closest-point walk, without a GPU: the structs of include/slamit.h against the ctypes
and numpy mirrors of the binding, the enumerators, the exported symbols, and the refusals the host makes before it looks for a device."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests.helpers import ROOT

STRUCTS = {   # C name -> (ctypes mirror, fields whose offsets are compared)
    "slamit_depth_plane": ("DepthPlane", ("data", "pitch", "width", "height", "type", "factor")),
    "slamit_rgbd_problem": ("RgbdProblem", ("plane", "mbf", "n", "kps", "kps_un")),
    "slamit_rgbd_result": ("RgbdResult", ("u_right", "depth", "status")),
    "slamit_rgbd_batch_rec": ("RgbdBatchRec", ("nframes", "cap", "d_planes", "d_mbf", "d_kps", "d_kps_un", "d_n", "d_u_right", "d_depth", "d_status")),
    "slamit_unproject_frame": ("UnprojectFrame", ("fx", "invfy", "Rwc", "Ow", "th_depth", "min_points", "mode", "ctor", "n_levels", "scale_factors")),
    "slamit_unproject_counts": ("UnprojectCounts", ("n_candidates", "n_close", "n_visited", "n_created", "n_total", "n_map")),
    "slamit_unproject_problem": ("UnprojectProblem", ("frame", "n", "kps_un", "depth", "tracked")),
    "slamit_unproject_result": ("UnprojectResult", ("status", "order", "pos", "normal", "max_dist", "min_dist", "counts")),
    "slamit_unproject_batch_rec": ("UnprojectBatchRec", ("nframes", "cap", "d_frames", "d_n", "d_kps_un", "d_depth", "d_tracked", "d_pos", "d_octave",
                                                         "d_skip", "d_normal", "d_max_dist", "d_min_dist", "d_status", "d_order", "d_counts")),
}
SYMBOLS = ("slamit_rgbd_depth", "slamit_rgbd_depth_batch", "slamit_rgbd_depth_batch_dev", "slamit_unproject_closest", "slamit_unproject_closest_batch",
           "slamit_unproject_closest_batch_dev")


def test_struct_layouts_match_the_header(tmp_path):
    from weiner_slamit_v2_amd import api

    lines = []
    for cname, (_, fields) in STRUCTS.items():
        lines.append('printf("%%zu", sizeof(%s));' % cname)
        lines += ['printf(" %%zu", offsetof(%s, %s));' % (cname, f) for f in fields]
        lines.append('printf("\\n");')
    lines.append('printf("%d %d %d %d %d %d %d\\n", SLAMIT_DEPTH_F32, SLAMIT_DEPTH_U16, SLAMIT_UNPROJECT_CLOSEST, SLAMIT_UNPROJECT_ALL, '
                 'SLAMIT_UNPROJECT_CTOR_FRAME, SLAMIT_UNPROJECT_CTOR_KEYFRAME, SLAMIT_STEREO_MAX_KP);')
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "slamit.h"\nint main(void) {\n%s\nreturn 0;\n}\n' % "\n".join(lines)
    c = str(tmp_path / "_layout.c")
    open(c, "w").write(src)
    exe = str(tmp_path / "_layout")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), c, "-o", exe])   # the header is plain C
    rows = [[int(v) for v in line.split()] for line in subprocess.check_output([exe]).decode().splitlines()]
    for row, (cname, (mirror, fields)) in zip(rows, STRUCTS.items()):
        m = getattr(api, mirror)
        assert row[0] == C.sizeof(m), cname
        assert row[1:] == [getattr(m, f).offset for f in fields], cname
    assert rows[-1] == [api.DEPTH_TYPES.index("f32"), api.DEPTH_TYPES.index("u16"), api.UNPROJECT_MODES.index("CLOSEST"), api.UNPROJECT_MODES.index("ALL"),
                        api.UNPROJECT_CTORS.index("FRAME"), api.UNPROJECT_CTORS.index("KEYFRAME"), api.STEREO_MAX_KP]
    # the numpy records of the resident forms are the same structs
    for dt, m in ((api.UNPROJECT_FRAME_DTYPE, api.UnprojectFrame), (api.DEPTH_PLANE_DTYPE, api.DepthPlane)):
        assert dt.itemsize == C.sizeof(m)
        assert all(dt.fields[name][1] == getattr(m, name).offset for name in dt.names)
    assert tuple(name for name, _ in api.UnprojectCounts._fields_) == api.UNPROJECT_COUNTS


def test_symbols_are_exported_and_bound():
    from weiner_slamit_v2_amd import api, build

    build.build()
    lib = api.lib()
    for s in SYMBOLS:
        assert hasattr(lib, s) and s in api.EXPORTS and getattr(lib, s).argtypes is not None, s
    for f in ("rgbd_depth", "rgbd_depth_batch", "rgbd_depth_batch_dev", "unproject_closest", "unproject_closest_batch", "unproject_closest_batch_dev"):
        assert callable(getattr(api, f))


def test_refusals_need_no_device():
    """Every refusal is made on the host before a launch: it is the same with and without a GPU, it leaves a message, and the
    outputs are untouched."""
    from tests import unproject_ref as ur
    from weiner_slamit_v2_amd import api

    pr = ur.fixture("min0")
    cases = [(dict(pr, n_levels=0), -1, "n_levels"), (dict(pr, n_levels=17), -1, "n_levels"), (dict(pr, mode=2), -1, "mode"),
             (dict(pr, min_points=-1), -1, "min_points"), (dict(pr, ctor=5), -1, "ctor")]
    for bad, code, word in cases:
        try:
            api.unproject_closest(bad)
            raise AssertionError("accepted " + word)
        except api.SlamitError as e:
            assert "(%d)" % code in str(e) and word in str(e), str(e)
    big = dict(pr, n=8192, kps_un=np.zeros(8192, api.KP_DTYPE), depth=np.ones(8192, np.float32), tracked=np.zeros(8192, np.uint8))
    try:
        api.unproject_closest(big)
        raise AssertionError("accepted 8192 keypoints")
    except api.SlamitError as e:
        assert "(-3)" in str(e) and "SLAMIT_STEREO_MAX_KP" in str(e)
    # a missing array, through the raw entry point; the outputs keep their bytes
    rec = api.unproject_frame_record(pr)
    P, R = api.UnprojectProblem(), api.UnprojectResult()
    C.memmove(C.byref(P.frame), rec.ctypes.data, C.sizeof(api.UnprojectFrame))
    n = int(pr["n"])
    status = np.full(n, 77, np.uint8)
    P.n, P.kps_un, P.depth, P.tracked = n, pr["kps_un"].ctypes.data, pr["depth"].ctypes.data, None
    R.status = status.ctypes.data
    assert api.lib().slamit_unproject_closest(0, C.byref(P), C.byref(R)) == -1
    assert b"null array" in api.lib().slamit_last_error() and np.all(status == 77)
    # the RGB-D lookup: element type, pitch, capacity
    rg = ur.rgbd_fixture("u16_one")
    Q, S = api.RgbdProblem(), api.RgbdResult()
    out = np.full((3, int(rg["n"])), 9.0, np.float32)
    st = np.full(int(rg["n"]), 9, np.uint8)
    Q.plane = api.DepthPlane(rg["storage"].ctypes.data, 2, rg["width"], rg["height"], 1, 1.0)   # pitch below a row's bytes
    Q.mbf, Q.n, Q.kps, Q.kps_un = 38.6, int(rg["n"]), rg["kps"].ctypes.data, rg["kps_un"].ctypes.data
    S.u_right, S.depth, S.status = out[0].ctypes.data, out[1].ctypes.data, st.ctypes.data
    assert api.lib().slamit_rgbd_depth(0, C.byref(Q), C.byref(S)) == -1 and b"geometry" in api.lib().slamit_last_error()
    Q.plane.pitch, Q.plane.type = rg["storage"].strides[0], 2
    assert api.lib().slamit_rgbd_depth(0, C.byref(Q), C.byref(S)) == -1 and b"element type" in api.lib().slamit_last_error()
    Q.plane.type, Q.n = 1, 8192
    assert api.lib().slamit_rgbd_depth(0, C.byref(Q), C.byref(S)) == -3
    assert np.all(out == 9.0) and np.all(st == 9)
    # nothing to do is valid without a device
    assert api.lib().slamit_unproject_closest_batch(0, 0, None, None) == 0 and api.lib().slamit_rgbd_depth_batch(0, 0, None, None) == 0
    assert api.unproject_closest(ur.shape_fixture(0))["n_candidates"] == 0
