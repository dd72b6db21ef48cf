"""The eight "batch of problems" host-form calls write the caller's arrays to exactly their length: every caller output is allocated with
64 sentinel bytes on either side, a batch of three problems (n = 65, 0, 1) is run through api.lib() and api.py's ctypes structures, and the
sentinels must be intact, the outputs equal bit for bit to those of the same problems run singly, and the empty problem's outputs untouched.

slamit_pnp_refine_batch refuses a subset of fewer than four correspondences, so its third problem has n = 4, the smallest it accepts.
The two RANSAC calls run with n_hyp = 5 for every problem, and once more with n_hyp = 0 for one that has correspondences."""
import ctypes as C

import numpy as np
import pytest

from weiner_slamit_v2_amd import api, synth

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xA5
SIZES = (65, 0, 1)


class Guarded:
    """`count` elements of `dtype` for the library to write, every byte FILL, with GUARD bytes of FILL on either side"""

    def __init__(self, count, dtype):
        self.nbytes = int(count) * np.dtype(dtype).itemsize
        self.raw = np.full(GUARD + self.nbytes + GUARD, FILL, np.uint8)
        self.ptr = self.raw.ctypes.data + GUARD

    def payload(self):
        return self.raw[GUARD:GUARD + self.nbytes].tobytes()

    def guards_intact(self):
        return bool((self.raw[:GUARD] == FILL).all() and (self.raw[GUARD + self.nbytes:] == FILL).all())

    def untouched(self):
        return bool((self.raw == FILL).all())


def cut(pr, n, keys):
    """the problem with its per-point arrays cut to the first n entries"""
    q = dict(pr)
    for k in keys:
        if q.get(k) is not None:
            q[k] = np.ascontiguousarray(q[k][:n])
    q["n"] = n
    return q


def outputs(R, o, spec, n):
    """one guarded array per (field, dtype, elements per point) of spec, for n points; an empty problem gets room for three, all of which
    has to stay as it is"""
    for key, dt, per in spec:
        o[key] = Guarded(per * (n or 3), dt)
        setattr(R, key, o[key].ptr)


def inputs(P, pr, spec):
    keep = []
    for key, dt in spec:
        if pr.get(key) is not None:
            a = np.ascontiguousarray(pr[key], dt)
            setattr(P, key, a.ctypes.data)
            keep.append(a)
    return keep


# ---- one filler per call: (P[i], R[i], problem, guarded outputs by name, variant) -> what has to stay alive --------------------------

FRUSTUM_OUT = (("status", np.uint8, 1), ("proj", np.float32, 3), ("view_cos", np.float32, 1), ("level", np.int32, 1), ("uvr", np.float32, 3),
               ("level_min", np.int32, 1), ("level_max", np.int32, 1), ("valid", np.uint8, 1))
FRUSTUM_IN = (("pos", np.float32), ("normal", np.float32), ("max_dist", np.float32), ("min_dist", np.float32), ("skip", np.uint8))


def fill_frustum(P, R, pr, o, v):
    rec = api.frustum_frame_record(pr)
    C.memmove(C.byref(P.frame), rec.ctypes.data, C.sizeof(api.FrustumFrame))
    P.n, R.n_in_view = pr["n"], 77
    outputs(R, o, FRUSTUM_OUT, pr["n"])
    return inputs(P, pr, FRUSTUM_IN)


PROJECT_OUT = (("status", np.uint8, 1), ("proj", np.float32, 2), ("level", np.int32, 1), ("uvr", np.float32, 3), ("level_min", np.int32, 1),
               ("level_max", np.int32, 1), ("valid", np.uint8, 1))
PROJECT_IN = FRUSTUM_IN + (("octave", np.int32),)


def fill_project(P, R, pr, o, v):
    rec = api.project_camera_record(pr)
    C.memmove(C.byref(P.camera), rec.ctypes.data, C.sizeof(api.ProjectCamera))
    P.n, R.n_valid = pr["n"], 77
    outputs(R, o, PROJECT_OUT, pr["n"])
    if v["ur"]:
        o["ur"], o["bf"] = Guarded(pr["n"] or 3, np.float32), 35.0 + pr["n"] % 7
    return inputs(P, pr, PROJECT_IN)


TRI_IN = (("kp1_xy", np.float32), ("kp2_xy", np.float32), ("octave1", np.int32), ("octave2", np.int32), ("scale_factors1", np.float32),
          ("level_sigma2_1", np.float32), ("scale_factors2", np.float32), ("level_sigma2_2", np.float32))
TRI_STEREO_IN = tuple((k, np.float32) for k in ("ur1", "ur2", "depth1", "depth2", "raw1_xy", "raw2_xy"))
TRI_POINT_KEYS = ("kp1_xy", "kp2_xy", "octave1", "octave2", "ur1", "ur2", "depth1", "depth2", "raw1_xy", "raw2_xy")


def fill_triangulate(P, R, pr, o, v):
    for key, k in (("Tcw1", 12), ("Tcw2", 12), ("intr1", 6), ("intr2", 6)):
        setattr(P, key, (C.c_float * k)(*[float(x) for x in np.asarray(pr[key], np.float32).reshape(-1)]))
    P.n, P.n_levels, P.ratio_factor, R.n_accepted = pr["n"], int(pr["n_levels"]), float(pr["ratio_factor"]), 77
    outputs(R, o, (("status", np.uint8, 1), ("x3d", np.float32, 3)), pr["n"])
    if v["source"]:
        o["source"] = Guarded(pr["n"] or 3, np.uint8)
    keep = inputs(P, pr, TRI_IN)
    if v["stereo"]:
        t = api.TriangulateStereo()
        keep += inputs(t, pr, TRI_STEREO_IN)
        t.mb1, t.mb2, t.bf = float(pr["mb1"]), float(pr["mb2"]), float(pr["bf"])
        o["stereo record"] = t
    return keep


def fill_rgbd(P, R, pr, o, v):
    plane = pr["plane"]
    P.plane = api.DepthPlane(plane.ctypes.data, plane.strides[0], plane.shape[1], plane.shape[0], 1 if plane.dtype == np.uint16 else 0, float(pr["factor"]))
    P.mbf, P.n = float(pr["mbf"]), pr["n"]
    outputs(R, o, (("u_right", np.float32, 1), ("depth", np.float32, 1), ("status", np.uint8, 1)), pr["n"])
    return inputs(P, pr, (("kps", api.KP_DTYPE), ("kps_un", api.KP_DTYPE))) + [plane]


UNPROJECT_OUT = (("status", np.uint8, 1), ("order", np.int32, 1), ("pos", np.float32, 3), ("normal", np.float32, 3), ("max_dist", np.float32, 1),
                 ("min_dist", np.float32, 1))


def fill_unproject(P, R, pr, o, v):
    rec = api.unproject_frame_record(pr)
    C.memmove(C.byref(P.frame), rec.ctypes.data, C.sizeof(api.UnprojectFrame))
    P.n = pr["n"]
    C.memset(C.byref(R.counts), 0x4D, C.sizeof(api.UnprojectCounts))
    outputs(R, o, UNPROJECT_OUT, pr["n"])
    return inputs(P, pr, (("kps_un", api.KP_DTYPE), ("depth", np.float32), ("tracked", np.uint8)))


def ransac_outputs(R, o, pr, first, per, dtype, bits):
    n, nh = pr["n"], pr["n_hyp"]
    live = n > 0 and nh > 0
    o[first] = Guarded(per * nh if live else 3 * per, dtype)
    o["n_inliers"] = Guarded(nh if live else 3, np.int32)
    setattr(R, first, o[first].ptr)
    R.n_inliers = o["n_inliers"].ptr
    if bits:
        o["inlier_bits"] = Guarded(nh * ((n + 31) // 32) if live else 3, np.uint32)
        R.inlier_bits = o["inlier_bits"].ptr


def fill_pnp(P, R, pr, o, v):
    P.n, P.n_hyp = pr["n"], pr["n_hyp"]
    P.intr = (C.c_double * 4)(*[float(x) for x in pr["intr"]])
    ransac_outputs(R, o, pr, "pose", 12, np.float64, v["bits"])
    return inputs(P, pr, (("p3d", np.float32), ("p2d", np.float32), ("max_err", np.float32), ("quads", np.int32)))


def fill_pnp_refine(P, R, pr, o, v):
    P.n = pr["n"]
    P.intr = (C.c_double * 4)(*[float(x) for x in pr["intr"]])
    R.pose, R.n_inliers = (C.c_double * 12)(*([7.0] * 12)), 77
    if v["bits"]:
        o["inlier_bits"] = Guarded((pr["n"] + 31) // 32 or 3, np.uint32)
        R.inlier_bits = o["inlier_bits"].ptr
    return inputs(P, pr, (("p3d", np.float32), ("p2d", np.float32), ("max_err", np.float32), ("subset_bits", np.uint32)))


def fill_sim3(P, R, pr, o, v):
    P.n, P.n_hyp, P.fix_scale = pr["n"], pr["n_hyp"], int(pr["fix_scale"])
    P.intr1, P.intr2 = (C.c_float * 4)(*[float(x) for x in pr["intr1"]]), (C.c_float * 4)(*[float(x) for x in pr["intr2"]])
    ransac_outputs(R, o, pr, "t12", 13, np.float32, v["bits"])
    return inputs(P, pr, (("x1", np.float32), ("x2", np.float32), ("max_err1", np.float32), ("max_err2", np.float32), ("triples", np.int32)))


ZERO4 = bytes(4)
# name -> (problem structure, result structure, filler, the result's own fields that are outputs, what those hold after an empty problem:
# the counts are documented to be zeroed, Refine() writes nothing)
CALLS = {
    "frustum": (api.FrustumProblem, api.FrustumResult, fill_frustum, ("n_in_view",), ZERO4),
    "project": (api.ProjectProblem, api.ProjectResult, fill_project, ("n_valid",), ZERO4),
    "triangulate": (api.TriangulateProblem, api.TriangulateResult, fill_triangulate, ("n_accepted",), ZERO4),
    "rgbd": (api.RgbdProblem, api.RgbdResult, fill_rgbd, (), b""),
    "unproject": (api.UnprojectProblem, api.UnprojectResult, fill_unproject, ("counts",), bytes(24)),
    "pnp": (api.PnpProblem, api.PnpResult, fill_pnp, (), b""),
    "pnp_refine": (api.PnpRefineProblem, api.PnpRefineResult, fill_pnp_refine, ("pose", "n_inliers"), np.full(12, 7.0).tobytes() + (77).to_bytes(4, "little")),
    "sim3": (api.Sim3RansacProblem, api.Sim3RansacResult, fill_sim3, (), b""),
}


def invoke(name, m, P, R, outs, v):
    L = api.lib()
    if name == "frustum":
        return L.slamit_frustum_batch(0, m, P, R)
    if name == "project":
        if not v["ur"]:
            return L.slamit_project_batch_stereo(0, m, P, R, None, None)
        bf = np.array([o["bf"] for o in outs], np.float32)
        urp = (C.c_void_p * m)(*[o["ur"].ptr for o in outs])
        return L.slamit_project_batch_stereo(0, m, P, R, bf.ctypes.data, C.cast(urp, C.c_void_p))
    if name == "triangulate":
        T = (C.POINTER(api.TriangulateStereo) * m)()
        SRC = (C.c_void_p * m)()
        for i, o in enumerate(outs):
            if v["stereo"]:
                T[i] = C.pointer(o["stereo record"])
            if v["source"]:
                SRC[i] = o["source"].ptr
        return L.slamit_triangulate_stereo_batch(0, m, P, T if v["stereo"] else None, R, SRC if v["source"] else None)
    fn = {"rgbd": L.slamit_rgbd_depth_batch, "unproject": L.slamit_unproject_closest_batch, "pnp": L.slamit_pnp_ransac_batch,
          "pnp_refine": L.slamit_pnp_refine_batch, "sim3": L.slamit_sim3_ransac_batch}[name]
    return fn(0, m, P, R)


def run(name, problems, v):
    """-> per problem: ({output name: its bytes}, the bytes of the result structure's own outputs, whether every array is untouched)"""
    PT, RT, fill, own, _ = CALLS[name]
    m = len(problems)
    P, R = (PT * m)(), (RT * m)()
    outs, keep = [{} for _ in problems], []
    for i, pr in enumerate(problems):
        keep.append(fill(P[i], R[i], pr, outs[i], v))
    rc = invoke(name, m, P, R, outs, v)
    assert rc == 0, (name, v, rc)
    res = []
    for i, o in enumerate(outs):
        arrays = {k: g for k, g in o.items() if isinstance(g, Guarded)}
        for k, g in arrays.items():
            assert g.guards_intact(), (name, v, i, k)
        scalars = b"".join(bytes(getattr(R[i], f)) if not isinstance(getattr(R[i], f), int) else int(getattr(R[i], f)).to_bytes(4, "little", signed=True)
                           for f in own)
        res.append(({k: g.payload() for k, g in arrays.items()}, scalars, all(g.untouched() for g in arrays.values())))
    del keep
    return res


def check(name, problems, v, empty):
    """the batch against its problems run singly; empty: the indices of the problems that have nothing to do"""
    batch = run(name, problems, v)
    for i, pr in enumerate(problems):
        single = run(name, [pr], v)[0]
        assert batch[i][1] == single[1], (name, v, i, "the result structure")
        assert batch[i][0].keys() == single[0].keys()
        for k in single[0]:
            assert batch[i][0][k] == single[0][k], (name, v, i, k)
        if i in empty:
            assert batch[i][2] and batch[i][1] == CALLS[name][4], (name, v, i, "an empty problem's outputs")


def test_frustum():
    pr = synth.synth_frustum(seed=3, n=65)
    check("frustum", [cut(pr, n, [k for k, _ in FRUSTUM_IN]) for n in SIZES], {}, {1})


@pytest.mark.parametrize("ur", [False, True])
def test_project(ur):
    probs = [cut(synth.synth_project(seed=4 + i, n=65, form=form), n, [k for k, _ in PROJECT_IN])
             for i, (n, form) in enumerate(zip(SIZES, ("LAST_FRAME", "RELOC", "FUSE")))]
    check("project", probs, {"ur": ur}, {1})


@pytest.mark.parametrize("stereo,source", [(True, True), (True, False), (False, True)])
def test_triangulate(stereo, source):
    pr = synth.synth_triangulation_stereo(n=65, seed=5)
    check("triangulate", [cut(pr, n, TRI_POINT_KEYS) for n in SIZES], {"stereo": stereo, "source": source}, {1})


def test_rgbd():
    pr = synth.synth_rgbd(seed=6, n=65, pad=3)
    check("rgbd", [cut(pr, n, ("kps", "kps_un")) for n in SIZES], {}, {1})


@pytest.mark.parametrize("mode", ["CLOSEST", "ALL"])
def test_unproject(mode):
    pr = synth.synth_unproject(seed=7, n=65, min_points=20, mode=api.UNPROJECT_MODES.index(mode))
    if mode == "ALL":
        pr["tracked"] = None
    check("unproject", [cut(pr, n, ("kps_un", "depth", "tracked")) for n in SIZES], {}, {1})


def with_hyp(pr, n, nh, key, k, keys):
    q = cut(pr, n, keys)
    q["n_hyp"] = nh
    q[key] = np.random.RandomState(100 + n).randint(0, max(n, 1), (nh, k)).astype(np.int32)
    return q


RANSAC_SHAPES = [((65, 5), (0, 5), (1, 5)), ((65, 5), (65, 0), (1, 5))]


@pytest.mark.parametrize("bits", [True, False])
@pytest.mark.parametrize("shapes", RANSAC_SHAPES)
def test_pnp_ransac(shapes, bits):
    pr = synth.synth_pnp(n=65, seed=8)
    check("pnp", [with_hyp(pr, n, nh, "quads", 4, ("p3d", "p2d", "max_err")) for n, nh in shapes], {"bits": bits}, {1})


@pytest.mark.parametrize("bits", [True, False])
def test_pnp_refine(bits):
    pr = synth.synth_pnp(n=65, seed=9)
    probs = []
    for n in (65, 0, 4):
        q = cut(pr, n, ("p3d", "p2d", "max_err"))
        flags = np.zeros(((n + 31) // 32) * 32, np.uint8)
        flags[:n] = np.arange(n) % 3 != 1 if n > 4 else 1
        q["subset_bits"] = np.packbits(flags, bitorder="little").view(np.uint32)
        probs.append(q)
    check("pnp_refine", probs, {"bits": bits}, {1})


@pytest.mark.parametrize("bits", [True, False])
@pytest.mark.parametrize("shapes", RANSAC_SHAPES)
def test_sim3_ransac(shapes, bits):
    pr = synth.synth_sim3_ransac(n=65, seed=10)
    check("sim3", [with_hyp(pr, n, nh, "triples", 3, ("x1", "x2", "max_err1", "max_err2")) for n, nh in shapes], {"bits": bits}, {1})
