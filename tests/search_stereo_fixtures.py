"""The synth_search_stereo fixtures the CPU and GPU tests of the right-image gate share, and the rules they run under.

m = 200 queries everywhere.  (er_mode, n, crowd) -> (seed, displaced_frac).  The seeds are chosen so that, at every size of 63
keypoints and more, the gate matters: the model's matches differ from the monocular run's on at least 20 queries and the gate
removes the Hamming-best candidate of at least 10 (tests/test_search_stereo_ref.py asserts it and states the counts).  A frame
of about 64 keypoints, 15 % of them taken on entry and half of them stereo, gives some 40 monocular matches, 20 of them on stereo
keypoints: there 90 % of the stereo targets are displaced; at 300 keypoints 75 %.  n = 0 and n = 1 cannot meet the condition (no
keypoint, and one keypoint that the first accepted query takes): they are the empty and single-lane edges of the kernel.  The one crowd case is RADIUS: Fuse's chi2
gate leaves a window no more than the keypoints within 2.8 sigma of its centre, never more than the stored list holds."""
import numpy as np

from weiner_slamit_v2_amd import synth

M = 200
RADIUS, CHI2 = 1, 2
FIXTURES = {
    (RADIUS, 0, False): (0, 0.9), (RADIUS, 1, False): (2, 0.9), (RADIUS, 63, False): (12, 0.9), (RADIUS, 64, False): (31, 0.9),
    (RADIUS, 65, False): (36, 0.9), (RADIUS, 300, False): (0, 0.75), (RADIUS, 300, True): (0, 0.75),
    (CHI2, 0, False): (0, 0.9), (CHI2, 1, False): (2, 0.9), (CHI2, 63, False): (12, 0.9), (CHI2, 64, False): (5, 0.9),
    (CHI2, 65, False): (28, 0.9), (CHI2, 300, False): (0, 0.75),
}
SIZES = (0, 1, 63, 64, 65, 300)
GATED = [k for k in FIXTURES if k[1] >= 63]   # where the fixture condition can hold


def rule(er_mode, stereo):
    """SearchByProjection's rule for RADIUS, Fuse's (TH_LOW, the 5.99 gate) for CHI2: keyword arguments of api.ORBmatcher.guided_search,
    oracle.bindings.guided_search and search_stereo_ref.guided_search alike."""
    if er_mode == CHI2:
        return dict(th_dist=50, use_ratio=False, nnratio=0.6, chi2_gate=5.99, inv_level_sigma2=stereo["inv_level_sigma2"])
    return dict(th_dist=100, use_ratio=True, nnratio=0.8)


_cache = {}


def fixture(er_mode, n, crowd=False):
    """(frame, queries, stereo): built once per key and shared; nobody changes it."""
    key = (er_mode, n, crowd)
    if key not in _cache:
        seed, frac = FIXTURES[key]
        # the crowd's windows (th = 8: up to 115 px over a 60 x 60 px patch) hold more candidates than the batch form stores
        _cache[key] = synth.synth_search_stereo(n, M, seed, er_mode=er_mode, displaced_frac=frac, crowd=crowd, th=8.0 if crowd else 3.0)
    return _cache[key]


def model_kw(stereo):
    """the stereo dict as search_stereo_ref.guided_search's keyword arguments"""
    return dict(er_mode=stereo["er_mode"], kp_ur=stereo["kp_ur"], q_ur=stereo["q_ur"], q_ur_stride=stereo["q_ur_stride"],
                chi2_gate_stereo=stereo["chi2_gate_stereo"])


def api_stereo(stereo):
    """the stereo dict as api.ORBmatcher.guided_search's `stereo` argument"""
    return {k: stereo[k] for k in ("er_mode", "kp_ur", "q_ur", "q_ur_stride", "chi2_gate_stereo")}


# ---- hand-made one-query cases: (name, frame, queries, rule keywords, stereo, the keypoint the query must take or -1) ----------

def _frame(xy, ur, flips):
    """keypoints at xy, octave 0, descriptor i = the query's (all 0xA5) with flips[i] low bits flipped; 64 x 48 grid over 640 x 480"""
    n = len(xy)
    desc = np.full((n, 32), 0xA5, np.uint8)
    for i, k in enumerate(flips):
        bits = np.unpackbits(desc[i])
        bits[:k] ^= 1
        desc[i] = np.packbits(bits)
    frame = dict(kp_xy=np.asarray(xy, np.float32).reshape(-1, 2), kp_octave=np.zeros(n, np.int32), desc=desc, kp_taken=np.zeros(n, np.uint8),
                 min_x=0.0, min_y=0.0, inv_w=0.1, inv_h=0.1)
    return frame, np.asarray(ur, np.float32)


def _query(u, v, r):
    return dict(uvr=np.array([[u, v, r]], np.float32), level_min=np.zeros(1, np.int32), level_max=np.full(1, -1, np.int32),
                desc=np.full((1, 32), 0xA5, np.uint8), valid=np.ones(1, np.uint8), takes=np.ones(1, np.uint8))


def hand_cases():
    f32 = np.float32
    out = []
    radius = dict(th_dist=100, use_ratio=False, nnratio=0.8)
    fuse = dict(th_dist=50, use_ratio=False, nnratio=0.6, chi2_gate=5.99, inv_level_sigma2=np.ones(8, np.float32))

    def add(name, xy, ur, flips, uvr, rule_kw, er_mode, q_ur, expect):
        frame, kur = _frame(xy, ur, flips)
        st = dict(er_mode=er_mode, kp_ur=kur, q_ur=np.array([q_ur], np.float32), q_ur_stride=1, chi2_gate_stereo=7.8)
        out.append((name, frame, _query(*uvr), rule_kw, st, expect))

    one = [(100.0, 100.0)]
    add("radius: er == r is kept", one, [50.0], [0], (100, 100, 8), radius, RADIUS, 58.0, 0)
    add("radius: er one ulp above r is skipped", one, [50.0], [0], (100, 100, 8), radius, RADIUS, np.nextafter(f32(58.0), f32(np.inf)), -1)
    add("radius: kp_ur == 0 is monocular", one, [0.0], [0], (100, 100, 8), radius, RADIUS, 500.0, 0)
    add("radius: kp_ur just above 0 is stereo", one, [np.nextafter(f32(0), f32(1))], [0], (100, 100, 8), radius, RADIUS, 500.0, -1)
    add("radius: a NaN q_ur is kept", one, [50.0], [0], (100, 100, 8), radius, RADIUS, np.nan, 0)
    add("chi2: kp_ur == 0 is stereo", one, [0.0], [0], (100, 100, 8), fuse, CHI2, 500.0, -1)
    add("chi2: kp_ur == -1 is monocular", one, [-1.0], [0], (100, 100, 8), fuse, CHI2, 500.0, 0)
    # the 7.8 boundary with ex = ey = 0 and sigma2 = 1: the largest float er with er * er <= 7.8f, and the next float
    er = f32(np.sqrt(7.8))
    while f32(er * er) > f32(7.8):
        er = np.nextafter(er, f32(0))
    while f32(np.nextafter(er, f32(9)) ** 2) <= f32(7.8):
        er = np.nextafter(er, f32(9))
    add("chi2: e2 at 7.8 is kept", one, [0.0], [0], (100, 100, 8), fuse, CHI2, er, 0)
    add("chi2: e2 one step above 7.8 is skipped", one, [0.0], [0], (100, 100, 8), fuse, CHI2, np.nextafter(er, f32(9)), -1)
    # a mono (0) and a stereo (1) keypoint in one Fuse window, both 2.5 px from the centre: e2 = 6.25 fails 5.99 and passes 7.8;
    # the mono one is the Hamming-best, so the answer shows which gate each met
    two = [(102.5, 100.0), (97.5, 100.0)]
    add("chi2: mono gated by 5.99, stereo by 7.8 (e2 = 6.25)", two, [-1.0, 40.0], [0, 10], (100, 100, 8), fuse, CHI2, 40.0, 1)
    # both 2.25 px away (e2 = 5.0625 passes 5.99); the stereo one, Hamming-best, adds er = 2: 9.0625 fails 7.8
    two = [(102.25, 100.0), (97.75, 100.0)]
    add("chi2: stereo rejected by its third term, mono kept", two, [-1.0, 40.0], [10, 0], (100, 100, 8), fuse, CHI2, 42.0, 0)
    return out
